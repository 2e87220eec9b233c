"""GPU parity of the prior-time model (PriorBNNmodel / get_grouping) against reference goldens."""
import numpy as np
import pytest
import torch

from golden_util import O, assert_close_mostly, cfg_of, check, load, prior_inputs, regen_noise, stats_of, t

pytestmark = pytest.mark.gpu

from recombiner_amd import prior_model as PM  # noqa: E402

DEV = "cuda"
CASES = ["cifar", "protein", "patch2d", "patch1d", "patch3d"]


def build(d):
    cfg = cfg_of(d)
    n = int(d["n"])
    m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["data_dim"],
                         cfg["pixel_sizes"], cfg["upsample_factors"], cfg["latent_dim"], cfg["patch"],
                         cfg["patch_nums"], cfg["hierarchical_patch_nums"], random_seed=42, device=DEV)
    torch.manual_seed(123)
    lt = PM.LinearTransform(m.dims).to(DEV)
    torch.manual_seed(124)
    up = PM.Upsample(cfg["data_dim"], cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
    return cfg, n, m, lt, up


def feed(m, eps_list):
    q = [e.clone() for e in eps_list]
    m.noise_source = lambda shape: q.pop(0)
    return q


@pytest.mark.parametrize("name", CASES)
def test_init_forward_kl(name):
    d = load(f"prior_{name}.npz")
    cfg, n, m, lt, up = build(d)
    # A1 / A2 / A3 init parity (CPU generator draws, identical order)
    assert np.array_equal(m.loc.detach().cpu().numpy(), d["init_loc"])
    assert np.array_equal(m.lpe_loc.detach().cpu().numpy(), d["init_lpe_loc"])
    if cfg["patch"]:
        assert np.array_equal(m.h_loc.detach().cpu().numpy(), d["init_h_loc"])
        assert np.array_equal(m.hh_loc.detach().cpu().numpy(), d["init_hh_loc"])
    np.testing.assert_allclose(stats_of([a.cpu() for a in lt.A]), d["A_stats"], rtol=1e-12)
    np.testing.assert_allclose(stats_of([p.cpu() for p in up.parameters()]), d["up_stats"], rtol=1e-12)
    _, geo, _, p, A, upo, X, Y, pri = prior_inputs(d)
    with torch.no_grad():
        for k in ["log_scale", "lpe_log_scale", "h_log_scale", "hh_log_scale"]:
            if k in p:
                getattr(m, k).copy_(p[k].to(DEV))
    feed(m, regen_noise(d, "fwd_eps"))
    with torch.no_grad():
        y = m.forward(X.to(DEV)[None].expand(n, -1, -1), lt, up)
    check(d, "fwd_yhat", y, rtol=2e-4, atol=2e-5)
    prg = [None if q is None else q.to(DEV) for q in pri]
    with torch.no_grad():
        kl = m.calculate_kl(*prg).item()
    np.testing.assert_allclose(kl, float(d["kl"]), rtol=1e-5)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("tm", [True, False])
def test_train_3_steps(name, tm):
    """fused pipeline == reference autograd + Adam after 3 steps (A8), incl. the shared mappings."""
    d = load(f"prior_{name}.npz")
    cfg, n, m, lt, up = build(d)
    _, geo, _, p, A, upo, X, Y, pri = prior_inputs(d)
    with torch.no_grad():
        for k in ["log_scale", "lpe_log_scale", "h_log_scale", "hh_log_scale"]:
            if k in p:
                getattr(m, k).copy_(p[k].to(DEV))
    tag = "tm1" if tm else "tm0"
    feed(m, regen_noise(d, f"{tag}_eps"))
    prg = [None if q is None else q.to(DEV) for q in pri]
    mse, kl, elbo = m.train(3, 2e-4, X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV), *prg, lt, up, 1e-4,
                            training_mappings=tm)
    np.testing.assert_allclose([mse, kl], d[f"{tag}_ret"], rtol=2e-4)
    np.testing.assert_allclose(elbo, d[f"{tag}_elbo"], rtol=2e-4)
    # Adam moves every parameter by ~lr per step whatever the gradient scale: compare absolutely
    for k in ["loc", "log_scale", "lpe_loc", "lpe_log_scale", "h_loc", "h_log_scale", "hh_loc", "hh_log_scale"]:
        if hasattr(m, k):
            check(d, f"{tag}_{k}", getattr(m, k), rtol=1e-4, atol=3e-5)
    assert_close_mostly(lt.A[-1], d[f"{tag}_A3"], rtol=1e-3, atol=3e-5, what="A3")
    assert_close_mostly(up.conv3.weight, d[f"{tag}_conv3_w"], rtol=1e-3, atol=3e-5, what="conv3")


def test_autograd_path_matches_fused_path():
    """forward()/calculate_kl() + torch autograd + torch.optim.Adam == train() (same noise)."""
    d = load("prior_cifar.npz")
    _, geo, _, p, A, upo, X, Y, pri = prior_inputs(d)
    prg = [None if q is None else q.to(DEV) for q in pri]
    res = []
    for mode in ("fused", "autograd"):
        cfg, n, m, lt, up = build(d)
        feed(m, regen_noise(d, "tm1_eps"))
        x = X.to(DEV)[None].expand(n, -1, -1)
        y = Y.to(DEV)
        if mode == "fused":
            m.train(3, 2e-4, x, y, *prg, lt, up, 1e-4, training_mappings=True)
        else:
            opt = torch.optim.Adam(list(m.parameters()) + list(lt.parameters()) + list(up.parameters()), 2e-4)
            for _ in range(3):
                yh = m.forward(x, lt, up)
                loss = torch.mean((yh - y) ** 2) * n + m.calculate_kl(*prg) * 1e-4
                opt.zero_grad()
                loss.backward()
                opt.step()
        res.append([m.loc.detach().clone(), m.log_scale.detach().clone(), m.lpe_loc.detach().clone(),
                    lt.A[0].detach().clone(), up.conv1.weight.detach().clone()])
    for a, b in zip(*res):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=2e-6)


def test_get_grouping_matches_golden():
    d = load("grouping.npz")
    r = PM.get_grouping(t(d, "g_ql").to(DEV), t(d, "g_qs").to(DEV), t(d, "g_pl").to(DEV), t(d, "g_ps").to(DEV))
    names = ["group_idx", "start", "end", "group2param", "param2group", "n_groups", "group_kls", "weights"]
    for k, v in zip(names, r):
        if k in ("group_kls", "weights"):
            np.testing.assert_allclose(np.asarray(v), d[f"g_{k}"], rtol=1e-5)
        else:
            assert np.array_equal(np.asarray(v), d[f"g_{k}"]), k


def test_graph_replay_runs_every_step_and_matches_eager():
    """the captured-graph path executes exactly n_epoch steps and produces the same parameters as eager
    stepping when both consume the same device noise stream."""
    d = load("prior_cifar.npz")
    _, geo, _, p, A, upo, X, Y, pri = prior_inputs(d)
    prg = [None if q is None else q.to(DEV) for q in pri]
    res = []
    for use_graph in (True, False):
        cfg, n, m, lt, up = build(d)
        m.use_graph = use_graph
        torch.manual_seed(99)
        x = X.to(DEV)[None].expand(n, -1, -1)
        mse, kl, elbo = m.train(12, 2e-4, x, Y.to(DEV), *prg, lt, up, 1e-4, training_mappings=True)
        assert len(elbo) == 12 and all(e != 0 for e in elbo)
        res.append((m.loc.detach().clone(), lt.A[1].detach().clone(), np.array(elbo)))
    # RNG streams differ between captured and eager execution, so compare statistics, not bits:
    # every parameter must have moved by about lr * 12 and the ELBO curves must agree closely
    moved = (res[0][0] - res[1][0]).abs().max().item()
    assert moved < 12 * 2e-4 * 2 + 1e-6
    np.testing.assert_allclose(res[0][2], res[1][2], rtol=5e-3)


def test_cached_graph_is_reused_with_new_priors_and_beta():
    """Second train() call on the same data replays the graph captured by the first one; the values that change between
    EM iterations (priors, beta, the noise counter) reach it through device memory.  An exact twin -- a fresh model
    loaded with the state after call 1, capturing its own graph for call 2 -- must give the same result (bf16 mode:
    deterministic kernels, same counter-based noise)."""
    import copy
    d = load("prior_cifar.npz")
    _, geo, _, p, A, upo, X, Y, pri = prior_inputs(d)
    prg = [None if q is None else q.to(DEV) for q in pri]
    prg2 = [None if q is None else (q * 1.3 + 0.001) for q in prg]          # "refit" priors of the next EM iteration
    cfg, n, m, lt, up = build(d)
    m.precision = 1
    x, y = X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV)
    torch.manual_seed(7)
    _, _, e1 = m.train(12, 2e-4, x, y, *prg, lt, up, 1e-4, training_mappings=True)
    assert m._ws is not None and m._ws["graphs"] is not None
    ws = m._ws
    snap = (copy.deepcopy(m.state_dict()), copy.deepcopy(lt.state_dict()), copy.deepcopy(up.state_dict()))
    _, kl2, e2 = m.train(9, 2e-4, x, y, *prg2, lt, up, 3e-2, training_mappings=True)      # fewer steps, new beta
    assert m._ws is ws and len(e2) == 9                                     # same workspace, graph replayed
    assert int(ws["rng_ctr"].item()) == 21 and int(ws["step_t"].item()) == 9
    # the twin
    cfg, n, m2, lt2, up2 = build(d)
    m2.precision = 1
    m2.load_state_dict(snap[0]); lt2.load_state_dict(snap[1]); up2.load_state_dict(snap[2])
    m2._rng_ctr_init = 12
    torch.manual_seed(7)
    _, kl2b, e2b = m2.train(9, 2e-4, x, y, *prg2, lt2, up2, 3e-2, training_mappings=True)
    np.testing.assert_allclose(e2, e2b, rtol=1e-5)
    assert kl2 == pytest.approx(kl2b, rel=1e-6)
    assert float((m.loc - m2.loc).abs().max()) < 1e-6 and float((lt.A[0] - lt2.A[0]).abs().max()) < 1e-6
    # and the new beta / priors really took effect: the KL term dominates the second ELBO curve, not the first
    assert abs(e2[0]) > 10 * abs(e1[-1])


def test_graph_survives_a_checkpoint_that_moves_the_live_mappings():
    """main_prior_training.py:334-338 pickles `linear_transform.cpu()` / `upsample_net.cpu()` and moves them back: that
    re-allocates every parameter storage while id(module) stays equal.  A cached step graph would go on reading and
    Adam-updating the freed storages (the live mappings would silently stop training): the workspace key holds the storage
    addresses, so the next train() call re-captures.  Twin: the same calls with the mappings never moved."""
    import copy
    d = load("prior_cifar.npz")
    _, geo, _, p, A, upo, X, Y, pri = prior_inputs(d)
    prg = [None if q is None else q.to(DEV) for q in pri]
    res = []
    for move in (True, False):
        cfg, n, m, lt, up = build(d)
        m.precision = 1
        x, y = X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV)
        torch.manual_seed(7)
        m.train(8, 1e-3, x, y, *prg, lt, up, 1e-4, training_mappings=True)
        assert m._ws is not None and m._ws["graphs"] is not None
        ws_before = m._ws
        if move:
            keep = [torch.empty(1 << 20, device=DEV) for _ in range(4)]      # occupy the allocator's free blocks ...
            ptrs = [q.data_ptr() for q in list(lt.parameters()) + list(up.parameters())]
            lt.cpu(); up.cpu()
            junk = [torch.full((q.numel(),), 7.0, device=DEV) for q in list(lt.parameters()) + list(up.parameters())]
            lt.to(DEV); up.to(DEV)                                          # ... so the parameters land somewhere else
            assert [q.data_ptr() for q in list(lt.parameters()) + list(up.parameters())] != ptrs
            del keep, junk
        a_mid = lt.A[0].detach().clone()
        m._rng_ctr_init = 8                   # a re-captured workspace continues the noise counter where the old one stood
        m._train_calls -= 1 if move else 0    # ... and derives the same noise seed
        m.train(8, 1e-3, x, y, *prg, lt, up, 1e-4, training_mappings=True)
        assert (m._ws is not ws_before) == move
        assert float((lt.A[0] - a_mid).abs().max()) > 1e-5                  # the LIVE mappings kept training
        res.append((lt.A[0].detach().clone(), up.conv3.weight.detach().clone(), m.loc.detach().clone()))
    for a, b in zip(*res):
        assert float((a - b).abs().max()) < 1e-6


@pytest.mark.parametrize("name,n_data", [("cifar", 32), ("protein", 32), ("kodak", 1), ("audio", 1), ("video", 1)])
def test_every_preset_captures_and_replays_in_the_throughput_mode(name, n_data):
    """production path (no injected noise) of every reference preset in the bf16 mode: the step must capture as a HIP
    graph (no host-side operation may hide in it), replay on the second call, and produce finite, decreasing losses."""
    import warnings
    from recombiner_amd import config, utils
    cfg = config.configs[name]
    n = n_data * (int(np.prod(cfg["patch_nums"])) if cfg["patch"] else 1)
    X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], n, cfg["output_dim"], seed=0)
    m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["data_dim"], cfg["pixel_sizes"],
                         cfg["upsample_factors"], cfg["latent_dim"], cfg["patch"], cfg["patch_nums"],
                         cfg["hierarchical_patch_nums"], random_seed=42, device=DEV)
    m.precision = 1
    torch.manual_seed(1)
    lt = PM.LinearTransform(m.dims).to(DEV)
    up = PM.Upsample(cfg["data_dim"], cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
    D, s0, lat = m._d_net, 0.0211547, list(m.lpe_loc.shape[1:])
    pri = [torch.zeros(D, device=DEV), torch.full((D,), s0, device=DEV), torch.zeros(lat, device=DEV), torch.full(lat, s0, device=DEV)]
    pri += ([torch.zeros(D, device=DEV), torch.full((D,), s0, device=DEV)] * 2) if cfg["patch"] else [None] * 4
    Xd, Yd = X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # a failed capture warns and falls back: not acceptable here
        _, _, e1 = m.train(6, 1e-3, Xd, Yd, *pri, lt, up, 1e-8, training_mappings=True)
        ws = m._ws
        assert ws is not None and ws["graphs"] is not None
        _, _, e2 = m.train(6, 1e-3, Xd, Yd, *pri, lt, up, 1e-8, training_mappings=True)
    assert m._ws is ws and len(e1) == len(e2) == 6
    assert np.isfinite(e1).all() and np.isfinite(e2).all()
    assert np.mean(e2) > np.mean(e1)                          # ELBO = -(loss): the second call continues to improve


def test_removed_stream_fork_bits_are_refused_and_a_remaining_one_replays():
    """`stream_forks` takes combinations of the bits 2, 4 and 8 only: a removed ordering (32) is a ValueError before anything
    is built or captured, and a single remaining bit (2) trains as a replayed graph."""
    from recombiner_amd import config, utils
    cfg, n = config.configs["cifar"], 8
    X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], n, cfg["output_dim"], seed=0)
    m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["data_dim"], cfg["pixel_sizes"],
                         cfg["upsample_factors"], cfg["latent_dim"], cfg["patch"], cfg["patch_nums"],
                         cfg["hierarchical_patch_nums"], random_seed=42, device=DEV)
    m.precision = 1
    torch.manual_seed(1)
    lt = PM.LinearTransform(m.dims).to(DEV)
    up = PM.Upsample(cfg["data_dim"], cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
    D, s0, lat = m._d_net, 0.0211547, list(m.lpe_loc.shape[1:])
    pri = [torch.zeros(D, device=DEV), torch.full((D,), s0, device=DEV), torch.zeros(lat, device=DEV), torch.full(lat, s0, device=DEV)]
    pri += [None] * 4
    Xd, Yd = X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV)
    m.stream_forks = 32
    with pytest.raises(ValueError, match="2.*4.*8.*DESIGN.md"):
        m.train(12, 1e-3, Xd, Yd, *pri, lt, up, 1e-8, training_mappings=True)
    assert m._ws is None
    m.stream_forks = 2
    _, _, elbo = m.train(12, 1e-3, Xd, Yd, *pri, lt, up, 1e-8, training_mappings=True)
    assert m._ws is not None and m._ws["graphs"] is not None and m._ws["graphs"][0] == "one"
    assert len(elbo) == 12 and np.isfinite(elbo).all()


@pytest.mark.parametrize("name,width,prec", [("patch2d", 48, 1), ("patch3d", 64, 2), ("patch1d", 64, 1), ("cifar", 64, 1),
                                             ("cifar", 48, 2)])
def test_wide_siren_variants_train_like_the_oracle(name, width, prec):
    """BASELINE.json's throughput variants (Kodak patches at width 48, 3-D video at width 64 in f16, ...): the golden
    cases' geometry with wider hidden layers, two training steps incl. the shared mappings on the oracle's own noise;
    ELBO / MSE / KL within 16-bit operand rounding of the fp32 CPU oracle, parameters within Adam's step size."""
    d = load(f"prior_{name}.npz")
    cfg = dict(cfg_of(d))
    cfg["hidden_dims"] = [width] * 3
    n = int(d["n"])
    geo = O.Geometry.from_config(cfg)
    p = O.init_prior_params(geo, n, seed=42)
    A = O.make_linear_transform(geo.dims, seed=123)
    upo = O.UpsampleNet(geo.data_dim, geo.paddings, geo.layerwise_scale_factors, seed=124)
    X = O.fourier_features(cfg["pixel_sizes"], cfg["fourier_dim"])
    torch.manual_seed(5)
    Y = torch.rand(n, X.shape[0], cfg["output_dim"])
    s0 = 0.0211547
    pri = [torch.zeros_like(p["loc"][0]), torch.full_like(p["loc"][0], s0),
           torch.zeros_like(p["lpe_loc"][0]), torch.full_like(p["lpe_loc"][0], s0)]
    pri += ([torch.zeros_like(p["loc"][0]), torch.full_like(p["loc"][0], s0)] * 2) if cfg["patch"] else [None] * 4
    m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["data_dim"], cfg["pixel_sizes"],
                         cfg["upsample_factors"], cfg["latent_dim"], cfg["patch"], cfg["patch_nums"],
                         cfg["hierarchical_patch_nums"], random_seed=42, device=DEV)
    m.precision = prec
    torch.manual_seed(123)
    lt = PM.LinearTransform(m.dims).to(DEV)
    torch.manual_seed(124)
    up = PM.Upsample(cfg["data_dim"], cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
    np.testing.assert_array_equal(m.loc.detach().cpu().numpy(), p["loc"].numpy())      # same init draws (A1)
    torch.manual_seed(77)
    noise = O.Noise()
    mse_o, kl_o, elbo_o = O.prior_train(geo, p, X[None].repeat(n, 1, 1), Y, pri, A, upo, 2, 2e-4, 1e-4, True, noise)
    feed(m, noise.drawn)
    prg = [None if q is None else q.to(DEV) for q in pri]
    mse, kl, elbo = m.train(2, 2e-4, X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV), *prg, lt, up, 1e-4,
                            training_mappings=True)
    np.testing.assert_allclose([mse, kl], [mse_o, kl_o], rtol=2e-3)
    np.testing.assert_allclose(elbo, elbo_o, rtol=2e-3)
    assert_close_mostly(m.loc, p["loc"].detach(), rtol=0, atol=1.5e-4, max_frac=0.02, hard_atol=8.2e-4, what="loc")
    assert_close_mostly(lt.A[1], A[1].detach(), rtol=0, atol=1.5e-4, max_frac=0.02, hard_atol=8.2e-4, what="A1")


@pytest.mark.parametrize("case,prec", [("wide_patch2d_w48", 1), ("wide_patch3d_w64", 2), ("wide_cifar_w64", 1),
                                       ("wide_patch2d_w48", 0), ("wide_patch3d_w64", 0), ("wide_cifar_w64", 0)])
def test_wide_variants_against_reference_goldens(case, prec):
    """the same variants against vectors produced by the REFERENCE itself at widths 48 / 64 (oracle/make_golden.py
    --only wide; the CPU suite pins the oracle to them exactly): 16-bit HIP path within operand rounding, and the fp32
    parity mode (siren_mlp_generic.hip: any hidden width up to 64) at the tolerances of the width-32 golden tests."""
    d = load(case + ".npz")
    cfg, n, m, lt, up = build(d)
    m.precision = prec
    _, geo, _, p, A, upo, X, Y, pri = prior_inputs(d)
    feed(m, regen_noise(d, "tm1_eps"))
    prg = [None if q is None else q.to(DEV) for q in pri]
    mse, kl, elbo = m.train(2, 2e-4, X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV), *prg, lt, up, 1e-4, training_mappings=True)
    np.testing.assert_allclose([mse, kl], d["tm1_ret"], rtol=2e-3 if prec else 2e-4)
    np.testing.assert_allclose(elbo, d["tm1_elbo"], rtol=2e-3 if prec else 2e-4)
    got = m.loc.detach().cpu().numpy().reshape(-1)
    if "tm1_loc" in d.files:
        sub = d["tm1_loc"].reshape(-1)
    else:                                   # large entries are kept as a strided subsample (+ moments)
        sub, got = d["tm1_loc__sub"], got[::int(d["tm1_loc__stride"])]
    diff = np.abs(got - sub)
    if prec:
        assert (diff > 1.5e-4).mean() < 0.02 and diff.max() < 8.2e-4          # Adam moves every element by <= lr per step
        assert_close_mostly(lt.A[-1], d["tm1_A3"], rtol=0, atol=1.5e-4, max_frac=0.02, hard_atol=8.2e-4, what="A3")
    else:                                   # fp32 mode: as test_train_3_steps
        assert (diff > 3e-5 + 1e-4 * np.abs(sub)).mean() < 0.002, float(diff.max())
        assert_close_mostly(lt.A[-1], d["tm1_A3"], rtol=1e-3, atol=3e-5, what="A3")


def test_sharded_training_rehearsal_two_ranks_one_gpu():
    """world_size 2 over gloo with both ranks on this GPU: mappings stay identical across ranks, and the segmented-graph
    replay (asynchronous all-reduce between captured segments) reproduces eager stepping.  (The RCCL path itself needs
    as many GPUs as ranks; the driver runs it.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RCB_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29541", os.path.join(root, "tools", "dist_rehearsal.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "REHEARSAL OK ws=2" in out.stdout
    # and the shards train exactly like one process holding all INRs (same parameters, data and injected noise)
    assert "SHARDED == UNSHARDED OK ws=2" in out.stdout


def test_hidden_layers_of_different_widths_fp32():
    """PriorBNNmodel with hidden_dims = [24, 40, 16] (the reference accepts any list, prior_model.py:84-85): two training steps
    in the fp32 parity mode, mappings trained, against the CPU oracle on the same injected noise"""
    from recombiner_amd import config, utils
    cfg = dict(config.configs["cifar"])
    cfg["hidden_dims"] = [24, 40, 16]
    n = 3
    geo = O.Geometry.from_config(cfg)
    X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], n, cfg["output_dim"], seed=0)
    m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["data_dim"], cfg["pixel_sizes"],
                         cfg["upsample_factors"], cfg["latent_dim"], cfg["patch"], cfg["patch_nums"],
                         cfg["hierarchical_patch_nums"], random_seed=42, device=DEV)
    assert m._d_net == geo.d_net == 24 * 33 + 40 * 25 + 16 * 41 + 3 * 17
    torch.manual_seed(123)
    lt = PM.LinearTransform(m.dims).to(DEV)
    torch.manual_seed(124)
    up = PM.Upsample(cfg["data_dim"], cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
    torch.manual_seed(7)
    eps = [torch.randn(n, 1, 512), torch.randn(n, 1, geo.d_net), torch.randn(n, 1, 512), torch.randn(n, 1, geo.d_net)]
    q = [e.clone() for e in eps]
    m.noise_source = lambda shape: q.pop(0)
    s0 = 0.0211547
    pri = [torch.zeros(geo.d_net), torch.full((geo.d_net,), s0), torch.zeros(2, 2, 128), torch.full((2, 2, 128), s0)]
    prg = [p.to(DEV) for p in pri] + [None] * 4
    mse, kl, elbo = m.train(2, 2e-4, X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV), *prg, lt, up, 1e-8, training_mappings=True)
    p = O.init_prior_params(geo, n, seed=42)
    A = O.make_linear_transform(geo.dims, seed=123)
    upo = O.UpsampleNet(geo.data_dim, geo.paddings, geo.layerwise_scale_factors, seed=124)
    replay = [eps[0].reshape(n, 2, 2, 128), eps[1], eps[2].reshape(n, 2, 2, 128), eps[3]]
    mse_o, kl_o, elbo_o = O.prior_train(geo, p, X[None].repeat(n, 1, 1), Y, pri + [None] * 4, A, upo, 2, 2e-4, 1e-8, True,
                                        O.Noise(replay))
    np.testing.assert_allclose(elbo, elbo_o, rtol=2e-4)
    np.testing.assert_allclose(m.loc.detach().cpu().numpy(), p["loc"].numpy(), rtol=1e-4, atol=3e-5)
    np.testing.assert_allclose(lt.A[1].detach().cpu().numpy(), A[1].numpy(), rtol=1e-3, atol=3e-5)


def test_bench_plain_run_reports_the_headline_only():
    """A plain `python bench.py` run sets up, warms up, times the steps and prints the result line, nothing more: no live
    roofline of the SIREN kernel and no full report on stderr (those, the CPU baseline and the untimed extras come with
    --full)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RCB_DIST_BACKEND")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--inrs", "64"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["unit"] == "INRs trained/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16" and rec["steps"] == 3
    assert rec["value"] == pytest.approx(64 / (rec["ms_per_step"] * 1e-3) / (200 + 549 * 100))
    assert rec["roofline"] is None and "comm" not in rec
    assert not any(ln.startswith("{") for ln in out.stderr.splitlines()), out.stderr[-2000:]


def test_bench_gpus_flag_launches_ranks():
    """`python bench.py --gpus 2` (no launcher) must start two ranks itself and report n_gpus = 2 -- here over gloo with
    both ranks on the one GPU of the box (the rehearsal switch) -- and must refuse the RCCL form on a one-GPU box."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RCB_DIST_BACKEND")}
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "1", "--inrs", "64",
           "--full", "--no-cpu-baseline", "--no-extras"]
    if torch.cuda.device_count() < 2:
        out = subprocess.run(cmd, env=base, capture_output=True, text=True, timeout=600)
        assert out.returncode != 0 and "--gpus 2 requested" in out.stderr
    out = subprocess.run(cmd, env=dict(base, RCB_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["n_gpus"] == 2 and rec["config"]["inrs_per_gpu"] == 64 and rec["value"] > 0
    # the sharded step's communication report (--full): both buckets, every segment, mappings identical on both ranks
    comm = rec["comm"]
    assert comm["mappings_identical_across_ranks"] is True and comm["backend"] == "gloo"
    assert comm["allreduce_bytes_per_step"] == 4 * (3 * 1056 * 1056 + 99 * 99 + 251024) and len(comm["segment_ms"]) == 4


def test_bench_two_ranks_over_rccl():
    """N > 1 readiness: with two GPUs visible, `python bench.py --gpus 2` runs the sharded step over RCCL (backend nccl on
    ROCm) -- two ranks, one per GPU, mappings bit-identical across the ranks after training.  Skipped on one-GPU boxes (the
    gloo rehearsal above covers the code path there)."""
    import json
    import os
    import subprocess
    import sys
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RCB_DIST_BACKEND")}
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "2", "--inrs", "512",
           "--full", "--no-cpu-baseline", "--no-extras"]
    out = subprocess.run(cmd, env=dict(base, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["n_gpus"] == 2 and rec["value"] > 0
    assert rec["comm"]["backend"] == "nccl" and rec["comm"]["mappings_identical_across_ranks"] is True
    # the launcher probed the captured form on the same two ranks first; whichever form that selected is the one that ran
    choice = rec["comm"]["step_form_choice"]
    assert choice.startswith(("collectives captured", "four segments")), choice
    if choice.startswith("collectives captured"):
        assert rec["comm"]["step_form"].startswith("one captured graph"), rec["comm"]


@pytest.mark.parametrize("n", [1, 3, 5, 258])
def test_odd_batch_sizes_in_the_throughput_mode(n):
    """batch sizes that are no multiple of the kernels' pass sizes (4 INRs per stage-2 pass, 4-element groups of the flat
    posterior / reparam paths, 256 persistent workgroups): the bf16 step must capture, replay and agree with the fp32
    parity mode on the same injected noise to 16-bit operand rounding."""
    from recombiner_amd import config, utils
    cfg = config.configs["cifar"]
    X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], n, 3, seed=3)
    res = {}
    for prec in (0, 1):
        m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["data_dim"], cfg["pixel_sizes"],
                             cfg["upsample_factors"], cfg["latent_dim"], False, None, None, random_seed=42, device=DEV)
        m.precision = prec
        torch.manual_seed(123)
        lt = PM.LinearTransform(m.dims).to(DEV)
        torch.manual_seed(124)
        up = PM.Upsample(2, cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
        gen = torch.Generator(device=DEV).manual_seed(9)
        m.noise_source = lambda shape: torch.randn(shape, device=DEV, generator=gen)
        D, s0 = m._d_net, 0.0211547
        pri = [torch.zeros(D, device=DEV), torch.full((D,), s0, device=DEV), torch.zeros(2, 2, 128, device=DEV),
               torch.full((2, 2, 128), s0, device=DEV)] + [None] * 4
        _, _, elbo = m.train(8, 2e-4, X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV), *pri, lt, up, 1e-8, training_mappings=True)
        res[prec] = np.array(elbo)
    assert np.isfinite(res[1]).all() and len(res[1]) == 8
    np.testing.assert_allclose(res[1], res[0], rtol=2e-3)
    # and the production path (in-kernel noise) at this size
    m.noise_source = None
    _, _, e2 = m.train(8, 2e-4, X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV), *pri, lt, up, 1e-8, training_mappings=True)
    assert np.isfinite(e2).all()


def test_fused_next_sample_equals_separate_sampling_kernels():
    """PriorBNNmodel.fuse_next_sample: drawing step t + 1's sample inside step t's posterior update gives bitwise the same
    training as the per-step sampling kernels (same Philox counters, same arithmetic), eager and replayed."""
    from recombiner_amd import config, utils
    cfg = config.configs["cifar"]
    n = 8
    X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], n, 3, seed=2)
    Xd, Yd = X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV)      # kept alive: the workspace (noise counter, seed) is keyed on them
    outs = []
    for fuse in (True, False):
        torch.manual_seed(77)                      # (the in-kernel noise seed takes torch.initial_seed() in)
        m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["data_dim"], cfg["pixel_sizes"],
                             cfg["upsample_factors"], cfg["latent_dim"], False, None, None, random_seed=42, device=DEV)
        m.precision = 1
        m.fuse_next_sample = fuse
        torch.manual_seed(123)
        lt = PM.LinearTransform(m.dims).to(DEV)
        torch.manual_seed(124)
        up = PM.Upsample(2, cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
        D, s0 = m._d_net, 0.0211547
        pri = [torch.zeros(D, device=DEV), torch.full((D,), s0, device=DEV), torch.zeros(2, 2, 128, device=DEV),
               torch.full((2, 2, 128), s0, device=DEV)] + [None] * 4
        elbos = []
        for n_steps in (2, 7):                     # an eager call, then a call long enough to capture and replay
            elbos += m.train(n_steps, 2e-4, Xd, Yd, *pri, lt, up, 1e-8, training_mappings=True)[2]
        outs.append([torch.tensor(elbos), m.loc.detach().clone(), m.lpe_loc.detach().clone(), m.log_scale.detach().clone()] +
                    [p.detach().clone() for p in lt.parameters()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["audio", "kodak"])
def test_fused_next_lpe_sample_of_the_three_level_presets(name):
    """Patch presets: the latent weights are three levels (stored noise), the lpe -- two thirds of what a step samples -- is one
    plain level whose noise is drawn in the kernels; with fuse_next_sample its next sample comes out of its posterior update.
    Bitwise the same training as with the per-step sampling kernel, eager and replayed."""
    from recombiner_amd import config, utils
    cfg = config.configs[name]
    n = int(np.prod(cfg["patch_nums"]))
    X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], n, cfg["output_dim"], seed=2)
    Xd, Yd = X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV)
    outs = []
    for fuse in (True, False):
        torch.manual_seed(77)
        m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["data_dim"], cfg["pixel_sizes"],
                             cfg["upsample_factors"], cfg["latent_dim"], cfg["patch"], cfg["patch_nums"],
                             cfg["hierarchical_patch_nums"], random_seed=42, device=DEV)
        m.precision = 1
        m.fuse_next_sample = fuse
        torch.manual_seed(123)
        lt = PM.LinearTransform(m.dims).to(DEV)
        torch.manual_seed(124)
        up = PM.Upsample(cfg["data_dim"], cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
        D, s0, lat = m._d_net, 0.0211547, list(m.lpe_loc.shape[1:])
        pri = [torch.zeros(D, device=DEV), torch.full((D,), s0, device=DEV), torch.zeros(lat, device=DEV), torch.full(lat, s0, device=DEV)]
        pri += [torch.zeros(D, device=DEV), torch.full((D,), s0, device=DEV)] * 2
        elbos = []
        torch.manual_seed(5)                       # the weights' stored noise comes from torch's generator
        for n_steps in (2, 7):
            elbos += m.train(n_steps, 2e-4, Xd, Yd, *pri, lt, up, 1e-8, training_mappings=True)[2]
        assert ("smp_lpe" in m._ws) == fuse and "smp_net" not in m._ws
        outs.append([torch.tensor(elbos), m.loc.detach().clone(), m.h_loc.detach().clone(), m.lpe_loc.detach().clone(),
                     m.lpe_log_scale.detach().clone()] + [p.detach().clone() for p in lt.parameters()])
    assert np.isfinite(outs[0][0].numpy()).all()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["patch1d", "patch2d", "patch3d", "cifar"])
def test_map_hierarchical_model_to_int_weights_against_the_reference_function(name):
    """A5 as a callable with the reference's signature (utils.py:122-137): outputs of the reference function itself
    (tests/golden/hier_map.npz) on the same noise stream.  The kernel performs the reference's operations in its order
    (mul, add per level; levels summed left to right), un-fused: bit-identical.  Gradients against the fp64 adjoint."""
    import json
    from recombiner_amd import utils as U
    d = load("hier_map.npz")
    cfg = json.loads(str(d[f"{name}_cfg"]))
    args = [torch.from_numpy(d[f"{name}_{k}"]).to(DEV) for k in ("loc", "scale", "h_loc", "h_scale", "hh_loc", "hh_scale")]
    N, D = args[0].shape
    for S in (1, 3):
        torch.manual_seed(int(d[f"{name}_S{S}_seed"]))
        eps = [torch.randn(N, S, D) for _ in range(3 if cfg["patch"] else 1)]
        q = [e.clone() for e in eps]
        leaf = [a.clone().requires_grad_(True) for a in args]
        out = U.map_hierarchical_model_to_int_weights(bool(cfg["patch"]), *leaf, S, cfg["hierarchical_patch_nums"],
                                                      cfg["patch_nums"], cfg["data_dim"], noise_source=lambda shape: q.pop(0))
        assert tuple(out.shape) == (N, S, D)
        assert np.array_equal(out.detach().cpu().numpy(), d[f"{name}_S{S}_out"]), (name, S)
        # adjoint: d/d(loc_L) = sum of the upstream gradient over samples and member patches, d/d(scale_L) the same of g * eps
        g = torch.randn(N, S, D, dtype=torch.float64)
        out.backward(g.float().to(DEV))
        geo = O.Geometry.from_config(cfg)
        maps = [torch.arange(N)] + ([m.long() for m in geo.level_maps(N)] if cfg["patch"] else [])
        for lvl, (m, e) in enumerate(zip(maps, eps)):
            rows = args[2 * lvl].shape[0]
            gl = torch.zeros(rows, D, dtype=torch.float64).index_add_(0, m, g.sum(1))
            gs = torch.zeros(rows, D, dtype=torch.float64).index_add_(0, m, (g * e.double()).sum(1))
            np.testing.assert_allclose(leaf[2 * lvl].grad.cpu().double().numpy(), gl.numpy(), rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(leaf[2 * lvl + 1].grad.cpu().double().numpy(), gs.numpy(), rtol=1e-5, atol=1e-5)
        if not cfg["patch"]:
            assert leaf[2].grad is None and leaf[4].grad is None
    # the name is importable where upstream imports it from (prior_model.py:10, test_model.py:12)
    from recombiner_amd import test_model as TM
    assert PM.map_hierarchical_model_to_int_weights is U.map_hierarchical_model_to_int_weights is TM.map_hierarchical_model_to_int_weights


@pytest.mark.parametrize("prec", [0, 1])
def test_two_hidden_layers_of_width_32_at_model_level(prec):
    """BASELINE configs[0] read literally: a "2-layer width-32 SIREN" (hidden_dims = [32, 32]) on the CIFAR geometry, 16 INRs.
    The reference builds its INR from whatever list it is given (prior_model.py:84-85); three Adam steps of the whole model
    incl. the mappings against the oracle on the same noise -- fp32 parity mode at fp32 tolerance, bf16 mode within operand
    rounding."""
    from recombiner_amd import config, utils
    cfg = dict(config.configs["cifar"], hidden_dims=[32, 32])
    n = 16
    geo = O.Geometry.from_config(cfg)
    X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], n, cfg["output_dim"], seed=0)
    m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["data_dim"], cfg["pixel_sizes"],
                         cfg["upsample_factors"], cfg["latent_dim"], cfg["patch"], cfg["patch_nums"],
                         cfg["hierarchical_patch_nums"], random_seed=42, device=DEV)
    m.precision = prec
    assert m._d_net == geo.d_net == 32 * 33 + 32 * 33 + 3 * 33
    torch.manual_seed(123)
    lt = PM.LinearTransform(m.dims).to(DEV)
    torch.manual_seed(124)
    up = PM.Upsample(cfg["data_dim"], cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
    steps = 3
    torch.manual_seed(7)
    eps = []
    for _ in range(steps):
        eps += [torch.randn(n, 1, 512), torch.randn(n, 1, geo.d_net)]
    feed(m, eps)
    s0 = 0.0211547
    pri = [torch.zeros(geo.d_net), torch.full((geo.d_net,), s0), torch.zeros(2, 2, 128), torch.full((2, 2, 128), s0)]
    prg = [p.to(DEV) for p in pri] + [None] * 4
    mse, kl, elbo = m.train(steps, 2e-4, X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV), *prg, lt, up, 1e-8, training_mappings=True)
    p = O.init_prior_params(geo, n, seed=42)
    A = O.make_linear_transform(geo.dims, seed=123)
    upo = O.UpsampleNet(geo.data_dim, geo.paddings, geo.layerwise_scale_factors, seed=124)
    replay = []
    for k in range(steps):
        replay += [eps[2 * k].reshape(n, 2, 2, 128), eps[2 * k + 1]]
    mse_o, kl_o, elbo_o = O.prior_train(geo, p, X[None].repeat(n, 1, 1), Y, pri + [None] * 4, A, upo, steps, 2e-4, 1e-8, True,
                                        O.Noise(replay))
    np.testing.assert_allclose(elbo, elbo_o, rtol=2e-4 if prec == 0 else 1e-3)
    if prec == 0:
        assert_close_mostly(m.loc, p["loc"].numpy(), rtol=1e-4, atol=3e-5, what="loc")
    else:      # bf16 operands: the bound of test_wide_siren_variants_train_like_the_oracle (Adam turns rounding-size gradients into full steps)
        assert_close_mostly(m.loc, p["loc"].numpy(), rtol=0, atol=1.5e-4, max_frac=0.02, hard_atol=8.2e-4, what="loc")
    np.testing.assert_allclose(kl, kl_o, rtol=1e-4 if prec == 0 else 2e-3)


def test_redrawn_noise_and_operand_planes_train_like_the_stored_forms():
    """Two round-4 switches of the bf16 training step against the forms they replace, eager and replayed, mappings trained:
    `redraw_noise` (the posterior update re-draws its step's noise from the counter, rcb_level_bwd.eps_from_rng, instead of
    reading the copy the sampler stored) is BITWISE the same training; `operand_planes` (h_w and the SIREN gradient as (hi, lo)
    bf16 planes) gives bitwise the same forward / data-gradient products and the same wide-layer weight gradients -- only the
    99-wide output layer's weight gradient reads float(hi) + float(lo) instead of the fp32 value (2^-17 relative), so the run
    agrees to fp32 rounding, not bit for bit."""
    from recombiner_amd import config, utils
    cfg = config.configs["cifar"]
    n = 8
    X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], n, 3, seed=2)
    Xd, Yd = X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV)
    outs = {}
    for tag, redraw, planes in (("base", False, False), ("redraw", True, False), ("planes", True, True)):
        torch.manual_seed(77)
        m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["data_dim"], cfg["pixel_sizes"],
                             cfg["upsample_factors"], cfg["latent_dim"], False, None, None, random_seed=42, device=DEV)
        m.precision, m.redraw_noise, m.operand_planes = 1, redraw, planes
        torch.manual_seed(123)
        lt = PM.LinearTransform(m.dims).to(DEV)
        torch.manual_seed(124)
        up = PM.Upsample(2, cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
        D, s0 = m._d_net, 0.0211547
        pri = [torch.zeros(D, device=DEV), torch.full((D,), s0, device=DEV), torch.zeros(2, 2, 128, device=DEV),
               torch.full((2, 2, 128), s0, device=DEV)] + [None] * 4
        elbos = []
        for n_steps in (2, 7):
            elbos += m.train(n_steps, 2e-4, Xd, Yd, *pri, lt, up, 1e-8, training_mappings=True)[2]
        outs[tag] = [torch.tensor(elbos), m.loc.detach().clone(), m.lpe_loc.detach().clone(), m.log_scale.detach().clone()] + \
                    [p.detach().clone() for p in lt.parameters()]
    for a, b in zip(outs["base"], outs["redraw"]):
        assert torch.equal(a, b)
    # (measured, tools/debug_planes.py: after four single-step calls every posterior and every wide mapping is still
    # bit-identical and the 99-wide mapping differs by 1.3e-6; over nine steps that difference reaches the other parameters
    # through Adam, which turns rounding-size gradient differences into steps of the order of lr)
    np.testing.assert_allclose(outs["planes"][0].numpy(), outs["base"][0].numpy(), rtol=1e-5)
    for a, b in zip(outs["base"][1:], outs["planes"][1:]):
        assert_close_mostly(b, a.cpu().numpy(), rtol=0, atol=2e-5, max_frac=0.02, hard_atol=2.5 * 2e-4 * 9)
