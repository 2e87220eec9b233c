"""GPU parity of the test-time model (TestBNNmodel: predict / KL / annealing / A* coding / training /
mini end-to-end compression) against reference goldens."""
import numpy as np
import pytest
import torch

from golden_util import DATASET_OF, O, cfg_of, check, level_kwargs, load, regen_noise, regen_noise_per_epoch, t, xy_of

pytestmark = pytest.mark.gpu

from recombiner_amd import prior_model as PM  # noqa: E402
from recombiner_amd import test_model as TM   # noqa: E402

DEV = "cuda"
NAMES = ["cifar", "patch2d", "patch1d", "patch3d"]        # patch3d: the video geometry (data_dim 3, per-column row permutations)


def xdev(d, n):
    return xy_of(d)[0].to(DEV)[None].expand(n, -1, -1)


def ydev(d):
    return xy_of(d)[1].to(DEV)


def build(d, name):
    cfg = cfg_of(d)
    n = int(d["n"])
    torch.manual_seed(123)
    dims = [cfg["input_dim"]] + cfg["hidden_dims"] + [cfg["output_dim"]]
    lt = PM.LinearTransform(dims).to(DEV)
    torch.manual_seed(124)
    up = PM.Upsample(cfg["data_dim"], cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
    kw = {}
    for pre in ([""] + (["h_", "hh_"] if cfg["patch"] else [])):
        k = level_kwargs(d, pre)
        kw.update({pre + a: b for a, b in k.items()})
    m = TM.TestBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["upsample_factors"],
                        cfg["latent_dim"], cfg["data_dim"], cfg["pixel_sizes"], cfg["patch"], cfg["patch_nums"],
                        cfg["hierarchical_patch_nums"], DATASET_OF[name.partition("_w")[0]], linear_transform=lt, upsample_net=up,
                        device=DEV, initial_beta=1e-5, **kw)
    return cfg, n, m


def set_post(d, cfg, m):
    with torch.no_grad():
        m.loc.copy_(t(d, "t_loc").to(DEV))
        m.log_scale.copy_(t(d, "t_log_scale").to(DEV))
        if cfg["patch"]:
            m.h_loc.copy_(t(d, "t_h_loc").to(DEV))
            m.h_log_scale.copy_(t(d, "t_h_log_scale").to(DEV))
            m.hh_loc.copy_(t(d, "t_hh_loc").to(DEV))
            m.hh_log_scale.copy_(t(d, "t_hh_log_scale").to(DEV))


def feed(m, eps):
    q = [e.clone() for e in eps]
    m.noise_source = lambda kind, shape: q.pop(0)


def feed_epochs(m, per_epoch):
    q = [e.clone() for ep in per_epoch for e in ep]
    m.noise_source = lambda kind, shape: q.pop(0)


@pytest.mark.parametrize("name", NAMES)
def test_init_predict_kl_anneal(name):
    d = load(f"test_{name}.npz")
    cfg, n, m = build(d, name)
    np.testing.assert_allclose(m.bpp, float(d["bpp"]), rtol=1e-12)
    if cfg["patch"]:
        assert np.array_equal(m.permute_patch_x_g2p, d["perm_x_g2p"].astype(np.int64))
        assert np.array_equal(m.h_permute_patch_x_g2p, d["h_perm_x_g2p"].astype(np.int64))
    set_post(d, cfg, m)
    X = xdev(d, n)
    for S in (1, 5):
        feed(m, regen_noise(d, f"pred_S{S}_eps"))
        with torch.no_grad():
            yp = m.predict(X, random_seed=None, sample_size=S)
        check(d, f"pred_S{S}", yp, rtol=2e-4, atol=2e-5)
    with torch.no_grad():
        np.testing.assert_allclose(m.calculate_kl().item(), float(d["kl_beta_weighted"]), rtol=2e-5)
    r = m.update_annealing_factors(False)
    arrs = r if cfg["patch"] else (r,)
    for a, k in zip(arrs, ["kls", "h_kls", "hh_kls"]):
        np.testing.assert_allclose(a, d[k], rtol=2e-5, atol=1e-9)
    np.testing.assert_array_equal(m.kl_beta.cpu().numpy(), d["beta_before"])
    m.update_annealing_factors(True)
    got = m.kl_beta.cpu().numpy()
    # decisions sit on fp32 KLs that differ by ulps between CPU and GPU: allow a vanishing fraction of flips
    assert (got != d["beta_after"]).mean() < 2e-3
    if cfg["patch"]:
        assert (m.h_kl_beta.cpu().numpy() != d["h_beta_after"]).mean() < 2e-3
        assert (m.hh_kl_beta.cpu().numpy() != d["hh_beta_after"]).mean() < 2e-3


@pytest.mark.parametrize("name", NAMES)
def test_sample_group_selects_reference_index(name):
    d = load(f"test_{name}.npz")
    cfg, n, m = build(d, name)
    set_post(d, cfg, m)
    for row, grp, idx, margin in d["enc_table"]:
        row, grp = int(row), int(grp)
        i, z, lw = m.sample_group(row, grp, 65536)
        # sigma = softplus(log_scale)/6 is evaluated on the GPU here (<= 1 ulp from the CPU value): the
        # index must agree whenever the reference's top-2 margin is not itself at rounding level
        if margin > 1e-3:
            assert i == int(idx), (row, grp, i, idx, margin)
            np.testing.assert_allclose(z.cpu().numpy(), d[f"enc_{row}_{grp}_z"], rtol=1e-12)
            # (sigma = softplus(log_scale) / 6 is taken on the device: an ulp of sigma is 1.2e-7 of a log-weight of several thousand)
            np.testing.assert_allclose(lw[:256].cpu().numpy(), d[f"enc_{row}_{grp}_lw_head"], rtol=1e-6, atol=1e-3)
    if cfg["patch"]:
        i, z, _ = m.h_sample_group(0, 1, 65536)
        assert i == int(d["h_enc_0_1"][0])
        i, z, _ = m.hh_sample_group(0, 2, 65536)
        assert i == int(d["hh_enc_0_2"][0])
        np.testing.assert_allclose(z.cpu().numpy(), d["hh_enc_0_2_z"], rtol=1e-6)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("path", ["fused", "autograd"])
def test_train_3_epochs(name, path):
    d = load(f"test_{name}.npz")
    cfg, n, m = build(d, name)
    set_post(d, cfg, m)
    X = xdev(d, n)
    Y = ydev(d)
    m.update_annealing_factors(True)          # the golden run did this before training
    feed_epochs(m, regen_noise_per_epoch(d, "train_eps", 3))
    opt = torch.optim.Adam(m.parameters(), lr=2e-4)
    if path == "autograd":
        m._fresh = lambda o: False             # force the generic autograd + optimizer.step() path
    m.train(X, Y, 3, opt, False, sample_size=5)
    check(d, "train_loc", m.loc, rtol=1e-4, atol=3e-5)
    check(d, "train_log_scale", m.log_scale, rtol=1e-4, atol=3e-5)
    assert (np.abs(m.kl_beta.cpu().numpy() - d["train_beta"]) > 1e-6 * d["train_beta"]).mean() < 2e-3
    if cfg["patch"]:
        check(d, "train_h_loc", m.h_loc, rtol=1e-4, atol=3e-5)
        check(d, "train_hh_log_scale", m.hh_log_scale, rtol=1e-4, atol=3e-5)


def test_end_to_end_cifar_first_rounds():
    """optimise 12 epochs, then 6 encode rounds with 2 fine-tune epochs each, with the torch GPU
    generator replaced by the reference's CPU noise stream; compare encoded indices with the
    reference run (golden e2e_cifar.npz)."""
    d = load("test_cifar.npz")
    e = load("e2e_cifar.npz")
    cfg, n, m = build(d, "cifar")
    X = xdev(d, n)
    Y = ydev(d)
    Dt, D = m._l1.D, m._d_net

    def cpu_stream(kind, shape):     # the reference draws on the CPU generator after torch.manual_seed(epoch)
        return torch.randn(shape)
    m.noise_source = cpu_stream
    m.optimize_posteriors(X, Y, n_epochs=12, lr=2e-4, verbose=False)
    check(e, "opt_loc", m.loc, rtol=1e-4, atol=3e-5)
    rounds = 6
    lv = m._l1
    for r in range(rounds):
        m._encode_round(lv, True, r)
        m.train(X, Y, 2, torch.optim.Adam(m.parameters(), lr=2e-4), False)
    done = lv.mask_groupwise
    assert done.sum() == rounds * n
    ref_done = e["idx"] != 0
    same_groups = (done & ref_done).sum() / done.sum()
    agree = (lv.idx_groupwise[done] == e["idx"][done]).mean()
    print("e2e agreement: groups", same_groups, "indices", agree)
    assert agree >= 0.9, agree


def test_end_to_end_patched_first_rounds():
    """3-level hierarchy (audio-like patched preset): optimise 12 epochs, then the first encode rounds of the
    top level (one group per level-3 row per round, 2 fine-tune epochs) against the reference run."""
    d = load("test_patch1d.npz")
    e = load("e2e_patch1d.npz")
    cfg, n, m = build(d, "patch1d")
    X = xdev(d, n)
    Y = ydev(d)
    m.noise_source = lambda kind, shape: torch.randn(shape)       # the reference's CPU stream (seeded per epoch)
    m.optimize_posteriors(X, Y, n_epochs=12, lr=2e-4, verbose=False)
    check(e, "opt_loc", m.loc, rtol=1e-4, atol=3e-5)
    lv = m._l3
    rounds = 4
    for r in range(rounds):
        m._encode_round(lv, True, r)
        m.train(X, Y, 2, torch.optim.Adam(m.parameters(), lr=2e-4), False)
    done = lv.mask_groupwise
    assert done.sum() == rounds * lv.rows
    agree = (lv.idx_groupwise[done] == e["hh_idx"][done]).mean()
    same_groups = (done & (e["hh_idx"] != 0)).sum() / done.sum()
    print("patched e2e: level-3 groups", same_groups, "indices", agree)
    assert agree >= 0.85, agree


def test_graph_replayed_training_tracks_eager_training():
    """captured-graph stepping (one noise stream per call) vs eager stepping (reseeded per epoch): different
    noise, same optimisation -- parameters move the same way and the per-group beta agree."""
    d = load("test_cifar.npz")
    out = []
    for use_graph in (True, False):
        cfg, n, m = build(d, "cifar")
        set_post(d, cfg, m)
        m.use_graph = use_graph
        X = xdev(d, n)
        Y = ydev(d)
        l0 = m.loc.detach().clone()
        m.train(X, Y, 40, torch.optim.Adam(m.parameters(), lr=2e-4), False)
        m.train(X, Y, 12, torch.optim.Adam(m.parameters(), lr=2e-4), False)      # second call re-uses the graphs
        out.append(((m.loc.detach() - l0).cpu().numpy(), m.kl_beta.cpu().numpy().copy()))
        if use_graph:
            assert m._ws is not None and set(m._ws["graphs"].keys()) == {True, False}
    (da, ba), (db, bb) = out
    cos = float((da * db).sum() / np.sqrt((da * da).sum() * (db * db).sum()))
    assert cos > 0.9, cos                       # same direction of travel
    assert abs(np.abs(da).mean() / np.abs(db).mean() - 1) < 0.1
    assert (ba != bb).mean() < 0.05


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("name", ["patch1d", "patch2d"])
def test_bitstream_round_trip_three_levels(name, precision):
    """N4 on a patched preset: encode every group of levels 3, 2, 1 (no fine-tuning), pack, and rebuild the encoded
    samples on a freshly constructed model from the indices alone: bit-identical parameters, same reconstruction
    (precision 1: the decoder runs the bf16 kernels, for patch2d the tiled phase-conv path of the stitched grid)."""
    from recombiner_amd import bitstream
    d = load(f"test_{name}.npz")
    cfg, n, m = build(d, name)
    m.precision = precision
    set_post(d, cfg, m)
    X = xdev(d, n)
    for lv in (m._l3, m._l2, m._l1):
        for r in range(lv.n_groups):
            m._encode_round(lv, True, r)
    blob = bitstream.encode(m)
    n_idx = sum(lv.rows * lv.n_groups for lv in (m._l1, m._l2, m._l3))
    assert bitstream.payload_bits(blob) == 16 * n_idx
    _, _, m2 = build(d, name)
    m2.precision = precision
    levels = bitstream.unpack_indices(blob)
    assert [a.shape for a in levels] == [(lv.rows, lv.n_groups) for lv in (m._l1, m._l2, m._l3)]
    bitstream.apply_indices(m2, levels)
    for a, b in zip((m._l1, m._l2, m._l3), (m2._l1, m2._l2, m2._l3)):
        assert torch.equal(a.sample, b.sample) and bool((b.mask == 1).all())
    with torch.no_grad():
        y1, y2 = m.predict(X), m2.predict(X)
    assert float((y1 - y2).abs().max()) < 1e-5
    m3 = build(d, name)[2]
    with pytest.raises(ValueError):
        bitstream.apply_indices(m3, levels[:1])                # a level missing
    with pytest.raises(ValueError):
        bitstream.encode(m3)                                   # nothing encoded yet


@pytest.mark.parametrize("precision", [0, 1])
def test_end_to_end_cifar_full_compression_matches_reference_psnr(precision):
    """(precision 0 = fp32 parity mode, 1 = the bf16 throughput mode: same rate, PSNR within 0.25 dB.)
    The COMPLETE compression of the reference run (golden e2e_cifar.npz: 12 optimisation epochs, then every one of the
    1511 groups A*-encoded with 2 fine-tune epochs per round, CPU noise stream): same rate by construction (one 16-bit
    index per group and image), PSNR per image within 0.1 dB of the reference's, most A* indices identical, and the
    standalone decoder reproduces the encoder's reconstruction from the bitstream."""
    from recombiner_amd import bitstream
    from recombiner_amd.utils import metric
    d = load("test_cifar.npz")
    e = load("e2e_cifar.npz")
    cfg, n, m = build(d, "cifar")
    m.precision = precision
    X = xdev(d, n)
    Y = ydev(d)
    m.noise_source = lambda kind, shape: torch.randn(shape)        # the reference's CPU stream (reseeded per epoch)
    m.optimize_posteriors(X, Y, n_epochs=12, lr=2e-4, verbose=False)
    dist = m.compress_posteriors(X, Y, n_epochs_finetune=2, h_n_epochs_finetune=2, hh_n_epochs_finetune=2, verbose=False,
                                 lr=2e-4, fine_tune_gap=1)
    lv = m._l1
    assert lv.mask_groupwise.all() and lv.idx_groupwise.shape == e["idx"].shape
    ref = np.asarray(e["distortion"], dtype=np.float64)
    agree = float((lv.idx_groupwise == e["idx"]).mean())
    print("full e2e (precision %d): PSNR ours" % precision, np.round(dist, 3), "reference", np.round(ref, 3),
          "index agreement %.3f" % agree)
    np.testing.assert_allclose(dist, ref, rtol=0, atol=0.1 if precision == 0 else 0.25)          # dB, per image
    assert abs(float(np.mean(dist)) - float(np.mean(ref))) < (0.05 if precision == 0 else 0.15)
    if precision == 0:
        assert agree > 0.5                                           # ties of near-equal candidates flip; most do not
    # rate: one 16-bit index per (image, group) -- identical to the reference's bpp by construction
    blob = bitstream.encode(m)
    assert bitstream.payload_bits(blob) == n * lv.n_groups * 16
    assert m.bpp == pytest.approx(lv.n_groups * 16 / 1024)
    # decoder: bitstream -> parameters -> reconstruction; PSNR of the decoded images == the encoder's report
    _, _, m2 = build(d, "cifar")
    m2.precision = precision
    bitstream.apply_indices(m2, bitstream.unpack_indices(blob))
    assert torch.equal(m2._l1.sample, lv.sample)
    with torch.no_grad():
        y_dec = m2.predict(X)
    # (fp32 parity mode: library kernels that are not bitwise reproducible between calls; one 8-bit rounding flip = 1.4e-3 dB)
    np.testing.assert_allclose(metric(Y.cpu().numpy(), y_dec.cpu().numpy(), "cifar"), dist, rtol=0,
                               atol=5e-3 if precision == 0 else 1e-3)
    # the reference's own final reconstruction, scored the same way, gives the reference's distortion (fixture sanity)
    np.testing.assert_allclose(metric(Y.cpu().numpy(), e["final_pred"], "cifar"), ref, rtol=0, atol=1e-3)


def test_end_to_end_patched_full_compression_matches_reference_psnr():
    """Same for the three-level (audio-like) patched preset: levels 3, 2, 1 encoded in full with 2 fine-tune epochs per
    round (golden e2e_patch1d.npz); distortion within tolerance of the reference's, decoder round trip exact."""
    from recombiner_amd import bitstream
    from recombiner_amd.utils import metric
    d = load("test_patch1d.npz")
    e = load("e2e_patch1d.npz")
    cfg, n, m = build(d, "patch1d")
    X = xdev(d, n)
    Y = ydev(d)
    m.noise_source = lambda kind, shape: torch.randn(shape)
    m.optimize_posteriors(X, Y, n_epochs=12, lr=2e-4, verbose=False)
    dist = np.asarray(m.compress_posteriors(X, Y, n_epochs_finetune=2, h_n_epochs_finetune=2, hh_n_epochs_finetune=2,
                                            verbose=False, lr=2e-4, fine_tune_gap=1), dtype=np.float64)
    ref = np.asarray(e["distortion"], dtype=np.float64)
    agree = [float((lv.idx_groupwise == e[k]).mean()) for lv, k in ((m._l3, "hh_idx"), (m._l2, "h_idx"), (m._l1, "idx"))]
    print("full patched e2e: distortion ours", np.round(dist, 3), "reference", np.round(ref, 3), "index agreement (L3, L2, L1)",
          np.round(agree, 3))
    assert dist.shape == ref.shape
    np.testing.assert_allclose(dist, ref, rtol=0, atol=0.15)
    assert abs(float(dist.mean()) - float(ref.mean())) < 0.08
    assert agree[0] > 0.5
    blob = bitstream.encode(m)
    _, _, m2 = build(d, "patch1d")
    bitstream.apply_indices(m2, bitstream.unpack_indices(blob))
    for a, b in zip((m._l1, m._l2, m._l3), (m2._l1, m2._l2, m2._l3)):
        assert torch.equal(a.sample, b.sample)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision", [0, 1])
def test_test_time_training_captures_graphs_for_every_preset(name, precision):
    """production path of TestBNNmodel.train (no injected noise): both step graphs (with / without the beta update)
    must capture -- a failed capture warns and falls back to eager stepping -- and the loss must stay finite."""
    import warnings
    d = load(f"test_{name}.npz")
    cfg, n, m = build(d, name)
    m.precision = precision
    set_post(d, cfg, m)
    X = xdev(d, n)
    Y = ydev(d)
    loc0 = m.loc.detach().clone()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m.train(X, Y, 40, torch.optim.Adam(m.parameters(), lr=2e-4), False, sample_size=5)
    assert m._ws is not None and set(m._ws["graphs"].keys()) == {True, False} and m.use_graph
    assert torch.isfinite(m.loc).all() and float((m.loc - loc0).abs().max()) > 0
    with torch.no_grad():
        assert torch.isfinite(m.predict(X)).all()


def _train12(m, X, Y):
    """three warm-up steps, the captured plain step, and the captured step with the beta update at epoch 10"""
    m.train(X, Y, 12, torch.optim.Adam(m.parameters(), lr=2e-4), False, sample_size=5)


def _bf16_model(d, name):
    cfg, n, m = build(d, name)
    m.precision = 1
    set_post(d, cfg, m)
    return m, xdev(d, n), ydev(d)


# what changes between two train() calls, one at a time (None: the storage of a level-2 parameter is re-allocated)
KEY_CHANGES = {"cifar": [("pe_bf16", False), ("stage1_bf16", False), ("split_terms", 3), ("beta_step_size", 0.2)],
               "patch1d": [("stitched_pe", False), ("h_loc", None)]}


@pytest.mark.parametrize("name", sorted(KEY_CHANGES))
def test_workspace_key_holds_what_the_captured_step_depends_on(name):
    """an identical second call finds its workspace again; a switch, a beta constant or a storage that the captured step
    depends on, changed before the next call, builds a new one (both graphs captured again) instead of replaying a stale graph"""
    m, X, Y = _bf16_model(load(f"test_{name}.npz"), name)
    _train12(m, X, Y)
    ws = m._ws
    assert ws is not None and set(ws["graphs"].keys()) == {True, False}
    _train12(m, X, Y)
    assert m._ws is ws
    for attr, value in KEY_CHANGES[name]:
        if value is None:
            prm = getattr(m, attr)
            prm.data = prm.data.clone()
        else:
            assert getattr(m, attr) != value
            setattr(m, attr, value)
        _train12(m, X, Y)
        assert m._ws is not ws, attr
        ws = m._ws                      # (the old one stays referenced up to here: `is not` cannot meet a recycled dict)
        assert set(ws["graphs"].keys()) == {True, False} and m.use_graph, attr
        for lv in m._levels:
            assert torch.isfinite(lv.loc).all() and torch.isfinite(lv.log_scale).all() and torch.isfinite(lv.kl_beta).all(), attr


def test_changed_beta_constant_acts_exactly():
    """beta_step_size is a kernel argument of the captured adjusting step: changed between two calls it must act exactly as on
    a model whose workspace was dropped by hand (three warm-up steps, new graphs), and differently from no change at all"""
    d = load("test_cifar.npz")

    def run(between):
        m, X, Y = _bf16_model(d, "cifar")
        _train12(m, X, Y)
        between(m)
        _train12(m, X, Y)
        return [(lv.loc.detach().clone(), lv.log_scale.detach().clone(), lv.kl_beta.clone()) for lv in m._levels]

    def changed(m):
        m.beta_step_size = 0.2

    def changed_and_dropped(m):
        m.beta_step_size = 0.2
        m._ws = None
    a, b, c = run(changed), run(changed_and_dropped), run(lambda m: None)
    for la, lb in zip(a, b):
        for ta, tb in zip(la, lb):
            assert torch.equal(ta, tb)
    assert any(bool((la[2] != lc[2]).any()) for la, lc in zip(a, c))


@pytest.mark.parametrize("width,precision", [(48, 1), (64, 2)])
def test_wide_variant_test_time_training_and_bit_exact_decode(width, precision):
    """BASELINE's width variants on the test-time path (S = 5 samples through the wide SIREN kernel, group-ordered
    parameters, generic posterior kernels where a 64-wide INR no longer fits the LDS-staged ones): the fine-tuning loss
    falls, every group of a few rounds is encoded, and a decoder built from the indices alone reproduces the encoder's
    parameters bit for bit and its reconstruction."""
    from recombiner_amd import bitstream, config, utils
    cfg = dict(config.configs["cifar"])
    cfg["hidden_dims"] = [width] * 3
    N = 6
    X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], N, 3, seed=0)
    dims = [cfg["input_dim"]] + cfg["hidden_dims"] + [cfg["output_dim"]]
    D = sum(dims[i + 1] * (dims[i] + 1) for i in range(4)) + 512
    bits = np.random.RandomState(0).gamma(0.7, 6.0, size=D).astype(np.float32)
    gi, gs, ge, g2p, p2g, G, gk, w = PM.get_grouping_by_kl(bits)

    def make():
        torch.manual_seed(123)
        lt = PM.LinearTransform(dims).to(DEV)
        torch.manual_seed(124)
        up = PM.Upsample(2, cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
        m = TM.TestBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], N, cfg["upsample_factors"],
                            cfg["latent_dim"], 2, cfg["pixel_sizes"], False, None, None, "cifar", linear_transform=lt,
                            upsample_net=up, p_loc=torch.zeros(D)[p2g], p_log_scale=torch.full((D,), -2.0)[p2g],
                            init_log_scale=torch.full((D,), -4.0), param_to_group=p2g, group_to_param=g2p, n_groups=G,
                            group_start_index=gs, group_end_index=ge, group_idx=gi, device=DEV, initial_beta=1e-8)
        m.precision = precision
        return m

    m = make()
    Xd, Yd = X.to(DEV)[None].expand(N, -1, -1), Y.to(DEV)
    with torch.no_grad():
        y0 = m.predict(Xd, random_seed=0, sample_size=1)
    mse0 = float(((y0 - Yd) ** 2).mean())
    m.train(Xd, Yd, 30, torch.optim.Adam(m.parameters(), lr=2e-3), False, sample_size=5)
    with torch.no_grad():
        y1 = m.predict(Xd, random_seed=0, sample_size=1)
    mse1 = float(((y1 - Yd) ** 2).mean())
    assert np.isfinite(mse1) and mse1 < 0.97 * mse0, (mse0, mse1)      # (white-noise targets: slow to fit)
    for r in range(G):
        m._encode_round(m._l1, True, r)
    assert m.compressed_mask_groupwise.all()
    blob = bitstream.encode(m)
    m2 = make()
    bitstream.apply_indices(m2, bitstream.unpack_indices(blob))
    assert torch.equal(m2._l1.sample, m._l1.sample)
    with torch.no_grad():
        ya, yb = m.predict(Xd), m2.predict(Xd)
    assert float((ya - yb).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------------
# BASELINE configs[4]: the 3-D patched (video) geometry at test time -- fp32 parity mode above (NAMES), and here the
# width-64 / f16 variant and the head of a compression run
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [2, 0])
def test_patch3d_width64_f16_test_time_path(precision):
    """TestBNNmodel at data_dim 3, hidden width 64, f16 operands (precision 2), against vectors of the REFERENCE classes run
    with hidden_dims = [64] * 3 (test_patch3d_w64.npz): constructor state exact; predict, KL, annealing and three
    training epochs within 16-bit operand rounding; A* indices exact (scoring never leaves fp64).  precision 0: the same in
    the fp32 parity mode (fp32 SIREN at width 64: siren_mlp_generic.hip) at fp32 tolerances."""
    name = "patch3d_w64"
    d = load(f"test_{name}.npz")
    cfg, n, m = build(d, name)
    assert cfg["hidden_dims"] == [64, 64, 64] and cfg["data_dim"] == 3
    m.precision = precision
    np.testing.assert_allclose(m.bpp, float(d["bpp"]), rtol=1e-12)
    assert np.array_equal(m.permute_patch_x_g2p, d["perm_x_g2p"].astype(np.int64))
    assert np.array_equal(m.h_permute_patch_x_g2p, d["h_perm_x_g2p"].astype(np.int64))
    set_post(d, cfg, m)
    X, Y = xdev(d, n), ydev(d)
    for S in (1, 5):
        feed(m, regen_noise(d, f"pred_S{S}_eps"))
        with torch.no_grad():
            yp = m.predict(X, random_seed=None, sample_size=S)
        if precision:
            check(d, f"pred_S{S}", yp, rtol=2e-2, atol=4e-3)             # f16 operands, fp32 accumulation
        else:
            check(d, f"pred_S{S}", yp, rtol=2e-4, atol=2e-5)
    r = m.update_annealing_factors(False)
    for a, k in zip(r, ["kls", "h_kls", "hh_kls"]):
        np.testing.assert_allclose(a, d[k], rtol=2e-5, atol=1e-9)       # KL is fp32 / fp64 in every mode
    for row, grp, idx, margin in d["enc_table"]:
        i, z, lw = m.sample_group(int(row), int(grp), 65536)
        if margin > 1e-3:
            assert i == int(idx)
    assert m.h_sample_group(0, 1, 65536)[0] == int(d["h_enc_0_1"][0])
    assert m.hh_sample_group(0, 2, 65536)[0] == int(d["hh_enc_0_2"][0])
    m.update_annealing_factors(True)
    feed_epochs(m, regen_noise_per_epoch(d, "train_eps", 3))
    m.train(X, Y, 3, torch.optim.Adam(m.parameters(), lr=2e-4), False, sample_size=5)
    # three Adam steps of lr 2e-4 move every element by <= 6e-4; with 16-bit operands the normalised step of an element
    # whose gradient is near zero may differ in sign
    for key, prm in (("train_loc", m.loc), ("train_h_loc", m.h_loc), ("train_hh_loc", m.hh_loc)):
        got = prm.detach().cpu().numpy().reshape(-1)
        if key in d.files:
            exp = d[key].reshape(-1)
        else:
            exp, got = d[key + "__sub"], got[::int(d[key + "__stride"])]
        diff = np.abs(got - exp)
        if precision:
            assert (diff > 1.5e-4).mean() < 0.03 and diff.max() < 1.25e-3, (key, float((diff > 1.5e-4).mean()), float(diff.max()))
        else:
            assert (diff > 3e-5 + 1e-4 * np.abs(exp)).mean() < 0.002, (key, float(diff.max()))


@pytest.mark.parametrize("precision", [0, 1])
def test_end_to_end_patch3d_first_rounds(precision):
    """head of a compression run on the 3-D patched geometry (golden e2e_patch3d.npz, produced by the reference's own
    methods in the order of compress_posteriors' loop body): 12 optimisation epochs, then three encode rounds of the top
    level with two fine-tune epochs each, on the reference's CPU noise stream."""
    d = load("test_patch3d.npz")
    e = load("e2e_patch3d.npz")
    cfg, n, m = build(d, "patch3d")
    m.precision = precision
    X, Y = xdev(d, n), ydev(d)
    m.noise_source = lambda kind, shape: torch.randn(shape)
    m.optimize_posteriors(X, Y, n_epochs=12, lr=2e-4, verbose=False)
    if precision == 0:
        check(e, "opt_loc", m.loc, rtol=1e-4, atol=3e-5)
        check(e, "opt_hh_loc", m.hh_loc, rtol=1e-4, atol=3e-5)
    lv = m._l3
    for r in range(3):
        m._encode_round(lv, True, r)
        m.train(X, Y, 2, torch.optim.Adam(m.parameters(), lr=2e-4), False)
    ref = e["hh_rounds"]                                   # (row, group, index) in encode order
    idx = lv.idx_groupwise
    done = lv.mask_groupwise
    assert done.sum() == 3 * lv.rows
    hits = sum(bool(done[int(r), int(g)]) and idx[int(r), int(g)] == i for r, g, i in ref)
    print("patch3d e2e head (precision %d): %d of %d (row, group, index) triples equal the reference's" % (precision, hits, len(ref)))
    assert hits >= (len(ref) - 1 if precision == 0 else len(ref) // 2)
    if precision == 0:
        # 12 + 6 Adam steps of lr 2e-4: an element whose gradient is ~0 may take a step in the other direction
        from golden_util import assert_close_mostly
        assert_close_mostly(m.hh_loc, e["hh_loc_after"], rtol=1e-3, atol=5e-5, max_frac=2e-3, hard_atol=8e-4, what="hh_loc_after")


def test_rec_long_groups_against_reference_golden():
    """groups of 338 / 360 parameters (and one of 6) scored by the REFERENCE's sample_group (rec_long_groups.npz): the
    exact scorer and the certified fast scorer both return the reference's index and sample; log-weights within the
    fp32-log shift (see test_rec_long_groups_against_oracle)."""
    from recombiner_amd import ops
    d = load("rec_long_groups.npz")
    K = 65536
    gum = torch.from_numpy(O.gumbel_table(42)).to(DEV)
    enc = d["enc_table"]
    lens = sorted(set(int(v) for v in enc[:, 4]))
    tabs = ops.RecTables.from_dict({gl: O.sobol_normal_table(gl) for gl in lens}, DEV, K)
    D = int(d["p_loc"].shape[0])
    loc = torch.zeros(3, D)
    ls = torch.zeros(3, D)
    rows, starts, glens = [], [], []
    for row, grp, idx, margin, gl in enc:
        row, grp, gl = int(row), int(grp), int(gl)
        s0 = int(d["start"][grp])
        loc[row, s0:s0 + gl] = torch.from_numpy(d[f"enc_{row}_{grp}_loc"])
        ls[row, s0:s0 + gl] = torch.from_numpy(d[f"enc_{row}_{grp}_log_scale"])
        rows.append(row), starts.append(s0), glens.append(gl)
    assert max(glens) >= 300
    # identical fp32 scoring inputs for both sides: sigma = softplus(log_scale) / 6 taken on the CPU like the reference
    # (the device's softplus differs by an ulp in some elements, which moves z by 1e-6 relative -- not the scorer's business)
    # -- and on the very slices the reference passes to softplus (test_model.py:507-512): torch's vectorised CPU kernels
    # round the last ulp differently for the vector body and the scalar tail, so the position in the slice matters
    scale = torch.zeros(3, D)
    p_scale_c = torch.ones(D)
    pls = torch.from_numpy(d["p_log_scale"])
    for r_, s_, g_ in zip(rows, starts, glens):
        scale[r_, s_:s_ + g_] = O.st(ls[r_, s_:s_ + g_])
        p_scale_c[s_:s_ + g_] = O.st(pls[s_:s_ + g_])
    scale[scale == 0] = 1.0
    scale, p_scale = scale.to(DEV), p_scale_c.to(DEV)
    p_loc = torch.from_numpy(d["p_loc"]).to(DEV)
    for mode in (ops.REC_EXACT, ops.REC_FAST):
        idx, z, best, _ = ops.rec_score_argmax(loc.to(DEV), scale, p_loc, p_scale, tabs, gum, rows, starts, glens, mode=mode)
        for b, (row, grp, ref_idx, margin, gl) in enumerate(enc):
            assert int(idx[b]) == int(ref_idx), (mode, b, int(idx[b]), ref_idx, margin)
            np.testing.assert_allclose(z[b, :int(gl)].cpu().numpy(), d[f"enc_{int(row)}_{int(grp)}_z"], rtol=1e-12)
            assert float(best[b, 0] - best[b, 1]) == pytest.approx(float(margin), rel=1e-4, abs=1e-6)
