"""The combined launches of the captured training step (csrc/step_fused.hip) against the separate launches they replace.  Every merge keeps the arithmetic per element and every summation order: the criterion
is equality to the bit (torch.equal), never a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from recombiner_amd import _lib, config, ops, utils
from recombiner_amd import prior_model as PM

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _eq(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a.view(torch.uint8) if a.dtype == torch.bfloat16 else a, b.view(torch.uint8) if b.dtype == torch.bfloat16 else b), what


# ---- rcb_step_prepare ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms,stage1_bf16", [(2, True), (3, True), (2, False)])
def test_step_prepare_equals_begin_pack_and_weff_build(terms, stage1_bf16):
    gen = torch.Generator().manual_seed(11)
    sizes = [1056, 1056, 1056, 99]                     # the CIFAR SIREN's layer vectors
    slices, lo = [], 0
    for n in sizes:
        slices.append((lo, lo + n))
        lo += n
    A = [(torch.randn(n, n, generator=gen) * 0.03).to(DEV) for n in sizes]
    W1 = (torch.randn(64, 128, 5, 5, generator=gen) * 0.05).to(DEV)
    b1 = torch.randn(64, generator=gen).to(DEV)
    W2 = (torch.randn(64, 64, 3, 3, generator=gen) * 0.05).to(DEV)
    W3 = (torch.randn(16, 64, 3, 3, generator=gen) * 0.05).to(DEV)
    tab = ops.adam_table(2e-4, 16).to(DEV)
    for step_value in (0, 5, 40):                      # (40: past the table, clamped to its last row)
        step = torch.tensor([step_value], device=DEV, dtype=torch.int64)
        # reference: the three launches
        ref_t = ops.ATransform(slices, DEV, terms)
        ref_t.packed.fill_(7.0)
        dyn_r = torch.full((2,), -1.0, device=DEV)
        slots_r = torch.arange(1024, device=DEV, dtype=torch.int64) + 3
        ops.step_begin(tab, step, dyn_r, slots_r)
        ref_t.prepare(A)
        ref_w = ops.upconv_weff_build(W1, b1, W2, W3, stage1_bf16)
        # one launch
        new_t = ops.ATransform(slices, DEV, terms)
        new_t.packed.fill_(7.0)
        dyn_n = torch.full((2,), -1.0, device=DEV)
        slots_n = torch.arange(1024, device=DEV, dtype=torch.int64) + 3
        new_w = ops.step_prepare(tab, step, dyn_n, slots_n, new_t, A, W1, b1, W2, W3, stage1_bf16)
        torch.cuda.synchronize()
        _eq(ref_t.packed, new_t.packed, "packed A planes")
        for name, r, n_ in zip(("Weff1", "b1rep", "Weff2", "Weff3"), ref_w, new_w):
            _eq(r, n_, name)
        # the fragment pack: 16-byte fragments [18432, 20480) are an unused region nobody writes (include/rcb.h)
        assert ref_w[4].numel() == new_w[4].numel() == 22528 * 16
        for lo, hi in ((0, 18432), (20480, 22528)):
            _eq(ref_w[4][lo * 16:hi * 16], new_w[4][lo * 16:hi * 16], "fragment pack [%d, %d)" % (lo, hi))
        _eq(dyn_r, dyn_n, "dyn")
        _eq(slots_r, slots_n, "KL slots")
        assert int(slots_n.abs().sum()) == 0 and int(step) == step_value


# ---- rcb_step_tail ------------------------------------------------------------------------------------------------------
def _tail_state(rows, cols, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(DEV)
    lv = ops.LevelSpec(r(rows, cols, scale=0.05), r(rows, cols, scale=0.3) - 4.0, cols, rows)
    st = {k: (r(rows, cols, scale=1e-3).abs() if k.startswith("v") else r(rows, cols, scale=1e-3)) for k in ("m_loc", "v_loc", "m_ls", "v_ls")}
    shapes = [(1056, 1056), (99, 99), (64, 128, 5, 5), (64,), (16, 64, 3, 3), (1000,), (1025,), (1,), (3, 341), (64, 64, 3, 3)]
    ps = [r(*s, scale=0.05) for s in shapes]
    gs = [r(*s, scale=1e-3) for s in shapes]
    ms = [r(*s, scale=1e-3) for s in shapes]
    vs = [r(*s, scale=1e-3).abs() for s in shapes]
    return dict(lv=lv, st=st, ps=ps, gs=gs, ms=ms, vs=vs,
                p_loc=torch.zeros(cols, device=DEV), p_scale=torch.full((cols,), 0.02, device=DEV),
                d=r(rows, 1, cols, scale=1e-3), sse=r(rows, scale=1.0).abs(),
                tab=ops.adam_table(2e-4, 8).to(DEV), dyn=torch.zeros(2, device=DEV),
                step=torch.zeros(1, device=DEV, dtype=torch.int64), ctr=torch.tensor([41], device=DEV, dtype=torch.int64),
                slots=torch.zeros(1024, device=DEV, dtype=torch.int64), beta=torch.tensor([0.37], device=DEV),
                mse_log=torch.zeros(8, device=DEV, dtype=torch.float64), kl_log=torch.zeros(8, device=DEV, dtype=torch.float64),
                tickets=torch.zeros(ops.STEP_TAIL_TICKETS, device=DEV, dtype=torch.int32), buf=ops.sample_buffers(lv, True))


@pytest.mark.parametrize("rows,cols,redraw", [(64, 512, False), (64, 512, True), (5, 3268, False), (257, 512, True)])
def test_step_tail_equals_posterior_update_adam_and_step_end(rows, cols, redraw):
    """three steps in a row on the same state (the ticket counters must come back to zero): parameters, all moments, the next
    sample and its bf16 copy, the KL slots' sum, the MSE / KL log entries, the step and noise counters"""
    seed = 0x1234567890ABCDEF
    a, b = _tail_state(rows, cols, 21), _tail_state(rows, cols, 21)
    for s in (a, b):
        ops.reparam_rng(s["lv"], seed, 1, s["ctr"], want_bf16=True, buffers=s["buf"])
    for it in range(3):
        for s, fused in ((a, False), (b, True)):
            cfg = ops.adam_cfg(2e-4, 1, dyn=s["dyn"])
            ops.step_begin(s["tab"], s["step"], s["dyn"], s["slots"])
            # (a contribution of an earlier kernel of the step, as the network level's update leaves one)
            s["slots"][17] += 123456789 + it
            args = (s["lv"], s["p_loc"], s["p_scale"], False, 1.0, s["d"], None if redraw else s["buf"][1], 1)
            kwargs = dict(state=s["st"], kl_accum=s["slots"], kl_scalar_dev=s["beta"],
                          next_sample=ops.NextSample(s["buf"], seed, 1, s["ctr"], 1, redraw_eps=redraw))
            if fused:
                assert ops.step_tail(args, kwargs, s["ps"], s["gs"], s["ms"], s["vs"], cfg, s["tickets"], s["step"], s["sse"], 0.25,
                                     s["mse_log"], s["kl_log"], aux_counter=s["ctr"])
            else:
                ops.posterior_bwd(*args, adam=cfg, **kwargs)
                ops.adam_multi(s["ps"], s["gs"], s["ms"], s["vs"], cfg)
                ops.step_end(s["step"], s["sse"], 0.25, s["slots"], s["mse_log"], s["kl_log"], aux_counter=s["ctr"])
        torch.cuda.synchronize()
        assert int(b["tickets"].abs().sum()) == 0, "ticket counters not put back"
        _eq(a["lv"].loc, b["lv"].loc, "loc")
        _eq(a["lv"].log_scale, b["lv"].log_scale, "log_scale")
        for k in a["st"]:
            _eq(a["st"][k], b["st"][k], k)
        for k in ("ps", "ms", "vs"):
            for i, (x, y) in enumerate(zip(a[k], b[k])):
                _eq(x, y, f"{k}[{i}]")
        _eq(a["buf"][0], b["buf"][0], "next sample")
        _eq(a["buf"][1], b["buf"][1], "next noise")
        # (the bf16 copy's rows are padded to a multiple of 8 columns; nobody writes the padding)
        _eq(a["buf"][2][:, :cols].contiguous(), b["buf"][2][:, :cols].contiguous(), "next sample, bf16 copy")
        assert int(a["slots"].sum()) == int(b["slots"].sum()) and int(a["slots"][-1]) == int(b["slots"][-1]) == 0
        _eq(a["mse_log"], b["mse_log"], "MSE log")
        _eq(a["kl_log"], b["kl_log"], "KL log")
        assert int(a["step"]) == int(b["step"]) == it + 1 and int(a["ctr"]) == int(b["ctr"]) == 42 + it
        assert float(b["kl_log"][it]) > 0 and float(b["mse_log"][it]) > 0


def test_step_tail_declines_levels_off_the_flat_path():
    """a level whose element count is no multiple of 4 does not take the flat fast path: step_tail launches nothing and says so"""
    s = _tail_state(3, 3267, 5)
    cfg = ops.adam_cfg(2e-4, 1)
    eps = torch.randn(3, 1, 3267, device=DEV)
    before = s["lv"].loc.clone()
    ok = ops.step_tail((s["lv"], s["p_loc"], s["p_scale"], False, 1.0, s["d"], eps, 1), dict(state=s["st"], kl_accum=s["slots"]),
                       s["ps"], s["gs"], s["ms"], s["vs"], cfg, s["tickets"], s["step"], s["sse"], 1.0, s["mse_log"], s["kl_log"])
    torch.cuda.synchronize()
    assert ok is False and torch.equal(before, s["lv"].loc) and int(s["step"]) == 0


# ---- the training step ---------------------------------------------------------------------------------------------------
def _train(monkeypatch, fused_env, n, steps, precision, training_mappings, calls=1):
    if fused_env is None:
        monkeypatch.delenv("RCB_STEP_FUSED", raising=False)
    else:
        monkeypatch.setenv("RCB_STEP_FUSED", fused_env)
    cfg = config.configs["cifar"]
    X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], n, 3, seed=2)
    Xd, Yd = X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV)
    torch.manual_seed(77)                      # (the in-kernel noise seed takes torch.initial_seed() in)
    m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["data_dim"], cfg["pixel_sizes"],
                         cfg["upsample_factors"], cfg["latent_dim"], False, None, None, random_seed=42, device=DEV)
    m.precision = precision
    torch.manual_seed(123)
    lt = PM.LinearTransform(m.dims).to(DEV)
    torch.manual_seed(124)
    up = PM.Upsample(2, cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
    D, s0 = m._d_net, 0.0211547
    pri = [torch.zeros(D, device=DEV), torch.full((D,), s0, device=DEV), torch.zeros(2, 2, 128, device=DEV),
           torch.full((2, 2, 128), s0, device=DEV)] + [None] * 4
    launched = {"prepare": 0, "tail": 0}
    real_prepare, real_tail = ops.step_prepare, ops.step_tail

    def count_prepare(*a, **k):
        launched["prepare"] += 1
        return real_prepare(*a, **k)

    def count_tail(*a, **k):
        r = real_tail(*a, **k)
        launched["tail"] += int(bool(r))
        return r
    monkeypatch.setattr(ops, "step_prepare", count_prepare)
    monkeypatch.setattr(ops, "step_tail", count_tail)
    out = {"elbo": [], "mse": [], "kl": []}
    for _ in range(calls):
        mse, kl, elbo = m.train(steps, 2e-4, Xd, Yd, *pri, lt, up, 1e-8, training_mappings=training_mappings)
        out["elbo"] += list(elbo)
        out["mse"].append(mse)
        out["kl"].append(kl)
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "step_prepare", real_prepare)
    monkeypatch.setattr(ops, "step_tail", real_tail)
    params = {"model." + k: v.detach().clone() for k, v in m.named_parameters()}
    params.update({"lt." + k: v.detach().clone() for k, v in lt.named_parameters()})
    params.update({"up." + k: v.detach().clone() for k, v in up.named_parameters()})
    return out, params, launched


def _same(run_a, run_b):
    (out_a, par_a, _), (out_b, par_b, _) = run_a, run_b
    assert out_a["elbo"] == out_b["elbo"] and out_a["mse"] == out_b["mse"] and out_a["kl"] == out_b["kl"]
    assert np.isfinite(out_a["elbo"]).all()
    assert par_a.keys() == par_b.keys() and len(par_a) >= 4 + 4 + 6
    for k in par_a:
        _eq(par_a[k], par_b[k], k)


def test_training_step_with_combined_launches_equals_separate_launches(monkeypatch):
    """CIFAR preset, 64 INRs, 12 steps (eager warm-up, capture, replay), then a second call on the cached graph"""
    fused = _train(monkeypatch, None, 64, 12, 1, True, calls=2)
    assert fused[2]["prepare"] >= 4 and fused[2]["tail"] >= 4, fused[2]          # (3 eager steps + the capture, at least)
    sep = _train(monkeypatch, "0", 64, 12, 1, True, calls=2)
    assert sep[2] == {"prepare": 0, "tail": 0}
    _same(fused, sep)


@pytest.mark.parametrize("precision,training_mappings", [(1, False), (0, True), (0, False)])
def test_other_configurations_keep_the_separate_launches(monkeypatch, precision, training_mappings):
    """frozen mappings (no pack, no weight build, no Adam on the mappings in the step) and the fp32 mode (no packed A, no
    phase-form weights, no forked backward): nothing is combined, the step still runs, and RCB_STEP_FUSED changes nothing."""
    on = _train(monkeypatch, None, 64, 12, precision, training_mappings)
    off = _train(monkeypatch, "0", 64, 12, precision, training_mappings)
    assert on[2] == {"prepare": 0, "tail": 0} and off[2] == {"prepare": 0, "tail": 0}
    for run in (on, off):
        assert len(run[0]["elbo"]) == 12 and np.isfinite(run[0]["elbo"]).all()
    if precision != 0:
        _same(on, off)
    # (fp32 mode: the upsampling net runs on MIOpen and the A transform on library GEMMs, whose weight gradients are not
    # bitwise reproducible from run to run; the two runs took the same launches -- counted above -- which is the claim here)
