"""Deep SIRENs (5 to 7 hidden layers of one width): the 16-bit kernel family (siren_mlp_rowwave.hip) against an fp32 restatement of
the MLP and a CPU emulation of its operand rounding, its input layouts and options against the plain launch, the fp32 parity
path at depth, and the models / drivers at depth against the CPU oracle (run with -m gpu; the descriptor check runs without)."""
import math
import os

import numpy as np
import pytest
import torch

from golden_util import O, assert_close_mostly, cfg_of, load

from recombiner_amd import config, drivers, ops, utils  # noqa: E402
from recombiner_amd import prior_model as PM  # noqa: E402
from recombiner_amd.ops import SirenMeta  # noqa: E402

DEV = "cuda"
gpu = pytest.mark.gpu


def g(x):
    return None if x is None else x.to(DEV).contiguous()


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _case(F, E, n_hidden, C, P, N, S, seed, hidden):
    """inputs of one launch; weights at the SIREN initialisation scale of the width (sqrt(6 / hidden) / 30)"""
    gen = torch.Generator().manual_seed(seed)
    dims = [F + E] + [hidden] * n_hidden + [C]
    D = sum(dims[i + 1] * (dims[i] + 1) for i in range(len(dims) - 1))
    xf = torch.rand(P, F, generator=gen) * 2 - 1
    pe = torch.randn(N * S, P, E, generator=gen) * 0.5
    wv = (torch.rand(N * S, D, generator=gen) * 2 - 1) * (np.sqrt(6 / hidden) / 30)
    y = torch.rand(N, P, C, generator=gen)
    return dims, D, xf, pe, wv, y


def _layers(dims, wv):
    """rows of layer vectors [bias | W(in, out)] -> [(W [G, in, out], b [G, out])]"""
    out, lo = [], 0
    for l in range(len(dims) - 1):
        n = dims[l + 1] * (dims[l] + 1)
        v = wv[:, lo:lo + n]
        out.append((v[:, dims[l + 1]:].reshape(-1, dims[l], dims[l + 1]), v[:, :dims[l + 1]]))
        lo += n
    return out


def _mlp(dims, xf, pe, wv):
    """the MLP in plain fp32 torch: x @ W + b, sin(30 x)"""
    x = torch.cat([xf[None].expand(pe.shape[0], -1, -1), pe], -1)
    lay = _layers(dims, wv)
    for l, (W, b) in enumerate(lay):
        x = x @ W + b.unsqueeze(1)
        if l != len(lay) - 1:
            x = torch.sin(30.0 * x)
    return x


def _emulate(dims, xf, pe, wv, prec, tgt=None, scale=None, dy=None):
    """CPU emulation of the 16-bit kernels' arithmetic: weights, layer inputs, sines and dz rounded to the operand type, fp32
    accumulation and cosines, sine layers in revolutions, f16 weights / gradients scaled by 2^10.  -> y, sse, dW, dpe"""
    T = torch.bfloat16 if prec == 1 else torch.float16
    WS = GS = 1.0 if prec == 1 else 1024.0
    r = lambda t: t.to(T).float()                                                   # noqa: E731
    w0 = 30.0
    kw = float(np.float32(w0 / (2 * math.pi))) * WS
    lay = _layers(dims, wv)
    nl = len(lay)
    h = [r(torch.cat([xf[None].expand(pe.shape[0], -1, -1), pe], -1))]
    cos = []
    for l in range(nl - 1):
        W, b = lay[l]
        z = (h[-1] @ r(W * kw) + (b * kw).unsqueeze(1)) / WS
        h.append(r(torch.sin(2 * math.pi * z)))
        cos.append(torch.cos(2 * math.pi * z))
    W, b = lay[-1]
    y = (h[-1] @ r(W * WS)) / WS + b.unsqueeze(1)
    if tgt is not None:
        diff = y - tgt
        sse = (diff ** 2).sum((1, 2))
        dz = r(2.0 * GS * scale * diff)
    else:
        sse = None
        dz = r(dy * GS)
    grads = [None] * nl
    for l in range(nl - 1, -1, -1):
        W, b = lay[l]
        grads[l] = torch.cat([dz.sum(1), (h[l].transpose(1, 2) @ dz).flatten(1)], 1) / GS
        if l > 0:
            dz = r((dz @ r(W * w0).transpose(1, 2)) * cos[l - 1])
        else:
            F = xf.shape[1]
            dpe = (dz @ r(W[:, F:] * WS).transpose(1, 2)) / (GS * WS)
    return y, sse, torch.cat(grads, 1), dpe


def _meta(case, prec):
    return SirenMeta(samples=case["S"], n_pix=case["P"], fourier_dim=case["F"], pe_dim=case["E"], n_hidden=case["n_hidden"],
                     hidden=case["hidden"], out_dim=case["C"], precision=prec)


CASES = [dict(F=16, E=16, C=3, P=1024, N=3, S=1),      # cifar
         dict(F=16, E=16, C=1, P=100, N=2, S=2),       # ragged last tile, 2 samples, audio output
         dict(F=18, E=16, C=3, P=192, N=2, S=1)]       # video input width 34 (two k-steps in layer 0)


@gpu
@pytest.mark.parametrize("n_hidden", [5, 7])
@pytest.mark.parametrize("hidden", [16, 24, 32])
@pytest.mark.parametrize("prec", [1, 2])
def test_deep_siren_against_fp32_restatement(prec, hidden, n_hidden):
    """forward, fused loss + backward (sse, dW, dpe) and plain backward against fp32 autograd at the initialisation scale;
    repeated launches are bit-identical.  The limit of each quantity is the larger of the depth-3 limit of the narrow family and
    three times the error of a CPU emulation of the same network with operands rounded as the kernel rounds them (fp32
    accumulation): depth compounds the operand rounding through sin(30 z).
    Measured on MI355X, worst over the cases, widths and depths (the emulation is within a few per cent of each): bf16 y 2.0e-2,
    sse 4.0e-4, dW 5.6e-3, dpe 2.6e-2, plain backward dW 1.6e-2, dpe 2.5e-2; f16 y 1.9e-3, sse 4.4e-5, dW 5.9e-4, dpe 2.9e-3,
    plain backward dW 2.0e-3, dpe 3.2e-3.  (The emulation here only scales the fp32 yardstick's limits with depth; the kernel
    against an fp64 evaluator with the same rounding points, per layer, input half and row: test_hip_siren_operand_exact.py,
    family "deep".)"""
    lim3 = np.array({1: (2.0e-2, 6e-4, 9e-3, 3.0e-2, 9e-3, 3.0e-2), 2: (2.7e-3, 6e-5, 1.4e-3, 3.6e-3, 1.4e-3, 3.6e-3)}[prec])
    for case in CASES:
        case = dict(case, hidden=hidden, n_hidden=n_hidden)
        S, N, P, C = case["S"], case["N"], case["P"], case["C"]
        dims, D, xf, pe, wv, y = _case(seed=3, **case)
        meta = _meta(case, prec)
        assert meta.d_net == D
        pe_r, wv_r = pe.clone().requires_grad_(True), wv.clone().requires_grad_(True)
        y_ref = _mlp(dims, xf, pe_r, wv_r)
        tgt = y.repeat_interleave(S, 0)
        scale = 1.0 / (S * P * C)
        (((y_ref - tgt) ** 2).sum() * scale).backward()
        sse_ref = ((y_ref.detach() - tgt) ** 2).sum((1, 2))
        dy = 1e-3 * torch.randn(N * S, P, C, generator=torch.Generator().manual_seed(9))
        pe_b, wv_b = pe.clone().requires_grad_(True), wv.clone().requires_grad_(True)
        (_mlp(dims, xf, pe_b, wv_b) * dy).sum().backward()
        refs = [y_ref.detach(), sse_ref, wv_r.grad, pe_r.grad, wv_b.grad, pe_b.grad]

        ye, ssee, dwe, dpee = _emulate(dims, xf, pe, wv, prec, tgt=tgt, scale=scale)
        _, _, dwbe, dpebe = _emulate(dims, xf, pe, wv, prec, dy=dy)
        emu = np.array([rel_err(a, b) for a, b in zip([ye, ssee, dwe, dpee, dwbe, dpebe], refs)])

        y_hip = ops.siren_fwd(g(xf), g(pe), g(wv), meta)
        sse, dw, dpe = ops.siren_loss_bwd(g(xf), g(pe), g(wv), g(y), scale, meta)
        dwb, dpeb = ops.siren_bwd(g(xf), g(pe), g(wv), g(dy), meta)
        e = np.array([rel_err(a, b) for a, b in zip([y_hip, sse, dw, dpe, dwb, dpeb], refs)])
        lim = np.maximum(lim3, 3 * emu)
        print("width %d NH %d prec %d P %d: kernel y %.2e sse %.2e dW %.2e dpe %.2e | bwd dW %.2e dpe %.2e" % (hidden, n_hidden, prec, P, *e))
        print("    emulation                 y %.2e sse %.2e dW %.2e dpe %.2e | bwd dW %.2e dpe %.2e" % tuple(emu))
        assert (e < lim).all(), (e, lim)
        # bitwise deterministic: no atomics, fixed summation order
        sse2, dw2, dpe2 = ops.siren_loss_bwd(g(xf), g(pe), g(wv), g(y), scale, meta)
        assert torch.equal(sse, sse2) and torch.equal(dw, dw2) and torch.equal(dpe, dpe2)
        assert torch.equal(ops.siren_fwd(g(xf), g(pe), g(wv), meta), y_hip)
        dwb2, dpeb2 = ops.siren_bwd(g(xf), g(pe), g(wv), g(dy), meta)
        assert torch.equal(dwb, dwb2) and torch.equal(dpeb, dpeb2)


@gpu
@pytest.mark.parametrize("n_hidden", [5, 7])
@pytest.mark.parametrize("hidden", [16, 32, 40])
def test_deep_siren_fp32_parity(hidden, n_hidden):
    """the fp32 parity mode at 5 / 7 hidden layers (plain-FMA kernel) against the restatement and its autograd, within the
    tolerances of test_siren_fp32_with_different_hidden_widths.  Weights at the SIREN initialisation scale (unit gain per layer:
    at the 0.05 of the depth-3 test, sin(30 z) multiplies the last-bit differences of z by ~ 2.5 per layer) and the restatement
    in float64, so that the limits measure the kernel's fp32 arithmetic and not that of the restatement"""
    gen = torch.Generator().manual_seed(3)
    F, E, C, P, N = 16, 16, 3, 70, 3
    dims = [F + E] + [hidden] * n_hidden + [C]
    D = sum(dims[i + 1] * (dims[i] + 1) for i in range(len(dims) - 1))
    xf = torch.rand(P, F, generator=gen) * 2 - 1
    pe = torch.randn(N, P, E, generator=gen) * 0.5
    wv = (torch.rand(N, D, generator=gen) * 2 - 1) * (np.sqrt(6 / hidden) / 30)
    y = torch.rand(N, P, C, generator=gen)
    meta = SirenMeta(1, P, F, E, n_hidden, hidden, C)
    assert meta.d_net == D
    out = ops.siren_fwd(g(xf), g(pe), g(wv), meta)
    wv_r, pe_r = wv.double().requires_grad_(True), pe.double().requires_grad_(True)
    ref = _mlp(dims, xf.double(), pe_r, wv_r)
    assert rel_err(out, ref) < 1e-5
    loss = ((ref - y.double()) ** 2).sum() / (P * C)
    loss.backward()
    sse, dw, dpe = ops.siren_loss_bwd(g(xf), g(pe), g(wv), g(y), 1.0 / (P * C), meta)
    assert rel_err(sse.sum() / (P * C), loss.detach()) < 1e-5
    assert rel_err(dw, wv_r.grad) < 2e-5 and rel_err(dpe, pe_r.grad) < 2e-5


@gpu
@pytest.mark.parametrize("hidden,n_hidden,prec", [(16, 5, 1), (24, 7, 2), (32, 7, 1), (32, 6, 2)])
@pytest.mark.parametrize("F", [16, 18])
def test_deep_siren_16bit_inputs_equal_fp32_inputs(F, prec, hidden, n_hidden):
    """bf16 pe (and the 16-bit copy of xf that comes with it) against the same values in fp32: bit-identical results; dpe is then
    written as bf16, equal to the fp32 dpe rounded"""
    case = dict(F=F, E=16, n_hidden=n_hidden, C=3, P=1000, N=3, S=2, hidden=hidden)
    dims, D, xf, pe, wv, y = _case(seed=11, **case)
    meta = _meta(case, prec)
    pe16 = g(pe).bfloat16()
    pe32 = pe16.float()
    scale = 1.0 / 6000
    assert torch.equal(ops.siren_fwd(g(xf), pe32, g(wv), meta), ops.siren_fwd(g(xf), pe16, g(wv), meta))
    s32, w32, d32 = ops.siren_loss_bwd(g(xf), pe32, g(wv), g(y), scale, meta)
    s16, w16, d16 = ops.siren_loss_bwd(g(xf), pe16, g(wv), g(y), scale, meta)             # with the xf copy
    assert d16.dtype == torch.bfloat16
    assert torch.equal(s32, s16) and torch.equal(w32, w16) and torch.equal(d32.bfloat16(), d16)
    os.environ["RCB_SIREN_NO_XF16"] = "1"
    try:
        s16b, w16b, d16b = ops.siren_loss_bwd(g(xf), pe16, g(wv), g(y), scale, meta)     # bf16 pe, fp32 xf
    finally:
        del os.environ["RCB_SIREN_NO_XF16"]
    assert torch.equal(s16b, s16) and torch.equal(w16b, w16) and torch.equal(d16b, d16)
    dy = 1e-3 * torch.randn(6, 1000, 3, device=DEV)
    wb32, db32 = ops.siren_bwd(g(xf), pe32, g(wv), dy, meta)
    wb16, db16 = ops.siren_bwd(g(xf), pe16, g(wv), dy, meta)
    assert torch.isfinite(wb32).all() and torch.equal(wb32, wb16) and torch.equal(db32.bfloat16(), db16)


def _stitch(t, S, pn, ps):
    """[N * S rows (row = n * S + s), P, E] -> the stitched channel-last grids [S * nd, *(pn_i * ps_i), E]"""
    G, P, E = t.shape
    dd, N = len(pn), G // S
    nd = N // int(np.prod(pn))
    v = t.view(nd, *pn, S, *ps, E)
    perm = [1 + dd, 0] + [x for i in range(dd) for x in (1 + i, 2 + dd + i)] + [2 + 2 * dd]
    return v.permute(perm).reshape(S * nd, *[a * b for a, b in zip(pn, ps)], E).contiguous()


@gpu
@pytest.mark.parametrize("pn,ps,S,hidden,n_hidden,prec", [((2, 3), (8, 16), 2, 16, 6, 1), ((3,), (200,), 1, 32, 5, 1),
                                                          ((2, 1, 2), (4, 6, 10), 1, 24, 7, 2), ((2, 2), (16, 16), 1, 32, 7, 2)])
def test_deep_siren_stitched_pe_layout_is_bit_identical(pn, ps, S, hidden, n_hidden, prec):
    """rcb_siren_desc.pe_grid_dims: pe / dpe inside the stitched grids of the patched presets == the patch-major launch"""
    P, per = int(np.prod(ps)), int(np.prod(pn))
    case = dict(F=16, E=16, n_hidden=n_hidden, C=3, P=P, N=2 * per, S=S, hidden=hidden)
    dims, D, xf, pe, wv, y = _case(seed=41, **case)
    meta = _meta(case, prec)
    pe16 = g(pe).bfloat16()
    lay = ops.PeLayout(pn, ps)
    st = _stitch(pe16, S, list(pn), list(ps))
    assert torch.equal(ops.siren_fwd(g(xf), st, g(wv), meta, pe_layout=lay), ops.siren_fwd(g(xf), pe16, g(wv), meta))
    scale = 1.0 / (S * P * 3)
    s1, w1, d1 = ops.siren_loss_bwd(g(xf), pe16, g(wv), g(y), scale, meta)
    s2, w2, d2 = ops.siren_loss_bwd(g(xf), st, g(wv), g(y), scale, meta, pe_layout=lay)
    assert d2.shape == st.shape and torch.equal(s1, s2) and torch.equal(w1, w2)
    assert torch.equal(d2, _stitch(d1, S, list(pn), list(ps)))


@gpu
@pytest.mark.parametrize("hidden,n_hidden,prec", [(16, 7, 1), (24, 5, 2), (32, 7, 1)])
def test_deep_siren_pixel_chunks_and_gradient_planes(hidden, n_hidden, prec):
    """pixel_chunks = 4 + rcb_siren_reduce_chunks against the unchunked launch (dpe equal, dW the same sums in another fixed
    association); the bf16 copy and the (hi, lo) planes of the gradient equal dW rounded and its remainder"""
    case = dict(F=16, E=16, n_hidden=n_hidden, C=3, P=1000, N=3, S=2, hidden=hidden)
    dims, D, xf, pe, wv, y = _case(seed=17, **case)
    meta = _meta(case, prec)
    assert ops.siren_pixel_chunks(6, meta) == 1
    pe16 = g(pe).bfloat16()
    scale = 1.0 / 6000
    y1 = ops.siren_fwd(g(xf), pe16, g(wv), meta, pixel_chunks=1)
    assert torch.equal(ops.siren_fwd(g(xf), pe16, g(wv), meta, pixel_chunks=4), y1)
    s1, w1, d1, c1 = ops.siren_loss_bwd(g(xf), pe16, g(wv), g(y), scale, meta, want_bf16=True, pixel_chunks=1)
    assert torch.equal(c1, w1.bfloat16())
    s4, w4, d4, c4 = ops.siren_loss_bwd(g(xf), pe16, g(wv), g(y), scale, meta, want_bf16=True, pixel_chunks=4)
    assert torch.equal(d4, d1) and rel_err(s4, s1) < 2e-6 and rel_err(w4, w1) < 2e-6
    assert torch.equal(c4, w4.bfloat16())
    s5, w5, d5 = ops.siren_loss_bwd(g(xf), pe16, g(wv), g(y), scale, meta, pixel_chunks=4)
    assert torch.equal(w5, w4) and torch.equal(s5, s4)
    dy = 1e-3 * torch.randn(6, 1000, 3, device=DEV)
    wb1, db1 = ops.siren_bwd(g(xf), pe16, g(wv), dy, meta, pixel_chunks=1)
    wb4, db4 = ops.siren_bwd(g(xf), pe16, g(wv), dy, meta, pixel_chunks=4)
    assert torch.equal(db4, db1) and rel_err(wb4, wb1) < 2e-6
    for chunks in (1, 4):
        sp, none, dp, planes = ops.siren_loss_bwd(g(xf), pe16, g(wv), g(y), scale, meta, want_planes=True, pixel_chunks=chunks)
        ref = w1 if chunks == 1 else w4
        assert none is None and torch.equal(dp, d1)
        assert torch.equal(planes.hi, ref.bfloat16())
        assert torch.equal(planes.lo, (ref - ref.bfloat16().float()).bfloat16())


@gpu
@pytest.mark.parametrize("hidden,n_hidden", [(16, 7), (32, 5)])
def test_deep_siren_row_alone_equals_row_in_a_batch(hidden, n_hidden):
    """batch invariance: a row's outputs and gradient are the same bits whether it is launched alone or inside 4096 CIFAR rows
    (the family and pixel_chunks follow from the descriptor's geometry, never from the row count)"""
    F, E, C, P, G = 16, 16, 3, 1024, 4096
    meta = SirenMeta(1, P, F, E, n_hidden, hidden, C, precision=1)
    gen = torch.Generator(device=DEV).manual_seed(5)
    xf = torch.rand(P, F, device=DEV, generator=gen) * 2 - 1
    pe = (torch.randn(G, P, E, device=DEV, generator=gen) * 0.5).bfloat16()
    wv = (torch.rand(G, meta.d_net, device=DEV, generator=gen) * 2 - 1) * (np.sqrt(6 / hidden) / 30)
    y = torch.rand(G, P, C, device=DEV, generator=gen)
    assert ops.siren_pixel_chunks(G, meta) == ops.siren_pixel_chunks(1, meta)
    yb = ops.siren_fwd(xf, pe, wv, meta)
    sb, wb, db = ops.siren_loss_bwd(xf, pe, wv, y, 1e-4, meta)
    for r in (0, 1234, G - 1):
        sl = slice(r, r + 1)
        assert torch.equal(ops.siren_fwd(xf, pe[sl].contiguous(), wv[sl].contiguous(), meta), yb[sl])
        s1, w1, d1 = ops.siren_loss_bwd(xf, pe[sl].contiguous(), wv[sl].contiguous(), y[sl].contiguous(), 1e-4, meta)
        assert torch.equal(s1, sb[sl]) and torch.equal(w1, wb[sl]) and torch.equal(d1, db[sl])


@gpu
def test_deep_siren_refusals():
    """8 hidden layers in every mode, 16-bit widths other than 16 / 24 / 32 beyond 4 layers, and the clock probe are refused"""
    P = 64
    xf = torch.zeros(P, 16, device=DEV)
    pe = torch.zeros(1, P, 16, device=DEV)
    for prec in (0, 1, 2):
        meta = SirenMeta(1, P, 16, 16, 8, 32, 3, precision=prec)
        with pytest.raises(ops.RcbError):
            ops.siren_fwd(xf, pe, torch.zeros(1, meta.d_net, device=DEV), meta)
        with pytest.raises(ops.RcbError):
            ops.siren_loss_bwd(xf, pe, torch.zeros(1, meta.d_net, device=DEV), torch.zeros(1, P, 3, device=DEV), 1.0, meta)
    for prec in (1, 2):
        for width in (48, 64):
            meta = SirenMeta(1, P, 16, 16, 5, width, 3, precision=prec)
            with pytest.raises(ops.RcbError):
                ops.siren_fwd(xf, pe, torch.zeros(1, meta.d_net, device=DEV), meta)
    meta = SirenMeta(1, P, 16, 16, 6, 16, 3, precision=1)
    with pytest.raises(ops.RcbError):
        ops.siren_loss_bwd(xf, pe, torch.zeros(1, meta.d_net, device=DEV), torch.zeros(1, P, 3, device=DEV), 1.0, meta,
                           clock_probe=torch.zeros(256, 4, dtype=torch.int64, device=DEV))


def test_deep_siren_width_list_beyond_four_layers_is_refused():
    """a per-layer width list longer than the descriptor's four entries is refused on the host with RcbError (fp32 mode, where
    lists exist), in the 16-bit modes as well"""
    hid = (16, 24, 16, 24, 16)
    for prec in (0, 1):
        meta = SirenMeta(1, 64, 16, 16, 5, 24, 3, precision=prec, hidden_dims=hid)
        with pytest.raises(ops.RcbError):
            ops._siren_desc(meta, torch.zeros(1, meta.d_net), torch.zeros(64, 16), torch.zeros(1, 64, 16))


def _feed(m, eps_list):
    q = [e.clone() for e in eps_list]
    m.noise_source = lambda shape: q.pop(0)
    return q


@gpu
@pytest.mark.parametrize("name,dims,prec", [("cifar", [32] * 6, 0), ("cifar", [16] * 7, 1), ("patch2d", [32] * 5, 1),
                                            ("cifar", [24] * 6, 2)])
def test_deep_siren_models_train_like_the_oracle(name, dims, prec):
    """two training steps with trained mappings on the oracle's own noise at 5..7 hidden layers: fp32 within the tolerances of
    test_hidden_layers_of_different_widths_fp32, the 16-bit modes within those of the narrow family's model test"""
    d = load(f"prior_{name}.npz")
    cfg = dict(cfg_of(d))
    cfg["hidden_dims"] = list(dims)
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
    np.testing.assert_array_equal(m.loc.detach().cpu().numpy(), p["loc"].numpy())
    torch.manual_seed(77)
    noise = O.Noise()
    mse_o, kl_o, elbo_o = O.prior_train(geo, p, X[None].repeat(n, 1, 1), Y, pri, A, upo, 2, 2e-4, 1e-4, True, noise)
    _feed(m, noise.drawn)
    prg = [None if q is None else q.to(DEV) for q in pri]
    mse, kl, elbo = m.train(2, 2e-4, X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV), *prg, lt, up, 1e-4, training_mappings=True)
    if prec == 0:
        np.testing.assert_allclose(elbo, elbo_o, rtol=2e-4)
        np.testing.assert_allclose(m.loc.detach().cpu().numpy(), p["loc"].numpy(), rtol=1e-4, atol=3e-5)
        np.testing.assert_allclose(lt.A[1].detach().cpu().numpy(), A[1].numpy(), rtol=1e-3, atol=3e-5)
        return
    np.testing.assert_allclose([mse, kl], [mse_o, kl_o], rtol=2e-3)
    np.testing.assert_allclose(elbo, elbo_o, rtol=2e-3)
    assert_close_mostly(m.loc, p["loc"].detach(), rtol=0, atol=1.5e-4, max_frac=0.02, hard_atol=8.2e-4, what="loc")
    assert_close_mostly(lt.A[1], A[1].detach(), rtol=0, atol=1.5e-4, max_frac=0.02, hard_atol=8.2e-4, what="A1")


@gpu
def test_deep_siren_graph_replay_matches_eager():
    """[32] * 7, bf16: the captured-graph training step runs and produces what eager stepping produces (the statistics the
    width-32 graph test compares: the device noise streams of captured and eager execution differ)"""
    d = load("prior_cifar.npz")
    cfg = dict(cfg_of(d), hidden_dims=[32] * 7)
    n = int(d["n"])
    X = O.fourier_features(cfg["pixel_sizes"], cfg["fourier_dim"])
    torch.manual_seed(5)
    Y = torch.rand(n, X.shape[0], cfg["output_dim"])
    geo = O.Geometry.from_config(cfg)
    s0 = 0.0211547
    pri = [torch.zeros(geo.d_net), torch.full((geo.d_net,), s0), torch.zeros(2, 2, 128), torch.full((2, 2, 128), s0)]
    prg = [q.to(DEV) for q in pri] + [None] * 4
    res = []
    for use_graph in (True, False):
        m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["data_dim"], cfg["pixel_sizes"],
                             cfg["upsample_factors"], cfg["latent_dim"], cfg["patch"], cfg["patch_nums"],
                             cfg["hierarchical_patch_nums"], random_seed=42, device=DEV)
        m.precision = 1
        m.use_graph = use_graph
        torch.manual_seed(123)
        lt = PM.LinearTransform(m.dims).to(DEV)
        torch.manual_seed(124)
        up = PM.Upsample(cfg["data_dim"], cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
        torch.manual_seed(99)
        mse, kl, elbo = m.train(12, 2e-4, X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV), *prg, lt, up, 1e-4, training_mappings=True)
        assert len(elbo) == 12 and all(np.isfinite(elbo)) and all(e != 0 for e in elbo)
        if use_graph:
            assert m._ws is not None and m._ws["graphs"] is not None
        res.append((m.loc.detach().clone(), np.array(elbo)))
    moved = (res[0][0] - res[1][0]).abs().max().item()
    assert moved < 12 * 2e-4 * 2 + 1e-6
    np.testing.assert_allclose(res[0][1], res[1][1], rtol=5e-3)


@gpu
def test_deep_siren_compression_round_trip(tmp_path):
    """[16] * 6, bf16 mode: prior training with a checkpoint, compression of a few CIFAR-sized images, and the standalone decoder
    reproduces the encoder's reconstruction bit for bit"""
    from recombiner_amd import bitstream
    cfg = dict(config.configs["cifar"], hidden_dims=[16] * 6)
    n = 16
    X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], n, 3, seed=2)
    path = os.path.join(tmp_path, "PRIOR16x6.pkl")
    out = drivers.train_prior(cfg, "cifar", X.to(DEV)[None].expand(n, -1, -1), Y, max_bitrate=0.5, device=DEV, n_em_iter=2,
                              first_epochs=5, epochs=5, lr=2e-3, checkpoint_path=path, checkpoint_every=1, precision=1,
                              log=lambda *a: None)
    assert np.isfinite(out["elbo"]).all()
    ck = drivers.load_checkpoint(path)
    Xd = X.to(DEV)[None].expand(4, -1, -1)
    dist, model = drivers.compress(cfg, "cifar", ck, Xd, Y[:4], device=DEV, n_epochs=4, finetune_epochs=1, precision=1)
    assert np.isfinite(dist).all()
    blob = bitstream.encode(model)
    y_dec = bitstream.decode(cfg, "cifar", ck, blob, Xd, 4, device=DEV, precision=1)
    with torch.no_grad():
        assert torch.equal(y_dec, model.predict(Xd))
