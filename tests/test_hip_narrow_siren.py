"""Narrow SIRENs (uniform hidden width 16 / 24) in the 16-bit modes (siren_mlp_rowwave.hip): the kernel family against an fp32
restatement of the MLP, its input layouts and options against the plain launch, and the models / drivers at these widths
against the CPU oracle (run with -m gpu)."""
import os

import numpy as np
import pytest
import torch

from golden_util import O, assert_close_mostly, cfg_of, load

pytestmark = pytest.mark.gpu

from recombiner_amd import config, drivers, ops, utils  # noqa: E402
from recombiner_amd import prior_model as PM  # noqa: E402
from recombiner_amd.ops import SirenMeta  # noqa: E402

DEV = "cuda"


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


def _mlp(dims, xf, pe, wv):
    """the MLP in plain fp32 torch: x @ W + b, sin(30 x), rows of layer vectors [bias | W(in, out)]"""
    G = pe.shape[0]
    x = torch.cat([xf[None].expand(G, -1, -1), pe], -1)
    lo, nl = 0, len(dims) - 1
    for l in range(nl):
        n = dims[l + 1] * (dims[l] + 1)
        v = wv[:, lo:lo + n]
        x = x @ v[:, dims[l + 1]:].reshape(G, dims[l], dims[l + 1]) + v[:, :dims[l + 1]].unsqueeze(1)
        if l != nl - 1:
            x = torch.sin(30.0 * x)
        lo += n
    return x


def _meta(case, prec):
    return SirenMeta(samples=case["S"], n_pix=case["P"], fourier_dim=case["F"], pe_dim=case["E"], n_hidden=case["n_hidden"],
                     hidden=case["hidden"], out_dim=case["C"], precision=prec)


CASES = [dict(F=16, E=16, n_hidden=3, C=3, P=1024, N=3, S=1),      # cifar
         dict(F=16, E=16, n_hidden=1, C=3, P=100, N=2, S=2),       # ragged last tile, 2 samples
         dict(F=16, E=16, n_hidden=4, C=1, P=800, N=2, S=1),       # audio output
         dict(F=18, E=16, n_hidden=3, C=3, P=192, N=2, S=1)]       # video input width 34 (two k-steps in layer 0)


@pytest.mark.parametrize("hidden", [16, 24])
@pytest.mark.parametrize("prec", [1, 2])
def test_narrow_siren_against_fp32_restatement(prec, hidden):
    """forward, fused loss + backward (sse, dW, dpe) and plain backward against fp32 autograd at the initialisation scale, within
    the limits of the width-32 kernels (test_siren_16bit_operands_at_init_scale); repeated launches are bit-identical.
    Measured on MI355X, worst over the cases and both widths: bf16 y 7.1e-3, sse 2.5e-4, dW 2.8e-3, dpe 1.4e-2, plain backward
    dW 7.4e-3; f16 y 1.2e-3, sse 3.5e-5, dW 3.9e-4, dpe 1.7e-3, plain backward dW 1.1e-3.  (These limits carry the operands'
    rounding noise; the kernel's own arithmetic is held per layer, input half and row against an fp64 evaluator with its
    rounding points in test_hip_siren_operand_exact.py, family "narrow", 1 to 4 hidden layers.)"""
    lim = {1: (2.0e-2, 6e-4, 9e-3, 3.0e-2), 2: (2.7e-3, 6e-5, 1.4e-3, 3.6e-3)}[prec]
    worst = np.zeros(6)
    for case in CASES:
        case = dict(case, hidden=hidden)
        S, N, P, C = case["S"], case["N"], case["P"], case["C"]
        dims, D, xf, pe, wv, y = _case(seed=3, **case)
        meta = _meta(case, prec)
        assert meta.d_net == D
        pe_r, wv_r = pe.clone().requires_grad_(True), wv.clone().requires_grad_(True)
        y_ref = _mlp(dims, xf, pe_r, wv_r)
        tgt = y.repeat_interleave(S, 0)
        scale = 1.0 / (S * P * C)
        (((y_ref - tgt) ** 2).sum() * scale).backward()
        y_hip = ops.siren_fwd(g(xf), g(pe), g(wv), meta)
        sse, dw, dpe = ops.siren_loss_bwd(g(xf), g(pe), g(wv), g(y), scale, meta)
        dy = 1e-3 * torch.randn(N * S, P, C, generator=torch.Generator().manual_seed(9))
        pe_b, wv_b = pe.clone().requires_grad_(True), wv.clone().requires_grad_(True)
        (_mlp(dims, xf, pe_b, wv_b) * dy).sum().backward()
        dwb, dpeb = ops.siren_bwd(g(xf), g(pe), g(wv), g(dy), meta)
        e = np.array([rel_err(y_hip, y_ref.detach()), rel_err(sse, ((y_ref.detach() - tgt) ** 2).sum((1, 2))),
                      rel_err(dw, wv_r.grad), rel_err(dpe, pe_r.grad), rel_err(dwb, wv_b.grad), rel_err(dpeb, pe_b.grad)])
        worst = np.maximum(worst, e)
        # bitwise deterministic: no atomics, fixed summation order
        sse2, dw2, dpe2 = ops.siren_loss_bwd(g(xf), g(pe), g(wv), g(y), scale, meta)
        assert torch.equal(sse, sse2) and torch.equal(dw, dw2) and torch.equal(dpe, dpe2)
        assert torch.equal(ops.siren_fwd(g(xf), g(pe), g(wv), meta), y_hip)
        dwb2, dpeb2 = ops.siren_bwd(g(xf), g(pe), g(wv), g(dy), meta)
        assert torch.equal(dwb, dwb2) and torch.equal(dpeb, dpeb2)
    print("width %d prec %d: worst rel err y %.2e sse %.2e dW %.2e dpe %.2e | bwd dW %.2e dpe %.2e" % (hidden, prec, *worst))
    assert (worst[:4] < np.array(lim)).all(), (worst, lim)
    assert worst[4] < lim[2] and worst[5] < lim[3], (worst, lim)


@pytest.mark.parametrize("hidden", [16, 24])
@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("F", [16, 18])
def test_narrow_siren_16bit_inputs_equal_fp32_inputs(F, prec, hidden):
    """bf16 pe (and the 16-bit copy of xf that comes with it) against the same values in fp32: bit-identical results; dpe is then
    written as bf16, equal to the fp32 dpe rounded"""
    case = dict(F=F, E=16, n_hidden=3, C=3, P=1000, N=3, S=2, hidden=hidden)
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


@pytest.mark.parametrize("pn,ps,S,hidden,prec", [((2, 3), (8, 16), 2, 16, 1), ((3,), (200,), 1, 24, 1), ((2, 1, 2), (4, 6, 10), 1, 16, 2),
                                                 ((2, 2), (16, 16), 1, 24, 2)])
def test_narrow_siren_stitched_pe_layout_is_bit_identical(pn, ps, S, hidden, prec):
    """rcb_siren_desc.pe_grid_dims: pe / dpe inside the stitched grids of the patched presets == the patch-major launch"""
    P, per = int(np.prod(ps)), int(np.prod(pn))
    case = dict(F=16, E=16, n_hidden=3, C=3, P=P, N=2 * per, S=S, hidden=hidden)
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


@pytest.mark.parametrize("hidden,prec", [(16, 1), (24, 2)])
def test_narrow_siren_pixel_chunks_and_gradient_planes(hidden, prec):
    """pixel_chunks = 4 + rcb_siren_reduce_chunks against the unchunked launch (dpe equal, dW the same sums in another fixed
    association); the bf16 copy and the (hi, lo) planes of the gradient equal dW rounded and its remainder"""
    case = dict(F=16, E=16, n_hidden=3, C=3, P=1000, N=3, S=2, hidden=hidden)
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


def test_narrow_siren_refusals():
    """per-layer width lists stay fp32-only, F or E above 32 and the clock probe are refused by the narrow family"""
    xf = torch.zeros(64, 40, device=DEV)
    pe = torch.zeros(1, 64, 8, device=DEV)
    bad = SirenMeta(1, 64, 40, 8, 3, 16, 3, precision=1)
    with pytest.raises(ops.RcbError):
        ops.siren_fwd(xf, pe, torch.zeros(1, bad.d_net, device=DEV), bad)
    mixed = SirenMeta(1, 64, 16, 16, 2, 24, 3, precision=1, hidden_dims=(16, 24))
    with pytest.raises(ops.RcbError):
        ops.siren_fwd(xf[:, :16].contiguous(), torch.zeros(1, 64, 16, device=DEV), torch.zeros(1, mixed.d_net, device=DEV), mixed)
    meta = SirenMeta(1, 64, 16, 16, 3, 16, 3, precision=1)
    with pytest.raises(ops.RcbError):
        ops.siren_loss_bwd(xf[:, :16].contiguous(), torch.zeros(1, 64, 16, device=DEV), torch.zeros(1, meta.d_net, device=DEV),
                           torch.zeros(1, 64, 3, device=DEV), 1.0, meta, clock_probe=torch.zeros(256, 4, dtype=torch.int64, device=DEV))


def _feed(m, eps_list):
    q = [e.clone() for e in eps_list]
    m.noise_source = lambda shape: q.pop(0)
    return q


@pytest.mark.parametrize("name,width,prec", [("cifar", 16, 1), ("patch2d", 24, 1), ("cifar", 24, 2)])
def test_narrow_siren_models_train_like_the_oracle(name, width, prec):
    """two training steps with trained mappings on the oracle's own noise at hidden width 16 / 24: ELBO / MSE / KL within 16-bit
    operand rounding of the fp32 CPU oracle, parameters within Adam's step size (the tolerances of the width-48 / 64 variants)"""
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
    np.testing.assert_array_equal(m.loc.detach().cpu().numpy(), p["loc"].numpy())
    torch.manual_seed(77)
    noise = O.Noise()
    mse_o, kl_o, elbo_o = O.prior_train(geo, p, X[None].repeat(n, 1, 1), Y, pri, A, upo, 2, 2e-4, 1e-4, True, noise)
    _feed(m, noise.drawn)
    prg = [None if q is None else q.to(DEV) for q in pri]
    mse, kl, elbo = m.train(2, 2e-4, X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV), *prg, lt, up, 1e-4, training_mappings=True)
    np.testing.assert_allclose([mse, kl], [mse_o, kl_o], rtol=2e-3)
    np.testing.assert_allclose(elbo, elbo_o, rtol=2e-3)
    assert_close_mostly(m.loc, p["loc"].detach(), rtol=0, atol=1.5e-4, max_frac=0.02, hard_atol=8.2e-4, what="loc")
    assert_close_mostly(lt.A[1], A[1].detach(), rtol=0, atol=1.5e-4, max_frac=0.02, hard_atol=8.2e-4, what="A1")


def test_narrow_siren_compression_round_trip(tmp_path):
    """width 16, bf16 mode: prior training with a checkpoint, compression of a few CIFAR-sized images, and the standalone decoder
    reproduces the encoder's reconstruction bit for bit"""
    from recombiner_amd import bitstream
    cfg = dict(config.configs["cifar"], hidden_dims=[16] * 3)
    n = 16
    X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], n, 3, seed=2)
    path = os.path.join(tmp_path, "PRIOR16.pkl")
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
