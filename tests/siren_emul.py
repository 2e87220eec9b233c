"""The arithmetic of the 16-bit SIREN kernels (recombiner_amd/csrc/siren_mlp_{bf16,wave,wide,rowwave}.hip) in fp64 on the CPU.

Plain torch, float64.  Values are rounded to the operand type (bf16 or f16, round to nearest even) at exactly the points where
the kernels round them; sums, products, sines and cosines in between are fp64, i.e. exact at the scale of anything compared
here.  What a kernel output then differs by is the order of its fp32 accumulations, the error of the hardware v_sin / v_cos,
and the operands that those two push across a 16-bit rounding boundary (`perturb` below estimates that floor).

Rounding points (DESIGN.md section 4.4.1 has the same table, with one column per family):

  R1  hidden-layer forward weights      T(f32(w * f32(WS * k_hi)))          k_hi = f32(w0 / 2 pi): the accumulator is in revolutions
  R2  output-layer forward weights      T(f32(w * WS))
  R3  data-gradient weights             T(f32(w * w0))                      layers 1 .. NH (w0 folded in, no WS)
  R4  pe-gradient weights               T(f32(w * WS))                      layer 0, rows F .. F + E
  R5  inputs                            T(xf), T(pe)                        (pe stored as bf16: T(bf16(pe)), the caller passes bf16(pe))
  R6  hidden biases                     f32(f32(b * k_hi) * WS), fp32 in the accumulator      switch bias="fp32"
                                        T(b') + T(f32(b' - T(b'))), b' as above               switch bias="hilo" (wave family)
  R7  sine of every hidden layer        T(sin(2 pi t)), t = acc / WS        also the [pixel][feature] image of the weight gradient
  R8  cosine of every hidden layer      T(cos(2 pi t))                      switch cos="packed"
                                        cos(2 pi t) unrounded               switch cos="fp32"
  R9  output-layer dz                   T(2 GS dy_scale (y - target))  or  T(GS dy);  zero beyond C and beyond P
  R10 hidden-layer dz                   T(dh * cos), dh = dz_above @ R3^T   (carries GS)
  R11 store of dpe                      bf16(dpe) where pe / dpe are stored as bf16           switch dpe_store="bf16"
  --  epilogues, fp32, not rounded      dW = sum_pixels dz (x) input / GS;  dpe = dz_0 @ R4^T / (GS WS);  y = acc / WS + b_out

GS = WS = 1 for bf16 and 2^10 for f16.  With mode=None nothing is rounded and k_hi is w0 / 2 pi in fp64: the evaluator is then
the plain MLP (test_siren_emul_cpu.py ties that to autograd).  That form is what the two fp32 families (siren_mlp.hip,
siren_mlp_generic.hip) are held to; their case sets, their route and the fp32 yardstick of their limits are at the end.
"""
import math

import torch

F64 = torch.float64

# significand bits (with the implicit one), smallest normal exponent, largest finite value
FORMATS = {"bf16": (8, -126, float(torch.finfo(torch.bfloat16).max)), "f16": (11, -14, 65504.0)}
SCALES = {None: 1.0, "bf16": 1.0, "f16": 1024.0}           # GRAD_SCALE = W_SCALE of siren_op16.h
ULP = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}               # relative spacing of the operand type


def round_to(x, mode):
    """fp64 tensor -> nearest value of the operand type (ties to even, gradual underflow, overflow to infinity), as fp64"""
    if mode is None:
        return x
    sig, emin, fmax = FORMATS[mode]
    x = x.to(F64)
    _, e = torch.frexp(x)                                   # |x| = m 2^e, 0.5 <= m < 1
    q = torch.ldexp(torch.ones_like(x), torch.clamp(e - 1, min=emin) - (sig - 1))
    r = torch.round(x / q) * q                              # torch.round: half to even; x / q and r * q are exact
    r = torch.where(r.abs() > fmax, torch.copysign(torch.full_like(x, math.inf), x), r)
    return torch.where(torch.isfinite(x), r, x)


def f32(x):
    return x.to(torch.float32).to(F64)


def layer_slices(dims):
    """[(offset of the layer vector, n_in, n_out)]; a layer vector is [bias(out) | W(in, out)]"""
    out, lo = [], 0
    for l in range(len(dims) - 1):
        out.append((lo, dims[l], dims[l + 1]))
        lo += dims[l + 1] * (dims[l] + 1)
    return out


def blocks_of_dw(dims, F):
    """the blocks a weight gradient row is judged in: (kind, layer, slice of the row)"""
    out = []
    for l, (lo, nin, nout) in enumerate(layer_slices(dims)):
        out.append(("bias", l, slice(lo, lo + nout)))
        w0_ = lo + nout
        if l == 0:
            out.append(("fourier", 0, slice(w0_, w0_ + F * nout)))
            out.append(("pe", 0, slice(w0_ + F * nout, w0_ + nin * nout)))
        else:
            out.append(("weight", l, slice(w0_, w0_ + nin * nout)))
    return out


class Faults:
    """deliberately wrong arithmetic, for the test that the limits discriminate (never a property of a kernel)"""
    sine_unrounded = None          # layer whose sine stays unrounded
    bias_grad_scale = None         # (layer, factor)
    drop_last_pixel = False        # the last valid pixel left out of dW
    fourier_scale = None           # factor on the Fourier half of layer 0's weight gradient
    round_before_khi = False       # weights rounded before the multiplication by k_hi
    no_grad_scale = False          # dz rounded without GRAD_SCALE
    leak_last_dz = False           # the last valid pixel's dz also left in one padded slot of its tile (whose inputs the kernels
                                   # clamp to, or zero beside, the last valid pixel): that pixel twice in dW; needs P % 32 != 0

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Faults, k), k
            setattr(self, k, v)


def siren_emul(dims, xf, pe, wv, S, *, mode=None, bias="fp32", cos="packed", dpe_store=None, w0=30.0, target=None, dy_scale=None,
               dy=None, perturb=0.0, faults=None):
    """-> dict(y [G, P, C]; with target + dy_scale: sse [G], dW [G, D], dpe [G, P, E]; with dy instead: dW, dpe of the plain backward)

    dims    [F + E, hidden .., C]: any widths, any depth
    xf      [P, F] shared coordinate features; pe [G, P, E]; wv [G, D]; target [G / S, P, C] (row g uses target g // S)
    mode    None | "bf16" | "f16";  bias "fp32" | "hilo";  cos "packed" | "fp32";  dpe_store None | "bf16"   (see the table above)
    perturb relative change of every pre-activation (1 + perturb): stands for another fp32 accumulation order
    """
    ft = faults or Faults()
    T = lambda v: round_to(v, mode)                         # noqa: E731
    r32 = f32 if mode is not None else (lambda v: v)
    GS = WS = SCALES[mode]
    G, P, E = pe.shape
    F = xf.shape[-1]
    nl = len(dims) - 1
    NH = nl - 1
    C = dims[-1]
    k_hi = w0 / (2.0 * math.pi)
    if mode is not None:
        k_hi = float(torch.tensor(k_hi, dtype=torch.float32))
    wv = wv.to(F64)
    Ws, bs = [], []
    for lo, nin, nout in layer_slices(dims):
        bs.append(wv[:, lo:lo + nout])
        Ws.append(wv[:, lo + nout:lo + nout * (nin + 1)].reshape(G, nin, nout))
    x0 = T(torch.cat([xf.to(F64)[None].expand(G, -1, -1), pe.to(F64)], -1))                           # R5
    # ---- forward
    h, hs, cs = x0, [], []
    for l in range(NH):
        if ft.round_before_khi:
            Wf = T(Ws[l]) * (WS * k_hi)
        else:
            Wf = T(r32(Ws[l] * r32(torch.tensor(WS * k_hi, dtype=F64))))                             # R1
        b = r32(r32(bs[l] * k_hi) * WS)                                                              # R6
        if bias == "hilo" and mode is not None:
            bh = T(b)
            b = bh + T(r32(b - bh))
        else:
            assert bias in ("fp32", "hilo")
        t = (h @ Wf + b.unsqueeze(1)) / WS * (1.0 + perturb)                                          # revolutions
        s, c = torch.sin(2.0 * math.pi * t), torch.cos(2.0 * math.pi * t)
        h = s if ft.sine_unrounded == l else T(s)                                                    # R7
        assert cos in ("packed", "fp32")
        cs.append(T(c) if cos == "packed" else c)                                                    # R8
        hs.append(h)
    y = (h @ T(r32(Ws[NH] * WS))) / WS + bs[NH].unsqueeze(1)                                          # R2
    out = {"y": y}
    if target is None and dy is None:
        return out
    # ---- output gradient
    if target is not None:
        diff = y - target.to(F64).repeat_interleave(S, 0)
        out["sse"] = (diff * diff).sum((1, 2))
        dz_true = 2.0 * dy_scale * diff
    else:
        dz_true = dy.to(F64)
    dz = T(dz_true) * GS if ft.no_grad_scale else T(dz_true * GS)                                     # R9
    # ---- backward
    dW = torch.zeros_like(wv)
    inputs = [x0] + hs
    nP = P - 1 if ft.drop_last_pixel else P
    for l in range(nl - 1, -1, -1):
        lo, nin, nout = layer_slices(dims)[l]
        gb = dz[:, :nP].sum(1) / GS
        gw = inputs[l][:, :nP].transpose(1, 2) @ dz[:, :nP] / GS
        if ft.leak_last_dz:
            assert P % 32, "no padded slot in the last tile"
            gb = gb + dz[:, P - 1] / GS
            gw = gw + inputs[l][:, P - 1:].transpose(1, 2) @ dz[:, P - 1:] / GS
        if ft.bias_grad_scale is not None and ft.bias_grad_scale[0] == l:
            gb = gb * ft.bias_grad_scale[1]
        if l == 0 and ft.fourier_scale is not None:
            gw = torch.cat([gw[:, :F] * ft.fourier_scale, gw[:, F:]], 1)
        dW[:, lo:lo + nout] = gb
        dW[:, lo + nout:lo + nout * (nin + 1)] = gw.reshape(G, -1)
        if l > 0:
            dh = dz @ T(r32(Ws[l] * w0)).transpose(1, 2)                                              # R3
            v = dh * cs[l - 1]
            dz = T(v / GS) * GS if ft.no_grad_scale else T(v)                                        # R10
        else:
            out["dpe"] = round_to(dz @ T(r32(Ws[0][:, F:] * WS)).transpose(1, 2) / (GS * WS), dpe_store)   # R4, R11
    out["dW"] = dW
    return out


# ---- inputs shared by the CPU and the GPU tests -------------------------------------------------------------------------------
def make_case(F, E, dims_hidden, C, P, N, S, seed, scale="init"):
    """seeded inputs; scale "init": weights and biases uniform in +-sqrt(6 / hidden) / 30; "model": weights 3e-4, biases 3e-2
    (the regime of test_siren_model_scale_weights)"""
    gen = torch.Generator().manual_seed(seed)
    dims = [F + E] + list(dims_hidden) + [C]
    G = N * S
    D = sum(dims[i + 1] * (dims[i] + 1) for i in range(len(dims) - 1))
    xf = torch.rand(P, F, generator=gen) * 2 - 1
    pe = torch.randn(G, P, E, generator=gen) * 0.5
    if scale == "init":
        wv = (torch.rand(G, D, generator=gen) * 2 - 1) * (math.sqrt(6.0 / dims_hidden[0]) / 30.0)
    else:
        wv = (torch.rand(G, D, generator=gen) * 2 - 1) * 3e-4
        for lo, nin, nout in layer_slices(dims):
            wv[:, lo:lo + nout] = (torch.rand(G, nout, generator=gen) * 2 - 1) * 0.03
    y = torch.rand(N, P, C, generator=gen)
    dy = 1e-3 * torch.randn(G, P, C, generator=gen)          # gradient-sized: unit-scale dy overflows the f16 operands
    return dict(dims=dims, F=F, E=E, C=C, P=P, N=N, S=S, D=D, xf=xf, pe=pe, wv=wv, y=y, dy=dy, dy_scale=1.0 / (S * P * C),
                hidden=dims_hidden[0], n_hidden=len(dims_hidden), scale=scale, hidden_dims=tuple(dims_hidden))


# ---- the input sets of test_hip_siren_operand_exact.py (GPU) and test_siren_emul_cpu.py -----------------------------------------
def case_of(hidden, nh, F=16, C=3, P=33, N=1, S=1, chunks=1, scale="init", variant="f32pe", seed=0, E=16, hidden_dims=None):
    """variant: "f32pe" fp32 pe storage; "in16" bf16 pe + the 16-bit copy of xf (16-bit input rows); "pe16" bf16 pe with
    RCB_SIREN_NO_XF16=1 (fp32 xf rows, bf16 pe rows).  hidden_dims: the hidden widths one by one where they differ (fp32 mode
    only; `hidden` is then their maximum and `nh` their number, as in ops.SirenMeta)"""
    if hidden_dims is not None:
        assert len(hidden_dims) == nh and max(hidden_dims) == hidden
        hidden_dims = tuple(hidden_dims)
    return dict(hidden=hidden, nh=nh, F=F, C=C, P=P, N=N, S=S, chunks=chunks, scale=scale, variant=variant, seed=seed, E=E,
                hidden_dims=hidden_dims)


# The smallest shapes at which these kernels can still go wrong: one 32-pixel tile, one tile plus one pixel (also as the only
# row of the launch), five tiles split unevenly over two workgroups; S = 2 (a target shared by two rows); F = 18 (two k-steps in
# layer 0, a Fourier half that is no multiple of 8, packed cosines in the 16-bit-row variant); C = 1; the model scale.
CASES = {
    # siren_mlp_bf16.hip has instances for 2 and 3 hidden layers only: 1 and 4 layers at width 32 are refused in the 16-bit modes
    # (test_width_32_with_one_or_four_hidden_layers_has_no_16bit_instance); those depths run at widths 16 / 24 below
    "wg32": [case_of(32, 3, P=32, seed=1), case_of(32, 3, seed=2), case_of(32, 3, N=2, S=2, seed=3), case_of(32, 3, P=160, N=2, chunks=2, seed=4),
             case_of(32, 3, F=18, S=2, seed=5), case_of(32, 3, C=1, N=2, seed=6), case_of(32, 2, seed=7),
             case_of(32, 3, N=2, variant="in16", seed=8), case_of(32, 3, N=2, variant="pe16", seed=8), case_of(32, 3, F=18, variant="in16", seed=9),
             case_of(32, 3, N=2, scale="model", seed=10)],
    # whole tiles only, bf16 only, bf16 pe and the 16-bit copy of xf only: what the family has instances for
    "wave": [case_of(32, 3, P=64, variant="in16", seed=11), case_of(32, 3, P=64, N=2, S=2, variant="in16", seed=12),
             case_of(32, 3, P=160, N=2, chunks=2, variant="in16", seed=13), case_of(32, 3, P=160, variant="in16", seed=14),
             case_of(32, 3, P=64, N=2, scale="model", variant="in16", seed=15)],
    "wide": [case_of(48, 3, P=32, seed=21), case_of(48, 3, seed=22), case_of(48, 3, N=2, S=2, seed=23), case_of(48, 3, P=160, N=2, chunks=2, seed=24),
             case_of(64, 3, S=2, seed=25), case_of(64, 3, F=18, N=2, seed=26), case_of(64, 3, C=1, seed=27), case_of(64, 3, N=2, variant="in16", seed=28),
             case_of(64, 3, F=18, variant="pe16", seed=29), case_of(48, 3, N=2, scale="model", seed=30), case_of(64, 3, scale="model", seed=31)],
    "narrow": [case_of(16, 3, P=32, seed=41), case_of(16, 3, seed=42), case_of(16, 1, N=2, S=2, seed=43), case_of(16, 4, P=160, N=2, chunks=2, seed=44),
               case_of(16, 3, F=18, seed=45), case_of(24, 3, N=2, S=2, seed=46), case_of(24, 4, F=18, seed=47), case_of(24, 1, C=1, N=2, seed=48),
               case_of(24, 3, P=160, chunks=2, seed=49), case_of(24, 3, N=2, variant="in16", seed=50), case_of(16, 3, variant="pe16", seed=51),
               case_of(16, 3, N=2, scale="model", seed=52), case_of(24, 3, scale="model", seed=53)],
    "deep": [case_of(16, 5, P=32, seed=61), case_of(16, 5, seed=62), case_of(16, 7, N=2, S=2, seed=63), case_of(32, 6, P=160, N=2, chunks=2, seed=64),
             case_of(32, 6, F=18, seed=65), case_of(16, 7, C=1, seed=66), case_of(32, 6, N=2, variant="in16", seed=67),
             case_of(16, 5, N=2, scale="model", seed=68), case_of(32, 6, scale="model", seed=69)],
}
CASES["wg32"] += CASES["wave"]          # the sibling families are held to the same evaluator on the same inputs

# The two fp32 families (precision 0; test_hip_siren_fp32_exact.py), held to the evaluator with mode=None: the plain MLP in fp64.
# At most 4 rows of one to five tiles.
CASES_FP32 = {
    # siren_mlp.hip, width 32 on the fp32 MFMA: every instance X(NH, KS, NB) of RCB_SIREN_FP32_INSTANCES (test_siren_emul_cpu.py
    # holds that against siren_route.h); P = 32 leaves three of the four waves without a tile, P = 1 / 31 / 33 pad a tile, 160 is
    # five tiles dealt 2, 1, 1, 1; C beyond 16 fills the second half of the output rows; F + E = 48 pads the second input block
    "fp32": [case_of(32, 3, P=32, seed=101), case_of(32, 1, C=1, P=1, seed=102), case_of(32, 2, P=31, N=2, S=2, seed=103),
             case_of(32, 4, C=17, seed=104), case_of(32, 3, F=18, P=160, N=2, seed=105), case_of(32, 3, F=32, E=32, C=32, seed=106),
             case_of(32, 3, F=16, E=32, S=2, seed=107), case_of(32, 3, E=0, N=2, seed=108), case_of(32, 1, E=0, C=1, seed=109),
             case_of(32, 2, N=2, scale="model", seed=110), case_of(32, 3, F=32, E=32, scale="model", seed=111)],
    # siren_mlp_generic.hip, plain FMAs: the instance of up to 5 linear layers (ML = 5) and the one of up to 8; width 1; widths that
    # are no multiple of 8; the 64 x 65 layer vector that fills all 17 gradient registers of a thread; per-layer widths, the widest
    # in the middle and at the end; C above every hidden width (it then sets the LDS row stride ws)
    "generic": [case_of(1, 1, seed=121), case_of(12, 3, N=2, S=2, seed=122), case_of(40, 2, P=160, seed=123),
                case_of(64, 1, F=32, E=32, seed=124), case_of(40, 3, hidden_dims=(24, 40, 16), seed=125),
                case_of(64, 3, C=1, hidden_dims=(8, 12, 64), seed=126), case_of(16, 5, seed=127), case_of(40, 7, N=2, seed=128),
                case_of(16, 7, C=32, P=1, seed=129), case_of(40, 5, E=0, seed=130), case_of(12, 2, C=32, S=2, seed=131),
                case_of(40, 3, N=2, scale="model", seed=132), case_of(16, 5, scale="model", seed=133)],
}
CASES.update(CASES_FP32)


def fp32_route(c):
    """the kernel instance that runs a case at precision 0, restated from siren_route.h (test_siren_emul_cpu.py holds this
    function to the header on every case of CASES_FP32): ("fp32", NH, KS, NB), ("generic", ML) or None (refused)"""
    nh, F, E = c["nh"], c["F"], c["E"]
    if c["hidden"] != 32 or c["hidden_dims"] is not None or nh > 4:
        return ("generic", 8 if nh + 1 > 5 else 5)
    for NH, KS, NB in ((3, 16, 1), (2, 16, 1), (3, 18, 2), (1, 16, 1), (4, 16, 1), (3, 32, 2)):
        if nh == NH and max(F, E) <= KS and (F + E + 31) // 32 == NB:
            return ("fp32", NH, KS, NB)
    return None


def switches(family, c):
    """the evaluator switches of a family: the wave family feeds the hidden biases through the matrix pipe as
    (hi, lo) halves; the cosine stays in fp32 in the narrow, deep and wave families and in the width-32 workgroup family's
    16-bit-row instance with one input block (COS32: the fused loss / backward only, the plain backward has no such instance),
    and is packed to the operand type everywhere else"""
    sw = dict(bias="hilo" if family == "wave" else "fp32", cos="packed", cos_bwd="packed")
    if family in ("narrow", "deep", "wave"):
        sw.update(cos="fp32", cos_bwd="fp32")
    elif family == "wg32" and c["variant"] == "in16" and c["F"] % 8 == 0:
        sw.update(cos="fp32")
    return sw


def build(c):
    return make_case(c["F"], c["E"], list(c["hidden_dims"] or [c["hidden"]] * c["nh"]), c["C"], c["P"], c["N"], c["S"], c["seed"], c["scale"])


# one small case per family, three hidden layers (the deep family's smallest is five), taken from CASES so that it is one of the
# cases the limits of test_hip_siren_operand_exact.py were measured on
DISCRIMINATION = {"wg32": CASES["wg32"][2], "wave": CASES["wave"][1], "wide": CASES["wide"][4], "narrow": CASES["narrow"][5],
                  "deep": CASES["deep"][1]}
# the fp32 families: a tile with padded slots (the fault that leaks into one needs it) and a target shared by two rows
DISCRIMINATION.update({"fp32": CASES["fp32"][2], "generic": CASES["generic"][1]})


# ---- the flip floor ------------------------------------------------------------------------------------------------------------
# A pre-activation that a kernel's fp32 accumulation order or the v_sin error puts on the other side of a 16-bit rounding boundary
# than the evaluator's fp64 value moves one activation by an ulp, and with it the y and dpe of its pixel and, less, every
# gradient entry.  No kernel can avoid that.  FLIP_FLOOR is the largest effect on a block, per operand type and block kind, of
# changing every pre-activation by a relative +-2^-22 in the evaluator alone, over all input sets above (divided by the block's
# largest entry; rounded up to two digits).  test_siren_emul_cpu.py::test_sensitivity_floor recomputes it and asserts that no
# block of any input set has more than FLIP_SHARE of its elements beyond it; the GPU test sets no "largest error" limit below it
# and accepts no element beyond twice it.
FLIP_SHARE = 1e-3
FLIP_FLOOR = {
    "bf16": {("y", "row"): 3.7e-03, ("sse", "row"): 1.8e-05, ("dpe", "row"): 5.8e-03, ("bwd_dpe", "row"): 5.6e-03, ("dW", "bias"): 1.4e-03, ("dW", "fourier"): 2.9e-03, ("dW", "pe"): 3.5e-03, ("dW", "weight"): 2.4e-03, ("bwd_dW", "bias"): 2.2e-03, ("bwd_dW", "fourier"): 2.2e-03, ("bwd_dW", "pe"): 2.6e-03, ("bwd_dW", "weight"): 2.6e-03, ("dpe16", "row"): 6.1e-03, ("bwd_dpe16", "row"): 5.7e-03},
    "f16": {("y", "row"): 6.6e-04, ("sse", "row"): 3.5e-06, ("dpe", "row"): 7.4e-04, ("bwd_dpe", "row"): 1.5e-03, ("dW", "bias"): 2.8e-04, ("dW", "fourier"): 3.0e-04, ("dW", "pe"): 3.4e-04, ("dW", "weight"): 3.0e-04, ("bwd_dW", "bias"): 3.8e-03, ("bwd_dW", "fourier"): 1.4e-03, ("bwd_dW", "pe"): 9.8e-04, ("bwd_dW", "weight"): 3.8e-04, ("dpe16", "row"): 5.2e-03, ("bwd_dpe16", "row"): 2.5e-03},
}


def run_emul(case, mode, bias="fp32", cos="packed", pe=None, perturb=0.0, faults=None, dpe_store=None, cos_bwd=None):
    """forward + fused loss / backward + plain backward of a case -> dict(y, sse, dW, dpe, bwd_dW, bwd_dpe); cos_bwd: the cosine
    form of the plain backward where it is another kernel instance than the fused loss / backward (default: the same)"""
    pe = case["pe"] if pe is None else pe
    kw = dict(mode=mode, bias=bias, cos=cos, perturb=perturb, faults=faults, dpe_store=dpe_store)
    a = siren_emul(case["dims"], case["xf"], pe, case["wv"], case["S"], target=case["y"], dy_scale=case["dy_scale"], **kw)
    b = siren_emul(case["dims"], case["xf"], pe, case["wv"], case["S"], dy=case["dy"], **dict(kw, cos=cos_bwd or cos))
    a["bwd_dW"], a["bwd_dpe"] = b["dW"], b["dpe"]
    return a


def block_errors(case, out, ref, suffix=""):
    """per-block errors of the outputs of one case: {(output + suffix, kind): [the errors of each block's elements]}

    A block is one row's y / dpe, one row's sse, or one row's share of one layer's bias gradient / weight gradient (layer 0: the
    Fourier and the pe rows separately).  Every block is divided by ITS OWN largest reference entry.  `suffix` names the dpe
    outputs of the variants that store dpe as bf16 ("16"): their last rounding is a bf16 one and they get limits of their own."""
    res = {}
    G = ref["y"].shape[0]

    def add(key, o, r):
        if r.numel() == 0:                                  # E = 0: no dpe, no pe rows in layer 0
            return
        e = ((o.to(F64) - r).abs() / (r.abs().max() + 1e-300)).reshape(-1)
        res.setdefault(key, []).append(e)

    for name in ("y", "sse", "dpe", "bwd_dpe"):
        if out.get(name) is None:
            continue
        if ref[name].numel() == 0:
            continue
        for g_ in range(G):
            add((name + (suffix if "dpe" in name else ""), "row"), out[name][g_].cpu(), ref[name][g_])
    for name in ("dW", "bwd_dW"):
        if out.get(name) is None:
            continue
        for kind, l, sl in blocks_of_dw(case["dims"], case["F"]):
            for g_ in range(G):
                add((name, kind), out[name][g_, sl].cpu(), ref[name][g_, sl])
    return res


def block_stats(errs):
    """{(output, kind, "max" | "med"): the worst over the blocks of a block's largest / median element error}

    The largest error of a block is set by the few elements behind an operand that crossed a rounding boundary (one activation
    moved by an ulp moves its pixel's y and dpe); the median is not, and is where arithmetic that differs in EVERY element shows."""
    out = {}
    for (name, kind), blocks in errs.items():
        out[(name, kind, "max")] = max(float(e.max()) for e in blocks)
        out[(name, kind, "med")] = max(float(e.median()) for e in blocks)
    return out


# ---- the fp32 families: yardstick and limits -------------------------------------------------------------------------------------
# The fp32 kernels (siren_mlp.hip, siren_mlp_generic.hip) round nowhere but in their fp32 arithmetic, so the evaluator they are held
# to is mode=None, and what a correct kernel differs by is fp32 rounding in ITS order of operations.  How large that is on a
# given input set is measured, not assumed: fp32_restatement below is the same MLP and its gradients in fp32 torch on the CPU, run
# as the case stands and once more with the hidden units of every layer and the pixels reversed (an exact permutation of the
# problem; the outputs are permuted back) -- two correct fp32 evaluations that differ only in summation order.  The yardstick of
# a key (output, block kind, "max" | "med") is the larger of the two runs' block_stats against the fp64 evaluator, the worst over
# the cases of a family and scale group (pooled: a bias block at C = 1 has one element, whose error can be 0 by chance); the
# limit is FP32_K times that, at least LIMIT_FLOOR.  Nothing here comes from a kernel.
LIMIT_FLOOR = 2.0 ** -20          # sixteen fp32 ulps of the block's largest entry (the floor of test_hip_siren_operand_exact.py)
FP32_K = 4.0                      # the kernel and the restatement make the same number of fp32 roundings in different orders, so
                                  # their error ratio scatters around 1 (the kernels' two-float range reduction is the more
                                  # accurate sine, which pushes it below); 4 leaves room for the scatter on blocks of few elements
FP32_CONDITION = {"init": 1e-4, "model": 1e-5}      # no limit of a scale group may exceed this share of a block's largest entry


def _reverse_hidden(dims, wv):
    """rows of layer vectors with the hidden units of every layer in reverse order (its own inverse; also maps a gradient back)"""
    out, G, nl = torch.empty_like(wv), wv.shape[0], len(dims) - 1
    for l, (lo, nin, nout) in enumerate(layer_slices(dims)):
        b, W = wv[:, lo:lo + nout], wv[:, lo + nout:lo + nout * (nin + 1)].reshape(G, nin, nout)
        if l > 0:
            W = W.flip(1)
        if l < nl - 1:
            W, b = W.flip(2), b.flip(1)
        out[:, lo:lo + nout] = b
        out[:, lo + nout:lo + nout * (nin + 1)] = W.reshape(G, -1)
    return out


def fp32_restatement(case, reverse=False):
    """the outputs of run_emul in fp32 torch with autograd, forward as test_hip_kernels._oracle_mlp (x @ W + b, sin(30 x));
    reverse: the hidden units of every layer and the pixels in reverse order, the outputs permuted back"""
    dims, S, f = case["dims"], case["S"], torch.float32
    xf, pe0, wv0, tgt, dy = (case[k].to(f) for k in ("xf", "pe", "wv", "y", "dy"))
    if reverse:
        xf, pe0, tgt, dy, wv0 = xf.flip(0), pe0.flip(1), tgt.flip(1), dy.flip(1), _reverse_hidden(dims, wv0)
    G, nl, out = pe0.shape[0], len(dims) - 1, {}
    for plain in (False, True):
        pe, wv = pe0.clone().requires_grad_(True), wv0.clone().requires_grad_(True)
        x = torch.cat([xf[None].expand(G, -1, -1), pe], -1)
        for l, (lo, nin, nout) in enumerate(layer_slices(dims)):
            x = x @ wv[:, lo + nout:lo + nout * (nin + 1)].reshape(G, nin, nout) + wv[:, lo:lo + nout].unsqueeze(1)
            if l != nl - 1:
                x = torch.sin(30.0 * x)
        if plain:
            x.backward(dy)
            out.update(bwd_dW=wv.grad, bwd_dpe=pe.grad)
        else:
            diff = x - tgt.repeat_interleave(S, 0)
            ((diff * diff).sum() * case["dy_scale"]).backward()
            out.update(y=x.detach(), sse=(diff.detach() ** 2).sum((1, 2)), dW=wv.grad, dpe=pe.grad)
    if reverse:
        out = {k: _reverse_hidden(dims, v) if "dW" in k else v if k == "sse" else v.flip(1) for k, v in out.items()}
    return out


_BUILT, _YARDSTICK = {}, {}


def fp32_cases(family):
    """[(c, its inputs, the fp64 evaluator's outputs)] of CASES_FP32[family], computed once and shared (leave them unchanged)"""
    if family not in _BUILT:
        built = [(c, build(c)) for c in CASES_FP32[family]]
        _BUILT[family] = [(c, case, run_emul(case, None)) for c, case in built]
    return _BUILT[family]


def fp32_yardstick(family):
    """{scale group: {key: the worst over the group's cases of the two restatement runs' block_stats against the fp64 evaluator}}"""
    if family not in _YARDSTICK:
        tab = {}
        for c, case, ref in fp32_cases(family):
            grp = tab.setdefault(c["scale"], {})
            for rev in (False, True):
                for k, v in block_stats(block_errors(case, fp32_restatement(case, rev), ref)).items():
                    grp[k] = max(grp.get(k, 0.0), v)
        _YARDSTICK[family] = tab
    return _YARDSTICK[family]


def fp32_limits(family):
    """{scale group: {key: max(FP32_K * yardstick, LIMIT_FLOOR)}}"""
    return {grp: {k: max(FP32_K * v, LIMIT_FLOOR) for k, v in tab.items()} for grp, tab in fp32_yardstick(family).items()}


def over_limits(stats, limits):
    """the entries of block_stats that exceed their limit (or are no number): [(key, value, limit)]"""
    return [(k, v, limits[k]) for k, v in stats.items() if not v <= limits[k]]
