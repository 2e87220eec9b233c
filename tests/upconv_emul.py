"""The arithmetic of the upsampling net's sub-pixel convolution kernels (recombiner_amd/csrc/upconv.hip, phaseconv.hip, stage1.hip
and their weight maps upconv_weff.hip / prepare_bodies.h, phase_weight.hip) in fp64, written from the definition of the stage

    nearest-upsample(f) -> conv(k, pad) (-> LeakyReLU 0.01)        (f, k, pad) = (2, 3, 1) and (4, 5, 2), 1 to 3 grid axes

on channel-last grids: explicit loops over the kernel taps on the up-sampled, zero-padded grid.  Plain torch, float64, nothing
from recombiner_amd: no indexing code is shared with what this judges.  Output pixel p of an axis has phase a = p mod f, and its
kernel tap kk reads up-sampled pixel p + kk - pad, i.e. source pixel floor((p + kk - pad) / f).  The kernels never build the
up-sampled grid: per phase they pre-sum the taps that land on one source pixel.  Here that shows only as a rounding point -- the
taps of such a group are replaced by (their rounded sum, 0, 0, ..) IN THE TAP LOOP -- and as the layouts `eff_layout` /
`big_layout`, which pick the sums out in the order the kernels store them.

Rounding points: the switches of `Rounding`, each named after the source line it mirrors.  With Rounding() nothing is rounded and
the evaluator is the plain stage (test_upconv_emul_cpu.py ties that to F.interpolate + F.conv{1,2,3}d and autograd).

  weff     pre-summed weight -> bf16; the sum in fp32, ascending tap order   weff_elem (phaseconv.hip), weff_of (prepare_bodies.h),
                                                                             bigweight_kernel (phase_weight.hip)
  x_in     fp32 stage input -> bf16                                          to_bf16x8 (stage1.hip)
  preact   stored pre-activation -> bf16                                     `(float)(__bf16)acc[..]` (s1_fwd1d_kernel); the bf16 z1
                                                                             that input mode 2 of upconv.hip reads is stored by its producer
  slope32  LeakyReLU / LeakyReLU' as ONE fp32 product by 0.01f               lrelu() on load (raw_frag<1>, <3>: then -> bf16) or in the
                                                                             epilogue; `o[k] * (x > 0.f ? 1.0f : SLOPE)` in the data gradients
  out      result -> "bf16" | "f32"                                          the epilogues' `(__bf16)` / fp32 stores
  dy       fp32 upstream gradient -> bf16                                    RCB_COMMITD (upconv_dgrad3_lds_kernel), raw_frag<2>
                                                                             (upconv_wgrad_kernel): the MFMA operand is bf16 in every mode

Two seeded input generators.  `lattice(case)`: small integers, on which every partial sum of every output is exactly representable
in fp32, so a kernel must return the fp64 result, rounded once, bit for bit, whatever its summation order -- the generator ASSERTS
the condition  sum |product| / lsb < 2^24  for every element of every output (lsb: the largest power of two dividing every
product).  `gridded(case)`: bf16 values at the scale of the existing tests with taps on a 2^-12 grid (every tap sum exact in fp32
in any order), for the a-priori bound  |got - ref| <= u_out (|ref| + g) + g,  g = n 2^-23 sum |x_i w_i|  per element, which
`evaluate` supplies per element (`S_*`: the sums of absolute products, `n_*`: the numbers of accumulated terms).
"""
import itertools
import math
from dataclasses import dataclass, replace
from types import SimpleNamespace

import torch

F64 = torch.float64
SLOPE = 0.01
SLOPE32 = float(torch.tensor(0.01, dtype=torch.float32))        # 0.01f
EXACT = 2.0 ** 24                                               # integers below it survive every fp32 addition
EPS32 = 2.0 ** -23                                              # one fp32 ulp of a value in [1, 2)
U_BF16 = 2.0 ** -8                                              # rounding to the nearest bf16 (8 significant bits): relative error


def bf16(x):
    """fp64 -> nearest bf16 (ties to even, gradual underflow), as fp64: ONE rounding (torch's cast from fp64 goes through fp32).
    The quantum is built from the exponent bits: exact on every device (no pow / ldexp of a library)"""
    x = x.to(F64).contiguous()
    e = ((x.view(torch.int64) >> 52) & 0x7FF) - 1023           # 2^e <= |x| < 2^(e + 1)  (zero: clamped below)
    q = ((torch.clamp(e, min=-126) - 7 + 1023) << 52).view(F64)
    return torch.round(x / q) * q                               # torch.round: half to even; x / q and r * q are exact


def f32(x):
    return x.to(torch.float32).to(F64)


@dataclass(frozen=True)
class Rounding:
    weff: bool = False
    x_in: bool = False
    preact: bool = False
    slope32: bool = False
    out: str = None            # forward result: None | "bf16" | "f32"
    dy: bool = False
    dx: str = None             # data-gradient result: None | "bf16" | "f32"


class Faults:
    """deliberately wrong evaluators, for the tests that the checks discriminate (never a property of a kernel)"""
    drop_corner_tap = False        # one of the 2^d pre-summed taps left out at the first corner pixel of the last datapoint
    halo_zero = False              # the left halo pixel of the last ragged 32-position tile (last axis) read as zero
    swap_phases = False            # the two phases of the last axis exchanged in the first 32-channel block
    no_bias_last = False           # the bias left off the last output channel
    slope_from_neighbour = False   # LeakyReLU' taken from the next pixel along the last axis
    last_is_copy = False           # the last datapoint evaluated as a copy of the one before it (forward)
    skip_batch_entry = False       # the last datapoint left out of the weight and bias gradient
    acc_bf16 = False               # accumulation carried in bf16 after every tap (forward)
    dy_switch_flipped = False      # the `dy` switch the other way round: the fp32 dy not rounded where the kernels round it

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Faults, k), k
            setattr(self, k, v)


@dataclass(frozen=True)
class Geo:
    f: int
    k: int
    pad: int
    nd: int

    def offsets(self):
        """[phase a][tap kk] -> source pixel relative to the output pixel's own: floor((a + kk - pad) / f)"""
        return [[math.floor((a + kk - self.pad) / self.f) for kk in range(self.k)] for a in range(self.f)]

    def phases(self):
        return list(itertools.product(range(self.f), repeat=self.nd))

    def taps(self):
        return list(itertools.product(range(self.k), repeat=self.nd))        # lexicographic = ascending tap order

    def groups(self, a):
        """{source offset per axis: [the kernel taps of phase `a` that read it], ascending}"""
        off, out = self.offsets(), {}
        for kk in self.taps():
            out.setdefault(tuple(off[a[d]][kk[d]] for d in range(self.nd)), []).append(kk)
        return out


def lrelu(v, slope32):
    return torch.where(v > 0, v, f32(v * SLOPE32) if slope32 else v * SLOPE)


def dlrelu(acc, sign_src, slope32):
    """acc * LeakyReLU'(sign_src): the slope wherever the stored value is not positive (`x > 0.f ? 1.0f : SLOPE`)"""
    return torch.where(sign_src > 0, acc, f32(acc * SLOPE32) if slope32 else acc * SLOPE)


def rounded(v, how):
    return v if how is None else (bf16(v) if how == "bf16" else f32(v))


# ---- the stage, tap by tap -----------------------------------------------------------------------------------------------------
def tap_weights(W, geo, presum=None):
    """conv weight [Co, Ci, *k] -> Wt [*phases, *taps, Co, Ci]: the weight kernel tap kk has at output pixels of phase a.
    presum None: W's tap, whatever the phase (the plain stage).  Otherwise the taps of a phase that read the same source pixel are
    replaced by (their sum, 0, 0, ..) -- the same stage unless the sum rounds: "f64" exact; "f32" summed in fp32 in ascending tap
    order (the fp32 effective weights of rcb_upconv_weff_build, rcb_phase_bigweight); "bf16": that sum rounded to bf16 (the MFMA
    operand).  True means "bf16"."""
    presum = "bf16" if presum is True else (presum or None)
    Co, Ci = W.shape[:2]
    Wt = torch.zeros([geo.f] * geo.nd + [geo.k] * geo.nd + [Co, Ci], dtype=F64, device=W.device)
    for a in geo.phases():
        if presum is None:
            for kk in geo.taps():
                Wt[a + kk] = W[(slice(None), slice(None)) + kk]
            continue
        for taps in geo.groups(a).values():
            s = torch.zeros(Co, Ci, dtype=F64 if presum == "f64" else torch.float32, device=W.device)
            for kk in taps:
                s = s + W[(slice(None), slice(None)) + kk].to(s.dtype)
            Wt[a + taps[0]] = bf16(s.to(F64)) if presum == "bf16" else s.to(F64)
    return Wt


def up_pad(x, geo):
    """x [B, *g, C] -> the nearest-upsampled grid with `pad` zero pixels around it"""
    for ax in range(geo.nd):
        x = x.repeat_interleave(geo.f, dim=1 + ax)
    return torch.nn.functional.pad(x, [0, 0] + [geo.pad, geo.pad] * geo.nd)


def _in_slice(a, kk, g, geo):
    """the padded up-sampled pixels that tap kk reads for the output pixels of phase a"""
    return (slice(None),) + tuple(slice(a[d] + kk[d], a[d] + kk[d] + geo.f * (g[d] - 1) + 1, geo.f) for d in range(geo.nd))


def _out_slice(a, geo):
    return (slice(None),) + tuple(slice(a[d], None, geo.f) for d in range(geo.nd))


def forward_acc(x, Wt, b, geo, acc_bf16=False, skip=None):
    """y[p] = b + sum_kk Wt[phase of p][kk] x_up[p + kk - pad]: [B, *g, Ci] -> [B, *(f g), Co], nothing rounded (`acc_bf16`: the
    fault).  `skip(a, kk)` -> a [B, *g] mask of output pixels at which that tap is left out (faults), or None."""
    g, xp = list(x.shape[1:-1]), up_pad(x, geo)
    y = torch.zeros([x.shape[0]] + [geo.f * v for v in g] + [Wt.shape[-2]], dtype=F64, device=x.device)
    for a in geo.phases():
        acc = b.to(F64).expand([x.shape[0]] + g + [Wt.shape[-2]]).clone()
        for kk in geo.taps():
            w = Wt[a + kk]
            if not bool(w.any()):
                continue
            term = xp[_in_slice(a, kk, g, geo)] @ w.t()
            if skip is not None:
                m = skip(a, kk)
                if m is not None:
                    term = torch.where(m.unsqueeze(-1), torch.zeros_like(term), term)
            acc = acc + term
            if acc_bf16:
                acc = bf16(acc)
        y[_out_slice(a, geo)] = acc
    return y


def dgrad_acc(dy, Wt, geo):
    """the adjoint of forward_acc in x: dy [B, *(f g), Co] -> [B, *g, Ci] (every up-sampled pixel hands its sum to its source)"""
    g = [v // geo.f for v in dy.shape[1:-1]]
    dxp = torch.zeros([dy.shape[0]] + [geo.f * v + 2 * geo.pad for v in g] + [Wt.shape[-1]], dtype=F64, device=dy.device)
    for a in geo.phases():
        d = dy[_out_slice(a, geo)]
        for kk in geo.taps():
            w = Wt[a + kk]
            if bool(w.any()):
                dxp[_in_slice(a, kk, g, geo)] += d @ w
    dxu = dxp[(slice(None),) + tuple(slice(geo.pad, geo.pad + geo.f * v) for v in g)]
    shape = [dy.shape[0]]
    for v in g:
        shape += [v, geo.f]
    return dxu.reshape(shape + [Wt.shape[-1]]).sum(dim=[2 + 2 * d for d in range(geo.nd)])


def wgrad_acc(x, dy, geo):
    """-> (dWp [*phases, *taps, Co, Ci]: the gradient of tap kk collected at the output pixels of phase a alone, db [Co]).
    The conv weight's gradient is the sum over the phases (conv_layout); the gradient of a pre-summed weight is the entry of any
    one tap of its group (they read the same source pixel): eff_layout / big_layout take the first."""
    g, xp = list(x.shape[1:-1]), up_pad(x, geo)
    Co, Ci = dy.shape[-1], x.shape[-1]
    dWp = torch.zeros([geo.f] * geo.nd + [geo.k] * geo.nd + [Co, Ci], dtype=F64, device=x.device)
    for a in geo.phases():
        d = dy[_out_slice(a, geo)].reshape(-1, Co)
        for kk in geo.taps():
            dWp[a + kk] = d.t() @ xp[_in_slice(a, kk, g, geo)].reshape(-1, Ci)
    return dWp, dy.reshape(-1, Co).sum(0)


# ---- the layouts of the kernels --------------------------------------------------------------------------------------------------
def conv_layout(T):
    """[*phases, *taps, Co, Ci] -> the conv weight's gradient [Co, Ci, *k]"""
    nd = (T.dim() - 2) // 2
    return T.sum(dim=list(range(nd))).permute(nd, nd + 1, *range(nd))


def eff_layout(T, geo):
    """[*phases, *taps, Co, Ci] -> the 2^d-tap form [*t, Ci, *a, Co] (t = 0, 1: the first and the second source pixel a phase reads
    on an axis); for two axes that is Weff[ty][tx][ci][a][b][co] of upconv.hip"""
    off = geo.offsets()
    lo = [min(o) for o in off]
    assert all(max(o) - l <= 1 for o, l in zip(off, lo)), "a phase reads more than two source pixels per axis"
    out = torch.zeros([2] * geo.nd + [T.shape[-1]] + [geo.f] * geo.nd + [T.shape[-2]], dtype=T.dtype, device=T.device)
    for a in geo.phases():
        for key, taps in geo.groups(a).items():
            t = tuple(key[d] - lo[a[d]] for d in range(geo.nd))
            out[t + (slice(None),) + a] = T[a + taps[0]].t()
    return out


def eff_grad_to_conv(dWeff, geo):
    """the gradient of the 2^d-tap weights [*t, Ci, *a, Co] -> the conv weight's gradient [Co, Ci, *k]: every kernel tap collects
    the gradient of the pre-summed weight it is part of, over all phases (rcb_upconv_weff_grad, pc_wgrad_fold_kernel)"""
    off = geo.offsets()
    lo = [min(o) for o in off]
    out = torch.zeros([dWeff.shape[-1], dWeff.shape[geo.nd]] + [geo.k] * geo.nd, dtype=dWeff.dtype, device=dWeff.device)
    for a in geo.phases():
        for key, taps in geo.groups(a).items():
            t = tuple(key[d] - lo[a[d]] for d in range(geo.nd))
            for kk in taps:
                out[(slice(None), slice(None)) + kk] += dWeff[t + (slice(None),) + a].t()
    return out


def big_layout(T, geo):
    """[*phases, *taps, Co, Ci] -> Wbig [3^d Ci, f^d Co] of rcb_phase_bigweight: rows (window offset -1 / 0 / +1 per axis,
    lexicographic; ci), columns (phases lexicographic; co); zero where a phase does not read a window pixel"""
    Co, Ci = T.shape[-2:]
    out = torch.zeros([3] * geo.nd + [Ci] + [geo.f] * geo.nd + [Co], dtype=T.dtype, device=T.device)
    for a in geo.phases():
        for key, taps in geo.groups(a).items():
            out[tuple(o + 1 for o in key) + (slice(None),) + a] = T[a + taps[0]].t()
    return out.reshape(3 ** geo.nd * Ci, geo.f ** geo.nd * Co)


def phase_forward(x, Weff, b, geo):
    """the stage in PHASE form from the 2^d-tap weights [*t, Ci, *a, Co] (only to show that eff_layout's weights reproduce the
    plain stage; nothing is judged against this)"""
    off, g = geo.offsets(), list(x.shape[1:-1])
    lo = [min(o) for o in off]
    halo = max(max(-l, 0) for l in lo) + 1
    xp = torch.nn.functional.pad(x, [0, 0] + [halo, halo] * geo.nd)
    y = torch.zeros([x.shape[0]] + [geo.f * v for v in g] + [Weff.shape[-1]], dtype=F64, device=x.device)
    for a in geo.phases():
        acc = b.to(F64).expand([x.shape[0]] + g + [Weff.shape[-1]]).clone()
        for t in itertools.product(range(2), repeat=geo.nd):
            sl = (slice(None),) + tuple(slice(halo + lo[a[d]] + t[d], halo + lo[a[d]] + t[d] + g[d]) for d in range(geo.nd))
            acc = acc + xp[sl] @ Weff[t + (slice(None),) + a]
        y[_out_slice(a, geo)] = acc
    return y


def dense_map(W, grid, geo):
    """the stage on a fixed small grid as one dense matrix [(source pixel, ci), (output pixel, co)] (stage 1 of the CIFAR net on
    its 2 x 2 latent grid: Weff1[s, t, i, y, x, o] of upconv_weff.hip), from the definition: the images of the unit inputs"""
    Ci, n = W.shape[1], int(math.prod(grid)) * W.shape[1]
    eye = torch.eye(n, dtype=F64, device=W.device).view([n] + list(grid) + [Ci])
    return forward_acc(eye, tap_weights(W, geo), torch.zeros(W.shape[0], dtype=F64, device=W.device), geo).reshape(n, -1)


def dense_map_grad(dM, w_shape, grid, geo):
    """the adjoint of dense_map: dM [(source pixel, ci), (output pixel, co)] -> dW [Co, Ci, *k]"""
    Co, Ci = w_shape[:2]
    n = int(math.prod(grid)) * Ci
    eye = torch.eye(n, dtype=F64, device=dM.device).view([n] + list(grid) + [Ci])
    return conv_layout(wgrad_acc(eye, dM.to(F64).view([n] + [geo.f * v for v in grid] + [Co]), geo)[0])


# ---- cases -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """one kernel configuration on one shape.  kernel: "phaseconv" | "stage1" | "upconv2" | "upconv3";  shape (B, *grid)
    x_mode  "act": bf16 activations (phaseconv, upconv3) | "pre_f32" / "pre_bf16": pre-activation, LeakyReLU on load (upconv2;
            modes 1 / 2 of rcb_upconv_*) | "f32": fp32 latent grid (stage1)
    leaky   LeakyReLU in the forward epilogue;  out: forward result;  dy: "bf16" | "f32";  dx: data-gradient result
    sign    "mixed" | "pos" (stage input positive: no slope on load or in LeakyReLU') | "nonneg" (the chains)"""
    kernel: str
    shape: tuple
    cout: int
    x_mode: str = "act"
    leaky: bool = False
    out: str = "bf16"
    dy: str = "bf16"
    dx: str = "bf16"
    sign: str = "mixed"
    amp: int = 4               # |activation|, |dy| <= amp on the lattice
    tap: int = 7               # |conv tap|, |bias| <= tap on the lattice
    seed: int = 0

    @property
    def geo(self):
        return Geo(4, 5, 2, 1) if self.kernel == "stage1" else Geo(2, 3, 1, len(self.shape) - 1)

    @property
    def cin(self):
        return 128 if self.kernel == "stage1" else 64

    @property
    def rounding(self):
        """where the kernel of this case rounds"""
        return Rounding(weff=True, x_in=self.x_mode == "f32", preact=self.kernel == "stage1", slope32=True, out=self.out,
                        dy=self.dy == "f32", dx=self.dx)

    @property
    def id(self):
        s = "%s-%s-c%d" % (self.kernel, "x".join(str(v) for v in self.shape), self.cout)
        if self.kernel.startswith("upconv"):
            s += "-x_%s-out_%s-dy_%s" % (self.x_mode, ("leaky_" if self.leaky else "linear_") + self.out, self.dy)
        elif self.kernel == "phaseconv":
            s += "-leaky" if self.leaky else "-linear"
        return s + ("" if self.sign == "mixed" else "-" + self.sign)


def phaseconv_case(shape, cout, **kw):
    return Case("phaseconv", tuple(shape), cout, leaky=cout == 64, **kw)


def stage1_case(B, g, **kw):
    return Case("stage1", (B, g), 64, x_mode="f32", leaky=True, dx="f32", **kw)


def upconv2_case(B, x_mode, **kw):
    """stage 2 of the CIFAR geometry: grid 8, 64 -> 64 channels, pre-activation input, LeakyReLU + bf16 out, dx in x's type"""
    return Case("upconv2", (B, 8, 8), 64, x_mode=x_mode, leaky=True, dx="f32" if x_mode == "pre_f32" else "bf16", **kw)


def upconv3_case(B, out, dy, **kw):
    """stage 3: grid 16, 64 -> 16 channels, bf16 activations in, linear fp32 or bf16 out, fp32 or bf16 dy"""
    return Case("upconv3", (B, 16, 16), 16, out=out, dy=dy, **kw)


def operand(case, x, R):
    """the stage input as the MFMA operand of the forward pass and of the weight gradient"""
    if case.x_mode == "f32":
        return bf16(x) if R.x_in else x
    if case.x_mode in ("pre_f32", "pre_bf16"):
        v = lrelu(x, R.slope32)
        return bf16(v) if R.slope32 else v                   # raw_frag<1> / <3>: lrelu in fp32, then the bf16 operand
    return x


def _skip_of(case, ft, g, dev):
    """the taps a forward fault leaves out: -> skip(a, kk) for forward_acc"""
    geo = case.geo
    if not (ft.drop_corner_tap or ft.halo_zero):
        return None
    off = geo.offsets()
    B = case.shape[0]
    ts = 32 * ((g[-1] - 1) // 32)                              # first source pixel of the last 32-position tile of the last axis

    def skip(a, kk):
        o = tuple(off[a[d]][kk[d]] for d in range(geo.nd))
        m = None
        if ft.drop_corner_tap and all(v == 0 for v in a) and all(v == 0 for v in o):
            m = torch.zeros([B] + g, dtype=torch.bool, device=dev)
            m[(B - 1,) + (0,) * geo.nd] = True                 # the corner pixel's own source pixel, datapoint B - 1
        if ft.halo_zero and o[-1] == -1 and ts > 0:
            m = torch.zeros([B] + g, dtype=torch.bool, device=dev) if m is None else m
            m[..., ts] = True                                  # source pixel ts - 1 is the tile's left halo
        return m
    return skip


def evaluate(case, inp, R=None, faults=None, want=("fwd", "dgrad", "wgrad")):
    """the kernels' results for the inputs `inp` (x, W, b, dy: fp64 tensors holding the values the kernels are given), rounded as
    `R` says (default: where the kernel of the case rounds), plus per element the sum of absolute products S_* and the number of
    accumulated terms n_* behind it.  -> namespace(y, dx, dW (the layout the kernel returns), db, dbx (upconv2: channel sums of dx))"""
    R = case.rounding if R is None else R
    ft = faults or Faults()
    geo, g = case.geo, list(case.shape[1:])
    x, W, b, dy = inp.x, inp.W, inp.b, inp.dy
    dev = x.device
    Wt = tap_weights(W, geo, "bf16" if R.weff else None)
    xop = operand(case, x, R)
    res = SimpleNamespace()
    one_w = (Wt != 0).to(F64).amax(dim=(-1, -2), keepdim=True).expand_as(Wt)        # 1 on the taps that are accumulated
    if "fwd" in want:
        skip = _skip_of(case, ft, g, dev)
        bb = b.clone()
        if ft.no_bias_last:
            bb[-1] = 0
        acc = forward_acc(xop, Wt, bb, geo, acc_bf16=ft.acc_bf16, skip=skip)
        if ft.swap_phases:
            blk = slice(0, min(32, case.cout))
            even, odd = acc[..., 0::2, blk].clone(), acc[..., 1::2, blk].clone()
            acc[..., 0::2, blk], acc[..., 1::2, blk] = odd, even
        if ft.last_is_copy:
            acc[-1] = acc[-2]
        v = bf16(acc) if R.preact else acc
        if case.leaky:
            v = lrelu(v, R.slope32)
        res.y = rounded(v, R.out)
        res.S_y = forward_acc(xop.abs(), Wt.abs(), b.abs(), geo)
        res.n_y = forward_acc(torch.ones_like(xop), one_w, torch.ones_like(b), geo) + 2      # + the bias, + the slope product
    dyr = R.dy != ft.dy_switch_flipped
    dyop = bf16(dy) if dyr else dy
    if "dgrad" in want:
        acc = dgrad_acc(dyop, Wt, geo)
        if case.kernel == "stage1":
            v = acc                                            # dz is the gradient of the pre-activation: no factor here
        else:
            src = x                                            # the STORED stage input: its sign is LeakyReLU'
            if ft.slope_from_neighbour:
                src = torch.roll(src, -1, dims=-2)
            v = dlrelu(acc, src, R.slope32)
        res.dx = rounded(v, R.dx)
        res.S_dx = dgrad_acc(dyop.abs(), Wt.abs(), geo)
        res.S_dx_out = res.S_dx if case.kernel == "stage1" else dlrelu(res.S_dx, x, R.slope32)     # at the scale of the result
        res.n_dx = dgrad_acc(torch.ones_like(dyop), one_w, geo) + 1                           # + the slope product
        if case.kernel == "upconv2":                            # per-channel sums of dx as stored (the bias gradient of stage 1)
            res.dbx = res.dx.reshape(-1, case.cin).sum(0)
            res.S_dbx = res.dx.abs().reshape(-1, case.cin).sum(0)
    if "wgrad" in want:
        xw, dw_ = xop, dyop
        if ft.skip_batch_entry:
            xw, dw_ = xop[:-1], dyop[:-1]
        dWp, res.db = wgrad_acc(xw, dw_, geo)
        Sp, res.S_db = wgrad_acc(xop.abs(), dyop.abs(), geo)
        n_pos = float(math.prod(g) * case.shape[0])
        lay = {"phaseconv": conv_layout, "stage1": lambda T: big_layout(T, geo)}.get(case.kernel, lambda T: eff_layout(T, geo))
        res.dW, res.S_dW = lay(dWp), lay(Sp)
        res.n_dW = n_pos * (geo.f ** geo.nd if case.kernel == "phaseconv" else 1)             # conv layout: every phase adds in
        res.n_db = n_pos * geo.f ** geo.nd
    return res


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _gen(case):
    return torch.Generator().manual_seed(1000 + case.seed + 7 * sum(case.shape) + case.cout)


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).to(F64)


def lsb_of(t):
    """the largest power of two (2^-40 .. 2^40) that divides every entry of t"""
    t = t.to(F64)
    lo, hi = -40, 40                                          # divisible by 2^lo (asserted), search the largest such exponent
    assert bool((torch.round(t * 2.0 ** 40) == t * 2.0 ** 40).all()), "finer than 2^-40"
    while lo < hi:
        mid = (lo + hi + 1) // 2
        s = t * 2.0 ** -mid
        if bool((torch.round(s) == s).all()):
            lo = mid
        else:
            hi = mid - 1
    return 2.0 ** lo


def lattice_inputs(case, device="cpu"):
    """seeded small integers: activations and dy in [-amp, amp], taps and biases in [-tap, tap].  sign "pos": the stage input in
    [1, amp], so that the LeakyReLU on load and the LeakyReLU' of the data gradient never apply the slope (a LeakyReLU in the
    EPILOGUE may: it acts on an exact sum, one fp32 product, deterministic); "nonneg" (the chains): everything >= 0, biases >= 1"""
    gen, geo = _gen(case), case.geo
    B, g = case.shape[0], list(case.shape[1:])
    a, t = case.amp, case.tap
    nn = case.sign == "nonneg"
    x = _ints(gen, [B] + g + [case.cin], {"pos": 1, "nonneg": 0}.get(case.sign, -a), a)
    W = _ints(gen, [case.cout, case.cin] + [geo.k] * geo.nd, 0 if nn else -t, t)
    b = _ints(gen, [case.cout], 1 if nn else -t, t)
    dy = _ints(gen, [B] + [geo.f * v for v in g] + [case.cout], 0 if nn else -a, a)
    return SimpleNamespace(x=x.to(device), W=W.to(device), b=b.to(device), dy=dy.to(device))


def assert_exact(name, S, *operands):
    """THE condition: with every product a multiple of lsb, an fp32 sum is exact in any order if sum |product| / lsb < 2^24"""
    lsb = 1.0
    for o in operands:
        lsb *= lsb_of(o)
    q = float(S.max()) / lsb
    assert q < EXACT, "%s: sum |product| / lsb = %.0f >= 2^24: the case is not exact in every summation order" % (name, q)
    return q


def lattice(case, device="cpu", want=("fwd", "dgrad", "wgrad")):
    """-> (inputs, expected results): lattice inputs and the fp64 results rounded where the kernel rounds, after ASSERTING for
    every element of every output that it is exact in any fp32 summation order"""
    inp = lattice_inputs(case, device)
    R = case.rounding
    ref = evaluate(case, inp, R, want=want)
    geo = case.geo
    Wt = tap_weights(inp.W, geo, "bf16")
    xop = operand(case, inp.x, R)
    dyop = bf16(inp.dy) if R.dy else inp.dy
    ref.q = {}
    if "fwd" in want:
        lsb_b = lsb_of(inp.b)
        assert lsb_b >= lsb_of(xop) * lsb_of(Wt) or not bool(inp.b.any())
        ref.q["y"] = assert_exact(case.id + " y", ref.S_y, xop, Wt)
    if "dgrad" in want:
        ref.q["dx"] = assert_exact(case.id + " dx", ref.S_dx, dyop, Wt)
        if case.kernel == "upconv2":
            if case.sign == "mixed":
                ref.dbx = None            # a dx under the slope is f32(sum * 0.01f): 24 significant bits, their sum is on no lattice
            else:
                ref.q["dbx"] = assert_exact(case.id + " dbx", ref.S_dbx, ref.dx)
    if "wgrad" in want:
        ref.q["dW"] = assert_exact(case.id + " dW", ref.S_dW, xop, dyop)
        ref.q["db"] = assert_exact(case.id + " db", ref.S_db, dyop)
    return inp, ref


def gridded_inputs(case, device="cpu"):
    """seeded values at the scale of test_hip_upsample.py: activations LeakyReLU(N(0, 1)) (pre-activations and latents N(0, 1) / 2),
    dy 0.1 N(0, 1), biases 0.1 N(0, 1); conv taps random multiples of 2^-12 with |tap| <= 2^-5 (the magnitude of 0.5 / sqrt(64 3^d)):
    every tap sum is exact in fp32 in any order, its rounding to bf16 real and deterministic.  Everything the kernels read as bf16
    is a bf16 value; an fp32 dy (case.dy == "f32") and an fp32 pre-activation keep their fp32 mantissas."""
    gen, geo = _gen(case), case.geo
    B, g = case.shape[0], list(case.shape[1:])
    n = lambda *s: torch.randn(*s, generator=gen, dtype=F64)       # noqa: E731
    x = n(B, *g, case.cin)
    if case.x_mode == "act":
        x = bf16(torch.where(x > 0, x, 0.01 * x))
    elif case.x_mode == "pre_bf16":
        x = bf16(x)
    else:
        x = f32(0.5 * x) if case.x_mode == "f32" else f32(x)
    W = torch.randint(-128, 129, tuple([case.cout, case.cin] + [geo.k] * geo.nd), generator=gen).to(F64) * 2.0 ** -12
    b = f32(0.1 * n(case.cout))
    dy = 0.1 * n(B, *[geo.f * v for v in g], case.cout)
    dy = f32(dy) if case.dy == "f32" else bf16(dy)
    return SimpleNamespace(x=x.to(device), W=W.to(device), b=b.to(device), dy=dy.to(device))


def gridded(case, device="cpu", faults=None, want=("fwd", "dgrad", "wgrad")):
    """-> (inputs, reference): the operands rounded where the kernel rounds them, the RESULTS left unrounded in fp64; with S_* / n_*
    for the bound of `bound`"""
    inp = gridded_inputs(case, device)
    return inp, evaluate(case, inp, replace(case.rounding, out=None, dx=None, preact=False), faults, want)


def bound(ref_v, S, n, out, roundings=1):
    """|got - ref| <= u_out (|ref| + g) + g,  g = n 2^-23 sum |x_i w_i|: n fp32 additions lose at most one ulp of a partial sum
    each (whether the hardware rounds or truncates; a partial sum is at most sum |x_i w_i| (1 + n 2^-23), absorbed by counting
    the bias and the slope product as terms of their own), and the result is rounded to the nearest bf16 once (u_out = 2^-8) or not
    at all (fp32: u_out = 0).  `roundings` (a number or a tensor like ref_v): where the kernel's DEFINITION rounds a result to
    bf16 twice on its way -- stage 1 stores LeakyReLU(bf16(z)) as bf16: two roundings where the slope applies, one where it
    does not (a bf16 value is its own rounding); rcb_tile_fold adds bf16 tile sums and rounds again -- u_out is 2^-8 per
    rounding; the second-order term 2^-16 |ref| is below g (g >= 64 * 2^-23 |ref| for every kernel here)."""
    g = n * EPS32 * S
    u = (U_BF16 if out == "bf16" else 0.0) * roundings
    return u * (ref_v.abs() + g) + g


def first_difference(got, ref, case, what):
    """a readable location of the first differing element: (batch, position per axis, phase per axis, channel)"""
    ne = (got.to(F64) != ref).nonzero()
    if ne.numel() == 0:
        return None
    idx = [int(v) for v in ne[0]]
    f = case.geo.f
    if what == "y":
        return "%d of %d differ; first at batch %d position %s phase %s channel %d: got %r, expected %r" % (
            ne.shape[0], ref.numel(), idx[0], [v // f for v in idx[1:-1]], [v % f for v in idx[1:-1]], idx[-1],
            float(got[tuple(idx)]), float(ref[tuple(idx)]))
    return "%d of %d differ; first at index %s of %s: got %r, expected %r" % (ne.shape[0], ref.numel(), idx, what,
                                                                             float(got[tuple(idx)]), float(ref[tuple(idx)]))


# ---- the cases of test_hip_upconv_exact.py (test_upconv_emul_cpu.py asserts the lattice condition for each of them) -------------
PHASECONV_SHAPES = [(3, 70), (2, 33), (1, 1), (2, 31), (2, 600),                    # 1-D; (2, 600): a workgroup walks several tile groups
                    (2, 5, 33), (1, 1, 1), (3, 9, 70),                              # 2-D
                    (2, 3, 4, 40), (1, 2, 3, 32), (1, 1, 1, 1)]                     # 3-D
PHASECONV_CASES = [phaseconv_case(s, c, seed=i) for i, s in enumerate(PHASECONV_SHAPES) for c in (64, 16)]
STAGE1_CASES = [stage1_case(B, g, seed=20 + i) for i, (B, g) in enumerate([(3, 70), (2, 33), (5, 6), (1, 1)])]
# stage 2 reads a PRE-activation: a negative one becomes bf16(x * 0.01f) on load, which is on no integer lattice, so the batches
# run on positive inputs (taps, biases and dy of either sign) ...
UPCONV2_CASES = [upconv2_case(B, m, sign="pos", seed=30 + B % 7) for m in ("pre_f32", "pre_bf16") for B in (1, 3, 5, 257, 261)]
# ... and the slope on small operands: x in [-2, 2] and taps in [-1, 1] keep sum |product| / lsb below 2^24 (asserted like everywhere)
UPCONV2_SLOPE_CASES = [upconv2_case(B, m, sign="mixed", amp=2, tap=1, seed=45 + B) for m in ("pre_f32", "pre_bf16") for B in (3, 5)]
UPCONV2_FWD_ONLY = [upconv2_case(1027, m, sign="pos", seed=40) for m in ("pre_f32", "pre_bf16")]        # the forward's second trip
UPCONV3_CASES = [upconv3_case(B, o, d, seed=50 + B % 7) for o, d in (("f32", "f32"), ("bf16", "bf16")) for B in (1, 3, 5, 257, 261)]
HALF_WG_CASE = upconv3_case(769, "f32", "f32", seed=60)


# ---- the chains: stage 2 -> stage 3 of the CIFAR geometry and of the stitched 2-D path ------------------------------------------
@dataclass(frozen=True)
class ChainCase:
    """z1 [n, H, W, 64] (bf16 pre-activation of stage 1) -> h2 = bf16(LeakyReLU(stage 2)) -> pe (stage 3, linear, bf16 or fp32), and
    the backward from dpe.  Non-negative lattice data (weights, biases, inputs, dpe >= 0, biases >= 1): every pre-activation is
    positive and LeakyReLU the identity.  The taps are sparse 0 / 1 so that the intermediate images stay small: h2 and dz2 are the
    deterministic bf16 rounding of an exact sum, and the exactness condition is asserted for the second stage's sums like for the
    first's."""
    n: int
    H: int
    W: int
    pe: str = "bf16"           # stage-3 result and dpe: "bf16" | "f32"
    z1: str = "pre_bf16"       # stage-2 input mode
    tap_p: float = 0.25        # probability of a non-zero tap
    seed: int = 0

    @property
    def id(self):
        return "chain23-%dx%dx%d-z1_%s-pe_%s" % (self.n, self.H, self.W, self.z1, self.pe)


def chain_inputs(cc, device="cpu"):
    gen = torch.Generator().manual_seed(500 + cc.seed + cc.n + 3 * cc.H + 5 * cc.W)
    sparse = lambda *s: (torch.rand(*s, generator=gen) < cc.tap_p).to(F64)       # noqa: E731
    z1 = _ints(gen, [cc.n, cc.H, cc.W, 64], 1, 2)                # > 0: LeakyReLU' is 1 everywhere
    W2, W3 = sparse(64, 64, 3, 3), sparse(16, 64, 3, 3)
    b2, b3 = _ints(gen, [64], 1, 2), _ints(gen, [16], 1, 2)
    dpe = sparse(cc.n, 4 * cc.H, 4 * cc.W, 16)
    return SimpleNamespace(**{k: v.to(device) for k, v in dict(z1=z1, W2=W2, b2=b2, W3=W3, b3=b3, dpe=dpe).items()})


def chain23(cc, inp, exact=True):
    """-> namespace(h2, pe, dz2, dW3, db3, dz1, dbx, dW2, db2) on the WHOLE grid (dW2 / dW3 in the Weff layout), S_dz1 / n_dz1 for
    the bound; with `exact` the condition of `assert_exact` is asserted for every sum of both stages"""
    c2 = Case("upconv2", (cc.n, cc.H, cc.W), 64, x_mode=cc.z1, leaky=True, dx="f32" if cc.z1 == "pre_f32" else "bf16", sign="nonneg")
    c3 = Case("upconv3", (cc.n, 2 * cc.H, 2 * cc.W), 16, out=cc.pe, dy=cc.pe, sign="nonneg")
    i2 = SimpleNamespace(x=inp.z1, W=inp.W2, b=inp.b2, dy=None)
    f2 = evaluate(c2, SimpleNamespace(x=inp.z1, W=inp.W2, b=inp.b2, dy=torch.zeros(1, dtype=F64, device=inp.z1.device)), want=("fwd",))
    r3 = evaluate(c3, SimpleNamespace(x=f2.y, W=inp.W3, b=inp.b3, dy=inp.dpe))
    i2.dy = r3.dx
    r2 = evaluate(c2, i2, want=("dgrad", "wgrad"))
    if exact:
        Wt2, Wt3 = tap_weights(inp.W2, c2.geo, "bf16"), tap_weights(inp.W3, c3.geo, "bf16")
        assert bool((f2.y > 0).all()) and bool((inp.z1 > 0).all()), "the chains run on positive pre-activations"
        assert_exact(cc.id + " h2", f2.S_y, inp.z1, Wt2)
        assert_exact(cc.id + " pe", r3.S_y, f2.y, Wt3)
        assert_exact(cc.id + " dz2", r3.S_dx, inp.dpe, Wt3)
        assert_exact(cc.id + " dW3", r3.S_dW, f2.y, inp.dpe)
        assert_exact(cc.id + " db3", r3.S_db, inp.dpe)
        assert_exact(cc.id + " dz1", r2.S_dx, r3.dx, Wt2)
        assert_exact(cc.id + " dW2", r2.S_dW, inp.z1, r3.dx)
        assert_exact(cc.id + " db2", r2.S_db, r3.dx)
        assert_exact(cc.id + " dbx", r2.S_dbx, r2.dx)
    return SimpleNamespace(h2=f2.y, pe=r3.y, dz2=r3.dx, dW3=r3.dW, db3=r3.db, dz1=r2.dx, dbx=r2.dbx, dW2=r2.dW, db2=r2.db,
                           S_dz1=r2.S_dx, n_dz1=r2.n_dx, S_dz2=r3.S_dx)


CIFAR_CHAINS = [ChainCase(5, 8, 8, pe="bf16", z1="pre_bf16", seed=1), ChainCase(3, 8, 8, pe="f32", z1="pre_f32", seed=2)]
# the stitched 2-D path: latent grids (5, 7) and (8, 12), i.e. stage-1 images of 20 x 28 and 32 x 48 pixels
STITCHED_CHAINS = [ChainCase(2, 20, 28, seed=3), ChainCase(1, 32, 48, seed=4)]


# ---- the faults the checks must see (test_upconv_emul_cpu.py: each changes its case's output; test_hip_upconv_exact.py: each fails
# against the kernels).  (name, case, Faults arguments, the output it shows in, the whole-tensor limit of the matching test of
# test_hip_upsample.py, "lattice" | "gridded") ------------------------------------------------------------------------------------
def _pc(shape, cout):
    return next(c for c in PHASECONV_CASES if c.shape == tuple(shape) and c.cout == cout)


DISCRIMINATION = [
    ("one tap dropped at a corner pixel of one datapoint", _pc((2, 3, 4, 40), 64), dict(drop_corner_tap=True), "y", 6e-3, "lattice"),
    ("one tap dropped at a corner pixel (stage 2 of the CIFAR net)", UPCONV2_CASES[1], dict(drop_corner_tap=True), "y", 1e-2, "lattice"),
    ("halo of the last ragged tile read as zero (phaseconv 1-D)", _pc((3, 70), 64), dict(halo_zero=True), "y", 6e-3, "lattice"),
    ("halo of the last ragged tile read as zero (phaseconv 3-D)", _pc((2, 3, 4, 40), 16), dict(halo_zero=True), "y", 6e-3, "lattice"),
    ("halo of the last ragged tile read as zero (stage 1, 1-D)", STAGE1_CASES[0], dict(halo_zero=True), "y", 8e-3, "lattice"),
    ("two phases of one axis exchanged for one 32-channel block", _pc((2, 5, 33), 64), dict(swap_phases=True), "y", 6e-3, "lattice"),
    ("bias left off the last output channel", _pc((2, 33), 16), dict(no_bias_last=True), "y", 6e-3, "lattice"),
    ("bias left off the last output channel (stage 3 of the CIFAR net)", UPCONV3_CASES[1], dict(no_bias_last=True), "y", 1e-2, "lattice"),
    ("LeakyReLU' taken from the neighbouring pixel", _pc((3, 9, 70), 64), dict(slope_from_neighbour=True), "dx", 8e-3, "lattice"),
    ("LeakyReLU' taken from the neighbouring pixel (stage 2)", UPCONV2_SLOPE_CASES[0], dict(slope_from_neighbour=True), "dx", 1e-2, "lattice"),
    ("last datapoint of a batch with B % 4 == 3 a copy of the one before", UPCONV2_CASES[1], dict(last_is_copy=True), "y", 1e-2, "lattice"),
    ("one batch entry left out of the weight gradient (phaseconv)", _pc((3, 70), 64), dict(skip_batch_entry=True), "dW", 2e-3, "lattice"),
    ("one batch entry left out of the weight gradient (stage 1)", STAGE1_CASES[0], dict(skip_batch_entry=True), "dW", 2e-3, "lattice"),
    ("one batch entry left out of the weight gradient (stage 3, B = 257)", UPCONV3_CASES[3], dict(skip_batch_entry=True), "dW", 2e-3, "lattice"),
    ("accumulation carried in bf16 after every tap (phaseconv 3-D)", _pc((2, 3, 4, 40), 64), dict(acc_bf16=True), "y", 6e-3, "gridded"),
    ("accumulation carried in bf16 after every tap (stage 3, fp32 out)", UPCONV3_CASES[1], dict(acc_bf16=True), "y", 6e-3, "gridded"),
    ("the bf16 rounding of an fp32 dy on the wrong side of the mode switch", UPCONV3_CASES[1], dict(dy_switch_flipped=True), "dW", 2e-3, "gridded"),
]
