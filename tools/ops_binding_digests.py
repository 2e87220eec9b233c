"""SHA-256 of what the ops.py wrappers with more than one launch path return, on seeded inputs at the smallest shapes that reach
every path: run it in two trees that load the same built library and compare the output line by line (a refactor of the
binding must not move a bit).

  python tools/ops_binding_digests.py [--tree DIR]      DIR: the tree whose recombiner_amd is imported (default: this one);
                                                        RCB_LIB names the library when DIR has none of its own

A case the library refuses prints its error text instead of a digest; the two trees must agree on that line too."""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from recombiner_amd import ops  # noqa: E402

DEV = "cuda"
bf16 = torch.bfloat16


def sha(t):
    if t is None:
        return "None"
    if isinstance(t, ops.Planes):
        return "planes(" + sha(t.hi) + "," + sha(t.lo) + ")"
    if isinstance(t, (list, tuple)):
        return "[" + ",".join(sha(v) for v in t) + "]"
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:24]


def case(name, fn):
    try:
        out = fn()
        torch.cuda.synchronize()
        line = " ".join(sha(t) for t in (out if isinstance(out, (tuple, list)) else (out,)))
    except ops.RcbError as e:
        line = "refused: " + str(e).replace(ops._lib.LIB_PATH, "<lib>")
    print(f"{name:58s} {line}", flush=True)


def rnd(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV)


# ---- siren_loss_bwd / siren_bwd: width 32, F = E = 16, C = 3, 4 rows of 64 pixels ------------------------------------------
def siren_inputs(n_hidden, precision, layout):
    gen = torch.Generator().manual_seed(100 + n_hidden)
    meta = ops.SirenMeta(1, 64, 16, 16, n_hidden, 32, 3, precision=precision)
    xf = (torch.rand(64, 16, generator=gen) * 2 - 1).to(DEV)
    pe = rnd(gen, 4, 64, 16, scale=0.5)
    wv = ((torch.rand(4, meta.d_net, generator=gen) * 2 - 1) * (np.sqrt(6 / 32) / 30) * 3.0).to(DEV)
    y = torch.rand(4, 64, 3, generator=gen).to(DEV)
    dy = rnd(gen, 4, 64, 3, scale=1e-3)
    lay = None
    if precision:
        pe = pe.to(bf16)
    if layout:                                    # the same values seen as one stitched 16 x 16 grid of 2 x 2 patches of 8 x 8
        lay = ops.PeLayout((2, 2), (8, 8))
        pe = pe.view(2, 2, 1, 8, 8, 16).permute(2, 0, 3, 1, 4, 5).reshape(1, 16, 16, 16).contiguous()
    return meta, xf, pe, wv, y, dy, lay


for n_hidden in (2, 3):
    for layout in (False, True):
        meta, xf, pe, wv, y, dy, lay = siren_inputs(n_hidden, 1, layout)
        for chunks in (1, 2):
            for form, kw in (("fp32", {}), ("bf16", dict(want_bf16=True)), ("planes", dict(want_planes=True))):
                case(f"siren_loss_bwd h{n_hidden} p1 layout{int(layout)} chunks{chunks} {form}",
                     lambda: ops.siren_loss_bwd(xf, pe, wv, y, 1.0 / 192, meta, pixel_chunks=chunks, pe_layout=lay, **kw))
            case(f"siren_loss_bwd h{n_hidden} p1 layout{int(layout)} chunks{chunks} no dpe",
                 lambda: ops.siren_loss_bwd(xf, pe, wv, y, 1.0 / 192, meta, want_dpe=False, pixel_chunks=chunks, pe_layout=lay))
            if not layout:
                case(f"siren_bwd      h{n_hidden} p1 chunks{chunks}", lambda: ops.siren_bwd(xf, pe, wv, dy, meta, pixel_chunks=chunks))
    meta, xf, pe, wv, y, dy, _ = siren_inputs(n_hidden, 0, False)
    case(f"siren_loss_bwd h{n_hidden} p0 fp32", lambda: ops.siren_loss_bwd(xf, pe, wv, y, 1.0 / 192, meta))
    case(f"siren_bwd      h{n_hidden} p0", lambda: ops.siren_bwd(xf, pe, wv, dy, meta))

meta, xf, pe, wv, y, dy, _ = siren_inputs(3, 1, False)
probe = torch.zeros(256, 4, device=DEV, dtype=torch.int64)
case("siren_loss_bwd h3 p1 fp32 with clock_probe", lambda: ops.siren_loss_bwd(xf, pe, wv, y, 1.0 / 192, meta, clock_probe=probe))
print(f"{'  clock_probe written':58s} {bool(probe.any())}")

# ---- reparam_rng: an 8 x 520 level in its three buffer forms ----------------------------------------------------------------
gen = torch.Generator().manual_seed(7)
lv = ops.LevelSpec(rnd(gen, 8, 520, scale=0.05), rnd(gen, 8, 520, scale=0.3) - 4.0, 520, 8)
step = torch.tensor([41], device=DEV, dtype=torch.int64)
seed = 0x1234567890ABCDEF
case("reparam_rng fp32", lambda: ops.reparam_rng(lv, seed, 3, step))
case("reparam_rng fp32 + bf16 copy", lambda: ops.reparam_rng(lv, seed, 3, step, want_bf16=True))
case("reparam_rng bf16 buffers, copy not asked for", lambda: ops.reparam_rng(lv, seed, 3, step, buffers=ops.sample_buffers(lv, True)))
case("reparam_rng planes", lambda: ops.reparam_rng(lv, seed, 3, step, buffers=ops.sample_buffers(lv, planes=True)))
case("reparam_rng planes, no eps, group offset", lambda: ops.reparam_rng(
    lv, -5, 3, step, buffers=ops.sample_buffers(lv, planes=True, want_eps=False), group_offset=ops.rng_group_offset(2, 520)))
case("philox_normal", lambda: ops.philox_normal(4160, seed, 3, step, device=DEV))

# ---- step_prepare / upconv_weff_build: the one geometry they have ----------------------------------------------------------
gen = torch.Generator().manual_seed(11)
sizes = [1056, 1056, 1056, 99]
slices = [(sum(sizes[:i]), sum(sizes[:i + 1])) for i in range(len(sizes))]
A = [rnd(gen, n, n, scale=0.03) for n in sizes]
W1, b1 = rnd(gen, 64, 128, 5, 5, scale=0.05), rnd(gen, 64)
W2, W3 = rnd(gen, 64, 64, 3, 3, scale=0.05), rnd(gen, 16, 64, 3, 3, scale=0.05)
tab = ops.adam_table(2e-4, 16).to(DEV)


def written(w):
    """(Weff1, b1rep, Weff2, Weff3, the written ranges of the fragment pack: 16-byte entries [18432, 20480) are unused)"""
    return (*w[:4], w[4][:18432 * 16], w[4][20480 * 16:])


def prepare(bf16_out):
    tr = ops.ATransform(slices, DEV, 2)
    dyn = torch.full((2,), -1.0, device=DEV)
    slots = torch.arange(1024, device=DEV, dtype=torch.int64) + 3
    w = ops.step_prepare(tab, torch.tensor([5], device=DEV, dtype=torch.int64), dyn, slots, tr, A, W1, b1, W2, W3, bf16_out)
    return (*written(w), tr.packed, dyn, slots)


for bf16_out in (False, True):
    case(f"upconv_weff_build bf16_out={bf16_out}", lambda: written(ops.upconv_weff_build(W1, b1, W2, W3, bf16_out)))
    case(f"step_prepare      bf16_out={bf16_out}", lambda: prepare(bf16_out))


def begin():
    dyn, slots = torch.full((2,), -1.0, device=DEV), torch.arange(1024, device=DEV, dtype=torch.int64) + 3
    ops.step_begin(tab, torch.tensor([40], device=DEV, dtype=torch.int64), dyn, slots)
    return dyn, slots


def end(kl_log):
    stp, ctr = torch.tensor([2], device=DEV, dtype=torch.int64), torch.tensor([9], device=DEV, dtype=torch.int64)
    mse_log = torch.zeros(8, device=DEV, dtype=torch.float64)
    ops.step_end(stp, rnd(torch.Generator().manual_seed(3), 37).abs(), 0.25, torch.arange(1024, device=DEV, dtype=torch.int64), mse_log,
                 kl_log, ctr)
    return stp, ctr, mse_log, kl_log


case("step_begin", begin)
case("step_end", lambda: end(torch.zeros(6, device=DEV, dtype=torch.float64)))
case("step_end without a KL log", lambda: end(None))

# ---- upconv_wgrad / upconv_bwd_fused: stage-3 geometry, batch 2 -------------------------------------------------------------
gen = torch.Generator().manual_seed(9)
weff3 = rnd(gen, 2, 2, 64, 2, 2, 16, scale=0.05)
h2, dpe = rnd(gen, 2, 16, 16, 64).to(bf16), rnd(gen, 2, 32, 32, 16).to(bf16)
case("upconv_wgrad", lambda: ops.upconv_wgrad(h2, dpe, 16, 16))
case("upconv_bwd_fused", lambda: ops.upconv_bwd_fused(dpe, weff3, h2, 16, 16))

# ---- rec_score + rec_commit: 4 jobs, group lengths 1 to 3, 64 candidates ----------------------------------------------------
gen = torch.Generator().manual_seed(5)
K, rows, cols = 64, 4, 16
tabs = ops.RecTables(DEV, K)
for gl in (1, 2, 3):
    tabs.add(gl, torch.randn(K, gl, generator=gen).double())
gum = (-torch.log(-torch.log(torch.rand(K, generator=gen, dtype=torch.float64)))).to(DEV)
pl, ps = rnd(gen, cols, scale=0.01), (0.015 + 0.01 * torch.rand(cols, generator=gen)).to(DEV)
loc = pl[None] + ps[None] * 1.5 * rnd(gen, rows, cols)
scale = ps[None] * 0.5 * (0.5 + torch.rand(rows, cols, generator=gen).to(DEV))
jobs, _ = ops.RecJobs.from_host(DEV, [0, 1, 2, 3], [0, 5, 9, 13], [1, 2, 3, 3], group=[0, 1, 2, 3], rows=rows, cols=cols)


def rec(mode):
    idx, best, unc, logw0 = ops.rec_score(loc, scale, pl, ps, tabs, gum, jobs, mode, want_logw0=True)
    state = dict(enc_sample=torch.zeros(rows, cols, device=DEV), enc_mask=torch.zeros(rows, cols, device=DEV),
                 done=torch.zeros(rows, 4, device=DEV, dtype=torch.uint8), beta=torch.ones(rows, 4, device=DEV),
                 idx_groupwise=torch.full((rows, 4), -1, device=DEV, dtype=torch.int32))
    z = ops.rec_commit(pl, ps, tabs, jobs, idx, n_groups=4, want_z=True, **state)
    return (idx, best, unc, logw0, z, *state.values())


case("rec_score exact + rec_commit", lambda: rec(ops.REC_EXACT))
case("rec_score fast + rec_commit", lambda: rec(ops.REC_FAST))
case("rec_score_argmax (commit without state tensors)",
     lambda: ops.rec_score_argmax(loc, scale, pl, ps, tabs, gum, [0, 1, 2, 3], [0, 5, 9, 13], [1, 2, 3, 3]))

# ---- N4, whole-signal I/O: signal_patch* / recon_finish* ---------------------------------------------------------------------
# layouts of 1 to 3 axes at C = 3; a run R = patch_size[last] * C that is a multiple of 4 (the quad path) and one that is not (the
# element path); one signal of 2 x 2 patches of 32 x 32 x 3 = 12 288 elements, two chunks: the reduce kernel adds two partials
from recombiner_amd.utils import SampleFormat  # noqa: E402

N4_LAYOUTS = [("1d quad", (3,), (4,)), ("1d elem", (3,), (5,)), ("2d quad", (2, 2), (4, 4)), ("2d elem", (2, 2), (4, 3)),
              ("3d quad", (2, 1, 2), (2, 3, 4)), ("2d two chunks", (2, 2), (32, 32))]
N4_FORMATS = [("u8", SampleFormat.u8()), ("f32", SampleFormat.f32()), ("u16_12", SampleFormat.u16(12)), ("s16", SampleFormat.s16())]


def n4_signal(rng, shape, fmt):
    if fmt.kind == SampleFormat.F32:
        return torch.from_numpy(rng.rand(*shape).astype(np.float32)).to(DEV)
    if fmt.kind == SampleFormat.U8:
        return torch.from_numpy(rng.randint(0, 256, size=shape).astype(np.uint8)).to(DEV)
    if fmt.kind == SampleFormat.U16:
        return torch.from_numpy(rng.randint(0, 1 << fmt.depth, size=shape).astype(np.uint16)).to(DEV)
    return torch.from_numpy(rng.randint(-32768, 32768, size=shape).astype(np.int16)).to(DEV)


def n4_recon(rng, y):
    """a reconstruction near the targets y, a little outside [0, 1] here and there"""
    return (y * 1.02 - 0.01 + torch.from_numpy(rng.randn(*y.shape).astype(np.float32) * 0.01).to(DEV)).contiguous()


for lname, pn, ps in N4_LAYOUTS:
    lay = ops.PeLayout(pn, ps)
    grid = tuple(a * b for a, b in zip(pn, ps))
    n = 1 if lname == "2d two chunks" else 2
    for fname, fmt in N4_FORMATS:
        rng = np.random.RandomState(len(lname) * 7 + fmt.kind)
        sig = n4_signal(rng, (n, *grid, 3), fmt)
        y = ops.signal_patch(sig, lay, sample_format=fmt)
        rec = n4_recon(rng, y)
        case(f"signal_patch {lname} {fname}", lambda: y)
        if fmt.kind in (SampleFormat.U8, SampleFormat.F32):
            case(f"signal_patch {lname} {fname} by dtype", lambda: ops.signal_patch(sig, lay))
        case(f"recon_finish {lname} {fname}",
             lambda: ops.recon_finish(rec, y, layout=lay, sample_format=fmt, want_int=fmt.is_integer, want_whole=True))

lay = ops.PeLayout((2, 2), (4, 4))
for fname, fmt in N4_FORMATS:
    rng = np.random.RandomState(40 + fmt.kind)
    cf = n4_signal(rng, (2, 3, 8, 8), fmt)                     # channel-first storage
    big = n4_signal(rng, (3, 11, 13, 3), fmt)                  # a window at an offset of a larger signal
    small = n4_signal(rng, (2, 5, 7, 3), fmt)                  # below the grid on every axis
    small_cf = n4_signal(rng, (2, 3, 5, 7), fmt)
    case(f"signal_patch channel-first {fname}", lambda: ops.signal_patch(cf.movedim(1, -1), lay, sample_format=fmt))
    case(f"signal_patch offset view {fname}", lambda: ops.signal_patch(big[1:, 2:10, 3:11], lay, sample_format=fmt))
    out = torch.empty(8, 16, 3, device=DEV)
    case(f"signal_patch_pad 5x7 {fname} into out", lambda: ops.signal_patch_pad(small, lay, out=out, sample_format=fmt))
    case(f"signal_patch_pad 5x7 channel-first {fname}",
         lambda: ops.signal_patch_pad(small_cf.movedim(1, -1), lay, sample_format=fmt))
    if fmt.kind in (SampleFormat.U8, SampleFormat.F32):
        case(f"signal_patch_pad 5x7 {fname} by dtype", lambda: ops.signal_patch_pad(small, lay))
    y = ops.signal_patch_pad(small, lay, sample_format=fmt)
    rec = n4_recon(rng, y)
    case(f"recon_finish size 5x7 {fname}",
         lambda: ops.recon_finish(rec, y, layout=lay, size=(5, 7), sample_format=fmt, want_int=fmt.is_integer, want_whole=True))
    case(f"recon_finish size 5x7 {fname} no target", lambda: ops.recon_finish(rec, layout=lay, size=(5, 7), sample_format=fmt,
                                                                                want_whole=True))
    case(f"recon_finish size 8x4 {fname} scores only", lambda: ops.recon_finish(rec, y, layout=lay, size=(8, 4), sample_format=fmt))

rng = np.random.RandomState(50)
y = torch.from_numpy(rng.rand(8, 16, 3).astype(np.float32)).to(DEV)
rec = n4_recon(rng, y)
for mname, mode in (("8bit", ops.RECON_8BIT), ("raw", ops.RECON_RAW)):
    u8 = mode == ops.RECON_8BIT
    case(f"recon_finish {mname} by mode", lambda: ops.recon_finish(rec, y, layout=lay, mode=mode, want_u8=u8, want_whole=True))
    case(f"recon_finish {mname} by mode, size 5x7",
         lambda: ops.recon_finish(rec, y, layout=lay, mode=mode, want_u8=u8, want_whole=True, size=(5, 7)))
    case(f"recon_finish {mname} by mode, no layout", lambda: ops.recon_finish(rec, y, mode=mode, want_u8=u8, want_whole=True))
    case(f"recon_finish {mname} by mode, no target, no outputs", lambda: ops.recon_finish(rec, layout=lay, mode=mode))


def recon_into_out(size, fmt):
    shape = (2, *(size or (8, 8)), 3)
    q = torch.zeros(shape, device=DEV, dtype=torch.uint8 if fmt.dtype == torch.uint8 else torch.int16).view(fmt.dtype)
    out = (q, torch.zeros(shape, device=DEV), None,
           torch.zeros(2, device=DEV, dtype=torch.int32))
    got = ops.recon_finish(rec, y, layout=lay, size=size, sample_format=fmt, out=out)
    return (*got, got[0] is out[0], got[1] is out[1], got[3] is out[3])


def flagged(fn):
    out = fn()
    return [v if isinstance(v, torch.Tensor) or v is None else torch.tensor([int(v)]) for v in out]


case("recon_finish into out u16_12", lambda: flagged(lambda: recon_into_out(None, SampleFormat.u16(12))))
case("recon_finish into out u8 size 5x7", lambda: flagged(lambda: recon_into_out((5, 7), SampleFormat.u8())))

# ragged: three signals of different sizes, one transposed, one channel-first -- two runs of one channel stride, so two launches
for fname, fmt in N4_FORMATS:
    rng = np.random.RandomState(60 + fmt.kind)
    a, b, c = n4_signal(rng, (8, 8, 3), fmt), n4_signal(rng, (6, 5, 3), fmt), n4_signal(rng, (3, 7, 4), fmt)
    sigs = [a, b.transpose(0, 1), c.movedim(0, -1)]
    sizes = [(8, 8), (5, 6), (7, 4)]
    case(f"signal_patch_ragged {fname}", lambda: ops.signal_patch_ragged(sigs, lay, sample_format=fmt))
    if fmt.kind in (SampleFormat.U8, SampleFormat.F32):
        out = torch.empty(12, 16, 3, device=DEV)
        case(f"signal_patch_ragged {fname} by dtype into out", lambda: ops.signal_patch_ragged(sigs, lay, out=out))
    y = ops.signal_patch_ragged(sigs, lay, sample_format=fmt)
    rec = n4_recon(rng, y)
    case(f"recon_finish_ragged {fname} swap",
         lambda: ops.recon_finish_ragged(rec, y, layout=lay, sizes=sizes, swap=[False, True, False], sample_format=fmt,
                                         want_int=fmt.is_integer, want_whole=True))
    case(f"recon_finish_ragged {fname} scores only", lambda: ops.recon_finish_ragged(rec, y, layout=lay, sizes=sizes, sample_format=fmt))
case("recon_finish_ragged 8bit by mode, no target",
     lambda: ops.recon_finish_ragged(rec, layout=lay, sizes=sizes, mode=ops.RECON_8BIT, want_int=True, want_whole=True))
lay1 = ops.PeLayout((3,), (5,))
rng = np.random.RandomState(70)
sigs1 = [n4_signal(rng, (m, 3), SampleFormat.s16()) for m in (15, 4, 11)]
y1 = ops.signal_patch_ragged(sigs1, lay1, sample_format=SampleFormat.s16())
case("signal_patch_ragged 1d elem s16", lambda: y1)
case("recon_finish_ragged 1d elem s16", lambda: ops.recon_finish_ragged(n4_recon(rng, y1), y1, layout=lay1, sizes=[(15,), (4,), (11,)],
                                                                        sample_format=SampleFormat.s16(), want_int=True, want_whole=True))

# one refused call per wrapper (and per place that refuses: the wrapper's own checks, then the library's)
u8sig = torch.zeros(2, 8, 8, 3, device=DEV, dtype=torch.uint8)
yz = torch.zeros(8, 16, 3, device=DEV)
case("refusal signal_patch dtype", lambda: ops.signal_patch(u8sig.to(torch.int32), lay))
case("refusal signal_patch format dtype", lambda: ops.signal_patch(u8sig, lay, sample_format=SampleFormat.s16()))
case("refusal signal_patch grid", lambda: ops.signal_patch(u8sig[:, :7], lay))
case("refusal signal_patch out", lambda: ops.signal_patch(u8sig, lay, out=torch.empty(8, 16, 4, device=DEV)))
case("refusal signal_patch_pad above the grid", lambda: ops.signal_patch_pad(torch.zeros(2, 9, 8, 3, device=DEV), lay))
case("refusal signal_patch_pad 33 channels", lambda: ops.signal_patch_pad(torch.zeros(1, 8, 8, 33, device=DEV), lay))
case("refusal signal_patch_fmt 33 channels", lambda: ops.signal_patch(torch.zeros(1, 8, 8, 33, device=DEV), lay,
                                                                      sample_format=SampleFormat.f32()))
case("refusal signal_patch_ragged empty", lambda: ops.signal_patch_ragged([], lay))
case("refusal signal_patch_ragged mixed", lambda: ops.signal_patch_ragged([u8sig[0], u8sig[0].float()], lay))
case("refusal signal_patch_ragged dtype", lambda: ops.signal_patch_ragged([u8sig[0].to(torch.int32)], lay))
case("refusal signal_patch_ragged out", lambda: ops.signal_patch_ragged([u8sig[0]], lay, out=torch.empty(4, 16, 3, device=DEV).half()))
case("refusal signal_patch_ragged above the grid", lambda: ops.signal_patch_ragged([torch.zeros(9, 8, 3, device=DEV)], lay))
case("refusal recon_finish y", lambda: ops.recon_finish(yz.transpose(0, 1)))
case("refusal recon_finish target", lambda: ops.recon_finish(yz, yz[:4], layout=lay))
case("refusal recon_finish size axes", lambda: ops.recon_finish(yz, layout=lay, size=(5,)))
case("refusal recon_finish out", lambda: ops.recon_finish(yz, layout=lay, out=(None, torch.empty(2, 8, 8, 4, device=DEV), None, None)))
case("refusal recon_finish size above the grid", lambda: ops.recon_finish(yz, layout=lay, size=(9, 8), want_whole=True))
case("refusal recon_finish rows", lambda: ops.recon_finish(yz[:6].contiguous(), layout=lay, want_whole=True))
case("refusal recon_finish raw mode integers", lambda: ops.recon_finish(yz, layout=lay, mode=ops.RECON_RAW, want_u8=True))
case("refusal recon_finish_fmt f32 integers", lambda: ops.recon_finish(yz, layout=lay, sample_format=SampleFormat.f32(), want_int=True))
case("refusal recon_finish_ragged no sizes", lambda: ops.recon_finish_ragged(yz, layout=lay))
case("refusal recon_finish_ragged swap", lambda: ops.recon_finish_ragged(yz, layout=lay, sizes=[(8, 8), (8, 8)], swap=[True]))
case("refusal recon_finish_ragged y", lambda: ops.recon_finish_ragged(yz.double(), layout=lay, sizes=[(8, 8), (8, 8)]))
case("refusal recon_finish_ragged target", lambda: ops.recon_finish_ragged(yz, yz.half(), layout=lay, sizes=[(8, 8), (8, 8)]))
case("refusal recon_finish_ragged count", lambda: ops.recon_finish_ragged(yz, layout=lay, sizes=[(8, 8)]))
case("refusal recon_finish_ragged above the grid", lambda: ops.recon_finish_ragged(yz, layout=lay, sizes=[(8, 8), (8, 9)], want_whole=True))
case("refusal recon_finish_ragged_into buffer",
     lambda: ops.recon_finish_ragged_into(yz, None, lay, [(8, 8), (8, 8)], [(0, 24, 3), (192, 24, 3)], 384, ops.RECON_U16, 12,
                                          q_buf=torch.empty(384, device=DEV, dtype=torch.uint8)))
case("refusal recon_finish_ragged_into overlap",
     lambda: ops.recon_finish_ragged_into(yz, None, lay, [(8, 8), (8, 8)], [(0, 24, 3), (100, 24, 3)], 384, ops.RECON_8BIT, 0,
                                          q_buf=torch.empty(384, device=DEV, dtype=torch.uint8)))

# ---- N4 (417), the squared error by region: recon_regions ---------------------------------------------------------------------
# the quad path (runs, box rows and origins on 4-element boundaries: C = 4) and the element path (C = 3), with and without a
# size, a box that straddles patches, one that exceeds the extent, every format, by mode, no target, into `out`
for cname, Cc in (("quad", 4), ("elem", 3)):
    rng = np.random.RandomState(60 + Cc)
    yr = torch.from_numpy(rng.rand(8, 16, Cc).astype(np.float32)).to(DEV)
    recr = n4_recon(rng, yr)
    for fname, fmt in N4_FORMATS:
        case(f"recon_regions {cname} patch {fname}", lambda: ops.recon_regions(recr, yr, lay, (4, 4), sample_format=fmt))
        case(f"recon_regions {cname} 3x2 size 5x7 {fname}", lambda: ops.recon_regions(recr, yr, lay, (3, 2), size=(5, 7), sample_format=fmt))
    case(f"recon_regions {cname} 2x2 8bit by mode", lambda: ops.recon_regions(recr, yr, lay, (2, 2)))
    case(f"recon_regions {cname} row raw by mode", lambda: ops.recon_regions(recr, yr, lay, (1, 100), mode=ops.RECON_RAW))
    case(f"recon_regions {cname} no target", lambda: ops.recon_regions(recr, None, lay, (4, 4), size=(5, 7)))
    case(f"recon_regions {cname} into out",
         lambda: ops.recon_regions(recr, yr, lay, (4, 4), out=(torch.zeros(2, 2, 2, device=DEV, dtype=torch.float64),
                                                               torch.zeros(2, 2, 2, device=DEV, dtype=torch.int32))))
case("refusal recon_regions no layout", lambda: ops.recon_regions(yz, yz, None, (4, 4)))
case("refusal recon_regions region axes", lambda: ops.recon_regions(yz, yz, lay, (4,)))
case("refusal recon_regions region 0", lambda: ops.recon_regions(yz, yz, lay, (4, 0)))
case("refusal recon_regions size above the grid", lambda: ops.recon_regions(yz, yz, lay, (4, 4), size=(9, 8)))
case("refusal recon_regions out", lambda: ops.recon_regions(yz, yz, lay, (4, 4), out=(torch.empty(2, 2, device=DEV, dtype=torch.float64), None)))
