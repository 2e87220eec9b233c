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
