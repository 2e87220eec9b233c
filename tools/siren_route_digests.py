"""SHA-256 of what the SIREN wrappers return for one case per leaf of the router (recombiner_amd/csrc/siren_route.h), on seeded
inputs at the smallest shapes: 4 rows, samples 1 and 2, 64 and 33 pixels.  In the style of tools/ops_binding_digests.py: run it
in two trees and / or on two builds of the library and compare the output line by line -- a refactor of the host side must not
move a bit or a refusal.  Under `rocprofv3 --kernel-trace` the same run gives the sequence of kernels and launch geometries.

  python tools/siren_route_digests.py [--tree DIR]      DIR: the tree whose recombiner_amd is imported (default: this one);
                                                        RCB_LIB names the library when DIR has none of its own"""
import argparse
import ctypes as C
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
LIB = ops._lib.load()
G = 4


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
    print(f"{name:66s} {line}", flush=True)


def inputs(meta, pe16):
    gen = torch.Generator().manual_seed(1000 * meta.n_hidden + 10 * meta.hidden + meta.n_pix + meta.samples)
    P, F, E, Cc = meta.n_pix, meta.fourier_dim, meta.pe_dim, meta.out_dim
    xf = (torch.rand(P, F, generator=gen) * 2 - 1).to(DEV)
    pe = (torch.randn(G, P, E, generator=gen) * 0.5).to(DEV) if E else None
    fan = max(meta.dims[1:-1])
    wv = ((torch.rand(G, meta.d_net, generator=gen) * 2 - 1) * (np.sqrt(6 / fan) / 30) * 3.0).to(DEV)
    y = torch.rand(G // meta.samples, P, Cc, generator=gen).to(DEV)
    dy = (torch.randn(G, P, Cc, generator=gen) * 1e-3).to(DEV)
    if pe16 and pe is not None:
        pe = pe.to(bf16)
    return xf, pe, wv, y, dy


SHAPES = ((1, 64), (2, 33))


def run(tag, F, E, Cc, nh, hid, precision, pe16=False, modes=("fwd", "bwd", "loss"), shapes=SHAPES, hidden_dims=None, chunks=(1,),
        **loss_kw):
    for S, P in shapes:
        meta = ops.SirenMeta(S, P, F, E, nh, hid, Cc, precision=precision, hidden_dims=hidden_dims)
        xf, pe, wv, y, dy = inputs(meta, pe16)
        for ch in chunks:
            name = f"{tag} S{S} P{P}" + (f" chunks{ch}" if ch > 1 else "")
            if "fwd" in modes:
                case(name + " fwd", lambda: ops.siren_fwd(xf, pe, wv, meta, pixel_chunks=ch))
            if "bwd" in modes:
                case(name + " bwd", lambda: ops.siren_bwd(xf, pe, wv, dy, meta, pixel_chunks=ch))
            if "bwd no dpe" in modes:
                case(name + " bwd no dpe", lambda: ops.siren_bwd(xf, pe, wv, dy, meta, want_dpe=False, pixel_chunks=ch))
            if "loss" in modes:
                case(name + " loss", lambda: ops.siren_loss_bwd(xf, pe, wv, y, 1.0 / (S * P * Cc), meta, pixel_chunks=ch, **loss_kw))
            if "loss no dpe" in modes:
                case(name + " loss no dpe",
                     lambda: ops.siren_loss_bwd(xf, pe, wv, y, 1.0 / (S * P * Cc), meta, want_dpe=False, pixel_chunks=ch, **loss_kw))


# ---- fp32 on the matrix cores: the six instances (NH, KS, NB) --------------------------------------------------------------
for nh, F, E in ((3, 16, 16), (2, 16, 16), (3, 18, 16), (1, 16, 16), (4, 16, 16), (3, 32, 32)):
    run(f"fp32 nh{nh} F{F} E{E}", F, E, 3, nh, 32, 0)
# ---- fp32 on the plain-FMA kernel: another width, a width list, 5 hidden layers --------------------------------------------
run("generic w48", 16, 16, 3, 3, 48, 0)
run("generic widths 24 40 8", 16, 16, 3, 3, 40, 0, hidden_dims=(24, 40, 8))
run("generic nh5", 16, 16, 3, 5, 32, 0)
# ---- 16-bit, width 32, one workgroup per row: four instances x bf16 / f16 x fwd, bwd, loss, loss with 16-bit input rows -----
WG = ((3, 16, 16, 3), (3, 16, 16, 1), (3, 18, 16, 3), (2, 16, 16, 3))
LIB.rcb_debug_siren_wave_tiles(0)
for nh, F, E, Cc in WG:
    for prec in (1, 2):
        run(f"workgroup p{prec} nh{nh} F{F} E{E} C{Cc}", F, E, Cc, nh, 32, prec)
        run(f"workgroup p{prec} nh{nh} F{F} E{E} C{Cc} 16-bit rows", F, E, Cc, nh, 32, prec, pe16=True, modes=("loss", "bwd"), chunks=(1, 2))
# ---- one wave per row: loss / backward x dpe / no dpe, forced (2) and switched off (0); the default (1) at 4 rows -------------
for tiles in (2, 0, 1):
    LIB.rcb_debug_siren_wave_tiles(tiles)
    run(f"wave tiles={tiles} nh3 F16 E16 C3", 16, 16, 3, 3, 32, 1, pe16=True, modes=("bwd", "bwd no dpe", "loss", "loss no dpe"),
        shapes=((1, 64), (2, 64)), chunks=(1, 2))
    run(f"wave tiles={tiles} f16 (no instance)", 16, 16, 3, 3, 32, 2, pe16=True, modes=("loss",), shapes=((1, 64),))
    run(f"wave tiles={tiles} C1 (no instance)", 16, 16, 1, 3, 32, 1, pe16=True, modes=("loss",), shapes=((1, 64),))
# ---- widths 48 / 64: the four instances ----------------------------------------------------------------------------------
for F, E, Cc, W in ((16, 16, 3, 48), (16, 16, 3, 64), (18, 16, 3, 64), (16, 16, 1, 64)):
    for prec in (1, 2):
        run(f"wide p{prec} F{F} E{E} C{Cc} w{W}", F, E, Cc, 3, W, prec)
        run(f"wide p{prec} F{F} E{E} C{Cc} w{W} 16-bit rows", F, E, Cc, 3, W, prec, pe16=True, modes=("loss", "bwd"), chunks=(1, 2))
# ---- one wave per row at widths 16 / 24 (1 .. 4 layers) and 16 / 24 / 32 (5 .. 7 layers), KS 1 and 2 -----------------------
for hid in (16, 24, 32):
    for nh in range(1 if hid < 32 else 5, 8):
        run(f"rowwave p1 w{hid} nh{nh} KS1", 16, 16, 3, nh, hid, 1, pe16=True)
        run(f"rowwave p2 w{hid} nh{nh} KS2", 32, 32, 3, nh, hid, 2, modes=("fwd", "loss"), shapes=((2, 33),))
run("rowwave p1 w16 nh3 KS2 by C", 16, 16, 20, 3, 16, 1, chunks=(1, 2))
# ---- the 16-bit forms of the gradient, chunked and not -----------------------------------------------------------------------
for kw in (dict(want_bf16=True), dict(want_planes=True)):
    form = "bf16 copy" if "want_bf16" in kw else "planes"
    run(f"workgroup p1 {form}", 16, 16, 3, 3, 32, 1, pe16=True, modes=("loss",), chunks=(1, 2), **kw)
    run(f"wide p2 w64 {form}", 16, 16, 3, 3, 64, 2, pe16=True, modes=("loss",), chunks=(1, 2), **kw)
    run(f"rowwave p1 w24 nh5 {form}", 16, 16, 3, 5, 24, 1, pe16=True, modes=("loss",), chunks=(1, 2), **kw)
# ---- refusals that need real pointers ------------------------------------------------------------------------------------------
ONE = ((1, 64),)
run("refusal workgroup nh4 (not instantiated)", 16, 16, 3, 4, 32, 1, shapes=ONE)
run("refusal workgroup F32 E32 (not instantiated)", 32, 32, 3, 3, 32, 2, shapes=ONE)
run("refusal wide w48 nh2 (not instantiated)", 16, 16, 3, 2, 48, 1, shapes=ONE)
run("refusal wide w64 C2 (not instantiated)", 16, 16, 2, 3, 64, 2, shapes=ONE)
run("refusal fp32 nh4 F18 (no kernel for)", 18, 16, 3, 4, 32, 0, shapes=ONE)
run("refusal fp32 nh2 F32 E32 (no kernel for)", 32, 32, 3, 2, 32, 0, shapes=ONE)
run("refusal rowwave w16 F34", 34, 16, 3, 3, 16, 1, shapes=ONE)
run("refusal rowwave w32 nh6 E34", 16, 34, 3, 6, 32, 2, shapes=ONE)
run("refusal generic width list 32 100", 16, 16, 3, 2, 64, 0, hidden_dims=(32, 100), shapes=ONE)
run("refusal fp32 chunks", 16, 16, 3, 3, 32, 0, shapes=ONE, chunks=(2,))
run("refusal chunks above the tiles", 16, 16, 3, 3, 32, 1, shapes=ONE, chunks=(3,))
probe = torch.zeros(256, 4, device=DEV, dtype=torch.int64)
run("refusal rowwave w16 clock_probe", 16, 16, 3, 3, 16, 1, shapes=ONE, modes=("loss",), clock_probe=probe)
run("refusal rowwave w32 nh5 clock_probe", 16, 16, 3, 5, 32, 2, shapes=ONE, modes=("loss",), clock_probe=probe)
run("workgroup p1 clock_probe", 16, 16, 3, 3, 32, 1, shapes=ONE, modes=("loss",), clock_probe=probe)
print(f"{'  clock_probe written':66s} {bool(probe.any())}")


def null_dwvec(entry, planes):
    """the entry called with dwvec = NULL: refused unless both planes take the gradient"""
    meta = ops.SirenMeta(1, 64, 16, 16, 3, 32, 3, precision=1)
    xf, pe, wv, y, dy = inputs(meta, True)
    pl = ops.Planes(G, meta.d_net, DEV) if planes else None
    d, _ = ops._siren_desc(meta, wv, xf, pe, dw_planes=pl)
    sse, dpe = torch.empty(G, device=DEV), torch.empty_like(pe)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    if entry == "rcb_siren_bwd":
        rc = LIB.rcb_siren_bwd(C.byref(d), p(xf), p(pe), p(wv), p(dy), None, p(dpe), ops.stream_ptr())
    else:
        rc = LIB.rcb_siren_loss_bwd(C.byref(d), p(xf), p(pe), p(wv), p(y), 1.0 / 192, p(sse), None, p(dpe), ops.stream_ptr())
    ops.check(rc, entry)
    return (pl, dpe) if entry == "rcb_siren_bwd" else (sse, pl, dpe)


for entry in ("rcb_siren_bwd", "rcb_siren_loss_bwd"):
    case(f"{entry} dwvec NULL, no planes", lambda: null_dwvec(entry, False))
    case(f"{entry} dwvec NULL, planes", lambda: null_dwvec(entry, True))
