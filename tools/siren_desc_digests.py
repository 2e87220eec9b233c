"""What the SIREN entry points answer to a fixed lattice of descriptors, through the built library, with every data pointer NULL:
an accepted descriptor ends in the entry's own "null pointer" refusal, so nothing is ever launched and the tool runs on any
machine.  Per entry: one SHA-256 over the (code, rcb_last_error_string()) lines and the counts of the outcomes.  Run it on two
builds of the library and compare: a refactor of the host side must not move a line.  rcb_siren_reduce_chunks tests its
pointers first, so with NULL pointers every one of its lines is that one refusal: its digest pins that order and nothing about
the descriptor rule (the chunked cases of tools/siren_route_digests.py run it with real pointers).

  python tools/siren_desc_digests.py [--lib PATH] [--lines FILE] [--write-golden]

--lines FILE writes every line (about 1.7 million, the four entries interleaved); --write-golden records tests/golden/siren_desc_outcomes.json, which
tests/test_siren_route_cpu.py holds the built library to.  tests/siren_route_sweep.cpp walks the same lattice."""
import argparse
import collections
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "siren_desc_outcomes.json")

# ---- the lattice (tests/siren_route_sweep.cpp states the same lists) --------------------------------------------------------
PRECISIONS = (-1, 0, 1, 2, 3)
HIDDEN = (0, 1, 8, 16, 17, 24, 32, 33, 48, 64, 65)
N_HIDDEN = tuple(range(9))
WIDTH_LISTS = ("none", "uniform", "mixed")
MIXED = (24, 40, 8, 16)
FEC = ((16, 16, 3), (16, 16, 1), (18, 16, 3), (16, 0, 3), (32, 32, 32), (34, 32, 3), (16, 16, 33), (15, 16, 3), (16, 12, 3))
N_PIX = (32, 33)
CHUNKS = (0, 1, 2, 3)
N_ROWS, SAMPLES, STRIDE = 4, 2, 1 << 16
ENTRIES = ("rcb_siren_fwd", "rcb_siren_bwd", "rcb_siren_loss_bwd", "rcb_siren_reduce_chunks")


def siren_desc_type():
    sys.path.insert(0, ROOT)
    from recombiner_amd._lib import SirenDesc
    return SirenDesc


def base_desc(SirenDesc):
    d = SirenDesc()
    d.n_rows, d.samples, d.w_row_stride, d.dw_bf16_stride, d.w0 = N_ROWS, SAMPLES, STRIDE, STRIDE, 30.0
    return d


def lattice(SirenDesc, plane):
    """yields (label, descriptor); the descriptor object is reused.  plane: an address for dw_bf16 / dw_lo (never dereferenced)"""
    d = base_desc(SirenDesc)
    for prec, hid, nh, wl in itertools.product(PRECISIONS, HIDDEN, N_HIDDEN, WIDTH_LISTS):
        d.precision, d.hidden, d.n_hidden = prec, hid, nh
        widths = {"none": (0,) * 4, "uniform": (hid,) * 4, "mixed": MIXED}[wl]
        for i in range(4):
            d.hidden_dims[i] = widths[i]
        head = f"p{prec} w{hid} nh{nh} {wl}"
        for (F, E, Cc), P in itertools.product(FEC, N_PIX):
            d.fourier_dim, d.pe_dim, d.out_dim, d.n_pix = F, E, Cc, P
            mid = f"{head} F{F} E{E} C{Cc} P{P}"
            for chunks, pe16, dw16 in itertools.product(CHUNKS, (0, 1), (0, 1)):
                d.pixel_chunks, d.pe_bf16, d.dw_bf16 = chunks, pe16, plane if dw16 else None
                yield f"{mid} ch{chunks} pe16={pe16} dw16={dw16}", d


def extras(SirenDesc, plane):
    """stitched pe layouts, the low plane without the high one, row strides, width lists out of range, a null descriptor"""
    def fresh(**kw):
        d = base_desc(SirenDesc)
        d.precision, d.hidden, d.n_hidden, d.fourier_dim, d.pe_dim, d.out_dim, d.n_pix, d.pe_bf16 = 1, 32, 3, 16, 16, 3, 64, 1
        for k, v in kw.items():
            if isinstance(v, tuple):
                for i, x in enumerate(v):
                    getattr(d, k)[i] = x
            else:
                setattr(d, k, v)
        return d
    yield "null descriptor", None
    grids = [(1, (1,), (64,)), (2, (2, 2), (8, 8)), (3, (1, 2, 1), (4, 4, 4)), (2, (2, 1), (8, 8)), (2, (3, 1), (8, 8)),
             (2, (2, 2), (8, 4)), (2, (2, 0), (8, 8)), (2, (2, 2), (0, 8)), (4, (2, 2), (8, 8)), (-1, (2, 2), (8, 8)),
             (2, (4, 1), (8, 8)), (2, (1, 1), (64, 1)), (1, (2,), (64,)), (3, (1, 1, 1), (1, 1, 64))]
    for nd, pn, ps in grids:
        for prec, E, rows in ((1, 16, 4), (2, 16, 8), (0, 16, 4), (1, 0, 4), (1, 16, 6)):
            yield (f"grid nd{nd} pn{pn} ps{ps} p{prec} E{E} rows{rows}",
                   fresh(pe_grid_dims=nd, pe_patch_nums=pn, pe_patch_size=ps, precision=prec, pe_dim=E, n_rows=rows,
                         pe_bf16=int(prec > 0 and E > 0)))
    yield "grid 8192-pixel axis", fresh(pe_grid_dims=2, pe_patch_nums=(1, 1), pe_patch_size=(2, 8192), n_pix=16384)
    yield "grid 2^20 pixels", fresh(pe_grid_dims=2, pe_patch_nums=(1, 1), pe_patch_size=(1024, 1024), n_pix=1 << 20)
    for prec in (0, 1, 2):
        yield f"dw_lo without dw_bf16 p{prec}", fresh(precision=prec, pe_bf16=0, dw_lo=plane)
        yield f"dw_lo with dw_bf16 p{prec}", fresh(precision=prec, pe_bf16=0, dw_lo=plane, dw_bf16=plane)
        yield f"planes, two chunks p{prec}", fresh(precision=prec, pe_bf16=0, dw_lo=plane, dw_bf16=plane, pixel_chunks=2)
    dnet = 32 * 33 + 2 * 32 * 33 + 3 * 33
    for stride in (dnet - 1, dnet):
        yield f"w_row_stride {stride}", fresh(w_row_stride=stride)
        yield f"dw_bf16_stride {stride}", fresh(dw_bf16=plane, dw_bf16_stride=stride)
    yield "w_row_stride of a width list", fresh(precision=0, pe_bf16=0, hidden=40, hidden_dims=MIXED[:3], w_row_stride=24 * 33 + 40 * 25 + 8 * 41 + 3 * 9)
    yield "w_row_stride below a width list", fresh(precision=0, pe_bf16=0, hidden=40, hidden_dims=MIXED[:3], w_row_stride=24 * 33 + 40 * 25 + 8 * 41 + 3 * 9 - 1)
    for widths in ((32, 100, 32, 0), (32, 0, 32, 0), (32, -4, 32, 0), (64, 64, 64, 64), (65, 1, 1, 1)):
        for nh in (2, 3, 4):
            yield f"width list {widths} nh{nh}", fresh(precision=0, pe_bf16=0, n_hidden=nh, hidden_dims=widths)
    for rows, samples, P in ((0, 1, 64), (4, 0, 64), (4, 3, 64), (4, 2, 0), (4, 2, 1 << 30), (1 << 29, 1, 64)):
        yield f"rows{rows} samples{samples} P{P}", fresh(n_rows=rows, samples=samples, n_pix=P, pixel_chunks=2 if rows > 4 else 0)
    yield "pe_bf16 = 2", fresh(pe_bf16=2)
    yield "reduce: chunks 2", fresh(pixel_chunks=2)


def run(lib, lines_out=None):
    """-> {entry: {"sha256" over all lines, "descriptors" / "accepted" of the lattice, "extras" / "extras_accepted", "by_code"}}"""
    SirenDesc = siren_desc_type()
    keep = C.create_string_buffer(16)
    plane = C.addressof(keep)
    last = lib.rcb_last_error_string
    last.restype = C.c_char_p
    nul = C.c_void_p(0)
    calls = []
    for entry in ENTRIES:
        fn = getattr(lib, entry)
        fn.restype = C.c_int
        if entry == "rcb_siren_loss_bwd":
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 4
            args = (nul, nul, nul, nul, C.c_float(0.25), nul, nul, nul, nul)
        else:
            n_ptr = {"rcb_siren_fwd": 5, "rcb_siren_bwd": 7, "rcb_siren_reduce_chunks": 5}[entry]
            fn.argtypes = [C.c_void_p] * (1 + n_ptr)
            args = (nul,) * n_ptr
        # [call, arguments, "accepted" text, sha, by code, descriptors (lattice, extras), accepted (lattice, extras)]
        calls.append((fn, args, entry[4:].encode() + b": null pointer", hashlib.sha256(), collections.Counter(), [0, 0], [0, 0],
                      entry.encode() + b" "))
    for part, descs in enumerate((lattice(SirenDesc, plane), extras(SirenDesc, plane))):
        for label, d in descs:
            ref, label = None if d is None else C.byref(d), label.encode()
            for fn, args, accept, sha, codes, n, accepted, tag in calls:
                rc = fn(ref, *args)
                text = last() if rc else b""
                line = b"%s: %d %s\n" % (label, rc, text)
                sha.update(line)
                codes[rc] += 1
                n[part] += 1
                accepted[part] += text == accept
                if lines_out is not None:
                    lines_out.write(tag + line)
    out = {}
    for entry, (fn, args, accept, sha, codes, n, accepted, tag) in zip(ENTRIES, calls):
        out[entry] = {"sha256": sha.hexdigest(), "descriptors": n[0], "accepted": accepted[0], "extras": n[1],
                      "extras_accepted": accepted[1], "by_code": {str(k): v for k, v in sorted(codes.items())}}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.environ.get("RCB_LIB") or os.path.join(ROOT, "recombiner_amd", "lib", "librcb_hip.so"))
    ap.add_argument("--lines")
    ap.add_argument("--write-golden", action="store_true")
    a = ap.parse_args()
    f = open(a.lines, "wb") if a.lines else None
    res = run(C.CDLL(a.lib), f)
    print(json.dumps(res, indent=1))
    if a.write_golden:
        with open(GOLDEN, "w") as g:
            json.dump(res, g, indent=1)
            g.write("\n")
