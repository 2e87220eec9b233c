"""The five 16-bit SIREN kernel families against the operand-exact fp64 evaluator (tests/siren_emul.py); run with -m gpu.

The fp32-yardstick tests (test_hip_kernels.py, test_hip_narrow_siren.py, test_hip_deep_siren.py) compare the kernels with an
fp32 restatement of the MLP, so their limits carry the rounding noise of the 16-bit operands (bf16 at the initialisation scale:
y 2e-2, dW 9e-3, dpe 3e-2 of the tensor's largest entry).  Here the reference rounds where the kernels round, and what is left
is the order of the fp32 accumulations, the error of v_sin / v_cos, and the operands those two push across a rounding boundary.
Errors are taken per block (siren_emul.block_errors), each block divided by its own largest reference entry.

What the MI355X measurement found (MEASURED below; recorded fp32-yardstick errors in bf16: y 6.4e-3, dW 2.9e-3, dpe 1.0e-2):
  * the MEDIAN element error of a block is at fp32 level in every family and mode (bf16: y 2e-8 .. 3e-8, dpe 1e-9 .. 4e-9, dW
    1e-8 .. 5e-5 of the block's largest entry): no family rounds anywhere the evaluator does not, and none misses a rounding
    point.  These limits are 100 to 10^5 times tighter than the fp32 yardstick's;
  * the LARGEST element error of a block (bf16: y up to 1.4e-3, dW 1.1e-3, dpe 2.7e-3) is only 2 to 5 times below the
    yardstick's figures, not ten: it is one operand moved by an ulp because the kernel's fp32 pre-activation (accumulation
    order, v_sin / v_cos error) falls on the other side of a bf16 boundary than the fp64 one.  Evidence: the CPU sensitivity
    run (test_siren_emul_cpu.py, pre-activations changed by 2^-22) reproduces that level without any kernel (y 2.1e-3, dW
    3.4e-3, dpe 3.3e-3), the errors sit in single pixels (median 2e-8), and the narrow family, where no operand flipped in
    the forward pass, has y within 7.6e-8.  No rounding point can remove it, so each block kind carries both limits, and the
    limit on the largest error is never below the flip floor of its kind (siren_emul.FLIP_FLOOR; bf16 y 3.7e-3, dW 1.4e-3 ..
    3.5e-3, dpe 5.8e-3: 3 to 6 times below the yardstick's limits of 2e-2 / 9e-3 / 3e-2, which is as tight as a limit on
    single elements can be made; the tenfold and tighter statement is the median's).
No kernel was changed.
"""
import math
import os

import pytest
import torch

import siren_emul as se

pytestmark = pytest.mark.gpu

from recombiner_amd import _lib, ops  # noqa: E402
from recombiner_amd.ops import SirenMeta  # noqa: E402

DEV = "cuda"
MODES = {1: "bf16", 2: "f16"}


CASES, DISCRIMINATION, switches, build = se.CASES, se.DISCRIMINATION, se.switches, se.build


def run_kernels(c, case, prec, wave):
    """forward, fused loss + backward, plain backward of one case on the family pinned by `wave` (rcb_debug_siren_wave_tiles: 0 the
    workgroup kernels, 2 the wave family whatever the number of rows) -> dict like siren_emul.run_emul, pe as the kernels saw it"""
    g = lambda x: x.to(DEV).contiguous()          # noqa: E731
    meta = SirenMeta(samples=c["S"], n_pix=c["P"], fourier_dim=c["F"], pe_dim=16, n_hidden=c["nh"], hidden=c["hidden"],
                     out_dim=c["C"], precision=prec)
    assert meta.d_net == case["D"]
    xf, wv, pe = g(case["xf"]), g(case["wv"]), g(case["pe"])
    if c["variant"] != "f32pe":
        pe = pe.bfloat16()
    xf16 = ops.xf_bf16(xf, prec) if c["variant"] == "in16" else None
    lib = _lib.load()
    fam = lib.rcb_debug_siren_wave_tiles(wave)
    if c["variant"] == "pe16":
        os.environ["RCB_SIREN_NO_XF16"] = "1"
    try:
        y = ops.siren_fwd(xf, pe, wv, meta, pixel_chunks=c["chunks"])
        sse, dw, dpe = ops.siren_loss_bwd(xf, pe, wv, g(case["y"]), case["dy_scale"], meta, pixel_chunks=c["chunks"], xf16=xf16)
        dw2, dpe2 = ops.siren_bwd(xf, pe, wv, g(case["dy"]), meta, pixel_chunks=c["chunks"])
    finally:
        lib.rcb_debug_siren_wave_tiles(fam)
        os.environ.pop("RCB_SIREN_NO_XF16", None)
    out = dict(y=y, sse=sse, dW=dw, dpe=dpe, bwd_dW=dw2, bwd_dpe=dpe2)
    return {k: v.float().cpu() for k, v in out.items()}, pe.float().cpu()


# ---- limits -----------------------------------------------------------------------------------------------------------------
# Per (family, mode): for every output and block kind the worst over the family's cases of a block's LARGEST element error and
# of its MEDIAN element error (siren_emul.block_stats), as MEASURED on MI355X; the limit is three times that -- the project's
# convention (test_siren_16bit_operands_at_init_scale) -- with the lower bounds of limits_of below.  Regenerate with `pytest -m gpu -s` (one
# line per family and mode).  dpe16 / bwd_dpe16: dpe stored as bf16 (the variants with bf16 pe), rounding R11 of the evaluator.
KINDS = [("y", "row"), ("sse", "row"), ("dW", "bias"), ("dW", "fourier"), ("dW", "pe"), ("dW", "weight"), ("dpe", "row"),
         ("dpe16", "row"), ("bwd_dW", "bias"), ("bwd_dW", "fourier"), ("bwd_dW", "pe"), ("bwd_dW", "weight"), ("bwd_dpe", "row"),
         ("bwd_dpe16", "row")]
KEYS = [k + (s,) for k in KINDS for s in ("max", "med")]
LIMIT_FLOOR = 2.0 ** -20          # sixteen fp32 ulps of the block's largest entry: what a statistic measured as 0 is held to
MEASURED = {
    # LIMITS-TABLE-BEGIN
    ("wg32", "bf16"): {
        ("y", "row", "max"): 1.35e-03, ("y", "row", "med"): 1.69e-08, ("sse", "row", "max"): 7.37e-06, ("sse", "row", "med"): 7.37e-06,
        ("dW", "bias", "max"): 2.33e-04, ("dW", "bias", "med"): 1.50e-05, ("dW", "fourier", "max"): 6.24e-04, ("dW", "fourier", "med"): 3.01e-05,
        ("dW", "pe", "max"): 1.03e-03, ("dW", "pe", "med"): 2.63e-05, ("dW", "weight", "max"): 4.69e-04, ("dW", "weight", "med"): 1.40e-06,
        ("dpe", "row", "max"): 2.17e-03, ("dpe", "row", "med"): 2.20e-09, ("dpe16", "row", "max"): 2.75e-03, ("dpe16", "row", "med"): 0.00e+00,
        ("bwd_dW", "bias", "max"): 1.79e-03, ("bwd_dW", "bias", "med"): 2.23e-04, ("bwd_dW", "fourier", "max"): 1.29e-03, ("bwd_dW", "fourier", "med"): 5.02e-05,
        ("bwd_dW", "pe", "max"): 2.31e-03, ("bwd_dW", "pe", "med"): 4.44e-05, ("bwd_dW", "weight", "max"): 8.76e-04, ("bwd_dW", "weight", "med"): 3.61e-08,
        ("bwd_dpe", "row", "max"): 2.63e-03, ("bwd_dpe", "row", "med"): 1.37e-09, ("bwd_dpe16", "row", "max"): 1.39e-03, ("bwd_dpe16", "row", "med"): 0.00e+00,
    },
    ("wg32", "f16"): {
        ("y", "row", "max"): 1.30e-04, ("y", "row", "med"): 1.79e-08, ("sse", "row", "max"): 5.71e-07, ("sse", "row", "med"): 5.71e-07,
        ("dW", "bias", "max"): 5.99e-05, ("dW", "bias", "med"): 1.50e-05, ("dW", "fourier", "max"): 1.64e-04, ("dW", "fourier", "med"): 1.29e-05,
        ("dW", "pe", "max"): 2.23e-04, ("dW", "pe", "med"): 4.65e-06, ("dW", "weight", "max"): 1.13e-04, ("dW", "weight", "med"): 8.95e-06,
        ("dpe", "row", "max"): 3.31e-04, ("dpe", "row", "med"): 8.11e-09, ("dpe16", "row", "max"): 1.38e-03, ("dpe16", "row", "med"): 0.00e+00,
        ("bwd_dW", "bias", "max"): 3.61e-04, ("bwd_dW", "bias", "med"): 1.65e-05, ("bwd_dW", "fourier", "max"): 1.46e-04, ("bwd_dW", "fourier", "med"): 6.45e-06,
        ("bwd_dW", "pe", "max"): 2.68e-04, ("bwd_dW", "pe", "med"): 4.68e-06, ("bwd_dW", "weight", "max"): 3.60e-04, ("bwd_dW", "weight", "med"): 6.26e-06,
        ("bwd_dpe", "row", "max"): 1.07e-04, ("bwd_dpe", "row", "med"): 5.52e-09, ("bwd_dpe16", "row", "max"): 1.77e-03, ("bwd_dpe16", "row", "med"): 0.00e+00,
    },
    ("wide", "bf16"): {
        ("y", "row", "max"): 1.77e-04, ("y", "row", "med"): 3.29e-08, ("sse", "row", "max"): 3.95e-07, ("sse", "row", "med"): 3.95e-07,
        ("dW", "bias", "max"): 1.31e-04, ("dW", "bias", "med"): 3.29e-06, ("dW", "fourier", "max"): 6.31e-04, ("dW", "fourier", "med"): 8.72e-06,
        ("dW", "pe", "max"): 3.95e-04, ("dW", "pe", "med"): 1.27e-05, ("dW", "weight", "max"): 6.86e-05, ("dW", "weight", "med"): 2.43e-07,
        ("dpe", "row", "max"): 6.14e-04, ("dpe", "row", "med"): 4.40e-09, ("dpe16", "row", "max"): 0.00e+00, ("dpe16", "row", "med"): 0.00e+00,
        ("bwd_dW", "bias", "max"): 7.88e-04, ("bwd_dW", "bias", "med"): 2.32e-05, ("bwd_dW", "fourier", "max"): 7.48e-04, ("bwd_dW", "fourier", "med"): 4.63e-06,
        ("bwd_dW", "pe", "max"): 9.47e-04, ("bwd_dW", "pe", "med"): 1.13e-05, ("bwd_dW", "weight", "max"): 5.29e-04, ("bwd_dW", "weight", "med"): 1.09e-08,
        ("bwd_dpe", "row", "max"): 4.61e-04, ("bwd_dpe", "row", "med"): 3.83e-09, ("bwd_dpe16", "row", "max"): 1.43e-03, ("bwd_dpe16", "row", "med"): 0.00e+00,
    },
    ("wide", "f16"): {
        ("y", "row", "max"): 1.08e-04, ("y", "row", "med"): 2.84e-08, ("sse", "row", "max"): 4.05e-07, ("sse", "row", "med"): 4.05e-07,
        ("dW", "bias", "max"): 3.95e-05, ("dW", "bias", "med"): 4.20e-06, ("dW", "fourier", "max"): 1.61e-04, ("dW", "fourier", "med"): 7.74e-06,
        ("dW", "pe", "max"): 1.87e-04, ("dW", "pe", "med"): 7.24e-06, ("dW", "weight", "max"): 1.01e-04, ("dW", "weight", "med"): 1.54e-06,
        ("dpe", "row", "max"): 4.28e-04, ("dpe", "row", "med"): 8.60e-09, ("dpe16", "row", "max"): 2.53e-03, ("dpe16", "row", "med"): 0.00e+00,
        ("bwd_dW", "bias", "max"): 3.12e-04, ("bwd_dW", "bias", "med"): 3.61e-05, ("bwd_dW", "fourier", "max"): 3.88e-04, ("bwd_dW", "fourier", "med"): 1.52e-05,
        ("bwd_dW", "pe", "max"): 5.20e-04, ("bwd_dW", "pe", "med"): 1.11e-05, ("bwd_dW", "weight", "max"): 2.67e-04, ("bwd_dW", "weight", "med"): 3.97e-06,
        ("bwd_dpe", "row", "max"): 3.34e-04, ("bwd_dpe", "row", "med"): 7.55e-09, ("bwd_dpe16", "row", "max"): 1.79e-04, ("bwd_dpe16", "row", "med"): 0.00e+00,
    },
    ("narrow", "bf16"): {
        ("y", "row", "max"): 7.55e-08, ("y", "row", "med"): 1.99e-08, ("sse", "row", "max"): 1.10e-07, ("sse", "row", "med"): 1.10e-07,
        ("dW", "bias", "max"): 6.60e-05, ("dW", "bias", "med"): 0.00e+00, ("dW", "fourier", "max"): 2.64e-04, ("dW", "fourier", "med"): 2.88e-08,
        ("dW", "pe", "max"): 3.80e-04, ("dW", "pe", "med"): 3.02e-08, ("dW", "weight", "max"): 9.44e-05, ("dW", "weight", "med"): 8.32e-09,
        ("dpe", "row", "max"): 7.19e-04, ("dpe", "row", "med"): 0.00e+00, ("dpe16", "row", "max"): 0.00e+00, ("dpe16", "row", "med"): 0.00e+00,
        ("bwd_dW", "bias", "max"): 1.24e-04, ("bwd_dW", "bias", "med"): 1.22e-05, ("bwd_dW", "fourier", "max"): 6.55e-05, ("bwd_dW", "fourier", "med"): 1.75e-08,
        ("bwd_dW", "pe", "max"): 8.86e-05, ("bwd_dW", "pe", "med"): 1.92e-08, ("bwd_dW", "weight", "max"): 7.61e-05, ("bwd_dW", "weight", "med"): 3.75e-06,
        ("bwd_dpe", "row", "max"): 3.06e-04, ("bwd_dpe", "row", "med"): 0.00e+00, ("bwd_dpe16", "row", "max"): 0.00e+00, ("bwd_dpe16", "row", "med"): 0.00e+00,
    },
    ("narrow", "f16"): {
        ("y", "row", "max"): 2.58e-04, ("y", "row", "med"): 2.53e-08, ("sse", "row", "max"): 6.41e-07, ("sse", "row", "med"): 6.41e-07,
        ("dW", "bias", "max"): 1.10e-04, ("dW", "bias", "med"): 2.28e-05, ("dW", "fourier", "max"): 1.95e-04, ("dW", "fourier", "med"): 3.74e-05,
        ("dW", "pe", "max"): 3.15e-04, ("dW", "pe", "med"): 4.40e-05, ("dW", "weight", "max"): 1.99e-04, ("dW", "weight", "med"): 2.68e-05,
        ("dpe", "row", "max"): 3.91e-04, ("dpe", "row", "med"): 4.07e-06, ("dpe16", "row", "max"): 1.45e-03, ("dpe16", "row", "med"): 0.00e+00,
        ("bwd_dW", "bias", "max"): 4.34e-04, ("bwd_dW", "bias", "med"): 9.42e-05, ("bwd_dW", "fourier", "max"): 2.06e-04, ("bwd_dW", "fourier", "med"): 4.94e-05,
        ("bwd_dW", "pe", "max"): 2.60e-04, ("bwd_dW", "pe", "med"): 3.85e-05, ("bwd_dW", "weight", "max"): 5.48e-04, ("bwd_dW", "weight", "med"): 5.27e-05,
        ("bwd_dpe", "row", "max"): 3.56e-04, ("bwd_dpe", "row", "med"): 2.22e-06, ("bwd_dpe16", "row", "max"): 0.00e+00, ("bwd_dpe16", "row", "med"): 0.00e+00,
    },
    ("deep", "bf16"): {
        ("y", "row", "max"): 1.04e-03, ("y", "row", "med"): 1.83e-08, ("sse", "row", "max"): 2.08e-06, ("sse", "row", "med"): 2.08e-06,
        ("dW", "bias", "max"): 1.38e-04, ("dW", "bias", "med"): 3.35e-05, ("dW", "fourier", "max"): 5.96e-04, ("dW", "fourier", "med"): 3.18e-05,
        ("dW", "pe", "max"): 1.11e-03, ("dW", "pe", "med"): 4.50e-05, ("dW", "weight", "max"): 2.87e-04, ("dW", "weight", "med"): 2.06e-05,
        ("dpe", "row", "max"): 2.33e-03, ("dpe", "row", "med"): 8.76e-10, ("dpe16", "row", "max"): 0.00e+00, ("dpe16", "row", "med"): 0.00e+00,
        ("bwd_dW", "bias", "max"): 3.54e-04, ("bwd_dW", "bias", "med"): 4.42e-05, ("bwd_dW", "fourier", "max"): 2.87e-04, ("bwd_dW", "fourier", "med"): 8.12e-06,
        ("bwd_dW", "pe", "max"): 3.45e-04, ("bwd_dW", "pe", "med"): 8.05e-06, ("bwd_dW", "weight", "max"): 3.62e-04, ("bwd_dW", "weight", "med"): 1.71e-05,
        ("bwd_dpe", "row", "max"): 8.29e-04, ("bwd_dpe", "row", "med"): 6.12e-10, ("bwd_dpe16", "row", "max"): 0.00e+00, ("bwd_dpe16", "row", "med"): 0.00e+00,
    },
    ("deep", "f16"): {
        ("y", "row", "max"): 6.38e-04, ("y", "row", "med"): 2.31e-08, ("sse", "row", "max"): 1.46e-06, ("sse", "row", "med"): 1.46e-06,
        ("dW", "bias", "max"): 2.88e-04, ("dW", "bias", "med"): 6.95e-05, ("dW", "fourier", "max"): 3.51e-04, ("dW", "fourier", "med"): 7.08e-05,
        ("dW", "pe", "max"): 3.56e-04, ("dW", "pe", "med"): 4.89e-05, ("dW", "weight", "max"): 2.59e-04, ("dW", "weight", "med"): 3.49e-05,
        ("dpe", "row", "max"): 6.66e-04, ("dpe", "row", "med"): 6.10e-09, ("dpe16", "row", "max"): 1.13e-04, ("dpe16", "row", "med"): 0.00e+00,
        ("bwd_dW", "bias", "max"): 8.90e-04, ("bwd_dW", "bias", "med"): 3.24e-04, ("bwd_dW", "fourier", "max"): 6.09e-04, ("bwd_dW", "fourier", "med"): 8.08e-05,
        ("bwd_dW", "pe", "max"): 4.79e-04, ("bwd_dW", "pe", "med"): 6.93e-05, ("bwd_dW", "weight", "max"): 8.90e-04, ("bwd_dW", "weight", "med"): 9.43e-05,
        ("bwd_dpe", "row", "max"): 7.44e-04, ("bwd_dpe", "row", "med"): 5.97e-09, ("bwd_dpe16", "row", "max"): 1.18e-03, ("bwd_dpe16", "row", "med"): 0.00e+00,
    },
    ("wave", "bf16"): {
        ("sse", "row", "max"): 9.30e-07, ("sse", "row", "med"): 9.30e-07, ("dW", "bias", "max"): 7.96e-05, ("dW", "bias", "med"): 3.98e-06,
        ("dW", "fourier", "max"): 4.61e-04, ("dW", "fourier", "med"): 6.72e-06, ("dW", "pe", "max"): 5.25e-04, ("dW", "pe", "med"): 1.16e-05,
        ("dW", "weight", "max"): 1.74e-04, ("dW", "weight", "med"): 8.59e-08, ("dpe16", "row", "max"): 2.56e-03, ("dpe16", "row", "med"): 0.00e+00,
        ("bwd_dW", "bias", "max"): 9.16e-04, ("bwd_dW", "bias", "med"): 1.50e-08, ("bwd_dW", "fourier", "max"): 1.15e-03, ("bwd_dW", "fourier", "med"): 7.46e-08,
        ("bwd_dW", "pe", "max"): 1.56e-03, ("bwd_dW", "pe", "med"): 4.20e-08, ("bwd_dW", "weight", "max"): 6.76e-04, ("bwd_dW", "weight", "med"): 7.13e-07,
        ("bwd_dpe16", "row", "max"): 1.77e-03, ("bwd_dpe16", "row", "med"): 0.00e+00,
    },
    # LIMITS-TABLE-END
}


def limits_of(family_mode, measured):
    """A block's MEDIAN element error: three times the measurement (at least LIMIT_FLOOR).  Its LARGEST element error: three times
    the measurement, and not below the flip floor of that block kind (siren_emul.FLIP_FLOOR) -- where no operand happened to flip
    on these inputs the measurement is at fp32 level (narrow bf16 y: 7.6e-8), and one flip after a compiler update that reorders
    an accumulation would otherwise fail the test with no kernel defect."""
    floor = se.FLIP_FLOOR[family_mode[1]]
    return {k: max(3.0 * v, floor[k[:2]] if k[2] == "max" else LIMIT_FLOOR) for k, v in measured.items()}


LIMITS = {fm: limits_of(fm, tab) for fm, tab in MEASURED.items()}

# An element may exceed the limit on a block's largest error when more than one flipped operand meets in it: at most FLIP_SHARE
# of the block's elements (none in a block of fewer than 1000), and none beyond FLIP_CAP of its block kind, twice the flip floor.
FLIP_SHARE = se.FLIP_SHARE
FLIP_CAP = {m: {k: 2.0 * v for k, v in tab.items()} for m, tab in se.FLIP_FLOOR.items()}


def check_blocks(errs, limits, mode, what):
    """local counterpart of golden_util.assert_close_mostly for per-block errors -> list of violations.  Every block: its median
    element error within the "med" limit of its (output, block kind); every element within the "max" limit, except a share of at
    most FLIP_SHARE of the block's elements, none of them above the FLIP_CAP of the block kind."""
    bad = []
    for (name, kind), blocks in errs.items():
        lmax, lmed = limits[(name, kind, "max")], limits[(name, kind, "med")]
        for e in blocks:
            over = int((e > lmax).sum())
            if over and (over > math.floor(FLIP_SHARE * e.numel()) or float(e.max()) > FLIP_CAP[mode][(name, kind)]):
                bad.append("%s %s/%s: %d of %d elements above %.2e, worst %.2e" % (what, name, kind, over, e.numel(), lmax, float(e.max())))
            if float(e.median()) > lmed:
                bad.append("%s %s/%s: median error %.2e above %.2e" % (what, name, kind, float(e.median()), lmed))
    return bad


def case_errors(family, c, prec, wave, **emul_kw):
    """block errors of one case run on the family pinned by `wave` against the evaluator with the family's switches (or emul_kw's)"""
    case = build(c)
    out, pe_seen = run_kernels(c, case, prec, wave)
    if wave:
        out["y"] = None                # the forward pass has no wave instance
    kw = dict(switches(family, c), **emul_kw)
    stored16 = c["variant"] != "f32pe"
    ref = se.run_emul(case, MODES[prec], pe=pe_seen, dpe_store="bf16" if stored16 else None, **kw)
    return se.block_errors(case, out, ref, "16" if stored16 else ""), out, ref


def line(family, mode, worst):
    return "%s %s: " % (family, mode) + "  ".join("%s/%s/%s %.2e" % (k + (worst[k],)) for k in KEYS if k in worst)


def worst_of(stats_list):
    worst = {}
    for st in stats_list:
        for k, v in st.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


FAMILY_MODES = [(f, p) for f in ("wg32", "wide", "narrow", "deep") for p in (1, 2)] + [("wave", 1)]


@pytest.mark.parametrize("family,prec", FAMILY_MODES)
def test_family_against_operand_exact_evaluator(family, prec):
    """Every case of CASES[family]: forward y, fused loss (sse, dW, dpe) and plain backward (dW, dpe) within LIMITS of the
    evaluator run with the family's switches, block by block; prints the worst per-block error of each output."""
    mode = MODES[prec]
    per_case = [(c, case_errors(family, c, prec, 2 if family == "wave" else 0)[0]) for c in CASES[family]]
    print("\n" + line(family, mode, worst_of(se.block_stats(e) for _, e in per_case)))
    assert (family, mode) in LIMITS, "no measured limits for %s %s" % (family, mode)
    bad = []
    for c, errs in per_case:
        bad += check_blocks(errs, LIMITS[(family, mode)], mode, str(c))
    assert not bad, "\n".join(bad)


def test_wave_and_workgroup_family_against_the_same_evaluator():
    """The sibling families on the wave family's cases (whole tiles, bf16 pe, 16-bit xf rows): each within its own limits of the
    SAME evaluator, which differs between them by the documented bias switch alone (fp32 in the accumulator / (hi, lo) halves
    through the matrix pipe); both keep the cosine in fp32 in the fused loss / backward on these inputs.  (Their 5e-4 comparison
    against each other stays in test_siren_wave_family_against_the_workgroup_family.)"""
    for fam, wave in (("wg32", 0), ("wave", 2)):
        assert switches(fam, CASES["wave"][0]) == dict(bias="hilo" if wave else "fp32", cos="fp32", cos_bwd="fp32" if wave else "packed")
        per_case = [(c, case_errors(fam, c, 1, wave)[0]) for c in CASES["wave"]]
        print("\n" + line(fam + " on the wave family's cases", "bf16", worst_of(se.block_stats(e) for _, e in per_case)))
        bad = []
        for c, errs in per_case:
            bad += check_blocks(errs, LIMITS[(fam, "bf16")], "bf16", "%s %s" % (fam, c))
        assert not bad, "\n".join(bad)


def test_width_32_with_one_or_four_hidden_layers_has_no_16bit_instance():
    """siren_mlp_bf16.hip is instantiated for 2 and 3 hidden layers; 1 and 4 are an error in the 16-bit modes, not a fall-back"""
    for nh in (1, 4):
        case = se.make_case(16, 16, [32] * nh, 3, 33, 1, 1, 0)
        meta = SirenMeta(1, 33, 16, 16, nh, 32, 3, precision=1)
        with pytest.raises(ops.RcbError):
            ops.siren_fwd(case["xf"].to(DEV), case["pe"].to(DEV), case["wv"].to(DEV), meta)


# ---- the limits discriminate ----------------------------------------------------------------------------------------------------
# the fp32-yardstick limits of each family at the initialisation scale, (y, dW, dpe) of the tensor's largest entry
OLD_LIMITS = {"bf16": (2.0e-2, 9e-3, 3.0e-2), "f16": (2.7e-3, 1.4e-3, 3.6e-3)}
def mutations(family, c, mode):
    F = se.Faults
    m = [("sine of layer 1 unrounded", dict(faults=F(sine_unrounded=1))),
         ("bias gradient of layer 1 x (1 + 2^-7)", dict(faults=F(bias_grad_scale=(1, 1.0 + 2.0 ** -7)))),
         ("last valid pixel left out of dW", dict(faults=F(drop_last_pixel=True))),
         ("Fourier half of layer 0's dW x 1.01", dict(faults=F(fourier_scale=1.01))),
         ("weights rounded before the k_hi multiplication", dict(faults=F(round_before_khi=True)))]
    if family == "wave":
        m.append(("bias taken as fp32 instead of (hi, lo)", dict(bias="fp32")))
    if mode == "f16":
        m.append(("GRAD_SCALE omitted before the rounding of dz", dict(faults=F(no_grad_scale=True))))
    return m


@pytest.mark.parametrize("family,prec", FAMILY_MODES)
def test_new_limits_see_what_the_fp32_yardstick_cannot(family, prec):
    """The kernel's outputs against deliberately wrong evaluators (siren_emul.Faults; nothing is injected into a kernel): each one
    FAILS the per-block limits.  The line printed beside it APPROXIMATES what the fp32-yardstick tests would have said: it takes
    the difference between the kernel and the wrong evaluator against the tensor's largest entry and compares it with that
    mode's fp32-yardstick limit; it does not run the fp32 restatement those tests use."""
    mode = MODES[prec]
    c = DISCRIMINATION[family]
    wave = 2 if family == "wave" else 0
    assert not check_blocks(case_errors(family, c, prec, wave)[0], LIMITS[(family, mode)], mode, "unmutated")
    unseen = []
    for name, kw in mutations(family, c, mode):
        errs, out, ref = case_errors(family, c, prec, wave, **kw)
        bad = check_blocks(errs, LIMITS[(family, mode)], mode, name)
        old = [float((out[o].double() - ref[o]).abs().max() / ref[o].abs().max()) < lim
               for o, lim in zip(("y", "dW", "dpe"), OLD_LIMITS[mode]) if out[o] is not None]
        print("%s %s: %-48s %s new limit / about %s old limit (whole-tensor difference to the wrong evaluator, not the fp32 restatement)"
              % (family, mode, name, "fails" if bad else "PASSES", "passes" if all(old) else "fails"))
        if not bad:
            unseen.append(name)
    assert not unseen, "mutations the per-block limits do not see: %s" % unseen
