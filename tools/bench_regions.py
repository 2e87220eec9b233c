"""Timing of the per-region squared error (ops.recon_regions: rcb_recon_regions, ABI 417) at sizes a user runs:

  (a) 32 clips of 24 x 128 x 128 x 3 on the video preset's grid (patches of 24 x 16 x 16), by frame;
  (b) 24 images of 768 x 512 x 3 on the kodak preset's grid (patches of 64 x 64), by patch and by tiles of 16 x 16;

each against two baselines on the same tensors, the three sides alternating:

  floor   ops.recon_finish returning only sse (one sum per signal): it reads the same bytes, so it is the time this kernel should
          sit near.  The ratio is written down, not gated.
  torch   the composition it replaces: recon_finish(want_whole) for both operands, the fp32 difference, the fp64 square, reshape
          and sum per region.

Before anything is timed the figures are checked: every sse_r against math.fsum of that region's exact fp64 terms (taken from the
torch composition's squares, on the host), within n_r * 2^-53 * sum(terms).  Timing: a host clock around each side's work --
allocations and launches included -- ending in a device synchronise; medians over the repetitions.
Usage: python tools/bench_regions.py [--reps 30] [--out FILE]"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from recombiner_amd import config, ops, utils  # noqa: E402


def composition(y, t, lay, region, want_terms=False):
    """the torch composition -> sse per region [n, *nr] (and the exact terms [n * n_regions, n_r]); the regions divide the grid here"""
    _, wv, _, _ = ops.recon_finish(y, layout=lay, mode=ops.RECON_8BIT, want_whole=True)
    _, wt, _, _ = ops.recon_finish(t, layout=lay, mode=ops.RECON_RAW, want_whole=True)
    d = (wt - wv).double()
    sq = d * d
    n, grid, C = sq.shape[0], sq.shape[1:-1], sq.shape[-1]
    split = [v for g, r in zip(grid, region) for v in (g // r, r)]
    sq = sq.reshape(n, *split, C)
    nd = len(grid)
    boxes = sq.permute(0, *[1 + 2 * i for i in range(nd)], *[2 + 2 * i for i in range(nd)], 1 + 2 * nd)      # [n, *nr, *region, C]
    sums = boxes.reshape(n, *[g // r for g, r in zip(grid, region)], -1).sum(-1)
    return (sums, boxes.reshape(-1, int(np.prod(region)) * C)) if want_terms else sums


def check(y, t, lay, region):
    sse_r, n_bad_r = ops.recon_regions(y, t, lay, region)
    sums, terms = composition(y, t, lay, region, want_terms=True)
    assert int(n_bad_r.abs().sum()) == 0 and sse_r.shape == sums.shape
    got, terms = sse_r.reshape(-1).cpu().numpy(), terms.cpu().numpy()
    worst = 0.0
    for g, row in zip(got, terms):
        exact = math.fsum(row)
        bound = row.size * 2.0 ** -53 * exact
        assert abs(g - exact) <= bound, (g, exact, bound)
        worst = max(worst, abs(g - exact) / bound)
    return got.size, terms.shape[1], worst


def measure(sides, reps):
    times = {name: [] for name, _ in sides}
    for _ in range(3):
        for _, fn in sides:
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return {name: np.array(v) * 1e3 for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regions: needs a GPU (no fall-back)")
    dev = "cuda"
    lines = ["tools/bench_regions.py, %s, device: %s" % (time.strftime("%Y-%m-%d"), torch.cuda.get_device_name(0)),
             "%d repetitions after 3 of warm-up, the three sides alternating; host clock around each side's work, ending in a device "
             "synchronise" % args.reps,
             "regions = ops.recon_regions; floor = ops.recon_finish, sse only (one sum per signal, the same bytes read); torch = "
             "recon_finish(want_whole) of both operands, fp32 difference, fp64 square, reshape, sum per region"]
    workloads = [("(a) 32 clips of 24 x 128 x 128 x 3", "video", 32, [("by frame", "frame")]),
                 ("(b) 24 images of 512 x 768 x 3", "kodak", 24, [("by patch", "patch"), ("by tiles of 16 x 16", (16, 16))])]
    g = torch.Generator(device=dev).manual_seed(0)
    for title, preset, n, cuts in workloads:
        lay = utils.signal_layout(config.configs[preset])
        per, P, C = int(np.prod(lay.patch_nums)), int(np.prod(lay.patch_size)), config.configs[preset]["output_dim"]
        t = torch.rand(n * per, P, C, device=dev, generator=g)
        y = (t + 0.05 * torch.randn(n * per, P, C, device=dev, generator=g)).contiguous()
        for what, by in cuts:
            region = utils.region_of(lay, by)
            n_regions, n_r, worst = check(y, t, lay, region)
            res = measure([("regions", lambda: ops.recon_regions(y, t, lay, region)),
                           ("floor", lambda: ops.recon_finish(y, t, layout=lay)),
                           ("torch", lambda: composition(y, t, lay, region))], args.reps)
            nbytes = 2 * y.numel() * 4
            lines.append("%s, grid of %r patches of %r, %s: %d regions of %d elements (%d workgroups of 256 threads); every sse_r within "
                         "n_r * 2^-53 * sum(terms) of fsum, worst error / bound %.3g"
                         % (title, lay.patch_nums, lay.patch_size, what, n_regions, n_r, n_regions * -(-n_r // 8192), worst))
            for name in ("regions", "floor", "torch"):
                v = res[name]
                lines.append("  %-7s median %.3f ms  (min %.3f, p90 %.3f)%s" % (
                    name, np.median(v), v.min(), np.percentile(v, 90),
                    "" if name == "torch" else "  -> %.0f GB/s of y + target at the median" % (nbytes / np.median(v) / 1e6)))
            lines.append("  regions / floor = %.3f   regions / torch = %.3f"
                         % (np.median(res["regions"]) / np.median(res["floor"]), np.median(res["regions"]) / np.median(res["torch"])))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
