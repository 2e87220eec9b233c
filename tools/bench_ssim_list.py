"""Timing of rcb_ssim_list (N4 415) on one MI355X against the loop it replaces: one ops.ssim_sums call per image, which is what
utils.ssim_device did for a list before the list entry existed.  Both sides do the same kernel work; the list side does it in one
memset, scales - 1 pooling and `scales` SSIM launches plus one table upload, the loop in n times the launches and allocations.
  K  24 uint8 images of 768 x 512 x 3, every third one a portrait image passed as its transposed view, five scales
  M  24 uint8 images of seeded sizes between 256 and 1024 per side, five scales
  V  4 clips of 24 x 128 x 128 x 3 scored as 96 frames (ops.ssim_sums_frames) at one scale, against 96 single calls
  control  24 contiguous landscape images through the list entry against ONE batched rcb_ssim call: what the table lookup and the
           upload cost
Before anything is timed the sums of the two sides must be equal (torch.equal).  Host clock around each side's work, ending in a
device synchronise; the two sides alternate; medians over the repetitions.
Usage: python tools/bench_ssim_list.py [--reps 30] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recombiner_amd import ops  # noqa: E402


def pair(g, *shape):
    """a smooth uint8 image with noise and a disturbed copy of it, [*shape] on the device"""
    H, W = shape[-3], shape[-2]
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = 127.5 + 90.0 * torch.sin(yy / 23.0) * torch.cos(xx / 17.0)
    a = (base[..., None] + torch.randint(-20, 21, shape, generator=g)).clamp(0, 255).to(torch.uint8)
    b = (a.int() + torch.randint(-6, 7, shape, generator=g)).clamp(0, 255).to(torch.uint8)
    return a.cuda(), b.cuda()


def loop_of(a, b, scales):
    """one ssim_sums call per image -> the list of their sums (stacked only for the comparison, never inside the timing)"""
    return lambda: [ops.ssim_sums(x[None], y[None], scales=scales)[0] for x, y in zip(a, b)]


def workloads():
    g = torch.Generator().manual_seed(0)
    out = []
    # K: landscape 512 x 768; every third image is stored portrait (768 x 512) and passed as its transposed view
    a, b = [], []
    for k in range(24):
        if k % 3 == 2:
            x, y = pair(g, 768, 512, 3)
            a.append(x.transpose(0, 1)), b.append(y.transpose(0, 1))
        else:
            x, y = pair(g, 512, 768, 3)
            a.append(x), b.append(y)
    out.append(("K", "24 images of 768 x 512 x 3, every third a transposed portrait view, 5 scales",
                lambda a=a, b=b: ops.ssim_sums_list(a, b, scales=5), loop_of(a, b, 5), "loop of 24 ssim_sums calls"))
    # M: seeded sizes
    rng = np.random.default_rng(21)
    a, b = [], []
    for k in range(24):
        x, y = pair(g, int(rng.integers(256, 1025)), int(rng.integers(256, 1025)), 3)
        a.append(x), b.append(y)
    out.append(("M", "24 images of seeded sizes in 256 .. 1024 per side (%d .. %d pixels), 5 scales"
                % (min(x.shape[0] * x.shape[1] for x in a), max(x.shape[0] * x.shape[1] for x in a)),
                lambda a=a, b=b: ops.ssim_sums_list(a, b, scales=5), loop_of(a, b, 5), "loop of 24 ssim_sums calls"))
    # V: clips
    ca, cb = pair(g, 4, 24, 128, 128, 3)
    fa, fb = list(ca.flatten(0, 1)), list(cb.flatten(0, 1))
    out.append(("V", "4 clips of 24 x 128 x 128 x 3 as 96 frames, 1 scale",
                lambda: ops.ssim_sums_frames(ca, cb, scales=1).flatten(0, 1), loop_of(fa, fb, 1), "loop of 96 ssim_sums calls"))
    # control
    sa, sb = pair(g, 24, 512, 768, 3)
    la, lb = list(sa), list(sb)
    out.append(("control", "24 contiguous images of 768 x 512 x 3, 5 scales",
                lambda: ops.ssim_sums_list(la, lb, scales=5), lambda: ops.ssim_sums(sa, sb, scales=5)[0],
                "one batched ssim_sums call"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim_list needs the GPU: a timing taken anywhere else says nothing")
    if args.reps < 30:
        raise SystemExit("at least 30 repetitions")
    lines = ["tools/bench_ssim_list.py on one MI355X (gfx950): rcb_ssim_list (\"list\") against the calls it replaces (\"other\"); %d"
             % args.reps,
             "repetitions after 3 of warm-up, the two sides alternating; host clock around each side's work -- allocations, table upload,",
             "memset and launches included -- ending in a device synchronise.  The sums of the two sides were compared with torch.equal",
             "before anything was timed.",
             "device: %s" % torch.cuda.get_device_name(0)]
    for name, what, list_side, other_side, other_name in workloads():
        theirs = other_side()
        if not torch.equal(list_side(), torch.cat(theirs) if isinstance(theirs, list) else theirs):
            raise SystemExit("%s: the sums of the list call and of the %s differ: nothing timed" % (name, other_name))
        for _ in range(3):
            list_side(), other_side()
        torch.cuda.synchronize()
        times = {"list": [], "other": []}
        for _ in range(args.reps):
            for side, fn in (("list", list_side), ("other", other_side)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[side].append((time.perf_counter() - t0) * 1e3)
        t = {k: np.asarray(v) for k, v in times.items()}
        med = {k: float(np.median(v)) for k, v in t.items()}
        lines.append("%s: %s; other = %s.  sums equal." % (name, what, other_name))
        for side in ("list", "other"):
            lines.append("  %-5s median %.3f ms  (min %.3f, p90 %.3f)" % (side, med[side], t[side].min(), np.percentile(t[side], 90)))
        apart = t["list"].max() < t["other"].min() or t["other"].max() < t["list"].min()
        overlap = np.percentile(t["list"], 90) >= t["other"].min() and np.percentile(t["other"], 90) >= t["list"].min()
        lines.append("  list / other = %.3f  (%s)" % (med["list"] / med["other"],
                     "every repetition of one side is below every repetition of the other" if apart else
                     "the two sides' min .. p90 ranges overlap: the difference is inside the spread" if overlap else
                     "the min .. p90 ranges of the two sides do not overlap"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
