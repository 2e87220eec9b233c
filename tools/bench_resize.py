"""Timing of rcb_resize (N4 416) on one MI355X against the same step composed of torch operators on the same device: permute to
channel-first, convert to float, interpolate(mode="bilinear", antialias=True), round, clamp, convert to uint8, permute back.
Case: 32 uint8 clips of 24 x 240 x 320 x 3, centre-cropped to 240 x 240 (a view: utils.center_crop) and resized to 128 x 128 --
data/video.py:26-31 for 32 UCF-101 clips.  Before anything is timed the integers of the two sides must be within 1 of each other
(the composition filters in fp32).  Host clock around each side's work, ending in a device synchronise; the two sides alternate;
medians over the repetitions.
Usage: python tools/bench_resize.py [--reps 30] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recombiner_amd import ops, utils  # noqa: E402


def composition(view, size):
    """the step in torch operators; view uint8 [n, T, H, W, C] (any strides) -> uint8 [n, T, H_out, W_out, C] contiguous"""
    n, T, H, W, Cc = view.shape
    x = view.permute(0, 1, 4, 2, 3).reshape(n * T, Cc, H, W).float()
    y = torch.nn.functional.interpolate(x, size=size, mode="bilinear", antialias=True, align_corners=False)
    y = y.round().clamp(0, 255).to(torch.uint8)
    return y.reshape(n, T, Cc, *size).permute(0, 1, 3, 4, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize needs the GPU: a timing taken anywhere else says nothing")
    n, T, H, W, Cc, crop, size = 32, 24, 240, 320, 3, (240, 240), (128, 128)
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = 127.5 + 90.0 * torch.sin(yy / 23.0) * torch.cos(xx / 17.0)
    clips = (base[None, None, :, :, None] + torch.randint(-40, 41, (n, T, H, W, Cc), generator=g)).clamp(0, 255).to(torch.uint8).cuda()
    view = utils.center_crop(clips, crop, (2, 3))
    assert not view.is_contiguous()

    def kernel():
        return ops.resize(view, size)

    def torch_side():
        return composition(view, size)

    got, want = kernel(), torch_side()
    diff = (got.int() - want.int()).abs()
    worst, share = int(diff.max().item()), float((diff > 0).float().mean().item())
    if tuple(got.shape) != tuple(want.shape) or worst > 1:
        raise SystemExit("the torch composition and rcb_resize differ by %d: nothing timed" % worst)
    for _ in range(3):
        kernel(), torch_side()
    torch.cuda.synchronize()
    times = {"rcb_resize": [], "torch": []}
    for _ in range(args.reps):
        for name, fn in (("rcb_resize", kernel), ("torch", torch_side)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    moved = n * T * Cc * (crop[0] * crop[1] + size[0] * size[1])              # bytes: every sample of the crop in, every result out
    lines = ["tools/bench_resize.py on one MI355X (gfx950): %d uint8 clips of %d x %d x %d x %d, centre crop %d x %d (a view), resized"
             % (n, T, H, W, Cc, *crop),
             "to %d x %d; %d repetitions, the two sides alternating; host clock around each side's work, ending in a device"
             % (*size, args.reps),
             "synchronise (the rcb_resize side: ops.resize, i.e. the allocation of the output and the table, the tap tables on the",
             "host, their upload with its stream synchronise, one launch).",
             "device: %s" % torch.cuda.get_device_name(0),
             "integers of the two sides: largest difference %d (required: at most 1), share that differ %.5f (the composition"
             % (worst, share),
             "filters in fp32 and rounds the fp32 value)."]
    for name in ("rcb_resize", "torch"):
        t = np.asarray(times[name])
        lines.append("%-10s median %.3f ms  (min %.3f, p90 %.3f)" % (name, np.median(t), t.min(), np.percentile(t, 90)))
    lines.append("rcb_resize / torch = %.3f" % (med["rcb_resize"] / med["torch"]))
    lines.append("bytes the step has to move (the crop in, the result out, one byte per sample): %.1f MB -> %.1f GB/s at the kernel's"
                 % (moved / 1e6, moved / 1e9 / (med["rcb_resize"] / 1e3)))
    lines.append("median (the whole call, the host work included).")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
