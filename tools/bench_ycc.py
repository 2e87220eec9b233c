"""Timing of the Y'CbCr entries (ops.ycc_to_rgb, ops.ycc_sse: rcb_ycc_to_rgb, rcb_ycc_sse, ABI 418) at sizes a user runs:

  (a) 32 clips of 24 x 240 x 320 I420 frames in one buffer -> RGB;
  (b) ycc_sse at 4:2:0 on 32 clips of 24 x 128 x 128 x 3;
  (c) ycc_sse at 4:2:0 on 24 images of 512 x 768 x 3;

each against two baselines on the same tensors, the three sides alternating:

  torch   the same arithmetic composed from torch fp64 ops on the device (the header's order of operations, torch.round = half to
          even): the requirement is that the entry is faster than this.
  floor   a plain device copy (Tensor.copy_) that moves the same number of bytes as the entry reads plus writes.  The ratio is
          written down, not gated.

Before anything is timed the outputs are verified: the entry equals the torch composition on the whole workload, and both equal the
numpy evaluator (tests/ycc_emul.py) on the first signal.  Timing: a host clock around each side's work -- allocations and launches
included -- ending in a device synchronise; medians over the repetitions.
Usage: python tools/bench_ycc.py [--reps 30] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ycc_emul as E  # noqa: E402
from recombiner_amd import ops, utils  # noqa: E402


def quantise(v, L=255.0):
    return torch.round(torch.clamp(v, 0.0, L))


def torch_inverse(y, cb, cr, mx, ss):
    """rcb_ycc_to_rgb composed from torch fp64 ops (even sizes): replicate, subtract, three products and two sums per channel"""
    n, o = torch.from_numpy(mx.n).to(y.device), mx.o
    up = lambda c: c.repeat_interleave(2, dim=-1).repeat_interleave(2, dim=-2) if ss == 2 else c
    Y, Cb, Cr = y.double() - o[0], up(cb).double() - o[1], up(cr).double() - o[2]
    return torch.stack([quantise((n[k, 0] * Y + n[k, 1] * Cb) + n[k, 2] * Cr).to(torch.uint8) for k in range(3)], dim=-1)


def torch_forward(rgb, mx, ss):
    """rcb_rgb_to_ycc composed from torch fp64 ops (even sizes) -> the three planes as fp64 integers"""
    m, off = torch.from_numpy(mx.m).to(rgb.device), mx.off
    r, g, b = (rgb[..., k].double() for k in range(3))
    out = []
    for k in range(3):
        p = (m[k, 0] * r + m[k, 1] * g) + m[k, 2] * b
        if k and ss == 2:
            p = ((p[..., 0::2, 0::2] + p[..., 0::2, 1::2]) + (p[..., 1::2, 0::2] + p[..., 1::2, 1::2])) * 0.25
        out.append(quantise(p + off[k]))
    return out


def torch_sse(a, b, mx, ss):
    pa, pb = torch_forward(a, mx, ss), torch_forward(b, mx, ss)
    return torch.stack([((x - y) ** 2).sum(dim=(-2, -1)).to(torch.int64) for x, y in zip(pa, pb)], dim=-1)


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


def report(lines, title, res, moved_bytes):
    lines.append(title)
    for name in ("entry", "floor", "torch"):
        v = res[name]
        lines.append("  %-6s median %.3f ms  (min %.3f, p90 %.3f)%s" % (
            name, np.median(v), v.min(), np.percentile(v, 90),
            "" if name == "torch" else "  -> %.0f GB/s read + written at the median" % (moved_bytes / np.median(v) / 1e6)))
    e, f, t = (np.median(res[k]) for k in ("entry", "floor", "torch"))
    lines.append("  entry / floor = %.3f   entry / torch = %.3f   (%s than the torch composition)"
                 % (e / f, e / t, "FASTER" if e < t else "NOT faster"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ycc: needs a GPU (no fall-back)")
    dev = "cuda"
    mx = utils.ycc_matrix("bt709", False, None)
    lines = ["tools/bench_ycc.py, %s, device: %s" % (time.strftime("%Y-%m-%d"), torch.cuda.get_device_name(0)),
             "%d repetitions after 3 of warm-up, the three sides alternating; host clock around each side's work, ending in a device "
             "synchronise" % args.reps,
             "entry = ops.ycc_to_rgb / ops.ycc_sse; torch = the same arithmetic from torch fp64 ops on the device; floor = Tensor.copy_ "
             "moving the bytes the entry reads plus writes.  uint8, BT.709 limited range, 4:2:0.",
             "verified first: entry == torch composition on the whole workload, both == tests/ycc_emul.py on the first signal"]
    g = torch.Generator(device=dev).manual_seed(0)

    # (a) I420 -> RGB
    n, T, H, W = 32, 24, 240, 320
    raw = torch.randint(0, 256, (n * T * (H * W * 3 // 2),), device=dev, dtype=torch.uint8, generator=g)
    (y, cb, cr), ss = utils.yuv_planes(raw, n, T, H, W, "i420")
    got = ops.ycc_to_rgb(y, cb, cr, mx, ss)
    assert torch.equal(got, torch_inverse(y, cb, cr, mx, ss))
    want = E.ycc_to_rgb(*(p[0].cpu().numpy().astype(np.int64) for p in (y, cb, cr)), mx.n, mx.o, 255, ss)
    assert np.array_equal(got[0].cpu().numpy(), want.astype(np.uint8))
    moved = raw.numel() + got.numel()
    half = torch.empty(moved // 2, device=dev, dtype=torch.uint8)
    half2 = torch.empty_like(half)
    res = measure([("entry", lambda: ops.ycc_to_rgb(y, cb, cr, mx, ss)), ("floor", lambda: half2.copy_(half)),
                   ("torch", lambda: torch_inverse(y, cb, cr, mx, ss))], args.reps)
    report(lines, "(a) 32 clips of 24 x 240 x 320 I420 frames in one buffer -> RGB [32, 24, 240, 320, 3] (%.0f MB in, %.0f MB out)"
           % (raw.numel() / 1e6, got.numel() / 1e6), res, moved)
    del raw, y, cb, cr, got, half, half2

    # (b), (c) the per-plane squared error
    for title, shape in (("(b) ycc_sse at 4:2:0, 32 clips of 24 x 128 x 128 x 3", (32, 24, 128, 128, 3)),
                         ("(c) ycc_sse at 4:2:0, 24 images of 512 x 768 x 3", (24, 512, 768, 3))):
        a = torch.randint(0, 256, shape, device=dev, dtype=torch.uint8, generator=g)
        noise = torch.randint(-6, 7, shape, device=dev, dtype=torch.int16, generator=g)
        b = (a.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)
        got = ops.ycc_sse(a, b, mx, 2)
        assert torch.equal(got, torch_sse(a, b, mx, 2))
        want = E.ycc_sse(a[0].cpu().numpy().astype(np.int64), b[0].cpu().numpy().astype(np.int64), mx.m, mx.off, 255, 2)
        assert got[0].cpu().numpy().reshape(-1).tolist() == [int(v) for v in want.reshape(-1)]
        H, W = shape[-3], shape[-2]
        psnr = utils.psnr_ycc_from_sse(got, H, W, 2)
        moved = 2 * a.numel()
        other = torch.empty_like(a)
        res = measure([("entry", lambda: ops.ycc_sse(a, b, mx, 2)), ("floor", lambda: other.copy_(a)),
                       ("torch", lambda: torch_sse(a, b, mx, 2))], args.reps)
        report(lines, "%s (2 x %.0f MB read; mean PSNR-Y %.2f dB, (6 Y + Cb + Cr) / 8 %.2f dB)"
               % (title, a.numel() / 1e6, psnr[..., 0].mean(), psnr[..., 3].mean()), res, moved)
        del a, b, noise, other
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
