"""Timing of rcb_ssim (N4 414) on one MI355X against the same definition composed of torch operators on the same device: fp64
grouped conv2d with the 11 x 11 outer-product window on {a, b, a a, b b, a b}, the per-position formula, avg_pool2d between the
scales.  Case: 24 uint8 images of 768 x 512 x 3, five scales.  Before anything is timed the two sides' figures (SSIM and MS-SSIM
per image) must agree within 1e-10.  Host clock around each side's work, ending in a device synchronise; the two sides
alternate; medians over the repetitions.  Operation counts are computed from the shapes below.
Usage: python tools/bench_ssim.py [--reps 30] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recombiner_amd import ops, utils  # noqa: E402

FP64_PEAK = 78.6e12                    # vector fp64, FMA counted as two operations (the public specification of the MI355X)


def composition(a, b, scales):
    """the definition in torch operators -> (mean ssim, mean cs) per scale, each fp64 [n, C]; a, b uint8 [n, H, W, C]"""
    w = torch.from_numpy(utils.ssim_window()).to(a.device)
    Cc = a.shape[-1]
    k2 = torch.outer(w, w)[None, None].expand(5 * Cc, 1, 11, 11).contiguous()
    c1, c2 = utils.ssim_constants(utils.SampleFormat.u8())
    x, y = a.permute(0, 3, 1, 2).double(), b.permute(0, 3, 1, 2).double()
    out = []
    for s in range(scales):
        if s:
            x, y = torch.nn.functional.avg_pool2d(x, 2), torch.nn.functional.avg_pool2d(y, 2)
        m = torch.nn.functional.conv2d(torch.cat([x, y, x * x, y * y, x * y], 1), k2, groups=5 * Cc)
        ma, mb, maa, mbb, mab = m.split(Cc, 1)
        saa, sbb, sab = maa - ma * ma, mbb - mb * mb, mab - ma * mb
        cs = (2 * sab + c2) / (saa + sbb + c2)
        ssim = (2 * ma * mb + c1) / (ma * ma + mb * mb + c1) * cs
        out.append((ssim.mean((2, 3)), cs.mean((2, 3))))
    return out


def composition_figures(per_scale):
    ssim = per_scale[0][0].mean(1)
    wts = utils.MSSSIM_WEIGHTS
    ms = torch.ones_like(per_scale[0][0])
    for s, (m_ssim, m_cs) in enumerate(per_scale):
        ms = ms * torch.clamp(m_cs if s < len(per_scale) - 1 else m_ssim, min=0.0) ** wts[s]
    return ssim.cpu().numpy(), ms.mean(1).cpu().numpy()


def operations(n, H, W, Cc, scales):
    """fp64 multiplies and adds the definition needs, from the shapes: per filtered value 11 multiplies and 10 adds, five maps,
    a row pass over Hs x (Ws - 10) values and a column pass over the positions; 3 products per sample; 18 per position for the
    formula (the two divisions counted as one operation each)"""
    total = 0
    for s in range(scales):
        Hs, Ws = H >> s, W >> s
        pos = (Hs - 10) * (Ws - 10)
        total += n * Cc * (5 * 21 * (Hs * (Ws - 10) + pos) + 3 * Hs * Ws + 18 * pos)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim needs the GPU: a timing taken anywhere else says nothing")
    n, H, W, Cc, scales = 24, 512, 768, 3, 5
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = 127.5 + 90.0 * torch.sin(yy / 23.0) * torch.cos(xx / 17.0)
    a = (base[None, :, :, None] + torch.randint(-20, 21, (n, H, W, Cc), generator=g)).clamp(0, 255).to(torch.uint8).cuda()
    b = (a.cpu().int() + torch.randint(-6, 7, (n, H, W, Cc), generator=g)).clamp(0, 255).to(torch.uint8).cuda()

    def kernel():
        return ops.ssim_sums(a, b, scales=scales)[0]

    def torch_side():
        return composition(a, b, scales)

    sums = kernel()
    got_ssim, got_ms = utils.ssim_from_sums(sums, H, W), utils.msssim_from_sums(sums, H, W)
    want_ssim, want_ms = composition_figures(torch_side())
    err = max(float(np.abs(got_ssim - want_ssim).max()), float(np.abs(got_ms - want_ms).max()))
    if not err <= 1e-10:
        raise SystemExit("the torch composition and rcb_ssim disagree by %.3g: nothing timed" % err)
    for _ in range(3):
        kernel(), torch_side()
    torch.cuda.synchronize()
    times = {"rcb_ssim": [], "torch": []}
    for _ in range(args.reps):
        for name, fn in (("rcb_ssim", kernel), ("torch", torch_side)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    ops_n = operations(n, H, W, Cc, scales)
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = ["tools/bench_ssim.py on one MI355X (gfx950): %d uint8 images of %d x %d x %d, %d scales; %d repetitions, the two sides"
             % (n, W, H, Cc, scales, args.reps),
             "alternating; host clock around each side's work, ending in a device synchronise (the rcb_ssim side: ops.ssim_sums, i.e. the",
             "allocation of sums and workspace, the memset, %d pool and %d ssim launches)." % (scales - 1, scales),
             "device: %s" % torch.cuda.get_device_name(0),
             "figures of the two sides (SSIM and MS-SSIM per image) agree within %.3g (required: 1e-10); mean SSIM %.6f, mean MS-SSIM %.6f"
             % (err, float(got_ssim.mean()), float(got_ms.mean()))]
    for name in ("rcb_ssim", "torch"):
        t = np.asarray(times[name])
        lines.append("%-9s median %.3f ms  (min %.3f, p90 %.3f)" % (name, np.median(t), t.min(), np.percentile(t, 90)))
    lines.append("rcb_ssim / torch = %.3f" % (med["rcb_ssim"] / med["torch"]))
    est = ops_n / FP64_PEAK * 1e3
    lines.append("fp64 multiplies and adds of the definition, from the shapes: %.3g; at the %.1f TFLOP/s vector fp64 peak (FMA = 2) that is"
                 % (ops_n, FP64_PEAK / 1e12))
    lines.append("%.3f ms -- the call reaches %.1f %% of it (the definition forbids contraction, so half the peak is the ceiling of"
                 % (est, 100.0 * est / med["rcb_ssim"]))
    lines.append("separate multiplies and adds; the halo of the 16 x 16 tiles repeats 26 / 16 of the row pass).")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
