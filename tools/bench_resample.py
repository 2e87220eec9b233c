"""Timing of rcb_resample (N4 419) on one MI355X, ops.resample as a whole call, against
  (a) the same step composed of torch operators on the same device: int16 -> fp64 (and the channel mean), torchaudio's formulation
      of the filter (its clamped sinc kernel, zero padding of (width, width + o), conv1d with stride o), rint, clamp, int16 --
      independent of the code under test;
  (b) a device copy of the bytes the step has to move (every source sample in, every result out).
Workloads: 1024 mono clips of 132 300 s16 samples at 44 100 Hz -> 48 000 samples at 16 000 Hz (one rank's share of the audio
configuration the README quotes); 256 stereo clips of 144 000 samples at 48 000 Hz -> mono at 16 000 Hz; 8 : 1 on the first
workload's bytes.  Before anything is timed the integers of the two sides must be within 1 of each other (the composition sums in
another order).  Host clock around each side's work, ending in a device synchronise; the sides alternate; medians.
Usage: python tools/bench_resample.py [--reps 20] [--out FILE]"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recombiner_amd import ops  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402


def torchaudio_kernel(o, n, device):
    """torchaudio.functional._get_sinc_resample_kernel at its defaults for the reduced rates, fp64"""
    lowpass_filter_width, rolloff = 6, 0.99
    base_freq = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base_freq)
    idx = torch.arange(-width, width + o, dtype=torch.float64, device=device)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64, device=device)[:, None, None] / n + idx
    t *= base_freq
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t *= math.pi
    kernels = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64, device=device), t.sin() / t)
    kernels *= window * (base_freq / o)
    return kernels, width


def composition(pcm, o, n, kernel, width, mean, length):
    """pcm int16 [N, L, C] -> int16 [N, length, 1 or C] contiguous, in torch operators"""
    N, L, Cc = pcm.shape
    x = pcm.to(torch.float64)
    x = x.mean(dim=2, keepdim=True) if mean else x
    x = x.permute(0, 2, 1).reshape(-1, 1, L)
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (width, width + o)), kernel, stride=o)
    y = y.transpose(1, 2).reshape(x.shape[0], -1)[:, :length]
    y = torch.round(y).clamp_(-32768, 32767).to(torch.int16)
    return y.reshape(N, -1, length).permute(0, 2, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample needs the GPU: a timing taken anywhere else says nothing")
    s16 = SampleFormat.s16()
    g = torch.Generator().manual_seed(0)
    workloads = [("1024 mono clips, 44 100 -> 16 000 Hz", 1024, 132300, 1, 44100, 16000, None, 48000),
                 ("256 stereo clips -> mono, 48 000 -> 16 000 Hz", 256, 144000, 2, 48000, 16000, [0.5, 0.5], 48000),
                 ("1024 mono clips, 8 : 1", 1024, 132300, 1, 128000, 16000, None, None)]
    lines = ["tools/bench_resample.py on one MI355X (gfx950); %d repetitions, the sides alternating; host clock around each side's"
             % args.reps,
             "work, ending in a device synchronise (the rcb_resample side: ops.resample, i.e. the allocation of the output and the",
             "table, the taps on the host, their upload with its stream synchronise, one launch).",
             "device: %s" % torch.cuda.get_device_name(0)]
    for name, N, L, Cc, rate_in, rate_out, mix, length in workloads:
        d = math.gcd(rate_in, rate_out)
        o, n = rate_in // d, rate_out // d
        length = length or -(-n * L // o)
        t = torch.arange(L, dtype=torch.float32)
        tone = 9000.0 * torch.sin(t / 37.0) + 5000.0 * torch.sin(t / 3.1)
        pcm = (tone[None, :, None] + torch.randint(-6000, 6001, (N, L, Cc), generator=g)).clamp(-32768, 32767).to(torch.int16).cuda()
        kernel, width = torchaudio_kernel(o, n, pcm.device)

        def ours():
            return ops.resample(pcm, rate_in, rate_out, sample_format=s16, mix=mix, length=length)

        def torch_side():
            return composition(pcm, o, n, kernel, width, mix is not None, length)

        moved = 2 * (N * L * Cc + N * length)                # bytes: every source sample in, every result out
        half = torch.empty(moved // 2, dtype=torch.uint8, device=pcm.device)
        other = torch.empty_like(half)

        def copy():
            return other.copy_(half)

        got, want = ours(), torch_side()
        diff = (got.int() - want.int()).abs()
        worst, share = int(diff.max().item()), float((diff > 0).float().mean().item())
        if tuple(got.shape) != tuple(want.shape) or worst > 1:
            raise SystemExit("%s: the torch composition and rcb_resample differ by %d: nothing timed" % (name, worst))
        del got, want, diff
        sides = (("rcb_resample", ours), ("torch", torch_side), ("copy", copy))
        for _ in range(3):
            for _, fn in sides:
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k, _ in sides}
        for _ in range(args.reps):
            for k, fn in sides:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: float(np.median(v)) for k, v in times.items()}
        lines.append("")
        lines.append("%s: int16 [%d, %d, %d] -> [%d, %d, 1], %d : %d; integers of the two sides: largest difference %d, share that"
                     % (name, N, L, Cc, N, length, o, n, worst))
        lines.append("differ %.2g" % share)
        for k, _ in sides:
            v = np.asarray(times[k])
            lines.append("  %-12s median %.3f ms  (min %.3f, p90 %.3f)" % (k, np.median(v), v.min(), np.percentile(v, 90)))
        lines.append("  rcb_resample / torch = %.3f;  rcb_resample / copy = %.2f;  %.1f MB moved -> %.0f GB/s at the median of the whole call"
                     % (med["rcb_resample"] / med["torch"], med["rcb_resample"] / med["copy"], moved / 1e6,
                        moved / 1e9 / (med["rcb_resample"] / 1e3)))
        del pcm, half, other
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
