"""A/B of the per-signal I/O ends (rcb_signal_patch_ragged + rcb_recon_finish_ragged, one call each) against the loop of single calls
of the by-value entries (rcb_signal_patch_pad + rcb_recon_finish_crop, one pair per signal, with a transpose copy before and after
for the portraits), on a Kodak-like set: 24 uint8 signals of 768 x 512 x 3, a third of them portrait.

Both sides produce the targets y of all signals and, from them, the 8-bit signals in their own orientation; the outputs are compared
bit for bit before anything is timed.  Timing: a host clock around each side's work ending in a device synchronise, the two sides
alternating, medians over the repetitions.  Usage: python tools/bench_ragged.py [--reps 40] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from recombiner_amd import config, ops, utils  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged: needs a GPU (no fall-back)")
    dev = "cuda"
    n, C, long_, short = 24, 3, 768, 512
    fitted = utils.fit_config(config.configs["kodak"], (short, long_))
    lay = utils.signal_layout(fitted)
    g = torch.Generator().manual_seed(0)
    portrait = [k % 3 == 2 for k in range(n)]
    sigs = [torch.randint(0, 256, (long_, short, C) if p else (short, long_, C), generator=g, dtype=torch.uint8).to(dev) for p in portrait]
    sizes = [(short, long_)] * n

    def new():
        y = ops.signal_patch_ragged([s.transpose(0, 1) if p else s for s, p in zip(sigs, portrait)], lay)
        q, _, _, _ = ops.recon_finish_ragged(y, layout=lay, sizes=sizes, swap=portrait, want_int=True)
        return y, q

    def loop():
        ys, qs = [], []
        for s, p in zip(sigs, portrait):
            v = s.transpose(0, 1).contiguous() if p else s
            y = ops.signal_patch_pad(v[None], lay)
            q = ops.recon_finish(y, layout=lay, size=(short, long_), want_u8=True)[0][0]
            ys.append(y)
            qs.append(q.transpose(0, 1).contiguous() if p else q)
        return ys, qs

    (y_a, q_a), (y_b, q_b) = new(), loop()
    assert torch.equal(y_a.view(torch.int32), torch.cat(y_b).view(torch.int32))
    assert all(torch.equal(a, b) and torch.equal(a, s) for a, b, s in zip(q_a, q_b, sigs))       # and the round trip is exact
    times = {"ragged": [], "loop": []}
    for _ in range(5):
        new(), loop()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for name, fn in (("ragged", new), ("loop", loop)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    elems = n * long_ * short * C
    moved = elems * (1 + 4 + 4 + 1)                          # source, y written, y read, 8-bit output
    extra = sum(portrait) * long_ * short * C * 2 * 2         # the loop's transpose copies: read + write, before and after
    lines = ["%d uint8 signals of %d x %d x %d, %d of them portrait; grid %r patches of %r; %d repetitions, the two sides alternating"
             % (n, long_, short, C, sum(portrait), lay.patch_nums, lay.patch_size, args.reps),
             "outputs of the two sides equal bit for bit (targets and 8-bit signals); the 8-bit signals equal the sources",
             "device: %s" % torch.cuda.get_device_name(0)]
    for name, b in (("ragged", moved), ("loop", moved + extra)):
        t = np.array(times[name]) * 1e3
        lines.append("%-7s median %.3f ms  (min %.3f, p90 %.3f)  calls %d  bytes moved %d  -> %.0f GB/s at the median"
                     % (name, np.median(t), t.min(), np.percentile(t, 90), 2 if name == "ragged" else 2 * n + 2 * sum(portrait), b,
                        b / np.median(t) / 1e6))
    lines.append("ragged / loop = %.3f" % (np.median(times["ragged"]) / np.median(times["loop"])))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
