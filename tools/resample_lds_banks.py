"""Counts, by the bank rule of ds_read_b64 on gfx950 (64 dword banks; the two 32-lane halves of a wave are served one after the
other; distinct addresses on one bank cost one LDS cycle each), what the tap loop of csrc/resample.hip pays for its LDS reads: per
ratio, over every tile start phase, the LDS cycles per half-wave read relative to a conflict-free one -- worst and mean -- with the
span stored at idx (plain) and at idx + (idx >> a) (padded; 2^a the largest power of two in o / n, for the even whole ratios the
kernel pads).  No device needed:
    python tools/resample_lds_banks.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recombiner_amd import utils  # noqa: E402

TILE = 256
RATES = [(48000, 16000), (44100, 16000), (22050, 16000), (8000, 16000), (16000, 44100), (128000, 16000), (2, 1), (4, 1), (6, 1),
         (5, 1), (7, 2)]


def cycles(addr):
    """LDS cycles of one half-wave ds_read_b64 of the doubles at index addr (active lanes only)"""
    worst = 1
    for half in (0, 1):                                      # the two dwords of a double lie on neighbouring banks
        banks = {}
        for a in set(int(v) for v in addr):
            banks.setdefault((2 * a + half) % 64, set()).add(a)
        worst = max(worst, max(len(s) for s in banks.values()))
    return worst


def main():
    print("rates            o : n     rule    plain worst / mean   padded worst / mean")
    for rate_in, rate_out in RATES:
        o, n, first, count, _ = utils.resample_taps(rate_in, rate_out)
        even = o != n and o % (2 * n) == 0
        rule = "padded" if even else "plain"
        a = ((o // n) & -(o // n)).bit_length() - 1 if even else 31
        res = {}
        for name, shift in (("plain", 31), ("padded", a)):
            seen = []
            for p0 in range(0, n, max(1, n // 16)):          # tile start phases
                i = p0 + np.arange(TILE)
                m0 = (i // n) * o + first[i % n]
                r0 = m0 - m0[0]
                cnt = count[i % n]
                for h in range(TILE // 32):
                    lanes = slice(32 * h, 32 * h + 32)
                    for j in range(int(cnt[lanes].max())):
                        live = cnt[lanes] > j
                        r = r0[lanes][live] + j
                        seen.append(cycles(r + (r >> shift)))
            res[name] = (max(seen), float(np.mean(seen)))
        print("%6d -> %6d %4d : %-4d  %-6s  %5d / %.2f         %5d / %.2f" % (rate_in, rate_out, o, n, rule, *res["plain"], *res["padded"]))


if __name__ == "__main__":
    main()
