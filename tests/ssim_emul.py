"""The SSIM / MS-SSIM definition of include/rcb.h (N4, 414) in numpy fp64, written from the definition and not from the kernel:
what rcb_ssim must give bit for bit.  Every numpy product and sum below is one IEEE fp64 operation on its own (numpy fuses
nothing), in the order the header fixes.

  window     11 taps, sigma 1.5, normalised                                  Evaluator.window
  constants  C1 = (0.01 L)^2, C2 = (0.03 L)^2                                Evaluator.constants
  filter     separable, last spatial axis first, taps ascending              Evaluator.filter2
  maps       per position and channel {ssim, cs}                             Evaluator.maps
  pooling    integer 2 x 2 block sums, a trailing odd row / column dropped   Evaluator.pool
  sums       Python-integer sums of rint(value * 2^36) per scale and channel Evaluator.sums
  figures    SSIM and MS-SSIM from those sums                                Evaluator.ssim_figure / msssim_figure

The steps are methods so that tests/test_ssim_emul_cpu.py can break one at a time (its mutants) and show which check notices."""
import numpy as np

TAPS = 11
FX = 1 << 36                                        # RCB_SSIM_FX_SCALE
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


class Evaluator:
    def window(self):
        k = np.arange(TAPS, dtype=np.float64)
        g = np.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2))
        return g / g.sum()

    def constants(self, L):
        return (0.01 * L) ** 2, (0.03 * L) ** 2

    def tap(self, v, k, n, axis):
        """the n samples that tap k multiplies, along `axis`"""
        return np.take(v, np.arange(k, k + n), axis=axis)

    def filter_axis(self, v, w, axis):
        n = v.shape[axis] - (TAPS - 1)
        acc = w[0] * self.tap(v, 0, n, axis)
        for k in range(1, TAPS):
            acc = acc + w[k] * self.tap(v, k, n, axis)
        return acc

    def filter2(self, v, w):
        """v [H, W, C] -> [H - 10, W - 10, C]: the last spatial axis first"""
        return self.filter_axis(self.filter_axis(v, w, 1), w, 0)

    def cs_numerator(self, sab, c2):
        return 2.0 * sab + c2

    def maps(self, a, b, L, div=1.0):
        """integer arrays a, b [H, W, C] (block sums at a coarser scale, `div` = 4^s then) -> (ssim, cs), fp64 [H-10, W-10, C]"""
        w = self.window()
        c1, c2 = self.constants(L)
        a = np.asarray(a).astype(np.float64) / div          # exact: div is a power of 4
        b = np.asarray(b).astype(np.float64) / div
        ma, mb = self.filter2(a, w), self.filter2(b, w)
        m_aa, m_bb, m_ab = self.filter2(a * a, w), self.filter2(b * b, w), self.filter2(a * b, w)
        maa, mbb, mab = ma * ma, mb * mb, ma * mb
        saa, sbb, sab = m_aa - maa, m_bb - mbb, m_ab - mab
        cs = self.cs_numerator(sab, c2) / ((saa + sbb) + c2)
        lum = (2.0 * mab + c1) / ((maa + mbb) + c1)
        return lum * cs, cs

    def pool(self, q):
        """integer [H, W, C] -> [H // 2, W // 2, C]: the sum of every 2 x 2 block, a trailing odd row / column dropped"""
        q = np.asarray(q).astype(np.int64)
        H2, W2 = q.shape[0] // 2, q.shape[1] // 2
        q = q[:2 * H2, :2 * W2]
        return q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2]

    def scale_maps(self, a, b, L, scales):
        """[(ssim, cs)] per scale 0 .. scales-1; ValueError when a scale has a side below 11"""
        a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
        out = []
        for s in range(scales):
            if s:
                a, b = self.pool(a), self.pool(b)
            if min(a.shape[0], a.shape[1]) < TAPS:
                raise ValueError("scale %d of the image is %d x %d: both sides must be at least %d"
                                 % (s, a.shape[0], a.shape[1], TAPS))
            out.append(self.maps(a, b, L, float(4 ** s)))
        return out

    def sums(self, a, b, L, scales=1):
        """Python integers [scales][C][2]: {sum rint(ssim * 2^36), sum rint(cs * 2^36)} over the positions"""
        out = []
        for ssim, cs in self.scale_maps(a, b, L, scales):
            per = []
            for c in range(ssim.shape[-1]):
                per.append([sum(int(v) for v in np.rint(m[..., c] * float(FX)).ravel()) for m in (ssim, cs)])
            out.append(per)
        return out

    @staticmethod
    def positions(H, W, s):
        return ((H >> s) - (TAPS - 1)) * ((W >> s) - (TAPS - 1))

    def ssim_figure(self, sums, H, W):
        """mean over scale-0 positions and channels"""
        total = sum(int(ch[0]) for ch in sums[0])
        return float(total) / float(FX) / float(self.positions(H, W, 0) * len(sums[0]))

    def channel_figure(self, means):
        """MS-SSIM of one channel from its five means (cs of scales 0 .. 3, ssim of scale 4)"""
        p = max(means[0], 0.0) ** MS_WEIGHTS[0]
        for s in range(1, 5):
            p = p * max(means[s], 0.0) ** MS_WEIGHTS[s]
        return p

    def msssim_figure(self, sums, H, W):
        if len(sums) != 5 or min(H, W) < TAPS << 4:
            raise ValueError("MS-SSIM takes five scales: both sides at least 176, got %d x %d with %d scales" % (H, W, len(sums)))
        C = len(sums[0])
        per = []
        for c in range(C):
            means = [float(int(sums[s][c][1 if s < 4 else 0])) / float(FX) / float(self.positions(H, W, s)) for s in range(5)]
            per.append(self.channel_figure(means))
        total = per[0]
        for v in per[1:]:
            total = total + v
        return total / float(C)


_E = Evaluator()
window, constants, maps, pool, scale_maps, sums = _E.window, _E.constants, _E.maps, _E.pool, _E.scale_maps, _E.sums
ssim_figure, msssim_figure, positions = _E.ssim_figure, _E.msssim_figure, _E.positions


def level_max(kind, depth):
    """L of a sample format: 255 for uint8 (kind 0), 2^depth - 1 for u16 (kind 2)"""
    return 255 if kind == 0 else (1 << depth) - 1


def batch_sums(a, b, L, scales=1):
    """a, b [n, H, W, C] -> numpy int64 [n, scales, C, 2], the layout of rcb_ssim's `sums`"""
    return np.asarray([sums(x, y, L, scales) for x, y in zip(a, b)], dtype=np.int64)


def batch_map(a, b, L):
    """a, b [n, H, W, C] -> fp64 [n, H-10, W-10, C, 2], the layout of rcb_ssim's `map`"""
    return np.stack([np.stack(maps(x, y, L), axis=-1) for x, y in zip(a, b)])
