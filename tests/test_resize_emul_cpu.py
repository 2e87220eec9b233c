"""The definition of rcb_resize (include/rcb.h, N4 416) on the CPU: the evaluator tests/resize_emul.py against torch's fp64
interpolate(mode="bilinear", antialias=True, align_corners=False) -- on the CPU the operator torchvision's Resize runs -- and
against torch's native uint8 path (what the reference's loader runs); the C planner rcb_resize_taps against the evaluator's
taps bit for bit; utils.center_crop, the argument checks of utils.resize_to_preset and rcb_resize_table_bytes."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_emul as E
from golden_util import ROOT

from recombiner_amd import _lib, config, utils

# (H, W) -> (H_out, W_out); inputs np.random.RandomState(0).randint(0, 256, (2, 3, h, w))
CASES = [((240, 240), (128, 128)), ((240, 320), (128, 128)), ((171, 131), (128, 128)), ((100, 90), (128, 128)),
         ((37, 53), (16, 16)), ((16, 16), (16, 16)), ((129, 255), (128, 128)), ((7, 5), (16, 16))]
MISTAKES = [dict(antialias=False), dict(round_between=True), dict(half_pixel=False), dict(normalise=False)]
UNROUNDED_TOL = 1e-11                                        # (8.6e-14 observed)
TIE_WINDOW = 1e-9
TIE_SHARE = 1e-3                                             # (8.2e-5 observed at the worst)


def _src(hw):
    return np.random.RandomState(0).randint(0, 256, (2, 3, *hw))


_TORCH64 = {}


def _torch64(k):
    """torch's fp64 result of case k, unrounded [2, 3, H_out, W_out]: computed once"""
    if k not in _TORCH64:
        hw, size = CASES[k]
        _TORCH64[k] = F.interpolate(torch.from_numpy(_src(hw)).double(), size=size, mode="bilinear", antialias=True,
                                    align_corners=False).numpy()
    return _TORCH64[k]


def _compare(k, **switches):
    """the evaluator (with `switches`) against torch in fp64 on case k -> (largest difference of the unrounded values, share of
    integers that differ away from a tie, share of integers that differ within TIE_WINDOW of k + 1/2)"""
    hw, size = CASES[k]
    a = E.unrounded(_src(hw)[..., None], size, **switches)[..., 0]
    t = _torch64(k)
    diff = float(np.abs(a - t).max())
    qa, qt = np.rint(np.clip(a, 0, 255)), np.rint(np.clip(t, 0, 255))
    near_tie = np.abs(a - np.floor(a) - 0.5) <= TIE_WINDOW
    differ = qa != qt
    return diff, float((differ & ~near_tie).mean()), float((differ & near_tie).mean())


def _agrees(k, **switches):
    diff, off_tie, at_tie = _compare(k, **switches)
    return diff <= UNROUNDED_TOL and off_tie == 0.0 and at_tie <= TIE_SHARE


def test_evaluator_is_torchs_fp64_antialiased_bilinear():
    for k, (hw, size) in enumerate(CASES):
        diff, off_tie, at_tie = _compare(k)
        print("%s -> %s: unrounded |diff| %.3g, integers differing off a tie %.3g, at a tie %.3g" % (hw, size, diff, off_tie, at_tie))
        assert diff <= UNROUNDED_TOL and off_tie == 0.0 and at_tie <= TIE_SHARE, (hw, size)


@pytest.mark.parametrize("mistake", MISTAKES, ids=lambda m: next(iter(m)))
def test_each_deliberate_mistake_fails_that_comparison(mistake):
    failed = [CASES[k] for k in range(len(CASES)) if not _agrees(k, **mistake)]
    print("%r fails on %d of %d cases" % (mistake, len(failed), len(CASES)))
    assert failed


def test_first_axis_first_differs_in_the_last_bits_only():
    k = CASES.index(((37, 53), (16, 16)))
    hw, size = CASES[k]
    a = E.unrounded(_src(hw)[..., None], size)
    b = E.unrounded(_src(hw)[..., None], size, first_axis_first=True)
    assert not np.array_equal(a.view(np.int64), b.view(np.int64)) and np.abs(a - b).max() < 1e-11
    assert _agrees(k, first_axis_first=True)                 # (torch's fp64 comparison cannot tell the two orders apart)


def test_distance_to_torchs_uint8_path():
    """what the reference's loader runs: fixed-point weights and a rounding to uint8 between the passes.  Never more than one
    step from the definition; the share of samples that differ is recorded (printed; with RCB_WRITE_PROFILES=1 written to
    profiles/r22_resize_vs_uint8_path.txt, which is how that file was made), not asserted"""
    lines = ["# rcb_resize's definition (tests/resize_emul.py: fp64, one rounding) against torch's native uint8 path of",
             "# interpolate(mode='bilinear', antialias=True) on the CPU -- fixed-point weights, a rounding to uint8 between the",
             "# two passes; inputs np.random.RandomState(0).randint(0, 256, (2, 3, h, w)).  Written by",
             "# tests/test_resize_emul_cpu.py::test_distance_to_torchs_uint8_path with RCB_WRITE_PROFILES=1 (torch %s)."
             % torch.__version__.split("+")[0],
             "# case                     samples   differ   share    largest difference"]
    for hw, size in CASES:
        src = _src(hw)
        mine = E.resize(src[..., None], size)[..., 0].astype(np.int64)
        theirs = F.interpolate(torch.from_numpy(src.astype(np.uint8)), size=size, mode="bilinear", antialias=True,
                               align_corners=False).numpy().astype(np.int64)
        d = np.abs(mine - theirs)
        lines.append("%-26s %7d  %7d   %.4f   %d" % ("%dx%d -> %dx%d" % (*hw, *size), d.size, int((d > 0).sum()),
                                                      float((d > 0).mean()), int(d.max())))
        assert d.max() <= 1, (hw, size)
    print("\n".join(lines))
    if os.environ.get("RCB_WRITE_PROFILES"):                 # (a plain run leaves the tree as it is: the figures are in the output)
        with open(os.path.join(ROOT, "profiles", "r22_resize_vs_uint8_path.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


# ---------------------------------------------------------------------------------------------------
# the C planner
# ---------------------------------------------------------------------------------------------------
PAIRS = [(a, b) for a in range(1, 41) for b in range(1, 41)] + [(240, 128), (320, 128), (512, 32), (513, 32), (768, 512), (5, 4096)]


def _planner(n_in, n_out, max_taps=E.MAX_TAPS):
    """rcb_resize_taps -> (return code, first, count, w); the arrays keep their sentinels where nothing was written"""
    lib = _lib.load()
    first, count = np.full(n_out, -7, dtype=np.int32), np.full(n_out, -7, dtype=np.int32)
    w = np.full((n_out, max_taps), -7.0, dtype=np.float64)
    rc = lib.rcb_resize_taps(n_in, n_out, ctypes.c_void_p(first.ctypes.data), ctypes.c_void_p(count.ctypes.data),
                             ctypes.c_void_p(w.ctypes.data), max_taps)
    return rc, first, count, w


def test_planner_is_the_evaluators_taps_bit_for_bit():
    refused = 0
    for n_in, n_out in PAIRS:
        rc, first, count, w = _planner(n_in, n_out)
        if n_in > 16 * n_out:
            refused += 1
            assert rc == -3 and np.all(first == -7) and np.all(w == -7.0), (n_in, n_out)
            with pytest.raises(_lib.RcbError, match="16 : 1"):
                utils.resize_taps(n_in, n_out)
            continue
        ef, ec, ew = E.taps(n_in, n_out)
        assert rc == int(ec.max()), (n_in, n_out)
        assert np.array_equal(first, ef) and np.array_equal(count, ec), (n_in, n_out)
        assert np.array_equal(w.view(np.int64), ew.view(np.int64)), (n_in, n_out)
        uf, uc, uw = utils.resize_taps(n_in, n_out)
        assert uf.dtype == np.int32 and uw.shape == (n_out, 33)
        assert np.array_equal(uf, ef) and np.array_equal(uc, ec) and np.array_equal(uw.view(np.int64), ew.view(np.int64))
        # the properties
        assert np.all(count >= 1) and np.all(first >= 0) and np.all(first + count <= n_in), (n_in, n_out)
        for i in range(n_out):
            assert abs(math.fsum(w[i, :count[i]]) - 1.0) <= 2 * 2.0 ** -52, (n_in, n_out, i)
            assert np.all(w[i, count[i]:].view(np.int64) == 0), (n_in, n_out, i)          # padded with +0.0
        if n_in == n_out:
            assert np.all(count == 1) and np.array_equal(first, np.arange(n_out)) and np.all(w[:, 0] == 1.0)
    assert refused > 0 and (513, 32) in PAIRS
    assert _planner(240, 128)[0] == 4 and _planner(512, 32)[0] == 32 and max(_planner(a, b)[0] for a, b in PAIRS) <= E.MAX_TAPS


def test_what_the_planner_refuses():
    rc, first, _, w = _planner(240, 128, max_taps=3)         # rows too short for the 4 taps of 240 -> 128
    assert rc == -2 and np.all(first == -7) and np.all(w == -7.0)
    assert _planner(240, 128, max_taps=4)[0] == 4
    lib = _lib.load()
    one = np.zeros(40, dtype=np.float64)
    p = ctypes.c_void_p(one.ctypes.data)
    assert lib.rcb_resize_taps(0, 1, p, p, p, 33) == -2 and lib.rcb_resize_taps(1, 0, p, p, p, 33) == -2
    assert lib.rcb_resize_taps(4, 4, None, p, p, 33) == -1 and lib.rcb_resize_taps(4, 4, p, p, None, 33) == -1
    assert lib.rcb_resize_taps(17, 1, p, p, p, 33) == -3 and lib.rcb_resize_taps(16, 1, p, p, p, 33) == 16


def test_table_bytes():
    lib = _lib.load()
    for (H, W), (Ho, Wo) in CASES + [((272, 40), (17, 20)), ((5, 20), (4096, 5))]:
        ky, kx = int(E.taps(H, Ho)[1].max()), int(E.taps(W, Wo)[1].max())
        assert lib.rcb_resize_table_bytes(H, W, Ho, Wo) == 8 * (Ho * (1 + ky) + Wo * (1 + kx)), (H, W, Ho, Wo)
    assert lib.rcb_resize_table_bytes(16, 16, 16, 16) == 8 * 2 * 16 * 2
    for bad in ((0, 4, 4, 4), (4, 4, 0, 4), (4, 4, 4, -1), (513, 4, 32, 4), (4, 513, 4, 32)):
        assert lib.rcb_resize_table_bytes(*bad) == -1, bad


# ---------------------------------------------------------------------------------------------------
# the views around the kernel
# ---------------------------------------------------------------------------------------------------
def test_center_crop_is_torchvisions_rule():
    t = torch.arange(2 * 11 * 14 * 3).reshape(2, 11, 14, 3)
    for h, w in ((11, 14), (10, 13), (9, 12), (8, 9), (1, 1), (6, 14)):        # odd and even margins, halves rounded to even
        top, left = int(round((11 - h) / 2.0)), int(round((14 - w) / 2.0))
        assert (top, left) == (E.center_crop_start(11, h), E.center_crop_start(14, w))
        v = utils.center_crop(t, (h, w), (1, 2))
        assert torch.equal(v, t[:, top:top + h, left:left + w]) and v.data_ptr() == t[:, top:, left:].data_ptr()
        assert torch.equal(utils.center_crop(t, (h, w), (-3, -2)), v)
    assert [E.center_crop_start(n, 4) for n in (4, 5, 6, 7, 8, 9)] == [0, 0, 1, 2, 2, 2]       # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert torch.equal(utils.center_crop(t, (5,), (2,)), t[:, :, 4:9])
    with pytest.raises(ValueError, match="crop asks for"):
        utils.center_crop(t, (12, 14), (1, 2))
    with pytest.raises(ValueError, match="crop asks for"):
        utils.center_crop(t, (0, 14), (1, 2))
    with pytest.raises(ValueError, match="sizes for"):
        utils.center_crop(t, (4, 4), (1,))


def test_what_resize_to_preset_refuses():
    """the argument checks come before anything touches a device: CPU tensors reach them"""
    video, kodak = config.configs["video"], config.configs["kodak"]
    pn, ps = utils.preset_grid(video)
    T = pn[0] * ps[0]
    clip = torch.zeros(1, T + 1, 30, 40, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="frames"):
        utils.resize_to_preset(video, clip[:, :T - 1])
    with pytest.raises(ValueError, match="channels"):
        utils.resize_to_preset(video, clip[..., :2])
    with pytest.raises(ValueError, match="channels"):
        utils.resize_to_preset(video, clip, channels_first=True)
    with pytest.raises(ValueError, match="crop asks for"):
        utils.resize_to_preset(video, clip, crop=(31, 30))
    with pytest.raises(ValueError, match="crop asks for"):
        utils.resize_to_preset(kodak, torch.zeros(1, 40, 30, 3, dtype=torch.uint8), crop=(31, 30))    # (swapped first: 30 x 40)
    with pytest.raises(ValueError, match="axes"):
        utils.resize_to_preset(video, clip[0])
    with pytest.raises(ValueError, match="crop is"):
        utils.resize_to_preset(video, clip, crop=(30,))
    with pytest.raises(ValueError, match="data_dim"):
        utils.resize_to_preset(config.configs["audio"], torch.zeros(1, 100, 1))
