"""InrGeometry.report_ssim(sizes=) through the one-call list entry and InrGeometry.report_ssim_frames (N4 415) on untrained models
built from the goldens as tests/test_hip_ssim_model.py builds them: the figures equal the evaluator (tests/ssim_emul.py) applied
to the integers ops.recon_finish(want_int=True) delivers for the same sample and to the source, as floats."""
import numpy as np
import pytest
import torch

from golden_util import load
from test_hip_extent_model import _cifar, _patch2d
from test_hip_recon_model import _checkpoint
from test_hip_ssim_model import _delivered, _model, _report, _want
from test_hip_test_model import DEV, build

pytestmark = pytest.mark.gpu

from recombiner_amd import ops, utils  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402

SEED = 5


def _patch3d():
    d = load("test_patch3d.npz")
    cfg, _, m = build(d, "patch3d")
    return cfg, _checkpoint(d, cfg, m)


def _report_frames(m, x, signals, **kw):
    torch.manual_seed(SEED)
    return m.report_ssim_frames(x, signals, **kw)


def _want_frames(q, src, L):
    """the evaluator per frame: q, src [n][T, H, W, C]"""
    return [_want(list(clip), list(s), L) for clip, s in zip(q, src)]


def test_a_list_of_sizes_is_scored_in_one_call(monkeypatch):
    """the list of tests/test_hip_ssim_model.py (a 40 x 70, a 64 x 64 and a transposed 70 x 40 signal on 2 x 4 patches): the
    evaluator's figures, from ONE ssim_sums_list call and no ssim_sums call"""
    cfg, ck = _patch2d()
    fitted = utils.fit_config(cfg, (40, 70))
    assert utils.preset_grid(fitted)[0] == [2, 4]
    m, x = _model(fitted, "kodak", ck, 3)
    Cc = fitted["output_dim"]
    rng = np.random.RandomState(8)
    src = [rng.randint(0, 256, size=(*s, Cc)).astype(np.uint8) for s in ((40, 70), (64, 64), (70, 40))]
    sigs = [torch.from_numpy(a).to(DEV) for a in src]
    sizes = [(40, 70), (64, 64), (40, 70)]
    views = [sigs[0], sigs[1], sigs[2].transpose(0, 1)]
    calls = {"list": 0, "single": 0}
    real_list, real_single = ops.ssim_sums_list, ops.ssim_sums

    def counted_list(*a, **kw):
        calls["list"] += 1
        return real_list(*a, **kw)

    def counted_single(*a, **kw):
        calls["single"] += 1
        return real_single(*a, **kw)
    monkeypatch.setattr(ops, "ssim_sums_list", counted_list)
    monkeypatch.setattr(ops, "ssim_sums", counted_single)
    got = _report(m, x, views, sizes=sizes)
    assert calls == {"list": 1, "single": 0}
    q = _delivered(m, x, SampleFormat.u8(), sizes=sizes)
    want = _want(q, [src[0], src[1], src[2].transpose(1, 0, 2)], 255)
    assert got.shape == (3,) and got.dtype == np.float64 and got.tolist() == want


@pytest.fixture(scope="module")
def video():
    cfg, ck = _patch3d()
    assert utils.preset_grid(cfg) == ([1, 2, 2], [24, 16, 16])
    m, x = _model(cfg, "video", ck, 2)
    return cfg, m, x


def test_frames_on_the_whole_grid_and_at_a_size(video):
    """2 clips of 24 x 32 x 32 on the 3-D patched golden geometry, then of 20 x 28 x 30 inside it"""
    cfg, m, x = video
    Cc = cfg["output_dim"]
    src = np.random.RandomState(11).randint(0, 256, size=(2, 24, 32, 32, Cc)).astype(np.uint8)
    sig = torch.from_numpy(src).to(DEV)
    got = _report_frames(m, x, sig)
    q = _delivered(m, x, SampleFormat.u8())
    assert q[0].shape == (24, 32, 32, Cc) and got.shape == (2, 24) and got.dtype == np.float64
    assert got.tolist() == _want_frames(q, src, 255)
    assert np.all(got < 1.0) and np.all(got > -1.0)
    # the same clips through strides: the frame axis innermost but for the channels
    moved = sig.permute(0, 2, 3, 1, 4).contiguous().permute(0, 3, 1, 2, 4)
    assert not moved.is_contiguous() and _report_frames(m, x, moved).tolist() == got.tolist()
    # at the signals' own size: T from `size`
    size = (20, 28, 30)
    part = sig[:, :20, :28, :30]
    got = _report_frames(m, x, part, size=size)
    q = _delivered(m, x, SampleFormat.u8(), size=size)
    assert q[0].shape == (20, 28, 30, Cc) and got.shape == (2, 20)
    assert got.tolist() == _want_frames(q, src[:, :20, :28, :30], 255)
    # ... and a model scored against what it delivers is exactly 1 in every frame
    mine = torch.from_numpy(np.stack(q)).to(DEV)
    assert _report_frames(m, x, mine, size=size).tolist() == [[1.0] * 20] * 2


def test_frames_of_12_bit_clips(video):
    cfg, m, x = video
    Cc = cfg["output_dim"]
    fmt = SampleFormat.u16(12)
    src = np.random.RandomState(12).randint(0, 4096, size=(2, 24, 32, 32, Cc))
    sig = torch.from_numpy(src.astype(np.int16)).to(DEV).view(torch.uint16)
    got = _report_frames(m, x, sig, sample_format=fmt)
    q = _delivered(m, x, fmt)
    assert q[0].dtype == np.uint16 and got.shape == (2, 24)
    assert got.tolist() == _want_frames(q, src, 4095)


def test_what_report_ssim_frames_refuses(video):
    cfg, m, x = video
    u8 = torch.zeros(2, 24, 32, 32, cfg["output_dim"], dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="integers"):
        m.report_ssim_frames(x, u8.float())
    with pytest.raises(ValueError, match="too small"):
        m.report_ssim_frames(x, u8, multiscale=True)
    with pytest.raises(ValueError, match="sample_format"):
        m.report_ssim_frames(x, u8.to(torch.int16))
    with pytest.raises(ValueError, match="u8 and u16"):
        m.report_ssim_frames(x, u8.to(torch.int16), sample_format=SampleFormat.s16())
    with pytest.raises(ValueError, match="too small"):
        m.report_ssim_frames(x, u8[:, :, :10], size=(24, 10, 32))
    with pytest.raises(ValueError, match="expected"):
        m.report_ssim_frames(x, u8[:, :23])
    with pytest.raises(ValueError, match="2-D presets"):
        m.report_ssim(x, u8[:, 0])                       # the image report still refuses a 3-D preset
    c2, ck2 = _cifar()
    m2, x2 = _model(c2, "cifar", ck2, 1)
    with pytest.raises(ValueError, match="3-D presets"):
        m2.report_ssim_frames(x2, torch.zeros(1, 1, 32, 32, 3, dtype=torch.uint8, device=DEV))
