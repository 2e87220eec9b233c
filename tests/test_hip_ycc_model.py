"""InrGeometry.report_ycc / report_ycc_frames / report_ssim_luma and drivers.compress_ycc (N4 418) on untrained models built from
the goldens as tests/test_hip_ssim_list_model.py builds them: the figures equal the evaluator (tests/ycc_emul.py) applied to host
copies of the integers ops.recon_finish(want_int=True) delivers for the same sample and to the source, as floats."""
import math

import numpy as np
import pytest
import torch

import ssim_emul as S
import ycc_emul as E
from test_hip_extent_model import KW, _cifar
from test_hip_ssim_list_model import _patch3d
from test_hip_ssim_model import _delivered, _model
from test_hip_test_model import DEV

pytestmark = pytest.mark.gpu

from recombiner_amd import drivers, utils  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402

SEED = 5


def _seeded(call, *a, **kw):
    """predict draws noise: a report scores the sample _delivered forms"""
    torch.manual_seed(SEED)
    return call(*a, **kw)


def _psnr(sse, count, L):
    return math.inf if sse == 0 else 10.0 * math.log10((L * L * count) / sse)


def _want(q, src, mx, ss, L):
    """the evaluator's figures of delivered integers q against src, both [..., H, W, 3]: [..., 4] as nested lists"""
    sse = E.ycc_sse(np.asarray(q).astype(np.int64), np.asarray(src).astype(np.int64), mx.m, mx.off, L, ss)
    H, W = np.asarray(src).shape[-3:-1]
    Hc, Wc = E.chroma_size(H, W, ss)
    out = np.empty(sse.shape[:-1] + (4,))
    for idx in np.ndindex(*sse.shape[:-1]):
        y, cb, cr = (_psnr(int(sse[idx + (k,)]), c, L) for k, c in enumerate((H * W, Hc * Wc, Hc * Wc)))
        out[idx] = [y, cb, cr, (6.0 * y + cb + cr) / 8.0]
    return out.tolist()


@pytest.mark.parametrize("depth", [0, 10])
def test_images_on_the_grid_and_at_their_own_size(depth):
    """two images on the unpatched CIFAR golden geometry (32 x 32), then 27 x 30 inside it (odd chroma sizes), uint8 and 10-bit"""
    cfg, ck = _cifar()
    m, x = _model(cfg, "cifar", ck, 2)
    fmt = SampleFormat.u16(depth) if depth else SampleFormat.u8()
    L = E.peak(fmt.kind, fmt.depth)
    mx = utils.ycc_matrix("bt709", False, fmt)
    src = np.random.RandomState(3).randint(0, L + 1, size=(2, 32, 32, 3))
    sig = torch.from_numpy(src.astype(np.int16 if depth else np.uint8)).to(DEV)
    sig = sig.view(torch.uint16) if depth else sig
    for size in (None, (27, 30)):
        part, host = (sig, src) if size is None else (sig[:, :27, :30], src[:, :27, :30])
        q = _delivered(m, x, fmt, size=size)
        for ss in (2, 0):
            got = _seeded(m.report_ycc, x, part, mx, subsampling=ss, size=size, sample_format=fmt if depth else None)
            assert got.dtype == np.float64 and got.shape == (2, 4)
            assert got.tolist() == _want(np.stack(q), host, mx, ss, L), (size, ss)
            assert np.all(np.isfinite(got)) and np.all(got < 40.0)
    # a model scored against what it delivers: every sum is zero
    mine = torch.from_numpy(np.stack(_delivered(m, x, fmt)).astype(np.int16 if depth else np.uint8)).to(DEV)
    mine = mine.view(torch.uint16) if depth else mine
    assert np.all(np.isinf(_seeded(m.report_ycc, x, mine, mx, sample_format=fmt if depth else None)))


def test_luma_ssim_is_the_existing_scorer_on_the_luma_planes():
    cfg, ck = _cifar()
    m, x = _model(cfg, "cifar", ck, 2)
    mx = utils.ycc_matrix("bt601", True, None)
    src = np.random.RandomState(4).randint(0, 256, size=(2, 28, 30, 3)).astype(np.uint8)
    got = _seeded(m.report_ssim_luma, x, torch.from_numpy(src).to(DEV), mx, size=(28, 30))
    q = np.stack(_delivered(m, x, SampleFormat.u8(), size=(28, 30)))
    ya, yb = (E.rgb_to_ycc(t.astype(np.int64), mx.m, mx.off, 255, 0)[0][..., None] for t in (q, src))
    want = [S.ssim_figure(S.sums(a, b, 255, 1), 28, 30) for a, b in zip(ya, yb)]
    assert got.dtype == np.float64 and got.tolist() == want


@pytest.fixture(scope="module")
def video():
    cfg, ck = _patch3d()
    assert utils.preset_grid(cfg) == ([1, 2, 2], [24, 16, 16]) and cfg["output_dim"] == 3
    m, x = _model(cfg, "video", ck, 2)
    return cfg, m, x


def test_frames_of_clips(video):
    """2 clips of 24 x 32 x 32 on the 3-D patched golden geometry, then of 20 x 27 x 30 inside it"""
    cfg, m, x = video
    mx = utils.ycc_matrix("bt709", False, None)
    src = np.random.RandomState(11).randint(0, 256, size=(2, 24, 32, 32, 3)).astype(np.uint8)
    sig = torch.from_numpy(src).to(DEV)
    got = _seeded(m.report_ycc_frames, x, sig, mx)
    q = np.stack(_delivered(m, x, SampleFormat.u8()))
    assert got.shape == (2, 24, 4) and got.dtype == np.float64 and got.tolist() == _want(q, src, mx, 2, 255)
    size = (20, 27, 30)
    got = _seeded(m.report_ycc_frames, x, sig[:, :20, :27, :30], mx, subsampling=1, size=size)
    q = np.stack(_delivered(m, x, SampleFormat.u8(), size=size))
    assert got.shape == (2, 20, 4) and got.tolist() == _want(q, src[:, :20, :27, :30], mx, 1, 255)
    luma = _seeded(m.report_ssim_luma_frames, x, sig, mx)
    assert luma.shape == (2, 24) and np.all(luma < 1.0) and np.all(luma > -1.0)


def test_what_the_reports_refuse(video):
    cfg, m, x = video
    mx = utils.ycc_matrix("bt709", False, None)
    u8 = torch.zeros(2, 24, 32, 32, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="integers"):
        m.report_ycc_frames(x, u8.float(), mx)
    with pytest.raises(ValueError, match="sample_format"):
        m.report_ycc_frames(x, u8.to(torch.int16), mx)
    with pytest.raises(ValueError, match="expected"):
        m.report_ycc_frames(x, u8[:, :23], mx)
    with pytest.raises(ValueError, match="2-D presets"):
        m.report_ycc(x, u8[:, 0], mx)
    with pytest.raises(ValueError, match="2-D presets"):
        m.report_ssim_luma(x, u8[:, 0], mx)
    with pytest.raises(ValueError, match="formed for"):
        m.report_ycc_frames(x, u8, utils.ycc_matrix("bt709", False, SampleFormat.u16(10)))
    c2, ck2 = _cifar()
    m2, x2 = _model(c2, "cifar", ck2, 1)
    with pytest.raises(ValueError, match="3-D presets"):
        m2.report_ycc_frames(x2, u8[:1], mx)
    m2.dims = list(m2.dims[:-1]) + [1]
    with pytest.raises(ValueError, match="three channels needed"):
        m2.report_ycc(x2, torch.zeros(1, 32, 32, 1, dtype=torch.uint8, device=DEV), mx)


def _host_rgb(planes, mx, ss, L=255):
    y, cb, cr = (p.astype(np.int64) for p in planes)
    return E.ycc_to_rgb(y, cb, cr, mx.n, mx.o, L, ss).astype(np.uint8)


def test_the_driver_on_a_444_image():
    """planes of another size than the grid: converted, resized, coded; the appended figures are report_ycc of the returned model
    against the returned source, and everything in front is compress_resized on the host-converted RGB"""
    cfg, ck = _cifar()
    mx = utils.ycc_matrix("bt601", True, None)
    planes = [np.random.RandomState(20 + k).randint(0, 256, size=(2, 40, 48)).astype(np.uint8) for k in range(3)]
    torch.manual_seed(7)
    out = drivers.compress_ycc(cfg, "cifar", ck, [torch.from_numpy(p) for p in planes], 0, mx, **KW)
    torch.manual_seed(7)
    plain = drivers.compress_resized(cfg, "cifar", ck, torch.from_numpy(_host_rgb(planes, mx, 0)), **KW)
    assert len(out) == len(plain) + 1 == 4
    assert np.array_equal(np.asarray(out[0]), np.asarray(plain[0])) and torch.equal(out[2], plain[2])
    assert torch.equal(out[1].loc, plain[1].loc)
    model, resized, scores = out[1], out[2], out[3]
    assert scores.dtype == np.float64 and scores.shape == (2, 4) and np.all(np.isfinite(scores))
    x = utils.preset_inputs(cfg, DEV)[None].expand(2, -1, -1)
    torch.manual_seed(SEED)
    again = model.report_ycc(x, resized, mx, subsampling=0)
    q = np.stack(_delivered(model, x, SampleFormat.u8()))
    assert again.tolist() == _want(q, resized.cpu().numpy(), mx, 0, 255)
    assert model.compressed_mask_groupwise.all() and scores.tolist() == again.tolist()     # (every group coded: predict draws nothing)


def test_the_driver_on_a_tiny_i420_clip():
    cfg, ck = _patch3d()
    mx = utils.ycc_matrix("bt709", False, None)
    n, T, H, W = 1, 24, 36, 40
    raw = np.random.RandomState(30).randint(16, 236, size=(n * T * (H * W + 2 * (H // 2) * (W // 2)),)).astype(np.uint8)
    kw = dict(KW, n_epochs=2)
    torch.manual_seed(7)
    out = drivers.compress_ycc(cfg, "video", ck, torch.from_numpy(raw), "i420", mx, size=(n, T, H, W), **kw)
    frames = raw.reshape(n, T, -1)
    planes = [frames[..., :H * W].reshape(n, T, H, W), frames[..., H * W:H * W + H * W // 4].reshape(n, T, H // 2, W // 2),
              frames[..., H * W + H * W // 4:].reshape(n, T, H // 2, W // 2)]
    torch.manual_seed(7)
    plain = drivers.compress_resized(cfg, "video", ck, torch.from_numpy(_host_rgb(planes, mx, 2)), **kw)
    assert len(out) == len(plain) + 1 == 4
    assert np.array_equal(np.asarray(out[0]), np.asarray(plain[0])) and torch.equal(out[2], plain[2])
    assert torch.equal(out[1].loc, plain[1].loc)
    assert tuple(out[2].shape) == (1, 24, 32, 32, 3)
    scores = out[3]
    assert scores.dtype == np.float64 and scores.shape == (1, 24, 4) and np.all(np.isfinite(scores))
    model, resized = out[1], out[2]
    x = utils.preset_inputs(cfg, DEV)[None].expand(4, -1, -1)
    torch.manual_seed(SEED)
    again = model.report_ycc_frames(x, resized, mx, subsampling=2)
    q = np.stack(_delivered(model, x, SampleFormat.u8()))
    assert again.tolist() == _want(q, resized.cpu().numpy(), mx, 2, 255)
    assert model.compressed_mask_groupwise.all() and scores.tolist() == again.tolist()
    with pytest.raises(ValueError, match="size="):
        drivers.compress_ycc(cfg, "video", ck, torch.from_numpy(raw), "i420", mx, **KW)
