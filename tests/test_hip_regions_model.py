"""InrGeometry.report_regions / report_regions_signals / report_frames and the `regions=` argument of the whole-signal drivers (N4
417) on untrained models built from the goldens as tests/test_hip_ssim_list_model.py builds them: every figure is utils.PSNR of the
host copies of that box, within psnr_bound_db."""
import numpy as np
import pytest
import torch

import region_emul as R
from test_hip_extent_model import KW, _cifar, _patch2d
from test_hip_ssim_list_model import _patch3d
from test_hip_ssim_model import _model
from test_hip_test_model import DEV
from test_recon_emul_cpu import psnr_bound_db

pytestmark = pytest.mark.gpu

from recombiner_amd import drivers, utils  # noqa: E402

SEED = 5


def _seeded(call, *a, **kw):
    """predict draws noise: every report of one comparison scores the same sample"""
    torch.manual_seed(SEED)
    return call(*a, **kw)


def _host_boxes(m, x, y, cfg, region, size, rounds=True):
    """utils.PSNR of every box of the host copies -> [n, *nr], and the element counts [*nr]"""
    with torch.no_grad():
        pred = _seeded(m.predict, x).detach().float().cpu().numpy()
    pn, ps = utils.preset_grid(cfg)
    wp, wt = R.whole_cropped(pred, pn, ps, size), R.whole_cropped(y.cpu().numpy(), pn, ps, size)
    extent = wp.shape[1:-1]
    counts = utils.region_counts(extent, region, wp.shape[-1])
    want = np.zeros((wp.shape[0], *counts.shape))
    for idx, sl in R.boxes(extent, region):
        for d in range(wp.shape[0]):
            want[(d,) + idx] = utils.PSNR(wt[(d,) + sl], wp[(d,) + sl], round=rounds)
    return want, counts


def _agree(got, want, counts):
    assert got.dtype == np.float64 and got.shape == want.shape and np.all(want < 60.0)
    bound = np.vectorize(psnr_bound_db)(counts)[None]
    print(f"worst |diff| / bound = {np.max(np.abs(got - want) / bound):.3g}")
    assert np.all(np.abs(got - want) <= bound)


@pytest.fixture(scope="module")
def photos():
    """two 40 x 70 images on the 2-D patched golden geometry fitted to them: 2 x 4 patches of 32 x 32, the last column wholly padded"""
    cfg, ck = _patch2d()
    fitted = utils.fit_config(cfg, (40, 70))
    assert utils.preset_grid(fitted) == ([2, 4], [32, 32])
    m, x = _model(fitted, "kodak", ck, 2)
    sig = torch.from_numpy(np.random.RandomState(8).randint(0, 256, size=(2, 40, 70, fitted["output_dim"])).astype(np.uint8)).to(DEV)
    return fitted, m, x, sig


@pytest.mark.parametrize("region", ["patch", (16, 16), "row"])
def test_report_regions_counts_real_samples_only(photos, region):
    fitted, m, x, sig = photos
    size = (40, 70)
    y = m.patch_signals(sig, size=size)
    box = utils.region_of(fitted, region)
    got = _seeded(m.report_regions, x, y, region=region, size=size)
    assert got.shape == (2, *utils.region_grid(size, box))
    want, counts = _host_boxes(m, x, y, fitted, box, size)
    assert int(counts.sum()) == 40 * 70 * fitted["output_dim"]                # the padded column of patches is in no region
    _agree(got, want, counts)
    # against the whole signals: the same targets, the same figures
    assert np.array_equal(_seeded(m.report_regions_signals, x, sig, region=region, size=size), got)
    # without a size the regions tile the grid, padding and all
    full = _seeded(m.report_regions, x, y, region=region)
    assert full.shape == (2, *utils.region_grid((64, 128), box))
    want, counts = _host_boxes(m, x, y, fitted, box, None)
    _agree(full, want, counts)


@pytest.fixture(scope="module")
def video():
    cfg, ck = _patch3d()
    assert utils.preset_grid(cfg) == ([1, 2, 2], [24, 16, 16])
    m, x = _model(cfg, "video", ck, 2)
    sig = torch.from_numpy(np.random.RandomState(11).randint(0, 256, size=(2, 24, 32, 32, cfg["output_dim"])).astype(np.uint8)).to(DEV)
    return cfg, m, x, sig


def test_report_frames_and_the_batch_figure(video):
    cfg, m, x, sig = video
    y = m.patch_signals(sig)
    got = _seeded(m.report_frames, x, y)
    want, counts = _host_boxes(m, x, y, cfg, (1, 32, 32), None)
    assert got.shape == (2, 24) and counts.shape == (24, 1, 1)
    _agree(got, want.reshape(2, 24), counts.reshape(24))
    assert np.array_equal(_seeded(m.report_frames, x, sig), got)                  # whole clips are cut on the device first
    assert np.array_equal(_seeded(m.report_regions, x, y, region="frame").reshape(2, 24), got)
    # the fp64 mean of the frames' squared errors, weighted by their counts, is `report`'s batch figure
    n = np.broadcast_to(counts.reshape(1, 24).astype(np.float64), got.shape)
    mse = float((10.0 ** (-got / 10.0) * n).sum() / n.sum())
    batch = _seeded(m.report, x, y)
    assert isinstance(batch, float) and abs(-10.0 * np.log10(mse) - batch) <= 1e-12 * abs(batch)
    # ... which is not the video convention, the mean of the per-frame figures
    assert got.mean() != batch
    # at the clips' own size
    size = (20, 28, 30)
    part = sig[:, :20, :28, :30]
    got = _seeded(m.report_frames, x, part, size=size)
    yp = m.patch_signals(part, size=size)
    want, counts = _host_boxes(m, x, yp, cfg, (1, 32, 32), size)
    assert got.shape == (2, 20) and int(counts.sum()) == 20 * 28 * 30 * cfg["output_dim"]
    _agree(got, want.reshape(2, 20), counts.reshape(20))
    # patches of the codec: which patch is worst
    by_patch = _seeded(m.report_regions, x, y, region="patch")
    want, counts = _host_boxes(m, x, y, cfg, (24, 16, 16), None)
    assert by_patch.shape == (2, 1, 2, 2)
    _agree(by_patch, want, counts)


def test_what_the_region_reports_refuse(photos):
    fitted, m, x, sig = photos
    y = m.patch_signals(sig, size=(40, 70))
    with pytest.raises(ValueError, match="3-D"):
        m.report_frames(x, y)
    with pytest.raises(ValueError, match="3-D"):
        m.report_regions(x, y, region="frame")
    with pytest.raises(ValueError, match="region_of"):
        m.report_regions(x, y, region="tile")
    with pytest.raises(ValueError, match="box"):
        m.report_regions(x, y, region=(16,))


def test_the_drivers_append_the_figures_only_when_asked():
    cfg, ck = _cifar()
    u8 = torch.from_numpy(np.random.RandomState(7).randint(0, 256, size=(2, 28, 30, 3)).astype(np.uint8))
    plain = drivers.compress_signals_any(cfg, "cifar", ck, u8, **KW)
    asked = drivers.compress_signals_any(cfg, "cifar", ck, u8, regions=(16, 16), **KW)
    assert len(plain) == 3 and len(asked) == 4
    assert [type(v) for v in plain] == [type(v) for v in asked[:3]] and np.shape(plain[0]) == np.shape(asked[0]) == (2,)
    extra = asked[3]
    assert isinstance(extra, np.ndarray) and extra.dtype == np.float64 and extra.shape == (2, 2, 2)      # 28 x 30 by 16 x 16
    assert np.all(np.isfinite(extra)) and np.all(extra < 60.0)


def test_the_resizing_driver_appends_them_too():
    """a source of another size, resized to the grid first: the figures are those of the resized signal"""
    cfg, ck = _cifar()
    big = torch.from_numpy(np.random.RandomState(9).randint(0, 256, size=(2, 40, 48, 3)).astype(np.uint8))
    plain = drivers.compress_resized(cfg, "cifar", ck, big, **KW)
    asked = drivers.compress_resized(cfg, "cifar", ck, big, regions=(16, 16), **KW)
    assert len(plain) == 3 and len(asked) == 4 and [type(v) for v in plain] == [type(v) for v in asked[:3]]
    assert asked[3].dtype == np.float64 and asked[3].shape == (2, 2, 2) and np.all(np.isfinite(asked[3]))
