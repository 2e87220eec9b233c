"""InrGeometry.report_ssim on untrained models built from the goldens as tests/test_hip_extent_model.py builds them (no optimisation:
the figure of whatever the model delivers): the figure equals the evaluator (tests/ssim_emul.py) applied to the integers
ops.recon_finish(want_int=True) delivers for the same sample and to the source, as floats."""
import numpy as np
import pytest
import torch

import ssim_emul as E
from golden_util import load
from test_hip_extent_model import _cifar, _patch2d
from test_hip_test_model import DEV, build

pytestmark = pytest.mark.gpu

from recombiner_amd import drivers, ops, utils  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402

SEED = 5


def _model(cfg, dataset, ck, n_signals):
    pn, _ = utils.preset_grid(cfg)
    n_rows = n_signals * int(np.prod(pn))
    m = drivers.build_test_model(cfg, dataset, ck, n_rows, DEV)
    m.precision = 1
    return m, utils.preset_inputs(cfg, DEV)[None].expand(n_rows, -1, -1)


def _delivered(m, x, fmt, size=None, sizes=None):
    """the integers the model delivers for the sample that report_ssim scores (predict draws noise: the same seed)"""
    torch.manual_seed(SEED)
    with torch.no_grad():
        y = m.predict(x).detach().float().contiguous()
    if sizes is not None:
        q, _, _, _ = ops.recon_finish_ragged(y, layout=m.signal_layout(), sizes=sizes, sample_format=fmt, want_int=True)
        return [t.cpu().numpy() for t in q]
    q, _, _, _ = ops.recon_finish(y, layout=m.signal_layout(), size=size, sample_format=fmt, want_int=True)
    return list(q.cpu().numpy())


def _report(m, x, signals, **kw):
    torch.manual_seed(SEED)
    return m.report_ssim(x, signals, **kw)


def _host(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return (a.view(np.uint16) if a.dtype == np.int16 else a).astype(np.int64)


def _want(q, src, L, multiscale=False):
    out = []
    for a, b in zip(q, src):
        H, W = a.shape[:2]
        sums = E.sums(_host(a), _host(b), L, 5 if multiscale else 1)
        out.append(E.msssim_figure(sums, H, W) if multiscale else E.ssim_figure(sums, H, W))
    return out


@pytest.mark.parametrize("depth", [0, 12])
def test_unpatched_preset_at_the_signals_own_size(depth):
    """two 28 x 30 images on the unpatched CIFAR golden geometry (32 x 32), uint8 and 12-bit"""
    cfg, ck = _cifar()
    m, x = _model(cfg, "cifar", ck, 2)
    fmt = SampleFormat.u16(depth) if depth else SampleFormat.u8()
    L = E.level_max(fmt.kind, depth)
    src = np.random.RandomState(3).randint(0, L + 1, size=(2, 28, 30, 3))
    sig = torch.from_numpy(src.astype(np.int16 if depth else np.uint8)).to(DEV)
    if depth:
        sig = sig.view(torch.uint16)
    got = _report(m, x, sig, size=(28, 30), sample_format=fmt if depth else None)
    q = _delivered(m, x, fmt, size=(28, 30))
    assert q[0].shape == (28, 30, 3) and got.dtype == np.float64 and got.shape == (2,)
    assert got.tolist() == _want(q, src, L)
    assert np.all(got < 1.0) and np.all(got > -1.0)
    # ... and the figure of a model scored against what it delivers is exactly 1
    mine = torch.from_numpy(np.stack(q).view(np.int16) if depth else np.stack(q)).to(DEV)
    assert _report(m, x, mine.view(torch.uint16) if depth else mine, size=(28, 30), sample_format=fmt).tolist() == [1.0, 1.0]


def test_patched_preset_multiscale():
    """one 176 x 180 image on the 2-D patched golden geometry, fitted to 6 x 6 patches of 32 x 32"""
    cfg, ck = _patch2d()
    fitted = utils.fit_config(cfg, (176, 180))
    assert utils.preset_grid(fitted)[0] == [6, 6]
    m, x = _model(fitted, "kodak", ck, 1)
    Cc = fitted["output_dim"]
    yy, xx = np.meshgrid(np.arange(176), np.arange(180), indexing="ij")
    base = 127.5 + 100.0 * np.sin(yy / 9.0) * np.cos(xx / 7.0)
    src = np.stack([np.rint(base * (0.6 + 0.1 * c)) for c in range(Cc)], axis=-1).astype(np.uint8)[None]
    sig = torch.from_numpy(src).to(DEV)
    q = _delivered(m, x, SampleFormat.u8(), size=(176, 180))
    ms = _report(m, x, sig, size=(176, 180), multiscale=True)
    assert ms.shape == (1,) and ms.tolist() == _want(q, src, 255, multiscale=True)
    ss = _report(m, x, sig, size=(176, 180))
    assert ss.tolist() == _want(q, src, 255)
    # the signal on the model's whole grid, read through a window of a larger image (utils.signal_view's kind of view)
    big = torch.zeros(1, 200, 200, Cc, device=DEV, dtype=torch.uint8)
    big[:, 3:179, 5:185] = sig
    pad = torch.nn.functional.pad(sig.permute(0, 3, 1, 2).float(), (0, 12, 0, 16), mode="replicate").permute(0, 2, 3, 1).to(torch.uint8)
    whole = _report(m, x, pad)
    assert whole.tolist() == _want(_delivered(m, x, SampleFormat.u8()), pad.cpu().numpy(), 255)
    assert _report(m, x, big[:, 3:179, 5:185], size=(176, 180)).tolist() == ss.tolist()


def test_a_list_of_sizes_with_a_portrait_signal():
    """a 40 x 70 and a 64 x 64 signal and a 70 x 40 portrait one on one grid of 2 x 4 patches: the portrait signal goes in as
    compress_signal_list passes it, its transposed view with the landscape extent in `sizes`"""
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
    assert not views[2].is_contiguous()
    got = _report(m, x, views, sizes=sizes)
    q = _delivered(m, x, SampleFormat.u8(), sizes=sizes)
    want = _want(q, [src[0], src[1], src[2].transpose(1, 0, 2)], 255)
    assert got.shape == (3,) and got.tolist() == want
    # alone, with its own size, a signal has the same figure: the sums do not know the batch
    assert _report(m, x, torch.stack([views[2]] * 3), size=(40, 70))[2] == got[2]


def test_what_report_ssim_refuses():
    cfg, ck = _cifar()
    m, x = _model(cfg, "cifar", ck, 1)
    u8 = torch.zeros(1, 28, 30, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="integers"):
        m.report_ssim(x, u8.float(), size=(28, 30))
    with pytest.raises(ValueError, match="sample_format"):
        m.report_ssim(x, u8.to(torch.int16), size=(28, 30))
    with pytest.raises(ValueError, match="u8 and u16"):
        m.report_ssim(x, u8.to(torch.int16), size=(28, 30), sample_format=SampleFormat.s16())
    with pytest.raises(ValueError, match="too small"):
        m.report_ssim(x, u8, size=(28, 30), multiscale=True)
    with pytest.raises(ValueError, match="too small"):
        m.report_ssim(x, u8[:, :10], size=(10, 30))
    with pytest.raises(ValueError, match="expected"):
        m.report_ssim(x, u8, size=(28, 29))
    with pytest.raises(ValueError, match="exclude"):
        m.report_ssim(x, [u8[0]], size=(28, 30), sizes=[(28, 30)])
    d = load("test_patch1d.npz")
    _, n, m1 = build(d, "patch1d")
    with pytest.raises(ValueError, match="2-D"):
        m1.report_ssim(None, torch.zeros(1, 64, 1, dtype=torch.uint8, device=DEV))
