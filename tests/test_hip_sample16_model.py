"""16-bit signals end to end (drivers.compress_signals_any(sample_format=) -> version-3 bitstream -> bitstream.decode_signal_any) on the
small models and with the smallest settings of tests/test_hip_extent_model.py (16-bit mode, 4 optimisation epochs, 1 fine-tune epoch):
the targets that reach the optimiser are the evaluator's (tests/sample16_emul.py) bit for bit, the stream carries the extent and the
format, the decoder returns the format's integers at the signal's own size, and the distortion is the figure of that delivered signal."""
import os

import numpy as np
import pytest
import torch

import extent_emul as X
import recon_emul as E
import sample16_emul as Q
import signal_emul as S
from golden_util import load
from test_hip_extent_model import KW, _patch2d, _spied
from test_hip_recon_model import _checkpoint
from test_hip_test_model import DEV, build

pytestmark = pytest.mark.gpu

from recombiner_amd import bitstream, drivers, utils  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402


def _patch1d():
    d = load("test_patch1d.npz")
    cfg, _, m = build(d, "patch1d")
    return cfg, _checkpoint(d, cfg, m)


def psnr_sum_order_bound_db(n):
    """|metric_from_sse(a) - metric_from_sse(b)| in dB for two fp64 sums of the same n non-negative terms in different orders, one of
    them correctly rounded: the sums differ by at most n * 2^-53 relative (the bound of tests/test_hip_recon.py), PSNR = -10 log10(sse
    / n), and 10 log10(1 + e) <= 4.3430 e; the fp64 division, logarithm and product add a few ulps of a figure below 100 dB (1.5e-14
    each): 1e-12 covers them"""
    return 4.3430 * n * 2.0 ** -53 * 1.01 + 1e-12


@pytest.mark.parametrize("name", ["s16_clip", "u16_12_image"])
def test_16_bit_signals_end_to_end(name, tmp_path):
    """(a) one s16 clip of 410 samples on the 1-D patched golden geometry (patches of 160, level 2 groups 2): it fits to 4 patches, the
    third cut short and the last wholly padded; (b) one 12-bit 40 x 70 image on the 2-D patched golden (patches of 32 x 32): 2 x 4"""
    rng = np.random.RandomState(7)
    if name == "s16_clip":
        (cfg, ck), dataset, fmt, size, want_pn = _patch1d(), "audio", Q.S16, (410,), [4]
        q = rng.randint(-32768, 32768, size=(1, *size, 1)).astype(np.int16)
    else:
        (cfg, ck), dataset, fmt, size, want_pn = _patch2d(), "kodak", Q.u16(12), (40, 70), [2, 4]
        q = rng.randint(0, 4096, size=(1, *size, 3)).astype(np.uint16)
    f = SampleFormat(*fmt)
    n, Cc = q.shape[0], q.shape[-1]
    path = os.path.join(tmp_path, "a.rcb")
    (dist, model, fitted), seen = _spied(lambda: drivers.compress_signals_any(cfg, dataset, ck, torch.from_numpy(q), bitstream_path=path,
                                                                              sample_format=f, **KW))
    assert model.compressed_mask_groupwise.all()
    pn, ps = utils.preset_grid(fitted)
    assert pn == want_pn and ps == list(cfg["pixel_sizes"][:len(size)])
    # the targets that reach optimize_posteriors: the evaluator's edge-padded targets, bit for bit
    (x_seen, y_seen), = seen
    want_y = Q.targets(q, pn, ps, fmt, pad=True)
    assert y_seen.is_cuda and tuple(y_seen.shape) == want_y.shape == (n * int(np.prod(pn)), int(np.prod(ps)), Cc)
    assert np.array_equal(S.bits(y_seen.cpu().numpy()), S.bits(want_y))
    rows = y_seen.shape[0]
    # the stream: version 3, carrying the extent and the format; without the format the same model writes version 2
    blob = open(path, "rb").read()
    assert bitstream.unpack_header(blob) == dict(version=3, extent=tuple(size), sample_format=f)
    levels, extent = bitstream.unpack(blob)
    assert extent == tuple(size) and levels[0].shape[0] == rows
    assert blob == bitstream.encode(model, extent=size, sample_format=f)
    v2 = bitstream.encode(model, extent=size)
    assert bitstream.unpack_header(v2) == dict(version=2, extent=tuple(size), sample_format=None)
    assert v2 == bitstream.encode(model, extent=size, sample_format=SampleFormat.implied(dataset))
    assert all(np.array_equal(a, b) for a, b in zip(bitstream.unpack_indices(v2), levels))
    # the decoder: the format's integers at the signal's own size = `finish` of the patch-level decoder's output, cropped
    torch.manual_seed(77)
    got = bitstream.decode_signal_any(cfg, dataset, ck, blob, device=DEV, precision=1, as_integer=True)
    torch.manual_seed(77)
    y_dec = bitstream.decode(fitted, dataset, ck, blob, None, rows, device=DEV, precision=1)
    assert got.dtype == f.dtype and got.is_cuda and tuple(got.shape) == q.shape
    assert y_dec.dtype == torch.float32 and tuple(y_dec.shape) == tuple(y_seen.shape)
    want = Q.finish_whole(y_dec.cpu().numpy(), want_y, pn, ps, fmt, size=size)
    assert want["q"].dtype == q.dtype and np.array_equal(got.cpu().numpy(), want["q"])
    assert np.array_equal(S.bits(want["whole"]), S.bits(Q.to_target(want["q"], fmt)))          # (the lattice of the integers)
    torch.manual_seed(77)                                      # (one more decode each: once is enough)
    if name == "s16_clip":                                     # the fp32 form is the same lattice
        whole = bitstream.decode_signal_any(cfg, dataset, ck, blob, device=DEV, precision=1)
        assert whole.dtype == torch.float32 and np.array_equal(S.bits(whole.cpu().numpy()), S.bits(want["whole"]))
    else:                                                      # as_uint8 is the older name of as_integer
        again = bitstream.decode_signal_any(cfg, dataset, ck, blob, device=DEV, precision=1, as_uint8=True)
        assert again.dtype == f.dtype and np.array_equal(again.cpu().numpy(), want["q"])
    # the distortion: of the delivered signal, over the real samples only
    n_mean = int(np.prod(size)) * Cc
    want_dist = utils.metric_from_sse(want["sse"], n_mean, dataset)
    err, bound = abs(float(dist) - float(want_dist)), psnr_sum_order_bound_db(n_mean)
    print(f"{name} {size}: distortion {dist}, from the evaluator's sse {want_dist}, |diff| {err:.3g} dB, bound {bound:.3g} dB")
    assert isinstance(dist, float) and np.isfinite(dist) and err <= bound
    raw = utils.metric_from_sse(Q.finish_whole(y_dec.cpu().numpy(), want_y, pn, ps, Q.F32FMT, size=size)["sse"], n_mean, dataset)
    assert raw != want_dist                                   # (for audio: the reference's unrounded figure is another number)
    # a version-2 stream of the same model still decodes exactly as before: the preset's implied format
    torch.manual_seed(77)
    if dataset == "audio":
        old = bitstream.decode_signal_any(cfg, dataset, ck, v2, device=DEV, precision=1)
        crop = (slice(None),) + tuple(slice(0, s) for s in size)
        assert np.array_equal(S.bits(old.cpu().numpy()), S.bits(np.ascontiguousarray(E.stitch(y_dec.cpu().numpy(), pn, ps)[crop])))
        with pytest.raises(ValueError, match="no 8-bit form"):
            bitstream.decode_signal_any(cfg, dataset, ck, v2, device=DEV, precision=1, as_uint8=True)
    else:
        old = bitstream.decode_signal_any(cfg, dataset, ck, v2, device=DEV, precision=1, as_uint8=True)
        assert old.dtype == torch.uint8
        assert np.array_equal(old.cpu().numpy(), X.finish_crop(y_dec.cpu().numpy(), None, pn, ps, size, mode=0)["u8"])
    with pytest.raises(ValueError, match="decode_signal_any"):
        bitstream.decode_signal(fitted, dataset, ck, blob, None, rows, device=DEV, precision=1)


def test_16_bit_tensors_need_a_format():
    cfg, ck = _patch1d()
    pcm = torch.zeros(1, 410, 1, dtype=torch.int16)
    with pytest.raises(ValueError, match="sample_format"):
        drivers.compress_signals_any(cfg, "audio", ck, pcm, **KW)
    with pytest.raises(ValueError, match="sample_format"):
        drivers.compress_signals(cfg, "audio", ck, torch.zeros(1, 640, 1, dtype=torch.uint16), **KW)
