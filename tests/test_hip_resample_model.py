"""The callers of rcb_resample (N4 419) on the small 1-D patched model of the goldens, built as tests/test_hip_sample16_model.py
builds it: utils.resample_to_preset and drivers.compress_resampled on stereo 16-bit PCM clips "at 44.1 kHz", downmixed and brought
to the model's grid at "16 kHz" -- the returned source is ops.resample of the input and the evaluator's integers, it is what the
optimiser is given and what the figures are scored against, and the stream is that of a signal at the grid, which
bitstream.decode_signal decodes to int16."""
import math
import os

import numpy as np
import pytest
import torch

import resample_emul as E
import sample16_emul as Q
import signal_emul as S
from test_hip_extent_model import KW, _spied
from test_hip_sample16_model import _patch1d
from test_hip_test_model import DEV
from test_recon_emul_cpu import psnr_bound_db

pytestmark = pytest.mark.gpu

from recombiner_amd import bitstream, drivers, ops, utils  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402

RATES = (44100, 16000)
S16 = SampleFormat.s16()


def test_stereo_clips_are_resampled_coded_and_scored_at_the_grid(tmp_path):
    cfg, ck = _patch1d()
    pn, ps = utils.preset_grid(cfg)
    grid, n = pn[0] * ps[0], 2
    assert cfg["data_dim"] == 1 and cfg["output_dim"] == 1
    L = -(-grid * 441 // 160) + 57                           # a little more than the grid needs: the cut is not the source's end
    assert E.length(L, *RATES) > grid
    rng = np.random.RandomState(11)
    src = (6000.0 * rng.standard_normal((n, L, 2)).cumsum(axis=1) / np.sqrt(np.arange(1, L + 1))[None, :, None]).clip(-32768, 32767)
    src = src.astype(np.int16)
    want = E.resample(src, *RATES, taps_from=utils.resample_taps(*RATES), mix=[0.5, 0.5], length_out=grid)
    assert want.shape == (n, grid, 1) and want.dtype == np.int16
    pcm = torch.from_numpy(src)
    # the step alone: the evaluator's integers, from either storage order, and ops.resample of the input
    resampled = utils.resample_to_preset(cfg, pcm.to(DEV), RATES[0], sample_format=S16)
    assert resampled.dtype == torch.int16 and resampled.is_contiguous() and np.array_equal(resampled.cpu().numpy(), want)
    cf = torch.from_numpy(np.ascontiguousarray(src.transpose(0, 2, 1))).to(DEV)
    assert torch.equal(utils.resample_to_preset(cfg, cf, RATES[0], channels_first=True, sample_format=S16), resampled)
    assert torch.equal(ops.resample(pcm.to(DEV), *RATES, sample_format=S16, mix=[0.5, 0.5], length=grid), resampled)
    uneven = utils.resample_to_preset(cfg, pcm.to(DEV), RATES[0], mix=[1.0, 0.0], sample_format=S16)
    assert torch.equal(uneven, utils.resample_to_preset(cfg, pcm.to(DEV)[..., :1], RATES[0], mix=None, sample_format=S16))
    with pytest.raises(ValueError, match="compress_signals_any"):
        utils.resample_to_preset(cfg, pcm.to(DEV)[:, :L - 80], RATES[0], sample_format=S16)
    # the driver
    path = os.path.join(tmp_path, "a.rcb")
    (out, seen) = _spied(lambda: drivers.compress_resampled(cfg, "audio", ck, pcm, RATES[0], sample_format=S16, regions="patch",
                                                            bitstream_path=path, **KW))
    assert len(out) == 4
    dist, model, coded, by_patch = out
    assert torch.equal(coded, resampled) and model.compressed_mask_groupwise.all()
    (_, y_seen), = seen
    want_y = Q.targets(want, pn, ps, Q.S16)
    assert np.array_equal(S.bits(y_seen.cpu().numpy()), S.bits(want_y))
    n_rows = n * int(np.prod(pn))
    x = drivers._default_x(None, cfg, DEV, n_rows)
    # report_signals against the returned source gives the driver's figure (the preset's own, unrounded one) ...
    n_elems = n * grid
    figure = model.report(x, model.patch_signals(coded, sample_format=S16))
    print("compress_resampled %r, report against the returned source %r" % (dist, figure))
    assert isinstance(figure, float) and np.isfinite(dist) and abs(float(dist) - figure) <= psnr_bound_db(n_elems)
    # ... and, on the s16 lattice, the figure of the integers the decoder delivers
    blob = open(path, "rb").read()
    head = bitstream.unpack_header(blob)
    assert head["extent"] is None and head["sample_format"] == S16                            # a signal at the grid; no rate in it
    dec = bitstream.decode_signal(cfg, "audio", ck, blob, None, n_rows, device=DEV, precision=1, as_integer=True)
    assert dec.dtype == torch.int16 and tuple(dec.shape) == (n, grid, 1)
    on_lattice = model.report_signals(x, coded, sample_format=S16)
    d = Q.to_target(dec.cpu().numpy(), Q.S16).astype(np.float64) - Q.to_target(want, Q.S16).astype(np.float64)
    decoded = utils.metric_from_sse([math.fsum((d * d).reshape(-1))], n_elems, "audio")
    # encoder and decoder agree to 1e-5 in y (tests/test_hip_drivers.py) and a sample moves by at most one more step of 2^-16
    # where that crosses a rounding boundary: the rms error moves by at most that shift (triangle inequality), so
    # |d PSNR| <= -20 log10(1 - shift / rms), rms = 10^(-PSNR / 20)
    bound = -20.0 * math.log10(1.0 - (1e-5 + 2.0 ** -16) / 10.0 ** (-float(on_lattice) / 20.0))
    print("on the s16 lattice %r, the decoded integers against the returned source %r, bound %.3g dB" % (on_lattice, decoded, bound))
    assert np.isfinite(on_lattice) and abs(float(on_lattice) - float(decoded)) <= bound
    # regions= appended the per-patch figures of the resampled signal
    assert isinstance(by_patch, np.ndarray) and by_patch.dtype == np.float64 and by_patch.shape == (n, pn[0])
    assert np.all(np.isfinite(by_patch))
    again = model.report_regions_signals(x, coded, region="patch", sample_format=S16)
    assert np.array_equal(again, by_patch)
