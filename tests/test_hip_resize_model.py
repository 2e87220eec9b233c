"""The callers of rcb_resize (N4 416) on small models built from the goldens as tests/test_hip_ssim_list_model.py builds them:
utils.resize_to_preset on the 3-D patched golden geometry -- the resized clips are what patch_signals cuts and what report_signals /
report_ssim_frames score against -- and drivers.compress_resized on the 2-D patched one, from a portrait image larger than the
grid to a bitstream that bitstream.decode_signal decodes at the grid's size."""
import math
import os

import numpy as np
import pytest
import torch

import recon_emul as R
import resize_emul as E
import signal_emul as S
from test_hip_extent_model import KW, _patch2d, _spied
from test_hip_ssim_list_model import _patch3d, _report_frames, _want_frames
from test_hip_ssim_model import _delivered, _model
from test_hip_test_model import DEV
from test_recon_emul_cpu import psnr_bound_db

pytestmark = pytest.mark.gpu

from recombiner_amd import bitstream, drivers, utils  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402

SEED = 5


def test_clips_are_resized_to_the_video_geometry_and_scored_there():
    """uint8 clips [2, T + 2, 30, 40, C] -> the first T frames, centre-cropped to 30 x 30, resized to the grid's 32 x 32"""
    cfg, ck = _patch3d()
    pn, ps = utils.preset_grid(cfg)
    assert (pn, ps) == ([1, 2, 2], [24, 16, 16])
    T, G, Cc = 24, (32, 32), cfg["output_dim"]
    src = np.random.RandomState(31).randint(0, 256, size=(2, T + 2, 30, 40, Cc)).astype(np.uint8)
    clips = torch.from_numpy(src).to(DEV)
    resized = utils.resize_to_preset(cfg, clips, crop=(30, 30))
    assert resized.dtype == torch.uint8 and tuple(resized.shape) == (2, T, *G, Cc) and resized.is_contiguous()
    left = E.center_crop_start(40, 30)
    assert left == 5
    want = E.resize(src[:, :T, :, left:left + 30], G)
    assert np.array_equal(resized.cpu().numpy(), want)
    # channel-first clips, as a video library hands them over: the same bits
    cf = torch.from_numpy(np.ascontiguousarray(src.transpose(0, 4, 1, 2, 3))).to(DEV)
    assert torch.equal(utils.resize_to_preset(cfg, cf, crop=(30, 30), channels_first=True), resized)
    # what the model cuts from it: the evaluator's patch targets
    m, x = _model(cfg, "video", ck, 2)
    y = m.patch_signals(resized)
    assert np.array_equal(S.bits(y.cpu().numpy()), S.bits(S.targets(want, pn, ps)))
    # the distortion and the per-frame SSIM of an untrained model against the resized source: the existing evaluators
    torch.manual_seed(SEED)
    got = m.report_signals(x, resized)
    torch.manual_seed(SEED)
    with torch.no_grad():
        y_pred = m.predict(x).detach().float().cpu().numpy()
    fin = R.finish(y_pred, target=S.targets(want, pn, ps), patch_nums=pn, patch_size=ps, mode=0)
    n_elems = int(np.prod(want.shape[1:]))
    figure = utils.metric_from_sse(fin["sse"], n_elems, "video")
    print("report_signals %r, recon_emul %r" % (got, figure))
    assert isinstance(got, float) and abs(got - figure) <= psnr_bound_db(2 * n_elems)
    frames = _report_frames(m, x, resized)
    q = _delivered(m, x, SampleFormat.u8())
    assert frames.shape == (2, T) and frames.tolist() == _want_frames(q, want, 255)


def test_a_portrait_image_is_coded_at_the_grid_and_decoded_there(tmp_path):
    cfg, ck = _patch2d()
    pn, ps = utils.preset_grid(cfg)
    G = (pn[0] * ps[0], pn[1] * ps[1])
    Cc = cfg["output_dim"]
    long, short = max(G) + 37, min(G) + 21
    assert long > short
    src = np.random.RandomState(32).randint(0, 256, size=(1, Cc, long, short)).astype(np.uint8)      # portrait, channel-first
    img = torch.from_numpy(src)
    resized = utils.resize_to_preset(cfg, img.to(DEV), channels_first=True)
    land = src.transpose(0, 3, 2, 1)                        # [1, short, long, C]: the landscape orientation
    want = E.resize(land, G)
    assert tuple(resized.shape) == (1, *G, Cc) and np.array_equal(resized.cpu().numpy(), want)
    path = os.path.join(tmp_path, "a.rcb")
    (dist, model, coded), seen = _spied(lambda: drivers.compress_resized(cfg, "kodak", ck, img, channels_first=True,
                                                                          bitstream_path=path, **KW))
    assert torch.equal(coded, resized) and model.compressed_mask_groupwise.all()
    (_, y_seen), = seen
    assert np.array_equal(S.bits(y_seen.cpu().numpy()), S.bits(S.targets(want, pn, ps)))
    blob = open(path, "rb").read()
    assert bitstream.unpack(blob)[1] is None                # a signal at the preset's grid: no extent in the stream
    n_rows = int(np.prod(pn))
    dec = bitstream.decode_signal(cfg, "kodak", ck, blob, None, n_rows, device=DEV, precision=1, as_uint8=True)
    assert dec.dtype == torch.uint8 and tuple(dec.shape) == (1, *G, Cc)
    # the driver's distortion is that of the decoded integers against the resized source
    terms = R.terms(S.unit8(dec.cpu().numpy()), S.unit8(want))
    figure = utils.metric_from_sse([math.fsum(terms.reshape(-1))], terms.size, "kodak")
    print("compress_resized %r, the decoded integers against the resized source %r" % (dist, figure))
    # (encoder and decoder agree to 1e-5 in y, tests/test_hip_drivers.py; one 8-bit rounding flip moves the PSNR of a 32 x 32 x 3
    # image by 1.4e-3 dB and that of this larger one by less: the bound of that test)
    assert np.isfinite(dist) and abs(float(dist) - figure) <= 5e-3
