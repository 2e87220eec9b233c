"""Lists of signals of mixed sizes and orientations end to end (drivers.compress_signal_list -> version-4 bitstreams ->
bitstream.decode_signal_list) on the small models and with the settings of tests/test_hip_extent_model.py (16-bit mode, 4 optimisation
epochs, 1 fine-tune epoch): per bucket the targets that reach the optimiser are the evaluator's (tests/ragged_emul.py) bit for bit, the
stream carries every size and swap flag, the decoder returns each signal at its own shape and orientation, and the distortion counts
the real samples only."""
import os

import numpy as np
import pytest
import torch

import ragged_emul as R
import sample16_emul as Q
import signal_emul as S
from test_hip_extent_model import KW, _cifar, _patch2d, _spied
from test_hip_sample16_model import _patch1d
from test_hip_test_model import DEV
from test_recon_emul_cpu import psnr_bound_db

pytestmark = pytest.mark.gpu

from recombiner_amd import bitstream, drivers, utils  # noqa: E402
from recombiner_amd.utils import SampleFormat  # noqa: E402


@pytest.mark.parametrize("name,dataset,sizes,want", [
    ("cifar", "cifar", [(28, 30), (32, 32), (31, 17)], [([1, 1], [0, 1, 2])]),
    ("patch2d", "kodak", [(40, 70), (70, 40), (64, 100), (30, 60)], [([2, 4], [0, 1, 2]), ([1, 2], [3])])])
def test_a_list_of_mixed_sizes_and_orientations(name, dataset, sizes, want, tmp_path):
    """(a) three images on the unpatched CIFAR preset, the third portrait; (b) four on the 2-D patched golden geometry (patches of
    32 x 32, level 2 groups 1 x 2): three share the 2 x 4 grid, one of them portrait, the fourth takes the 1 x 2 grid"""
    cfg, ck = _cifar() if name == "cifar" else _patch2d()
    before = repr(cfg)
    Cc = cfg["output_dim"]
    rng = np.random.RandomState(7)
    u8 = [rng.randint(0, 256, size=(*s, Cc)).astype(np.uint8) for s in sizes]
    (dist, records, bpp), seen = _spied(lambda: drivers.compress_signal_list(cfg, dataset, ck, [torch.from_numpy(a) for a in u8],
                                                                             bitstream_dir=str(tmp_path), **KW))
    assert repr(cfg) == before and len(records) == len(seen) == len(want)
    swaps = [s[0] > s[1] for s in sizes]
    decoded = [None] * len(sizes)
    bits = 0
    for b, (rec, (x_seen, y_seen), (want_pn, want_idx)) in enumerate(zip(records, seen, want)):
        fitted, model, idx = rec["config"], rec["model"], rec["indices"]
        pn, ps = utils.preset_grid(fitted)
        assert pn == want_pn and idx == want_idx and model.compressed_mask_groupwise.all()
        G = tuple(a * c for a, c in zip(pn, ps))
        views = [u8[k].transpose(1, 0, 2) if swaps[k] else u8[k] for k in idx]           # along the model's axes
        msizes = [v.shape[:-1] for v in views]
        assert [tuple(s) for s in rec["sizes"]] == [tuple(s) for s in msizes] and rec["swaps"] == [swaps[k] for k in idx]
        # the targets that reach optimize_posteriors: the evaluator's, bit for bit
        want_y = R.targets(views, pn, ps, Q.U8)
        assert y_seen.is_cuda and tuple(y_seen.shape) == want_y.shape == (len(idx) * int(np.prod(pn)), int(np.prod(ps)), Cc)
        assert np.array_equal(S.bits(y_seen.cpu().numpy()), S.bits(want_y))
        assert torch.equal(x_seen[0], utils.preset_inputs(cfg, DEV)) and x_seen.shape[0] == y_seen.shape[0]
        # the stream: version 4 with the sizes and the swaps
        blob = rec["stream"]
        assert blob == open(os.path.join(tmp_path, "bucket_%d.rcb" % b), "rb").read()
        assert bitstream.unpack_header(blob) == dict(version=4, extent=None, sample_format=SampleFormat.u8(),
                                                     extents=[tuple(int(v) for v in s) for s in msizes], swaps=rec["swaps"])
        assert bitstream.unpack(blob)[0][0].shape[0] == y_seen.shape[0]
        bits += bitstream.payload_bits(blob)
        with pytest.raises(ValueError, match="decode_signal_list"):
            bitstream.decode_signal_any(cfg, dataset, ck, blob, device=DEV, precision=1)
        # the decoder: each signal at its own shape and orientation = the crop (and transpose) of the patch-level decoder's grid
        torch.manual_seed(77)
        got = bitstream.decode_signal_list(cfg, dataset, ck, blob, device=DEV, precision=1, as_integer=True)
        torch.manual_seed(77)
        grid = bitstream.decode(fitted, dataset, ck, blob, None, y_seen.shape[0], device=DEV, precision=1, as_uint8=True)
        grid = grid.reshape(len(idx), *G, Cc)
        for j, k in enumerate(idx):
            crop = grid[j][tuple(slice(0, s) for s in msizes[j])]
            if swaps[k]:
                crop = crop.transpose(0, 1)
            assert got[j].dtype == torch.uint8 and got[j].is_contiguous() and tuple(got[j].shape) == u8[k].shape
            assert torch.equal(got[j], crop)
            decoded[k] = got[j].cpu().numpy()
    assert abs(bpp - bits / sum(int(np.prod(s)) for s in sizes)) <= 1e-12
    # the distortion: numpy's figure over the real samples
    if dataset == "cifar":
        want_d = np.array([utils.metric(S.unit8(a)[None], S.unit8(d)[None], dataset)[0] for a, d in zip(u8, decoded)])
        bounds = np.array([psnr_bound_db(a.size) for a in u8])
        assert np.shape(dist) == (len(sizes),)
    else:
        flat = lambda arrs: np.concatenate([S.unit8(a).reshape(-1) for a in arrs])       # noqa: E731
        want_d, bounds = utils.metric(flat(u8), flat(decoded), dataset), psnr_bound_db(sum(a.size for a in u8))
        assert isinstance(dist, float)
    err = np.abs(np.asarray(dist, dtype=np.float64) - np.asarray(want_d, dtype=np.float64))
    print(f"{name}: distortion {dist}, numpy over the real samples {want_d}, |diff| {err} dB, bound {bounds} dB")
    assert np.all(err <= bounds) and np.all(np.asarray(dist) < 60.0)


def test_equal_sizes_are_coded_as_the_single_size_driver_codes_them():
    """(c) two 28 x 30 images through the list driver and through compress_signals_any: the same index arrays and payload bits"""
    cfg, ck = _cifar()
    u8 = torch.from_numpy(np.random.RandomState(7).randint(0, 256, size=(2, 28, 30, 3)).astype(np.uint8))
    dist_l, records, bpp = drivers.compress_signal_list(cfg, "cifar", ck, list(u8), **KW)
    dist_a, model, _ = drivers.compress_signals_any(cfg, "cifar", ck, u8, **KW)
    assert len(records) == 1 and records[0]["indices"] == [0, 1] and records[0]["swaps"] == [False, False]
    la, ll = bitstream.unpack_indices(bitstream.encode(model, extent=(28, 30))), bitstream.unpack_indices(records[0]["stream"])
    assert len(la) == len(ll) and all(np.array_equal(a, b) for a, b in zip(la, ll))
    assert bitstream.payload_bits(records[0]["stream"]) == bitstream.payload_bits(bitstream.encode(model, extent=(28, 30)))
    assert abs(bpp - bitstream.payload_bits(records[0]["stream"]) / (2 * 28 * 30)) <= 1e-12
    assert np.abs(np.asarray(dist_l) - np.asarray(dist_a)).max() <= 1e-9        # the same sums, divided once each


def test_s16_clips_of_two_lengths_share_one_stream():
    """(d) PCM clips of 410 and 500 samples on the 1-D patched golden geometry (patches of 160, level 2 groups 2): both fit 4 patches"""
    cfg, ck = _patch1d()
    rng = np.random.RandomState(7)
    pcm = [rng.randint(-32768, 32768, size=(n, 1)).astype(np.int16) for n in (410, 500)]
    f = SampleFormat.s16()
    with pytest.raises(ValueError, match="sample_format"):
        drivers.compress_signal_list(cfg, "audio", ck, [torch.from_numpy(a) for a in pcm], **KW)
    (dist, records, bpp), seen = _spied(lambda: drivers.compress_signal_list(cfg, "audio", ck, [torch.from_numpy(a) for a in pcm],
                                                                             sample_format=f, **KW))
    (rec,), ((_, y_seen),) = records, seen
    pn, ps = utils.preset_grid(rec["config"])
    assert pn == [4] and rec["indices"] == [0, 1] and isinstance(dist, float) and np.isfinite(dist)
    want_y = R.targets(pcm, pn, ps, Q.S16)
    assert np.array_equal(S.bits(y_seen.cpu().numpy()), S.bits(want_y))
    hdr = bitstream.unpack_header(rec["stream"])
    assert hdr["version"] == 4 and hdr["sample_format"] == f and hdr["extents"] == [(410,), (500,)] and hdr["swaps"] == [False, False]
    torch.manual_seed(77)
    got = bitstream.decode_signal_list(cfg, "audio", ck, rec["stream"], device=DEV, precision=1, as_integer=True)
    torch.manual_seed(77)
    y_dec = bitstream.decode(rec["config"], "audio", ck, rec["stream"], None, y_seen.shape[0], device=DEV, precision=1)
    want = R.finish(y_dec.cpu().numpy(), want_y, pn, ps, Q.S16, [(410,), (500,)])
    for g, w, a in zip(got, want["q"], pcm):
        assert g.dtype == torch.int16 and tuple(g.shape) == a.shape and np.array_equal(g.cpu().numpy(), w)
    want_d = utils.metric_from_sse(want["sse"], np.array([410, 500]), "audio")
    assert abs(dist - want_d) <= 4.3430 * 640 * 2.0 ** -53 * 1.01 + 1e-12      # (the order of 640 additions per clip: test_hip_sample16_model)
    assert abs(bpp - bitstream.payload_bits(rec["stream"]) / 910) <= 1e-12
