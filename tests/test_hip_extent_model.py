"""Signals of any size end to end (drivers.compress_signals_any -> version-2 bitstream -> bitstream.decode_signal_any) on small
models, with the smallest settings of tests/test_hip_signal_model.py (16-bit mode, 4 optimisation epochs, 1 fine-tune epoch): the
targets that reach the optimiser are the evaluator's edge-padded targets bit for bit, the stream carries the size, the decoder returns
the signals at their own size, and the distortion counts the real samples only."""
import os

import numpy as np
import pytest
import torch

import extent_emul as X
import signal_emul as S
from golden_util import GOLDEN, cfg_of, load
from test_extent_emul_cpu import _v1_bytes
from test_hip_recon_model import _checkpoint
from test_hip_test_model import DEV, build
from test_recon_emul_cpu import psnr_bound_db

pytestmark = pytest.mark.gpu

from recombiner_amd import bitstream, drivers, utils  # noqa: E402

KW = dict(device=DEV, n_epochs=4, finetune_epochs=1, precision=1)


def _cifar():
    return cfg_of(load("psnr_smooth_cifar.npz")), drivers.load_checkpoint(os.path.join(GOLDEN, "PRIOR_ref_smooth_cifar.pkl.gz"))


def _patch2d():
    d = load("test_patch2d.npz")
    cfg, _, m = build(d, "patch2d")
    return cfg, _checkpoint(d, cfg, m)


def _spied(call):
    """run `call` with TestBNNmodel.optimize_posteriors recording the (x, y) it is given -> (result, [(x, y), ...])"""
    seen = []
    orig = drivers.TestBNNmodel.optimize_posteriors

    def spy(self, x, y, **kw):
        seen.append((x.clone(), y.clone()))
        return orig(self, x, y, **kw)
    drivers.TestBNNmodel.optimize_posteriors = spy
    try:
        return call(), seen
    finally:
        drivers.TestBNNmodel.optimize_posteriors = orig


@pytest.mark.parametrize("name,dataset,n,size,want_pn", [("cifar", "cifar", 2, (28, 30), None), ("patch2d", "kodak", 1, (40, 70), [2, 4])])
def test_signals_smaller_than_the_grid(name, dataset, n, size, want_pn, tmp_path):
    """(a) two 28 x 30 images on the unpatched CIFAR preset; (b) one 40 x 70 image on the 2-D patched golden geometry (patches of
    32 x 32, level 2 groups 1 x 2): it fits to 2 x 4 patches, the last column of patches wholly padded"""
    cfg, ck = _cifar() if name == "cifar" else _patch2d()
    before = repr(cfg)
    Cc = cfg["output_dim"]
    u8 = np.random.RandomState(7).randint(0, 256, size=(n, *size, Cc)).astype(np.uint8)
    path = os.path.join(tmp_path, "a.rcb")
    (dist, model, fitted), seen = _spied(lambda: drivers.compress_signals_any(cfg, dataset, ck, torch.from_numpy(u8), bitstream_path=path,
                                                                              **KW))
    assert repr(cfg) == before and model.compressed_mask_groupwise.all()
    pn, ps = utils.preset_grid(fitted)
    assert ps == list(cfg["pixel_sizes"]) and (fitted == cfg if want_pn is None else fitted["patch_nums"] == want_pn)
    G = tuple(a * b for a, b in zip(pn, ps))
    # the targets that reach optimize_posteriors: the evaluator's edge-padded targets, bit for bit
    (x_seen, y_seen), = seen
    want_y = X.targets(u8, pn, ps)
    assert y_seen.is_cuda and tuple(y_seen.shape) == want_y.shape == (n * int(np.prod(pn)), int(np.prod(ps)), Cc)
    assert np.array_equal(S.bits(y_seen.cpu().numpy()), S.bits(want_y))
    assert torch.equal(x_seen[0], utils.preset_inputs(cfg, DEV)) and x_seen.shape[0] == y_seen.shape[0]
    # the stream: version 2, carrying the size
    blob = open(path, "rb").read()
    levels, extent = bitstream.unpack(blob)
    assert extent == tuple(size) and levels[0].shape[0] == y_seen.shape[0]
    assert blob == bitstream.encode(model, extent=size) and bitstream.encode(model) == _v1_bytes([a.astype(np.int64) for a in levels])
    with pytest.raises(ValueError, match="decode_signal_any"):
        bitstream.decode_signal(fitted, dataset, ck, blob, None, y_seen.shape[0], device=DEV, precision=1)
    # the decoder: the signals at their own size = the crop of the patch-level decoder's grid
    torch.manual_seed(77)
    got = bitstream.decode_signal_any(cfg, dataset, ck, blob, device=DEV, precision=1, as_uint8=True)
    torch.manual_seed(77)
    grid = bitstream.decode(fitted, dataset, ck, blob, None, y_seen.shape[0], device=DEV, precision=1, as_uint8=True)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == u8.shape
    crop = (slice(None),) + tuple(slice(0, s) for s in size)
    assert torch.equal(got, grid.reshape(n, *G, Cc)[crop])
    if name == "cifar":                                    # (one more decode: once is enough) the fp32 form is the same lattice
        torch.manual_seed(77)
        f32 = bitstream.decode_signal_any(cfg, dataset, ck, blob, device=DEV, precision=1)
        assert np.array_equal(S.bits(f32.cpu().numpy()), S.bits(S.unit8(got.cpu().numpy())))
    # the distortion: numpy's figure of that cropped decode against the source, over the real samples only
    want = utils.metric(S.unit8(u8), S.unit8(got.cpu().numpy()), dataset)
    assert np.shape(dist) == np.shape(want) == ((n,) if dataset == "cifar" else ())
    n_mean = int(np.prod(size)) * Cc * (1 if dataset == "cifar" else n)
    err = np.abs(np.asarray(dist, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max()
    print(f"{name} {size}: distortion {dist}, numpy on the cropped decode {want}, |diff| {err:.3g} dB, bound {psnr_bound_db(n_mean):.3g} dB")
    assert err <= psnr_bound_db(n_mean) and np.all(np.asarray(dist) < 60.0)
    # ... and it is not the figure over the padded grid
    if G != tuple(size):
        padded = utils.metric(S.unit8(X.pad_edge(u8, pn, ps)), S.unit8(grid.reshape(n, *G, Cc).cpu().numpy()), dataset)
        assert np.all(np.asarray(padded) != np.asarray(dist))


def test_signals_of_the_presets_own_size_are_coded_as_before(tmp_path):
    """(c) 32 x 32 images through compress_signals_any and through compress_signals: the same index arrays, the same distortion, and
    encode(model) without an extent is the version-1 stream, byte for byte"""
    cfg, ck = _cifar()
    n = 2
    u8 = torch.from_numpy(np.random.RandomState(7).randint(0, 256, size=(n, 3, 32, 32)).astype(np.uint8))
    pa, pb = os.path.join(tmp_path, "a.rcb"), os.path.join(tmp_path, "b.rcb")
    dist_a, model_a = drivers.compress_signals(cfg, "cifar", ck, u8, channels_first=True, bitstream_path=pa, **KW)
    dist_b, model_b, fitted = drivers.compress_signals_any(cfg, "cifar", ck, u8, channels_first=True, bitstream_path=pb, **KW)
    assert fitted == cfg and fitted is not cfg
    blob_a, blob_b = open(pa, "rb").read(), open(pb, "rb").read()
    la, lb = bitstream.unpack_indices(blob_a), bitstream.unpack_indices(blob_b)
    assert len(la) == len(lb) == 1 and np.array_equal(la[0], lb[0])
    assert bitstream.unpack(blob_a)[1] is None and bitstream.unpack(blob_b)[1] == (32, 32)
    assert blob_a == _v1_bytes(la) == bitstream.encode(model_a) == bitstream.encode(model_b)
    assert bitstream.payload_bits(blob_a) == bitstream.payload_bits(blob_b)
    err = np.abs(np.asarray(dist_a, dtype=np.float64) - np.asarray(dist_b, dtype=np.float64)).max()
    assert np.shape(dist_a) == np.shape(dist_b) == (n,) and err <= psnr_bound_db(32 * 32 * 3)     # (numpy float32 / device fp64)
