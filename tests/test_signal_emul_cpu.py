"""The premises of the rcb_signal_patch tests (tests/test_hip_signal.py), checked on the CPU: the evaluator tests/signal_emul.py cuts
patches in the order recon_emul.stitch puts them back and in the reference loaders' formulation, its q / 255 is torch's on the CPU
and survives the 8-bit rounding of rcb_recon_finish, and the host helpers utils.signal_view / utils.preset_inputs are what the GPU
tests take them for."""
import numpy as np
import pytest
import torch

import recon_emul as E
import signal_emul as S
from recombiner_amd import config, utils

F32 = np.float32
GEOMS = [((5,), (7,), 1), ((2, 3), (4, 5), 3), ((1, 2, 2), (3, 2, 4), 3), ((2, 3, 2), (2, 3, 5), 2)]


# ---- the cut ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn,ps,C", GEOMS)
def test_patch_inverts_the_stitch(pn, ps, C):
    """patch(stitch(a)) == a and stitch(patch(w)) == w on random arrays (1-D, 2-D, 3-D; every value distinct, so a misplaced element
    shows): the order rcb_signal_patch writes is the order rcb_recon_finish reads"""
    n_data = 3
    N, P = n_data * int(np.prod(pn)), int(np.prod(ps))
    a = np.random.RandomState(1).permutation(N * P * C).reshape(N, P, C).astype(F32)
    w = E.stitch(a, pn, ps)
    assert w.shape == (n_data, *[x * y for x, y in zip(pn, ps)], C)
    assert np.array_equal(S.patch(w, pn, ps), a)
    assert np.array_equal(E.stitch(S.patch(w, pn, ps), pn, ps), w)
    assert np.array_equal(S.patch(w, pn, ps), E.cut(w, pn, ps))
    assert S.patch(w[:0], pn, ps).shape == (0, P, C)


@pytest.mark.parametrize("pn,ps,C", GEOMS)
def test_patch_is_the_reference_loaders_formulation(pn, ps, C):
    """data/image.py:30-46, data/video.py:54-73, data/audio.py:125-140: nested loops over the patch index, a slice of the [C, *spatial]
    tensor per patch, each pushed through to_grid_coordinates_and_features (the product's own), the features stacked"""
    nd, n_data = len(pn), 2
    G = [x * y for x, y in zip(pn, ps)]
    whole = torch.from_numpy(np.random.RandomState(2).rand(n_data, *G, C).astype(F32))
    rows = []
    for d in range(n_data):
        tensor = whole[d].movedim(-1, 0)                                  # [C, *spatial], as ToTensor gives it
        if nd == 1:
            for i in range(G[0] // ps[0]):
                rows.append(utils.to_grid_coordinates_and_features(tensor[..., i * ps[0]: i * ps[0] + ps[0]])[1])
        elif nd == 2:
            for i in range(G[0] // ps[0]):
                for j in range(G[1] // ps[1]):
                    p_ = tensor[:, i * ps[0]: i * ps[0] + ps[0], j * ps[1]: j * ps[1] + ps[1]]
                    rows.append(utils.to_grid_coordinates_and_features(p_)[1])
        else:
            for t_ in range(G[0] // ps[0]):
                for i in range(G[1] // ps[1]):
                    for j in range(G[2] // ps[2]):
                        p_ = tensor[..., t_ * ps[0]: t_ * ps[0] + ps[0], i * ps[1]: i * ps[1] + ps[1], j * ps[2]: j * ps[2] + ps[2]]
                        rows.append(utils.to_grid_coordinates_and_features(p_)[1])
    want = torch.stack(rows).numpy()
    assert np.array_equal(S.patch(whole.numpy(), pn, ps), want)


# ---- q / 255 -------------------------------------------------------------------------------------------------------------------
def test_unit8_is_torchs_division_on_every_byte():
    """all 256 byte values: the evaluator's fp32 division is bit-equal to torch's on the CPU, as ToTensor (float().div(255)) and as
    data/video.py:31 (uint8 tensor / 255) write it; and it is not the reciprocal multiply"""
    q = np.arange(256, dtype=np.uint8)
    t = torch.from_numpy(q)
    got = S.bits(S.unit8(q))
    assert np.array_equal(got, S.bits(t.float().div(255).numpy()))
    assert (t / 255).dtype == torch.float32 and np.array_equal(got, S.bits((t / 255).numpy()))
    assert S.unit8(np.uint8(255)) == F32(1) and S.unit8(np.uint8(0)) == F32(0) and S.unit8(np.uint8(51)).dtype == F32
    recip = q.astype(F32) * (F32(1) / F32(255))
    assert (S.bits(recip) != got).any()                                   # (the shortcut the kernel must not take differs somewhere)


def test_round8_gives_every_byte_back():
    """all 256 byte values: rcb_recon_finish's 8-bit rounding of q / 255 is q again, and its fp32 value the same bits -- what the
    GPU round trip (signal_patch, then recon_finish against the same y) rests on: u8 == source, sse == 0"""
    q = np.arange(256, dtype=np.uint8)
    v = S.unit8(q)
    q2, v2 = E.round8(v)
    assert np.array_equal(q2, q.astype(F32)) and np.array_equal(S.bits(v2), S.bits(v))
    assert np.array_equal(E.terms(v2, v), np.zeros(256))


# ---- utils.signal_view ---------------------------------------------------------------------------------------------------------
def _cfg(name, **kw):
    return dict(config.configs[name], **kw)


def _is_view_of(v, base):
    lo, hi = base.data_ptr(), base.data_ptr() + base.numel() * base.element_size()
    return lo <= v.data_ptr() < hi and v.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()


def test_signal_view_channels_first_window_and_swap():
    cfg = _cfg("kodak", pixel_sizes=[4, 6], patch_nums=[2, 3])            # a window of 8 x 18 pixels
    rng = np.random.RandomState(3)
    # channels-first, larger than the preset, default origin: the leading whole patches
    a = torch.from_numpy(rng.rand(2, 3, 11, 23).astype(F32))
    v = utils.signal_view(cfg, a, channels_first=True)
    assert tuple(v.shape) == (2, 8, 18, 3) and _is_view_of(v, a) and v.data_ptr() == a.data_ptr()
    assert v.stride() == (3 * 11 * 23, 23, 1, 11 * 23)
    assert np.array_equal(v.numpy(), a.numpy().transpose(0, 2, 3, 1)[:, :8, :18])
    # a window at an odd origin of a channel-last signal
    b = torch.from_numpy(rng.randint(0, 256, size=(2, 11, 23, 3)).astype(np.uint8))
    v = utils.signal_view(cfg, b, origin=(3, 5))
    assert tuple(v.shape) == (2, 8, 18, 3) and _is_view_of(v, b) and v.data_ptr() == b.data_ptr() + (3 * 23 + 5) * 3
    assert np.array_equal(v.numpy(), b.numpy()[:, 3:11, 5:23])
    # portrait input: the spatial axes are swapped (data/image.py:18-19), unless asked not to
    c = torch.from_numpy(rng.rand(1, 20, 9, 3).astype(F32))
    v = utils.signal_view(cfg, c)
    assert _is_view_of(v, c) and np.array_equal(v.numpy(), c.numpy().transpose(0, 2, 1, 3)[:, :8, :18])
    with pytest.raises(ValueError):
        utils.signal_view(cfg, c, landscape=False)                        # 9 < 18 pixels on the second axis
    d = torch.from_numpy(rng.rand(1, 20, 19, 3).astype(F32))
    assert np.array_equal(utils.signal_view(cfg, d, landscape=False).numpy(), d.numpy()[:, :8, :18])
    assert np.array_equal(utils.signal_view(cfg, d).numpy(), d.numpy().transpose(0, 2, 1, 3)[:, :8, :18])


def test_signal_view_other_presets_and_refusals():
    cfg1 = _cfg("audio", pixel_sizes=[5], patch_nums=[3])
    a = torch.arange(2 * 1 * 17, dtype=torch.float32).reshape(2, 1, 17)
    v = utils.signal_view(cfg1, a, channels_first=True, origin=[2])
    assert tuple(v.shape) == (2, 15, 1) and np.array_equal(v.numpy()[..., 0], a.numpy()[:, 0, 2:17])
    cfg3 = _cfg("video", pixel_sizes=[3, 4, 4], patch_nums=[1, 2, 2])
    b = torch.rand(2, 4, 3, 9, 8)                                         # [n, T, C, H, W] is not channels-first: move it by hand
    v = utils.signal_view(cfg3, b.movedim(2, -1), origin=(1, 0, 0))
    assert tuple(v.shape) == (2, 3, 8, 8, 3) and np.array_equal(v.numpy(), b.numpy().transpose(0, 1, 3, 4, 2)[:, 1:4, :8, :8])
    cfgc = config.configs["cifar"]                                        # unpatched: the window is pixel_sizes
    c = torch.rand(3, 3, 32, 32)
    assert tuple(utils.signal_view(cfgc, c, channels_first=True).shape) == (3, 32, 32, 3)
    for bad, kw in ((torch.rand(1, 31, 32, 3), {}), (torch.rand(1, 32, 32, 3), dict(origin=(1, 0))), (torch.rand(1, 32, 32, 4), {}),
                    (torch.rand(1, 32, 32, 3), dict(origin=(-1, 0))), (torch.rand(32, 3), {}), (torch.rand(1, 32, 32, 3), dict(origin=(0,)))):
        with pytest.raises(ValueError):
            utils.signal_view(cfgc, bad, **kw)
    pn, ps = utils.preset_grid(config.configs["kodak"])
    assert (pn, ps) == ([8, 12], [64, 64]) and utils.preset_grid(cfgc) == ([1, 1], [32, 32])
    assert utils.preset_grid(config.configs["video"]) == ([1, 8, 8], [24, 16, 16])


@pytest.mark.parametrize("name", sorted(config.configs))
def test_preset_inputs_are_the_synthetic_inputs(name):
    cfg = config.configs[name]
    X = utils.preset_inputs(cfg)
    want = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], 1, cfg["output_dim"], seed=0)[0]
    assert X.dtype == torch.float32 and tuple(X.shape) == (int(np.prod(cfg["pixel_sizes"])), cfg["input_dim"] - 16)
    assert torch.equal(X, want) and utils.preset_inputs(cfg, "cpu").device.type == "cpu"
