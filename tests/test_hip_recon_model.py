"""The callers of rcb_recon_finish on small models from the goldens (the helper of tests/test_hip_test_model.py): TestBNNmodel.report
against _report, and the decoder's 8-bit / whole-signal outputs against the evaluator tests/recon_emul.py."""
import numpy as np
import pytest
import torch

import recon_emul as E
from golden_util import level_kwargs, load, regen_noise
from test_hip_test_model import DEV, build, feed, set_post, xdev, ydev
from test_recon_emul_cpu import psnr_bound_db

pytestmark = pytest.mark.gpu

from recombiner_amd import bitstream  # noqa: E402


@pytest.mark.parametrize("name", ["cifar", "patch2d"])
def test_report_agrees_with_the_host_report(name):
    """report(x, y) -- rounding and squared error on the device, fp64 sums -- against _report(x, y) -- numpy on a host copy, float32
    mean -- on ONE reconstruction (predict draws noise: both score the same sample), within the bound derived in
    tests/test_recon_emul_cpu.py; same shape and type"""
    d = load(f"test_{name}.npz")
    cfg, n, m = build(d, name)
    set_post(d, cfg, m)
    X, Y = xdev(d, n), ydev(d)
    feed(m, regen_noise(d, "pred_S1_eps"))
    with torch.no_grad():
        y_pred = m.predict(X)
    m.predict = lambda x, **kw: y_pred
    want, got = m._report(X, Y), m.report(X, Y)
    assert np.shape(got) == np.shape(want) and isinstance(got, float) == isinstance(want, float)
    assert (np.shape(got) == (n,)) if name == "cifar" else isinstance(got, float)
    n_mean = Y[0].numel() if name == "cifar" else Y.numel()
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max()
    print(f"{name}: report {got}, _report {want}, |diff| {err:.3g} dB, bound {psnr_bound_db(n_mean):.3g} dB")
    assert err <= psnr_bound_db(n_mean) and np.all(np.asarray(got) < 60.0)
    assert np.array_equal(np.asarray(m.report(X, Y, on_device=False)), np.asarray(want))
    assert (m.recon_layout() is None) == (name == "cifar")


def _checkpoint(d, cfg, m):
    """the eight objects of a prior checkpoint (drivers.build_test_model's input) that carry the golden's grouping and priors"""
    out = []
    for pre in ["", "h_", "hh_"]:
        if pre and not cfg["patch"]:
            out += [(None,) * 8, (None, None, 1e-5, None)]
            continue
        kw = level_kwargs(d, pre)
        g2p, p2g = kw["group_to_param"], kw["param_to_group"]
        assert np.array_equal(np.argsort(p2g), g2p)
        scale = torch.nn.functional.softplus(kw["p_log_scale"]) / 6            # the checkpoint stores sigma, in parameter order
        als = kw["init_log_scale"] if kw["init_log_scale"] is not None else torch.full_like(kw["p_loc"], -4.0)
        out += [(kw["group_idx"], kw["group_start_index"], kw["group_end_index"], g2p, p2g, kw["n_groups"], None, None),
                (kw["p_loc"][g2p], scale[g2p], 1e-5, als[g2p])]
    return out + [m.linear_transform, m.upsample_net]


def test_decoder_returns_8_bit_whole_signals():
    """2-D patched golden: encode every group, then the standalone decoder with as_uint8: uint8 [n_data, H, W, C], equal to
    np.round(clip(decode(...)) * 255) stitched by the evaluator; decode_signal gives the same on the fp32 lattice; audio has no
    8-bit form"""
    d = load("test_patch2d.npz")
    cfg, n, m = build(d, "patch2d")
    m.precision = 1
    set_post(d, cfg, m)
    X = xdev(d, n)
    for lv in (m._l3, m._l2, m._l1):
        for r in range(lv.n_groups):
            m._encode_round(lv, True, r)
    blob = bitstream.encode(m)
    ck = _checkpoint(d, cfg, m)
    y = bitstream.decode(cfg, "kodak", ck, blob, X, n, device=DEV, precision=1)
    u8 = bitstream.decode(cfg, "kodak", ck, blob, X, n, device=DEV, precision=1, as_uint8=True)
    pn, ps = cfg["patch_nums"], cfg["pixel_sizes"]
    n_data = n // int(np.prod(pn))
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (n_data, pn[0] * ps[0], pn[1] * ps[1], cfg["output_dim"])
    yh = y.cpu().numpy()
    want = E.stitch(np.round(np.clip(yh, 0, 1) * 255), pn, ps)
    assert want.dtype == np.float32 and np.array_equal(u8.cpu().numpy(), want.astype(np.uint8))
    whole = bitstream.decode_signal(cfg, "kodak", ck, blob, X, n, device=DEV, precision=1)
    assert whole.dtype == torch.float32 and np.array_equal(whole.cpu().numpy(), E.stitch(E.round8(yh)[1], pn, ps))
    with pytest.raises(ValueError):
        bitstream.decode(cfg, "audio", ck, blob, X, n, device=DEV, as_uint8=True)
    with pytest.raises(ValueError):
        bitstream.decode_signal(cfg, "protein", ck, blob, X, n, device=DEV, as_uint8=True)
