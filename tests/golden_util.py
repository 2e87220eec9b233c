"""Helpers shared by the parity tests: fixture loading, compact-array checks, input rebuilds."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_cpu as O  # noqa: E402  (oracle = checker only)


def load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def cfg_of(d):
    return json.loads(str(d["cfg"]))


def has(d, key):
    return key in d.files or (key + "__sub") in d.files


def check(d, key, actual, rtol=1e-5, atol=1e-6, what=""):
    """Compare ``actual`` with fixture entry ``key`` stored whole or as subsample+moments."""
    a = actual.detach().cpu().numpy() if torch.is_tensor(actual) else np.asarray(actual)
    if key in d.files:
        exp = d[key]
        assert a.shape == exp.shape, (key, a.shape, exp.shape)
        np.testing.assert_allclose(a, exp, rtol=rtol, atol=atol, err_msg=f"{what}{key}")
        return
    sub, stride = d[key + "__sub"], int(d[key + "__stride"])
    assert tuple(a.shape) == tuple(d[key + "__shape"]), (key, a.shape)
    flat = a.reshape(-1)
    np.testing.assert_allclose(flat[::stride], sub, rtol=rtol, atol=atol, err_msg=f"{what}{key} (subsample)")
    f64 = flat.astype(np.float64)
    got = np.array([f64.sum(), np.abs(f64).sum(), (f64 * f64).sum()])
    exp = d[key + "__stats"]
    n = flat.size
    tol = np.array([atol * n + rtol * exp[1], atol * n + rtol * exp[1], 2 * (atol * exp[1] + rtol * exp[2]) + 1e-30])
    assert np.all(np.abs(got - exp) <= tol), (key, got, exp, tol)


def regen_noise(d, prefix, seed=None):
    """Noise tensors = torch.manual_seed(seed) then randn(shape) in the recorded order; the
    recorded moments pin the regeneration."""
    shapes = json.loads(str(d[prefix + "_shapes"]))
    seed = int(d[prefix + "_seed"]) if seed is None else seed
    torch.manual_seed(seed)
    out = [torch.randn(tuple(s)) for s in shapes]
    st = d[prefix + "_stats"]
    for e, s in zip(out, st):
        a = e.double()
        got = np.array([a.sum().item(), a.abs().sum().item(), (a * a).sum().item()])
        np.testing.assert_allclose(got, s, rtol=1e-9, atol=1e-9)
    return out


def regen_noise_per_epoch(d, prefix, n_epochs):
    """Test-time training reseeds with the epoch index before every step."""
    shapes = json.loads(str(d[prefix + "_shapes"]))
    per = len(shapes) // n_epochs
    out, k = [], 0
    for ep in range(n_epochs):
        torch.manual_seed(ep)
        out.append([torch.randn(tuple(s)) for s in shapes[k:k + per]])
        k += per
    st = d[prefix + "_stats"]
    flat = [e for ep in out for e in ep]
    for e, s in zip(flat, st):
        a = e.double()
        np.testing.assert_allclose(np.array([a.sum().item(), a.abs().sum().item(), (a * a).sum().item()]), s,
                                   rtol=1e-9, atol=1e-9)
    return out


def t(d, key):
    return torch.from_numpy(np.array(d[key])) if key in d.files else None


def prior_inputs(d):
    """Rebuild the inputs of a prior_<name>.npz case with the oracle's own constructors."""
    cfg = cfg_of(d)
    geo = O.Geometry.from_config(cfg)
    n = int(d["n"])
    p = O.init_prior_params(geo, n, seed=42)
    for k in ["log_scale", "lpe_log_scale", "h_log_scale", "hh_log_scale"]:
        if ("p_" + k) in d.files:
            p[k] = t(d, "p_" + k).clone()
    A = O.make_linear_transform(geo.dims, seed=123)
    up = O.UpsampleNet(geo.data_dim, geo.paddings, geo.layerwise_scale_factors, seed=124)
    X = t(d, "X")
    if X is None:  # stored as subsample + moments: rebuild and verify
        X = O.fourier_features(cfg["pixel_sizes"], cfg["fourier_dim"])
        check(d, "X", X, rtol=0, atol=1e-6)
    Y = t(d, "Y")
    if Y is None:
        torch.manual_seed(5)
        Y = torch.rand(n, X.shape[0], cfg["output_dim"])
        check(d, "Y", Y, rtol=0, atol=0)
    pri = [t(d, "prior_" + k) for k in ["pl", "ps", "ll", "ls", "hl", "hs", "hhl", "hhs"]]
    return cfg, geo, n, p, A, up, X, Y, pri


def stats_of(tensors):
    out = []
    for a in tensors:
        a = a.detach().double()
        out.append([a.sum().item(), a.abs().sum().item(), (a * a).sum().item()])
    return np.array(out)


def level_kwargs(d, pre=""):
    return dict(p_loc=t(d, f"kw_{pre}p_loc"), p_log_scale=t(d, f"kw_{pre}p_log_scale"),
                init_log_scale=t(d, f"kw_{pre}init_log_scale"),
                group_idx=d[f"{pre}G_group_idx"].astype(np.int64),
                group_start_index=d[f"{pre}G_start"].astype(np.int64),
                group_end_index=d[f"{pre}G_end"].astype(np.int64),
                group_to_param=d[f"{pre}G_group2param"].astype(np.int64),
                param_to_group=d[f"{pre}G_param2group"].astype(np.int64),
                n_groups=int(d[f"{pre}G_n_groups"]))


DATASET_OF = {"cifar": "cifar", "protein": "protein", "patch2d": "kodak", "patch1d": "audio", "patch3d": "video"}


def assert_close_mostly(actual, expected, rtol, atol, max_frac=1e-3, hard_atol=7e-4, what=""):
    """Adam normalises each gradient by its own running magnitude, so an element whose gradient is
    ~0 can move by up to lr per step in either direction: allow a tiny fraction of such elements
    (bounded by lr * steps = hard_atol), everything else must meet rtol/atol."""
    a = actual.detach().cpu().numpy() if torch.is_tensor(actual) else np.asarray(actual)
    e = np.asarray(expected)
    diff = np.abs(a - e)
    bad = diff > (atol + rtol * np.abs(e))
    assert bad.mean() <= max_frac, (what, float(bad.mean()))
    assert diff.max() <= hard_atol, (what, float(diff.max()))


def xy_of(d, y_seed=5):
    """(X [P, F], Y [n, P, C]) of a test_*.npz / e2e case: stored whole, or -- large geometries -- rebuilt (Fourier features of
    the coordinate grid; targets = torch.manual_seed(5), rand) and verified against the stored subsample + moments."""
    cfg = cfg_of(d)
    n = int(d["n"])
    X = t(d, "X")
    if X is None:
        X = O.fourier_features(cfg["pixel_sizes"], cfg["fourier_dim"])
        check(d, "X", X, rtol=0, atol=1e-6)
    Y = t(d, "Y")
    if Y is None:
        torch.manual_seed(y_seed)
        Y = torch.rand(n, X.shape[0], cfg["output_dim"])
        check(d, "Y", Y, rtol=0, atol=0)
    return X, Y


def structured_A(dims):
    """the stand-in for learned mappings of the checkpoint fixture (oracle/make_golden.py::structured_A): identity plus a
    small circulant pattern -- restated here so that the test can verify what the reference-written pickle carries"""
    mats = []
    for i in range(1, len(dims)):
        L = dims[i] * (dims[i - 1] + 1)
        r = torch.arange(L)
        base = torch.tensor([0.5, -0.25, 0.125, 0.375, -0.5, 0.25, -0.125, -0.375]) / 8
        mats.append(torch.eye(L) + base[(r[:, None] + 3 * r[None, :]) % 8] / L)
    return mats


def smooth_images(n, pixel_sizes, seed):
    """the synthetic images of the R-D fixtures (oracle/make_golden.py::smooth_images, restated: the fixtures store the
    seeds and moment checksums, not the pixels): per channel three 2-D sinusoids, scaled into [0.1, 0.9]"""
    rng = np.random.RandomState(seed)
    h, w = pixel_sizes
    yy, xx = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    out = np.zeros([n, h * w, 3], dtype=np.float32)
    for i in range(n):
        for c in range(3):
            img = np.zeros([h, w])
            for _ in range(3):
                fx, fy = rng.uniform(-2.5, 2.5, size=2)
                img += rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * (fx * xx + fy * yy) + rng.uniform(0, 2 * np.pi))
            img = 0.5 + 0.4 * img / np.abs(img).max()
            out[i, :, c] = img.reshape(-1)
    return torch.from_numpy(out)


def moment_stats(t):
    a = t.detach().double()
    return np.array([a.sum().item(), a.abs().sum().item(), (a * a).sum().item()])


def load_rd_fixture(n_test=64):
    """The reference's rate-distortion runs with a prior it trained itself (oracle/make_golden.py --only rd): n_test = 16 ->
    rd_trained_cifar.npz (round 3: 16 held-out images, four repetitions per rate, + the pinned noise stream of the first);
    n_test = 64 -> rd_trained_cifar_n64_r0.npz / _r1.npz (round 4: 64 held-out images -- a run's mean PSNR is a mean over four
    times as many images -- one file per rate).  Returns a dict with the union of the keys (r0_*, r1_*, schedule, data seeds)."""
    if n_test == 16:
        return dict(np.load(os.path.join(GOLDEN, "rd_trained_cifar.npz"), allow_pickle=False))
    out = {}
    import glob
    for ri in (0, 1):
        files = [os.path.join(GOLDEN, "rd_trained_cifar_n%d_r%d.npz" % (n_test, ri))]
        files += sorted(glob.glob(os.path.join(GOLDEN, "rd_trained_cifar_n%d_r%d_s*.npz" % (n_test, ri))))     # further repetitions
        for fi, f in enumerate(files):
            d = np.load(f, allow_pickle=False)
            for k in d.files:
                if k.startswith("r") and k[1].isdigit() and not k.startswith("r%d_" % ri):
                    continue
                per_run = k.startswith("r%d_" % ri) and k.split("_", 1)[1] in ("traj", "em_seed", "psnr_train", "n_groups", "bpp",
                                                                              "psnr_after_opt", "psnr")
                if fi == 0 or k not in out:
                    out[k] = d[k]
                elif per_run:                      # repetitions of the same experiment: stacked along the run axis
                    out[k] = np.concatenate([np.asarray(out[k]), np.asarray(d[k])], 0)
    return out


def product_checkpoint():
    """the checkpoint of the product -> reference interchange test (drivers.save_checkpoint's eight objects: a grouping of
    seeded KL weights, a seeded prior, seeded mappings -- the upsampling net with its fast-path cache attached, which must not
    travel) and the predict() input of that test.  oracle/make_golden.py --only ckpt_read has the reference read it."""
    from recombiner_amd import config, prior_model as PM, utils
    from recombiner_amd.upsample_fast import phase_module
    cfg = config.configs["cifar"]
    dims = [cfg["input_dim"]] + cfg["hidden_dims"] + [cfg["output_dim"]]
    torch.manual_seed(3)
    lt = PM.LinearTransform(dims)
    up = PM.Upsample(cfg["data_dim"], cfg["paddings"], cfg["layerwise_scale_factors"])
    phase_module(up)
    D = 3267 + 512
    g1 = PM.get_grouping_by_kl(np.random.RandomState(0).gamma(0.7, 4.0, size=D).astype(np.float32))
    gen = torch.Generator().manual_seed(1)
    p_loc, p_scale = 0.01 * torch.randn(D, generator=gen), 0.02 + 0.01 * torch.rand(D, generator=gen)
    avg_ls = -4 + 0.1 * torch.randn(D, generator=gen)
    ck = [g1, (p_loc, p_scale, 3e-7, avg_ls), (None,) * 8, (None, None, 3e-7, None), (None,) * 8, (None, None, 3e-7, None), lt, up]
    X, _ = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], 1, 3, seed=0)
    return ck, X


def pickle_globals(path, resolve=None):
    """-> (objects, sorted `module.name` globals): the file of sequential pickles read with find_class recording every global it
    asks its reader to resolve; `resolve` maps such a name to a class of the reader's choice (else the usual lookup)."""
    import pickle
    seen = set()

    class Recorder(pickle.Unpickler):
        def find_class(self, module, name):
            seen.add(module + "." + name)
            if resolve and module + "." + name in resolve:
                return resolve[module + "." + name]
            return super().find_class(module, name)

    objs = []
    with open(path, "rb") as f:
        while f.peek(1):
            objs.append(Recorder(f).load())
    return objs, sorted(seen)
