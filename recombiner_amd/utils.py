"""Host-side helpers of the hot path: layer bookkeeping, patch stitching around the upsampling
net, synthetic coordinate inputs, metrics.  Mirrors the helper surface of the reference's
utils.py (names and argument meaning).  The arithmetic-heavy helper of the reference,
`map_hierarchical_model_to_int_weights` (utils.py:122-198), is the HIP sampling kernel
(`rcb_reparam_fwd` over index maps built by `hierarchy_row_maps`): the model classes call the
kernel on their own parameters, the function of that name below keeps the reference's signature
for code that calls it directly.
"""
import copy

import numpy as np
import torch


# ---------------------------------------------------------------------------------------------
# parameter bookkeeping (utils.py:216-232)
# ---------------------------------------------------------------------------------------------
def count_layer_params(in_dim, out_dim):
    return in_dim * out_dim + out_dim


def count_net_params(in_dim, hidden_dims, out_dim):
    dims = [in_dim] + list(hidden_dims) + [out_dim]
    n_params = [count_layer_params(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]
    return n_params, np.cumsum(n_params)


# ---------------------------------------------------------------------------------------------
# hierarchy index maps (utils.py:151-185 expressed as gathers)
# ---------------------------------------------------------------------------------------------
def hierarchy_row_maps(n_inr, patch_nums, hierarchical_patch_nums, data_dim):
    """patch n -> row of the level-2 posterior, row of the level-3 posterior."""
    ppd = int(np.prod(patch_nums))
    l2 = hierarchical_patch_nums["level2"]
    ngrp = [patch_nums[i] // l2[i] for i in range(data_dim)]
    n = np.arange(n_inr)
    datum, local = n // ppd, n % ppd
    pos = np.unravel_index(local, patch_nums)
    grp = np.ravel_multi_index(tuple(pos[i] // l2[i] for i in range(data_dim)), ngrp)
    return (datum * int(np.prod(ngrp)) + grp).astype(np.int64), datum.astype(np.int64)


class _HierSampleFn(torch.autograd.Function):
    """sum over the levels of loc_L[row_L(n)] + scale_L[row_L(n)] * eps_L[n, s]: rcb_reparam_fwd with
    rcb_level.scale_is_sigma; the adjoint (sums over samples and over the patches that share a row) is torch plumbing."""

    @staticmethod
    def forward(ctx, S, maps, eps, *params):
        from . import ops
        n = params[0].shape[0]
        lv = [ops.LevelSpec(params[2 * i].detach().contiguous(), params[2 * i + 1].detach().contiguous(), params[0].shape[1], n,
                            row_map=maps[i], scale_is_sigma=True) for i in range(len(maps))]
        ctx.maps, ctx.eps, ctx.rows = maps, eps, [p.shape[0] for p in params[::2]]
        return ops.reparam_fwd(lv, eps, S)

    @staticmethod
    def backward(ctx, g):
        out = []
        for m, e, r in zip(ctx.maps, ctx.eps, ctx.rows):
            gl, gs = g.sum(1), (g * e).sum(1)
            if m is not None:
                idx = torch.as_tensor(m, device=g.device, dtype=torch.long)
                gl = torch.zeros(r, g.shape[-1], device=g.device, dtype=g.dtype).index_add_(0, idx, gl)
                gs = torch.zeros(r, g.shape[-1], device=g.device, dtype=g.dtype).index_add_(0, idx, gs)
            out += [gl, gs]
        return (None, None, None, *out)


def map_hierarchical_model_to_int_weights(use_hierarchical_model, loc, scale, h_loc, h_scale, hh_loc, hh_scale, sample_size,
                                          hierarchical_patch_nums, patch_nums, data_dim, noise_source=None):
    """Samples the (1- or 3-level) hierarchical model to the INR weights before the linear transform, `h_w`
    [N, sample_size, D] -- the reference's function of this name (utils.py:122-198; same positional arguments: `scale` etc.
    are standard deviations, i.e. st(log_scale) with the encoded-group masks already applied, as prior_model.py:140-145 and
    test_model.py:289-298 pass them).  Per element, in the reference's operation order:
        h_w[n, s] = (loc[n] + scale[n] * e1[n, s]) + (h_loc[r2(n)] + e2[n, s] * h_scale[r2(n)]) + (hh_loc[r3(n)] + hh_scale[r3(n)] * e3[n, s])
    with r2 / r3 the level-2 / level-3 rows of patch n (`hierarchy_row_maps`; the reference materialises them with
    reshape / repeat).  One launch of `rcb_reparam_fwd` (rcb_level.scale_is_sigma = 1); differentiable in all six tensors.
    Noise: three standard-normal draws of shape [N, sample_size, D] in the order level 1, 2, 3 (one draw when
    `use_hierarchical_model` is false) from the device generator, as `torch.randn_like` upstream, or from
    `noise_source(shape)` (extra keyword, used by the parity tests to inject the reference's stream)."""
    from . import ops
    if not loc.is_cuda:
        raise ops.RcbError("map_hierarchical_model_to_int_weights: tensors must live on the GPU (no CPU fallback exists)")
    N, D = loc.shape
    S = int(sample_size)

    def draw():
        if noise_source is not None:
            return noise_source((N, S, D)).to(loc.device, torch.float32).reshape(N, S, D).contiguous()
        return torch.randn(N, S, D, device=loc.device, dtype=torch.float32)

    if use_hierarchical_model:
        if data_dim not in (1, 2, 3):
            raise NotImplementedError
        m2, m3 = hierarchy_row_maps(N, patch_nums, hierarchical_patch_nums, data_dim)
        if h_loc.shape[0] != int(m2.max()) + 1 or hh_loc.shape[0] != int(m3.max()) + 1:
            raise ops.RcbError("map_hierarchical_model_to_int_weights: level-2 / level-3 rows do not match the patch hierarchy")
        maps, params = (None, m2, m3), (loc, scale, h_loc, h_scale, hh_loc, hh_scale)
    else:
        maps, params = (None,), (loc, scale)
    eps = tuple(draw() for _ in maps)
    params = tuple(p.to(torch.float32) for p in params)
    return _HierSampleFn.apply(S, maps, eps, *params)


# ---------------------------------------------------------------------------------------------
# latent positional encodings -> per-pixel inputs (utils.py:4-120)
# ---------------------------------------------------------------------------------------------
def map_lpe_to_inr_inputs(upsample_net, latent_pe, latent_dim, pixel_sizes, upsample_factors, patch, patch_nums,
                          data_dim, stitched=False):
    """latent_pe [S, N, ...] -> pe [N, S, P, C_out] (channel-last, P row-major over the pixel grid).
    Patched presets: the latent grids of all patches of a datapoint are stitched into one grid,
    upsampled together, and cut back into patches.
    `stitched` (patched presets only): skip the cut-back and return the upsampling net's channel-last output on the stitched
    grids, [S * n_datapoints, *(patch_nums[i] * pixel_sizes[i]), C_out], for kernels that address the patches inside it
    (rcb_siren_desc.pe_grid_dims, ops.PeLayout(patch_nums, pixel_sizes))."""
    S, N = latent_pe.shape[:2]
    lat = [pixel_sizes[i] // upsample_factors[i] for i in range(data_dim)]
    z = latent_pe.reshape(S, N, *lat, -1)
    assert z.shape[-1] == latent_dim
    if not patch:
        o = upsample_net(z.reshape(S * N, *lat, latent_dim).movedim(-1, 1)).movedim(1, -1)
        pe = o.reshape(S, N, -1, o.shape[-1])
    else:
        pn = list(patch_nums)
        nd = N // int(np.prod(pn))
        z = z.reshape(S, nd, *pn, *lat, latent_dim)
        inter = [2 + i + j * data_dim for i in range(data_dim) for j in range(2)]
        z = z.permute([0, 1] + inter + [2 + 2 * data_dim])
        z = z.reshape(S * nd, *[pn[i] * lat[i] for i in range(data_dim)], latent_dim)
        o = upsample_net(z.movedim(-1, 1)).movedim(1, -1)
        if stitched:
            return o.contiguous()
        ch = o.shape[-1]
        split = [v for i in range(data_dim) for v in (pn[i], pixel_sizes[i])]
        o = o.reshape(S, nd, *split, ch)
        back = [2 + 2 * i for i in range(data_dim)] + [3 + 2 * i for i in range(data_dim)]
        pe = o.permute([0, 1] + back + [2 + 2 * data_dim]).reshape(S, N, -1, ch)
    return pe.permute(1, 0, 2, 3)


# ---------------------------------------------------------------------------------------------
# synthetic coordinate inputs (utils.py:265-297 + data/image.py:24-27)
# ---------------------------------------------------------------------------------------------
def make_coord_grid(shape, range, device=None):
    axes = []
    for i, s in enumerate(shape):
        lo, hi = range[i] if isinstance(range[0], (list, tuple)) else range
        axes.append(lo + (hi - lo) * ((0.5 + torch.arange(s, device=device)) / s))
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)


def to_grid_coordinates_and_features(datum):
    """datum [C, *spatial] -> (coords [P, dd] in (-1,1), features [P, C])."""
    sp = datum.shape[1:]
    coords = make_coord_grid(sp, (-1, 1), device=datum.device).view(-1, len(sp))
    return coords, datum.reshape(datum.shape[0], -1).T


def fourier_embed(coords, feature_size):
    """cat(cos(pi v), sin(pi v)), v = coords (x) exp(linspace(0, ln 1024, F/(2 dd)))."""
    dd = coords.shape[-1]
    w = torch.exp(torch.linspace(0, np.log(1024), feature_size // (2 * dd), device=coords.device))
    v = torch.matmul(coords.unsqueeze(-1), w.unsqueeze(0)).view(*coords.shape[:-1], -1)
    return torch.cat([torch.cos(np.pi * v), torch.sin(np.pi * v)], dim=-1)


def synthetic_inputs(pixel_sizes, fourier_dim, n_inr, out_dim, seed=0):
    """Benchmark inputs: X[P,F] from the coordinate grid, Y ~ U[0,1) [N,P,C] (CPU RNG)."""
    coords, _ = to_grid_coordinates_and_features(torch.zeros(1, *pixel_sizes))
    X = fourier_embed(coords, fourier_dim)
    g = torch.Generator().manual_seed(seed)
    Y = torch.rand(n_inr, X.shape[0], out_dim, generator=g)
    return X, Y


def preset_inputs(config, device=None):
    """The coordinate features of one patch (one datapoint of an unpatched preset), X [P, F]: the grid of `pixel_sizes`
    embedded with `fourier_dim` features (data/image.py:24-27) -- what synthetic_inputs returns as X.  Evaluated on the CPU,
    like the reference's loaders, then moved to `device`: one array shared by all rows."""
    coords, _ = to_grid_coordinates_and_features(torch.zeros(1, *config["pixel_sizes"]))
    X = fourier_embed(coords, config["fourier_dim"])
    return X if device is None else X.to(device)


# ---------------------------------------------------------------------------------------------
# whole signals in memory -> what rcb_signal_patch reads (data/image.py:17-46, data/video.py:40-73, data/audio.py:112-140)
# ---------------------------------------------------------------------------------------------
class SampleFormat:
    """How the samples of a whole signal are stored (include/rcb.h, N4 412): a kind and, for u16, a depth.
      u8()     uint8, y = q / 255                                   -- what the image / video presets imply
      f32()    fp32, the bits unchanged; raw on the way out          -- what the audio / protein presets imply
      u16(b)   b-bit samples (9 <= b <= 16) in 16-bit unsigned words, y = q / (2^b - 1); a stored value above 2^b - 1 is not
               clamped.  torch.uint16, or an int16 tensor whose bits are reinterpreted
      s16()    16-bit PCM, y = (q + 32768) / 65536: the audio preset's (q / 32768 + 1) / 2 of data/audio.py:50-54, bit for bit
    `kind` is the library's src_kind and, on the way out, its mode (ops.RECON_8BIT / RECON_RAW / RECON_U16 / RECON_S16)."""
    U8, F32, U16, S16 = 0, 1, 2, 3
    _NAMES = {0: "u8", 1: "f32", 2: "u16", 3: "s16"}

    def __init__(self, kind, depth=0):
        if isinstance(kind, bool) or isinstance(depth, bool) or not isinstance(kind, (int, np.integer)) \
                or not isinstance(depth, (int, np.integer)):
            raise ValueError("SampleFormat: kind %r and depth %r must be integers" % (kind, depth))
        if kind not in self._NAMES:
            raise ValueError("SampleFormat: kind %r (0 = u8, 1 = f32, 2 = u16, 3 = s16)" % (kind,))
        if kind == self.U16 and not 9 <= depth <= 16:
            raise ValueError("SampleFormat: a u16 depth of %r (9 .. 16; 8-bit samples are u8)" % (depth,))
        if kind != self.U16 and depth != 0:
            raise ValueError("SampleFormat: %s has no depth (got %r)" % (self._NAMES[kind], depth))
        self.kind, self.depth = int(kind), int(depth)

    @classmethod
    def u8(cls):
        return cls(cls.U8)

    @classmethod
    def f32(cls):
        return cls(cls.F32)

    @classmethod
    def u16(cls, depth):
        return cls(cls.U16, depth)

    @classmethod
    def s16(cls):
        return cls(cls.S16)

    @classmethod
    def implied(cls, dataset):
        """the format a preset implies, which a bitstream need not carry: u8 where the metric rounds, else f32"""
        return cls.u8() if METRIC_ROUNDS[dataset] else cls.f32()

    @property
    def dtype(self):
        """the torch dtype of the samples (and of the integer output of ops.recon_finish)"""
        return (torch.uint8, torch.float32, torch.uint16, torch.int16)[self.kind]

    # THE integer-dtype rule: the torch dtype of the integers a reconstruction is delivered in, by kind (the library's mode); f32
    # has none, nor has a number that is no kind.  ops.recon_finish* and the bitstream decoders read it here
    INT_DTYPES = {U8: torch.uint8, U16: torch.uint16, S16: torch.int16}

    @property
    def int_dtype(self):
        return self.INT_DTYPES.get(self.kind)

    @property
    def is_integer(self):
        return self.int_dtype is not None

    def accepts(self, dtype):
        """whether a source tensor of `dtype` can be read in this format: its own dtype; u16 also takes int16 (the bits)"""
        return dtype == self.dtype or (self.kind == self.U16 and dtype == torch.int16)

    def __eq__(self, other):
        return isinstance(other, SampleFormat) and (self.kind, self.depth) == (other.kind, other.depth)

    def __hash__(self):
        return hash((self.kind, self.depth))

    def __repr__(self):
        return "SampleFormat.%s(%s)" % (self._NAMES[self.kind], self.depth if self.kind == self.U16 else "")


def preset_grid(config):
    """(patch_nums, patch_size) of a preset's whole signal: its patch grid, or one patch for the unpatched presets"""
    dd = config["data_dim"]
    ps = [int(v) for v in config["pixel_sizes"][:dd]]
    pn = [int(v) for v in config["patch_nums"][:dd]] if config["patch"] else [1] * dd
    return pn, ps


def signal_layout(config):
    """ops.PeLayout of a preset's whole signals (ops.signal_patch / ops.recon_finish); patch_nums of ones when unpatched"""
    from . import ops
    return ops.PeLayout(*preset_grid(config))


def signal_view(config, tensor, channels_first=False, origin=None, landscape=True):
    """A VIEW [n, *G, C] of signals in memory -- [n, *spatial, C], or [n, C, *spatial] with channels_first -- on the preset's grid G = patch_nums * pixel_sizes (pixel_sizes when unpatched): the channel axis moved
    last and the window of that size at `origin` (default 0 on every axis: the leading whole patches, which is what the
    reference's `range(x // patch_sizes[i])` loops keep).  landscape (2-D presets): the two spatial axes are swapped when the
    first is longer than the second, as data/image.py:18-19 rotates a portrait image; origin then counts on the swapped axes.
    Nothing is copied: ops.signal_patch takes the strides as they are.  ValueError when the signal is smaller than the preset
    (or the window leaves it), or its channels are not the preset's."""
    dd = config["data_dim"]
    if tensor.dim() != dd + 2:
        raise ValueError("signal_view: %d axes for a %d-D preset ([n, *spatial, C] expected)" % (tensor.dim(), dd))
    if channels_first:
        tensor = tensor.movedim(1, -1)
    if dd == 2 and landscape and tensor.shape[1] > tensor.shape[2]:
        tensor = tensor.transpose(1, 2)
    if tensor.shape[-1] != config["output_dim"]:
        raise ValueError("signal_view: %d channels, the preset has %d" % (tensor.shape[-1], config["output_dim"]))
    pn, ps = preset_grid(config)
    origin = [0] * dd if origin is None else [int(v) for v in origin]
    if len(origin) != dd:
        raise ValueError("signal_view: origin of %d entries for a %d-D preset" % (len(origin), dd))
    for i in range(dd):
        size = pn[i] * ps[i]
        if origin[i] < 0 or origin[i] + size > tensor.shape[1 + i]:
            raise ValueError("signal_view: axis %d of the signal has %d pixels, the preset's window [%d, %d) does not fit"
                             % (i, tensor.shape[1 + i], origin[i], origin[i] + size))
        tensor = tensor.narrow(1 + i, origin[i], size)
    return tensor


def fit_config(config, size):
    """A copy of the preset `config` whose grid holds a signal of `size` (one entry per spatial axis); the preset itself is
    never changed.  Patched presets: patch_nums[i] = ceil(size[i] / pixel_sizes[i]) rounded up to a multiple of
    hierarchical_patch_nums["level2"][i] (level 2 groups that many patches per axis), level3 = the new patch_nums, level2 as
    it is.  Unpatched presets: the config is unchanged and a size[i] > pixel_sizes[i] is a ValueError (one INR, one grid).
    The signal is then edge-padded to the grid (ops.signal_patch_pad) and cropped after decoding (ops.recon_finish(size=)).  The
    priors and groupings of a checkpoint are per parameter, so one trained at the preset's patch_nums drives any fitted config."""
    dd = config["data_dim"]
    size = [int(v) for v in size]
    if len(size) != dd or min(size) < 1:
        raise ValueError("fit_config: size %r for a %d-D preset (one positive entry per axis)" % (size, dd))
    ps = [int(v) for v in config["pixel_sizes"][:dd]]
    out = copy.deepcopy(config)
    if not config["patch"]:
        for i in range(dd):
            if size[i] > ps[i]:
                raise ValueError("fit_config: axis %d of the signal has %d positions, the unpatched preset's grid %d"
                                 % (i, size[i], ps[i]))
        return out
    l2 = [int(v) for v in config["hierarchical_patch_nums"]["level2"][:dd]]
    pn = [-(-(-(-size[i] // ps[i])) // l2[i]) * l2[i] for i in range(dd)]
    out["patch_nums"] = pn + list(config["patch_nums"][dd:])
    out["hierarchical_patch_nums"]["level3"] = list(out["patch_nums"])
    return out


def ragged_plan(config, sizes, landscape=True):
    """How a list of signals of mixed sizes and orientations is coded (drivers.compress_signal_list): pure host arithmetic.
    sizes[k]: signal k's extent per spatial axis, as it lies in memory.  Per signal the swap is decided -- 2-D presets with
    `landscape`, when the first axis is longer than the second, as signal_view rotates a portrait image -- and the signals are
    grouped into buckets by the grid that fit_config gives the (possibly swapped) size: signals share a model when they fit the
    same patch grid.  -> (swaps: a bool per signal, buckets: a list of dicts
        patch_nums  the fitted grid's patches per axis (ones for the unpatched presets, which have one bucket),
        config      the fitted config,
        indices     the signals of the bucket, in input order,
        sizes       their extents along the model's axes (after the swap)),
    buckets in the order of their first signal.  ValueError where fit_config raises it (an unpatched preset and a larger signal)."""
    dd = config["data_dim"]
    swaps, buckets, by_grid = [], [], {}
    for k, size in enumerate(sizes):
        size = [int(v) for v in size]
        if len(size) != dd:
            raise ValueError("ragged_plan: signal %d has %d axes, the preset %d" % (k, len(size), dd))
        sw = bool(dd == 2 and landscape and size[0] > size[1])
        if sw:
            size = [size[1], size[0]]
        fitted = fit_config(config, size)
        key = tuple(preset_grid(fitted)[0])
        if key not in by_grid:
            by_grid[key] = dict(patch_nums=list(key), config=fitted, indices=[], sizes=[])
            buckets.append(by_grid[key])
        by_grid[key]["indices"].append(k)
        by_grid[key]["sizes"].append(tuple(size))
        swaps.append(sw)
    return swaps, buckets


# ---------------------------------------------------------------------------------------------
# metrics (utils.py:200-260) -- host numpy, as in the reference
# ---------------------------------------------------------------------------------------------
def _round8(c):
    return np.round(np.clip(c, 0, 1) * 255) / 255


def PSNR(original, compressed, round, max_value=1):
    if round:
        compressed = _round8(compressed)
    mse = np.mean((original - compressed) ** 2)
    return (20 * np.log10(max_value / np.sqrt(mse))).item()


def batch_PSNR(original, compressed, round, max_value=1):
    b = original.shape[0]
    if round:
        compressed = _round8(compressed)
    mse = np.mean((original.reshape(b, -1) - compressed.reshape(b, -1)) ** 2, axis=-1)
    return 20 * np.log10(max_value / np.sqrt(mse))


def batch_RMSD(original, compressed, scale_factor):
    b = original.shape[0]
    return (((original * scale_factor - compressed * scale_factor) ** 2).reshape(b, -1).mean(-1) * 3) ** 0.5


def metric(original, compressed, dataset):
    if dataset == "cifar":
        return batch_PSNR(original, compressed, round=True, max_value=1)
    if dataset in ("kodak", "video"):
        return PSNR(original, compressed, round=True, max_value=1)
    if dataset == "audio":
        return PSNR(original, compressed, round=False, max_value=1)
    if dataset == "protein":
        return batch_RMSD(original, compressed, scale_factor=25)
    raise ValueError(dataset)


# ---------------------------------------------------------------------------------------------
# the same figures from exact per-datapoint sums formed on the device (rcb_recon_finish)
# ---------------------------------------------------------------------------------------------
METRIC_ROUNDS = {"cifar": True, "kodak": True, "video": True, "audio": False, "protein": False}


def metric_from_sse(sse, n_elems, dataset):
    """`metric` from the per-datapoint fp64 sums of squared errors `sse` [n_data] (ops.recon_finish: 8-bit mode for cifar /
    kodak / video, raw mode for audio / protein) and the element count of one datapoint, all in fp64:
    cifar -> PSNR per datapoint [n_data]; kodak / video / audio -> one PSNR over the whole batch (a float); protein ->
    RMSD per datapoint, 25 * sqrt(3 * sse / n).  Where `metric` takes a float32 mean in numpy's pairwise order, this divides
    an fp64 sum once.
    n_elems may be an array [n_data] of per-datapoint element counts (signals of mixed sizes, ops.recon_finish_ragged): the
    per-datapoint figures use sse_d / n_d, the batch-wide one sum(sse) / sum(n)."""
    if dataset not in METRIC_ROUNDS:
        raise ValueError(dataset)
    sse = np.asarray(sse, dtype=np.float64).reshape(-1)
    counts = np.asarray(n_elems, dtype=np.float64).reshape(-1)
    if np.ndim(n_elems) == 0:                                # one count for every datapoint
        counts = np.broadcast_to(counts, sse.shape)
    elif counts.size != sse.size:
        raise ValueError("metric_from_sse: %d element counts for %d datapoints" % (counts.size, sse.size))
    if dataset == "cifar":
        return -10.0 * np.log10(sse / counts)
    if dataset == "protein":
        return 25.0 * np.sqrt(3.0 * sse / counts)
    return (-10.0 * np.log10(sse.sum() / counts.sum())).item()


def metric_device(y_true, y_pred, dataset, layout=None, size=None, sample_format=None, sizes=None):
    """`metric(y_true, y_pred, dataset)` for GPU tensors [N, P, C] without copying them to the host: one pass of
    rcb_recon_finish (rounding to 8 bits where the dataset's metric does), then only the per-datapoint sums -- and the counts
    of non-finite elements, which make a datapoint's figure NaN as numpy's would be -- are read back.  layout: ops.PeLayout
    of a patched preset (rows = patches of stitched signals) or None (rows = datapoints); the batch-wide figures do not
    depend on it.
    size (needs a layout; patch_nums of ones for an unpatched preset): only the leading size[i] positions per axis of every
    signal are real, the rest edge padding (ops.signal_patch_pad) -- the figure is over the real samples alone
    (rcb_recon_finish_crop), the mean over prod(size) * C elements per signal.
    sample_format (SampleFormat): the lattice the reconstruction is rounded to -- it overrides the dataset's choice, so the figure is
    the distortion of the signal a decoder delivers in that format (rcb_recon_finish_fmt); the formula stays the dataset's.
    sizes (instead of size; needs a layout): one extent PER SIGNAL (rcb_recon_finish_ragged) -- per-datapoint figures over each
    signal's own prod(size) * C elements, the batch-wide figure over all real samples of the batch."""
    from . import ops
    if dataset not in METRIC_ROUNDS:
        raise ValueError(dataset)
    mode = ops.RECON_8BIT if METRIC_ROUNDS[dataset] else ops.RECON_RAW
    y_pred = y_pred.detach().to(torch.float32).contiguous()
    y_true = y_true.detach().to(device=y_pred.device, dtype=torch.float32).contiguous()
    Cc = y_pred.shape[-1]
    if sizes is not None:
        if size is not None:
            raise ValueError("metric_device: size and sizes exclude each other")
        _, _, sse, _n_bad = ops.recon_finish_ragged(y_pred, y_true, layout=layout, sizes=sizes, mode=mode, sample_format=sample_format)
        counts = np.asarray([int(np.prod([int(v) for v in s])) * Cc for s in sizes])
    else:
        _, _, sse, _n_bad = ops.recon_finish(y_pred, y_true, layout=layout, mode=mode, size=size, sample_format=sample_format)
        counts = y_pred.numel() // sse.numel() if size is None else int(np.prod([int(v) for v in size])) * Cc
    return metric_from_sse(sse.cpu().numpy(), counts, dataset)


# ---------------------------------------------------------------------------------------------
# the same figures by region -- per frame, per patch, per tile (rcb_recon_regions, include/rcb.h N4 417)
# ---------------------------------------------------------------------------------------------
def region_grid(extent, region):
    """boxes per axis when `extent` is tiled by boxes of `region` positions: nr[i] = ceil(extent[i] / region[i]); the boxes on the
    far edge are smaller.  ValueError for axes that do not match or an entry below 1."""
    extent, region = [int(v) for v in extent], [int(v) for v in region]
    if len(extent) != len(region) or not extent or min(extent) < 1 or min(region) < 1:
        raise ValueError("region_grid: extent %r and region %r (as many positive entries each)" % (extent, region))
    return tuple(-(-e // r) for e, r in zip(extent, region))


def region_counts(extent, region, channels):
    """int64 [*nr]: the elements of every box, prod(box_i) * channels -- what a region's sum is divided by.  Host arithmetic."""
    nr = region_grid(extent, region)
    counts = np.full(nr, int(channels), dtype=np.int64)
    for i, (e, r, n) in enumerate(zip(extent, region, nr)):
        e, r = int(e), int(r)
        box = np.minimum(r, e - np.arange(n, dtype=np.int64) * r)
        counts = counts * box.reshape([-1 if j == i else 1 for j in range(len(nr))])
    return counts


def region_of(config_or_layout, by):
    """The box of the usual regions of a preset (a config dict) or an ops.PeLayout, one entry per spatial axis:
      "patch"   patch_size: one figure per patch of the codec;
      "frame"   (1, G1, G2), 3-D only: one figure per frame of a clip -- the video convention is the mean of these per-frame PSNRs;
      "row"     one position of axis 0 and the whole of the others;
      a tuple of ints is taken as it is (one entry per axis, each >= 1)."""
    if isinstance(config_or_layout, dict):
        pn, ps = preset_grid(config_or_layout)
    else:
        pn, ps = list(config_or_layout.patch_nums), list(config_or_layout.patch_size)
    grid = [a * b for a, b in zip(pn, ps)]
    if isinstance(by, str):
        if by == "patch":
            return tuple(ps)
        if by == "frame":
            if len(grid) != 3:
                raise ValueError("region_of: frames are the positions of axis 0 of a 3-D signal, this one has %d axes" % len(grid))
            return (1, grid[1], grid[2])
        if by == "row":
            return (1, *grid[1:])
        raise ValueError("region_of: %r ('patch', 'frame', 'row' or a tuple of ints)" % (by,))
    box = tuple(int(v) for v in by)
    if len(box) != len(grid) or min(box) < 1:
        raise ValueError("region_of: a box of %r for a signal of %d axes (one entry >= 1 per axis)" % (box, len(grid)))
    return box


def metric_regions_from_sse(sse_r, counts, dataset):
    """Per-region figures [n_data, *nr] in fp64 from the sums `sse_r` [n_data, *nr] (ops.recon_regions) and the element counts
    [*nr] (region_counts): PSNR = -10 log10(sse / n) for cifar / kodak / video / audio, RMSD = 25 sqrt(3 sse / n) for protein.
    Every region gets its own figure, whatever the dataset's batch convention.  NaN passes through; a zero error gives inf."""
    if dataset not in METRIC_ROUNDS:
        raise ValueError(dataset)
    sse_r = np.asarray(sse_r, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.float64)
    if sse_r.ndim < 1 or tuple(sse_r.shape[1:]) != tuple(counts.shape):
        raise ValueError("metric_regions_from_sse: sums of shape %r, counts of shape %r" % (sse_r.shape, counts.shape))
    mse = sse_r / counts[None]
    if dataset == "protein":
        return 25.0 * np.sqrt(3.0 * mse)
    with np.errstate(divide="ignore"):
        return -10.0 * np.log10(mse)


def metric_regions_device(y_true, y_pred, dataset, layout, region, size=None, sample_format=None):
    """The dataset's figure per region of every signal, fp64 [n_data, *nr], for GPU tensors [N, P, C] without copying them to the
    host: one pass of rcb_recon_regions (rounding to 8 bits where the dataset's metric does, as metric_device), then only the
    per-region sums are read back.  layout: the signals' ops.PeLayout (patch_nums of ones when unpatched); region: one int per
    axis (region_of); size: the signals' real extent inside the grid -- the regions tile it, and padding belongs to none;
    sample_format: the lattice the reconstruction is rounded to instead of the dataset's choice."""
    from . import ops
    if dataset not in METRIC_ROUNDS:
        raise ValueError(dataset)
    mode = ops.RECON_8BIT if METRIC_ROUNDS[dataset] else ops.RECON_RAW
    y_pred = y_pred.detach().to(torch.float32).contiguous()
    y_true = y_true.detach().to(device=y_pred.device, dtype=torch.float32).contiguous()
    extent = [int(v) for v in size] if size is not None else [a * b for a, b in zip(layout.patch_nums, layout.patch_size)]
    counts = region_counts(extent, region, y_pred.shape[-1])
    sse_r, _n_bad_r = ops.recon_regions(y_pred, y_true, layout, region, mode=mode, size=size, sample_format=sample_format)
    return metric_regions_from_sse(sse_r.cpu().numpy(), counts, dataset)


# ---------------------------------------------------------------------------------------------
# SSIM / MS-SSIM of delivered integers against the source's, from the exact fixed-point sums of rcb_ssim (include/rcb.h, N4 414)
# ---------------------------------------------------------------------------------------------
SSIM_TAPS = 11
SSIM_FX_SCALE = float(1 << 36)                               # RCB_SSIM_FX_SCALE
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def ssim_window():
    """THE window of rcb_ssim: 11 taps, sigma 1.5, normalised, numpy fp64 -- formed here and nowhere else; the device gets the
    11 doubles and evaluates no exp"""
    k = np.arange(SSIM_TAPS, dtype=np.float64)
    g = np.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2))
    return g / g.sum()


def ssim_constants(sample_format):
    """(C1, C2) = ((0.01 L)^2, (0.03 L)^2) of an integer sample format, L = 255 (u8) or 2^depth - 1 (u16)"""
    if sample_format.kind not in (SampleFormat.U8, SampleFormat.U16):
        raise ValueError("SSIM is defined here for u8 and u16 samples, not %r" % (sample_format,))
    L = 255 if sample_format.kind == SampleFormat.U8 else (1 << sample_format.depth) - 1
    return (0.01 * L) ** 2, (0.03 * L) ** 2


def ssim_positions(H, W, scale=0):
    """window positions of scale `scale` of an H x W image: (floor(H / 2^s) - 10) * (floor(W / 2^s) - 10)"""
    return ((int(H) >> scale) - (SSIM_TAPS - 1)) * ((int(W) >> scale) - (SSIM_TAPS - 1))


def _ssim_sums_host(sums, H, W, scales=None):
    """-> (the sums as numpy int64 [n, scales, C, 2], H per image, W per image); H and W are one size for all images or one
    per image"""
    s = sums.detach().cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    if s.ndim != 4 or s.shape[-1] != 2 or s.dtype != np.int64:
        raise ValueError("the sums of rcb_ssim are int64 [n, scales, C, 2], got %s %r" % (s.dtype, s.shape))
    if scales is not None and s.shape[1] != scales:
        raise ValueError("%d scales are needed, the sums hold %d" % (scales, s.shape[1]))
    per = []
    for name, v in (("H", H), ("W", W)):
        v = [int(u) for u in np.asarray(v).reshape(-1)] if np.ndim(v) else [int(v)] * s.shape[0]
        if len(v) != s.shape[0]:
            raise ValueError("%d values of %s for the sums of %d images" % (len(v), name, s.shape[0]))
        per.append(v)
    for h, w in zip(*per):
        if ssim_positions(h, w, s.shape[1] - 1) < 1 or min(h >> (s.shape[1] - 1), w >> (s.shape[1] - 1)) < SSIM_TAPS:
            raise ValueError("an image of %d x %d has no %d scales (both sides at least %d)"
                             % (h, w, s.shape[1], SSIM_TAPS << (s.shape[1] - 1)))
    return s, per[0], per[1]


def ssim_from_sums(sums, H, W):
    """SSIM per image, fp64 [n], from rcb_ssim's sums [n, scales, C, 2] of H x W images (H, W: one size, or one per image as
    rcb_ssim_list scores them): the mean over the scale-0 positions and the channels, (exact integer sum over the channels) /
    2^36 / (positions * C)"""
    s, Hs, Ws = _ssim_sums_host(sums, H, W)
    return np.asarray([float(sum(int(v) for v in img[0, :, 0])) / SSIM_FX_SCALE / float(ssim_positions(h, w) * s.shape[2])
                       for img, h, w in zip(s, Hs, Ws)], dtype=np.float64)


def msssim_from_sums(sums, H, W):
    """MS-SSIM per image, fp64 [n], from five-scale sums (min(H, W) >= 176; H, W: one size, or one per image): per channel
    prod_{s<4} max(mean cs_s, 0)^w_s * max(mean ssim_4, 0)^w_4 with w = MSSSIM_WEIGHTS, the factors multiplied in scale order,
    then the mean over the channels -- the per-channel convention of the common PyTorch implementation.  Scale s is the
    floor-pooled one of rcb_ssim; for even sizes it coincides with the padded and the truncating conventions."""
    s, Hs, Ws = _ssim_sums_host(sums, H, W, scales=5)
    out = []
    for img, h, w in zip(s, Hs, Ws):
        total = None
        for c in range(s.shape[2]):
            p = None
            for k in range(5):
                mean = float(int(img[k, c, 1 if k < 4 else 0])) / SSIM_FX_SCALE / float(ssim_positions(h, w, k))
                f = max(mean, 0.0) ** MSSSIM_WEIGHTS[k]
                p = f if p is None else p * f
            total = p if total is None else total + p
        out.append(total / float(s.shape[2]))
    return np.asarray(out, dtype=np.float64)


def _ssim_need(who, H, W, multiscale):
    need = SSIM_TAPS << 4 if multiscale else SSIM_TAPS
    if min(H, W) < need:
        raise ValueError("%s: an image of %d x %d is too small for %s (both sides at least %d)"
                         % (who, H, W, "MS-SSIM's five scales" if multiscale else "SSIM's 11-tap window", need))


def ssim_device(a, b, sample_format=None, multiscale=False):
    """SSIM (or with `multiscale` MS-SSIM) of integer images on the GPU, fp64 [n]: a, b are [n, H, W, C] tensors of one integer
    dtype with ANY strides (ops.ssim_sums), or two LISTS of [H_k, W_k, C] tensors of mixed sizes and layouts, scored in one call
    whatever their number (ops.ssim_sums_list).  Only the sums are read back.  sample_format: ops.ssim_sums's.  An image too
    small for the scales asked (11 for SSIM, 176 for MS-SSIM, per side) is a ValueError."""
    from . import ops
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        if not isinstance(a, (list, tuple)) or not isinstance(b, (list, tuple)) or len(a) != len(b):
            raise ValueError("ssim_device: two lists of as many signals, or two tensors")
        if not a:
            return np.zeros(0, dtype=np.float64)
        for x in a:
            if x.dim() != 3:
                raise ValueError("ssim_device: images are [n, H, W, C], got %d axes" % (x.dim() + 1))
            _ssim_need("ssim_device", int(x.shape[0]), int(x.shape[1]), multiscale)
        sums = ops.ssim_sums_list(a, b, sample_format=sample_format, scales=5 if multiscale else 1)
        Hs, Ws = [int(x.shape[0]) for x in a], [int(x.shape[1]) for x in a]
        return msssim_from_sums(sums, Hs, Ws) if multiscale else ssim_from_sums(sums, Hs, Ws)
    if a.dim() != 4:
        raise ValueError("ssim_device: images are [n, H, W, C], got %d axes" % a.dim())
    H, W = int(a.shape[1]), int(a.shape[2])
    _ssim_need("ssim_device", H, W, multiscale)
    sums, _ = ops.ssim_sums(a, b, sample_format=sample_format, scales=5 if multiscale else 1)
    return msssim_from_sums(sums, H, W) if multiscale else ssim_from_sums(sums, H, W)


def ssim_frames_device(a, b, sample_format=None, multiscale=False):
    """SSIM (with `multiscale` MS-SSIM) per FRAME of integer clips a, b [n, T, H, W, C] (any strides) on the GPU, fp64 [n, T], in one
    call (ops.ssim_sums_frames); the caller averages.  sample_format and the size rule: ssim_device's."""
    from . import ops
    if a.dim() != 5:
        raise ValueError("ssim_frames_device: clips are [n, T, H, W, C], got %d axes" % a.dim())
    n, T, H, W = (int(v) for v in a.shape[:4])
    _ssim_need("ssim_frames_device", H, W, multiscale)
    if n * T == 0:
        return np.zeros((n, T), dtype=np.float64)
    sums = ops.ssim_sums_frames(a, b, sample_format=sample_format, scales=5 if multiscale else 1)
    flat = sums.reshape(n * T, *sums.shape[2:])
    return (msssim_from_sums(flat, H, W) if multiscale else ssim_from_sums(flat, H, W)).reshape(n, T)


# ---------------------------------------------------------------------------------------------
# resizing sources to a preset's grid (include/rcb.h, N4 416; data/video.py:26-31)
# ---------------------------------------------------------------------------------------------
RESIZE_MAX_TAPS = 33                                         # RCB_RESIZE_MAX_TAPS


def resize_taps(n_in, n_out):
    """The tap tables of one axis of rcb_resize, from the C planner (rcb_resize_taps; no device needed): -> (first int32 [n_out],
    count int32 [n_out], w float64 [n_out, 33], row i holding its count[i] normalised triangle weights and then +0.0).  A
    refused pair (a size below 1, a reduction steeper than 16 : 1) is an RcbError."""
    import ctypes
    from . import _lib
    lib = _lib.load()
    rows = max(int(n_out), 1)
    first, count = np.zeros(rows, dtype=np.int32), np.zeros(rows, dtype=np.int32)
    w = np.zeros((rows, RESIZE_MAX_TAPS), dtype=np.float64)
    rc = lib.rcb_resize_taps(int(n_in), int(n_out), ctypes.c_void_p(first.ctypes.data), ctypes.c_void_p(count.ctypes.data),
                             ctypes.c_void_p(w.ctypes.data), RESIZE_MAX_TAPS)
    if rc < 0:
        _lib.check(rc, "rcb_resize_taps")
    return first, count, w


def center_crop(tensor, size, axes):
    """A VIEW of `tensor` cropped about its centre to size[k] positions along axes[k]: the window starts at
    int(round((n - size) / 2.0)) with Python's round (half to even) -- torchvision's CenterCrop rule.  Nothing is copied.
    ValueError when an axis is shorter than the crop."""
    size, axes = [int(v) for v in size], [int(a) for a in axes]
    if len(size) != len(axes):
        raise ValueError("center_crop: %d sizes for %d axes" % (len(size), len(axes)))
    for s, a in zip(size, axes):
        n = int(tensor.shape[a])
        if s < 1 or s > n:
            raise ValueError("center_crop: axis %d has %d positions, the crop asks for %d" % (a, n, s))
        tensor = tensor.narrow(a, int(round((n - s) / 2.0)), s)
    return tensor


def resize_to_preset(config, signals, crop=None, channels_first=False, sample_format=None):
    """Image or video sources of any size -> the preset's grid, on the GPU: the resized signals [n, *grid, C] of the source's
    dtype, which are both what compress_signals / patch_signals cut and the SOURCE report_signals / report_ssim /
    report_ssim_frames score against.  signals: [n, *spatial, C] (or [n, C, *spatial] with channels_first) for a preset of
    data_dim 2 or 3, uint8, fp32 or a 16-bit dtype with sample_format=SampleFormat.u16(depth).  In order, all but the last step
    views: the channel axis is moved last; 3-D: the first grid[0] frames are kept (a shorter clip is a ValueError); 2-D: the two
    spatial axes are exchanged when the first is longer (signal_view's landscape rule); `crop` = (h, w): the centre crop of the
    last two spatial axes (center_crop); ops.resize of those two axes to the grid's (one rounding; include/rcb.h).  With
    crop=(240, 240) on the video preset this is data/video.py:27-31 -- the reference rounds twice there, see DESIGN 7."""
    from . import ops
    dd = config["data_dim"]
    if dd not in (2, 3):
        raise ValueError("resize_to_preset: presets of data_dim 2 and 3 have a size to resize to, not %d" % dd)
    if signals.dim() != dd + 2:
        raise ValueError("resize_to_preset: %d axes for a %d-D preset ([n, *spatial, C] expected)" % (signals.dim(), dd))
    if channels_first:
        signals = signals.movedim(1, -1)
    if signals.shape[-1] != config["output_dim"]:
        raise ValueError("resize_to_preset: %d channels, the preset has %d" % (signals.shape[-1], config["output_dim"]))
    pn, ps = preset_grid(config)
    grid = [pn[i] * ps[i] for i in range(dd)]
    if dd == 3:
        if signals.shape[1] < grid[0]:
            raise ValueError("resize_to_preset: a clip of %d frames, the preset takes the first %d" % (signals.shape[1], grid[0]))
        signals = signals.narrow(1, 0, grid[0])
    elif signals.shape[1] > signals.shape[2]:
        signals = signals.transpose(1, 2)
    if crop is not None:
        if len(crop) != 2:
            raise ValueError("resize_to_preset: crop is (h, w) of the last two spatial axes")
        signals = center_crop(signals, crop, (-3, -2))
    return ops.resize(signals, grid[-2:], sample_format=sample_format)


# ---------------------------------------------------------------------------------------------
# resampling audio to a preset's rate (include/rcb.h, N4 419; data/audio.py:39-46)
# ---------------------------------------------------------------------------------------------
RESAMPLE_MAX_TAPS = 97                                       # RCB_RESAMPLE_MAX_TAPS


def resample_taps(rate_in, rate_out):
    """The polyphase tap table of rcb_resample, from the C planner (rcb_resample_taps; no device needed): -> (o, n, first int32
    [n], count int32 [n], w float64 [n, 97]): rate_in : rate_out = o : n in lowest terms; output q n + p reads the samples from
    q o + first[p] on (first may be negative: zero padding) with row p's count[p] Hann-windowed sinc weights, then +0.0.  A refused
    pair (a rate below 1, a reduction steeper than 8 : 1, n > 1024 or o > 8192) is an RcbError."""
    import ctypes
    from . import _lib
    lib = _lib.load()
    o, n = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib.rcb_resample_taps(int(rate_in), int(rate_out), ctypes.byref(o), ctypes.byref(n), None, None, None, 0)
    if rc < 0:
        _lib.check(rc, "rcb_resample_taps")
    first, count = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
    w = np.zeros((n.value, RESAMPLE_MAX_TAPS), dtype=np.float64)
    rc = lib.rcb_resample_taps(int(rate_in), int(rate_out), ctypes.byref(o), ctypes.byref(n), ctypes.c_void_p(first.ctypes.data),
                               ctypes.c_void_p(count.ctypes.data), ctypes.c_void_p(w.ctypes.data), RESAMPLE_MAX_TAPS)
    if rc < 0:
        _lib.check(rc, "rcb_resample_taps")
    return o.value, n.value, first, count, w


def resample_length(L, rate_in, rate_out):
    """How many samples rcb_resample makes of L: ceil(L * rate_out / rate_in) in integer arithmetic (rcb_resample_length; no device
    needed).  A refused length or pair of rates is an RcbError."""
    from . import _lib
    lib = _lib.load()
    got = int(lib.rcb_resample_length(int(L), int(rate_in), int(rate_out)))
    if got < 0:
        raise _lib.RcbError("rcb_resample_length: " + (lib.rcb_last_error_string() or b"").decode())
    return got


def resample_to_preset(config, signals, rate_in, rate_out=16000, channels_first=False, mix="mean", sample_format=None):
    """Audio of any rate and channel count -> the preset's grid, on the GPU: the resampled signals [n, grid, C] of the source's
    dtype, which are both what compress_signals / patch_signals cut and the SOURCE report_signals scores against.  signals: [n, L,
    C] (or [n, C, L] with channels_first) for a preset of data_dim 1, int16 with sample_format=SampleFormat.s16() or fp32 (zero-
    centred: the padding at both ends is zeros).  In order: the channel axis is moved last (a view); the channels are mixed down
    to the preset's output_dim -- mix "mean": weights 1 / C; a sequence of C weights; None: the counts must agree already, and
    every channel is filtered on its own -- and resampled from rate_in to rate_out (16 000: the audio preset's, data/audio.py:39-46)
    in ONE ops.resample call, which computes exactly the grid's pixel_sizes x patch_nums outputs (48 000: 3 s) from the whole
    clip.  A clip that yields fewer is a ValueError: ops.resample + drivers.compress_signals_any code a signal of any length."""
    from . import ops
    dd = config["data_dim"]
    if dd != 1:
        raise ValueError("resample_to_preset: presets of data_dim 1 have a rate to resample to, not %d (resize_to_preset)" % dd)
    if signals.dim() != 3:
        raise ValueError("resample_to_preset: %d axes for a 1-D preset ([n, L, C] expected)" % signals.dim())
    if channels_first:
        signals = signals.movedim(1, -1)
    Cc, want = int(signals.shape[-1]), int(config["output_dim"])
    if isinstance(mix, str):
        if mix != "mean":
            raise ValueError("resample_to_preset: mix %r (\"mean\", C weights or None)" % (mix,))
        weights = None if Cc == want == 1 else [1.0 / Cc] * Cc
    else:
        weights = mix
    if weights is None and Cc != want:
        raise ValueError("resample_to_preset: %d channels, the preset has %d: mix=\"mean\" or C weights" % (Cc, want))
    if weights is not None:
        if want != 1:
            raise ValueError("resample_to_preset: a mix leaves 1 channel, the preset has %d" % want)
        if len(weights) != Cc:
            raise ValueError("resample_to_preset: %d mix weights for %d channels" % (len(weights), Cc))
    pn, ps = preset_grid(config)
    grid = pn[0] * ps[0]
    have = resample_length(int(signals.shape[1]), rate_in, rate_out)
    if have < grid:
        raise ValueError("resample_to_preset: %d samples at %d Hz are %d at %d Hz, the preset's grid has %d; ops.resample + "
                         "drivers.compress_signals_any code a signal of any length"
                         % (signals.shape[1], rate_in, have, rate_out, grid))
    return ops.resample(signals, rate_in, rate_out, sample_format=sample_format, mix=weights, length=grid)


# ---------------------------------------------------------------------------------------------
# Y'CbCr sources and per-plane scores (include/rcb.h, N4 418)
# ---------------------------------------------------------------------------------------------
YCC_STANDARDS = {"bt601": ("0.299", "0.114"), "bt709": ("0.2126", "0.0722"), "bt2020": ("0.2627", "0.0593")}   # (kr, kb)
YUV_LAYOUTS = {"i420": 2, "yv12": 2, "nv12": 2, "yuv422p": 1, "yuv444p": 0}                                     # -> subsampling


class YccMatrix:
    """What rcb_rgb_to_ycc (m [3, 3], off [3]) and rcb_ycc_to_rgb (n [3, 3], o [3]) take, numpy fp64, with what they were formed
    for: kr, kb (fractions.Fraction), full_range, sample_format."""

    def __init__(self, m, off, n, o, kr, kb, full_range, sample_format):
        self.m, self.off, self.n, self.o = m, off, n, o
        self.kr, self.kb, self.full_range, self.sample_format = kr, kb, full_range, sample_format

    def __repr__(self):
        return "YccMatrix(kr=%s, kb=%s, %s range, %r)" % (self.kr, self.kb, "full" if self.full_range else "limited", self.sample_format)


def _ycc_peak(sample_format, who):
    fmt = sample_format if sample_format is not None else SampleFormat.u8()
    if fmt.kind not in (SampleFormat.U8, SampleFormat.U16):
        raise ValueError("%s: Y'CbCr is defined here for u8 and u16 samples, not %r" % (who, fmt))
    d = 8 if fmt.kind == SampleFormat.U8 else fmt.depth
    return fmt, d, (1 << d) - 1


def ycc_matrix(standard, full_range=True, sample_format=None):
    """THE colour constants of the Y'CbCr entries, formed here and nowhere else (the device evaluates none) -> YccMatrix.
    standard: "bt601", "bt709", "bt2020" (kr, kb the decimal fractions of the recommendations), or a (kr, kb) pair of numbers
    (a float stands for its exact value), Fractions or decimal strings.  kg = (1 - kr) - kb.  With d the bit depth, L = 2^d - 1:
      full range     sy = sc = 1,                                     off = o = {0, 2^(d-1), 2^(d-1)}
      limited range  sy = 219 * 2^(d-8) / L,  sc = 224 * 2^(d-8) / L,  off = o = {16, 128, 128} * 2^(d-8)
      m = [[kr, kg, kb] * sy,
           [-kr / (2 (1 - kb)), -kg / (2 (1 - kb)), 1 / 2] * sc,
           [1 / 2, -kg / (2 (1 - kr)), -kb / (2 (1 - kr))] * sc]
      n = [[1 / sy, 0, 2 (1 - kr) / sc],                              (the closed forms R = y + 2 (1 - kr) cr, B = y + 2 (1 - kb) cb,
           [1 / sy, -2 kb (1 - kb) / (kg sc), -2 kr (1 - kr) / (kg sc)],   G = (y - kr R - kb B) / kg; no numeric matrix inverse)
           [1 / sy, 2 (1 - kb) / sc, 0]]
    Every coefficient is evaluated in exact rational arithmetic (fractions.Fraction) and rounded to fp64 ONCE, so it is the
    correctly rounded value of its formula whatever the order of the operations (tests/test_ycc_emul_cpu.py restates them)."""
    from fractions import Fraction as F
    fmt, d, L = _ycc_peak(sample_format, "ycc_matrix")
    if isinstance(standard, str):
        if standard not in YCC_STANDARDS:
            raise ValueError("ycc_matrix: standard %r (one of %s, or a (kr, kb) pair)" % (standard, ", ".join(sorted(YCC_STANDARDS))))
        kr, kb = (F(v) for v in YCC_STANDARDS[standard])
    else:
        kr, kb = (F(v) for v in standard)
    kg = (1 - kr) - kb
    if not (0 < kr < 1 and 0 < kb < 1 and 0 < kg < 1):
        raise ValueError("ycc_matrix: kr = %s, kb = %s leave kg = %s (all three lie strictly between 0 and 1)" % (kr, kb, kg))
    if full_range:
        sy = sc = F(1)
        off = [F(0), F(1 << (d - 1)), F(1 << (d - 1))]
    else:
        sy, sc = F(219 << (d - 8), L), F(224 << (d - 8), L)
        off = [F(16 << (d - 8)), F(128 << (d - 8)), F(128 << (d - 8))]
    half = F(1, 2)
    m = [[kr * sy, kg * sy, kb * sy],
         [-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, half * sc],
         [half * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc]]
    n = [[1 / sy, F(0), 2 * (1 - kr) / sc],
         [1 / sy, -2 * kb * (1 - kb) / (kg * sc), -2 * kr * (1 - kr) / (kg * sc)],
         [1 / sy, 2 * (1 - kb) / sc, F(0)]]
    as64 = lambda rows: np.asarray([[float(v) for v in r] for r in rows], dtype=np.float64)
    offs = np.asarray([float(v) for v in off], dtype=np.float64)
    return YccMatrix(as64(m), offs, as64(n), offs.copy(), kr, kb, bool(full_range), fmt)


def ycc_chroma_size(H, W, subsampling):
    """(Hc, Wc) of the chroma planes of an H x W frame: 0 = 4:4:4, 1 = 4:2:2 (Wc = (W + 1) // 2), 2 = 4:2:0 (Hc = (H + 1) // 2 too)"""
    if subsampling not in (0, 1, 2):
        raise ValueError("subsampling %r (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0)" % (subsampling,))
    return ((H + 1) // 2 if subsampling == 2 else H), ((W + 1) // 2 if subsampling else W)


def yuv_planes(buffer, n, T, H, W, layout, sample_format=None):
    """The three planes of n clips of T raw frames in ONE flat tensor, as strided VIEWS (nothing is copied) -> ((y [n, T, H, W],
    cb, cr [n, T, Hc, Wc]), subsampling): what ops.ycc_to_rgb takes.  A frame holds H W luma samples and then its chroma:
      "i420"     4:2:0, the Cb plane and then the Cr plane          "yv12"  4:2:0, Cr and then Cb
      "nv12"     4:2:0, one plane of interleaved Cb Cr pairs (column stride 2; P010-style with SampleFormat.u16)
      "yuv422p"  4:2:2 planar, Cb and then Cr                        "yuv444p"  4:4:4 planar, Cb and then Cr
    Frames follow each other without padding, H W + 2 Hc Wc samples each; odd sizes are legal (Hc, Wc round up).  buffer: a 1-D
    tensor of uint8 samples, or of a 16-bit dtype with sample_format=SampleFormat.u16(depth)."""
    if layout not in YUV_LAYOUTS:
        raise ValueError("yuv_planes: layout %r (one of %s)" % (layout, ", ".join(sorted(YUV_LAYOUTS))))
    fmt, _, _ = _ycc_peak(sample_format, "yuv_planes")
    if buffer.dim() != 1 or not fmt.accepts(buffer.dtype):
        raise ValueError("yuv_planes: a 1-D tensor of %r samples is needed, got %s %r" % (fmt, buffer.dtype, tuple(buffer.shape)))
    n, T, H, W = int(n), int(T), int(H), int(W)
    if min(n, T, H, W) < 1:
        raise ValueError("yuv_planes: %d clips of %d frames of %d x %d" % (n, T, H, W))
    ss = YUV_LAYOUTS[layout]
    Hc, Wc = ycc_chroma_size(H, W, ss)
    frame = H * W + 2 * Hc * Wc
    if buffer.numel() < n * T * frame:
        raise ValueError("yuv_planes: %d samples, %d clips of %d %s frames of %d x %d need %d"
                         % (buffer.numel(), n, T, layout, H, W, n * T * frame))
    base = buffer.storage_offset()
    y = buffer.as_strided((n, T, H, W), (T * frame, frame, W, 1), base)
    if layout == "nv12":
        first, second, row, col = H * W, H * W + 1, 2 * Wc, 2
    else:
        first, second, row, col = H * W, H * W + Hc * Wc, Wc, 1
    if layout == "yv12":
        first, second = second, first
    cb = buffer.as_strided((n, T, Hc, Wc), (T * frame, frame, row, col), base + first)
    cr = buffer.as_strided((n, T, Hc, Wc), (T * frame, frame, row, col), base + second)
    return (y, cb, cr), ss


def ycc_to_rgb_device(planes, matrix, subsampling, chroma="replicate", sample_format=None):
    """Planes (y, cb, cr) on the GPU (ops.ycc_to_rgb's; e.g. yuv_planes's views) -> RGB [n, (T,) H, W, 3] of the source's dtype.
    chroma: "replicate" -- the entry's own rule, every chroma sample repeated over its block -- or "bilinear": ops.resize of the
    two chroma planes to H x W (fp64 triangle filter, half-pixel centres: chroma sited at the CENTRE of its block; rounded to the
    sample lattice once) followed by the entry at 4:4:4.  Other sitings are not offered."""
    from . import ops
    y, cb, cr = planes
    if chroma == "replicate" or subsampling == 0:
        if chroma not in ("replicate", "bilinear"):
            raise ValueError("ycc_to_rgb_device: chroma %r ('replicate' or 'bilinear')" % (chroma,))
        return ops.ycc_to_rgb(y, cb, cr, matrix, subsampling, sample_format=sample_format)
    if chroma != "bilinear":
        raise ValueError("ycc_to_rgb_device: chroma %r ('replicate' or 'bilinear')" % (chroma,))
    size = (int(y.shape[-2]), int(y.shape[-1]))
    cb, cr = (ops.resize(c.unsqueeze(-1), size, sample_format=sample_format).squeeze(-1) for c in (cb, cr))
    return ops.ycc_to_rgb(y, cb, cr, matrix, 0, sample_format=sample_format)


def psnr_ycc_from_sse(sse, H, W, subsampling, sample_format=None):
    """rcb_ycc_sse's sums [..., 3] (int64 tensor or array) of H x W frames -> fp64 [..., 4] = {PSNR-Y, PSNR-Cb, PSNR-Cr,
    (6 Y + Cb + Cr) / 8}, the combined figure of the HM / JVET reports.  Each PSNR is 10 log10(L^2 count / sse), count = H W for Y
    and Hc Wc for a chroma plane; the numerator is a Python integer and the division the true division of two integers (correctly
    rounded); sse = 0 gives inf."""
    import math
    _, _, L = _ycc_peak(sample_format, "psnr_ycc_from_sse")
    s = sse.detach().cpu().numpy() if isinstance(sse, torch.Tensor) else np.asarray(sse)
    if s.ndim < 1 or s.shape[-1] != 3:
        raise ValueError("psnr_ycc_from_sse: the sums of rcb_ycc_sse are [..., 3], got %r" % (s.shape,))
    Hc, Wc = ycc_chroma_size(int(H), int(W), int(subsampling))
    counts = (int(H) * int(W), Hc * Wc, Hc * Wc)
    out = np.empty(s.shape[:-1] + (4,), dtype=np.float64)
    flat_in, flat_out = s.reshape(-1, 3), out.reshape(-1, 4)
    for row, res in zip(flat_in, flat_out):
        for k in range(3):
            v = int(row[k])
            if v < 0:
                raise ValueError("psnr_ycc_from_sse: a negative sum (%d)" % v)
            res[k] = math.inf if v == 0 else 10.0 * math.log10((L * L * counts[k]) / v)
        res[3] = (6.0 * res[0] + res[1] + res[2]) / 8.0
    return out


def ycc_device(a, b, matrix, subsampling=2, sample_format=None):
    """Per-plane PSNR of integer RGB images a against b in Y'CbCr, fp64 [n, 4] = {Y, Cb, Cr, (6 Y + Cb + Cr) / 8}: a, b [n, H, W, 3]
    GPU tensors of one integer dtype with ANY strides (ops.ycc_sse); only the sums are read back.  The twin of ssim_device."""
    from . import ops
    if a.dim() != 4:
        raise ValueError("ycc_device: images are [n, H, W, 3], got %d axes" % a.dim())
    if a.shape[0] == 0:
        return np.zeros((0, 4), dtype=np.float64)
    sse = ops.ycc_sse(a, b, matrix, subsampling, sample_format=sample_format)
    return psnr_ycc_from_sse(sse, a.shape[1], a.shape[2], subsampling, sample_format)


def ycc_frames_device(a, b, matrix, subsampling=2, sample_format=None):
    """`ycc_device` per FRAME of integer clips a, b [n, T, H, W, 3] (any strides), fp64 [n, T, 4], in one call; the caller
    averages.  The twin of ssim_frames_device."""
    from . import ops
    if a.dim() != 5:
        raise ValueError("ycc_frames_device: clips are [n, T, H, W, 3], got %d axes" % a.dim())
    if a.shape[0] * a.shape[1] == 0:
        return np.zeros((int(a.shape[0]), int(a.shape[1]), 4), dtype=np.float64)
    sse = ops.ycc_sse(a, b, matrix, subsampling, sample_format=sample_format)
    return psnr_ycc_from_sse(sse, a.shape[2], a.shape[3], subsampling, sample_format)
