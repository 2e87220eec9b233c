"""Host drivers mirroring the reference's two entry points on top of the MI355X models:

  * `train_prior(...)`      <- main_prior_training.py:25-341  (EM loop: train q -> adjust beta -> refit prior ->
                               every 10 iterations group parameters and write the checkpoint)
  * `compress(...)`         <- main_compression.py:25-178     (load checkpoint -> reorder priors into group order
                               -> TestBNNmodel -> optimise -> A* encode -> distortion + index arrays)

Data loading (data/*.py) is out of scope: both take tensors X [N,P,F] / [P,F] and Y [N,P,C].  The checkpoint is
the reference's own layout -- eight sequential pickles in one file, in the same order with the same tuple
contents (main_prior_training.py:284-335) -- so priors interchange with the reference in both directions
(`dropin/prior_model.py` provides the `prior_model.LinearTransform` / `prior_model.Upsample` class paths).
Under torch.distributed the INRs of `train_prior` are the local shard; the prior refit, the KL that drives
beta and the grouping statistics are all-reduced (recombiner_amd.dist).
"""
import contextlib
import io
import copy
import gzip
import pickle
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

from . import dist, ops, tuning
from .prior_model import LinearTransform, PriorBNNmodel, Upsample, get_grouping_by_kl
from .test_model import TestBNNmodel

LN2 = np.log(2.)


def bit_budgets(config, dataset, max_bitrate):
    """(budget_max, budget_min) in bits per INR (main_prior_training.py:75-83)."""
    px = np.prod(config['pixel_sizes'])
    lo = max(config['lowest_bitrate'], (max_bitrate - config['bitrate_range']))
    if dataset != 'audio':
        return max_bitrate * px, lo * px
    k = px * (3 / 48000) * 1000          # kbps * samples per patch * seconds per sample
    return max_bitrate * k, lo * k


def adjust_beta(kl_beta, kl_bits, budget_max, budget_min):
    """main_prior_training.py:144-154."""
    if kl_bits > budget_max:
        kl_beta *= 1.5
    if kl_bits < budget_min:
        kl_beta /= 1.5
    return min(max(kl_beta, 1e-20), 1)


def _grouping(q_loc, q_log_scale, p_loc, p_scale, group=None):
    """get_grouping over all ranks' INRs: per-parameter KL summed on the device, all-reduced, packed on the host."""
    colsum = ops.gauss_kl_colsum_fx(q_loc, q_log_scale, p_loc, p_scale, q_is_log=True)
    return get_grouping_by_kl(dist.grouping_weights(colsum, q_loc.shape[0], group))


def train_prior(config, dataset, X, Y, max_bitrate, device="cuda", seed=42, n_em_iter=550, first_epochs=200,
                epochs=100, lr=2e-4, kl_beta=1e-8, training_mappings=True, checkpoint_path=None, checkpoint_every=10,
                precision=0, group=None, log=print, noise_source=None):
    """Coordinate-ascent prior learning (main_prior_training.py:112-172).  Returns a dict with the model, mappings, priors,
    beta, the ELBO curve and the trajectory of the loop: per iteration (KL bits per INR before the beta rule, beta after it,
    MSE per INR).  noise_source: PriorBNNmodel.noise_source (a given epsilon stream instead of the device generator)."""
    tuning.enable_tuned_gemms()
    train_size = Y.shape[0]
    patch = config['patch']
    m = PriorBNNmodel(config['input_dim'], config['hidden_dims'], config['output_dim'], train_size, config['data_dim'],
                      config['pixel_sizes'], config['upsample_factors'], config['latent_dim'], patch,
                      config['patch_nums'], config['hierarchical_patch_nums'], random_seed=seed, device=device)
    m.precision = precision
    m.noise_source = noise_source
    lt = LinearTransform(m.dims).to(device)
    up = Upsample(config['data_dim'], config['paddings'], config['layerwise_scale_factors']).to(device)
    if dist.is_dist():
        # sharded: this model's mapping gradients are summed over `group` (None = every rank), nothing else is; the
        # shared mappings start from rank 0's values rather than from an assumption about identical seeds
        m.dp_group = group if group is not None else torch.distributed.group.WORLD
        if training_mappings:
            for prm in list(lt.parameters()) + list(up.parameters()):
                torch.distributed.broadcast(prm.data, torch.distributed.get_global_rank(m.dp_group, 0), group=m.dp_group)
    budget_max, budget_min = bit_budgets(config, dataset, max_bitrate)
    assert budget_min <= budget_max
    s0 = F.softplus(torch.tensor(-2.), beta=1, threshold=20) / 6

    def init_prior(shape):
        return torch.zeros(shape, device=device), torch.ones(shape, device=device) * s0.to(device)
    p_loc, p_scale = init_prior(m.loc.shape[1])
    p_lpe_loc, p_lpe_scale = init_prior(m.lpe_loc.shape[1:])
    p_h_loc = p_h_scale = p_hh_loc = p_hh_scale = None
    if patch:
        p_h_loc, p_h_scale = init_prior(m.h_loc.shape[-1])
        p_hh_loc, p_hh_scale = init_prior(m.hh_loc.shape[-1])
    X, Y = X.to(device), Y.to(device)
    rank, ws = dist.world(group)
    elbos, n_epoch, traj = [], first_epochs, []
    for it in range(n_em_iter):
        mse, _, e = m.train(n_epoch, lr, X, Y, p_loc, p_scale, p_lpe_loc, p_lpe_scale, p_h_loc, p_h_scale, p_hh_loc,
                            p_hh_scale, lt, up, kl_beta, training_mappings=training_mappings)
        elbos += e
        n_epoch = epochs
        # average KL in bits per INR over all ranks -> beta rule
        pack = torch.stack([m._kl_value([p_loc, p_scale, p_lpe_loc, p_lpe_scale, p_h_loc, p_h_scale, p_hh_loc, p_hh_scale]),
                            torch.tensor(float(train_size), dtype=torch.float64, device=m.loc.device)])
        pack = dist.allreduce_scalar(pack, group)
        kls = float(pack[0] / LN2 / pack[1])
        kl_beta = adjust_beta(kl_beta, kls, budget_max, budget_min)
        traj.append((kls, kl_beta, mse))
        # closed-form prior refit (moment matching over every rank's INRs)
        p_loc, p_scale = dist.refit_prior(m.loc, m.log_scale, group)
        p_lpe_loc, p_lpe_scale = dist.refit_prior(m.lpe_loc, m.lpe_log_scale, group)
        if patch:
            p_h_loc, p_h_scale = dist.refit_prior(m.h_loc, m.h_log_scale, group)
            p_hh_loc, p_hh_scale = dist.refit_prior(m.hh_loc, m.hh_log_scale, group)
        if it % checkpoint_every == 0 or it == n_em_iter - 1:
            log("EM iter %d: KL %.4f bits/INR, beta %.3e" % (it, kls, kl_beta))
            if checkpoint_path is not None:
                ck = build_checkpoint(m, lt, up, p_loc, p_scale, p_lpe_loc, p_lpe_scale, p_h_loc, p_h_scale, p_hh_loc,
                                      p_hh_scale, kl_beta, group)
                if rank == 0:
                    save_checkpoint(checkpoint_path, ck)
    return dict(model=m, linear_transform=lt, upsample_net=up, kl_beta=kl_beta, elbo=elbos, trajectory=traj,
                priors=(p_loc, p_scale, p_lpe_loc, p_lpe_scale, p_h_loc, p_h_scale, p_hh_loc, p_hh_scale))


def build_checkpoint(m, lt, up, p_loc, p_scale, p_lpe_loc, p_lpe_scale, p_h_loc, p_h_scale, p_hh_loc, p_hh_scale,
                     kl_beta, group=None):
    """The eight objects of the reference checkpoint, in file order (main_prior_training.py:186-335)."""
    def mean_rows(t):
        s = t.detach().sum(0, dtype=torch.float64).flatten()
        pack = torch.cat([s, torch.tensor([float(t.shape[0])], dtype=torch.float64, device=t.device)])
        pack = dist.allreduce_scalar(pack, group)
        return (pack[:-1] / pack[-1]).float().cpu()
    n = m.loc.shape[0]
    q_loc = torch.cat([m.loc.detach().flatten(1), m.lpe_loc.detach().flatten(1)], -1).contiguous()
    q_ls = torch.cat([m.log_scale.detach().flatten(1), m.lpe_log_scale.detach().flatten(1)], -1).contiguous()
    pl = torch.cat([p_loc.flatten(), p_lpe_loc.flatten()])
    ps = torch.cat([p_scale.flatten(), p_lpe_scale.flatten()])
    g1 = _grouping(q_loc, q_ls, pl, ps, group)
    avg_ls = torch.cat([mean_rows(m.log_scale), mean_rows(m.lpe_log_scale)])
    none8 = (None,) * 8
    if m.patch:
        g2 = _grouping(m.h_loc.detach(), m.h_log_scale.detach(), p_h_loc, p_h_scale, group)
        g3 = _grouping(m.hh_loc.detach(), m.hh_log_scale.detach(), p_hh_loc, p_hh_scale, group)
        l2 = (p_h_loc.cpu(), p_h_scale.cpu(), kl_beta, mean_rows(m.h_log_scale))
        l3 = (p_hh_loc.cpu(), p_hh_scale.cpu(), kl_beta, mean_rows(m.hh_log_scale))
    else:
        g2 = g3 = none8
        l2 = l3 = (None, None, kl_beta, None)
    return [g1, (pl.cpu(), ps.cpu(), kl_beta, avg_ls), g2, l2, g3, l3, lt, up]


_REF_CLASSES = {"LinearTransform": LinearTransform, "Upsample": Upsample}


@contextlib.contextmanager
def _reference_class_paths():
    """While active, LinearTransform / Upsample pickle as `prior_model.LinearTransform` / `prior_model.Upsample` -- the
    paths the reference's own pickles carry (main_prior_training.py:334-335) and main_compression.py:44-45 resolves --
    whatever is on sys.path.  (pickle checks that the named module really holds the class: a stand-in module is
    registered for the duration and whatever was there is put back.)"""
    stand_in = types.ModuleType("prior_model")
    saved_mod = sys.modules.get("prior_model")
    saved_paths = {n: c.__module__ for n, c in _REF_CLASSES.items()}
    for n, c in _REF_CLASSES.items():
        setattr(stand_in, n, c)
        c.__module__ = "prior_model"
    sys.modules["prior_model"] = stand_in
    try:
        yield
    finally:
        for n, c in _REF_CLASSES.items():
            c.__module__ = saved_paths[n]
        if saved_mod is None:
            sys.modules.pop("prior_model", None)
        else:
            sys.modules["prior_model"] = saved_mod


class _CheckpointUnpickler(pickle.Unpickler):
    """`prior_model.LinearTransform` / `prior_model.Upsample` resolve to the MI355X classes (same attribute, sub-module and
    parameter names as the reference's, prior_model.py:16-59), so a checkpoint written by the reference loads without the
    reference -- or `dropin/` -- on sys.path."""

    def find_class(self, module, name):
        if module in ("prior_model", "recombiner_amd.prior_model") and name in _REF_CLASSES:
            return _REF_CLASSES[name]
        return super().find_class(module, name)


def save_checkpoint(path, ck):
    """Writes the eight pickles (main_prior_training.py:284-335), loadable by the reference's main_compression.py.
    The two modules are pickled as CPU *copies*: moving the live modules to the CPU and back (what the reference does,
    :334-338) re-allocates their parameter storages, i.e. the addresses the captured training graphs read and update
    (PriorBNNmodel.train re-captures if that ever happens, see its workspace key)."""
    lt, up = ck[6], ck[7]
    with open(path, "wb") as f, _reference_class_paths():
        for obj in ck[:6]:
            pickle.dump(obj, f)
        pickle.dump(copy.deepcopy(lt).cpu(), f)
        pickle.dump(copy.deepcopy(up).cpu(), f)


def load_checkpoint(path):
    """-> list of the eight objects (main_compression.py:37-45); `path` may be gzip-compressed (test fixtures)."""
    out = []
    with open(path, "rb") as f:
        magic = f.read(2)
    opener = gzip.open if magic == b"\x1f\x8b" else open
    with opener(path, "rb") as f:
        for _ in range(8):          # eight independent pickle streams: a fresh unpickler (memo) for each
            out.append(_CheckpointUnpickler(f).load())
    return out


def build_test_model(config, dataset, checkpoint, n_datapoints, device="cuda", seed=42):
    """TestBNNmodel initialised from a prior checkpoint exactly as main_compression.py:47-133 does (priors and average
    log-scales reordered into group order).  Shared by the encoder (`compress`) and the decoder (`bitstream.decode`)."""
    g1, l1, g2, l2, g3, l3, lt, up = checkpoint
    group_idx, start, end, group2param, param2group, n_groups, _, _ = g1
    prior_loc, prior_scale, kl_beta, avg_ls = l1

    def inv_st(s):
        return torch.log(torch.exp(s * 6) - 1)
    kw = dict(p_loc=prior_loc.clone()[param2group].to(device), p_log_scale=inv_st(prior_scale).clone()[param2group].to(device),
              init_log_scale=avg_ls[param2group].cpu().detach(), param_to_group=param2group, group_to_param=group2param,
              n_groups=n_groups, group_start_index=start, group_end_index=end, group_idx=group_idx)
    if config['patch']:
        for pre, g, l in (("h_", g2, l2), ("hh_", g3, l3)):
            gi, gs, ge, g2p, p2g, ng, _, _ = g
            ploc, pscale, _, als = l
            kw.update({pre + "p_loc": ploc.clone()[p2g].to(device), pre + "p_log_scale": inv_st(pscale).clone()[p2g].to(device),
                       pre + "init_log_scale": als[p2g].cpu().detach(), pre + "param_to_group": p2g,
                       pre + "group_to_param": g2p, pre + "n_groups": ng, pre + "group_start_index": gs,
                       pre + "group_end_index": ge, pre + "group_idx": gi})
    return TestBNNmodel(config['input_dim'], config['hidden_dims'], config['output_dim'], n_datapoints,
                        config['upsample_factors'], config['latent_dim'], config['data_dim'], config['pixel_sizes'],
                        config['patch'], config['patch_nums'], config['hierarchical_patch_nums'], dataset,
                        linear_transform=lt.to(device), upsample_net=up.to(device), w0=30., c=6., random_seed=seed,
                        device=device, kl_upper_buffer=0., kl_lower_buffer=0.4, kl_adjust_gap=10, initial_beta=kl_beta,
                        beta_step_size=0.05, **kw)


def compress(config, dataset, checkpoint, x, y, device="cuda", seed=42, n_epochs=30000, lr=2e-4, precision=0,
             verbose=0, finetune_epochs=None, bitstream_path=None, sample_format=None):
    """main_compression.py:47-178 on an in-memory checkpoint (list from load_checkpoint / build_checkpoint).
    Returns (distortion, model); with `bitstream_path` the packed A* indices are written there (bitstream.py).
    sample_format (utils.SampleFormat): only written into the stream (version 3 when it is not the preset's implied format); the
    distortion returned here is the reference's figure on the patch targets."""
    tuning.enable_tuned_gemms()
    g1, _, g2, _, g3, _, _, _ = checkpoint
    n_groups = g1[5]
    h_n = hh_n = None
    if config['patch']:
        h_n, hh_n = g2[5], g3[5]
    x, y = x.to(device), y.to(device)
    model = build_test_model(config, dataset, checkpoint, y.shape[0], device, seed)
    model.precision = precision
    model.optimize_posteriors(x, y, n_epochs=n_epochs, lr=lr, verbose=verbose)
    ft = finetune_epochs
    distortion = model.compress_posteriors(
        x, y, n_epochs_finetune=ft if ft is not None else max(30000 // n_groups, 50),
        h_n_epochs_finetune=None if h_n is None else (ft if ft is not None else max(15000 // h_n, 20)),
        hh_n_epochs_finetune=None if hh_n is None else (ft if ft is not None else max(15000 // hh_n, 20)),
        verbose=verbose, lr=lr, fine_tune_gap=1, compress_from_group_with_largest_kl=True)
    if bitstream_path is not None:
        from . import bitstream
        _write_stream(bitstream_path, bitstream.encode(model, sample_format=sample_format))
    return distortion, model


def _write_stream(path, blob):
    with open(path, "wb") as f:
        f.write(blob)


def _default_x(x, config, device, n_rows):
    """x, or the preset's own coordinate features shared by all rows"""
    from . import utils
    return utils.preset_inputs(config, device)[None].expand(n_rows, -1, -1) if x is None else x


def _signal_views(what, signals, sample_format, device, config=None, channels_first=False, listed=False):
    """What every whole-signal driver does to its signals before they are cut, `what` naming the driver in the refusals: the format
    check, the axis check, the move to the device, the channel axis moved last, the channel check -> the list of views.  `signals`
    is a list of batches [n, *size, C], or with `listed` of single signals [*size, C] of one dtype.  config None: format check and
    move only (compress_signals, whose axes utils.signal_view moves and checks)."""
    lead = 0 if listed else 1                                # axes in front of the spatial ones
    views = []
    for k, t in enumerate(signals):
        # a 16-bit tensor does not say how deep its samples are (nor, for int16, whether they are PCM or reinterpreted u16)
        if sample_format is None and t.dtype in (torch.uint16, torch.int16):
            raise ValueError("%s: %s signals need sample_format= (utils.SampleFormat.u16(depth) or .s16()): the depth is not in the "
                             "dtype" % (what, t.dtype))
        if sample_format is not None and not sample_format.accepts(t.dtype):
            raise ValueError("%s: sample_format %r reads %s signals, got %s" % (what, sample_format, sample_format.dtype, t.dtype))
        if config is None:
            views.append(t.to(device))
            continue
        dd, Cc = config["data_dim"], config["output_dim"]
        if t.dim() != dd + 1 + lead or t.dtype != signals[0].dtype:
            raise ValueError("%s: signal %d is %s with %d axes; [*size, C] of %s expected for a %d-D preset"
                             % (what, k, t.dtype, t.dim(), signals[0].dtype, dd) if listed else
                             "%s: %d axes for a %d-D preset ([n, *size, C] expected)" % (what, t.dim(), dd))
        v = t.to(device).movedim(lead, -1) if channels_first else t.to(device)
        if v.shape[-1] != Cc:
            raise ValueError("%s: signal %d has %d channels, the preset %d" % (what, k, v.shape[-1], Cc) if listed else
                             "%s: %d channels, the preset has %d" % (what, v.shape[-1], Cc))
        views.append(v)
    return views


def compress_signals(config, dataset, checkpoint, signals, x=None, channels_first=False, origin=None, landscape=True,
                     sample_format=None, **kw):
    """`compress` on whole signals in memory -- uint8 (q / 255, as ToTensor and `video / 255`) or fp32, [n, *spatial, C] or
    [n, C, *spatial] with channels_first -- instead of patch targets: the preset's window of each signal (utils.signal_view,
    which also documents origin / landscape) is cut into y [N, P, C] on the device (rcb_signal_patch), where the reference's
    loaders slice on the host (data/image.py:30-46, data/video.py:54-73, data/audio.py:125-140).  x None: the preset's own
    coordinate features (utils.preset_inputs) shared by all rows.  Every other argument, and the result, is `compress`'s.
    sample_format (utils.SampleFormat): how the samples are stored; required for uint16 / int16 signals (ValueError without it),
    and written into the stream as `compress` documents."""
    from . import utils
    device = kw.get("device", "cuda")
    (moved,) = _signal_views("compress_signals", [signals], sample_format, device)
    view = utils.signal_view(config, moved, channels_first=channels_first, origin=origin, landscape=landscape)
    y = ops.signal_patch(view, utils.signal_layout(config), sample_format=sample_format)
    return compress(config, dataset, checkpoint, _default_x(x, config, device, y.shape[0]), y, sample_format=sample_format, **kw)


def compress_resized(config, dataset, checkpoint, signals, crop=None, channels_first=False, sample_format=None, regions=None, **kw):
    """`compress_signals` on sources of any size, brought to the preset's grid on the device first (utils.resize_to_preset, which
    documents crop / channels_first and the order of the steps: first frames, landscape swap, centre crop, one antialiased
    resize with one rounding -- data/video.py:26-31 with crop=(240, 240) on the video preset).  -> what compress_signals returns,
    plus the resized source [n, *grid, C] of the signals' dtype: the signal that was coded, hence the one the decoded integers are
    scored against (report_signals, report_ssim, report_ssim_frames).  The stream is that of a signal at the preset's grid:
    bitstream.decode_signal decodes it.  Every other argument is `compress`'s.
    regions ("patch", "frame", "row" or a box of one int per axis: utils.region_of; None: nothing changes): one more element is
    appended, the distortion figure per region of every resized signal, fp64 [n, *nr] (the model's report_regions_signals)."""
    from . import utils
    device = kw.get("device", "cuda")
    (moved,) = _signal_views("compress_resized", [signals], sample_format, device)
    resized = utils.resize_to_preset(config, moved, crop=crop, channels_first=channels_first, sample_format=sample_format)
    out = compress_signals(config, dataset, checkpoint, resized, landscape=False, sample_format=sample_format, **kw)
    if regions is None:
        return (*out, resized)
    n_rows = resized.shape[0] * int(np.prod(utils.preset_grid(config)[0]))
    by_region = out[1].report_regions_signals(_default_x(kw.get("x"), config, device, n_rows), resized, region=regions,
                                              sample_format=sample_format)
    return (*out, resized, by_region)


def compress_resampled(config, dataset, checkpoint, signals, rate_in, rate_out=16000, channels_first=False, mix="mean",
                       sample_format=None, regions=None, **kw):
    """`compress_signals` on audio of any rate and channel count, brought to the preset's rate, channel count and grid on the device
    first (utils.resample_to_preset, which documents rate_in / rate_out / channels_first / mix and the order of the steps: the
    downmix, then one windowed-sinc resampling with one rounding, cut to the grid's length -- what a loader does before
    data/audio.py:39-54 when the files are not LibriSpeech's).  -> what compress_signals returns, plus the resampled source
    [n, grid, C] of the signals' dtype: the signal that was coded, hence the one the decoded integers are scored against
    (report_signals).  The stream is that of a signal at the preset's grid and carries no rate: bitstream.decode_signal decodes
    it.  Every other argument is `compress`'s.
    regions ("patch", "row" or a box of one int: utils.region_of; None: nothing changes): one more element is appended, the
    distortion figure per region of every resampled signal, fp64 [n, *nr] (the model's report_regions_signals)."""
    from . import utils
    device = kw.get("device", "cuda")
    (moved,) = _signal_views("compress_resampled", [signals], sample_format, device)
    resampled = utils.resample_to_preset(config, moved, rate_in, rate_out=rate_out, channels_first=channels_first, mix=mix,
                                         sample_format=sample_format)
    out = compress_signals(config, dataset, checkpoint, resampled, landscape=False, sample_format=sample_format, **kw)
    if regions is None:
        return (*out, resampled)
    n_rows = resampled.shape[0] * int(np.prod(utils.preset_grid(config)[0]))
    by_region = out[1].report_regions_signals(_default_x(kw.get("x"), config, device, n_rows), resampled, region=regions,
                                              sample_format=sample_format)
    return (*out, resampled, by_region)


def compress_ycc(config, dataset, checkpoint, planes, layout_or_subsampling, matrix, crop=None, chroma="replicate", sample_format=None,
                 **kw):
    """`compress_resized` on Y'CbCr sources -- raw video and image planes as decoders and .yuv files deliver them -- converted to
    RGB on the device first (utils.ycc_to_rgb_device; rcb_ycc_to_rgb), for the 2-D and 3-D presets of three channels.
    planes: (y, cb, cr) tensors [n, (T,) H, W] / [n, (T,) Hc, Wc] of any strides with layout_or_subsampling = 0 / 1 / 2 (4:4:4,
    4:2:2, 4:2:0), or ONE flat tensor of raw frames with a layout name of utils.yuv_planes ("i420", "yv12", "nv12", "yuv422p",
    "yuv444p") and size=(n, T, H, W) among the keywords (T = 1 for a 2-D preset).  matrix: utils.ycc_matrix(...); chroma:
    "replicate" or "bilinear" (utils.ycc_to_rgb_device); crop: compress_resized's.
    -> what compress_resized returns (the resized RGB source last), plus one more element: the per-plane PSNR of the decoded
    integers against that source in Y'CbCr at the source's subsampling -- the model's report_ycc, fp64 [n, 4] (2-D), or
    report_ycc_frames, fp64 [n, T, 4] (3-D).  Every other argument is `compress`'s."""
    from . import utils
    device = kw.get("device", "cuda")
    dd = config["data_dim"]
    if dd not in (2, 3):
        raise ValueError("compress_ycc: presets of data_dim 2 and 3 take Y'CbCr sources, not %d" % dd)
    size = kw.pop("size", None)
    if isinstance(layout_or_subsampling, str):
        if size is None or len(size) != 4:
            raise ValueError("compress_ycc: a flat buffer of %r frames needs size=(n, T, H, W)" % (layout_or_subsampling,))
        (flat,) = _signal_views("compress_ycc", [planes], sample_format, device)
        views, ss = utils.yuv_planes(flat, *size, layout_or_subsampling, sample_format=sample_format)
        if dd == 2:
            if int(size[1]) != 1:
                raise ValueError("compress_ycc: a 2-D preset takes images: T = 1 in size, got %d" % int(size[1]))
            views = tuple(v[:, 0] for v in views)
    else:
        if size is not None:
            raise ValueError("compress_ycc: size= goes with a layout name; three planes carry their own shape")
        views, ss = tuple(_signal_views("compress_ycc", list(planes), sample_format, device)), int(layout_or_subsampling)
    rgb = utils.ycc_to_rgb_device(views, matrix, ss, chroma=chroma, sample_format=sample_format)
    out = compress_resized(config, dataset, checkpoint, rgb, crop=crop, sample_format=sample_format, **kw)
    model, resized = out[1], out[-1] if kw.get("regions") is None else out[-2]
    n_rows = resized.shape[0] * int(np.prod(utils.preset_grid(config)[0]))
    report = model.report_ycc if dd == 2 else model.report_ycc_frames
    return (*out, report(_default_x(kw.get("x"), config, device, n_rows), resized, matrix, subsampling=ss, sample_format=sample_format))


def compress_signals_any(config, dataset, checkpoint, signals, x=None, channels_first=False, bitstream_path=None,
                         sample_format=None, regions=None, **kw):
    """`compress_signals` for signals of ANY size that the preset can be fitted to: `signals` is [n, *size, C] (or [n, C, *size]
    with channels_first), uint8 or fp32, one size per call (a list of signals of mixed sizes: compress_signal_list).
    The config is fitted (utils.fit_config: patched presets get the
    next whole patch grid that level 2 divides; unpatched presets keep theirs and take signals up to it), the signals'
    edge samples are replicated out to that grid while they are cut into y on the device (rcb_signal_patch_pad), and `compress`
    runs with the fitted config -- a checkpoint trained at the preset's patch_nums drives it, its priors being per parameter.
    -> (distortion, model, fitted_config).  `distortion` counts the REAL samples only (rcb_recon_finish_crop); the training
    loss does not: padded samples are fitted at full weight and cost rate, and a wholly padded patch still costs its groups.
    The bitstream (bitstream_path) is version 2 and carries `size`; bitstream.decode_signal_any decodes and crops it.
    Rate: bpp = bitstream.payload_bits(blob) / (n * prod(size)), bits per real sample position.
    There is no landscape swap and no origin here: the signals are coded in the orientation they are passed in.  Signals of mixed
    sizes and orientations -- a photo set with portraits in it, clips of different lengths -- go through compress_signal_list, which
    swaps a portrait signal through its strides, buckets the sizes by the grid they fit and writes version-4 streams.  Every other
    argument is `compress`'s.
    sample_format (utils.SampleFormat; required for uint16 / int16 signals, ValueError without it): how the samples are stored.
    `distortion` is then formed on the format's lattice -- the figure of the signal decode_signal_any delivers.  For s16 audio
    that is the distortion of the delivered PCM, NOT the reference's figure, which scores the unrounded reconstruction
    (utils.metric, round=False).  A format other than the preset's implied one makes the stream version 3, which carries it.
    regions ("patch", "frame", "row" or a box of one int per axis: utils.region_of; None: nothing changes): one more element is
    appended to the result, the distortion figure per region over the REAL samples, fp64 [n, *nr] (the model's report_regions
    with size=): the regions tile `size`, so the patches on the far edges show what the padding fitted at full weight costs."""
    from . import bitstream, utils
    device = kw.get("device", "cuda")
    (view,) = _signal_views("compress_signals_any", [signals], sample_format, device, config, channels_first)
    size = tuple(int(v) for v in view.shape[1:-1])
    fitted = utils.fit_config(config, size)
    y = ops.signal_patch_pad(view, utils.signal_layout(fitted), sample_format=sample_format)
    x = _default_x(x, fitted, device, y.shape[0])
    _, model = compress(fitted, dataset, checkpoint, x, y, **kw)
    distortion = model.report(x, y, size=size, sample_format=sample_format)
    if bitstream_path is not None:
        _write_stream(bitstream_path, bitstream.encode(model, extent=size, sample_format=sample_format))
    if regions is not None:
        return distortion, model, fitted, model.report_regions(x, y, region=regions, size=size, sample_format=sample_format)
    return distortion, model, fitted


def compress_signal_list(config, dataset, checkpoint, signals, channels_first=False, landscape=True, sample_format=None,
                         bitstream_dir=None, **kw):
    """`compress_signals_any` for a LIST of signals of mixed sizes and orientations: signals[k] is [*size_k, C] (or [C, *size_k]
    with channels_first), all of one dtype.  utils.ragged_plan decides per signal whether its two axes are exchanged (2-D presets
    with `landscape`: a portrait signal is coded landscape, read through transposed strides, nothing copied) and groups the
    signals into buckets by the patch grid their size fits (utils.fit_config).  Per bucket: all its signals are cut into y in ONE
    rcb_signal_patch_ragged call, each edge-padded to the grid from its own extent; `compress` runs once with the fitted config;
    the distortion counts each signal's real samples (report(sizes=), rcb_recon_finish_ragged); the stream is version 4 and
    carries every size and swap flag (bitstream.decode_signal_list gives the signals back, a portrait one portrait).
    -> (distortion, records, bpp): distortion is an array of per-signal figures in input order (cifar, protein) or the one figure
    pooled over the real samples of the whole list (kodak, video, audio); records holds one dict per bucket -- indices (input
    positions of its signals), sizes (along the model's axes), swaps, model, config (fitted) and stream (the version-4 bytes; also
    written to bitstream_dir/bucket_<i>.rcb when a directory is given); bpp = sum of payload bits / sum of prod(size_k).
    As with compress_signals_any the padded samples are trained on at full weight and cost rate; there is one model per grid, and the
    swap exists for 2-D presets only.  sample_format: compress_signals_any's.  Every other argument is `compress`'s."""
    import os
    from . import bitstream, utils
    signals = list(signals)
    if not signals:
        raise ValueError("compress_signal_list: an empty list of signals")
    if "bitstream_path" in kw:
        raise ValueError("compress_signal_list: one stream per bucket is written, to bitstream_dir")
    device = kw.get("device", "cuda")
    views = _signal_views("compress_signal_list", signals, sample_format, device, config, channels_first, listed=True)
    swaps, buckets = utils.ragged_plan(config, [tuple(v.shape[:-1]) for v in views], landscape=landscape)
    per_signal = dataset in ("cifar", "protein")
    figures = np.zeros(len(views), dtype=np.float64)
    pooled_err = pooled_n = 0.0
    records, bits, positions = [], 0, 0
    for b, bucket in enumerate(buckets):
        fitted, idx, sizes = bucket["config"], bucket["indices"], bucket["sizes"]
        cut = [views[k].transpose(0, 1) if swaps[k] else views[k] for k in idx]
        y = ops.signal_patch_ragged(cut, utils.signal_layout(fitted), sample_format=sample_format)
        x = _default_x(None, fitted, device, y.shape[0])
        _, model = compress(fitted, dataset, checkpoint, x, y, **kw)
        d = model.report(x, y, sizes=sizes, sample_format=sample_format)
        real = sum(int(np.prod(s)) for s in sizes)           # the bucket's real sample positions
        count = float(real * y.shape[-1])
        if per_signal:
            figures[idx] = d
        else:                                                # a PSNR over the bucket's real samples -> its share of the summed error
            pooled_err += 10.0 ** (-d / 10.0) * count
            pooled_n += count
        blob = bitstream.encode(model, extents=sizes, swaps=[swaps[k] for k in idx], sample_format=sample_format)
        if bitstream_dir is not None:
            os.makedirs(bitstream_dir, exist_ok=True)
            _write_stream(os.path.join(bitstream_dir, "bucket_%d.rcb" % b), blob)
        bits += bitstream.payload_bits(blob)
        positions += real
        records.append(dict(indices=list(idx), sizes=list(sizes), swaps=[swaps[k] for k in idx], model=model, config=fitted,
                            stream=blob))
    distortion = figures if per_signal else float(-10.0 * np.log10(pooled_err / pooled_n))
    return distortion, records, bits / positions


def rd_point(config, dataset, X, Y_train, Y_test, max_bitrate, device="cuda", seed=42, n_em_iter=550, first_epochs=200, epochs=100,
             lr=2e-4, n_opt=30000, finetune_epochs=None, precision=0, noise_source=None):
    """One rate-distortion point from scratch with the product alone: learn the prior (and the mappings) on Y_train
    (train_prior), build the checkpoint in memory, compress Y_test from it (compress) -> dict(bpp, psnr (per datapoint),
    n_groups, trajectory).  The composition main_prior_training.py -> main_compression.py performs through a file."""
    from . import bitstream
    nt, ne = Y_train.shape[0], Y_test.shape[0]
    Xd = X.to(device)
    out = train_prior(config, dataset, Xd[None].expand(nt, -1, -1), Y_train, float(max_bitrate), device=device, seed=seed,
                      n_em_iter=n_em_iter, first_epochs=first_epochs, epochs=epochs, lr=lr, precision=precision,
                      log=lambda *_: None, noise_source=noise_source)
    ck = build_checkpoint(out["model"], out["linear_transform"], out["upsample_net"], *out["priors"], out["kl_beta"])
    with contextlib.redirect_stdout(io.StringIO()):           # (the test-time model prints its expected bpp, like the reference's)
        dist_, model = compress(config, dataset, ck, Xd[None].expand(ne, -1, -1), Y_test.to(device), device=device, seed=seed,
                                n_epochs=n_opt, lr=lr, precision=precision, finetune_epochs=finetune_epochs)
    bits = bitstream.payload_bits(bitstream.encode(model))
    return dict(bpp=bits / (ne * int(np.prod(config["pixel_sizes"]))), psnr=np.asarray(dist_, dtype=np.float64),
                n_groups=int(ck[0][5]), trajectory=np.array(out["trajectory"]))
