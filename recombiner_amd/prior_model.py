"""Prior-learning model on MI355X: per-INR variational posteriors, batched SIREN forward/backward,
ELBO/KL, Adam -- the call surface of the reference's prior_model.py (same class / function names,
argument order and return values, cited per member) on top of hand-written HIP kernels.

Where the reference chains torch ops through autograd, `train()` here runs one fused pipeline per
step (train_step.py): sample (K1, in-kernel noise) -> upsampling net (hand-written phase-conv kernels in the 16-bit modes,
MIOpen only in the fp32 parity mode) -> A transform (atrans.hip) -> fused SIREN fwd+MSE+bwd (K3/K4) -> A-transform
backward -> upsampling-net backward -> fused reparam-bwd + KL-bwd + Adam (K1'/K5'/K11), replayed as one HIP graph.
`forward()` / `calculate_kl()` stay autograd-capable through custom Functions so user code written
against the reference API keeps working.  There is no CPU fallback.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from . import train_step
from .ops import LevelSpec, SirenMeta
from .upsample_fast import (hip_path_supported, tiled_2d_preferred, phase_form_preferred, phase_module,
                            stitched2d_module, upsample_cifar_hip)
from .utils import SampleFormat, count_net_params, hierarchy_row_maps, map_lpe_to_inr_inputs, metric_device, ssim_device, ssim_frames_device
from .utils import metric_regions_device, region_of, ycc_device, ycc_frames_device
from .utils import map_hierarchical_model_to_int_weights  # noqa: F401  (module-level name, as upstream imports it)


class LinearTransform(nn.Module):
    """Shared per-layer square maps A[l] (L_l x L_l), init U(-1,1)/L_l  (prior_model.py:16-21)."""

    def __init__(self, net_dims):
        super().__init__()
        mats = []
        for i in range(1, len(net_dims)):
            L = net_dims[i] * (net_dims[i - 1] + 1)
            mats.append((torch.rand(L, L) * 2 - 1) / L)
        self.A = nn.ParameterList(mats)


class Upsample(nn.Module):
    """Latent grid -> per-pixel encodings: 3 x (nearest upsample, conv), 128 -> 64 -> 64 -> 16 channels,
    kernels 5/3/3, LeakyReLU(0.01) after the first two convs  (prior_model.py:23-59).  Submodule names
    match the reference so state dicts / pickles interchange."""

    def __init__(self, kernel_dim, paddings, layerwise_scale_factors):
        super().__init__()
        conv = {1: nn.Conv1d, 2: nn.Conv2d, 3: nn.Conv3d}[kernel_dim]
        layerwise_scale_factors = [tuple(s) if isinstance(s, (list, tuple)) else s for s in layerwise_scale_factors]
        self.up1 = nn.Upsample(scale_factor=layerwise_scale_factors[0])
        self.conv1 = conv(128, 64, 5, padding=paddings[0])
        self.conv2 = conv(64, 64, 3, padding=paddings[1])
        self.conv3 = conv(64, 16, 3, padding=paddings[2])
        self.act1 = nn.LeakyReLU()
        self.up2 = nn.Upsample(scale_factor=layerwise_scale_factors[1])
        self.act2 = nn.LeakyReLU()
        self.up3 = nn.Upsample(scale_factor=layerwise_scale_factors[2])

    def forward(self, x):
        x = self.act1(self.conv1(self.up1(x)))
        x = self.act2(self.conv2(self.up2(x)))
        return self.conv3(self.up3(x))

    def __getstate__(self):
        # the fast evaluation paths cache their wrappers on the module (`_rcb_*`, upsample_fast.py); they share this module's
        # parameters and must neither travel in a checkpoint pickle (the reference could not load it) nor be carried over
        # by copy.deepcopy (the copy would keep evaluating the ORIGINAL's parameters)
        return {k: v for k, v in self.__dict__.items() if not k.startswith("_rcb_")}


class InrGeometry:
    # what PriorBNNmodel and TestBNNmodel share: the geometry of one INR (a mixin: the models set the members read here)

    def _pe_layout(self):
        # the patched presets in the 16-bit modes hand the SIREN kernel the upsampling net's output on the stitched grids
        # as it is (ops.PeLayout); None: pe is cut back into [N, S, P, 16]
        return self.recon_layout() if self.precision != 0 and self.stitched_pe else None

    def _pe(self, upsample_net, lpe, stitched=False, lpe16=None, weff_cache=None, weight_side_stream=None, fwd_fused=None):
        """lpe [S, N, *lat, C] -> pe [N, S, P, 16]: hand-written phase-conv kernels in the 16-bit modes
        where the geometry is instantiated, the nn.Module (MIOpen) otherwise.  `stitched`: see _pe_layout.
        lpe16: the producer's bf16 copy of lpe [N, Dlpe] (stage-1 operand; saves the cast pass).
        weff_cache: the phase-form weights in _UpsampleCifarFn's cache form: of THIS step (ops.step_prepare), or of frozen mappings.
        weight_side_stream: second stream for the weight-gradient side of the hand-written kernels' backward.
        fwd_fused: stages 2 + 3 of the hand-written forward as one launch (PriorTrainStep: its plan field; None: the
        environment's, which a model with a frozen weff_cache -- TestBNNmodel -- reads once and keeps, upsample_cifar_hip)."""
        if self.precision != 0 and hip_path_supported(upsample_net, self.pixel_sizes, self.upsample_factors, self.patch, self.data_dim):
            return upsample_cifar_hip(upsample_net, lpe, self.stage1_bf16, self.pe_bf16, frozen_cache=weff_cache, lpe16=lpe16,
                                      weight_side_stream=weight_side_stream, fwd_fused=fwd_fused)
        net = upsample_net
        if self.precision != 0 and tiled_2d_preferred(upsample_net, self.patch, self.data_dim):
            net = stitched2d_module(upsample_net)                  # stitched 2-D grid: phase-conv kernels on overlapping tiles
        elif self.precision != 0 and phase_form_preferred(self.data_dim, self.patch):
            net = phase_module(upsample_net) or upsample_net       # torch-level phase form: same function, fewer flops
        return map_lpe_to_inr_inputs(net, lpe, self.latent_dim, self.pixel_sizes, self.upsample_factors,
                                     self.patch, self.patch_nums, self.data_dim, stitched=stitched)

    def _meta(self, x, pe_dim, samples=1):
        return SirenMeta(samples=samples, n_pix=x.shape[-2], fourier_dim=x.shape[-1], pe_dim=pe_dim,
                         n_hidden=self.n_layers - 1, hidden=max(self.dims[1:-1]), out_dim=self.dims[-1], w0=self.w0,
                         precision=self.precision,
                         hidden_dims=tuple(self.dims[1:-1]) if len(set(self.dims[1:-1])) > 1 else None)

    def _layer_slices(self):
        cum = self.cum_param_sizes
        return [(0 if i == 0 else int(cum[i - 1]), int(cum[i])) for i in range(self.n_layers)]

    def group_to_layer(self, param, layer_idx):
        # reference API: the slice of a layer-vector row (.. x D_net) that belongs to layer `layer_idx`
        lo, hi = self._layer_slices()[layer_idx]
        return param[..., lo:hi]

    def recon_layout(self):
        """how the rows of a reconstruction [N, P, C] make up whole signals: ops.PeLayout of the patched presets, else None"""
        return self.signal_layout() if self.patch else None

    def signal_layout(self):
        """the grid of a whole signal, the unpatched presets as one patch per signal (what the signal entries take): the one place
        the models build their ops.PeLayout"""
        dd = self.data_dim
        return ops.PeLayout(self.patch_nums[:dd] if self.patch else [1] * dd, self.pixel_sizes[:dd])

    def report(self, x, y, on_device=True, size=None, sample_format=None, sizes=None):
        """TestBNNmodel (the model with `predict`, `dataset` and `_report`; it lives here because both models share this mixin):
        the distortion figure of `_report` -- an array per datapoint (cifar, protein) or one float -- without the host copy of the
        reconstruction: rounding and squared error run in rcb_recon_finish and only the per-datapoint fp64 sums come back
        (utils.metric_device).  Agrees with `_report` to the rounding of its float32 evaluation; on_device=False is `_report`.
        size: the signals' own extent inside this model's grid (y = patch_signals(signals, size)): the figure counts the real
        samples only, not the edge padding (rcb_recon_finish_crop); on the device only.
        sample_format (utils.SampleFormat): the lattice the reconstruction is rounded to instead of the dataset's own choice
        (utils.metric_device); on the device only.
        sizes (instead of size): one extent per signal (y = patch_signals(list, sizes=)); the figure counts each signal's real
        samples (rcb_recon_finish_ragged); on the device only."""
        if not on_device:
            if size is not None or sample_format is not None or sizes is not None:
                raise ValueError("report: the figure over a cropped extent or on a sample format's lattice is formed on the "
                                 "device only")
            return self._report(x, y)
        with torch.no_grad():
            y_pred = self.predict(x.to(self.loc.device))
        cropped = size is not None or sizes is not None         # (an extent needs the grid of the unpatched presets too)
        return metric_device(y, y_pred, self.dataset, self.signal_layout() if cropped else self.recon_layout(),
                             size=None if sizes is not None else size, sample_format=sample_format, sizes=sizes)

    def patch_signals(self, signals, size=None, sample_format=None, sizes=None):
        """whole signals [n, *grid, C] on the GPU (uint8 or fp32, any strides: utils.signal_view) -> the targets y [N, P, C] of
        this model's INRs, cut on the device in the row order of recon_layout (rcb_signal_patch); the inverse of the stitching
        in ops.recon_finish.  The unpatched presets are one patch per signal.
        size: the signals are [n, *size, C] with size[i] <= grid[i] and are edge-padded to the grid on the way
        (rcb_signal_patch_pad).
        sample_format (utils.SampleFormat): how the samples are stored -- needed for 16-bit signals (ops.signal_patch).
        sizes (instead of size): `signals` is a LIST of tensors [*sizes[k], C] of mixed sizes and memory layouts, each edge-padded
        to the grid in one call (ops.signal_patch_ragged)."""
        if sizes is not None:
            if size is not None:
                raise ValueError("patch_signals: size and sizes exclude each other")
            got = [tuple(int(v) for v in t.shape[:-1]) for t in signals]
            if got != [tuple(int(v) for v in s) for s in sizes]:
                raise ValueError("patch_signals: signals of extents %r, sizes %r" % (got, [tuple(s) for s in sizes]))
            return ops.signal_patch_ragged(signals, self.signal_layout(), sample_format=sample_format)
        if size is not None:
            if tuple(int(v) for v in size) != tuple(signals.shape[1:-1]):
                raise ValueError("patch_signals: signals of extent %r, size %r" % (tuple(signals.shape[1:-1]), tuple(size)))
            return ops.signal_patch_pad(signals, self.signal_layout(), sample_format=sample_format)
        return ops.signal_patch(signals, self.signal_layout(), sample_format=sample_format)

    def report_signals(self, x, signals, size=None, sample_format=None, sizes=None):
        """`report` against whole signals instead of patch targets (sizes: a list of signals, as patch_signals takes it)"""
        return self.report(x, self.patch_signals(signals, size, sample_format, sizes=sizes), size=size, sample_format=sample_format,
                           sizes=sizes)

    def report_regions(self, x, y, region="patch", size=None, sample_format=None):
        """The distortion figure of `report` BY REGION of every signal, fp64 [n, *nr] (the model with `predict` and `dataset`, as
        `report`): predict, then one pass of rcb_recon_regions (utils.metric_regions_device); only the per-region sums come back.
        Every region gets its own figure -- PSNR (RMSD for protein) over its own elements -- whatever the dataset's batch convention.
        region: "patch" (one figure per patch of the codec: which patch is worst), "frame" (3-D presets: one per frame), "row", or
        a box of one int per axis, e.g. (16, 16) tiles for a distortion map (utils.region_of).  The regions tile the signal's extent
        -- `size` (y = patch_signals(signals, size)), or the model's grid -- so a region on the far edge is smaller, and edge padding
        belongs to none: with size= the figures count real samples only.  sample_format: as `report`.
        This is NOT the video convention by itself: that is the mean over the frames of report_frames."""
        layout = self.signal_layout()
        box = region_of(layout, region)
        with torch.no_grad():
            y_pred = self.predict(x.to(self.loc.device))
        return metric_regions_device(y, y_pred, self.dataset, layout, box, size=size, sample_format=sample_format)

    def report_regions_signals(self, x, signals, region="patch", size=None, sample_format=None):
        """`report_regions` against whole signals instead of patch targets (as report_signals)"""
        return self.report_regions(x, self.patch_signals(signals, size, sample_format), region=region, size=size,
                                   sample_format=sample_format)

    def report_frames(self, x, y_or_signals, size=None, sample_format=None):
        """Per-frame PSNR of the clips this model delivers, fp64 [n, T] -- the PSNR twin of report_ssim_frames, for the 3-D presets,
        axis 0 of the grid being the frame axis.  The video convention is the MEAN of these per-frame PSNRs (and the curve over
        time); the caller averages.  `report` gives the other figure, one PSNR of the whole batch's mean squared error, which
        weights a bad frame more.  y_or_signals: patch targets [N, P, C] (fp32, what the model was fitted to) or whole clips
        [n, T, H, W, C] (of extent `size` when given), which are cut on the device first.  ValueError for a preset that is not
        3-D."""
        if self.data_dim != 3:
            raise ValueError("report_frames: frames are axis 0 of a 3-D preset, this one has %d axes" % self.data_dim)
        report = self.report_regions if y_or_signals.dim() == 3 else self.report_regions_signals
        by_frame = report(x, y_or_signals, region="frame", size=size, sample_format=sample_format)      # [n, T, 1, 1]
        return by_frame.reshape(by_frame.shape[:2])

    @staticmethod
    def _ssim_format(who, sigs, sample_format):
        """what the SSIM reports refuse of their sources -> the format the reconstruction is rounded to"""
        for t in sigs:
            if sample_format is None and t.dtype in (torch.uint16, torch.int16):
                raise ValueError("%s: %s signals need sample_format= (utils.SampleFormat.u16(depth)): the depth is not in "
                                 "the dtype" % (who, t.dtype))
            if t.dtype.is_floating_point:
                raise ValueError("%s: SSIM compares the delivered integers with the source's: %s signals have none"
                                 % (who, t.dtype))
        fmt = sample_format if sample_format is not None else SampleFormat.u8()
        if fmt.kind not in (SampleFormat.U8, SampleFormat.U16):
            raise ValueError("%s: SSIM is defined for u8 and u16 images, not %r" % (who, fmt))
        return fmt

    def report_ssim(self, x, signals, size=None, sample_format=None, sizes=None, multiscale=False):
        """SSIM (with `multiscale`: MS-SSIM) of the images this model delivers against the whole source `signals`, fp64 per signal
        (the model with `predict`, as `report`): predict, round to the format's integers at each signal's own size
        (ops.recon_finish(want_int=True, size=) / ops.recon_finish_ragged for sizes=), then rcb_ssim -- for sizes= ONE rcb_ssim_list
        call, whatever the length of the list -- on those integers against the integers of `signals` (utils.ssim_device; the
        definition is include/rcb.h's).  The figure of the DELIVERED image: nothing
        but the sums leaves the device.
        signals: [n, *size, C] integer images on the model's grid (size None) or of extent `size` inside it, any strides; with
        sizes= a LIST of [*sizes[k], C] tensors -- a portrait signal as compress_signal_list cuts it: its transposed view, and
        sizes[k] the landscape extent it fits the grid with.  sample_format: needed for 16-bit signals (None: uint8).
        ValueError, with the reason: a 1-D or 3-D preset, fp32 (or s16) signals, a 16-bit tensor without a format, an image
        smaller than 11 (multiscale: 176) per side."""
        if self.data_dim != 2:
            raise ValueError("report_ssim: SSIM is defined for 2-D presets, this one has %d axes" % self.data_dim)
        if sizes is not None and size is not None:
            raise ValueError("report_ssim: size and sizes exclude each other")
        listed = sizes is not None
        sigs = list(signals) if listed else [signals]
        fmt = self._ssim_format("report_ssim", sigs, sample_format)
        layout = self.signal_layout()
        grid = tuple(n * s for n, s in zip(layout.patch_nums, layout.patch_size))
        if listed:
            extents = [tuple(int(v) for v in s) for s in sizes]
        else:
            extents = [tuple(int(v) for v in size) if size is not None else grid]
        need = 176 if multiscale else 11
        for e in extents:
            if len(e) != 2 or min(e) < need:
                raise ValueError("report_ssim: an image of %s is too small for %s (both sides at least %d)"
                                 % (" x ".join(str(v) for v in e),
                                    "MS-SSIM's five scales" if multiscale else "SSIM's 11-tap window", need))
        dev = self.loc.device
        want = [e + (self.dims[-1],) for e in extents]
        got = [tuple(t.shape) for t in sigs] if listed else [tuple(signals.shape[1:])]
        if got != want:
            raise ValueError("report_ssim: signals of shape %r, expected %r" % (got, want))
        with torch.no_grad():
            y_pred = self.predict(x.to(dev)).detach().to(torch.float32).contiguous()
        if listed:
            q, _, _, _ = ops.recon_finish_ragged(y_pred, layout=layout, sizes=extents, sample_format=fmt, want_int=True)
            return ssim_device(q, [t.to(dev) for t in sigs], sample_format=fmt, multiscale=multiscale)
        q, _, _, _ = ops.recon_finish(y_pred, layout=layout, size=size, sample_format=fmt, want_int=True)
        return ssim_device(q, signals.to(dev), sample_format=fmt, multiscale=multiscale)

    def report_ssim_frames(self, x, signals, size=None, sample_format=None, multiscale=False):
        """Per-frame SSIM (with `multiscale`: MS-SSIM) of the clips this model delivers against the whole source `signals`, fp64
        [n, T]; the caller averages.  For the 3-D presets, axis 0 of the grid being the frame axis: predict, round to the format's
        integers (ops.recon_finish(want_int=True, size=)), then every frame of every clip in ONE rcb_ssim_list call against the
        source's (ops.ssim_sums_frames): nothing but the sums leaves the device.
        signals: [n, T, H, W, C] integer clips on the model's grid (size None) or of extent `size` = (T, H, W) inside it, any
        strides.  sample_format: needed for 16-bit signals (None: uint8).
        ValueError, with the reason: a preset that is not 3-D, fp32 (or s16) signals, a 16-bit tensor without a format, a frame
        smaller than 11 (multiscale: 176) per side, a wrong shape."""
        who = "report_ssim_frames"
        if self.data_dim != 3:
            raise ValueError("%s: per-frame SSIM is defined for 3-D presets, this one has %d axes" % (who, self.data_dim))
        fmt = self._ssim_format(who, [signals], sample_format)
        layout = self.signal_layout()
        grid = tuple(n * s for n, s in zip(layout.patch_nums, layout.patch_size))
        extent = tuple(int(v) for v in size) if size is not None else grid
        need = 176 if multiscale else 11
        if len(extent) != 3 or min(extent[1:]) < need:
            raise ValueError("%s: a frame of %s is too small for %s (both sides at least %d)"
                             % (who, " x ".join(str(v) for v in extent[1:]),
                                "MS-SSIM's five scales" if multiscale else "SSIM's 11-tap window", need))
        want = extent + (self.dims[-1],)
        if tuple(signals.shape[1:]) != want:
            raise ValueError("%s: signals of shape %r, expected %r" % (who, tuple(signals.shape[1:]), want))
        dev = self.loc.device
        with torch.no_grad():
            y_pred = self.predict(x.to(dev)).detach().to(torch.float32).contiguous()
        q, _, _, _ = ops.recon_finish(y_pred, layout=layout, size=size, sample_format=fmt, want_int=True)
        return ssim_frames_device(q, signals.to(dev), sample_format=fmt, multiscale=multiscale)


    def _ycc_integers(self, who, x, signals, size, sample_format, frames):
        """what the Y'CbCr reports share: the refusals of report_ssim plus "three channels needed", then predict and round to the
        format's integers at the signals' size -> (the delivered integers, the source on the device, the format)"""
        dd = 3 if frames else 2
        if self.data_dim != dd:
            raise ValueError("%s: defined for %d-D presets, this one has %d axes" % (who, dd, self.data_dim))
        fmt = self._ssim_format(who, [signals], sample_format)
        if self.dims[-1] != 3:
            raise ValueError("%s: three channels needed (R, G, B), this preset has %d" % (who, self.dims[-1]))
        layout = self.signal_layout()
        grid = tuple(n * s for n, s in zip(layout.patch_nums, layout.patch_size))
        extent = tuple(int(v) for v in size) if size is not None else grid
        want = extent + (3,)
        if len(extent) != dd or tuple(signals.shape[1:]) != want:
            raise ValueError("%s: signals of shape %r, expected %r" % (who, tuple(signals.shape[1:]), want))
        dev = self.loc.device
        with torch.no_grad():
            y_pred = self.predict(x.to(dev)).detach().to(torch.float32).contiguous()
        q, _, _, _ = ops.recon_finish(y_pred, layout=layout, size=size, sample_format=fmt, want_int=True)
        return q, signals.to(dev), fmt

    def report_ycc(self, x, signals, matrix, subsampling=2, size=None, sample_format=None):
        """PSNR per plane of the Y'CbCr form of the images this model delivers against the whole source `signals`, fp64 [n, 4] =
        {PSNR-Y, PSNR-Cb, PSNR-Cr, (6 Y + Cb + Cr) / 8} -- the figures of the video and image codec comparisons (the model with
        `predict`, as `report`; 2-D presets of three channels): predict, round to the format's integers
        (ops.recon_finish(want_int=True, size=)), then ONE rcb_ycc_sse call against the source's integers (utils.ycc_device; the
        definition is include/rcb.h's); only the sums leave the device.
        signals: [n, H, W, 3] integer RGB images on the model's grid (size None) or of extent `size` inside it, any strides.
        matrix: utils.ycc_matrix(...); subsampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0 (the planes both sides are brought to).
        ValueError, with the reason: what report_ssim refuses of its sources, a preset that is not 2-D, three channels needed."""
        q, src, fmt = self._ycc_integers("report_ycc", x, signals, size, sample_format, frames=False)
        return ycc_device(q, src, matrix, subsampling, sample_format=fmt)

    def report_ycc_frames(self, x, signals, matrix, subsampling=2, size=None, sample_format=None):
        """`report_ycc` per FRAME of the clips a 3-D preset delivers, fp64 [n, T, 4]; the caller averages (the video convention
        is the mean over the frames).  signals: [n, T, H, W, 3] integer clips on the model's grid or of extent `size` = (T, H, W)."""
        q, src, fmt = self._ycc_integers("report_ycc_frames", x, signals, size, sample_format, frames=True)
        return ycc_frames_device(q, src, matrix, subsampling, sample_format=fmt)

    def report_ssim_luma(self, x, signals, matrix, size=None, sample_format=None, multiscale=False):
        """SSIM (with `multiscale`: MS-SSIM) on LUMA -- what Wang et al. define it on -- of the images this model delivers against
        the source, fp64 [n]: both sides go through ops.rgb_to_ycc(want=("y",)) and the existing utils.ssim_device scores the
        planes as [n, H, W, 1].  Arguments and refusals: report_ycc's and report_ssim's size rule (11, multiscale 176, per side)."""
        q, src, fmt = self._ycc_integers("report_ssim_luma", x, signals, size, sample_format, frames=False)
        (ya,), (yb,) = (ops.rgb_to_ycc(t, matrix, 0, sample_format=fmt, want=("y",)) for t in (q, src))
        return ssim_device(ya.unsqueeze(-1), yb.unsqueeze(-1), sample_format=fmt, multiscale=multiscale)

    def report_ssim_luma_frames(self, x, signals, matrix, size=None, sample_format=None, multiscale=False):
        """`report_ssim_luma` per FRAME of the clips a 3-D preset delivers, fp64 [n, T] (utils.ssim_frames_device on the luma planes)."""
        q, src, fmt = self._ycc_integers("report_ssim_luma_frames", x, signals, size, sample_format, frames=True)
        (ya,), (yb,) = (ops.rgb_to_ycc(t, matrix, 0, sample_format=fmt, want=("y",)) for t in (q, src))
        return ssim_frames_device(ya.unsqueeze(-1), yb.unsqueeze(-1), sample_format=fmt, multiscale=multiscale)


class PriorBNNmodel(nn.Module, InrGeometry):
    """Training-set posteriors + batched INR evaluation (prior_model.py:62-262)."""

    def __init__(self, in_dim, hidden_dims, out_dim, train_size, data_dim, pixel_sizes, upsample_factors,
                 latent_dim, patch, patch_nums, hierarchical_patch_nums, random_seed=42, device="cuda",
                 init_log_scale=-4, c=6., w0=30.):
        super().__init__()
        self.random_seed, self.device = random_seed, device
        self.n_layers = len(hidden_dims) + 1
        self.dims = [in_dim] + list(hidden_dims) + [out_dim]
        self.patch, self.w0 = patch, float(w0)
        self.st = lambda x: F.softplus(x, beta=1, threshold=20) / 6
        self.data_dim, self.train_size, self.latent_dim = data_dim, train_size, latent_dim
        self.pixel_sizes, self.upsample_factors = pixel_sizes, upsample_factors
        self.patch_nums, self.hierarchical_patch_nums = patch_nums, hierarchical_patch_nums
        self.net_params_list, self.cum_param_sizes = count_net_params(in_dim, hidden_dims, out_dim)
        D = int(self.cum_param_sizes[-1])
        # (any list of hidden widths, as in the reference, prior_model.py:84-85: widths that differ run in the fp32 parity
        # mode on the plain-FMA kernel; the 16-bit modes take one width -- 32, 48 or 64 -- and say so when asked otherwise)

        # A1: same CPU-generator draw order as the reference (loc, h_loc, hh_loc, lpe_loc), then moved
        torch.manual_seed(random_seed)
        w_std = np.sqrt(c / hidden_dims[-1]) / w0

        def uni(rows):
            return nn.Parameter((torch.rand(rows, D) * w_std * 2 - w_std).to(device))

        def const(rows):
            return nn.Parameter((torch.zeros(rows, D) + init_log_scale).to(device))
        self.loc, self.log_scale = uni(train_size), const(train_size)
        if patch:
            r2 = train_size // int(np.prod(hierarchical_patch_nums["level2"]))
            r3 = train_size // int(np.prod(hierarchical_patch_nums["level3"]))
            self.h_loc, self.h_log_scale = uni(r2), const(r2)
            self.hh_loc, self.hh_log_scale = uni(r3), const(r3)
        lat = [pixel_sizes[i] // upsample_factors[i] for i in range(data_dim)]
        self.lpe_loc = nn.Parameter((torch.randn(train_size, *lat, latent_dim) * 0.1).to(device))
        self.lpe_log_scale = nn.Parameter((torch.zeros(train_size, *lat, latent_dim) + init_log_scale).to(device))
        self._lat = lat
        self._d_net, self._d_lpe = D, int(np.prod(lat)) * latent_dim
        self._maps = hierarchy_row_maps(train_size, patch_nums, hierarchical_patch_nums, data_dim) if patch else None
        self._levels_cache = None
        self.noise_source = None     # optional callable(shape) -> standard normal GPU tensor (eps injection)
        self.precision = 0           # 0 = fp32 MFMA, 1 = bf16 operands (throughput mode)
        self.dp_group = None         # torch.distributed group for sharded training of the shared mappings
        self.lowp_gemm = False       # 16-bit mode only: bf16-operand hipBLASLt GEMMs for the A transform
        self.stage1_bf16 = True      # 16-bit mode only: bf16-operand GEMMs for stage 1 of the upsampling net
        self.pe_bf16 = True          # 16-bit mode only: pe / dpe stored as bf16 (bit-identical, half the traffic)
        self.stitched_pe = True      # 16-bit mode, patched presets: the SIREN kernel reads pe / writes dpe inside the stitched grids
        self.split_gemm = True       # 16-bit mode only: split-bf16 (hi/lo) operands for the A-transform fwd / dgrad GEMMs
        self.split_terms = 2         # with split_gemm: 3 = both operands split; 2 = the mappings enter as bf16 (ops.ATransform)
        self.split_dgrad_terms = None  # with split_gemm: terms of the data-gradient GEMM (None = split_terms)
        self.wgrad_bf16 = True       # with split_gemm: bf16 high parts for the A weight-gradient GEMMs (sum over INRs)
        self.fused_noise = True      # draw eps inside the reparam kernel (Philox) when no noise_source is injected
        # with fused_noise: the posterior update of step t also draws the sample of step t + 1 (rcb_level_bwd.next_*), so
        # the sampling kernels -- a second read of every loc / log_scale -- run once per train() call instead of once per step
        self.fuse_next_sample = os.environ.get("RCB_FUSE_NEXT", "1") != "0"      # (the switch is for same-box A/B runs)
        # with split_gemm + fused_noise: the A transform's per-INR operands (h_w, and the SIREN gradient dwvec) may travel as the
        # (hi, lo) bf16 planes their producers write (ops.Planes) instead of fp32 rows + a bf16 copy: identical bits, no
        # conversion work in the A-transform kernels, 4 instead of 6 bytes per element written.  OFF by default: measured on
        # MI355X (round 4, same-box A/B) the plane kernels are no faster (forward 84.9 vs 80.6 us: the kernel is bound by the
        # operand stream into LDS and the lockstep of its eight waves, not by the conversion) and the producers' 2-byte plane
        # stores cost more than the bytes they save: 1.120 vs 1.095 ms per step.  Kept as a tested option (RCB_PLANES=1).
        self.operand_planes = os.environ.get("RCB_PLANES", "0") != "0"
        # with fuse_next_sample: the posterior update re-draws its step's noise from the counter instead of reading the copy
        # the sampler stored (rcb_level_bwd.eps_from_rng: same bits, 8 bytes per element less traffic)
        self.redraw_noise = os.environ.get("RCB_REDRAW_EPS", "1") != "0"
        # three-level presets: the latent weights' noise drawn in the sampling kernel (RCB_HIER_RNG=0: three randn launches; A/B)
        self.hier_rng = os.environ.get("RCB_HIER_RNG", "1") != "0"
        # concurrent streams inside the captured step (bit mask of 2, 4 and 8, see train_step.py; 0 = one stream; RCB_FORK
        # overrides; any other bit is a ValueError in train()).  Measured on MI355X, same-box A/B of
        # the 4096-INR CIFAR step (gpurun_out r04_ab5): one stream 1.162 ms; A-transform backward beside the upsampling net's
        # backward (2) 1.125; + the net's weight-gradient side on a third stream (6) 1.109; + the network level's posterior
        # update (HBM-bound) straight behind the A backward, i.e. beside the LDS / MFMA-bound upsampling kernels (14) 1.089:
        # -6.2 %.  Same kernels, same operands: bit-identical.  (The orderings once behind the bits 1, 16, 32 and 64 gained
        # nothing or lost 2 to 7 % and are gone: DESIGN.md section 4.5 keeps their measurements.)
        self.stream_forks = 14
        # measurement aid: take the SHARDED form of the step (four captured segments around two host-enqueued all-reduces)
        # even when `dp_group` has a single rank -- what the segmentation costs on the host, without a second GPU
        self.force_segments = False
        # sharded step: None = capture the all-reduces inside the step graph when the backend is RCCL ("nccl"), else four
        # segments around host-enqueued collectives; True / False force one form
        # None: automatic (inside the step graph when the backend is RCCL); RCB_CAPTURE_COLLECTIVES=0 / 1 forces the four-segment
        # form / the captured form without a code change (the escape hatch of a multi-GPU run)
        self.capture_collectives = {"0": False, "1": True}.get(os.environ.get("RCB_CAPTURE_COLLECTIVES", ""), None)
        # in-kernel noise: first row of this model's INRs inside a larger (virtual) batch.  Row r of the model draws the noise of
        # row rng_row_offset + r of that batch (ops.rng_group_offset): a shard or a sub-batch trained on its own then sees
        # exactly the noise of the unsharded run, given the same seed (`rng_seed_override`, else derived per model and rank)
        self.rng_row_offset = 0
        self.rng_seed_override = None
        self._train_calls = 0
        self._ws = None              # persistent training workspace (captured graphs + everything they reference)
        self._rng_ctr_init = 0       # first value of the noise counter of a new workspace (tests build exact twins)
        self.use_graph = True        # replay the training step as one captured HIP graph when possible

    # ---- level descriptions ------------------------------------------------------------------------
    def _levels(self):
        """LevelSpecs of the latent-weight hierarchy [level1, (level2, level3)] and of the lpe."""
        c = self._levels_cache
        if c is None or c["dev"] != self.loc.device:
            N, D = self.train_size, self._d_net
            net = [LevelSpec(self.loc, self.log_scale, D, N)]
            if self.patch:
                net.append(LevelSpec(self.h_loc, self.h_log_scale, D, N, row_map=self._maps[0]))
                net.append(LevelSpec(self.hh_loc, self.hh_log_scale, D, N, row_map=self._maps[1]))
            c = {"dev": self.loc.device, "net": net}
            self._levels_cache = c
        lpe = LevelSpec(self.lpe_loc.view(self.train_size, -1), self.lpe_log_scale.view(self.train_size, -1),
                        self._d_lpe, self.train_size)
        return c["net"], lpe

    def _noise(self, shape):
        if self.noise_source is not None:
            e = self.noise_source(tuple(shape))
            return e.to(self.loc.device, torch.float32).reshape(shape).contiguous()
        return torch.randn(shape, device=self.loc.device, dtype=torch.float32)

    # ---- reference API: helpers ----------------------------------------------------------------------
    def layer_to_weight(self, in_dim, out_dim, layer_param):
        bias = layer_param[:, :out_dim]
        weights = layer_param[:, out_dim:].reshape(-1, in_dim, out_dim)
        return weights, bias

    # ---- reference API: forward (autograd-capable) -----------------------------------------------------
    def forward(self, x, linear_transform, upsample_net, gradient_through_A=True):
        """x [N, P, F] (or [P, F] shared grid) -> y_hat [N, P, C]  (prior_model.py:129-179).
        Noise draw order as in the reference: lpe, level 1, level 2, level 3."""
        assert x.shape[0] == self.train_size or x.dim() == 2
        N = self.train_size
        net, lpe_lv = self._levels()
        e_lpe = self._noise((N, 1, self._d_lpe))
        lpe = ops.sample_levels([lpe_lv], [e_lpe], 1)                       # [N,1,Dlpe]
        lpe = lpe.reshape(N, *self._lat, self.latent_dim)[None]
        pe = self._pe(upsample_net, lpe)[:, 0]
        eps = [self._noise((N, 1, self._d_net)) for _ in net]
        h_w = ops.sample_levels(net, eps, 1)[:, 0]                          # [N, D_net]
        parts = []
        for idx, (lo, hi) in enumerate(self._layer_slices()):
            A = linear_transform.A[idx] if gradient_through_A else linear_transform.A[idx].detach()
            parts.append(h_w[:, lo:hi] @ A)
        wvec = torch.cat(parts, -1)
        return ops.SirenFn.apply(x, pe.contiguous(), wvec, self._meta(x, pe.shape[-1]))

    def calculate_kl(self, prior_loc, prior_scale, prior_lpe_loc, prior_lpe_scale, prior_h_loc, prior_h_scale,
                     prior_hh_loc, prior_hh_scale):
        """Sum of elementwise Gaussian KLs over all levels (prior_model.py:181-200) -> 0-d tensor."""
        def one(loc, ls, pl, ps):
            return ops.GaussKLFn.apply(loc, ls, pl.contiguous(), ps.contiguous(), False, None, None, None, None)
        kl = one(self.loc, self.log_scale, prior_loc, prior_scale)
        kl = kl + one(self.lpe_loc, self.lpe_log_scale, prior_lpe_loc, prior_lpe_scale)
        if self.patch:
            kl = kl + one(self.h_loc, self.h_log_scale, prior_h_loc, prior_h_scale)
            kl = kl + one(self.hh_loc, self.hh_log_scale, prior_hh_loc, prior_hh_scale)
        return kl

    def _kl_value(self, priors):
        """fp64 0-d KL on device, no autograd."""
        tot = None
        pairs = [(self.loc, self.log_scale, priors[0], priors[1]),
                 (self.lpe_loc, self.lpe_log_scale, priors[2], priors[3])]
        if self.patch:
            pairs += [(self.h_loc, self.h_log_scale, priors[4], priors[5]),
                      (self.hh_loc, self.hh_log_scale, priors[6], priors[7])]
        for loc, ls, pl, ps in pairs:
            r, _ = ops.gauss_kl(loc, ls, pl.contiguous(), ps.contiguous())
            tot = r.sum() if tot is None else tot + r.sum()
        return tot

    # ---- reference API: train (fused pipeline) -----------------------------------------------------------
    def train(self, n_epoch, lr, x, y, prior_loc, prior_scale, prior_lpe_loc, prior_lpe_scale, prior_h_loc,
              prior_h_scale, prior_hh_loc, prior_hh_scale, linear_transform, upsample_net, kl_beta,
              training_mappings=True, verbose=False):
        """n_epoch Adam steps on loss = mean((y_hat-y)^2)*N + kl_beta*KL with a fresh Adam
        (prior_model.py:202-262).  Returns (MSE_last/N, KL/N, ELBO list).  NB: shadows nn.Module.train
        exactly like the reference does."""
        dev = self.loc.device
        x = x.to(dev)
        y = y.to(dev).contiguous()
        N = y.shape[0]
        priors = [prior_loc, prior_scale, prior_lpe_loc, prior_lpe_scale, prior_h_loc, prior_h_scale,
                  prior_hh_loc, prior_hh_scale]
        priors = [None if p is None else p.detach().to(dev, torch.float32).contiguous() for p in priors]
        # the step itself -- what it launches (StepPlan), the workspace `self._ws` with its captured graphs, the segments -- lives
        # in train_step.py; a workspace whose key still holds is found again here, else a new one is built
        step = train_step.PriorTrainStep(self, n_epoch, lr, x, y, priors, linear_transform, upsample_net, training_mappings,
                                         verbose)
        ws = step.ws
        step.prime(kl_beta, priors)
        if step.plan.graphable and (ws["graphs"] is not None or n_epoch > train_step.N_WARM):
            left = n_epoch
            failure = None
            if ws["graphs"] is None:               # first call with this workspace: warm up eagerly, then capture
                for _ in range(train_step.N_WARM):
                    step.body()
                left -= train_step.N_WARM
                failure = step.capture()
            if failure is None:
                step.replay(left)
            else:
                import warnings
                warnings.warn(f"HIP graph capture of the training step failed ({failure}); running eagerly")
                ws["graphs"] = None
                self._ws = None
                self.use_graph = False
                for _ in range(left):
                    step.body()
        else:
            it = range(n_epoch)
            if verbose:
                from tqdm import tqdm
                it = tqdm(it)
            for _ in it:
                step.body()
        mse_buf, kl_buf = ws["mse_buf"][:n_epoch], ws["kl_buf"][:n_epoch]
        kl_final = self._kl_value(priors)
        # one transfer (one synchronisation) for everything the call returns: [elbo per step ..., last MSE, final KL]
        out_h = torch.cat([-(mse_buf + kl_buf * float(kl_beta)), mse_buf[-1:], kl_final.reshape(1)]).cpu()
        return float(out_h[-2]) / N, float(out_h[-1]) / N, out_h[:-2].tolist()


# ------------------------------------------------------------------------------------------------------
# grouping (prior_model.py:264-316) -- host side, as in the reference
# ------------------------------------------------------------------------------------------------------
def get_grouping(q_loc, q_scale, prior_loc, prior_scale):
    """Mean-over-rows KL in bits per parameter (HIP reduction), then greedy packing on the host."""
    rows = q_loc.shape[0]
    colsum = ops.gauss_kl_colsum(q_loc, q_scale, prior_loc, prior_scale, q_is_log=False)
    weights = (colsum / np.log(2.) / rows).to(torch.float32).cpu().numpy()
    return get_grouping_by_kl(weights)


def group_parameters(parameters, weights, max_weight=16):
    """Sequential greedy packing; the running sum keeps the dtype of `weights` (fp32 in practice)."""
    groups = [[parameters[0]]]
    run = weights[0]
    for i in range(1, len(parameters)):
        if run + weights[i] > max_weight:
            groups.append([parameters[i]])
            run = weights[i]
        else:
            groups[-1].append(parameters[i])
            run = run + weights[i]
    return groups


def get_grouping_by_kl(kls_bits):
    """-> (group_idx, group_start_index, group_end_index, group2param, param2group, n_groups,
    group_kls, weights) with the fixed np.random.seed(0) shuffle (prior_model.py:273-299)."""
    D = kls_bits.shape[0]
    np.random.seed(0)
    order = np.random.choice(D, D, False)
    np.random.seed(None)
    result = group_parameters(np.arange(D)[order], kls_bits[order])
    sizes = np.array([len(g) for g in result])
    n_groups = len(result)
    param2group = np.concatenate([np.asarray(g) for g in result])
    group2param = np.argsort(param2group)
    group_idx = np.repeat(np.arange(n_groups), sizes).astype(int)
    end = np.cumsum(sizes)
    start = end - sizes
    group_kls = np.array([sum(kls_bits[j] for j in g) for g in result])
    return group_idx, start, end, group2param, param2group, n_groups, group_kls, kls_bits
