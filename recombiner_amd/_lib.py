"""ctypes binding of librcb_hip.so (include/rcb.h).  The product has no CPU fallback: if the
library is missing or a call fails, an exception is raised."""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# RCB_LIB: alternative build of the same ABI (same-box A/B timing of kernel changes); never a different backend
LIB_PATH = os.environ.get("RCB_LIB") or os.path.join(_HERE, "lib", "librcb_hip.so")

class RcbError(RuntimeError):
    pass


class SirenDesc(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("samples", C.c_int32), ("n_pix", C.c_int32), ("fourier_dim", C.c_int32),
                ("pe_dim", C.c_int32), ("n_hidden", C.c_int32), ("hidden", C.c_int32), ("out_dim", C.c_int32),
                ("xf_inr_stride", C.c_int64), ("w_row_stride", C.c_int64), ("w0", C.c_float),
                ("precision", C.c_int32), ("pe_bf16", C.c_int32), ("dw_bf16", C.c_void_p), ("pixel_chunks", C.c_int32),
                ("xf_bf16", C.c_void_p), ("pe_grid_dims", C.c_int32), ("pe_patch_nums", C.c_int32 * 3),
                ("pe_patch_size", C.c_int32 * 3), ("dw_bf16_stride", C.c_int64), ("hidden_dims", C.c_int32 * 4),
                ("dw_lo", C.c_void_p), ("clock_probe", C.c_void_p)]


class Level(C.Structure):
    _fields_ = [("loc", C.c_void_p), ("log_scale", C.c_void_p), ("enc_sample", C.c_void_p),
                ("enc_mask", C.c_void_p), ("row_map", C.c_void_p), ("row_perm", C.c_void_p),
                ("col_map", C.c_void_p), ("eps", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32),
                ("cols_out", C.c_int32), ("scale_is_sigma", C.c_int32), ("mu_sigma_ws", C.c_void_p)]


class RecDesc(C.Structure):
    _fields_ = [("loc", C.c_void_p), ("scale", C.c_void_p), ("p_loc", C.c_void_p), ("p_scale", C.c_void_p),
                ("rows", C.c_int32), ("cols", C.c_int32), ("tables_t", C.c_void_p), ("table_absmax", C.c_void_p),
                ("max_glen", C.c_int32), ("gumbel", C.c_void_p), ("gumbel_absmax", C.c_double),
                ("n_candidates", C.c_int32), ("job_row", C.c_void_p), ("job_start", C.c_void_p),
                ("job_glen", C.c_void_p), ("n_jobs", C.c_int32)]


class AdamTensor(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64)]


class AdamCfg(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("step", C.c_int32), ("dyn_scalars", C.c_void_p)]


class LevelBwd(C.Structure):
    _fields_ = [("loc", C.c_void_p), ("log_scale", C.c_void_p), ("enc_mask", C.c_void_p), ("p_loc", C.c_void_p),
                ("p_scale", C.c_void_p), ("p_scale_is_log", C.c_int32), ("beta", C.c_void_p),
                ("group_idx", C.c_void_p), ("n_groups", C.c_int32), ("kl_scalar", C.c_float),
                ("d_out", C.c_void_p), ("eps", C.c_void_p), ("member_ptr", C.c_void_p),
                ("member_idx", C.c_void_p), ("row_perm_inv", C.c_void_p), ("col_inv", C.c_void_p),
                ("rows", C.c_int32), ("cols", C.c_int32), ("cols_out", C.c_int32), ("samples", C.c_int32),
                ("g_loc", C.c_void_p), ("g_log_scale", C.c_void_p), ("m_loc", C.c_void_p), ("v_loc", C.c_void_p),
                ("m_ls", C.c_void_p), ("v_ls", C.c_void_p), ("kl_accum", C.c_void_p), ("kl_scalar_dev", C.c_void_p),
                ("next_out", C.c_void_p), ("next_eps", C.c_void_p), ("next_out_bf16", C.c_void_p),
                ("next_ld_bf16", C.c_int64), ("rng_seed", C.c_uint64), ("rng_step_dev", C.c_void_p),
                ("rng_step_add", C.c_int64), ("rng_stream", C.c_uint32), ("eps_from_rng", C.c_uint32),
                ("rng_group_offset", C.c_uint64), ("next_out_lo", C.c_void_p), ("sample_sum_ws", C.c_void_p), ("col_map", C.c_void_p)]


_lib = None
# the header these mirrors were written against (include/rcb.h: RCB_VERSION) and the structures load() verifies by size
ABI_VERSION = 419
_MIRRORS = {0: SirenDesc, 1: Level, 2: LevelBwd, 3: AdamCfg, 4: AdamTensor, 5: RecDesc}

# The prototype of every entry point of include/rcb.h, in header order: name -> (restype, [argtypes]).  load() applies it, so
# ctypes converts Python numbers to the declared width and refuses an argument of the wrong class; the CPU tests hold the
# table and the mirrors above to the header text (tests/test_host_cpu.py).  rcb_stream_t and every data pointer are c_void_p
# (ptr() / addr() check what a tensor holds); a descriptor pointer takes byref(d), an array of the mirror, or None.
_int, _i32, _i64, _u32, _u64, _f32, _f64, _p = C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_double, C.c_void_p
_siren, _level, _level_bwd = C.POINTER(SirenDesc), C.POINTER(Level), C.POINTER(LevelBwd)
_adam_cfg, _adam_tensor, _rec = C.POINTER(AdamCfg), C.POINTER(AdamTensor), C.POINTER(RecDesc)
PROTOTYPES = {
    "rcb_version": (_int, []),
    "rcb_last_error_string": (C.c_char_p, []),
    "rcb_struct_bytes": (_i64, [_i32]),
    "rcb_debug_siren_wave_tiles": (_int, [_i32]),
    "rcb_siren_fwd": (_int, [_siren] + [_p] * 5),
    "rcb_siren_bwd": (_int, [_siren] + [_p] * 7),
    "rcb_siren_reduce_chunks": (_int, [_siren] + [_p] * 5),
    "rcb_siren_loss_bwd": (_int, [_siren, _p, _p, _p, _p, _f32, _p, _p, _p, _p]),
    "rcb_reparam_fwd": (_int, [_level, _i32, _i32, _i32, _i32, _p, _p]),
    "rcb_reparam_hier_rng_fwd": (_int, [_level, _i32, _i32, _i32, _p, _p, _u64, _p, _p, _u64, _p]),
    "rcb_philox_normal": (_int, [_p, _i64, _u64, _u32, _p, _i64, _u64, _p]),
    "rcb_reparam_rng_fwd": (_int, [_p, _p, _i64, _u64, _u32, _p, _p, _p, _p, _p, _i32, _i64, _u64, _p]),
    "rcb_gauss_kl": (_int, [_p, _p, _p, _p, _i32, _i32, _i32, _p, _p, _i32, _p, _p, _p, _p, _p]),
    "rcb_gauss_kl_colsum": (_int, [_p, _p, _i32, _p, _p, _i32, _i32, _p, _p]),
    "rcb_beta_update": (_int, [_p, _p, _p, _i32, _i32, _f64, _f64, _f64, _f64, _p]),
    "rcb_posterior_bwd": (_int, [_level_bwd, _adam_cfg, _p]),
    "rcb_adam_flat": (_int, [_p, _p, _p, _p, _i64, _adam_cfg, _p]),
    "rcb_adam_multi": (_int, [_adam_tensor, _i32, _adam_cfg, _p]),
    "rcb_debug_generic_kernels_only": (_int, [_i32]),
    "rcb_atrans_pack_elems": (_i64, [_i32, _p]),
    "rcb_atrans_pack": (_int, [_p, _i32, _p, _p, _i32, _p]),
    "rcb_atrans_plan": (_int, [_i64, _i32, _p, _i32, _p, _i32]),
    "rcb_atrans_apply": (_int, [_p, _i64, _p, _p, _i64, _p, _i64, _i64, _i32, _p, _p, _i32, _i32, _p, _p, _p, _p]),
    "rcb_atrans_workspace_floats": (_i64, [_i64, _i32, _p, _p]),
    "rcb_atrans_wgrad_narrow_workspace": (_i64, [_i32, _i32]),
    "rcb_atrans_wgrad_narrow": (_int, [_p, _p, _p, _i64, _p, _p, _p, _i64, _i64, _i32, _p, _p, _i32, _p]),
    "rcb_step_begin": (_int, [_p, _i64, _p, _p, _p, _p]),
    "rcb_step_end": (_int, [_p, _i32, _f64, _p, _p, _p, _i64, _p, _p, _p]),
    "rcb_step_prepare": (_int, [_p, _i64, _p, _p, _p, _p, _i32, _p, _p, _i32] + [_p] * 6 + [_i32, _p, _p, _p, _p]),
    "rcb_step_tail_eligible": (_int, [_level_bwd]),
    "rcb_step_tail": (_int, [_level_bwd, _adam_cfg, _adam_tensor, _i32, _p, _i32, _f64, _p, _p, _i64, _p, _p, _p, _p]),
    "rcb_col_moments": (_int, [_p, _p, _i32, _i32, _p, _p]),
    "rcb_rec_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "rcb_rec_score_argmax": (_int, [_rec, _i32, _p, _i64, _p, _p, _p, _p, _p]),
    "rcb_rec_commit": (_int, [_rec, _p, _p, _i32] + [_p] * 7),
    "rcb_upconv_fwd": (_int, [_p, _i32, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p]),
    "rcb_upconv_dgrad_partial_rows": (_i32, [_i32]),
    "rcb_upconv_dgrad": (_int, [_p, _i32, _p, _p, _i32, _p, _p, _i32, _i32, _i32, _p, _p]),
    "rcb_upconv_wgrad_workspace": (_i64, [_i32, _i32]),
    "rcb_upconv_wgrad": (_int, [_p, _i32, _p, _i32, _p, _p, _i32, _i32, _i32, _p, _i64, _p]),
    "rcb_upconv_bwd_fused": (_int, [_p] * 6 + [_i32, _i32, _i32, _p, _i64, _p, _p]),
    "rcb_upconv_fwd23": (_int, [_p, _i32, _p, _p, _p, _p, _i32, _i32, _p, _p]),
    "rcb_upconv_weff_build": (_int, [_p] * 6 + [_i32, _p, _p, _p, _p]),
    "rcb_upconv_weff_grad": (_int, [_p, _i32, _p, _p, _p, _p, _p, _p, _i32, _p, _p]),
    "rcb_tile_gather": (_int, [_p, _p] + [_i32] * 10 + [_p]),
    "rcb_tile_crop": (_int, [_p, _p] + [_i32] * 8 + [_p]),
    "rcb_tile_fold": (_int, [_p, _p] + [_i32] * 8 + [_p]),
    "rcb_phaseconv_pack_uint4": (_i64, [_i32, _i32, _i32]),
    "rcb_phaseconv_pack": (_int, [_p, _i32, _i32, _p, _p, _p]),
    "rcb_phaseconv_fwd": (_int, [_p] * 4 + [_i32] * 7 + [_p]),
    "rcb_phaseconv_dgrad": (_int, [_p] * 4 + [_i32] * 6 + [_p]),
    "rcb_phaseconv_wgrad_workspace": (_i64, [_i32, _i32]),
    "rcb_phaseconv_wgrad": (_int, [_p] * 5 + [_i64] + [_i32] * 6 + [_p]),
    "rcb_stage1_1d_fwd": (_int, [_p, _p, _p, _p, _i32, _i32, _p]),
    "rcb_stage1_1d_dgrad": (_int, [_p, _p, _p, _i32, _i32, _p]),
    "rcb_stage1_1d_wgrad_workspace": (_i64, []),
    "rcb_stage1_1d_wgrad": (_int, [_p] * 5 + [_i64, _i32, _i32, _p]),
    "rcb_window_gather": (_int, [_p, _p] + [_i32] * 6 + [_p]),
    "rcb_window_fold": (_int, [_p, _p] + [_i32] * 6 + [_p]),
    "rcb_phase_bigweight": (_int, [_p, _p, _i32, _i32, _p, _i32, _i32, _i32, _i32, _p]),
    "rcb_phase_bigweight_grad": (_int, [_p, _i32, _p, _i32, _p, _i32, _i32, _i32, _i32, _p]),
    "rcb_softplus_scale": (_int, [_p, _p, _i64, _p]),
    "rcb_recon_workspace_bytes": (_i64, [_i64, _i64]),
    "rcb_recon_finish": (_int, [_p, _p, _i64, _i32, _i32, _i32, _p, _p, _i32, _p, _p, _p, _p, _p, _i64, _p]),
    "rcb_signal_patch": (_int, [_p, _i32, _i64, _i32, _p, _p, _i32, _i64, _p, _i64, _p, _p]),
    "rcb_signal_patch_pad": (_int, [_p, _i32, _i64, _i32, _p, _p, _p, _i32, _i64, _p, _i64, _p, _p]),
    "rcb_recon_finish_crop": (_int, [_p, _p, _i64, _i32, _i32, _i32, _p, _p, _p, _i32, _p, _p, _p, _p, _p, _i64, _p]),
    "rcb_signal_patch_fmt": (_int, [_p, _i32, _i32, _i64, _i32, _p, _p, _p, _i32, _i64, _p, _i64, _p, _p]),
    "rcb_recon_finish_fmt": (_int, [_p, _p, _i64, _i32, _i32, _i32, _p, _p, _p, _i32, _i32, _p, _p, _p, _p, _p, _i64, _p]),
    "rcb_ragged_table_bytes": (_i64, [_i64]),
    "rcb_signal_patch_ragged": (_int, [_p, _i64, _i32, _i32, _i64, _i32, _p, _p, _p, _p, _i32, _i64, _p, _p, _i64, _p]),
    "rcb_recon_finish_ragged": (_int, [_p, _p, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _i64, _i32, _i32, _p, _p, _p, _p, _p, _i64, _p,
                                       _i64, _p]),
    "rcb_recon_regions_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "rcb_recon_regions": (_int, [_p, _p, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _i32, _i32, _p, _p, _p, _i64, _p]),
    "rcb_ssim_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32, _i32]),
    "rcb_ssim": (_int, [_p, _p, _i32, _i32, _i64, _i32, _i32, _i32, _p, _p, _p, _f64, _f64, _i32, _p, _p, _p, _i64, _p]),
    "rcb_ssim_list_table_bytes": (_i64, [_i64, _i32]),
    "rcb_ssim_list_workspace_bytes": (_i64, [_i64, _p, _i32, _i32]),
    "rcb_ssim_list_plan": (_int, [_i64, _p, _i32, _i32, _p, _i64]),
    "rcb_ssim_list": (_int, [_p, _i64, _p, _i64, _i32, _i32, _i64, _p, _p, _p, _i32, _p, _f64, _f64, _i32, _p, _p, _i64, _p, _i64,
                             _p]),
    "rcb_resize_taps": (_int, [_i32, _i32, _p, _p, _p, _i32]),
    "rcb_resize_table_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "rcb_resize": (_int, [_p, _i64, _i32, _i32, _i64, _i32, _i32, _i32, _i32, _p, _i64, _i32, _i32, _p, _p, _i64, _p]),
    "rcb_ycc_to_rgb": (_int, [_p] * 7 + [_i32, _i32, _i32, _i64, _i32, _i32, _i32, _p, _p, _p, _p]),
    "rcb_rgb_to_ycc": (_int, [_p, _i64, _p, _i64, _i32, _i32, _i32, _i64, _i32, _i32, _i32] + [_p] * 6),
    "rcb_ycc_sse": (_int, [_p, _i64, _p, _i64, _p, _i64, _p, _i64, _i32, _i32, _i32, _i64, _i32, _i32, _i32, _p, _p, _p, _p]),
    "rcb_resample_taps": (_int, [_i32, _i32, _p, _p, _p, _p, _p, _i32]),
    "rcb_resample_length": (_i64, [_i64, _i32, _i32]),
    "rcb_resample_table_bytes": (_i64, [_i32, _i32]),
    "rcb_resample": (_int, [_p, _i64, _i32, _i64, _i32, _i32, _p, _i64, _i32, _i32, _p, _f64, _f64, _i32, _p, _p, _i64, _p]),
}
EXPORTS = list(PROTOTYPES)


def load():
    """dlopen the in-tree library (raises if it has not been built) and give every entry point its prototype."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RcbError(f"{LIB_PATH} not found: run `python -m recombiner_amd.build` (no CPU fallback exists)")
        lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            if not hasattr(lib, name):
                raise RcbError(f"{LIB_PATH} does not export {name}")
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        if lib.rcb_version() != ABI_VERSION:
            raise RcbError(f"{LIB_PATH} is ABI version {lib.rcb_version()}, this binding was written against {ABI_VERSION}: "
                           "rebuild with `python -m recombiner_amd.build --force`")
        for which, cls in _MIRRORS.items():
            if lib.rcb_struct_bytes(which) != C.sizeof(cls):
                raise RcbError(f"{cls.__name__}: the library's structure has {lib.rcb_struct_bytes(which)} bytes, the ctypes "
                               f"mirror {C.sizeof(cls)} -- _lib.py has drifted from include/rcb.h")
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        msg = load().rcb_last_error_string().decode(errors="replace")
        raise RcbError(f"{what} failed with code {rc}: {msg}")


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, dtype=None, allow_none=False):
    """device pointer of a contiguous CUDA tensor (or NULL when allowed)."""
    if t is None:
        if allow_none:
            return C.c_void_p(0)
        raise RcbError("null tensor")
    if not t.is_cuda:
        raise RcbError("tensor must live on the GPU (the HIP path has no CPU fallback)")
    if not t.is_contiguous():
        raise RcbError("tensor must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise RcbError(f"expected {dtype}, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


def addr(t, dtype=None):
    """integer address for structure fields (None -> NULL)."""
    if t is None:
        return None
    return ptr(t, dtype).value
