/*
 * librcb_hip  --  C ABI of the MI355X (gfx950) kernels behind the RECOMBINER per-datapoint
 * INR training hot path.
 *
 * The reference (cambridge-mlg/RECOMBINER) is pure PyTorch and has no FFI of its own; each entry
 * point below replaces a sequence of torch ops on the reference's hot path and cites it
 * (file:line relative to the reference root).  Conventions:
 *   - plain device pointers + explicit sizes; the caller (PyTorch, or any HIP host) allocates
 *     every buffer including outputs; nothing is allocated, freed or synchronised inside (but for the one table upload of the
 *     two per-signal entries of 413, of the list entry of 415, of the resize entry of 416 and of the resample entry of 419, which say so);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it;
 *   - return value: 0 = ok, < 0 = argument/shape error (RCB_ERR_*), > 0 = hipError_t;
 *   - no global mutable state besides the thread-local last-error string; re-entrant per stream;
 *   - fp32 tensors are row-major and contiguous unless a stride argument says otherwise.
 */
#ifndef RCB_H_
#define RCB_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* major * 100 + minor; bumped with every change of a signature or of a structure layout (100: rounds 1-3; 400: round 4 --
 * rcb_level.scale_is_sigma, rcb_struct_bytes, the hi / lo operand planes of the A transform; 408: rcb_upconv_fwd23;
 * 409: rcb_recon_finish; 410: rcb_signal_patch; 411: rcb_signal_patch_pad, rcb_recon_finish_crop; 412: rcb_signal_patch_fmt,
 * rcb_recon_finish_fmt; 413: rcb_ragged_table_bytes, rcb_signal_patch_ragged, rcb_recon_finish_ragged; 414: rcb_ssim_workspace_bytes, rcb_ssim;
 * 415: rcb_ssim_list_table_bytes, rcb_ssim_list_workspace_bytes, rcb_ssim_list_plan, rcb_ssim_list;
 * 416: rcb_resize_taps, rcb_resize_table_bytes, rcb_resize; 417: rcb_recon_regions_workspace_bytes, rcb_recon_regions;
 * 418: rcb_ycc_to_rgb, rcb_rgb_to_ycc, rcb_ycc_sse; 419: rcb_resample_taps, rcb_resample_length, rcb_resample_table_bytes, rcb_resample).
 * A binding compares rcb_version() with the RCB_VERSION it was written against and rcb_struct_bytes() with the size of each of its mirrors. */
#define RCB_VERSION 419
#define RCB_OK 0
#define RCB_ERR_ARG (-1)
#define RCB_ERR_SHAPE (-2)
#define RCB_ERR_UNSUPPORTED (-3)
#define RCB_KL_SLOTS 1024
#define RCB_KL_FX_SCALE 16777216.0   /* 2^24: the KL slots count 2^-24 nats */

typedef void* rcb_stream_t;

int rcb_version(void);
const char* rcb_last_error_string(void);
/* sizeof() of the descriptor structures as this library was compiled -- which: 0 rcb_siren_desc, 1 rcb_level,
 * 2 rcb_level_bwd, 3 rcb_adam_cfg, 4 rcb_adam_tensor, 5 rcb_rec_desc; -1 for any other value.  A hand-written mirror of a
 * structure (ctypes, cffi ...) that has drifted from this header is caught at load time instead of corrupting a launch. */
#define RCB_STRUCT_SIREN_DESC 0
#define RCB_STRUCT_LEVEL 1
#define RCB_STRUCT_LEVEL_BWD 2
#define RCB_STRUCT_ADAM_CFG 3
#define RCB_STRUCT_ADAM_TENSOR 4
#define RCB_STRUCT_REC_DESC 5
int64_t rcb_struct_bytes(int32_t which);

/* ---------------------------------------------------------------------------------------------
 * K3 + K4: batched SIREN coordinate-MLP, one workgroup per (INR, sample).
 * Replaces prior_model.py:168-179 (+121-127) and test_model.py:347-355 (+269-280): per layer
 * `x = x @ W + b; x = sin(30 x)` with per-INR weights, and the MSE term prior_model.py:237 /
 * test_model.py:625-627.
 *
 * Input features of layer 0 are the concatenation [xf | pe] (prior_model.py:155): `xf` is the
 * Fourier embedding [*, P, F] (row stride xf_inr_stride between INRs, 0 = one grid shared by all
 * INRs), `pe` the upsampled positional encodings [G, P, E] (E may be 0 with pe = NULL).
 * `wvec` row g holds the layer vectors back to back, each `[bias(out) | W(in,out) row-major]`
 * (prior_model.py:125-126); rows are w_row_stride floats apart.  G = N*S; sample s of INR n is
 * row g = n*S + s; targets / xf are indexed by n = g / S.
 * Hidden width 16, 24, 32, 48 or 64 in the 16-bit modes (16 / 24: one wave per row, siren_mlp_rowwave.hip, F and E <= 32 each);
 * any width up to 64 in the fp32 mode (32 on the matrix cores, the others on a plain-FMA parity kernel, reference
 * prior_model.py:84-85); 1..7 hidden layers (8 linear layers: the A transform's RCB_ATRANS_MAX_LAYERS), out_dim <= 32,
 * F + E <= 64.  5..7 hidden layers take one width for every layer (no hidden_dims list): 16, 24 or 32 in the 16-bit modes (one
 * wave per row, siren_mlp_rowwave.hip, F, E and out_dim <= 32 each), any width up to 64 in the fp32 mode (plain-FMA parity kernel).
 * precision: 0 = fp32 MFMA (exact fp32 products); 1 = bf16 operands, 2 = f16 operands (both fp32 accumulate;
 * f16 carries gradients scaled by 2^10 internally).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_rows;        /* G = N * S workgroups                                   */
  int32_t samples;       /* S                                                       */
  int32_t n_pix;         /* P                                                       */
  int32_t fourier_dim;   /* F                                                       */
  int32_t pe_dim;        /* E                                                       */
  int32_t n_hidden;      /* number of hidden layers (1..7)                          */
  int32_t hidden;        /* hidden width (16-bit: 16, 24, 32, 48, 64; fp32: 1 .. 64) */
  int32_t out_dim;       /* C                                                       */
  int64_t xf_inr_stride; /* floats between INRs in xf; 0 = shared grid              */
  int64_t w_row_stride;  /* floats between rows of wvec and of dwvec                */
  float   w0;            /* sine frequency (30)                                     */
  int32_t precision;     /* 0 fp32, 1 bf16, 2 f16 operands                           */
  int32_t pe_bf16;       /* 1: pe and dpe are bf16 arrays (precision >= 1, pe_dim % 8 == 0): the 16-bit
                          * kernels round pe / dpe to bf16 for their MFMA operands anyway, so storing
                          * them as bf16 gives bit-identical results with half the traffic        */
  void* dw_bf16;         /* nullable, 16-bit kernels, rcb_siren_bwd / _loss_bwd only: besides dwvec, a bf16 copy of it,
                          * [n_rows][dw_bf16_stride] with dwvec's column layout -- the operand of the batched bf16
                          * weight-gradient GEMM of the A transform (rcb_atrans_*), written while the values are in
                          * registers instead of by a cast pass over dwvec                                      */
  int32_t pixel_chunks;  /* 0 / 1: one workgroup per row of wvec.  c > 1 (16-bit kernels): the 32-pixel tiles of every row
                          * are split over c workgroups (launches with few rows -- one Kodak photo is 96 INRs -- would
                          * otherwise leave most of the 256 CUs idle).  y_out / dpe are unaffected; dwvec and sse then
                          * receive PARTIAL results: dwvec [c][n_rows][w_row_stride], sse [c][n_rows], to be summed in
                          * chunk order by rcb_siren_reduce_chunks; dw_bf16 must be NULL (the reduction emits it)   */
  const void* xf_bf16;   /* nullable, 16-bit operand modes with pe_bf16 = 1: a 16-bit copy of xf IN THE OPERAND FORMAT (bf16 for
                          * precision 1, IEEE f16 for precision 2), rows padded with zeros to a multiple of 8 features
                          * ([P][8 * ceil(F / 8)], 16-byte rows; the per-row stride is xf_row_stride / F * that; since version
                          * 406 -- before, bf16 only, unpadded, and ignored unless F % 8 == 0).  The coordinate grid is constant
                          * for a whole run and the kernel rounds it to its operand format anyway: given the copy, both input
                          * halves are loaded as 16-bit rows (no widening to fp32 / re-rounding per tile, a third of the input
                          * registers).  The rounding of the inputs is the same with and without it.                 */
  int32_t pe_grid_dims;  /* 0: pe / dpe are [G][P][E].  1..3 (16-bit kernels): the rows are the PATCHES of stitched grids, as the
                          * reference's patched presets build them (utils.py:60-116: the latent grids of a datapoint's patches
                          * are stitched, upsampled together and cut back into patches): pe / dpe are the upsampling net's own
                          * channel-last output [S * n_datapoints][G_0]..[G_d-1][E], G_i = pe_patch_nums[i] * pe_patch_size[i];
                          * row g = n * S + s is patch n % prod(patch_nums) (row-major) of datapoint n / prod(patch_nums) in
                          * image s * n_datapoints + datapoint, its pixel p the row-major position inside the patch.  Saves
                          * the cut-back copy of pe and the stitching copy of dpe; results are bit-identical          */
  int32_t pe_patch_nums[3];  /* patches per axis (first pe_grid_dims entries)                                          */
  int32_t pe_patch_size[3];  /* pixels per axis of one patch; their product is n_pix                                   */
  int64_t dw_bf16_stride;    /* elements between the rows of dw_bf16 (>= the length of a row of layer vectors)         */
  int32_t hidden_dims[4];    /* all zero: every hidden layer is `hidden` wide.  Otherwise (n_hidden <= 4) the widths of the
                              * n_hidden hidden layers one by one (the reference builds its INR from any list, prior_model.py:84-85): fp32
                              * mode only (1 .. 64 each; the plain-FMA parity kernel), `hidden` = their maximum            */
  void* dw_lo;               /* nullable, with dw_bf16 (the HIGH plane): the LOW plane bf16(dwvec - dw_bf16), same layout and
                              * stride.  The pair is the plane operand of the A transform's data gradient (rcb_atrans_apply
                              * x_hi / x_lo): the same 4 bytes per element as the fp32 dwvec, which may then be NULL in
                              * rcb_siren_bwd / _loss_bwd (unchunked launches) and rcb_siren_reduce_chunks                */
  uint64_t* clock_probe;     /* nullable measurement aid (width-32 16-bit kernel; refused at widths 16 / 24): workgroup b < 256 writes clock_probe[4 b ..
                              * 4 b + 3] = {s_memtime, s_memrealtime at its start, s_memtime, s_memrealtime at its end}.  Both
                              * counters are read on the workgroup's own CU (s_memtime is not comparable between CUs), so
                              * (t2 - t0) / ((t3 - t1) / 1e8) is the SHADER CLOCK that workgroup ran at (s_memrealtime counts
                              * 100 MHz): the figure an issue-bound kernel's roofline is priced at -- MI355X lowers its clock
                              * under matrix / vector load, peak-clock rooflines overstate what such kernels can reach      */
} rcb_siren_desc;

/* Test hook: which kernel family runs the width-32 bf16 loss / backward launches whose inputs arrive as 16-bit rows (pe_bf16,
 * xf_bf16, [G][P][E] pe, rows of whole 32-pixel tiles): 1 (default) -> one WAVE per row (siren_mlp_wave.hip: 221 vs 236 us per
 * launch at BASELINE configs[1] size) where the rows fill the resident waves to 90 % in the last round, else -- and for
 * everything that family has no instance for -- one workgroup per row (siren_mlp_bf16.hip); 2 -> the wave family whatever
 * the number of rows (tests); 0 -> the workgroup family everywhere; < 0 only queries.  Returns the previous setting.  Both
 * families evaluate the same products with fp32 accumulation; they differ in the order in which the pixel tiles of a row are
 * summed and in how the bias enters the accumulator (fp32 value / two bf16 halves through the matrix pipe). */
int rcb_debug_siren_wave_tiles(int32_t tiles);

/* y_out[G, P, C] = MLP(x)                                                           */
int rcb_siren_fwd(const rcb_siren_desc* d, const float* xf, const void* pe, const float* wvec,
                  float* y_out, rcb_stream_t stream);

/* Given dy[G, P, C]: dwvec[G, :] (same layout/stride as wvec) and, if dpe != NULL, dpe[G, P, E].
 * The forward pass is recomputed in registers; no activations are read from memory.            */
int rcb_siren_bwd(const rcb_siren_desc* d, const float* xf, const void* pe, const float* wvec,
                  const float* dy, float* dwvec, void* dpe, rcb_stream_t stream);

/* Sum of the per-chunk partials of a pixel_chunks = c launch, in chunk order (deterministic): dwvec[g, :] = sum_k
 * dw_partial[k][g][:], sse[g] = sum_k sse_partial[k][g] (sse_partial / sse may be NULL for rcb_siren_bwd), and, if
 * d->dw_bf16 != NULL, the bf16 copy of the sums as rcb_siren_desc.dw_bf16 describes.                              */
int rcb_siren_reduce_chunks(const rcb_siren_desc* d, const float* dw_partial, const float* sse_partial, float* dwvec,
                            float* sse, rcb_stream_t stream);

/* Fused training pass: sse[g] = sum_{p,c} (y - target[g/S])^2 and the gradients of
 * dy_scale * sse[g] with respect to wvec row g and pe row g (dpe may be NULL).  With
 * dy_scale = 1/(S*P*C) this is the reference's `mean((y_hat - y)**2) * N` term.              */
int rcb_siren_loss_bwd(const rcb_siren_desc* d, const float* xf, const void* pe,
                       const float* wvec, const float* target, float dy_scale, float* sse,
                       float* dwvec, void* dpe, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K1 + K10: reparameterised sampling of the latent vector of every (INR, sample) from a 1- or
 * 3-level factorised Gaussian posterior.  Replaces utils.py:142-198, prior_model.py:140-145 and
 * the mask/permutation gathers test_model.py:289-298,320-330.
 *
 *   out[n, s, d] = sum_levels  mu_L(n, d) + sigma_L(n, d) * eps_L[n, s, d]
 *   mu    = loc * (1 - m) + enc_sample * m          sigma = softplus(log_scale)/6 * (1 - m) + 1e-15 * m
 * evaluated at source element (r, j):  j = col_map ? col_map[d] : d;  r0 = row_map ? row_map[n] : n;
 * r = row_perm ? row_perm[r0 * cols + j] : r0.  A level contributes to d < cols_out only.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  const float* loc;        /* [rows, cols]                                          */
  const float* log_scale;  /* [rows, cols]                                          */
  const float* enc_sample; /* nullable [rows, cols]                                 */
  const float* enc_mask;   /* nullable [rows, cols] (0/1)                           */
  const int32_t* row_map;  /* nullable [N]                                          */
  const int32_t* row_perm; /* nullable [rows, cols]                                 */
  const int32_t* col_map;  /* nullable [cols_out]                                   */
  const float* eps;        /* [N, S, cols_out]                                      */
  int32_t rows, cols, cols_out;
  int32_t scale_is_sigma;  /* 0: `log_scale` holds log-scales, sigma = softplus(.)/6 (the models' parameters).  1: it holds
                            * sigma itself -- the argument convention of utils.py:122-137, whose callers apply st() and the
                            * encoded-group masks first (prior_model.py:140-145, test_model.py:289-298); generic kernel only */
  float* mu_sigma_ws;      /* nullable scratch [2 * rows * cols]: gathered levels (col_map / row_perm) first pack the effective
                            * (mu, sigma) of every element as one 8-byte record there, contiguously; the sampler then gathers one
                            * record per level and element instead of up to four 4-byte values -- same samples bit for bit   */
} rcb_level;

int rcb_reparam_fwd(const rcb_level* levels, int32_t n_levels, int32_t n_inr, int32_t samples,
                    int32_t out_cols, float* out, rcb_stream_t stream);

/* Noise drawn in the kernel (prior_model.py:140-145 draws torch.randn_like and then forms loc + st(log_scale) * eps):
 * eps[i] ~ N(0,1) from Philox4x32-10 + Box-Muller, a pure function of (seed, rng_stream, step, i), where `step` is read
 * from device memory so that a replayed HIP graph draws fresh noise.  rcb_reparam_rng_fwd: plain case (one level, one
 * sample, no maps), flat over n = rows * cols elements; writes eps_out (for rcb_posterior_bwd; nullable: a consumer with
 * rcb_level_bwd.eps_from_rng re-draws it) and out, and, if out_bf16 != NULL, a bf16 copy of out as [n / cols][ld_bf16] rows
 * (the operand of the A transform's batched bf16 weight-gradient GEMM, written while the values are in registers); with
 * out_lo != NULL also the low plane bf16(out - out_bf16) in the same layout: (out_bf16, out_lo) are the plane operands of
 * rcb_atrans_apply, and `out` may then be NULL.
 * rcb_philox_normal materialises the same stream (step from step_dev if non-NULL, else step_host).
 * group_offset: element i draws from Philox group i / 4 + group_offset.  A launch over rows [r0, r0 + m) of a larger
 * [rows, cols] array with group_offset = r0 * cols / 4 (r0 * cols a multiple of 4) draws exactly the noise those rows get in
 * a launch over the whole array: a shard -- or a sub-batch -- sees the noise of the unsharded run.                  */
/* rcb_reparam_hier_rng_fwd: the training sample of the patched presets (utils.py:122-198: level 1 one row per INR, the coarser
 * levels behind row maps; one sample, every column produced, no masks / permutations) with the noise of every level drawn in
 * the kernel: level l uses rng stream rng_streams[l] (host array) with the element index n * cols + d of the [n_inr, cols] noise
 * array -- the indexing of rcb_reparam_rng_fwd, so level 1 on stream s draws what that call draws -- and the noise is written
 * to eps_out[l] (host array of device pointers, [n_inr * cols] each) for rcb_posterior_bwd.  rcb_level.eps is ignored.  Same
 * arithmetic and order as rcb_reparam_fwd on that noise: bit-identical.  n_inr * cols must be a multiple of 4.              */
int rcb_reparam_hier_rng_fwd(const rcb_level* levels, int32_t n_levels, int32_t n_inr, int32_t out_cols, float* const* eps_out,
                             float* out, uint64_t seed, const uint32_t* rng_streams, const int64_t* step_dev,
                             uint64_t group_offset, rcb_stream_t stream);
int rcb_philox_normal(float* out, int64_t n, uint64_t seed, uint32_t rng_stream, const int64_t* step_dev, int64_t step_host,
                      uint64_t group_offset, rcb_stream_t stream);
int rcb_reparam_rng_fwd(const float* loc, const float* log_scale, int64_t n, uint64_t seed, uint32_t rng_stream,
                        const int64_t* step_dev, float* eps_out, float* out, void* out_bf16, void* out_lo, int32_t cols,
                        int64_t ld_bf16, uint64_t group_offset, rcb_stream_t stream);


/* ---------------------------------------------------------------------------------------------
 * K5 + K6 + K7: KL( N(loc, softplus(log_scale)/6) || N(p_loc, p_scale) ) per element
 * (torch.distributions.kl._kl_normal_normal as used at prior_model.py:191-199, test_model.py:357-377,
 * 384-402), reduced per row and optionally per (row, group) segment.
 *   kl_row[r]      = sum_j w(r,j) * kl(r,j),  w = beta[r, group_idx[j]] if beta != NULL else 1
 *   kl_group[r,g]  = sum_{j in [seg_start[g], seg_end[g])} kl(r,j)        (unweighted, fp64)
 * p_scale_is_log: p_scale holds log-scales to be passed through softplus/6 (test_model.py:358).
 * ------------------------------------------------------------------------------------------- */
int rcb_gauss_kl(const float* loc, const float* log_scale, const float* p_loc, const float* p_scale,
                 int32_t p_scale_is_log, int32_t rows, int32_t cols, const float* beta,
                 const int32_t* group_idx, int32_t n_groups, const int32_t* seg_start,
                 const int32_t* seg_end, double* kl_row, double* kl_group, rcb_stream_t stream);

/* Per-parameter KL summed over rows: the statistic behind get_grouping (prior_model.py:264-271); q_scale holds sigma (or
 * log-scales if q_scale_is_log).  out_fx is int64 [cols + 1]: out_fx[j] = sum over the rows of every ELEMENT's KL rounded to
 * RCB_COLSUM_FX_SCALE units per nat (each element enters the integer grid on its own), accumulated as 64-bit integers:
 * the result does not depend on the order in which the workgroups (or, after an integer all-reduce, the ranks) contribute
 * nor on where the rows are cut into shards -- bitwise reproducible, sharded or not.  out_fx[cols] = number of elements
 * whose KL was NaN / Inf / >= 2^12 nats (counted, not summed; the caller turns a non-zero count into NaN).            */
#define RCB_COLSUM_FX_SCALE 1073741824.0        /* 2^30 */
int rcb_gauss_kl_colsum(const float* loc, const float* q_scale, int32_t q_scale_is_log, const float* p_loc,
                        const float* p_scale, int32_t rows, int32_t cols, int64_t* out_fx, rcb_stream_t stream);

/* K8: per-group beta annealing (test_model.py:404-413): groups above 16+upper bits get
 * beta *= (1+step), groups at or below 16-lower bits beta /= (1+step), clamp [0, 1e4]; encoded
 * groups (done != 0) keep their beta.                                                          */
int rcb_beta_update(const double* kl_group, float* beta, const uint8_t* done, int32_t rows,
                    int32_t n_groups, double bits, double upper, double lower, double step,
                    rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K1-bwd + K5-bwd + K11: one pass over a level's parameters that (a) gathers the gradient of the
 * sampled latents back to (loc, log_scale), (b) adds the analytic gradient of kl_weight * KL, and
 * (c) either writes the gradients (g_loc / g_log_scale != NULL) or applies one Adam step in place
 * (torch.optim.Adam defaults, prior_model.py:224-250, test_model.py:633-635).
 *
 * d_out[N, S, cols_out] is the gradient w.r.t. rcb_reparam_fwd's output.  Members of source row r0
 * (the INRs n with row_map[n] == r0) are member_idx[member_ptr[r0] .. member_ptr[r0+1]) (NULL =
 * identity).  row_perm_inv / col_inv are the inverse permutations of row_perm / col_map.
 * kl weight: kl_scalar * (beta ? beta[r, group_idx[j]] : 1).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  float lr, beta1, beta2, eps;
  int32_t step;            /* 1-based step count t                                  */
  const float* dyn_scalars;/* nullable device pair {lr/(1-beta1^t), sqrt(1-beta2^t)}: when set it overrides the
                              values derived from `step`, so a captured HIP graph can be replayed for every t   */
} rcb_adam_cfg;

typedef struct {
  float* loc;              /* [rows, cols] (updated in place when adam != NULL)     */
  float* log_scale;
  const float* enc_mask;   /* nullable                                              */
  const float* p_loc;      /* [cols]                                                */
  const float* p_scale;    /* [cols]                                                */
  int32_t p_scale_is_log;
  const float* beta;       /* nullable [rows, n_groups]                             */
  const int32_t* group_idx;/* nullable [cols]                                       */
  int32_t n_groups;
  float kl_scalar;
  const float* d_out;      /* [N, S, cols_out] ; nullable (KL-only)                 */
  const float* eps;        /* [N, S, cols_out]                                      */
  const int32_t* member_ptr;   /* nullable [rows+1]                                 */
  const int32_t* member_idx;   /* nullable                                          */
  const int32_t* row_perm_inv; /* nullable [rows, cols]                             */
  const int32_t* col_inv;      /* nullable [cols] : d of source column j            */
  int32_t rows, cols, cols_out, samples;
  float* g_loc;            /* nullable outputs [rows, cols]                         */
  float* g_log_scale;
  float* m_loc; float* v_loc; float* m_ls; float* v_ls;   /* Adam state            */
  int64_t* kl_accum;       /* nullable [RCB_KL_SLOTS], fixed point (RCB_KL_FX_SCALE units per nat, integer atomics: the sum does
                            * not depend on the order of the workgroups): partial sums of the unweighted elementwise KL (before the
                            * update) are atomically added to slots [0, RCB_KL_SLOTS - 1); their total is the KL.  The LAST slot
                            * counts workgroup sums that were NaN / Inf or beyond 2^30 nats (not representable): rcb_step_end
                            * logs NaN for such a step, as the reference's diverged run would                            */
  const float* kl_scalar_dev; /* nullable device scalar: the KL weight becomes kl_scalar * (*kl_scalar_dev), so a
                              captured graph can be replayed with a new beta (main_prior_training.py:144-154) */
  /* Optional (plain levels on the flat path only; next_out == NULL: off): the NEXT step's reparameterised sample drawn in
   * the same pass from the parameters just updated -- what rcb_reparam_rng_fwd would compute at step counter
   * *rng_step_dev + rng_step_add, bit for bit -- so that the sampling kernel of the next step (a second read of loc and
   * log_scale) disappears.  next_eps may alias eps: every element is read before it is written. */
  float* next_out;         /* nullable: [rows * cols] fp32 sample                                                */
  float* next_eps;         /* nullable: [rows * cols] the noise of that sample (read by the next step's call as `eps`;
                            * not needed when that call sets eps_from_rng)                                       */
  void* next_out_bf16;     /* nullable: bf16 copy of the sample as [rows][next_ld_bf16] -- the HIGH plane         */
  int64_t next_ld_bf16;
  uint64_t rng_seed;
  const int64_t* rng_step_dev;
  int64_t rng_step_add;
  uint32_t rng_stream;
  uint32_t eps_from_rng;   /* 1 (flat path, eps = NULL): this step's noise is not read from memory but re-drawn -- the noise
                            * of (rng_seed, rng_stream, counter *rng_step_dev + rng_step_add - 1), i.e. what the sampler of
                            * THIS step drew (rcb_reparam_rng_fwd at *rng_step_dev, or the previous call's next sample):
                            * the same bits, 8 bytes of traffic per element less                                  */
  uint64_t rng_group_offset; /* Philox group of element 0 (rcb_reparam_rng_fwd's group_offset), for the next sample and eps_from_rng */
  void* next_out_lo;       /* nullable, with next_out_bf16: the LOW plane bf16(sample - high plane), same layout.  With both
                            * planes next_out may be NULL: rcb_atrans_apply reads the planes (x_hi / x_lo)          */
  float* sample_sum_ws;    /* nullable scratch [2 * rows * cols_out]: levels without members, samples > 1 and col_inv (the
                            * test-time layout of level 1) first form their sums over the samples there, contiguously, and the
                            * update gathers two values per parameter instead of 2 * samples -- same results bit for bit  */
  const int32_t* col_map;  /* nullable [cols_out]: the map col_inv inverts (j = col_map[d]).  A performance hint only: with it
                            * (levels with members, every column produced) threads are indexed by d, the contiguous axis of
                            * d_out / eps, instead of by the parameter column -- same results bit for bit           */
} rcb_level_bwd;

int rcb_posterior_bwd(const rcb_level_bwd* lv, const rcb_adam_cfg* adam, rcb_stream_t stream);

/* K11: Adam on a flat fp32 array (shared mappings A / conv weights).                          */
int rcb_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, const rcb_adam_cfg* cfg,
                  rcb_stream_t stream);

/* The same update for a list of tensors in ONE launch (the optimiser step over the shared mappings,
 * main_prior_training.py / prior_model.py train(): torch.optim.Adam over linear_transform + upsample_net). */
#define RCB_ADAM_MAX_TENSORS 16
typedef struct {
  float* p;            /* parameters, updated in place */
  const float* g;      /* gradient                     */
  float* m;            /* exp_avg                      */
  float* v;            /* exp_avg_sq                   */
  int64_t n;           /* elements                     */
} rcb_adam_tensor;
int rcb_adam_multi(const rcb_adam_tensor* tensors, int32_t count, const rcb_adam_cfg* cfg, rcb_stream_t stream);

/* Test hook: on != 0 forces the generic kernels of rcb_reparam_fwd / rcb_posterior_bwd even where a specialised one
 * (flat 16-byte path, LDS-staged gather) applies; returns the previous setting.  The specialised kernels perform the
 * same operations in the same order, so both settings must give identical bits (tests/test_hip_kernels.py).     */
int rcb_debug_generic_kernels_only(int32_t on);

/* ---------------------------------------------------------------------------------------------
 * K2, hand-written: the A transform of all layer vectors in one launch per direction (atrans.hip).
 *   forward        wvec[:, lo_l:hi_l] = h_w[:, lo_l:hi_l] @ A[l]      prior_model.py:173-174, test_model.py:348-349
 *   data gradient  dh  [:, lo_l:hi_l] = dw [:, lo_l:hi_l] @ A[l]^T    (autograd of the line above)
 *   weight gradient dA[l] = h_w[:, lo_l:hi_l]^T @ dw[:, lo_l:hi_l]    (autograd; summed over the rows = INRs x samples)
 * Layer l is the square map A[l] [sizes[l], sizes[l]] (fp32, row-major); the layer vectors sit side by side in rows of
 * x / out (column offset of layer l = sizes[0] + ... + sizes[l-1], row strides ld_x / ld_out in elements, 4-byte
 * aligned rows suffice).  bf16 matrix cores with fp32 accumulation; the per-row operand is split x = hi + lo inside
 * the kernel, the mapping enters as bf16 (terms 2) or as hi + lo (terms 3: (hi + lo) A_hi + hi A_lo, ~2^-17 relative);
 * terms 1 = plain bf16 operands.  No atomics anywhere: results are bitwise reproducible.
 *
 * rcb_atrans_pack_elems : bf16 elements of the packed images of the mappings (4 planes: forward hi, gradient hi,
 *                         forward lo, gradient lo; each layer padded to a multiple of 32 both ways), < 0 on bad arguments
 * rcb_atrans_pack       : fp32 mappings -> packed images (once per step when they are trained); the lo planes only if want_lo
 * rcb_atrans_plan       : HOST: work decomposition for `rows` rows on n_cu compute units into plan[0 .. return value) (int32);
 *                         the caller keeps a 16-byte aligned device copy of all of it and the first RCB_ATRANS_PLAN_HEAD
 *                         entries on the host (plan[0] = workgroups, plan[2] = slices of the contraction: launches of few
 *                         rows cut it and add the partial sums in a fixed order) for rcb_atrans_apply
 * rcb_atrans_workspace_floats : fp32 elements of the workspace rcb_atrans_apply needs for that plan (0: none)
 *                         (plan = NULL with max_ints = 0: nothing is written, the return value is the number of ints needed;
 *                         a buffer that is too small is RCB_ERR_SHAPE, any other error RCB_ERR_ARG)
 * rcb_atrans_apply      : transpose = 0: out = x @ A (forward), 1: out = x @ A^T (data gradient).  The per-row operand comes
 *                         EITHER as fp32 rows `x` (x_hi = x_lo = NULL; split hi + lo inside the kernel) OR -- x = NULL -- as
 *                         the two bf16 PLANES its producer wrote: x_hi[r][c] = bf16(v), x_lo[r][c] = bf16(v - x_hi[r][c]),
 *                         rows ld_x16 elements apart (a multiple of 8; 32 = 64-byte rows stream best), same column layout.
 *                         The planes are the same 4 bytes per element as the fp32 row, carry exactly what the kernel would
 *                         have formed from it -- results are bit-identical -- and arrive in LDS as operand bits (no
 *                         conversion work); hi alone is the weight-gradient GEMM's operand.  Producers:
 *                         rcb_reparam_rng_fwd (out_bf16 + out_lo), rcb_level_bwd.next_out_bf16 + next_out_lo,
 *                         rcb_siren_desc.dw_bf16 + dw_lo.  x_lo may be NULL with terms = 1
 * rcb_atrans_wgrad_narrow : dA = h^T @ d for ONE narrow layer (the 99-wide output layer) in fp32, exact-product arithmetic,
 *                         fixed summation order; each operand EITHER as fp32 rows (h / d, pointing at the layer's first
 *                         column; the plane pointers NULL) OR as its (hi, lo) planes (h_hi, h_lo / d_hi, d_lo pointing at the
 *                         layer's first column, the fp32 pointer NULL; read as float(hi) + float(lo)); ld_h / ld_d = the row
 *                         stride in elements of whichever form is given; workspace: rcb_atrans_wgrad_narrow_workspace(L,
 *                         n_slabs) floats
 * ------------------------------------------------------------------------------------------- */
#define RCB_ATRANS_MAX_LAYERS 8
#define RCB_ATRANS_PLAN_HEAD 12
int64_t rcb_atrans_pack_elems(int32_t n_layers, const int32_t* sizes);
int rcb_atrans_pack(const float* const* A, int32_t n_layers, const int32_t* sizes, void* packed, int32_t want_lo,
                    rcb_stream_t stream);
int rcb_atrans_plan(int64_t rows, int32_t n_layers, const int32_t* sizes, int32_t n_cu, int32_t* plan, int32_t max_ints);
int rcb_atrans_apply(const float* x, int64_t ld_x, const void* x_hi, const void* x_lo, int64_t ld_x16, float* out,
                     int64_t ld_out, int64_t rows, int32_t n_layers, const int32_t* sizes, const void* packed, int32_t transpose,
                     int32_t terms, const int32_t* plan_dev, const int32_t* plan_head, float* workspace, rcb_stream_t stream);
int64_t rcb_atrans_workspace_floats(int64_t rows, int32_t n_layers, const int32_t* sizes, const int32_t* plan_head);
int64_t rcb_atrans_wgrad_narrow_workspace(int32_t L, int32_t n_slabs);
int rcb_atrans_wgrad_narrow(const float* h, const void* h_hi, const void* h_lo, int64_t ld_h, const float* d, const void* d_hi,
                            const void* d_lo, int64_t ld_d, int64_t rows, int32_t L, float* dA, float* workspace,
                            int32_t n_slabs, rcb_stream_t stream);

/* Bookkeeping of one optimisation step whose counter lives on the device, so that the whole step can be captured
 * once as a HIP graph and replayed (prior_model.py train() / test_model.py train() loop bodies):
 *   begin: dyn[0..1] = adam_table[step] ({lr / (1 - beta1^t), sqrt(1 - beta2^t)}, row clamped to the table);
 *          kl_slots[RCB_KL_SLOTS] = 0 (nullable)
 *   end  : mse_log[step] = mse_scale * sum(sse[0..n_sse)),  kl_log[step] = sum(kl_slots)  (each nullable, written
 *          only while step < n_log; fixed-order fp64 sums);  step += 1;  aux_counter (e.g. a noise counter that is not
 *          reset between train() calls) += 1                                                                        */
int rcb_step_begin(const float* adam_table, int64_t n_steps, const int64_t* step, float* dyn, int64_t* kl_slots,
                   rcb_stream_t stream);
int rcb_step_end(const float* sse, int32_t n_sse, double mse_scale, const int64_t* kl_slots, double* mse_log,
                 double* kl_log, int64_t n_log, int64_t* step, int64_t* aux_counter /* nullable: += 1 */,
                 rcb_stream_t stream);

/* Combined launches of a captured training step on one rank with the mappings trained (step_fused.hip).  Each is ONE
 * launch whose block ranges run the bodies of the separate entry points: every output is bit-identical to theirs.
 *   rcb_step_prepare = rcb_step_begin + rcb_atrans_pack + rcb_upconv_weff_build (arguments as theirs, in that order)
 *   rcb_step_tail    = rcb_posterior_bwd(lv, cfg) on its flat fast path + rcb_adam_multi(tensors, count, cfg) +
 *                      rcb_step_end(sse, n_sse, mse_scale, lv->kl_accum, mse_log, kl_log, n_log, step, aux_counter).
 *                      The log entry is written by the workgroup that finishes last; `tickets` are RCB_STEP_TAIL_TICKETS
 *                      device uint32 that are zero on entry and zero again on exit (zero-fill them once).  lv must satisfy rcb_step_tail_eligible (the conditions of
 *                      the flat fast path: plain level, one sample, Adam, 16-byte aligned arrays, rows * cols % 4 == 0),
 *                      else RCB_ERR_UNSUPPORTED: the caller issues the three launches.                              */
int rcb_step_prepare(const float* adam_table, int64_t n_steps, const int64_t* step, float* dyn, int64_t* kl_slots,
                     const float* const* A, int32_t n_layers, const int32_t* sizes, void* packed, int32_t want_lo,
                     const float* W1, const float* b1, const float* W2, const float* W3, void* weff1, void* b1rep,
                     int32_t bf16_out, float* weff2, float* weff3, void* frag_pack, rcb_stream_t stream);
#define RCB_STEP_TAIL_TICKETS 65
int rcb_step_tail_eligible(const rcb_level_bwd* lv);
int rcb_step_tail(const rcb_level_bwd* lv, const rcb_adam_cfg* cfg, const rcb_adam_tensor* tensors, int32_t count,
                  const float* sse, int32_t n_sse, double mse_scale, double* mse_log, double* kl_log, int64_t n_log,
                  int64_t* step, int64_t* aux_counter /* nullable: += 1 */, uint32_t* tickets, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K12: column moments for the closed-form prior refit (main_prior_training.py:157-172), as EXACT fixed-point sums.
 * For x = loc[rows, cols] and sigma = softplus(log_scale) / 6, every term v in {x, x^2, sigma^2} is split at 2^-30:
 * hi = floor(v 2^30), lo = rint((v 2^30 - hi) 2^32), and the parts are summed as 64-bit integers:
 * out_fx[q][0][j] = sum_r hi,  out_fx[q][1][j] = sum_r lo  for q = 0: x, 1: x^2, 2: sigma^2  (out_fx is int64
 * [3][2][cols] followed by ONE more element; value = (hi + lo 2^-32) 2^-30, resolution 2^-62).  Range: every term must
 * satisfy |v| < 2^12 -- i.e. |x| < 2^6 and sigma < 2^6, since x^2 and sigma^2 are terms -- for up to 2^20 rows over all
 * ranks (2^12 2^30 2^20 = 2^62).  Terms outside that range, NaN and Inf are not summed but counted in out_fx[6 cols]
 * (summed over ranks like the rest): a non-zero count means the refit must be NaN.  Integer addition is associative,
 * so the sums -- and the prior refit from them -- are bitwise independent of the order of the workgroups and, after an
 * integer all-reduce, of how the rows are sharded over ranks.  mean = sum x / n, M2 = sum x^2 - (sum x)^2 / n in fp64.
 * ------------------------------------------------------------------------------------------- */
#define RCB_MOM_FX_SCALE 1073741824.0            /* 2^30 */
#define RCB_MOM_FX_LO_SCALE 4294967296.0         /* 2^32 */
int rcb_col_moments(const float* loc, const float* log_scale, int32_t rows, int32_t cols, int64_t* out_fx,
                    rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K9: A* / relative-entropy-coding candidate scoring (test_model.py:501-533 sample_group, :535-584
 * h_/hh_ copies) and the commit of the chosen sample (test_model.py:586-619 compress_group), batched
 * over jobs.  Job b encodes columns [start[b], start[b]+glen[b]) of row row[b]:
 *   z_k    = p_loc + p_scale * xi_k                    (fp64: multiply, then add; xi = table of that group length)
 *   logw_k = sum_j logN(z_kj; loc, scale) - logN(z_kj; p_loc, p_scale) + gumbel[k]
 *   idx    = first argmax_k logw_k
 * loc/scale/p_loc/p_scale are fp32 (scale = softplus(log_scale)/6 precomputed by the caller).  Group lengths are
 * unbounded (the reference packs parameters until 16 bits of KL are reached, prior_model.py:301-316).
 * Candidate tables: the reference table (scrambled Sobol -> scipy norm.ppf, test_model.py:493-498) is fp32-precision
 * data in an fp64 container, so it is held as fp32, TRANSPOSED: tables_t[g] -> [g][K] (candidate index contiguous).
 * tables_t and table_absmax are DEVICE arrays of max_glen + 1 entries (NULL / 0 for unused lengths); the job arrays are
 * DEVICE arrays too, so an encode round needs no host round trip.  Jobs outside the matrix, with an unknown group
 * length or a missing table are rejected on the device: idx = -1, nothing committed.  A job all of whose scores are NaN
 * (a NaN in its posterior or prior row) has no arg-max: idx = -1 in both modes as well, best = (-inf, -inf), nothing
 * committed -- the caller sees the group as not coded; the reference's torch.argmax would code it at index 0.
 *
 * mode RCB_REC_EXACT: the reference arithmetic op for op (one workgroup per job).
 * mode RCB_REC_FAST : logw as a quadratic in xi (two fp64 FMAs per candidate and element, eight jobs share every table
 *   load), then a per-job certificate: if the gap between the two best fast scores exceeds a rigorous bound on
 *   |fast - exact| the exact arg-max is provably the same index; the remaining jobs (flagged in `uncertified`) are
 *   re-scored by the exact kernel inside the same call.  Indices are identical to RCB_REC_EXACT by construction.
 * Outputs: idx[n_jobs]; best[n_jobs, 2] (nullable) = (max, runner-up) log-weights; uncertified[n_jobs] (nullable);
 * logw_job0 (nullable, [K]) = all log-weights of job 0, always from the exact scorer.
 * `workspace`: rcb_rec_workspace_bytes(...) bytes, 16-byte aligned, caller-allocated.
 *
 * rcb_rec_commit: z = p_loc + p_scale * xi[idx] (fp64, mul then add) -> z_out[b, max_glen] (nullable, fp64),
 * enc_sample[row, start + j] = (float) z, enc_mask[row, start + j] = 1, and per (row, group = job_group[b]):
 * done = 1, beta = 0, idx_groupwise = idx  (each nullable).  The decoder rebuilds its samples with the same kernel.
 * ------------------------------------------------------------------------------------------- */
#define RCB_REC_EXACT 0
#define RCB_REC_FAST 1

typedef struct rcb_rec_desc {
  const float* loc;            /* [rows, cols] posterior means (group order)          (nullable for rcb_rec_commit) */
  const float* scale;          /* [rows, cols] posterior standard deviations           (nullable for rcb_rec_commit) */
  const float* p_loc;          /* [cols] */
  const float* p_scale;        /* [cols] */
  int32_t rows, cols;
  const float* const* tables_t; /* device array [max_glen + 1] of device pointers to fp32 [g][K] tables */
  const double* table_absmax;  /* device array [max_glen + 1]: max |xi| of each table  (nullable for rcb_rec_commit) */
  int32_t max_glen;
  const double* gumbel;        /* [K] fp64 (test_model.py:441-457)                      (nullable for rcb_rec_commit) */
  double gumbel_absmax;
  int32_t n_candidates;        /* K */
  const int32_t* job_row;      /* device arrays [n_jobs]; sorting the jobs by glen lets eight jobs share table loads */
  const int32_t* job_start;
  const int32_t* job_glen;
  int32_t n_jobs;
} rcb_rec_desc;

int64_t rcb_rec_workspace_bytes(int32_t n_jobs, int32_t max_glen, int32_t n_candidates);
int rcb_rec_score_argmax(const rcb_rec_desc* desc, int32_t mode, void* workspace, int64_t workspace_bytes, int32_t* idx,
                         double* best, uint8_t* uncertified, double* logw_job0, rcb_stream_t stream);
int rcb_rec_commit(const rcb_rec_desc* desc, const int32_t* idx, const int32_t* job_group, int32_t n_groups,
                   double* z_out, float* enc_sample, float* enc_mask, uint8_t* done, float* beta,
                   int32_t* idx_groupwise, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N1: the `nearest-upsample(2) -> conv3x3(pad 1)` stages of the upsampling net (prior_model.py:52-54:
 * up2/conv2/act2, up3/conv3) in sub-pixel (phase) form, bf16 MFMA / fp32 accumulate, channel-last images,
 * Cin = 64.  weff = kernel taps pre-summed per (phase, 2x2 window tap), fp32 [ty][tx][ci][a][b][co].
 *   fwd  : y[b, 2i+a, 2j+b', co] = bias[co] + sum weff[ty,tx,ci,a,b',co] * x[b, i+a+ty-1, j+b'+tx-1, ci]
 *          x: bf16 activations (x_is_f32_preact = 0), fp32 pre-activations (1) or bf16 pre-activations (2);
 *             LeakyReLU(0.01) is applied on load to pre-activations;
 *          y: bf16 with LeakyReLU applied (y_is_f32_linear = 0), fp32 linear output (1) or bf16 linear output (2).
 *   dgrad: dx = (conv^T dy) * LeakyReLU'(x)   (sign taken from the stored activation / pre-activation)
 *   wgrad: dweff = sum_b,i,j x (x) dy    (per-workgroup partial sums + fixed-order reduction)
 * Instantiated for (grid, cout) = (8, 64) [stage 2: fp32 or bf16 pre-activation in, bf16 out] and (16, 16)
 * [stage 3: bf16 in, fp32 or bf16 linear out; dy fp32 or bf16]; batch = number of images (INR x sample).
 * ------------------------------------------------------------------------------------------- */
int rcb_upconv_fwd(const void* x, int32_t x_is_f32_preact, const float* weff, const float* bias, void* y,
                   int32_t y_is_f32_linear, int32_t batch, int32_t grid, int32_t cout, const void* frag_pack,
                   rcb_stream_t stream);
/* dgrad, stage-2 geometry only: if dbias_partial != NULL it receives [rcb_upconv_dgrad_partial_rows(batch)][64]
 * per-workgroup channel sums of dx (= the bias gradient of the stage that produced x); elsewhere it must be NULL. */
int32_t rcb_upconv_dgrad_partial_rows(int32_t batch);
int rcb_upconv_dgrad(const void* dy, int32_t dy_is_f32, const float* weff, const void* x, int32_t x_is_f32_preact,
                     void* dx, float* dbias_partial, int32_t batch, int32_t grid, int32_t cout, const void* frag_pack,
                     rcb_stream_t stream);
/* wgrad writes (does not accumulate) dweff [2][2][64][2][2][cout] and, if non-NULL, dbias [cout] = sum of dy.
 * Each workgroup sums its INRs into its own slab of `workspace` and a second kernel adds the slabs in a fixed
 * order: no atomics, bitwise reproducible.  workspace: >= rcb_upconv_wgrad_workspace(batch, cout) floats.   */
int64_t rcb_upconv_wgrad_workspace(int32_t batch, int32_t cout);
int rcb_upconv_wgrad(const void* x, int32_t x_is_f32_preact, const void* dy, int32_t dy_is_f32, float* dweff,
                     float* dbias, int32_t batch, int32_t grid, int32_t cout, float* workspace,
                     int64_t workspace_floats, rcb_stream_t stream);
/* Stage-3 geometry (grid 16, cout 16, bf16 tensors): dgrad and wgrad of one stage in ONE pass over dy and x (each is
 * read once instead of twice).  dx as rcb_upconv_dgrad, dweff / dbias as rcb_upconv_wgrad (same workspace).          */
int rcb_upconv_bwd_fused(const void* dy, const float* weff, const void* x, void* dx, float* dweff, float* dbias,
                         int32_t batch, int32_t grid, int32_t cout, float* workspace, int64_t workspace_floats,
                         const void* frag_pack, rcb_stream_t stream);
/* 408: stages 2 and 3 of the CIFAR geometry forward in ONE launch: z1 [batch][8][8][64] -> h2 [batch][16][16][64] (bf16,
 * LeakyReLU applied; the backward reads it) and pe [batch][32][32][16] (bf16, linear), bit-identical to
 * rcb_upconv_fwd(grid 8, cout 64) followed by rcb_upconv_fwd(grid 16, cout 16): stage 3 reads every h2 image from LDS,
 * where stage 2 has just put it, instead of from HBM.  Only z1_is_f32_preact = 2 (bf16 pre-activation),
 * pe_is_f32_linear = 2 (bf16 linear) and a non-NULL frag_pack exist; every other combination, and a process started with
 * RCB_UPCONV_HALF_WG=1, returns RCB_ERR_UNSUPPORTED without launching anything (the caller runs the two launches).  The library
 * reads no switch of its own: RCB_UPCONV_FWD_FUSED=0 is the Python callers' (a field of their step plans) and makes them
 * keep the two launches.                                                                                              */
int rcb_upconv_fwd23(const void* z1, int32_t z1_is_f32_preact, const float* b2, const float* b3, void* h2, void* pe,
                     int32_t pe_is_f32_linear, int32_t batch, const void* frag_pack, rcb_stream_t stream);

/* The phase-form ("effective") weights of the CIFAR-geometry upsampling net from its conv weights, and the
 * transposed map for their gradients (one launch each; prior_model.py:39-57 defines the convolutions):
 *   weff1 [512][4096] (rows (s,t,i) of the 2x2x128 latent grid, columns (y,x,o) of the 8x8x64 stage-1 output) and
 *   b1rep [4096] in bf16 (bf16_out = 1) or fp32; weff2 [2][2][64][2][2][64], weff3 [2][2][64][2][2][16] fp32.
 *   grad: dW1 [64][128][5][5], dW2 [64][64][3][3], dW3 [16][64][3][3] written (not accumulated).               */
/* frag_pack (nullable, RCB_UPCONV_PACK_UINT4 x 16 bytes): the same effective weights as bf16 MFMA A-fragments in the
 * per-lane order the phase-conv kernels keep in registers, so that their prologue is a few coalesced 16-byte loads
 * instead of hundreds of strided scalar ones.  16-byte entries (8 bf16), lane = entry & 63, q = lane & 31, h = lane >> 5:
 *   [    0,  8192) stage-2 forward   [ph][mt][ty][tx][kb][lane]: weff2[ty][tx][16kb+8h+j][ph>>1][ph&1][32mt+q]
 *   [ 8192, 16384) stage-2 dgrad     [kh][mt][c][kb][lane], window combo n = 8kh+c: weff2[ty][tx][32mt+q][pa][pb][16kb+8h+j]
 *   [16384, 18432) stage-3 forward   [pa][pb][ty][tx][kb2][lane], A operands of v_mfma_f32_16x16x32_bf16:
 *                                    weff3[ty][tx][32kb2+8(lane>>4)+j][pa][pb][lane&15]; [18432, 20480) unused
 *   [20480, 22528) stage-3 dgrad     [n][mt][lane]: weff3[ty][tx][32mt+q][pa][pb][8h+j]
 * (ry = (n>>2)-1, rx = (n&3)-1, pa = ry&1, ty = ry<=0, pb = rx&1, tx = rx<=0.)  rcb_upconv_fwd / _dgrad take the pack
 * through their `frag_pack` argument; with NULL they build the fragments from `weff` themselves.                 */
#define RCB_UPCONV_PACK_UINT4 22528
int rcb_upconv_weff_build(const float* W1, const float* b1, const float* W2, const float* W3, void* weff1, void* b1rep,
                          int32_t bf16_out, float* weff2, float* weff3, void* frag_pack, rcb_stream_t stream);
int rcb_upconv_weff_grad(const void* dweff1, int32_t bf16_in, const float* dweff2, const float* dweff3, float* dW1,
                         float* dW2, float* dW3, const float* db1_partial /* nullable [n_partial][64] */,
                         int32_t n_partial, float* db1 /* nullable [64] = column sums of db1_partial */,
                         rcb_stream_t stream);

/* ---- overlapping tiles of a stitched grid (N1 for the patched presets; utils.py:71-116 stitches the patches of a
 * datapoint into one latent grid before the upsampling net, prior_model.py:52-54) ------------------------------------
 * The phase-conv kernels above work on small zero-halo images.  A large channel-last bf16 image [n][H][W][C] (C % 8 == 0)
 * is cut into tiles [n][Ty][Tx][T][T][C]; tile (ty, tx) holds pixels ty*step - off .. + T-1  x  tx*step - off .. + T-1.
 *   rcb_tile_gather: image -> tiles, zero outside the image and, with ring = 1, on the outermost row / column of each tile.
 *                    Source tiles of an upconv stage with grid G: T = G, step = G-1, off = 1, ring = 0 (tiles overlap by
 *                    one source pixel, so all but the outermost of a tile's 2G output rows see their whole window);
 *                    tiles of the upstream gradient: T = 2G, step = 2G-2, off = 2, ring = 1.
 *   rcb_tile_crop  : tiles -> image [n][H][W][C] from the inner T-2 rows / columns of every tile (step = T-2):
 *                    pixel y comes from tile (y+off) / (T-2), row (y+off) % (T-2) + 1.  Stage outputs: T = 2G, off = 1.
 *   rcb_tile_fold  : tiles -> image, the SUM of all tile elements that map to a pixel (step = T-1; adjoint of the ring-0
 *                    gather: border pixels belong to two tiles per axis); fp32 sum in a fixed order, rounded once to bf16.
 * Pure data movement (HBM-bound: bytes = image + tiles).                                                               */
int rcb_tile_gather(const void* img, void* tiles, int32_t n, int32_t H, int32_t W, int32_t C, int32_t Ty, int32_t Tx,
                    int32_t T, int32_t step, int32_t off, int32_t ring, rcb_stream_t stream);
int rcb_tile_crop(const void* tiles, void* img, int32_t n, int32_t H, int32_t W, int32_t C, int32_t Ty, int32_t Tx,
                  int32_t T, int32_t off, rcb_stream_t stream);
int rcb_tile_fold(const void* tiles, void* img, int32_t n, int32_t H, int32_t W, int32_t C, int32_t Ty, int32_t Tx,
                  int32_t T, int32_t off, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N1, grids of any dimension (nd = 1 audio / protein, 3 video; 2 is valid too): the `nearest-upsample(2) -> conv(3, pad 1)`
 * stages of the upsampling net (prior_model.py:52-54 with Conv1d / Conv3d) as direct sub-pixel convolutions on bf16 MFMA,
 * channel-last bf16 tensors, Cin = 64, Cout = 64 or 16 -- no window matrix.  x [B][g0][g1][g2][64] (axes k >= nd of
 * size 1), y [B][2 g...][Cout] (active axes doubled).
 *   rcb_phaseconv_pack : conv weight [Cout][64][3]^nd fp32 -> bf16 MFMA fragments of the pre-summed phase weights for the
 *                        forward and / or the data-gradient kernel (rcb_phaseconv_pack_uint4(nd, cout, which) 16-byte
 *                        units each; which 0 = forward, 1 = data gradient; either pointer may be NULL)
 *   rcb_phaseconv_fwd  : y = bias + sum over the 2^nd source taps of every phase (+ LeakyReLU(0.01) if leaky_out);
 *                        x holds ACTIVATIONS (post-LeakyReLU: the producer applies it)
 *   rcb_phaseconv_dgrad: dx = LeakyReLU'(x_act) * (transposed stage applied to dy [B][2 g...][Cout]); x_act = the stored
 *                        activations of the stage input (sign = derivative; NULL: no factor)
 *   rcb_phaseconv_wgrad: dW [Cout][64][3]^nd and dbias [Cout] (fp32) from the stage input activations and the gradient of
 *                        its linear output: contraction over all positions with both MFMA operands read transposed from
 *                        LDS images; per-workgroup fp32 slabs added in a fixed order (no atomics); `workspace`:
 *                        rcb_phaseconv_wgrad_workspace(nd, cout) floats, caller-allocated                              */
int64_t rcb_phaseconv_pack_uint4(int32_t nd, int32_t cout, int32_t which);
int rcb_phaseconv_pack(const float* conv_weight, int32_t nd, int32_t cout, void* fwd_frags, void* dgrad_frags,
                       rcb_stream_t stream);
int rcb_phaseconv_fwd(const void* x, const void* fwd_frags, const float* bias, void* y, int32_t B, int32_t g0, int32_t g1,
                      int32_t g2, int32_t nd, int32_t cout, int32_t leaky_out, rcb_stream_t stream);
int rcb_phaseconv_dgrad(const void* dy, const void* dgrad_frags, const void* x_act, void* dx, int32_t B, int32_t g0,
                        int32_t g1, int32_t g2, int32_t nd, int32_t cout, rcb_stream_t stream);
int64_t rcb_phaseconv_wgrad_workspace(int32_t nd, int32_t cout);
int rcb_phaseconv_wgrad(const void* x_act, const void* dy, float* dW, float* dbias, float* workspace, int64_t workspace_floats,
                        int32_t B, int32_t g0, int32_t g1, int32_t g2, int32_t nd, int32_t cout, rcb_stream_t stream);

/* Stage 1 of the 1-D upsampling net, direct (prior_model.py:23-51 with Conv1d: up1 (x4) -> conv1 (128 -> 64, k 5, pad 2) ->
 * act1; audio / protein presets): replaces the window-GEMM form (rcb_window_gather -> library GEMM -> LeakyReLU pass, and its
 * backward GEMMs / rcb_window_fold / casts) for nd = 1.  wbig = rcb_phase_bigweight's result for the stage, bf16 [3 * 128][4 * 64]
 * (row = tap * 128 + ci, column = phase * 64 + co; only two taps per phase are non-zero and only those are read).
 *   rcb_stage1_1d_fwd  : x [B][g][128] fp32 (rounded to bf16 as the operand) -> x1 [B][4 g][64] bf16 = LeakyReLU(bf16(bias + conv))
 *   rcb_stage1_1d_dgrad: dz [B][4 g][64] bf16 (gradient of the PRE-activation, as rcb_phaseconv_dgrad of stage 2 returns it)
 *                        -> dx [B][g][128] fp32
 *   rcb_stage1_1d_wgrad: -> dwbig [384][256] fp32 (zero where no phase reads; rcb_phase_bigweight_grad maps it onto the conv
 *                        weight) and dbias [64] fp32; per-workgroup slabs added in a fixed order (no atomics); `workspace`:
 *                        rcb_stage1_1d_wgrad_workspace() floats, caller-allocated.  All tensors 16-byte aligned.             */
int rcb_stage1_1d_fwd(const float* x, const void* wbig, const float* bias, void* x1, int32_t B, int32_t g, rcb_stream_t stream);
int rcb_stage1_1d_dgrad(const void* dz, const void* wbig, float* dx, int32_t B, int32_t g, rcb_stream_t stream);
int64_t rcb_stage1_1d_wgrad_workspace(void);
int rcb_stage1_1d_wgrad(const float* x, const void* dz, float* dwbig, float* dbias, float* workspace, int64_t workspace_floats,
                        int32_t B, int32_t g, rcb_stream_t stream);

/* 3^d-pixel windows of a channel-last bf16 grid x [B][g0][g1][g2][C] (nd = 1..3 windowed axes, unused trailing axes of size 1,
 * C % 8 == 0): the operand of the one-GEMM-per-stage phase form of the 1-D / 3-D upsampling nets (prior_model.py:23-59 with
 * Conv1d / Conv3d; every phase of the reference's stages reads inside the 3-pixel window around its source pixel).
 *   rcb_window_gather: cols [B*g0*g1*g2][3^nd][C], cols[b,p,k,:] = x[b, p + o(k) - 1, :] (0 outside), o(k) = base-3 digits of k
 *                      (axis 0 most significant).
 *   rcb_window_fold  : dx[b,p,:] = sum_k dcols[b, p - o(k) + 1, k, :] (the adjoint), fp32 sum in tap order, rounded to bf16. */
int rcb_window_gather(const void* x, void* cols, int32_t B, int32_t g0, int32_t g1, int32_t g2, int32_t C, int32_t nd,
                      rcb_stream_t stream);
int rcb_window_fold(const void* dcols, void* dx, int32_t B, int32_t g0, int32_t g1, int32_t g2, int32_t C, int32_t nd,
                    rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The window-GEMM weight of a  nearest-upsample(f) -> conv(k, pad)  stage (reference prior_model.py:23-59: up1 + conv1 of the
 * upsampling net, evaluated on the 1-D / 3-D and stitched 2-D grids as one GEMM over 3^d-pixel windows, all phases at once):
 *   Wbig[(n_0..n_d-1, ci), (a_0..a_d-1, co)] = sum of W[co][ci][kk] over the taps kk with floor((a_i + kk_i - pad) / f_i) + 1 == n_i
 * rcb_phase_bigweight: `wt` = the conv weight in channel-last order [k^nd][cin][cout] (fp32) -> big [3^nd * cin][prod(f) * cout],
 * bf16 (out_bf16 = 1) or fp32.  rcb_phase_bigweight_grad: its adjoint, dbig (bf16 or fp32) -> dwt [k^nd][cin][cout] fp32.
 * `f` holds nd upsampling factors (<= 8); k <= 8; every phase must stay inside the 3-pixel window (all reference stages do). */
int rcb_phase_bigweight(const float* wt, void* big, int32_t out_bf16, int32_t nd, const int32_t* f, int32_t k, int32_t pad,
                        int32_t cin, int32_t cout, rcb_stream_t stream);
int rcb_phase_bigweight_grad(const void* dbig, int32_t in_bf16, float* dwt, int32_t nd, const int32_t* f, int32_t k, int32_t pad,
                             int32_t cin, int32_t cout, rcb_stream_t stream);

/* sigma = softplus(log_scale)/6 elementwise (prior_model.py:88).                                */
int rcb_softplus_scale(const float* log_scale, float* scale, int64_t n, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4 (409): the decoder's last step and the distortion figure.  Replaces utils.py:200-260 (clip, x 255, np.round, / 255 and the
 * squared-error mean, in numpy on a host copy of the whole reconstruction) and its caller main_compression.py:154-167.
 * y [n_rows][n_pix][channels] fp32, 1 <= channels <= 32.  nd = 0: every row is a datapoint.  nd = 1..3: the rows are the PATCHES
 * of stitched signals, addressed as rcb_siren_desc.pe_grid_dims addresses them: row n is patch n % prod(patch_nums) (row-major)
 * of datapoint n / prod(patch_nums), its pixel p the row-major position inside the patch; prod(patch_size) = n_pix and n_rows is
 * a multiple of prod(patch_nums).  patch_nums / patch_size: HOST arrays of nd entries (ignored for nd = 0).
 * n_data = n_rows / prod(patch_nums) (n_rows for nd = 0).  `target`: nullable, the layout of y.
 *   mode 0 (8-bit): q = rintf(fminf(fmaxf(x, 0), 1) * 255.0f) -- an fp32 multiply, half to even as np.round -- and
 *                   v = (float)q / 255.0f, an IEEE fp32 division as numpy's;  mode 1 (raw: audio, protein): v = x.
 * Outputs, each nullable:
 *   u8    [n_data][G_0]..[G_nd-1][channels] uint8, G_i = patch_nums[i] * patch_size[i] ([n_rows][n_pix][channels] for nd = 0): q,
 *         mode 0 only; a NaN x gives 0
 *   whole the same stitched layout, fp32: v, either mode
 *   sse   [n_data] fp64: the sum over the datapoint's elements of (double)d * (double)d, d = t - v as an fp32 subtraction (what
 *         numpy forms elementwise); needs `target`
 *   n_bad [n_data] int32: the elements whose x or t is not finite (an element with both counts twice).  A datapoint with any has
 *         sse = NaN; no other datapoint is touched.
 * The sum uses no floating-point atomics: which elements a workgroup adds and the order of every addition depend on the geometry
 * of ONE datapoint alone, so a datapoint's sse is bitwise the same alone and inside any batch, and from run to run.
 * `workspace`: rcb_recon_workspace_bytes(n_data, elements per datapoint) bytes (-1: shape refused), 8-byte aligned,
 * caller-allocated.  Refused (RCB_ERR_*): nd > 3, channels out of range, n_pix != prod(patch_size), n_rows no multiple of
 * prod(patch_nums), u8 with mode 1, sse without target, more than 2^31 - 1 elements per datapoint, a workspace that is too small. */
int64_t rcb_recon_workspace_bytes(int64_t n_data, int64_t elems_per_datapoint);
int rcb_recon_finish(const float* y, const float* target, int64_t n_rows, int32_t n_pix, int32_t channels, int32_t nd,
                     const int32_t* patch_nums, const int32_t* patch_size, int32_t mode, uint8_t* u8, float* whole, double* sse,
                     int32_t* n_bad, void* workspace, int64_t workspace_bytes, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4 (410): the encoder's first step, whole signals -> the patch targets y.  Replaces data/image.py:30-46, data/video.py:54-73 and
 * data/audio.py:125-140 (a host loop of slices per patch, each flattened by utils.py:287-298) and the / 255 of ToTensor
 * (data/image.py:17) and of data/video.py:31.
 * `src` addresses n_data signals on the grid G_i = patch_nums[i] * patch_size[i], nd = 1..3, 1 <= channels <= 32: element
 * (d, g_0 .. g_nd-1, c) lies at src + d * data_stride + sum g_i * axis_stride[i] + c * channel_stride.  Strides are in ELEMENTS and
 * >= 0; patch_nums / patch_size / axis_stride: HOST arrays of nd entries.  The one rule covers channel-last and channel-first
 * sources, transposed axes, a window cut out of a larger signal and a broadcast channel (stride 0).  Unpatched presets pass
 * patch_nums of all ones.
 *   src_kind 0 (uint8): y = (float)q / 255.0f, one IEEE fp32 division (what ToTensor and `video / 255` give on the CPU)
 *   src_kind 1 (fp32):  the 32 bits unchanged -- NaN payloads, +-0, infinities and denormals keep their bits
 * y [n_data * prod(patch_nums)][prod(patch_size)][channels] fp32, contiguous, in the row order of rcb_recon_finish and of
 * rcb_siren_desc.pe_grid_dims: row n is patch n % prod(patch_nums) (row-major over patch_nums) of signal n / prod(patch_nums), its
 * pixel p the row-major position inside the patch.  rcb_recon_finish on this y with the same geometry gives the signals back
 * (both ends, and their _pad / _crop forms, decode that row order with the one routine of csrc/patch_grid.h).
 * Memory: quads of 4 consecutive elements of y.  With channel_stride = 1, axis_stride[nd-1] = channels, patch_size[nd-1] * channels a
 * multiple of 4 and the base pointers, data_stride and the outer strides keeping every run start on a 4-element boundary (y: 16
 * bytes), a quad is one 4-byte (uint8) / 16-byte (fp32) load and one 16-byte store; otherwise the same quads move element by
 * element.  The entry decides; both paths give the same bits.  Source offsets are 64-bit.
 * n_data = 0 succeeds and launches nothing.  Refused (RCB_ERR_*), nothing launched: nd outside 1..3, channels out of range, a
 * non-positive patch count or size, an unknown src_kind, a negative stride, more than 2^31 - 1 elements per signal, null src or y
 * with n_data > 0. */
int rcb_signal_patch(const void* src, int32_t src_kind, int64_t n_data, int32_t nd, const int32_t* patch_nums,
                     const int32_t* patch_size, int32_t channels, int64_t data_stride, const int64_t* axis_stride,
                     int64_t channel_stride, float* y, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4 (411): signals of any size.  The encoder replicates a signal's edge samples out to the grid the model accepts, the decoder
 * crops back, and the distortion figure counts the real samples only.
 *
 * rcb_signal_patch_pad is rcb_signal_patch for signals that hold only size[i] positions per axis, 1 <= size[i] <= G_i =
 * patch_nums[i] * patch_size[i] (`size`: a HOST array of nd entries; `src` addresses only that extent): grid position g_i reads
 * source position min(g_i, size[i] - 1) -- edge replication on the far side of every axis (np.pad(mode="edge") after the
 * signal).  Row order, q / 255 as one IEEE fp32 division, the bit-preserving fp32 move, 64-bit source offsets and any
 * non-negative strides are rcb_signal_patch's.  A quad of y that is 4 consecutive EXISTING source elements on a 4-element boundary
 * (the conditions of rcb_signal_patch, on the strides of the axes with more than one position) is one 4- / 16-byte load; every
 * other quad moves element by element through the clipped index; both give the same bits.  No read leaves the extent.
 * With size = G every bit of y is rcb_signal_patch's.  Refused: what rcb_signal_patch refuses, a null `size`, a size[i] outside
 * [1, G_i]. */
int rcb_signal_patch_pad(const void* src, int32_t src_kind, int64_t n_data, int32_t nd, const int32_t* patch_nums,
                         const int32_t* patch_size, const int32_t* size, int32_t channels, int64_t data_stride,
                         const int64_t* axis_stride, int64_t channel_stride, float* y, rcb_stream_t stream);

/* rcb_recon_finish_crop is rcb_recon_finish (nd = 1..3; unpatched presets pass patch_nums of ones) for datapoints of which only
 * the leading size[i] <= G_i positions per axis are real (`size`: a HOST array of nd entries).  Per element the arithmetic is
 * rcb_recon_finish's.  u8 / whole are contiguous [n_data][size_0]..[size_nd-1][channels]; only positions inside the extent are
 * written.  sse / n_bad keep the chunks and the order of additions of rcb_recon_finish over the PADDED datapoint (the same
 * workspace: rcb_recon_workspace_bytes(n_data, padded elements per datapoint)): an element outside the extent adds +0.0 and is
 * never counted as non-finite, whatever y and target hold there.  So sse is the sum over the real samples, bitwise what
 * rcb_recon_finish gives for a target that equals v outside the extent, and bitwise the same alone, in any batch and from run to
 * run (no floating-point atomics).  With size = G every output bit is rcb_recon_finish's.
 * Refused: what rcb_recon_finish refuses, nd = 0, a null `size`, a size[i] outside [1, G_i]. */
int rcb_recon_finish_crop(const float* y, const float* target, int64_t n_rows, int32_t n_pix, int32_t channels, int32_t nd,
                          const int32_t* patch_nums, const int32_t* patch_size, const int32_t* size, int32_t mode, uint8_t* u8,
                          float* whole, double* sse, int32_t* n_bad, void* workspace, int64_t workspace_bytes, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4 (412): 16-bit sample formats -- PCM audio (the reference's data/audio.py:50-54 forms (q / 32768 + 1) / 2 on the host) and
 * images / video of 9 to 16 bits.  The sample formats of both ends, defined once:
 *   kind 0 (uint8) and kind 1 (fp32; on the way out: raw) are rcb_signal_patch's and rcb_recon_finish's modes 0 and 1, unchanged.
 *   kind 2 (u16 at `depth` b, 9 <= b <= 16): samples stored in 16-bit unsigned words, M = 2^b - 1 (exact in fp32).
 *     in:   y = (float)q / (float)M, one IEEE fp32 division.  A stored value above M is NOT clamped: y > 1.
 *     out:  c = NaN ? 0 : fminf(fmaxf(x, 0), 1);  q = rintf(c * (float)M), an fp32 multiply rounded half to even;
 *           v = (float)(int)q / (float)M.  v is formed from the integer, so q = 0 gives +0.0 whatever the sign of x (not mode 0's
 *           -0.0).
 *   kind 3 (s16: 16-bit two's-complement PCM on the audio preset's [0, 1) normalisation; depth 0):
 *     in:   y = ((float)q + 32768.0f) / 65536.0f, every step exact: bit for bit the reference's (q / 32768 + 1) / 2 in fp32.
 *     out:  c as above;  u = fminf(rintf(c * 65536.0f), 65535.0f);  q = (int)u - 32768 as int16;  v = u / 65536.0f, exact.
 *   Round trip: out(in(q)) == q for every representable q -- 0 .. M at every depth, all of int16.
 *   sse keeps its definition, over d = t - v in fp32, with the chunks, the order of additions and the n_bad / NaN rules of
 *   rcb_recon_finish: the distortion of the signal the decoder delivers.
 *
 * rcb_signal_patch_fmt is rcb_signal_patch (`size` null) or rcb_signal_patch_pad (`size`: its HOST array) for src_kind 0 .. 3;
 * strides are in elements of the source type.  A quad of 4 consecutive 16-bit source elements is one 8-byte load under the
 * conditions of those entries, `src` and every run start 8-byte aligned; otherwise the quad moves element by element; both give
 * the same bits.  Kinds 0 and 1 give every bit of y the older entries give.
 * rcb_recon_finish_fmt is rcb_recon_finish (`size` null) or rcb_recon_finish_crop (`size`) for modes 0 .. 3, mode 2 = u16 at
 * `depth`, mode 3 = s16.  `q_out` (nullable): q in the stitched / cropped layout of `u8` -- uint8 (mode 0), uint16 (mode 2) or
 * int16 (mode 3).  A quad of 16-bit q is one 8-byte store when q_out is 8-byte aligned (the crop form: and size[nd-1] * channels is
 * a multiple of 4); otherwise element by element, the same bits.  Modes 0 and 1 give every output bit of the older entries, the
 * -0.0 of mode 0 included.
 * Refused (RCB_ERR_*), nothing launched: what the older entries refuse, a kind or mode outside 0 .. 3, a depth outside 9 .. 16 for
 * kind / mode 2, a non-zero depth for any other, q_out with mode 1.  The older entries keep refusing kind 2 and mode 2. */
int rcb_signal_patch_fmt(const void* src, int32_t src_kind, int32_t depth, int64_t n_data, int32_t nd, const int32_t* patch_nums,
                         const int32_t* patch_size, const int32_t* size, int32_t channels, int64_t data_stride,
                         const int64_t* axis_stride, int64_t channel_stride, float* y, rcb_stream_t stream);
int rcb_recon_finish_fmt(const float* y, const float* target, int64_t n_rows, int32_t n_pix, int32_t channels, int32_t nd,
                         const int32_t* patch_nums, const int32_t* patch_size, const int32_t* size, int32_t mode, int32_t depth,
                         void* q_out, float* whole, double* sse, int32_t* n_bad, void* workspace, int64_t workspace_bytes,
                         rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4 (413): batches of signals of mixed sizes and memory layouts -- the per-signal ("ragged") forms of rcb_signal_patch_fmt and
 * rcb_recon_finish_fmt.  All signals of a call share the patch grid G_i = patch_nums[i] * patch_size[i], the channels and the
 * sample format; each keeps its own extent and its own place and strides in one source / output buffer:
 *   sizes  HOST int32 [n_data][3]: the first nd entries of row d are signal d's extent along the grid axes, 1 <= size <= G_i
 *          (the others are ignored).
 *   spans  HOST int64 [n_data][4]: {offset, axis_stride[0 .. 2]} (the first nd strides count), in elements of the source / output
 *          type, all >= 0.  Element (g, c) of signal d lies at base + offset + sum g_i * axis_stride[i] + c * channel_stride; a
 *          transposed signal is only a matter of strides.
 *   table  device buffer of rcb_ragged_table_bytes(n_data) bytes (-1 for n_data < 0), 8-byte aligned, the caller's to allocate:
 *          the entry validates the host tables, writes their device copy (with a per-signal flag for the memory path) there on
 *          `stream` and synchronises the stream ONCE for that upload; on return the host arrays are the caller's again.  Because
 *          of that synchronisation these two entries are NOT for graph capture: they are the I/O ends, not part of the step.
 *
 * rcb_signal_patch_ragged: per signal exactly rcb_signal_patch_fmt with that signal's `size` and strides -- grid position g_i reads
 * min(g_i, size_i - 1), the four sample kinds of 412, rows d * prod(patch_nums) + patch of y as ever.  A signal whose strides and
 * alignment meet the vector-path conditions of rcb_signal_patch_pad takes the 4- / 8- / 16-byte loads, any other moves element by
 * element, in the same call, with the same bits.  `src_elems`: elements of the source buffer from `src`; a signal whose farthest
 * element offset + sum (size_i - 1) * axis_stride[i] + (channels - 1) * channel_stride is >= src_elems is refused, so every read
 * lies inside [src, src + src_elems).
 *
 * rcb_recon_finish_ragged: per signal exactly rcb_recon_finish_fmt with that signal's `size`; the channel stride is 1.  q_out /
 * whole (each nullable) are ONE buffer of out_elems elements each, signal d's values at its span.  Every signal must be dense with
 * its axes in some order: sorted by stride the innermost stride is `channels` and each next one the previous times that axis's
 * size (axes of size 1 are ignored); the ranges [offset, offset + channels * prod(size)) must be pairwise disjoint and lie inside
 * [0, out_elems) -- so every write lies inside the buffers and no two signals meet.  Elements of the buffers outside the spans are
 * not touched.  sse[d] / n_bad[d] keep the chunks and the order of additions over the PADDED datapoint (workspace:
 * rcb_recon_workspace_bytes(n_data, padded elements)); an element outside a signal's extent adds +0.0 and is never counted, and
 * sse[d] is bitwise rcb_recon_finish_fmt(size = sizes[d])'s for that signal alone -- in any batch, in any batch order, from run to
 * run.
 * Refused (RCB_ERR_*), nothing launched and nothing uploaded: what the _fmt entries refuse, null sizes / spans / table, table_bytes
 * below rcb_ragged_table_bytes(n_data) or a misaligned table, a size outside [1, G_i], a negative offset or stride, a reach past
 * src_elems, output strides that are not dense, overlapping spans, a span past out_elems.  n_data = 0 (n_rows = 0) succeeds and
 * launches nothing. */
int64_t rcb_ragged_table_bytes(int64_t n_data);
int rcb_signal_patch_ragged(const void* src, int64_t src_elems, int32_t src_kind, int32_t depth, int64_t n_data, int32_t nd,
                            const int32_t* patch_nums, const int32_t* patch_size, const int32_t* sizes, const int64_t* spans,
                            int32_t channels, int64_t channel_stride, float* y, void* table, int64_t table_bytes,
                            rcb_stream_t stream);
int rcb_recon_finish_ragged(const float* y, const float* target, int64_t n_rows, int32_t n_pix, int32_t channels, int32_t nd,
                            const int32_t* patch_nums, const int32_t* patch_size, const int32_t* sizes, const int64_t* spans,
                            int64_t out_elems, int32_t mode, int32_t depth, void* q_out, float* whole, double* sse, int32_t* n_bad,
                            void* workspace, int64_t workspace_bytes, void* table, int64_t table_bytes, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4 (417): the distortion figure by REGION -- per frame of a clip, per patch, per tile of a distortion map -- where the entries
 * above give one sum per datapoint.  rcb_recon_regions reads what rcb_recon_finish_fmt reads: y and `target` (nullable)
 * [n_rows][n_pix][channels] fp32, nd = 1..3 with patch_nums / patch_size, a nullable `size` (the extent sz; null: the grid G), mode
 * 0 .. 3 and depth; and `region`, a HOST array of nd entries, the box per axis, each >= 1 (a box may exceed the extent).  It writes
 * nothing but sums.
 *   Region grid: regions tile the EXTENT, not the grid: nr[i] = ceil(sz[i] / region[i]) boxes per axis, n_regions = prod nr[i], the
 *     region index row-major over (r_0 .. r_nd-1); region r is the box [r_i * region[i], min((r_i + 1) * region[i], sz[i])) -- a region
 *     on the far edge is a smaller box.  Padding (grid positions outside the extent) belongs to no region: it adds nothing, is never
 *     counted, is never read, and its values -- a NaN included -- cannot change any output bit.
 *   Elements of a region: the box's positions row-major with the channels innermost, n_r = prod(box_i) * channels of them: the order
 *     of the whole signal, NOT the patch order of y.  The value at an element is what rcb_recon_finish_fmt forms there for the same
 *     mode and depth: v, d = t - v in fp32, the term (double)d * (double)d.
 *   Sum: the additions rcb_recon_finish performs on a datapoint of n_r elements -- chunks of 8192 elements, thread t of 256 owning
 *     the quads t, t + 256, ... in element order, the xor butterfly over the lanes, the waves in wave order, then the chunk partials
 *     (thread t: partials t, t + 256, ..., the same butterfly).  So sse_r[d][r] is BITWISE the sse that rcb_recon_finish_fmt (nd = 0,
 *     n_pix = n_r / channels, same mode and depth) returns for that region's values copied out contiguously in that order; and
 *     bitwise the same alone, in any batch, in any batch order, from run to run, and on the 16-byte and the element-wise memory
 *     path (16-byte loads: min(region, sz)[nd-1] * channels, sz[nd-1] * channels and patch_size[nd-1] * channels multiples of 4,
 *     y and target 16-byte aligned; the entry decides).
 *   What does NOT hold: sum_r sse_r[d][r] is the datapoint's sse (rcb_recon_finish_fmt with the same size) only to within
 *     reordering -- the same terms, other additions -- not bitwise.  The one exception: a single region covering an unpatched signal
 *     (patch_nums of ones, size null), where the two orders coincide and so do the bits.
 *   n_bad_r [n_data][n_regions] int32: the non-finite y and target elements of the region (an element with both counts twice).  A
 *     region with n_bad_r > 0 has sse_r = NaN; no other region does.
 *   sse_r [n_data][n_regions] fp64; needs `target`.  Each output is nullable, not both.
 * `workspace`: rcb_recon_regions_workspace_bytes(n_data, n_regions, max_region_elems) bytes, 8-byte aligned, max_region_elems =
 * prod(min(region[i], sz[i])) * channels, the elements of the largest box; callable without a device; -1 for a shape it refuses: a
 * non-positive argument, more than 2^31 - 1 regions or elements, more than 2^31 - 1 workgroups = n_data * n_regions *
 * ceil(max_region_elems / 8192).  (A box of few elements still occupies a workgroup of 256 threads: tiles of 8 x 8 leave most lanes
 * idle.  The entry is exact there, not efficient.)
 * Nothing is uploaded and the stream is not synchronised: unlike the per-signal entries of 413, this one can be graph-captured.
 * Refused (RCB_ERR_*), nothing launched: null y / workspace / patch geometry / region, both outputs null, nd outside 1..3, a
 * region[i] < 1, channels outside 1..32, n_pix != prod(patch_size), n_rows no multiple of prod(patch_nums), a size[i] outside
 * [1, G_i], the mode and depth rules of rcb_recon_finish_fmt, sse_r without target, more than 2^31 - 1 elements per datapoint or
 * workgroups, a workspace that is too small or misaligned. */
int64_t rcb_recon_regions_workspace_bytes(int64_t n_data, int64_t n_regions, int64_t max_region_elems);
int rcb_recon_regions(const float* y, const float* target, int64_t n_rows, int32_t n_pix, int32_t channels, int32_t nd,
                      const int32_t* patch_nums, const int32_t* patch_size, const int32_t* size, const int32_t* region, int32_t mode,
                      int32_t depth, double* sse_r, int32_t* n_bad_r, void* workspace, int64_t workspace_bytes, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4 (414): SSIM and the sums of MS-SSIM (Wang et al. 2004, the usual constants) of decoded images against their sources, on the
 * INTEGERS of both: the second column of every codec comparison, which the reference (PSNR alone, utils.py:200-260) does not
 * report.  a, b: [n_img][H][W][C] samples of kind 0 (uint8, depth 0, L = 255) or kind 2 (16-bit unsigned words at `depth` b,
 * 9 <= b <= 16, L = 2^b - 1; a stored value above L is used as it is, as rcb_signal_patch_fmt does).  Each operand has its own
 * ELEMENT strides {image, row, column, channel} (HOST int64[4], >= 0): the addressing rule of rcb_signal_patch, 64-bit offsets --
 * channel-first storage, transposed axes, a window of a larger image, a broadcast channel; nothing need be contiguous.
 * The definition, every product and sum one IEEE fp64 operation (no contraction), divisions correctly rounded:
 *   window   `win`: HOST double[11], w = g / sum(g), g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)); c1 = (0.01 L)^2, c2 = (0.03 L)^2.  The
 *            caller forms all three (utils.ssim_window, utils.ssim_constants); the device evaluates no exp and no constant.
 *   filter   "valid" positions only, (H - 10) x (W - 10) per channel; separable, the LAST spatial axis first, taps ascending, the
 *            first product starting the sum:  t(r, x) = ((w0 v(r, x) + w1 v(r, x+1)) + ...) + w10 v(r, x+10), and m(y, x) the same
 *            over t(y+i, x); for v in {a, b, a a, b b, a b}, the products exact.
 *   formula  maa = ma ma, mbb = mb mb, mab = ma mb;  saa = m(a a) - maa, sbb = m(b b) - mbb, sab = m(a b) - mab (not clamped);
 *            cs = (2 sab + c2) / ((saa + sbb) + c2);  l = (2 mab + c1) / ((maa + mbb) + c1);  ssim = l cs.
 *            Identical operands give ssim = cs = 1.0 exactly: numerator and denominator are the same expressions.
 *   scales   scale s = 0 .. scales-1 works on floor(H / 2^s) x floor(W / 2^s); a sample is the INTEGER sum of its 2^s x 2^s block (a
 *            trailing odd row or column is dropped at each halving), used as sum / 4^s in fp64, which is exact.  Each scale needs
 *            both sides >= 11: five scales need min(H, W) >= 176.
 * sums [n_img][scales][C][2] int64, written (not accumulated into): {sum of rint(ssim * RCB_SSIM_FX_SCALE), sum of rint(cs *
 *      RCB_SSIM_FX_SCALE)} over the positions of that image, scale and channel, rint to nearest even.  Integer sums have no order,
 *      so an image's sums are bitwise the same alone, in a batch, in any batch order and from run to run (64-bit integer atomics
 *      after a memset of `sums` on the stream).  Terms lie in [-1, 1] * 2^36 and an image has at most 2^26 positions: |sum| < 2^62.
 * map  nullable, [n_img][H-10][W-10][C][2] fp64: {ssim, cs} of scale 0 per position.
 * workspace: rcb_ssim_workspace_bytes(n_img, H, W, C, scales) bytes (the block sums of scales 1 ..; 0 for one scale, when the pointer
 *      may be null; -1: shape refused), 16-byte aligned, caller-allocated.  No host synchronisation and no readback.
 * n_img = 0 succeeds and launches nothing.  Refused (RCB_ERR_*), nothing launched: kind 1 or 3 (or any other), a depth outside
 * 9 .. 16 for kind 2 or a non-zero depth for kind 0, C outside 1 .. 32, H or W below 11, scales outside 1 .. 5 or more scales than
 * the size allows, more than 2^26 positions per image, a negative stride, null a / b / sums / win / strides, a workspace that is too
 * small or misaligned.  The figures are formed on the host (utils.ssim_from_sums, utils.msssim_from_sums). */
#define RCB_SSIM_FX_SCALE 68719476736.0          /* 2^36 */
int64_t rcb_ssim_workspace_bytes(int64_t n_img, int32_t H, int32_t W, int32_t C, int32_t scales);
int rcb_ssim(const void* a, const void* b, int32_t kind, int32_t depth, int64_t n_img, int32_t H, int32_t W, int32_t C,
             const int64_t* a_strides, const int64_t* b_strides, const double* win, double c1, double c2, int32_t scales,
             int64_t* sums, double* map, void* workspace, int64_t workspace_bytes, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4 (415): rcb_ssim for a LIST of images of mixed sizes and memory layouts -- and so for the frames of video clips -- in one call:
 * one memset, scales - 1 pooling launches and `scales` SSIM launches, whatever n_img is.  All images share C, the sample format,
 * the window, the constants and `scales`; each keeps its own extent and its own place and strides in the operands' buffers:
 *   sizes    HOST int32 [n_img][2] = {H, W}.
 *   a_spans, b_spans  HOST int64 [n_img][4] = {offset, row stride, column stride, channel stride}, in elements, all >= 0.  Element
 *            (y, x, c) of image k lies at base + offset + y * rs + x * cs + c * chs, 64-bit offsets.  The channel stride is per
 *            image: channel-last, channel-first, transposed, windowed and broadcast-channel images may share one call.
 *   a_elems, b_elems  elements of the buffers from `a` and `b`; an image whose farthest element offset + (H - 1) rs + (W - 1) cs +
 *            (C - 1) chs is >= that count is refused, so every read lies inside [a, a + a_elems) and [b, b + b_elems).
 *   table    device buffer of rcb_ssim_list_table_bytes(n_img, scales) bytes (-1: n_img or scales refused), 8-byte aligned, the
 *            caller's to allocate.  The entry validates the host tables, writes their device copy there on `stream` and
 *            synchronises the stream ONCE for that upload -- the rule of the per-signal entries of 413: this entry is NOT for
 *            graph capture.  On return the host arrays are the caller's again.
 *   workspace  rcb_ssim_list_workspace_bytes(n_img, sizes, C, scales) bytes = the sum over k of rcb_ssim_workspace_bytes(1, H_k,
 *            W_k, C, scales) (-1: a shape refused), image k's block laid out as that call lays it out; 16-byte aligned; may be
 *            null for one scale.
 * Image k is scored exactly as rcb_ssim scores it with n_img = 1 and H_k x W_k -- same window, filter order, formula, floor pooling
 * of integer block sums, fixed-point terms.  sums [n_img][scales][C][2] int64, written (not accumulated into): image k's slice is
 * bitwise what rcb_ssim gives for that image alone, in any list, in any list order and from run to run.  Every image must allow
 * `scales`.  The list form has NO `map` output: the per-position {ssim, cs} of an image come from rcb_ssim.
 *
 * rcb_ssim_list_plan: the host arithmetic of the table, callable without a device; rcb_ssim_list builds its table through it.
 * Writes plan[(s * n_img + k) * 5 + {0 .. 4}] = {first tile, first pooling workgroup, workspace offset in uint32 elements of
 * operand a's block sums (b's follow 16-byte aligned behind them), H_s, W_s} of image k at scale s -- a tile is 16 x 16 window
 * positions, a pooling workgroup 256 block sums of both operands; scale 0 pools nothing: 0, 0 there -- then per scale
 * plan[5 * scales * n_img + 2 s + {0, 1}] = {tiles, pooling workgroups} of the whole list.  -> the number of ints written,
 * scales * (5 n_img + 2), or an error (< 0); max_ints below that number is RCB_ERR_SHAPE.
 *
 * Refused (RCB_ERR_*), nothing launched and nothing uploaded: everything rcb_ssim refuses, per image and naming the image; null
 * sizes, spans or table; a table or workspace that is too small or misaligned; a negative offset or stride; a reach past a_elems /
 * b_elems; more than 2^31 - 1 tiles (or pooling workgroups) at one scale over the list; more than 2^24 images.  n_img = 0
 * succeeds and launches nothing. */
int64_t rcb_ssim_list_table_bytes(int64_t n_img, int32_t scales);
int64_t rcb_ssim_list_workspace_bytes(int64_t n_img, const int32_t* sizes, int32_t C, int32_t scales);
int rcb_ssim_list_plan(int64_t n_img, const int32_t* sizes, int32_t C, int32_t scales, int64_t* plan, int64_t max_ints);
int rcb_ssim_list(const void* a, int64_t a_elems, const void* b, int64_t b_elems, int32_t kind, int32_t depth, int64_t n_img,
                  const int32_t* sizes, const int64_t* a_spans, const int64_t* b_spans, int32_t C, const double* win, double c1,
                  double c2, int32_t scales, int64_t* sums, void* workspace, int64_t workspace_bytes, void* table,
                  int64_t table_bytes, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4 (416): resize image and video sources -- what the reference's video loader does before anything else (data/video.py:26-31:
 * the first 24 frames, centre-cropped to 240 x 240 and resized to 128 x 128 with torchvision's Resize: bilinear, antialiased,
 * half-pixel centres) and what every codec comparison at a reduced resolution starts with.  The resized integers are the SOURCE
 * the finish and SSIM entries score against.  The centre crop is a view (utils.center_crop: top = int(round((H - h) / 2.0)),
 * Python's round, torchvision's rule); the filter is defined here.
 *
 * Taps of one axis of n_in input and n_out output positions, every step one IEEE fp64 operation (no contraction):
 *   scale = (double)n_in / n_out;  support = scale >= 1 ? scale : 1;  inv = scale >= 1 ? 1 / scale : 1
 *   output i:  center = scale * (i + 0.5);  first = max((int)((center - support) + 0.5), 0), the conversion truncating;
 *              last = min((int)((center + support) + 0.5), n_in);  count = last - first
 *              g_j = max(0, 1 - |(((first + j) - center) + 0.5) * inv|), j = 0 .. count - 1;  total = ((g_0 + g_1) + ...), ascending;
 *              w_j = g_j / total
 *   n_in == n_out:  first = i, count = 1, w_0 = 1.0 -- the formulas give that tap and behind it one of weight exactly 0, which is
 *   dropped on this axis, so that the identity returns every sample bit for bit, -0.0 and the non-finite ones included.
 *   n_in <= 16 n_out, hence count <= 33 = RCB_RESIZE_MAX_TAPS; a steeper reduction is RCB_ERR_UNSUPPORTED.  Upscaling by any
 *   factor is allowed.  Sides up to 2^24.
 * Filter: separable, the LAST spatial axis first, taps ascending, the first product starting the sum (w, f the taps of column x;
 *   u, g those of row y):  t(r, x) = ((w_0 v(r, f) + w_1 v(r, f+1)) + ...),  a(y, x) = ((u_0 t(g, x) + u_1 t(g+1, x)) + ...), v the
 *   sample as an exact fp64 value, t never rounded below fp64.
 * Output, L = 255 (kind 0) or 2^depth - 1 (kind 2):
 *   kind 0 (uint8) and kind 2 (u16 at depth 9 .. 16):  q = (int)rint(fmin(fmax(a, 0), L)), half to even: ONE rounding, at the end.  A
 *          stored 16-bit value above L goes in as it is and comes out clamped.
 *   kind 1 (fp32):  (float)a, one rounding, no clamp.  Non-finite values follow the arithmetic: a zero weight times an infinity
 *          is a NaN.
 *   kind 3 (s16) is refused: resampling audio is a different filter question, which rcb_resample (419, below) answers.
 * This is torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False) evaluated in fp64 and rounded
 * once (tests/test_resize_emul_cpu.py holds the two together).  torchvision's uint8 path -- fixed-point weights, a rounding to
 * uint8 BETWEEN the two passes -- is NOT copied: it differs from this definition by at most one step in a share of the samples
 * (12 - 20 % on random images; profiles/r22_resize_vs_uint8_path.txt).
 *
 * rcb_resize_taps: the host arithmetic above, callable without a device.  first, count: int32 [n_out]; w: double [n_out][max_taps],
 * row i holding its count taps and then +0.0.  -> the longest count of the axis, or an error (< 0): a size below 1 (RCB_ERR_SHAPE),
 * more than 16 : 1 or a side above 2^24 (RCB_ERR_UNSUPPORTED), a null pointer (RCB_ERR_ARG), max_taps below the longest count
 * (RCB_ERR_SHAPE; nothing is written).
 *
 * rcb_resize_table_bytes: the device table of rcb_resize for these sizes, 8 * (H_out * (1 + ky) + W_out * (1 + kx)) bytes, ky / kx
 * the longest count of the row / column axis: int32 first and count of both axes, then the weights at the pitch of their axis.
 * -1 for a refused shape.
 *
 * rcb_resize: src holds n signals of T frames (T = 1: images) of H_in x W_in positions and C channels.
 *   strides  HOST int64[5]: ELEMENT strides of {signal, frame, row, column, channel}, all >= 0; `offset` (>= 0): the element of
 *            signal 0, frame 0, row 0, column 0, channel 0 -- where the corner of a crop goes.  The addressing rule of
 *            rcb_signal_patch, 64-bit offsets: channel-first storage, transposed axes, a window of a larger signal, a broadcast
 *            channel and a clip's frame stride are all this one call; nothing need be contiguous.
 *   src_elems  elements of the source buffer from `src`; the farthest element read, offset + (n - 1) s_0 + (T - 1) s_1 +
 *            (H_in - 1) s_2 + (W_in - 1) s_3 + (C - 1) s_4, must lie below it (checked on the host): every read is inside.
 *   dst      contiguous [n][T][H_out][W_out][C] of the source's type.
 *   table    device buffer of rcb_resize_table_bytes(H_in, W_in, H_out, W_out) bytes, 8-byte aligned, the caller's to allocate.
 *            The entry builds both tap tables through rcb_resize_taps, writes them there on `stream` and synchronises the stream
 *            ONCE for that upload -- the rule of the entries of 413 and 415: an I/O end, NOT for graph capture.
 * One workgroup per tile of 8 x 32 output positions of one frame; the row-filtered values live in LDS as fp64.  A frame's output
 * is bitwise the same alone, in any batch and from run to run.  One input size per call; there is no list form.
 * n = 0 succeeds and launches nothing.  Refused (RCB_ERR_*), nothing launched and nothing uploaded: a kind other than 0, 1, 2; a
 * depth outside 9 .. 16 for kind 2 or non-zero for another kind; C outside 1 .. 32; a size (or T) below 1; n_in > 16 n_out on
 * either axis; a negative stride or offset; a reach past src_elems; null src, dst, strides or table; a table that is too small or
 * misaligned; more than 2^31 - 1 workgroups. */
#define RCB_RESIZE_MAX_TAPS 33
int rcb_resize_taps(int32_t n_in, int32_t n_out, int32_t* first, int32_t* count, double* w, int32_t max_taps);
int64_t rcb_resize_table_bytes(int32_t H_in, int32_t W_in, int32_t H_out, int32_t W_out);
int rcb_resize(const void* src, int64_t src_elems, int32_t kind, int32_t depth, int64_t n, int32_t T, int32_t H_in, int32_t W_in,
               int32_t C, const int64_t* strides, int64_t offset, int32_t H_out, int32_t W_out, void* dst, void* table,
               int64_t table_bytes, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4 (418): Y'CbCr on the device.  Raw video is planar Y'CbCr 4:2:0 at 8 or 10 bits, and codec comparisons report PSNR per plane
 * (PSNR-Y, and (6 Y + Cb + Cr) / 8 on 4:2:0 planes) and SSIM on luma; the entries above read and score interleaved RGB only.
 * rcb_ycc_to_rgb turns planes into the [..][H][W][3] signals rcb_resize / rcb_signal_patch / rcb_ssim take; rcb_rgb_to_ycc forms the
 * planes of an RGB signal; rcb_ycc_sse gives the squared error of two RGB signals per plane, only the sums leaving the device.
 *
 * Samples: kind 0 (uint8, depth 0, L = 255) or kind 2 (16-bit unsigned words at `depth` b, 9 <= b <= 16, L = 2^b - 1; a stored
 * value above L goes in as it is), as rcb_ssim.  Kinds 1 and 3 are refused.
 * Subsampling `ss`: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0.  A frame has H x W luma positions, any H, W >= 1 (odd sizes are legal), and
 * chroma planes of Hc x Wc with Hc = ss == 2 ? (H + 1) / 2 : H, Wc = ss ? (W + 1) / 2 : W.
 * The device evaluates no colour constant: the caller passes the matrix (HOST double[9], row-major) and the offsets (HOST
 * double[3]); utils.ycc_matrix forms them for BT.601 / 709 / 2020 at full or limited range, as win, c1, c2 are formed for rcb_ssim.
 * Every product and sum below is ONE IEEE fp64 operation, no contraction, in the order the parentheses give.
 *   Q(v) = (int)rint(fmin(fmax(v, 0), L)), half to even.  The clamp is to [0, L] only: the foot- and headroom of a limited range
 *          are not clamped away.
 * Forward (RGB -> Y'CbCr), r, g, b the samples of a position as exact fp64 values, plane k = 0 (Y), 1 (Cb), 2 (Cr):
 *   p_k(y, x) = (m[k][0] r + m[k][1] g) + m[k][2] b
 *   Y(y, x)      = Q(p_0(y, x) + off[0])
 *   4:4:4  C_k(y, x) = Q(p_k(y, x) + off[k])
 *   4:2:2  C_k(y, j) = Q((p_k(y, min(2j, W-1)) + p_k(y, min(2j+1, W-1))) * 0.5 + off[k])
 *   4:2:0  C_k(i, j) = Q(((p00 + p01) + (p10 + p11)) * 0.25 + off[k]),  p_ab = p_k(min(2i+a, H-1), min(2j+b, W-1))
 *   -- the mean is taken over UNROUNDED fp64 values, rows and columns clipped to the extent (edge replication on the far side),
 *   and the result is rounded ONCE.
 * Inverse (Y'CbCr -> RGB), channel k = 0 (R), 1 (G), 2 (B), Y, Cb, Cr the samples as exact fp64 values:
 *   v_k = (n[k][0] (Y - o[0]) + n[k][1] (Cb - o[1])) + n[k][2] (Cr - o[2]),  q_k = Q(v_k)
 *   -- the subtractions are exact; a zero coefficient is multiplied like any other.  Position (y, x) reads the chroma sample
 *   (ss == 2 ? y >> 1 : y, ss ? x >> 1 : x): replication.  A smoother chroma upsampling is rcb_resize of the chroma planes followed
 *   by this entry at 4:4:4 (utils.ycc_to_rgb_device, chroma="bilinear").
 *
 * rcb_ycc_to_rgb: py, pcb, pcr are the first samples of the three planes of n signals of T frames (T = 1: images); each plane has
 *   its own ELEMENT strides {signal, frame, row, column} (HOST int64[4], >= 0) and its own element count elems[k] (HOST int64[3],
 *   counted from the plane's pointer): the farthest element read, (n - 1) s_0 + (T - 1) s_1 + (rows - 1) s_2 + (columns - 1) s_3,
 *   must lie below it (checked on the host, as rcb_resize does): every read is inside.  One rule covers I420 / YV12 in one buffer
 *   (three views), NV12 / P010-style interleaved chroma (column stride 2) and a window of a larger frame.  `inv` is n, `o` is o.
 *   dst: contiguous [n][T][H][W][3] of the source's type.
 * rcb_rgb_to_ycc: src holds RGB through ELEMENT strides {signal, frame, row, column, channel} (HOST int64[5], >= 0), `offset`
 *   (>= 0) and src_elems -- the rule of rcb_resize: channel-first, transposed, windowed and broadcast sources; the farthest element
 *   read lies below src_elems.  oy [n][T][H][W] and ocb, ocr [n][T][Hc][Wc], contiguous, of the source's type; each is nullable, at
 *   least one is not.  oy alone is the luma plane rcb_ssim scores with C = 1.
 * rcb_ycc_sse: a, b are two RGB operands of the same n, T, H, W, each with its own strides, offset and element count as above.
 *   sse [n][T][3] int64, WRITTEN (not accumulated into): per frame and plane the sum of (qa - qb)^2 over the integers
 *   rcb_rgb_to_ycc delivers for a and for b -- H W terms for Y, Hc Wc for Cb and for Cr.  A frame has at most 2^26 positions and
 *   a term is < 2^32: a sum is < 2^58.  64-bit integer atomics after a memset of `sse` on the stream, one atomic per workgroup and
 *   plane; integer sums have no order, so a frame's row is bitwise the same alone, in any batch, in any batch order and from run
 *   to run.  utils.psnr_ycc_from_sse forms the figures.
 * A thread owns 2 x 4 positions (whole chroma blocks), a workgroup of 256 threads 16 x 128 positions of one frame.  uint8 RGB with
 * channel stride 1, column stride 3 and every row on a 4-byte boundary is read as three dwords per tile row (and dst / oy written
 * as dwords when W is a multiple of 4); any other layout goes element by element, with the same bits.  The entry decides.
 * No table, no workspace, nothing uploaded and no synchronisation: all three entries can be graph-captured.  n = 0 succeeds and
 * launches nothing.  Refused (RCB_ERR_*), nothing launched: a kind other than 0 / 2, a depth outside 9 .. 16 for kind 2 or non-zero
 * for kind 0; ss outside 0 .. 2; H, W or T below 1; more than 2^26 positions per frame; a negative stride or offset; a reach past an
 * element count; a null operand, matrix, offsets, strides or element-count array; rcb_rgb_to_ycc with all three outputs null;
 * more than 2^31 - 1 workgroups. */
int rcb_ycc_to_rgb(const void* py, const void* pcb, const void* pcr, const int64_t* elems, const int64_t* y_strides,
                   const int64_t* cb_strides, const int64_t* cr_strides, int32_t kind, int32_t depth, int32_t ss, int64_t n, int32_t T,
                   int32_t H, int32_t W, const double* inv, const double* o, void* dst, rcb_stream_t stream);
int rcb_rgb_to_ycc(const void* src, int64_t src_elems, const int64_t* strides, int64_t offset, int32_t kind, int32_t depth, int32_t ss,
                   int64_t n, int32_t T, int32_t H, int32_t W, const double* m, const double* off, void* oy, void* ocb, void* ocr,
                   rcb_stream_t stream);
int rcb_ycc_sse(const void* a, int64_t a_elems, const int64_t* a_strides, int64_t a_offset, const void* b, int64_t b_elems,
                const int64_t* b_strides, int64_t b_offset, int32_t kind, int32_t depth, int32_t ss, int64_t n, int32_t T, int32_t H,
                int32_t W, const double* m, const double* off, int64_t* sse, rcb_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4 (419): resample PCM audio to the preset's rate.  The audio preset is a 16 kHz preset (data/audio.py:39-46 hard-codes
 * LibriSpeech's rate; pixel_sizes x patch_nums = 48 000 samples are "3 s at 16 kHz"); audio elsewhere is 44.1 or 48 kHz and often
 * stereo.  The resampled samples are the SOURCE the finish entries score against, as the resized integers of rcb_resize are.
 *
 * The filter is the polyphase windowed-sinc resampler of torchaudio.functional.resample at its defaults -- Hann-windowed sinc,
 * lowpass_filter_width = 6, rolloff = 0.99 -- evaluated in fp64 with ONE rounding at the end.  Every step below is one IEEE fp64
 * operation, no contraction, in the order the parentheses give.
 * Rates:  g = gcd(rate_in, rate_out), o = rate_in / g, n = rate_out / g.
 *   o == n is the identity: one phase, first = 0, count = 1, w = 1.0 -- every sample is returned bit for bit (-0.0 and the
 *   non-finite ones included), as torchaudio returns its input.
 *   Otherwise o <= 8 n (reductions up to 8 : 1), n <= 1024 and o <= 8192; anything else is RCB_ERR_UNSUPPORTED.  48 000 -> 16 000
 *   (3 : 1), 44 100 -> 16 000 (441 : 160), 22 050 -> 16 000 (441 : 320), 8 000 -> 16 000 (1 : 2), 16 000 -> 44 100 (160 : 441) and
 *   128 000 -> 16 000 (8 : 1) are legal.
 * Taps, formed on the HOST:  base = (double)min(o, n) * 0.99;  width = (int)ceil(6.0 * o / base);  s = base / o
 *   phase p in [0, n), offset k in [-width, width + o):  t = (-(double)p / n + (double)k / o) * base
 *   a tap is kept where |t| < 6 STRICTLY; the kept k of a phase are contiguous: first[p] (which may be negative) and count[p]
 *   c = cos(((t * pi) / 6) / 2);  tp = t * pi;  w = ((tp == 0 ? 1 : sin(tp) / tp) * (c * c)) * s      (pi = 3.14159265358979323846)
 *   torchaudio clamps t to +-6 instead and keeps those taps, whose weight is about 4e-33 s: dropping them is this definition's one
 *   departure from it (tests/test_resample_emul_cpu.py holds the two together within 1e-9 on 16-bit magnitudes).
 *   The longest rows: 37 taps at 3 : 1, 34 at 441 : 160, 13 at every enlargement, 97 = RCB_RESAMPLE_MAX_TAPS at 8 : 1.
 * Filter:  L_out = ceil(n L_in / o) in integer arithmetic.  The caller may ask for the first length_out <= L_out outputs only; they
 *   are computed from the WHOLE source, so the first three seconds of a long recording have no artificial edge at their end.
 *   output i = q n + p:  a = ((w_0 v(m_0) + w_1 v(m_0 + 1)) + ...),  m_0 = q o + first[p], the count[p] taps ascending, the first
 *   product starting the sum.  A sample outside [0, L_in) is +0.0 and is multiplied and added like any other (zero padding,
 *   torchaudio's).
 * Channels:  mix == NULL: every channel is filtered on its own, C_out = C.  mix = HOST double[C]: ONE output channel, filtered
 *   from v(m) = ((g_0 x_0(m) + g_1 x_1(m)) + ...), formed in fp64 before the filter (x_c the sample as an exact fp64 value).
 * Affine:  after the filter a' = a * gain + bias, two operations; skipped altogether when gain == 1 && bias == 0.  gain = bias =
 *   0.5 lets a zero-centred fp32 waveform leave as the preset's (x + 1) / 2.
 * Output, the kind of the input:
 *   kind 3 (s16):   q = (int)rint(fmin(fmax(a', -32768), 32767)), half to even, ONE rounding.
 *   kind 1 (fp32):  (float)a', no clamp.  Non-finite values follow the arithmetic.
 *   kinds 0 and 2 are RCB_ERR_ARG: images are rcb_resize's.
 *
 * rcb_resample_taps: the host arithmetic above, callable without a device.  *o, *n: the ratio.  first, count: int32 [n];
 *   w: double [n][max_taps], row p holding its count[p] weights and then +0.0.  With first, count and w all NULL only *o and *n are
 *   written (how a caller sizes the three).  -> the longest count, or an error (< 0): a rate below 1 (RCB_ERR_SHAPE), an illegal
 *   ratio (RCB_ERR_UNSUPPORTED), null o or n, or only some of first, count, w null (RCB_ERR_ARG), max_taps below the longest count
 *   (RCB_ERR_SHAPE).  Nothing is written on an error.
 * rcb_resample_length: L_out of L_in samples (1 .. 2^31 - 1), or -1 for a refused length or pair of rates.
 * rcb_resample_table_bytes: the device table of rcb_resample for these rates, 8 n (1 + K) bytes, K the longest count: int32 first
 *   and count per phase, then the weights as [tap][phase] -- consecutive outputs are consecutive phases, so a wave reads a tap as
 *   one run of doubles.  -1 for a refused pair.
 * rcb_resample: src holds n_sig signals of L_in samples and C <= 8 channels.
 *   strides  HOST int64[3]: ELEMENT strides of {signal, sample, channel}, all >= 0; `offset` (>= 0): the element of signal 0,
 *            sample 0, channel 0.  The addressing rule of rcb_resize: channel-first storage, a window of a longer buffer and an
 *            expanded channel are all this one call; nothing need be contiguous.
 *   src_elems  elements of the source buffer from `src`; the farthest element read, offset + (n_sig - 1) s_0 + (L_in - 1) s_1 +
 *            (C - 1) s_2, must lie below it (checked on the host): every read is inside.
 *   dst      contiguous [n_sig][length_out][C_out] of the source's type.
 *   table    device buffer of rcb_resample_table_bytes(rate_in, rate_out) bytes, 8-byte aligned, the caller's to allocate.  The
 *            entry forms the taps, writes them there on `stream` and synchronises the stream ONCE for that upload -- the rule of
 *            the entries of 413, 415 and 416: an I/O end, NOT for graph capture.
 * One workgroup per tile of 256 consecutive outputs of one signal; the samples the tile needs are staged once in LDS as fp64,
 * after the mix.  A signal's output is bitwise the same alone, in any batch and from run to run.  One pair of rates per call.
 * n_sig = 0 succeeds and launches nothing.  Refused, nothing launched and nothing uploaded:
 *   RCB_ERR_ARG          a kind other than 1, 3; a negative stride or offset; null src, dst, strides or table
 *   RCB_ERR_SHAPE        C outside 1 .. 8; n_sig < 0; L_in < 1; a rate below 1; length_out outside 1 .. L_out; a reach past
 *                        src_elems; a table that is too small or misaligned
 *   RCB_ERR_UNSUPPORTED  o > 8 n, n > 1024 or o > 8192; L_out above 2^31 - 1; more than 2^31 - 1 workgroups.  (The entry also proves,
 *                        for the table it is about to upload, what the kernel relies on -- the first and the last tap ascend with
 *                        the output index, and no tile spans more samples than the LDS image holds -- and would refuse with this
 *                        code; no legal ratio fails either.) */
#define RCB_RESAMPLE_MAX_TAPS 97
int rcb_resample_taps(int32_t rate_in, int32_t rate_out, int32_t* o, int32_t* n, int32_t* first, int32_t* count, double* w,
                      int32_t max_taps);
int64_t rcb_resample_length(int64_t L_in, int32_t rate_in, int32_t rate_out);
int64_t rcb_resample_table_bytes(int32_t rate_in, int32_t rate_out);
int rcb_resample(const void* src, int64_t src_elems, int32_t kind, int64_t n_sig, int32_t L_in, int32_t C, const int64_t* strides,
                 int64_t offset, int32_t rate_in, int32_t rate_out, const double* mix, double gain, double bias, int32_t length_out,
                 void* dst, void* table, int64_t table_bytes, rcb_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RCB_H_ */
