// Combined launches of the captured training step (one rank, mappings trained: PriorBNNmodel.train's body()).
//
// The step's small kernels -- bookkeeping, the once-per-step conversions of the shared mappings, the optimiser step on
// them, the lpe level's posterior update -- move a few MB each and keep the chip nearly empty while they run, one behind
// the other on the step's serial head and tail.  None of them depends on its neighbours, so here they are BLOCK RANGES of
// one grid (dispatch by blockIdx.x, as in weff_grad_kernel / adam_multi_kernel):
//   rcb_step_prepare = rcb_step_begin + rcb_atrans_pack + rcb_upconv_weff_build
//   rcb_step_tail    = rcb_posterior_bwd (flat fast path, the lpe level) + rcb_adam_multi + rcb_step_end
// The bodies are the ones the separate launches run (posterior_bodies.h, prepare_bodies.h): the same arithmetic per element,
// the same workgroup shapes and summation orders, the same bits.  The kernel names carry no substring bench.py --full
// prices by (`kernel_table.per_inr`): they appear un-priced there.
#include <math.h>

#include "rcb_common.h"

#pragma clang fp contract(off)

#include "posterior_bodies.h"
#include "prepare_bodies.h"

using namespace rcb;

namespace {

struct StepBeginArgs {
  const float* table;
  long long n_steps;
  const long long* step;
  float* dyn;
  long long* kl_slots;
};

// blocks [0, n_pack): the packed images of the A matrices; [n_pack, n_pack + n_weff): the phase-form conv weights; the
// last block: the step's bookkeeping.  The three read different inputs and write different outputs: no ordering needed.
__global__ void __launch_bounds__(256) step_prepare_kernel(PackArgs pk, int n_pack, WeffArgs wf, int n_weff, StepBeginArgs sb) {
  const int blk = blockIdx.x;
  if (blk < n_pack) {
    atrans_pack_body(pk, blk);
  } else if (blk < n_pack + n_weff) {
    weff_build_body(wf, blk - n_pack);
  } else {
    step_begin_body<256>(sb.table, sb.n_steps, sb.step, sb.dyn, sb.kl_slots);
  }
}

struct StepEndArgs {
  const float* sse;
  int n_sse;
  double mse_scale;
  const long long* kl_slots;
  double* mse_log;
  double* kl_log;
  long long n_log;
  long long* step;
  long long* aux_counter;
  unsigned* tickets;     // [RCB_STEP_TAIL_TICKETS]: zero on entry, zero on exit
};

constexpr int kTicketGroups = RCB_STEP_TAIL_TICKETS - 1;

// blocks [0, n_post): the lpe level's posterior update, block for block the launch of posterior_flat_kernel (a block's KL
// sum is rounded to fixed point once: the contributions are that launch's only if the blocks are); [n_post, n_post +
// n_adam): Adam on the mappings.  The step's log entry needs every block's KL contribution and bumps the counters the
// posterior blocks read (the noise counter): it is written by the posterior workgroup that finishes LAST.  The Adam blocks
// share nothing with it (they read the Adam scalars and their own tensors) and take no part.  Every posterior workgroup
// draws a ticket -- in two levels, 64 group counters and one on top, because a few thousand device-scope atomics on ONE
// address queue up behind each other at the memory side -- and whoever draws a counter's last ticket puts it back to zero
// (the launch is replayed).  No fences (rcb_common.h, "the workgroup that finishes last"): a block's only output the
// epilogue reads is its KL contribution, an agent-scope integer atomic issued by thread 0, which waits for its completion
// before it draws the ticket; the epilogue reads the slots with agent-scope atomic loads.  The other direction -- the
// epilogue overwrites the noise counter the posterior blocks read -- is safe because a block reaches its barrier only after
// every thread has issued its stores, which need the loaded value.
// (84 registers = five waves per SIMD against the six of posterior_flat_kernel alone; forcing six costs 20 bytes of
// scratch per lane and measured 9 us SLOWER per step on the same box: left as the compiler allocates it)
__global__ void __launch_bounds__(256)
step_tail_kernel(PostBwdArgs post, long long n_total, int n_post, AdamMultiArgs adam, StepEndArgs se) {
  __shared__ int s_last;
  const int blk = blockIdx.x;
  if (blk >= n_post) {
    adam_multi_body(adam, blk - n_post);
    return;
  }
  posterior_flat_body(post, n_total, (unsigned)blk, (unsigned)n_post);
  __syncthreads();
  if (threadIdx.x == 0) {
    vmem_wait_all();
    const int g = blk % kTicketGroups;
    const unsigned in_group = (unsigned)((n_post - g + kTicketGroups - 1) / kTicketGroups);
    const unsigned groups = (unsigned)(n_post < kTicketGroups ? n_post : kTicketGroups);
    bool last = atomicAdd(se.tickets + 1 + g, 1u) == in_group - 1;
    if (last) {
      agent_store(se.tickets + 1 + g, 0u);
      last = atomicAdd(se.tickets, 1u) == groups - 1;
    }
    s_last = last;
  }
  __syncthreads();
  if (!s_last) return;
  step_end_body<256, true>(se.sse, se.n_sse, se.mse_scale, se.kl_slots, se.mse_log, se.kl_log, se.n_log, se.step, se.aux_counter);
  if (threadIdx.x == 0) se.tickets[0] = 0;
}

inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace

extern "C" int rcb_step_prepare(const float* adam_table, int64_t n_steps, const int64_t* step, float* dyn, int64_t* kl_slots,
                                const float* const* A, int32_t n_layers, const int32_t* sizes, void* packed, int32_t want_lo,
                                const float* W1, const float* b1, const float* W2, const float* W3, void* weff1, void* b1rep,
                                int32_t bf16_out, float* weff2, float* weff3, void* frag_pack, rcb_stream_t stream) {
  RCB_REQUIRE(adam_table && step && dyn && n_steps >= 1, RCB_ERR_ARG, "step_prepare: null pointer / empty table");
  RCB_REQUIRE(A && sizes && packed && n_layers >= 1 && n_layers <= RCB_ATRANS_MAX_LAYERS, RCB_ERR_ARG,
              "step_prepare: bad arguments (%d layers)", n_layers);
  RCB_REQUIRE(al16(packed), RCB_ERR_ARG, "step_prepare: packed buffer must be 16-byte aligned");
  for (int l = 0; l < n_layers; ++l) RCB_REQUIRE(A[l] && sizes[l] >= 1, RCB_ERR_ARG, "step_prepare: layer %d null / empty", l);
  RCB_REQUIRE(W1 && b1 && W2 && W3 && weff1 && b1rep && weff2 && weff3, RCB_ERR_ARG, "step_prepare: null conv tensor");
  PackArgs pk;
  const int n_pack = fill_pack_args(pk, A, n_layers, sizes, packed, want_lo);
  const WeffArgs wf{W1, b1, W2, W3, weff1, b1rep, weff2, weff3, bf16_out ? 1 : 0, reinterpret_cast<uint4*>(frag_pack)};
  const int n_weff = weff_build_blocks(frag_pack != nullptr);
  const StepBeginArgs sb{adam_table, (long long)n_steps, (const long long*)step, dyn, (long long*)kl_slots};
  step_prepare_kernel<<<n_pack + n_weff + 1, 256, 0, (hipStream_t)stream>>>(pk, n_pack, wf, n_weff, sb);
  RCB_LAUNCH_CHECK();
  return RCB_OK;
}

// 1 if rcb_posterior_bwd would take its flat fast path for this level (the only form rcb_step_tail combines)
extern "C" int rcb_step_tail_eligible(const rcb_level_bwd* lv) {
  if (!lv || !lv->loc || !lv->log_scale || !lv->p_loc || !lv->p_scale || lv->rows <= 0 || lv->cols <= 0) return 0;
  const long long n_total = (long long)lv->rows * lv->cols;
  const bool want_next = lv->next_out || lv->next_out_bf16;
  if (!(lv->d_out && lv->samples == 1 && lv->cols_out == lv->cols && !lv->enc_mask && !lv->beta && !lv->member_ptr && !lv->row_perm_inv &&
        !lv->col_inv && !lv->g_loc && !lv->g_log_scale && (n_total & 3) == 0 && al16(lv->loc) && al16(lv->log_scale) && al16(lv->d_out) &&
        (lv->eps_from_rng ? (lv->rng_step_dev && !lv->eps) : (lv->eps && al16(lv->eps))) && lv->m_loc && lv->v_loc && lv->m_ls && lv->v_ls &&
        al16(lv->m_loc) && al16(lv->v_loc) && al16(lv->m_ls) && al16(lv->v_ls)))
    return 0;
  if (lv->next_out_lo && !lv->next_out_bf16) return 0;
  if (want_next && !(lv->rng_step_dev && al16(lv->next_out) && al16(lv->next_eps) && (lv->next_out || lv->next_out_lo) &&
                     (!lv->next_out_bf16 || lv->next_ld_bf16 >= lv->cols)))
    return 0;
  return ((n_total >> 2) + 255) / 256 < (1LL << 30) ? 1 : 0;
}

extern "C" int rcb_step_tail(const rcb_level_bwd* lv, const rcb_adam_cfg* cfg, const rcb_adam_tensor* tensors, int32_t count,
                             const float* sse, int32_t n_sse, double mse_scale, double* mse_log, double* kl_log, int64_t n_log,
                             int64_t* step, int64_t* aux_counter, uint32_t* tickets, rcb_stream_t stream) {
  RCB_REQUIRE(lv && cfg && tensors && step && tickets, RCB_ERR_ARG, "step_tail: null pointer");
  RCB_REQUIRE(cfg->step >= 1, RCB_ERR_ARG, "step_tail: step must be >= 1");
  RCB_REQUIRE(rcb_step_tail_eligible(lv), RCB_ERR_UNSUPPORTED,
              "step_tail: the level does not take the flat fast path of rcb_posterior_bwd (use the separate launches)");
  RCB_REQUIRE(count >= 1 && count <= RCB_ADAM_MAX_TENSORS, RCB_ERR_ARG, "step_tail: %d tensors (1..%d)", count, RCB_ADAM_MAX_TENSORS);
  RCB_REQUIRE(n_sse >= 0 && n_log >= 0, RCB_ERR_SHAPE, "step_tail: negative size");
  PostBwdArgs post;
  post.L = *lv;
  post.adam = make_adam(cfg);
  const long long n_total = (long long)lv->rows * lv->cols;
  const int n_post = cdiv(n_total >> 2, 256);           // the grid of posterior_flat_kernel (uncapped): one trip per workgroup
  AdamMultiArgs ad;
  memset(&ad, 0, sizeof(ad));
  long long blocks = 0;
  for (int t = 0; t < count; ++t) {
    const rcb_adam_tensor& x = tensors[t];
    RCB_REQUIRE(x.n >= 0 && (x.n == 0 || (x.p && x.g && x.m && x.v)), RCB_ERR_ARG, "step_tail: tensor %d has a null pointer", t);
    ad.p[t] = x.p; ad.g[t] = x.g; ad.m[t] = x.m; ad.v[t] = x.v; ad.n[t] = x.n;
    ad.blk_start[t] = (int)blocks;
    blocks += (x.n + 1023) / 1024;
    RCB_REQUIRE(blocks < (1LL << 30), RCB_ERR_SHAPE, "step_tail: too many elements");
  }
  RCB_REQUIRE(blocks >= 1, RCB_ERR_ARG, "step_tail: nothing for Adam to update");
  ad.blk_start[count] = (int)blocks;
  ad.count = count;
  ad.s = post.adam;
  const StepEndArgs se{sse, n_sse, mse_scale, (const long long*)lv->kl_accum, mse_log, kl_log, (long long)n_log,
                       (long long*)step, (long long*)aux_counter, tickets};
  step_tail_kernel<<<n_post + (int)blocks, 256, 0, (hipStream_t)stream>>>(post, n_total, n_post, ad, se);
  RCB_LAUNCH_CHECK();
  return RCB_OK;
}
