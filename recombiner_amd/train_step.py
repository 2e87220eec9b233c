"""The training step behind PriorBNNmodel.train: every decision about what a step launches (StepPlan, computed in one place:
plan_step), the buffers and captured graphs that survive across train() calls (the workspace dict `model._ws`, keyed by the
plan plus the shapes, strides and storage addresses the kernels were recorded with -- a switch that changes what gets
captured cannot be missing from the key) and the step itself (PriorTrainStep), eager or as captured HIP graph(s)."""
import collections
import os
import types

import torch

from . import dist as rdist
from . import ops
from .upsample_fast import hip_path_supported

N_WARM = 3              # eager steps in front of the capture

# stream forks inside the (captured) step -- bit mask, same kernels on the same operands, so results are identical:
#   2: the A transform's backward beside the upsampling net's backward;  4: the weight-gradient side of the upsampling net's
#   backward beside its data path (upsample_cifar_hip(weight_side_stream=));  8 (with 2): the network level's posterior update
#   right behind the A transform's backward on the forked stream (it only needs dh)
FORK_A_BACKWARD, FORK_WEIGHT_SIDE, FORK_NET_UPDATE = 2, 4, 8

# the model's switches that enter the plan as they are; then the call's shapes and arguments, the environment, and what
# plan_step derives from all of them (each field is assigned exactly once there, with its meaning)
SWITCHES = ("precision", "patch", "lowp_gemm", "split_gemm", "split_terms", "split_dgrad_terms", "wgrad_bf16", "stage1_bf16",
            "pe_bf16", "fused_noise", "fuse_next_sample", "operand_planes", "redraw_noise", "hier_rng", "rng_row_offset",
            "rng_seed_override", "force_segments", "capture_collectives")
StepPlan = collections.namedtuple("StepPlan", SWITCHES + (
    "n", "n_pix", "n_out", "lr", "training_mappings", "world", "graphable", "fork_mask", "step_fused_env", "upconv_fwd_fused",
    "posterior_wg_per_cu",
    "lowp", "split", "sharded", "rng_lpe", "use_rng", "rng_hier", "goff_net", "goff_lpe", "want16", "lpe16_want", "fuse_next",
    "fuse_lpe", "planes", "redraw", "redraw_lpe", "pe_stitched", "capture_coll", "one_graph", "update_last", "fork_bwd",
    "fork_wside", "fork_update", "fused_step", "fused_head", "fused_tail"))


def plan_step(model, levels, y, lr, training_mappings, upsample_net, verbose=False):
    """the StepPlan (hashable: the first element of the workspace key) of one train() call, from the model's switches
    (`levels` = model._levels()), the call's arguments and the environment"""
    m, (net, lpe_lv) = model, levels
    cuda = m.loc.device.type == "cuda"
    D, d_lpe = m._d_net, m._d_lpe
    p = types.SimpleNamespace(**{k: getattr(m, k) for k in SWITCHES})
    N = p.n = y.shape[0]                                     # INRs; pixels per INR, output channels
    p.n_pix, p.n_out = y.shape[1], y.shape[2]
    p.lr, p.training_mappings = float(lr), bool(training_mappings)
    # Gradients of the shared mappings are summed over ranks only when the caller asked for it by setting `dp_group`
    # (drivers.train_prior and bench.py do): an initialised process group alone must not couple models that merely
    # live in the same job (several priors / bit-rates trained side by side).
    p.world = torch.distributed.get_world_size(m.dp_group) if m.dp_group is not None else 1
    # the step may be captured, and its workspace kept on the model
    p.graphable = bool(m.use_graph and m.noise_source is None and cuda and not verbose)
    # stream_forks, or RCB_FORK when set (0 off the GPU)
    mask = int(os.environ.get("RCB_FORK", str(m.stream_forks)))
    if mask & ~(FORK_A_BACKWARD | FORK_WEIGHT_SIDE | FORK_NET_UPDATE):
        raise ValueError(f"stream_forks / RCB_FORK = {mask}: only combinations of the bits 2 (A-transform backward on a second "
                         "stream), 4 (weight-gradient side of the upsampling net's backward on a third) and 8 (network level's "
                         "posterior update behind the A-transform backward) exist; the orderings behind the bits 1, 16, 32 and "
                         "64 measured no gain or a loss and were removed (DESIGN.md section 4.5 and its round-4 appendix)")
    p.fork_mask = mask if cuda else 0
    p.step_fused_env = os.environ.get("RCB_STEP_FUSED", "1")
    # stages 2 + 3 of the upsampling net's forward as one launch (upsample_cifar_hip(fwd_fused=); same bits): on unless
    # RCB_UPCONV_FWD_FUSED=0.  A plan field: a graph captured under one setting is never replayed under the other
    p.upconv_fwd_fused = bool(ops.upconv_fwd23_enabled())
    # (read by the posterior kernels' launcher when the library loads; rules the combined launches out)
    p.posterior_wg_per_cu = os.environ.get("RCB_POSTERIOR_WG_PER_CU", "0")
    p.lowp = bool(m.lowp_gemm and m.precision != 0)           # the A transform as library GEMMs on 16-bit operands
    # 16-bit modes: the A transform on the hand-written kernels of atrans.hip (ops.ATransform; every geometry)
    p.split = bool(m.split_gemm and m.precision != 0 and not m.lowp_gemm)
    # sharded: the mapping gradients of a step travel in two buckets of one flat buffer (dist.GradBuckets)
    p.sharded = bool(p.training_mappings and (p.world > 1 or (m.force_segments and m.dp_group is not None)))
    # in-kernel noise: a pure function of (seed, stream, counter, element); the counter lives in the workspace and is
    # never reset, so every step of every train() call draws fresh noise, replayed or not
    # (the lpe is a single plain level in every preset; the latent weights are one only without patches: the three-level
    # presets keep stored noise for the weights and draw the lpe's -- two thirds of what they sample -- in the kernels)
    p.rng_lpe = bool(m.fused_noise and m.noise_source is None and ops.rng_eligible(lpe_lv))
    p.use_rng = bool(p.rng_lpe and len(net) == 1 and ops.rng_eligible(net[0]))
    # three levels of latent weights (patched presets): every level's noise drawn in the sampling kernel (Philox streams 0, 2, 3
    # at the element index of the [N, D] noise arrays: independent of torch's generator and of how the rows are sharded) and
    # written for the posterior updates, instead of three randn launches read back by the kernel
    p.rng_hier = bool(m.hier_rng and p.rng_lpe and not p.use_rng and ops.hier_rng_eligible(net) and (N * D) % 4 == 0
                      and (m.rng_row_offset * D) % 4 == 0)
    # Philox group of this model's first row inside the larger (virtual) batch (PriorBNNmodel.rng_row_offset)
    p.goff_net = ops.rng_group_offset(m.rng_row_offset, D) if (p.use_rng or p.rng_hier) else 0
    p.goff_lpe = ops.rng_group_offset(m.rng_row_offset, d_lpe) if p.rng_lpe else 0
    p.want16 = bool(p.split and p.training_mappings and m.wgrad_bf16)     # bf16 operands of the weight gradient
    p.lpe16_want = bool(p.use_rng and m.stage1_bf16 and m.precision != 0 and not m.patch)     # bf16 copy of the lpe: stage-1 operand
    # the posterior updates of step t write the sample of step t + 1: both levels / the lpe level
    # (the fused form lives on the posterior update's flat path: element counts divisible by 4)
    p.fuse_next = bool(p.use_rng and m.fuse_next_sample and (N * D) % 4 == 0 and (N * d_lpe) % 4 == 0)
    p.fuse_lpe = bool(p.fuse_next or (p.rng_lpe and m.fuse_next_sample and (N * d_lpe) % 4 == 0))
    # the A transform's operands as (hi, lo) planes written by their producers (single-level presets with in-kernel noise;
    # layers must start at multiples of 8 columns for the 16-byte LDS-DMA pieces)
    p.planes = bool(p.split and p.use_rng and m.operand_planes
                    and all(lo % 8 == 0 for (lo, hi) in m._layer_slices() if (hi - lo) % 8 == 0))
    # the updates re-draw their step's noise from the counter instead of reading a stored copy
    p.redraw, p.redraw_lpe = bool(p.fuse_next and m.redraw_noise), bool(p.fuse_lpe and m.redraw_noise)
    p.pe_stitched = m._pe_layout() is not None          # pe stays on the stitched grids (PriorBNNmodel._pe_layout)
    # sharded step: with RCCL the two all-reduces are CAPTURED inside the one step graph (measured on this stack: an
    # all-reduce captures and replays correctly from the capturing stream and from a forked one, tools/rccl_capture_probe.py;
    # the four-segment form costs 142 us of host work per 1.09 ms step, bench.py `sharded_step_host_cost`); other
    # backends (gloo: the CPU rehearsals) keep the four captured segments around host-enqueued collectives
    # Default (capture_collectives None): captured on a ONE-rank RCCL communicator only -- that is all this form has ever
    # run on (the pool has one GPU per box).  With more ranks the four-segment form runs unless RCB_CAPTURE_COLLECTIVES=1
    # (or capture_collectives=True) opts in; bench.py's launcher sets it after an N-rank tools/rccl_capture_probe.py run
    # succeeded within its timeout, so that the first N > 1 execution of the captured form is never the measured one.
    p.capture_coll = bool(p.sharded and m.capture_collectives is not False
                          and (m.capture_collectives is True
                               or (torch.distributed.get_backend(m.dp_group) == "nccl" and p.world == 1)))
    # one rank / frozen mappings / captured collectives: the whole step is one graph (else four around the all-reduces)
    p.one_graph = bool(not p.sharded or p.capture_coll)
    # the network level's update is the step's last big kernel (PriorTrainStep.body)
    p.update_last = bool((p.fuse_next and not p.sharded) or p.capture_coll)
    # which of the fork bits apply: 2 needs the hand-written A transform and the fused next sample, 8 needs 2
    p.fork_bwd = bool((p.fork_mask & FORK_A_BACKWARD) and p.split and p.one_graph and p.fuse_next)
    p.fork_wside = bool(p.fork_mask & FORK_WEIGHT_SIDE)
    p.fork_update = bool(p.fork_bwd and (p.fork_mask & FORK_NET_UPDATE))
    # Combined launches (csrc/step_fused.hip) where the step is the one-rank form with the mappings trained -- the first
    # branch of body() -- and the kernels they combine are the ones this configuration runs anyway:
    #   head: step_begin + the pack of the A matrices + the phase-form conv weights (ops.step_prepare);
    #   tail: the lpe level's update + Adam on the mappings + step_end (ops.step_tail), behind the join with the forked
    #         stream (the network level's KL slots are an input).  A step whose network-level update is not on the forked
    #         stream keeps the separate launches.
    # Same bodies, same bits; RCB_STEP_FUSED=0 forces the separate launches (tests, same-box A/B).
    p.fused_step = bool(ops.step_fused_enabled() and cuda and p.fuse_next and not p.sharded and p.training_mappings)
    p.fused_head = bool(p.fused_step and p.split and m.precision != 0 and not p.pe_stitched
                        and hip_path_supported(upsample_net, m.pixel_sizes, m.upsample_factors, m.patch, m.data_dim))
    p.fused_tail = bool(p.fused_step and p.fork_update)
    return StepPlan(**vars(p))          # (a field misspelt or forgotten above is a TypeError here)


# what the segments of a step hand on (return values: nothing about a step outlives it)
#   seg1a -> _Forward: sse; dh3 = gradient of the latent weights' sample [N, 1, D]; eps = their noise per level (None: re-drawn by
#     the update); e_lpe; gA = gradients of the A matrices (views of bucket 0 in the sharded step); h0 = Work handle of
#     bucket 0's captured all-reduce, or None
#   seg1a -> _Tape: the upsampling net's autograd graph of the step (lpe_t -> pe_c) and the gradient dpe that enters it.  It must not
#     outlive seg1b: a graph kept alive from an eager warm-up step (default stream) into the capture (side stream) makes
#     its AccumulateGrad nodes cross streams and breaks the capture
#   seg1b -> _Backward: d_lpe; grads = gradients of A + conv in parameter order (None: fixed mappings); h1 like h0, bucket 1
_Forward = collections.namedtuple("_Forward", "sse dh3 eps e_lpe gA h0")
_Tape = collections.namedtuple("_Tape", "lpe_t pe_c dpe")
_Backward = collections.namedtuple("_Backward", "d_lpe grads h1")


class PriorTrainStep:
    """One train() call's view of the step: the plan, the workspace (found on the model when its key still holds, else built)
    and the model, mappings and data the kernels read."""
    # The step runs as four segments so that, under data-parallel sharding, the gradient bucket of the shared mappings is
    # all-reduced asynchronously BETWEEN captured graphs while work that does not depend on it proceeds:
    #   seg1a: sample .. SIREN .. A-transform backward | all-reduce(A grads, 13.4 MB) ||
    #   seg1b: upsampling-net backward | all-reduce(conv grads, 1 MB) || seg2: posterior update | wait |
    #   seg3: Adam on the mappings + bookkeeping.

    def __init__(self, model, n_epoch, lr, x, y, priors, linear_transform, upsample_net, training_mappings, verbose):
        self.model, self.x, self.y, self.upsample_net = model, x, y, upsample_net
        self.A = [a for a in linear_transform.A]
        self.conv = [p for p in upsample_net.parameters()]
        self.net, self.lpe_lv = model._levels()
        self.plan = plan = plan_step(model, (self.net, self.lpe_lv), y, lr, training_mappings, upsample_net, verbose)
        self.slices = model._layer_slices()
        self.dev = model.loc.device
        self.pe_lay = model._pe_layout() if plan.pe_stitched else None
        # Everything a captured step references lives in a workspace that survives across train() calls: Adam state
        # (re-zeroed per call = the reference's fresh optimiser), step counter, logs, and device copies of what changes
        # between calls (priors, beta, the noise counter).  The EM loop calls train() 550 times with 100 steps each;
        # re-capturing the graph every call costs ~14 ms = 9 % of such a call, replaying a cached one nothing.
        key = (plan, x.data_ptr(), tuple(x.shape), tuple(x.stride()), y.data_ptr(), id(linear_transform), id(upsample_net),
               tuple(None if q is None else tuple(q.shape) for q in priors),
               # the captured kernels read and Adam-update these STORAGES: Module.cpu()/.to() (a checkpoint written the
               # reference's way, main_prior_training.py:334-338) re-allocates param.data while id() stays equal
               tuple(q.data_ptr() for q in self.A + self.conv), tuple(q.data_ptr() for q in model.parameters()))
        ws = model._ws if plan.graphable else None
        if ws is not None and (ws["key"] != key or ws["rows"] < n_epoch):
            ws = None
        if ws is None:
            ws = self._new_workspace(key, n_epoch, priors)
            if plan.graphable:
                model._ws = ws
        else:
            ws["state_flat"].zero_()
        self.ws = ws
        self.split, self.flat = ws["split"], ws["flat"]
        self.fork, self.side = ws.get("fork_stream"), ws.get("side_stream")
        self.smp_net, self.smp_lpe = ws.get("smp_net"), ws.get("smp_lpe")
        self.rng_seed = ws["seed"] if plan.rng_seed_override is None else int(plan.rng_seed_override) & (2 ** 64 - 1)
        pri = ws["pri"]                # what the kernels read (stable addresses); `priors` = this call's values
        self.net_priors = [(pri[0], pri[1])] + ([(pri[4], pri[5]), (pri[6], pri[7])] if model.patch else [])
        # per-step Adam scalars and the step counter live on the device, so that one captured HIP graph of the
        # step body can be replayed for every step (the host launch cost of ~60 kernels is ~2 ms per step)
        self.cfg = ops.adam_cfg(plan.lr, 1, dyn=ws["dyn"])
        self.mse_scale = 1.0 / (plan.n_pix * plan.n_out)

    def _new_workspace(self, key, n_epoch, priors):
        m, p, dev, net, lpe_lv, AC = self.model, self.plan, self.dev, self.net, self.lpe_lv, self.A + self.conv
        # all Adam moments (per-INR levels and shared mappings) as views of ONE zero-filled buffer: a train() call resets
        # them with one launch instead of ~30 (the reference creates a fresh optimiser per call: main_prior_training.py)
        shapes = [lv.loc.shape for lv in net for _ in range(4)] + [lpe_lv.loc.shape] * 4
        if p.training_mappings:
            shapes += [q.shape for q in AC for _ in range(2)]
        state_flat, views = ops.zeroed_views(shapes, dev)

        def st4(lv):
            return {k: next(views) for k in ("m_loc", "v_loc", "m_ls", "v_ls")}
        rows = max(n_epoch, 256) if p.graphable else n_epoch
        rank_id = torch.distributed.get_rank(m.dp_group) if m.dp_group is not None else 0    # ranks must not draw the same noise
        m._train_calls += 1
        ws = dict(key=key, rows=rows, state_flat=state_flat, net_state=[st4(lv) for lv in net], lpe_state=st4(lpe_lv),
                  map_state=[(next(views), next(views)) for q in AC] if p.training_mappings else None,
                  tab=ops.adam_table(p.lr, rows).to(dev), dyn=torch.zeros(2, device=dev, dtype=torch.float32),
                  step_t=torch.zeros(1, device=dev, dtype=torch.long),
                  kl_slots=torch.zeros(1024, device=dev, dtype=torch.int64),       # fixed point, 2^-24 nats
                  tickets=torch.zeros(ops.STEP_TAIL_TICKETS, device=dev, dtype=torch.int32),     # rcb_step_tail: zero between launches
                  mse_buf=torch.zeros(rows, device=dev, dtype=torch.float64),
                  kl_buf=torch.zeros(rows, device=dev, dtype=torch.float64),
                  pri=[None if q is None else torch.empty_like(q) for q in priors],
                  beta_dev=torch.zeros(1, device=dev, dtype=torch.float32),
                  rng_ctr=torch.full((1,), int(m._rng_ctr_init), device=dev, dtype=torch.long), graphs=None,
                  seed=(int(m.random_seed) * 0x9E3779B97F4A7C15 + int(torch.initial_seed()) * 0xBF58476D1CE4E5B9
                        + m._train_calls * 0x94D049BB133111EB + rank_id * 0xD6E8FEB86659FD93) & (2 ** 64 - 1),
                  # sharded: the mapping gradients of a step travel in two buckets of one flat buffer (dist.GradBuckets)
                  flat=(rdist.GradBuckets([q.shape for q in self.A], [q.shape for q in self.conv], dev, m.dp_group)
                        if p.sharded else None),
                  # the bf16 copy of the coordinate grid the captured SIREN launches read: owned by the workspace,
                  # i.e. alive exactly as long as the graphs that reference its address
                  xf16=ops.xf_bf16(self.x, p.precision) if (p.precision in (1, 2) and dev.type == "cuda") else None)
        # 16-bit modes: the A transform on the hand-written kernels of atrans.hip (every geometry)
        ws["split"] = ops.ATransform(self.slices, dev, p.split_terms, p.split_dgrad_terms) if p.split else None
        # the samples the posterior updates write for the next step, the planes of h_w, the stored noise of the three levels
        if p.fuse_next:
            ws["smp_net"] = ops.sample_buffers(net[0], True, planes=p.planes, want_eps=not p.redraw)
            ws["smp_lpe"] = ops.sample_buffers(lpe_lv, True, want_eps=not p.redraw)
        elif p.fuse_lpe:
            ws["smp_lpe"] = ops.sample_buffers(lpe_lv, p.lpe16_want, want_eps=not p.redraw_lpe)
        elif p.planes:
            ws["smp_net"] = ops.sample_buffers(net[0], planes=True)
        if p.rng_hier:
            ws["hier_eps"] = [torch.empty(p.n, 1, m._d_net, device=dev, dtype=torch.float32) for _ in net]
        if p.fork_mask:
            ws["fork_stream"], ws["side_stream"] = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        return ws

    def prime(self, kl_beta, priors):
        """per call: reset the step counter, load beta and the priors, pack fixed mappings, draw the first step's sample"""
        ws, p = self.ws, self.plan
        ws["step_t"].zero_()
        ws["beta_dev"].fill_(float(kl_beta))
        for dst, src in zip(ws["pri"], priors):
            if dst is not None:
                dst.copy_(src)
        if self.split is not None and not p.training_mappings:
            self.split.prepare(self.A)                # fixed mappings: packed once per call, outside the captured step
        if p.fuse_lpe:
            # the sample of the call's first step (every later one comes out of the previous step's posterior update)
            if p.fuse_next:
                ops.reparam_rng(self.net[0], self.rng_seed, 0, ws["rng_ctr"], want_bf16=p.want16, buffers=self.smp_net,
                                group_offset=p.goff_net)
            ops.reparam_rng(self.lpe_lv, self.rng_seed, 1, ws["rng_ctr"], want_bf16=p.lpe16_want, buffers=self.smp_lpe,
                            group_offset=p.goff_lpe)

    # ---- seg1a: head, the two forward maps, SIREN loss + backward, A-transform backward ---------------------------------
    # the step's first launch -> the phase-form conv weights when it built them (in _UpsampleCifarFn's cache form)
    def head(self):
        ws, p, up = self.ws, self.plan, self.upsample_net
        if p.fused_head:
            c1, c2, c3 = up.conv1, up.conv2, up.conv3
            return {("weff", bool(p.stage1_bf16)): ops.step_prepare(ws["tab"], ws["step_t"], ws["dyn"], ws["kl_slots"], self.split,
                                                                    self.A, c1.weight, c1.bias, c2.weight, c3.weight, p.stage1_bf16)}
        ops.step_begin(ws["tab"], ws["step_t"], ws["dyn"], ws["kl_slots"])
        return None

    # ---- lpe sample -> upsampling net (under autograd) -> (lpe_t, e_lpe, pe_c)
    def pe_forward(self, weff_cache):
        m, p, N, lpe_lv, rng_ctr = self.model, self.plan, self.plan.n, self.lpe_lv, self.ws["rng_ctr"]
        lpe16 = None
        if p.fuse_lpe:                   # written by the previous step's posterior update (or by prime() before the first)
            smp = self.smp_lpe
            lpe, e_lpe, lpe16 = smp[0], smp[1], (smp[2][:, :lpe_lv.cols] if p.lpe16_want else None)
        elif p.rng_lpe:                  # (with lpe16_want also the bf16 copy: stage-1 operand)
            lpe, e_lpe, *o16 = ops.reparam_rng(lpe_lv, self.rng_seed, 1, rng_ctr, want_bf16=p.lpe16_want, group_offset=p.goff_lpe)
            lpe16 = o16[0] if o16 else None
        else:
            e_lpe = m._noise((N, 1, m._d_lpe))
            lpe = ops.reparam_fwd([lpe_lv], [e_lpe], 1)
        lpe_t = lpe.view(1, N, *m._lat, m.latent_dim).requires_grad_(True)
        with torch.enable_grad():
            if self.pe_lay is not None:                                  # stitched grids, addressed in place by the kernel
                pe_c = m._pe(self.upsample_net, lpe_t, stitched=True)
            else:
                pe = m._pe(self.upsample_net, lpe_t, lpe16=lpe16, weff_cache=weff_cache,
                           weight_side_stream=self.side if p.fork_wside else None, fwd_fused=p.upconv_fwd_fused)      # [N, 1, P, E]
                pe_c = pe.reshape(N, pe.shape[2], pe.shape[3]).contiguous()   # (not pe[:, 0]: select's backward
                #                                                               materialises zeros + a copy)
        return lpe_t, e_lpe, pe_c

    # ---- latent weights' sample -> A transform -> (h_w, h16, eps, wvec, A16)
    def net_forward(self):
        m, p, ws, net, split, A, slices = self.model, self.plan, self.ws, self.net, self.split, self.A, self.slices
        N, D, rng_ctr = p.n, m._d_net, ws["rng_ctr"]
        h16 = A16 = None
        if p.planes:                     # h_w as its (hi, lo) planes: from the previous step's update, or sampled here
            if not p.fuse_next:
                ops.reparam_rng(net[0], self.rng_seed, 0, rng_ctr, buffers=self.smp_net, group_offset=p.goff_net)
            h_w, eps = self.smp_net[2], [self.smp_net[1]]
        elif p.fuse_next:
            h_w, e0, h16 = self.smp_net[0], self.smp_net[1], (self.smp_net[2][:, :D] if p.want16 else None)
            eps, h_w = [e0], h_w.view(N, D)
        elif p.use_rng:
            h_w, e0, *o16 = ops.reparam_rng(net[0], self.rng_seed, 0, rng_ctr, want_bf16=p.want16, group_offset=p.goff_net)
            eps, h_w, h16 = [e0], h_w.view(N, D), (o16[0] if o16 else None)
        elif p.rng_hier:
            eps = ws["hier_eps"]
            h_w = ops.reparam_hier_rng(net, eps, self.rng_seed, (0, 2, 3)[:len(net)], rng_ctr, p.goff_net).view(N, D)
        else:
            eps = [m._noise((N, 1, D)) for _ in net]
            h_w = ops.reparam_fwd(net, eps, 1).view(N, D)
        # ---- A transform (dense GEMMs) --------------------------------------------------------------
        if p.lowp:
            # forward: f16 operands (11-bit mantissa; A pre-scaled by 2^10 so that the ~1e-4 products of
            # h_w @ A stay in f16's normal range) -- finer than the bf16 rounding the MLP kernel applies to
            # its weights anyway; backward GEMMs: bf16 operands (range-safe, gradients only)
            hf = h_w.to(torch.float16)
            wvec = torch.cat([torch.mm(hf[:, lo:hi], (a.detach() * 1024.0).to(torch.float16))
                              for (lo, hi), a in zip(slices, A)], 1).float() * (1.0 / 1024.0)
            h16 = h_w.to(torch.bfloat16)
            A16 = [a.detach().to(torch.bfloat16) for a in A]
        elif split is not None:
            if p.training_mappings and not p.fused_head:
                split.prepare(A)                  # the mappings change every step when they are trained
            wvec = split.forward(h_w, split.new_rows(N))
        else:
            wvec = ops.a_transform_mm(h_w, A, slices, torch.empty(N, D, device=self.dev, dtype=torch.float32))
        return h_w, h16, eps, wvec, A16

    # ---- fused SIREN forward + MSE + backward -> (sse, dw, dpe, dw16)
    def siren(self, pe_c, wvec):
        p, x, xf16 = self.plan, self.x, self.ws["xf16"]
        meta = self.model._meta(x, pe_c.shape[-1])
        dw16 = None
        if p.planes:        # the gradient leaves the kernel as its (hi, lo) planes: the A transform's operand form
            sse, _, dpe, dw = ops.siren_loss_bwd(x, pe_c.detach(), wvec, self.y, self.mse_scale, meta, want_planes=True,
                                                pe_layout=self.pe_lay, xf16=xf16)
        else:               # with want16 the kernel's epilogue also writes the bf16 copy of the gradient
            sse, dw, dpe, *o16 = ops.siren_loss_bwd(x, pe_c.detach(), wvec, self.y, self.mse_scale, meta, want_bf16=p.want16,
                                                    pe_layout=self.pe_lay, xf16=xf16)
            dw16 = o16[0] if o16 else None
        return sse, dw, dpe, dw16

    # ---- backward through the A transform (first: its gradients are the bulk of the all-reduce bucket)
    # -> (dh, gA, h0, keep); `keep`: see body()
    def a_backward(self, h_w, h16, dw, dw16, A16):
        p, split, flat, slices, N, D = self.plan, self.split, self.flat, self.slices, self.plan.n, self.model._d_net
        gA, h0, keep = [], None, None
        if p.fork_bwd:      # the A transform's backward on the second stream beside the upsampling net's backward
            self.fork.wait_stream(torch.cuda.current_stream())
            keep = (dw, dw16, h_w, h16)
        with torch.cuda.stream(self.fork if p.fork_bwd else None):        # (None: the current stream)
            if split is not None:
                dh = split.dgrad(dw, torch.empty(N, D, device=self.dev, dtype=torch.float32))
                if p.training_mappings:
                    gA = split.wgrad(h_w, dw, h16, dw16, p.wgrad_bf16)
            elif p.lowp:
                dw16 = dw.to(torch.bfloat16)
                dh = torch.cat([torch.mm(dw16[:, lo:hi], a16.t()) for (lo, hi), a16 in zip(slices, A16)], 1).float()
                if p.training_mappings:
                    gA = [torch.mm(h16[:, lo:hi].t(), dw16[:, lo:hi]).float() for (lo, hi) in slices]
            else:
                dh = ops.a_transform_mm(dw, self.A, slices, torch.empty(N, D, device=self.dev, dtype=torch.float32), transpose=True)
                if p.training_mappings:
                    gA = [torch.mm(h_w[:, lo:hi].t(), dw[:, lo:hi]) for (lo, hi) in slices]
            if p.training_mappings and flat is not None:
                gA = flat.pack(0, gA)
                if p.capture_coll:  # bucket 0 (13.4 of the 14.4 MB) leaves from this stream (forked or not), inside the graph
                    h0 = flat.reduce(0, async_op=True)
        return dh, gA, h0, keep

    def seg1a(self):
        """-> (_Forward, _Tape, keep)"""
        weff_cache = self.head()
        # ---- sample + the two forward maps.  With the fused next sample h_w was written by the previous step's posterior
        # update (the step's LAST big kernel, see body()): its A transform goes first, while h_w is still in the Infinity Cache
        # (measured: read cold, half a step later, the forward A transform takes 10 us longer)
        if self.plan.fuse_next:
            h_w, h16, eps, wvec, A16 = self.net_forward()
            lpe_t, e_lpe, pe_c = self.pe_forward(weff_cache)
        else:
            lpe_t, e_lpe, pe_c = self.pe_forward(weff_cache)
            h_w, h16, eps, wvec, A16 = self.net_forward()
        sse, dw, dpe, dw16 = self.siren(pe_c, wvec)
        dh, gA, h0, keep = self.a_backward(h_w, h16, dw, dw16, A16)
        return _Forward(sse, dh.view(self.plan.n, 1, -1), eps, e_lpe, gA, h0), _Tape(lpe_t, pe_c, dpe), keep

    # ---- seg1b: backward through the upsampling net ------------------------------------------------------------------------
    def seg1b(self, fwd, tape):
        p, flat = self.plan, self.flat
        inputs = [tape.lpe_t] + (self.conv if p.training_mappings else [])
        g_in = torch.autograd.grad(tape.pe_c, inputs, tape.dpe)
        d_lpe = g_in[0].reshape(p.n, 1, self.model._d_lpe).contiguous()
        grads = h1 = None
        if p.training_mappings:
            gc = [g.contiguous() for g in g_in[1:]]
            if flat is not None:
                gc = flat.pack(1, gc)
                if p.capture_coll:
                    h1 = flat.reduce(1, async_op=True)
            grads = fwd.gA + gc
        return _Backward(d_lpe, grads, h1)

    def comm(self, part):
        """sum of the mapping gradients over the ranks (the only per-step collectives): part 0 = the A matrices (13.4 of
        the 14.4 MB, ready before the upsampling backward starts), part 1 = the conv weights; returns the async handle"""
        if self.flat is None:
            return None
        return self.flat.reduce(part, async_op=True)

    # ---- seg2: the posterior updates ------------------------------------------------------------------------------------------
    # fused posterior update of the latent weights' levels (also accumulates the pre-update KL for the ELBO log)
    def update_net(self, fwd):
        p, ws = self.plan, self.ws
        nxt_net = None
        if p.fuse_next:            # the next step sees the noise counter + 1 (rcb_step_end increments it after this segment)
            smp = self.smp_net
            nxt_net = ops.NextSample((smp[0], smp[1], smp[2] if (p.want16 or p.planes) else None), self.rng_seed, 0,
                                     ws["rng_ctr"], 1, redraw_eps=p.redraw, group_offset=p.goff_net)
        for lv, (pl, ps), e, stt in zip(self.net, self.net_priors, fwd.eps, ws["net_state"]):
            ops.posterior_bwd(lv, pl, ps, False, 1.0, fwd.dh3, e, 1, adam=self.cfg, state=stt, kl_accum=ws["kl_slots"],
                              kl_scalar_dev=ws["beta_dev"], next_sample=nxt_net)

    def lpe_update_args(self, fwd, bwd):
        """arguments of the lpe level's posterior update (ops.posterior_bwd, without adam=)"""
        p, ws, pri = self.plan, self.ws, self.ws["pri"]
        nxt_lpe = None
        if p.fuse_lpe:
            smp = self.smp_lpe
            nxt_lpe = ops.NextSample((smp[0], smp[1], smp[2] if p.lpe16_want else None), self.rng_seed, 1, ws["rng_ctr"], 1,
                                     redraw_eps=p.redraw_lpe, group_offset=p.goff_lpe)
        return ((self.lpe_lv, pri[2].reshape(-1), pri[3].reshape(-1), False, 1.0, bwd.d_lpe, fwd.e_lpe, 1),
                dict(state=ws["lpe_state"], kl_accum=ws["kl_slots"], kl_scalar_dev=ws["beta_dev"], next_sample=nxt_lpe))

    def update_lpe(self, fwd, bwd):
        args, kwargs = self.lpe_update_args(fwd, bwd)
        ops.posterior_bwd(*args, adam=self.cfg, **kwargs)

    def seg2(self, fwd, bwd):
        self.update_net(fwd)
        self.update_lpe(fwd, bwd)

    # ---- seg3: Adam on the mappings + bookkeeping -------------------------------------------------------------------------
    def _adam_args(self, bwd):
        ms = self.ws["map_state"]
        return ([q.data for q in self.A + self.conv], [g.contiguous() for g in bwd.grads], [m_ for m_, _ in ms],
                [v_ for _, v_ in ms], self.cfg)

    def adam_mappings(self, fwd, bwd):
        for h_ in (fwd.h0, bwd.h1):             # captured collectives: the stream that runs Adam waits for both buckets
            if h_ is not None:
                h_.wait()
        if self.plan.training_mappings:
            ops.adam_multi(*self._adam_args(bwd))

    def step_end(self, fwd):
        ws = self.ws
        ops.step_end(ws["step_t"], fwd.sse, self.mse_scale, ws["kl_slots"], ws["mse_buf"], ws["kl_buf"], aux_counter=ws["rng_ctr"])

    def seg3(self, fwd, bwd):
        self.adam_mappings(fwd, bwd)
        self.step_end(fwd)

    def tail(self, fwd, bwd):
        """update_lpe + adam_mappings + step_end in one launch; False (nothing launched) if the level does not qualify"""
        ws = self.ws
        args, kwargs = self.lpe_update_args(fwd, bwd)
        return ops.step_tail(args, kwargs, *self._adam_args(bwd), ws["tickets"], ws["step_t"], fwd.sse, self.mse_scale,
                             ws["mse_buf"], ws["kl_buf"], aux_counter=ws["rng_ctr"])

    # ---- the step -----------------------------------------------------------------------------------------------------------
    def body(self):
        """one training step (eager, or recorded when called under a capture)"""
        p = self.plan
        if not p.update_last:
            fwd, tape, _ = self.seg1a()
            w0 = self.comm(0)
            bwd = self.seg1b(fwd, tape)
            del tape
            w1 = self.comm(1)
            self.seg2(fwd, bwd)
            for w_ in (w0, w1):
                if w_ is not None:
                    w_.wait()
            self.seg3(fwd, bwd)
            return
        # one rank (or collectives inside the graph): the network level's update -- which writes the next step's h_w -- is
        # the step's last big kernel, so that the next step's A transform (its first) finds h_w in the Infinity Cache
        fwd, tape, keep = self.seg1a()
        if p.fork_update:
            with torch.cuda.stream(self.fork):      # the network level's update needs dh only: straight behind the A backward
                self.update_net(fwd)
        bwd = self.seg1b(fwd, tape)
        del tape
        if p.fork_bwd:
            torch.cuda.current_stream().wait_stream(self.fork)
        # `keep` = the SIREN gradient and the sample (and their bf16 copies) that the forked stream reads.  They were
        # allocated on the main stream and are READ on the forked one: they must stay allocated until the streams have joined,
        # or the caching allocator hands their memory to the next main-stream allocation (the upsampling net's backward) while
        # the A transform is still reading it.  Nothing reads `keep`: holding it up to here is its whole purpose.
        del keep
        if p.fused_tail and self.tail(fwd, bwd):
            return                               # (the whole tail was that one launch)
        self.update_lpe(fwd, bwd)
        self.adam_mappings(fwd, bwd)
        if not p.fork_update:
            self.update_net(fwd)
        self.step_end(fwd)

    def capture(self):
        """record the step into the workspace's graph(s).  -> None, or the exception that made the capture fail here or
        (sharded) on another rank: capture is an optimisation, the caller falls back to eager stepping"""
        ws, p = self.ws, self.plan
        failure = None
        torch.cuda.synchronize()
        try:
            if p.one_graph:       # one rank / frozen mappings / captured collectives: the whole step is one graph
                graph = torch.cuda.CUDAGraph()
                # (thread_local: the process group's watchdog thread must not be able to invalidate the capture)
                with torch.cuda.graph(graph, capture_error_mode="thread_local" if p.sharded else "global"):
                    self.body()                        # records the step; nothing executes during capture
                ws["graphs"] = ("one", graph)
            else:                               # sharded: four graphs around the two eager, asynchronous all-reduces
                pool = torch.cuda.graph_pool_handle()
                graphs = []

                def record(seg, *args):
                    g = torch.cuda.CUDAGraph()
                    # thread_local: the process group's own threads (RCCL watchdog: event queries) must not be able
                    # to invalidate a capture in progress on this thread
                    with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
                        out = seg(*args)
                    graphs.append(g)
                    return out
                fwd, tape, _ = record(self.seg1a)
                bwd = record(self.seg1b, fwd, tape)
                del tape
                record(self.seg2, fwd, bwd)
                record(self.seg3, fwd, bwd)
                ws["graphs"] = ("segments", graphs)
        except Exception as exc:     # (a body that aborted in mid-capture leaves nothing behind: what its segments hand on --
            failure = exc            # fork state, the Work handles of collectives that were only RECORDED -- are return values,
            torch.cuda.synchronize()  # so an eager step cannot find them, skip its own all-reduce or wait on a dead handle)
        if self.flat is not None:
            # every rank must take the same route from here on: replayed segments and eager steps issue the same
            # collectives, but a rank that alone drops to eager would also alone flip `use_graph` for later calls.
            # No collective has EXECUTED during the capture attempt -- in the four-segment form they sit between the
            # segments, in the captured form they were recorded into a graph that is dropped -- so the ranks are
            # still aligned and can agree here.
            ok = torch.tensor([0 if failure is not None else 1], device=self.dev, dtype=torch.int32)
            torch.distributed.all_reduce(ok, op=torch.distributed.ReduceOp.MIN, group=self.model.dp_group)
            if int(ok.item()) == 0 and failure is None:
                failure = RuntimeError("capture failed on another rank")
        return failure

    def replay(self, k):
        kind, gr = self.ws["graphs"]
        for _ in range(k):
            if kind == "one":
                gr.replay()
            else:
                gr[0].replay()
                w0 = self.comm(0)
                gr[1].replay()
                w1 = self.comm(1)
                gr[2].replay()
                w0.wait()
                w1.wait()
                gr[3].replay()
