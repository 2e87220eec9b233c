"""The training step behind TestBNNmodel.train, in the form of train_step.py: plan (TestStepPlan), workspace (`model._ws`: the two
captured graphs, keyed by the plan plus the shapes, strides and storage addresses they were recorded with), step (TestTrainStep)."""
# compress_posteriors calls train() once per encode round, thousands of times per run: these captured graphs live longest
import collections
import types

import torch

from . import ops
from .upsample_fast import hip_path_supported

N_WARM = 3              # eager steps per workspace in front of the first capture (they are real steps)

# the model's switches that enter the plan as they are, and the constants of the beta update (Python floats: kernel
# arguments, i.e. baked into the captured graph of the adjusting step); then the call's values and what plan_test_step
# derives (each field is assigned exactly once there, with its meaning)
SWITCHES = ("precision", "patch", "split_gemm", "split_terms", "stage1_bf16", "pe_bf16", "stitched_pe")
BETA_CONSTANTS = ("bit_per_group", "kl_upper_buffer", "kl_lower_buffer", "beta_step_size")
TestStepPlan = collections.namedtuple("TestStepPlan", SWITCHES + BETA_CONSTANTS + (
    "samples", "lr", "eps", "n", "n_pix", "n_out", "split", "pe_stitched", "pe_hip", "want_xf16", "graphable"))


# the TestStepPlan (hashable) of one train() call, from the model `m`'s switches and the call's arguments
def plan_test_step(m, y, n_epochs, lr, eps, samples, verbose):
    cuda = m.loc.device.type == "cuda"
    p = types.SimpleNamespace(**{k: getattr(m, k) for k in SWITCHES}, **{k: float(getattr(m, k)) for k in BETA_CONSTANTS})
    p.samples = int(samples)                                 # S: samples per INR and step
    p.lr, p.eps = float(lr), float(eps)                      # of the fresh Adam the caller passed
    p.n, p.n_pix, p.n_out = y.shape                          # INRs; pixels per INR, output channels
    # 16-bit modes: the A transform on the hand-written kernels of atrans.hip (ops.ATransform), else library GEMMs
    p.split = bool(m.split_gemm and m.precision != 0)
    p.pe_stitched = m._pe_layout() is not None               # pe stays on the stitched grids (InrGeometry._pe_layout)
    # lpe -> pe on the hand-written upsampling kernels (InrGeometry._pe): where stage1_bf16 and pe_bf16 act
    p.pe_hip = bool(m.precision != 0 and hip_path_supported(m.upsample_net, m.pixel_sizes, m.upsample_factors, m.patch, m.data_dim))
    p.want_xf16 = bool(m.precision in (1, 2) and cuda)       # the SIREN launches read a 16-bit copy of the coordinate grid
    # the step may be replayed as captured graphs.  The LAST field: it decides whether this call captures and replays, not what
    # a capture holds, so it stays out of the workspace key -- a short or verbose call in between keeps the graphs
    p.graphable = bool(m.use_graph and m.noise_source is None and not verbose and n_epochs >= 8 and cuda)
    return TestStepPlan(**vars(p))          # (a field misspelt or forgotten above is a TypeError here)


class TestTrainStep:
    # One train() call's view of the step: the plan, the workspace (found on the model when its key still holds, else built)
    # and the model, mappings and data the kernels read.  What the parts of a step hand on are return values: nothing of a
    # step -- the autograd graph lpe_t -> pe_c in particular, see _Tape in train_step.py -- outlives body().
    __test__ = False

    def __init__(self, model, x, y, n_epochs, adam, samples, verbose):         # adam: the fresh optimiser's parameter group
        self.model, self.dev = model, model.loc.device
        self.x, self.y = x, y = x.to(self.dev), y.to(self.dev).contiguous()
        self.levels, self.specs = model._levels, model._level_specs()
        self.A, self.slices = [a.detach() for a in model.linear_transform.A], model._layer_slices()
        self.plan = plan = plan_test_step(model, y, n_epochs, adam["lr"], adam.get("eps", 1e-8), samples, verbose)
        self.pe_lay, self.meta = model._pe_layout(), model._meta(x, 16, plan.samples)
        # every tensor a captured kernel reads or writes, by storage address (Module.to() or an assignment to .data
        # re-allocates a storage while the Python object stays the same): per level the posterior, the prior, beta, the encode
        # progress and the index arrays of the sampler and of the grouping; the mappings
        held = [t for lv, sp in zip(self.levels, self.specs) for t in (
            sp.loc, sp.log_scale, sp.enc_sample, sp.enc_mask, sp.row_map, sp.row_perm, sp.col_map, sp.member_ptr, sp.member_idx,
            sp.row_perm_inv, sp.col_inv, lv.p_loc, lv.p_log_scale, lv.kl_beta, lv.d_done, lv.d_group_idx, lv.d_start, lv.d_end)]
        key = (plan[:-1], x.data_ptr(), tuple(x.shape), tuple(x.stride()), y.data_ptr(), tuple(y.shape), tuple(y.stride()),
               tuple(None if t is None else t.data_ptr() for t in held + self.A + list(model.upsample_net.parameters())))
        ws = model._ws
        self.reused = ws is not None and ws["key"] == key and ws["tab"].shape[0] >= n_epochs
        if not self.reused:
            ws = model._ws = self._new_workspace(key, n_epochs)
        self.ws, self.split = ws, ws["split"]
        self.cfg = ops.adam_cfg(plan.lr, 1, eps=plan.eps, dyn=ws["dyn"])

    # what survives across calls: its stable addresses let the two captured step graphs be reused by every fine-tune call
    def _new_workspace(self, key, n_epochs):
        p, dev = self.plan, self.dev
        # the Adam moments of all levels as views of one buffer: a fine-tune call (a few steps each, thousands of them
        # per compression run) resets them with one launch
        state_flat, views = ops.zeroed_views([lv.loc.shape for lv in self.levels for _ in range(4)], dev)
        return dict(key=key, tab=ops.adam_table(p.lr, max(n_epochs, 2048)).to(dev), state_flat=state_flat,
                    dyn=torch.zeros(2, device=dev), step_t=torch.zeros(1, device=dev, dtype=torch.long),
                    states=[{k: next(views) for k in ("m_loc", "v_loc", "m_ls", "v_ls")} for lv in self.levels],
                    graphs={}, warm=0,         # graphs: one per value of `adjust`; warm: eager steps taken so far
                    # bf16 copy of the coordinate grid: owned by the workspace that owns the graphs reading its address
                    xf16=ops.xf_bf16(self.x, p.precision) if p.want_xf16 else None,
                    split=ops.ATransform(self.slices, dev, p.split_terms) if p.split else None)

    # per call: a fresh optimiser (moments zeroed, step counter restarted); a new workspace packs the mappings, which are
    # fixed at test time
    def prime(self):
        ws = self.ws
        if self.reused:
            ws["state_flat"].zero_()
        ws["step_t"].zero_()
        if self.split is not None and not self.reused:
            self.split.prepare(self.A)

    # ---- the parts of a step, in launch order ---------------------------------------------------------------------------------
    # ---- noise and sample -> (eps per level, sample [N, S, Dtot])
    def sample(self):
        eps = self.model._draw_all(self.plan.samples)
        return eps, ops.reparam_fwd(self.specs, eps, self.plan.samples)

    # ---- lpe -> pe under autograd with respect to lpe_t only -> (lpe_t, pe_c)
    def pe_forward(self, sample):
        m, p = self.model, self.plan
        lpe_t = m._pe_from_sample(sample, p.samples).contiguous().requires_grad_(True)
        with torch.enable_grad():
            if self.pe_lay is not None:
                return lpe_t, m._pe(lpe_t, stitched=True)
            pe = m._pe(lpe_t)
            return lpe_t, pe.reshape(p.n * p.samples, p.n_pix, pe.shape[-1]).contiguous()

    # ---- A transform of the latent weights' sample -> wvec [N * S, D]
    def a_forward(self, sample):
        rows, D = self.plan.n * self.plan.samples, self.model._d_net
        h_w = sample[..., :D].reshape(rows, D)
        if self.split is not None:
            return self.split.forward(h_w, self.split.new_rows(rows))
        return ops.a_transform_mm(h_w, self.A, self.slices, torch.empty(rows, D, device=self.dev, dtype=torch.float32))

    # ---- fused SIREN forward + MSE + backward -> (dw, dpe)
    def siren(self, pe_c, wvec):
        p = self.plan
        _, dw, dpe = ops.siren_loss_bwd(self.x, pe_c.detach(), wvec, self.y, 1.0 / (p.samples * p.n_pix * p.n_out), self.meta,
                                        pe_layout=self.pe_lay, xf16=self.ws["xf16"])
        return dw, dpe

    # ---- data gradient of the A transform into dh [N * S, D]
    def a_backward(self, dw, dh):
        if self.split is not None:
            return self.split.dgrad(dw, dh)
        return ops.a_transform_mm(dw, self.A, self.slices, dh, transpose=True)

    # ---- -> (d_full [N, S, D + Dlpe]: the gradient of level 1's sample; dh3 [N, S, D]: of levels 2 and 3's, None without)
    def level_grads(self, dw, d_lpe):
        p, D, Dt, new = self.plan, self.model._d_net, self.levels[0].D, dict(device=self.dev, dtype=torch.float32)
        d_lpe = d_lpe.reshape(p.samples, p.n, -1).permute(1, 0, 2)
        if p.patch:           # levels 2 and 3 need the contiguous [N, S, D] gradient as well
            dh3 = self.a_backward(dw, torch.empty(p.n * p.samples, D, **new)).view(p.n, p.samples, D)
            return torch.cat([dh3, d_lpe], -1).contiguous(), dh3
        d_full = torch.empty(p.n, p.samples, Dt, **new)       # the GEMMs write straight into the level-1 gradient buffer
        self.a_backward(dw, d_full.view(p.n * p.samples, Dt)[:, :D])
        d_full[:, :, D:].copy_(d_lpe)
        return d_full, None

    # ---- fused posterior update (KL gradient, Adam) of every level
    def update_levels(self, eps, d_full, dh3):
        for li, (lv, sp, e, stt) in enumerate(zip(self.levels, self.specs, eps, self.ws["states"])):
            ops.posterior_bwd(sp, lv.p_loc, lv.p_log_scale, True, 1.0, d_full if li == 0 else dh3, e, self.plan.samples,
                              beta=lv.kl_beta, group_idx=lv.d_group_idx, n_groups=lv.n_groups, adam=self.cfg, state=stt)

    def beta_update(self, grp):
        p = self.plan
        for lv, gk in zip(self.levels, grp):
            ops.beta_update(gk, lv.kl_beta, lv.d_done, p.bit_per_group, p.kl_upper_buffer, p.kl_lower_buffer, p.beta_step_size)

    # ---- the step -----------------------------------------------------------------------------------------------------------
    def body(self, adjust):
        # one training step (eager, or recorded when called under a capture); `adjust`: with the beta update
        ws = self.ws
        ops.step_begin(ws["tab"], ws["step_t"], ws["dyn"])
        eps, sample = self.sample()
        lpe_t, pe_c = self.pe_forward(sample)
        dw, dpe = self.siren(pe_c, self.a_forward(sample))
        (d_lpe,) = torch.autograd.grad(pe_c, [lpe_t], dpe)                            # [S, N, *lat, C]
        d_full, dh3 = self.level_grads(dw, d_lpe)
        grp = [self.model._group_kls(lv) for lv in self.levels] if adjust else None
        self.update_levels(eps, d_full, dh3)
        if adjust:       # the old beta shaped this step's gradient; the new one acts from the next epoch on
            self.beta_update(grp)
        ops.step_end(ws["step_t"])

    # one step of the graph path: an eager warm-up step while the workspace has taken fewer than N_WARM (counted across calls),
    # else the replay of the graph of this `adjust`, captured when it is first met.  -> None, or the exception that made the
    # capture fail: capture is an optimisation, the step then ran eagerly and the caller goes on that way
    def graph_step(self, adjust):
        ws = self.ws
        g = ws["graphs"].get(adjust)
        if g is None and ws["warm"] < N_WARM:
            ws["warm"] += 1
            return self.body(adjust)
        if g is None:
            torch.cuda.synchronize()
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):          # records; executes nothing
                    self.body(adjust)
                ws["graphs"][adjust] = g
            except Exception as exc:
                torch.cuda.synchronize()
                self.body(adjust)
                return exc
        g.replay()
