"""Deep SIREN (5 to 7 hidden layers) measurements at BASELINE configs[1] size: 4096 CIFAR INRs of 1024 pixels.

    python tools/deep_siren_prof.py kernels   -> the bf16 loss / backward launch as the training step makes it (16-bit input rows:
                                                 bf16 pe + the xf copy, dpe, gradient planes) at 5 and 7 hidden layers of width 16
                                                 and 32, the depth-3 launches of the same widths (narrow / wave kernels) and the
                                                 fp32 parity launches of the same shapes; run it under
                                                 `rocprofv3 --kernel-trace --stats -- ...` for the per-kernel table, it also prints
                                                 its own event timings
    python tools/deep_siren_prof.py step      -> the whole bf16 training step (device noise, graph replay) at [16] * 7 and [32] * 7

The algorithmic bytes of one launch are printed with the kernel times: pe read + dpe written (bf16), targets, the rows of
weights read and their gradient planes written; the shared coordinate grid is read once from L2 per row and not counted."""
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recombiner_amd import ops  # noqa: E402
from recombiner_amd.ops import SirenMeta  # noqa: E402

DEV, N, P = "cuda", 4096, 1024
HBM_PEAK = 8.0e12


def _time(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def kernels(reps=20):
    out = {}
    shapes = [(nh, w, 1) for w in (16, 32) for nh in (3, 5, 7)] + [(nh, w, 0) for w in (16, 32) for nh in (3, 5, 7)]
    for nh, width, prec in shapes:
        meta = SirenMeta(1, P, 16, 16, nh, width, 3, precision=prec)
        torch.manual_seed(0)
        xf = torch.rand(P, 16, device=DEV) * 2 - 1
        pe = torch.randn(N, P, 16, device=DEV) * 0.5
        pe = pe.bfloat16() if prec else pe
        y = torch.rand(N, P, 3, device=DEV)
        wv = (torch.rand(N, meta.d_net, device=DEV) * 2 - 1) * (6 / width) ** 0.5 / 30
        x16 = ops.xf_bf16(xf, prec) if prec else None
        if prec:
            def fn():
                return ops.siren_loss_bwd(xf, pe, wv, y, 1.0 / (3 * P), meta, xf16=x16, want_planes=True)
        else:
            def fn():
                return ops.siren_loss_bwd(xf, pe, wv, y, 1.0 / (3 * P), meta)
        us = _time(fn, reps if prec else 3)
        pe_b = 2 if prec else 4
        row = P * 16 * pe_b * 2 + P * 3 * 4 + meta.d_net * 4 + meta.d_net * 4      # pe + dpe, targets, weights, gradient (planes / fp32)
        rec = {"n_hidden": nh, "width": width, "precision": prec, "us_per_launch_incl_host": round(us, 2), "bytes_per_row": row,
               "mb_per_launch": round(row * N / 1e6, 1), "hbm_fraction_at_8TBps": round(row * N / (us * 1e-6) / HBM_PEAK, 3)}
        print(json.dumps(rec), flush=True)
        out[(nh, width, prec)] = rec
    return out


def step(steps=20):
    import numpy as np
    from recombiner_amd import config, utils
    from recombiner_amd import prior_model as PM
    for width in (16, 32):
        cfg = dict(config.configs["cifar"])
        cfg["hidden_dims"] = [width] * 7
        X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], N, cfg["output_dim"], seed=0)
        m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], N, cfg["data_dim"], cfg["pixel_sizes"],
                             cfg["upsample_factors"], cfg["latent_dim"], cfg["patch"], cfg["patch_nums"],
                             cfg["hierarchical_patch_nums"], random_seed=42, device=DEV)
        m.precision = 1
        torch.manual_seed(1)
        lt = PM.LinearTransform(m.dims).to(DEV)
        up = PM.Upsample(cfg["data_dim"], cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
        s0, D = 0.0211547, m._d_net
        lat = list(m.lpe_loc.shape[1:])
        pri = [torch.zeros(D, device=DEV), torch.full((D,), s0, device=DEV), torch.zeros(lat, device=DEV),
               torch.full(lat, s0, device=DEV)] + [None] * 4
        Xd, Yd = X.to(DEV)[None].expand(N, -1, -1), Y.to(DEV)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m.train(6, 2e-4, Xd, Yd, *pri, lt, up, 1e-8, training_mappings=True)
            calls = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                _, _, elbo = m.train(steps, 2e-4, Xd, Yd, *pri, lt, up, 1e-8, training_mappings=True)
                e1.record()
                torch.cuda.synchronize()
                calls.append(e0.elapsed_time(e1) / steps)
        print(json.dumps({"hidden_dims": cfg["hidden_dims"], "ms_per_step_median": round(float(np.median(calls)), 4),
                          "calls_ms": [round(c, 4) for c in calls], "elbo_finite": bool(np.isfinite(elbo).all())}), flush=True)
        del m, lt, up
        torch.cuda.empty_cache()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    {"kernels": kernels, "step": step}[what]()
