"""Eager host cost of one ops.siren_loss_bwd and one ops.posterior_bwd call at shapes whose kernels are shorter than the call:
mean of 1000 back-to-back calls, the clock stopped once when the last call has returned (enqueue) and once after the one
synchronisation at the end (wall).  --tree DIR imports recombiner_amd from another tree (RCB_LIB names the library then)."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--calls", type=int, default=1000)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402
from recombiner_amd import ops  # noqa: E402

DEV = "cuda"
gen = torch.Generator().manual_seed(1)
meta = ops.SirenMeta(1, 64, 16, 16, 3, 32, 3, precision=1)
xf = (torch.rand(64, 16, generator=gen) * 2 - 1).to(DEV)
pe = (torch.randn(4, 64, 16, generator=gen) * 0.5).to(DEV).bfloat16()
wv = ((torch.rand(4, meta.d_net, generator=gen) * 2 - 1) * 0.04).to(DEV)
y = torch.rand(4, 64, 3, generator=gen).to(DEV)
xf16 = ops.xf_bf16(xf, 1)
lv = ops.LevelSpec((torch.randn(8, 520, generator=gen) * 0.05).to(DEV), torch.full((8, 520), -4.0, device=DEV), 520, 8)
p_loc, p_scale = torch.zeros(520, device=DEV), torch.full((520,), 0.02, device=DEV)
d, eps = (torch.randn(8, 1, 520, generator=gen) * 1e-3).to(DEV), torch.randn(8, 1, 520, generator=gen).to(DEV)
state = {k: torch.zeros_like(lv.loc) for k in ("m_loc", "v_loc", "m_ls", "v_ls")}
cfg = ops.adam_cfg(2e-4, 3)


def timed(fn):
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.calls):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / args.calls * 1e6, (time.perf_counter() - t0) / args.calls * 1e6


s = timed(lambda: ops.siren_loss_bwd(xf, pe, wv, y, 1.0 / 192, meta, xf16=xf16))
p = timed(lambda: ops.posterior_bwd(lv, p_loc, p_scale, False, 1.0, d, eps, 1, adam=cfg, state=state))
print("siren_loss_bwd_enqueue_us %.2f wall_us %.2f posterior_bwd_enqueue_us %.2f wall_us %.2f" % (*s, *p))
