"""Times fwd+bwd of the upsampling net variants at the bench shape (N=4096 CIFAR), then the forward of stages 2 + 3 alone: the
two rcb_upconv_fwd launches against the one rcb_upconv_fwd23 launch (`--fwd23-only`: just that)."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recombiner_amd import prior_model as PM
from recombiner_amd.upsample_fast import UpsampleFast
dev = "cuda"
FWD23_ONLY = "--fwd23-only" in sys.argv
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(argv[0]) if argv else 4096
torch.manual_seed(0)
net = PM.Upsample(2, [2, 1, 1], [4, 2, 2]).to(dev)
fast = UpsampleFast(net)
x = torch.randn(N, 128, 2, 2, device=dev, requires_grad=True)
g = torch.randn(N, 16, 32, 32, device=dev)

def run(fn, autocast=None, reps=5, cl=False):
    xi = x.contiguous(memory_format=torch.channels_last) if cl else x
    def once():
        if autocast:
            with torch.autocast("cuda", dtype=autocast):
                y = fn(xi)
        else:
            y = fn(xi)
        return torch.autograd.grad(y, [x] + list(net.parameters()), g.to(y.dtype))
    for _ in range(2):
        once()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = once()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, r

if not FWD23_ONLY:
    ref_ms, ref = run(net)
    print("nn.Module fp32           %.2f ms" % ref_ms)
    for name, fn, ac, cl in [("nn.Module fp32 channels_last", net, None, True), ("nn.Module bf16 autocast", net, torch.bfloat16, False),
                             ("phase form fp32", fast, None, False), ("phase form bf16 autocast", fast, torch.bfloat16, False)]:
        ms, r = run(fn, ac, cl=cl)
        err = max(((a.float() - b).abs().max() / (b.abs().max() + 1e-20)).item() for a, b in zip(r, ref))
        print("%-30s %.2f ms   max rel grad err %.2e" % (name, ms, err))


# ---- stages 2 + 3 forward alone: the pair of launches against the fused launch, alternating, medians of event times ----------
from recombiner_amd import ops
with torch.no_grad():
    _, _, e2, e3, pack = ops.upconv_weff_build(net.conv1.weight, net.conv1.bias, net.conv2.weight, net.conv3.weight, True)
    b2, b3 = net.conv2.bias.detach().contiguous(), net.conv3.bias.detach().contiguous()
z1 = torch.randn(N, 8, 8, 64, device=dev).to(torch.bfloat16)
out = (torch.empty(N, 16, 16, 64, device=dev, dtype=torch.bfloat16), torch.empty(N, 32, 32, 16, device=dev, dtype=torch.bfloat16))


def pair():
    h2 = ops.upconv_fwd(z1, e2, b2, 8, 64, out_f32=False, preact=True, pack=pack)
    return h2, ops.upconv_fwd(h2, e3, b3, 16, 16, out_f32=False, linear_bf16=True, pack=pack)


def fused():
    return ops.upconv_fwd23(z1, b2, b3, pack, out=out)


def event_us(fn, reps=20, blocks=5):
    """per-launch time of `reps` back-to-back launches between two events (the launch gaps overlap the kernels), per block"""
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return out


for fn in (pair, fused):
    fn()
ref_h2, ref_pe = pair()
got_h2, got_pe = fused()
print("fused == pair: h2 %s  pe %s" % (torch.equal(ref_h2, got_h2), torch.equal(ref_pe, got_pe)))
times = {"pair": [], "fused": []}
for _ in range(5):                      # alternating blocks
    times["pair"] += event_us(pair)
    times["fused"] += event_us(fused)
for k, v in times.items():
    v.sort()
    print("stages 2 + 3 forward, %-5s  N = %d: median %.1f us  min %.1f  max %.1f  (%d blocks of 20 back-to-back launches)"
          % (k, N, v[len(v) // 2], v[0], v[-1], len(v)))
