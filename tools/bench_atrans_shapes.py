"""Forward and data-gradient time of the A-transform kernels on the layer lists and row counts of the presets (events, median of
3 x 30 launches); RCB_LIB selects another build for a same-box A/B.   python tools/bench_atrans_shapes.py [label]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from recombiner_amd import ops
SHAPES = [(4096, (2112, 4160, 4160, 195)), (192, (1584, 2352, 2352, 147)), (192, (1056, 1056, 1056, 99)), (480, (1056, 1056, 1056, 99)),
          (256, (2112, 4160, 4160, 195)), (4096, (1584, 2352, 2352, 147)), (4096, (1056, 1056, 1056, 99)), (2500, (1056, 1056, 1056, 99))]
def timeit(fn, n=30):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
torch.manual_seed(0)
for rows, sizes in SHAPES:
    cum = [0]
    for n in sizes: cum.append(cum[-1] + n)
    D = cum[-1]
    x = torch.randn(rows, D, device="cuda") * 0.03
    A = [torch.randn(n, n, device="cuda") / n ** 0.5 for n in sizes]
    out = torch.empty(rows, D, device="cuda")
    tr = ops.ATransform(list(zip(cum[:-1], cum[1:])), "cuda", terms=2)
    tr.prepare(A)
    f = [timeit(lambda: tr.forward(x, out)) for _ in range(3)]
    d = [timeit(lambda: tr.dgrad(x, out)) for _ in range(3)]
    print("%s rows %5d %-26s wg %4d  forward %7.1f  dgrad %7.1f us (median of 3 x 30)" % ((sys.argv[1] if len(sys.argv) > 1 else ""), rows, sizes, int(tr._plan(rows)[1][0]), sorted(f)[1], sorted(d)[1]), flush=True)
