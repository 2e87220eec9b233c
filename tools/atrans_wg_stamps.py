"""Per-workgroup timeline of an A-transform launch (diagnostic build):

    python -m recombiner_amd.build --variant atwgstamps --only atrans.hip -DRCB_STAMPS_ATRANS_WG=1
    python tools/atrans_wg_stamps.py [rows] [terms] [nofit]

Every workgroup of the launch stamps its begin and end (s_memrealtime, 100 MHz, one clock for the whole chip; s_memtime for
the shader clock).  Printed:
  1. the planner's runs of the headline launch by type (layer:blocks of each segment): how many, how long, when they end
     relative to the first workgroup's begin, and the pole excess (median end of the runs that hold two layers of >= 8
     blocks minus median end of the plain 7-block runs);
  2. launches of injected plans in which every workgroup is ONE segment of w = 1..7 blocks, on a 33-chunk and on a 17-chunk
     layer: the difference is 16 chunk iterations, the rest the segment's prologue + epilogue; least-squares fit of the
     iteration time t(w) = a + b w and the planner's constants F = a / b, E = rest / b (block-chunk units)."""
import ctypes as C
import sys
import numpy as np
import kernel_stamps
kernel_stamps.select("ATRANS_WG")
import torch
from recombiner_amd import ops

REALTIME_MHZ = 100.0
HEAD = 12
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
terms = int(sys.argv[2]) if len(sys.argv) > 2 else 2
dev = "cuda"
torch.manual_seed(0)


def slices_of(sizes):
    cum = np.cumsum([0] + list(sizes))
    return [(int(cum[i]), int(cum[i + 1])) for i in range(len(sizes))]


def make(sizes):
    D = sum(sizes)
    x = torch.randn(rows, D, device=dev) * 0.03
    A = [torch.randn(n, n, device=dev) / n ** 0.5 for n in sizes]
    tr = ops.ATransform(slices_of(sizes), dev, terms=terms)
    tr.prepare(A)
    return tr, x, torch.empty(rows, D, device=dev)


def parse(raw):
    n_wg, n_segs = int(raw[0]), int(raw[1])
    head = (HEAD + n_wg + 1 + 3) // 4 * 4
    return raw[HEAD:HEAD + n_wg + 1], raw[head:head + 8 * n_segs].reshape(n_segs, 8)


def encode(runs):
    """plan integers of a launch with one workgroup per run (whole contraction: the layout rcb_atrans_plan writes for S = 1)"""
    begin, segs = [0], []
    for run in runs:
        segs += run
        begin.append(len(segs))
    n_wg = len(runs)
    head = (HEAD + n_wg + 1 + 3) // 4 * 4
    raw = np.zeros(head + 8 * len(segs), dtype=np.int32)
    raw[0], raw[1], raw[2] = n_wg, len(segs), 1
    raw[HEAD:HEAD + n_wg + 1] = begin
    raw[head:] = np.array(segs, dtype=np.int32).reshape(-1)
    return raw


def stamps(tr, x, out, n_wg, reps=9):
    """[reps, n_wg, 4] of the forward launch: realtime begin, end, shader clock begin, end"""
    for _ in range(20):
        tr.forward(x, out)
    res = []
    for _ in range(reps):
        torch.cuda.synchronize()
        tr.forward(x, out)
        torch.cuda.synchronize()
        res.append(kernel_stamps.read("ATRANS_WG", (n_wg, 4)))
    return np.stack(res)


# ---- 1. the planner's launch ------------------------------------------------------------------------------------------------------
sizes = [1056, 1056, 1056, 99]
tr, x, out = make(sizes)
raw = tr._plan(rows)[0].cpu().numpy()
begin, segs = parse(raw)
n_wg = len(begin) - 1
assert int(raw[2]) == 1 and n_wg <= 8192, "a launch of the S = 1 regime with at most 8192 workgroups expected"
st = stamps(tr, x, out, n_wg)
t0 = st[:, :, 0].min(1, keepdims=True)
dur = np.median((st[:, :, 1] - st[:, :, 0]) / REALTIME_MHZ, 0)
beg = np.median((st[:, :, 0] - t0) / REALTIME_MHZ, 0)
end = np.median((st[:, :, 1] - t0) / REALTIME_MHZ, 0)
cyc = np.median(st[:, :, 3] - st[:, :, 2], 0)
types, pole = {}, np.zeros(n_wg, dtype=bool)
nblk = [(n + 31) // 32 for n in sizes]
for i in range(n_wg):
    run = segs[begin[i]:begin[i + 1]]
    types.setdefault(" ".join("%d:%d" % (s[0], s[3]) for s in run), []).append(i)
    pole[i] = len({int(s[0]) for s in run if nblk[s[0]] >= 8}) > 1
print("atrans_kernel<%d, false> forward, %d rows x %s: %d workgroups, launch (first begin to last end, median of 9) %.1f us, "
      "shader clock / realtime clock = %.0f MHz" % (terms, rows, sizes, n_wg, np.median((st[:, :, 1].max(1) - t0[:, 0]) / REALTIME_MHZ),
                                                   np.median(cyc / dur)))
print("%-22s %5s %9s %9s %9s %9s %9s" % ("run (layer:blocks)", "n", "dur med", "dur min", "dur max", "begin med", "end med"))
for k, idx in sorted(types.items(), key=lambda kv: -np.median(end[kv[1]])):
    print("%-22s %5d %9.1f %9.1f %9.1f %9.1f %9.1f" % (k, len(idx), np.median(dur[idx]), dur[idx].min(), dur[idx].max(), np.median(beg[idx]),
                                                     np.median(end[idx])))
seven = np.array([len(segs[begin[i]:begin[i + 1]]) == 1 and segs[begin[i]][3] == 7 for i in range(n_wg)])
if pole.any() and seven.any():
    print("runs over two wide layers: %d, median duration %.1f us, median end %.1f us;  plain 7-block runs: %d, %.1f us, end %.1f us;  "
          "pole excess %.1f us, duration ratio %.2f" % (pole.sum(), np.median(dur[pole]), np.median(end[pole]), seven.sum(), np.median(dur[seven]),
                                                        np.median(end[seven]), np.median(end[pole]) - np.median(end[seven]),
                                                        np.median(dur[pole]) / np.median(dur[seven])))
else:
    print("no run holds two wide layers" if not pole.any() else "no plain 7-block run")

if "nofit" in sys.argv[3:]:
    sys.exit(0)

# ---- 2. one segment per workgroup, w = 1 .. 7 blocks, 33 and 17 chunks -----------------------------------------------------------------
sizes2 = [1056, 544]
tr2, x2, out2 = make(sizes2)
m_tiles, per_tile = (rows + 255) // 256, max(1, tr2.n_cu // ((rows + 255) // 256))
D = {}
for w in range(1, 8):
    for layer, nk in ((0, 33), (1, 17)):
        runs = [[[layer, 256 * mt, (j * w) % (nk - w + 1), w, 0, nk, -1, 0]] for mt in range(m_tiles) for j in range(per_tile)]
        plan = encode(runs)
        tr2._plans[rows] = (torch.from_numpy(plan).to(dev), (C.c_int32 * HEAD)(*[int(v) for v in plan[:HEAD]]), 0)
        s2 = stamps(tr2, x2, out2, len(runs), reps=5)
        D[w, nk] = float(np.median((s2[:, :, 1] - s2[:, :, 0]) / REALTIME_MHZ))
ws = np.arange(1, 8)
t = np.array([(D[w, 33] - D[w, 17]) / 16 for w in ws])
rest = np.array([D[w, 33] - 33 * tw for w, tw in zip(ws, t)])
b, a = np.polyfit(ws, t, 1)
print("\none segment of w blocks per workgroup, %d workgroups at once (median workgroup duration, us):" % (m_tiles * per_tile))
print("%3s %10s %10s %12s %12s" % ("w", "33 chunks", "17 chunks", "t(w) us", "rest us"))
for w, tw, r in zip(ws, t, rest):
    print("%3d %10.2f %10.2f %12.3f %12.2f" % (w, D[w, 33], D[w, 17], tw, r))
print("fit t(w) = a + b w:  a = %.3f us, b = %.3f us, largest residual %.3f us;  F = a / b = %.2f,  E = median rest / b = %.1f"
      % (a, b, float(np.abs(a + b * ws - t).max()), a / b, float(np.median(rest)) / b))
