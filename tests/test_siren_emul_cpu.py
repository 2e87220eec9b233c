"""CPU tests of the operand-exact SIREN evaluator (tests/siren_emul.py): it is the plain MLP when nothing is rounded, its rounding
is torch's, and the error floor that no kernel can beat (operands pushed across a 16-bit rounding boundary by a different fp32
accumulation order) is the one recorded in siren_emul.FLIP_FLOOR, which the GPU test (test_hip_siren_operand_exact.py) builds on.
Nothing here needs the kernels or their library: the input sets and the switches of the families live in siren_emul."""
import math

import pytest
import torch

import siren_emul as se

ALL_CASES = [(fam, c) for fam, cs in se.CASES.items() for c in cs]
IDS = ["%s-w%d-nh%d-F%d-C%d-P%d-N%dS%d-%s-%s" % (f, c["hidden"], c["nh"], c["F"], c["C"], c["P"], c["N"], c["S"], c["scale"], c["variant"])
       for f, c in ALL_CASES]


def _autograd_mlp(case, dy=None):
    """fp64 autograd of the plain MLP in the layout of test_hip_kernels._oracle_mlp: x @ W + b, sin(30 x), [bias | W(in, out)]"""
    dims, S = case["dims"], case["S"]
    pe = case["pe"].double().requires_grad_(True)
    wv = case["wv"].double().requires_grad_(True)
    G = pe.shape[0]
    x = torch.cat([case["xf"].double()[None].expand(G, -1, -1), pe], -1)
    nl = len(dims) - 1
    for l, (lo, nin, nout) in enumerate(se.layer_slices(dims)):
        b = wv[:, lo:lo + nout].unsqueeze(1)
        W = wv[:, lo + nout:lo + nout * (nin + 1)].reshape(G, nin, nout)
        x = x @ W + b
        if l != nl - 1:
            x = torch.sin(30.0 * x)
    if dy is None:
        diff = x - case["y"].double().repeat_interleave(S, 0)
        (case["dy_scale"] * (diff * diff).sum()).backward()
        return dict(y=x.detach(), sse=(diff * diff).sum((1, 2)).detach(), dW=wv.grad, dpe=pe.grad)
    x.backward(dy.double())
    return dict(dW=wv.grad, dpe=pe.grad)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("fam,c", ALL_CASES, ids=IDS)
def test_unrounded_evaluator_is_the_plain_mlp(fam, c):
    """every rounding switched off: y, sse, dW, dpe and the plain backward equal fp64 autograd of the plain MLP to 1e-12, on
    every shape of the GPU test, whatever the bias / cosine switches say (they only choose WHERE to round)"""
    case = se.build(c)
    ref, ref2 = _autograd_mlp(case), _autograd_mlp(case, case["dy"])
    for bias, cos in (("fp32", "packed"), ("hilo", "fp32")):
        out = se.run_emul(case, None, bias=bias, cos=cos)
        for k in ("y", "sse", "dW", "dpe"):
            assert _rel(out[k], ref[k]) < 1e-12, (k, _rel(out[k], ref[k]))
        assert _rel(out["bwd_dW"], ref2["dW"]) < 1e-12 and _rel(out["bwd_dpe"], ref2["dpe"]) < 1e-12
    # every block of a gradient row is there once and the blocks tile the row
    sl = sorted((s.start, s.stop) for _, _, s in se.blocks_of_dw(case["dims"], case["F"]))
    assert sl[0][0] == 0 and sl[-1][1] == case["D"] and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))


@pytest.mark.parametrize("mode,dtype", [("bf16", torch.bfloat16), ("f16", torch.float16)])
def test_rounding_helper_equals_torch_casts_bit_for_bit(mode, dtype):
    """a sweep of fp32 values with ties (exactly half way between two neighbours, both parities), f16's subnormals and the
    values around them, the largest finite values and the first that overflow, zeros, and random bit patterns"""
    sig, emin, fmax = se.FORMATS[mode]
    gen = torch.Generator().manual_seed(0)
    vals = [torch.randint(-2 ** 31, 2 ** 31 - 1, (200000,), generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32)]
    vals.append(torch.randn(100000, generator=gen) * torch.tensor(10.0) ** torch.randint(-9, 6, (100000,), generator=gen))
    # ties and their neighbours at every exponent of the format, the subnormal range included
    for e in range(emin - sig - 2, int(math.log2(fmax)) + 2):
        q = 2.0 ** max(e - (sig - 1), emin - (sig - 1))              # spacing of the format at 2^e
        base = 2.0 ** e
        for k in (0, 1, 2, 3, 2 ** (sig - 1) - 2, 2 ** (sig - 1) - 1):
            for frac in (0.5, 0.5 - 2.0 ** -12, 0.5 + 2.0 ** -12, 0.25, 0.75, 0.0):
                vals.append(torch.tensor([base + (k + frac) * q, (k + frac) * q], dtype=torch.float64).float())
    vals.append(torch.tensor([0.0, -0.0, fmax, fmax * (1 + 2.0 ** -(sig + 1)), fmax * (1 + 2.0 ** -sig), fmax * (1 + 2.0 ** -(sig + 2)),
                              2.0 ** emin, 2.0 ** (emin - sig + 1), 2.0 ** (emin - sig), 2.0 ** (emin - sig - 1) * 1.0001, 3.0e38]))
    x = torch.cat(vals)
    x = torch.cat([x, -x])
    x = x[torch.isfinite(x)]
    want = x.to(dtype)
    got = se.round_to(x.double(), mode)
    assert torch.equal(got.to(dtype).view(torch.int16), want.view(torch.int16))          # the same bits (signed zeros included)
    fin = torch.isfinite(want)
    assert torch.equal(got[fin], want[fin].double()) and torch.equal(torch.isinf(got), torch.isinf(want))
    assert int((want != x).sum()) > 1000 and int(torch.isinf(want).sum()) > 0              # the sweep rounds and overflows


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_sensitivity_floor(mode):
    """The evaluator against itself with every pre-activation changed by a relative 2^-22 (another fp32 accumulation order; both
    signs): a pre-activation that lands on the other side of a 16-bit rounding boundary moves one activation by an ulp, which no
    kernel can avoid.  Printed per input set: the largest per-block difference of each output (the floor), the largest share of
    one block's elements that move by more than a tenth of it, and the largest share of one block's elements beyond the recorded
    FLIP_FLOOR of the block kind.  Asserted for EVERY block of every input set: at most FLIP_SHARE (1e-3) of its elements lie
    beyond FLIP_FLOOR -- none, in a block of fewer than 1000 elements -- so that with the evaluator alone every input set keeps
    the flip share under the cap at every limit the GPU test sets (none of its limits on a largest error is below FLIP_FLOOR);
    and every entry of FLIP_FLOOR is reached to within 10 % by some input set, so that the table is the floor and not a loose
    bound.  An input set that breaks this gets another seed or scale, not another cap."""
    floor_all = {}
    for fam, c in ALL_CASES:
        if fam == "wave" and mode == "f16":
            continue
        case = se.build(c)
        stored16 = c["variant"] != "f32pe"
        kw = dict(se.switches(fam, c), pe=case["pe"].bfloat16().float() if stored16 else case["pe"], dpe_store="bf16" if stored16 else None)
        a = se.run_emul(case, mode, **kw)
        stat = {}
        for sign in (1.0, -1.0):
            b = se.run_emul(case, mode, perturb=sign * 2.0 ** -22, **kw)
            for key, blocks in se.block_errors(case, b, a, "16" if stored16 else "").items():
                lim = se.FLIP_FLOOR[mode][key]
                worst = max(float(e.max()) for e in blocks)
                tenth = max(float((e > worst / 10).double().mean()) for e in blocks) if worst > 0 else 0.0
                beyond = 0.0
                for e in blocks:
                    over = int((e > lim).sum())
                    beyond = max(beyond, over / e.numel())
                    assert over <= math.floor(se.FLIP_SHARE * e.numel()), (fam, c, key, over, e.numel(), float(e.max()), lim)
                st = stat.setdefault(key, [0.0, 0.0, 0.0])
                stat[key] = [max(st[0], worst), max(st[1], tenth), max(st[2], beyond)]
        for key, st in stat.items():
            floor_all[key] = max(floor_all.get(key, 0.0), st[0])
        print("%s %s %s: floor (share of a block above a tenth of it) [share of a block beyond FLIP_FLOOR]  %s"
              % (fam, mode, {k: c[k] for k in ("hidden", "nh", "F", "C", "P", "scale", "variant")},
                 "  ".join("%s/%s %.1e (%.0e) [%.0e]" % (k[0], k[1], *st) for k, st in stat.items())))
    print("%s floor over all input sets: %s" % (mode, "  ".join("%s/%s %.2e" % (k[0], k[1], v) for k, v in floor_all.items())))
    for key, v in se.FLIP_FLOOR[mode].items():
        assert 0.9 * v <= floor_all[key] <= v, (key, floor_all[key], v)
