"""CPU tests of the operand-exact SIREN evaluator (tests/siren_emul.py): it is the plain MLP when nothing is rounded, its rounding
is torch's, and the error floor that no kernel can beat (operands pushed across a 16-bit rounding boundary by a different fp32
accumulation order) is the one recorded in siren_emul.FLIP_FLOOR, which the GPU test (test_hip_siren_operand_exact.py) builds on.
Nothing here needs the kernels or their library: the input sets and the switches of the families live in siren_emul."""
import math
import os
import shutil
import subprocess

import pytest
import torch

import siren_emul as se

ALL_CASES = [(fam, c) for fam, cs in se.CASES.items() for c in cs]
IDS = ["%s-w%d-nh%d-F%d-C%d-P%d-N%dS%d-%s-%s" % (f, c["hidden"], c["nh"], c["F"], c["C"], c["P"], c["N"], c["S"], c["scale"], c["variant"])
       + ("-E%d-%s" % (c["E"], "x".join(map(str, c["hidden_dims"] or ()))) if f in se.CASES_FP32 else "") for f, c in ALL_CASES]
CASES_16BIT = [(f, c) for f, c in ALL_CASES if f not in se.CASES_FP32]      # the fp32 families round to no operand type


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
    if a.numel() == 0:                # E = 0: dpe has no element (autograd may leave its gradient unset)
        return 0.0
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
    for fam, c in CASES_16BIT:
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


# ---- the fp32 families (test_hip_siren_fp32_exact.py): premises of its limits, without a kernel ------------------------------------
FP32_FAMILIES = sorted(se.CASES_FP32)


def _route_program(tmp):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp / "siren_case_routes")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(os.path.dirname(os.path.abspath(__file__)), "siren_case_routes.cpp"), "-o", exe],
                   check=True)
    return exe


def test_fp32_cases_name_every_instance_of_the_route(tmp_path):
    """siren_route.h itself (compiled alone, tests/siren_case_routes.cpp) on the descriptor of every case of CASES_FP32: it
    accepts each, names the same instance in the three modes, that instance is the one siren_emul.fp32_route restates (which the
    GPU test asserts before it runs a case) and belongs to the case's family; and every instance of RCB_SIREN_FP32_INSTANCES and
    both layer capacities of the plain-FMA kernel are named by at least one case."""
    flat = [(fam, c) for fam in FP32_FAMILIES for c in se.CASES_FP32[fam]]
    args = [",".join(map(str, [c["hidden"], c["nh"], c["F"], c["E"], c["C"], c["P"], c["N"] * c["S"], c["S"]]
                         + list(c["hidden_dims"] or ()) + [0] * (4 - len(c["hidden_dims"] or ())))) for _, c in flat]
    run = subprocess.run([_route_program(tmp_path)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    lines = run.stdout.decode().splitlines()
    instances = {tuple([ln.split()[1]] + [int(v) for v in ln.split()[2:]]) for ln in lines if ln.startswith("instance ")}
    assert len(instances) == 8 and ("generic", 5) in instances and ("generic", 8) in instances
    routes = [ln.split(" -> ")[1].split() for ln in lines if ln.startswith("route ")]
    assert len(routes) == len(flat)
    named = set()
    for (fam, c), r in zip(flat, routes):
        got = tuple([r[0]] + [int(v) for v in r[1:]]) if r[0] != "refused" else None
        assert got == se.fp32_route(c) and got is not None and got[0] == fam, (fam, c, r)
        named.add(got)
    assert named == instances, instances - named


@pytest.mark.parametrize("family", FP32_FAMILIES)
def test_fp32_case_sets_are_small(family):
    """one to five 32-pixel tiles, at most 4 rows; E = 0, S = 2 with a shared target and both scale groups are there"""
    cs = se.CASES_FP32[family]
    assert all(1 <= c["P"] <= 160 and c["N"] * c["S"] <= 4 and c["variant"] == "f32pe" and c["chunks"] == 1 for c in cs)
    assert any(c["E"] == 0 for c in cs) and any(c["S"] == 2 for c in cs) and {c["scale"] for c in cs} == {"init", "model"}
    assert se.DISCRIMINATION[family] in cs and se.DISCRIMINATION[family]["P"] % 32


@pytest.mark.parametrize("family", FP32_FAMILIES)
def test_fp32_restatement_reversed_is_the_same_problem(family):
    """the two runs of fp32_restatement state one problem: they agree with each other at fp32 level on every block, the reversed
    run's outputs permuted back; and they are two summation orders, not one evaluation taken twice: not bit-identical"""
    differ = 0
    for c in se.CASES_FP32[family]:
        case = se.build(c)
        a, b = se.fp32_restatement(case), se.fp32_restatement(case, reverse=True)
        stats = se.block_stats(se.block_errors(case, a, {k: v.double() for k, v in b.items()}))
        assert max(stats.values()) < 1e-5, (c, stats)
        differ += any(not torch.equal(a[k], b[k]) for k in a)
    assert differ > len(se.CASES_FP32[family]) // 2


@pytest.mark.parametrize("family", FP32_FAMILIES)
def test_fp32_limits_meet_the_condition(family):
    """no limit above 1e-4 of a block's largest entry at the initialisation scale, 1e-5 at the model scale: the restatement alone
    meets it (nothing here comes from a kernel); a case that breaks it gets smaller phases, not a wider condition.  Prints the
    yardstick."""
    limits = se.fp32_limits(family)
    assert set(limits) == {"init", "model"}
    for grp, tab in se.fp32_yardstick(family).items():
        print("%s %s yardstick: %s" % (family, grp, "  ".join("%s/%s/%s %.2e" % (k + (v,)) for k, v in sorted(tab.items()))))
        assert {k[:2] for k in tab} >= {("y", "row"), ("sse", "row"), ("dW", "bias"), ("dW", "fourier"), ("dW", "pe"), ("dpe", "row"),
                                        ("bwd_dW", "bias"), ("bwd_dW", "fourier"), ("bwd_dW", "pe"), ("bwd_dpe", "row")}
        for k, v in limits[grp].items():
            assert se.LIMIT_FLOOR <= v <= se.FP32_CONDITION[grp], (family, grp, k, v)


FP32_FAULTS = [("layer 0's bias gradient x (1 + 2^-10)", dict(bias_grad_scale=(0, 1.0 + 2.0 ** -10))),
               ("last valid pixel left out of dW", dict(drop_last_pixel=True)),
               ("Fourier half of layer 0's dW x (1 + 2^-10)", dict(fourier_scale=1.0 + 2.0 ** -10)),
               ("last valid pixel's dz leaks into a padded slot", dict(leak_last_dz=True))]


@pytest.mark.parametrize("family", FP32_FAMILIES)
def test_fp32_limits_discriminate(family):
    """each deliberate mistake, applied to the fp64 evaluator alone and judged like a kernel's output, exceeds the limit of at
    least one key of the family's designated case, and of no output but the weight gradients, which alone they touch.  Printed
    beside it: the whole-tensor rel_err of the fp32-yardstick tests, whose limit on dW is 1e-4."""
    c = se.DISCRIMINATION[family]
    case = se.build(c)
    ref = se.run_emul(case, None)
    limits = se.fp32_limits(family)[c["scale"]]
    assert not se.over_limits(se.block_stats(se.block_errors(case, se.fp32_restatement(case), ref)), limits)
    for name, kw in FP32_FAULTS:
        wrong = se.run_emul(case, None, faults=se.Faults(**kw))
        bad = se.over_limits(se.block_stats(se.block_errors(case, wrong, ref)), limits)
        whole = max(_rel(wrong[k], ref[k]) for k in ("dW", "bwd_dW"))
        print("%s: %-48s %d keys above their limit; whole-tensor rel_err %.1e" % (family, name, len(bad), whole))
        assert bad and {k[0] for k, _, _ in bad} <= {"dW", "bwd_dW"}, (name, bad)
