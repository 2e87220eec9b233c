"""The sub-pixel convolution kernels of the upsampling net (upconv.hip, phaseconv.hip, stage1.hip and their weight maps) against the
fp64 evaluator of tests/upconv_emul.py, which is written from the definition of the stage and rounds where the kernels round.

Two checks, neither with a measured number in it:

  lattice   small-integer inputs on which every partial sum is exact in fp32 (the evaluator asserts sum |product| / lsb < 2^24 for
            every element of every output): the kernel must return the fp64 result, rounded once, BIT FOR BIT -- torch.equal, no
            element exempt.  A failure names the first differing element as (batch, position per axis, phase per axis, channel).
  gridded   bf16 activations at the scale of test_hip_upsample.py and taps on a 2^-12 grid: every element within
            |got - ref| <= u_out (|ref| + g) + g,  g = n 2^-23 sum |x_i w_i|  of the unrounded fp64 result (upconv_emul.bound).
            Lattice values cannot show a precision defect (a 16-bit accumulator, a second rounding, dropped low bits); these can.

Which shape reaches which kernel (the test ids carry the names):
  phaseconv_fwd    pc_fwd_kernel<nd, cout, act>: every case, cout 64 with LeakyReLU, cout 16 linear (the 16 x 16 x 32 MFMA branch)
  phaseconv_dgrad  pc_dgrad64_kernel<nd> at cout 64, pc_dgrad_kernel<nd, 16> at cout 16 (the dispatch looks at nothing else)
  phaseconv_wgrad  pc_wgrad1d_kernel on 1-D shapes, pc_wgrad2d_kernel on 2-D, pc_wgrad_kernel<3, .> on 3-D (+ reduce, fold)
                   (2, 600): 19 tiles in a row, a workgroup walks several tile groups; (1, 1..): one pixel, every tap but one in the halo
  stage1_1d_*      s1_fwd1d_kernel, s1_dgrad1d_kernel, s1_wgrad1d_kernel + s1_wgrad_sum_kernel, Wbig from rcb_phase_bigweight
  rcb_upconv_fwd   upconv_fwd2_reg_kernel<1> (fp32 pre-activation), <3> (bf16 pre-activation): B 1, 3, 5 (clamped last group of four),
                   257, 261, and 1027 = the second trip of workgroup 0 with a clamped group; upconv_fwd3_lds_kernel<16, 0, 8> (fp32
                   linear out), <16, 1, 8> (bf16 linear out): B 257 / 261 = second image of a workgroup; <16, ., 4>: B 769 in a child
                   process with RCB_UPCONV_HALF_WG=1
  rcb_upconv_dgrad upconv_dgrad2_reg_kernel<1>, <0> with the channel sums of dx; upconv_dgrad3_lds_kernel<16, 0> (fp32 dy), <16, 1>
  rcb_upconv_wgrad upconv_wgrad_kernel<64, 8, 1, 0>, <64, 8, 3, 0>, <16, 16, 0, 1> (fp32 dy), <16, 16, 0, 0> + upconv_wgrad_reduce_kernel
  rcb_upconv_bwd_fused  upconv_bwd3_fused_kernel (bf16 dy)
each of the upconv kernels with fragments built in the kernel (pack=None) and with the pack of rcb_upconv_weff_build.

The chains (CIFAR stages 2 -> 3 and the stitched 2-D path through rcb_tile_gather / _crop / _fold, forward and backward) run on
non-negative lattice data and are held to bit equality against the evaluator on the WHOLE grid: there is no seam.  One exception,
as the condition cannot be met there at any operand range: dz1 of the STITCHED backward.  A source pixel shared by two tiles gets
bf16(bf16(part A) + bf16(part B)) from rcb_tile_fold where the whole grid rounds the sum once, and the parts are sums of ~1000
products of a bf16-rounded dz2, not bf16 integers.  It is held to the a-priori bound instead, with u_out = 2^-8 for each of the two
roundings on its way (the parts are non-negative: their rounding errors add up to at most 2^-8 of the sum); every other output
of the stitched chain, dz2 included, is bit-equal.

The fp32-dy modes of stage 3 round dy to bf16 when they commit it to LDS (the MFMA operand is bf16 in every mode; DESIGN and
upsample_cifar_hip say so).  The evaluator mirrors that with its `dy` switch, the gridded fp32 dy carries fp32 mantissas, and the
discrimination test flips the switch: an evaluator that rounds dy on the other side of the mode switch than the kernels fails.

Worst error / bound on the first MI355X run (for information; no limit is derived from them): see RATIOS below.
"""
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":                                   # the child process of test_half_workgroup_instances
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(_here), _here]

import upconv_emul as ue  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
bf = torch.bfloat16

# worst |got - ref| / bound per kernel on gridded inputs, first MI355X run (printed by test_gridded_inputs_within_the_a_priori_bound)
RATIOS = """
phaseconv 1-D (2, 33)        cout 64: y 0.971  dx 0.925  dW 0.006  db 0.000     cout 16: y 0.946  dx 0.977  dW 0.004  db 0.000
phaseconv 2-D (2, 5, 33)     cout 64: y 0.966  dx 0.835  dW 0.000  db 0.000     cout 16: y 0.977  dx 0.971  dW 0.000  db 0.000
phaseconv 3-D (1, 2, 3, 32)  cout 64: y 0.966  dx 0.581  dW 0.000  db 0.000     cout 16: y 0.958  dx 0.844  dW 0.000  db 0.000
stage1_1d (2, 33)            y 0.915  dx 0.001  dW 0.012  db 0.000
upconv stage 2, B = 3        fp32 z1: y 0.970  dx 0.000 (fp32)  dW 0.003  db 0.000  dbx 0.000     bf16 z1: y 0.963  dx 0.818  dW 0.003  db 0.000  dbx 0.084
upconv stage 3, B = 3        fp32 out / dy: y 0.011  dx 0.959  dW 0.001  db 0.000     bf16 out / dy: y 0.967  dx 0.959  dW 0.001  db 0.000 (fused: the same)
stitched dz1 (two roundings) grid (5, 7): 0.988     grid (8, 12): 0.984
(a bf16 result sits just below 1 by construction: rounding to nearest uses all of u_out; the fp32 results show the room g leaves)
"""


# ---- running the kernels of a case -----------------------------------------------------------------------------------------------
def _kernel_names(case):
    nd = len(case.shape) - 1
    if case.kernel == "phaseconv":
        return "pc_fwd<%d,%d,%d>+%s+%s" % (nd, case.cout, case.leaky, "pc_dgrad64<%d>" % nd if case.cout == 64 else "pc_dgrad<%d,16>" % nd,
                                           {1: "pc_wgrad1d", 2: "pc_wgrad2d", 3: "pc_wgrad<3>"}[nd])
    if case.kernel == "stage1":
        return "s1_fwd1d+s1_dgrad1d+s1_wgrad1d"
    if case.kernel == "upconv2":
        m = 1 if case.x_mode == "pre_f32" else 3
        return "upconv_fwd2_reg<%d>+upconv_dgrad2_reg<%d>+upconv_wgrad<64,8,%d,0>" % (m, m == 1, m)
    o, d = int(case.out == "bf16"), int(case.dy == "bf16")
    return "upconv_fwd3_lds<16,%d,8>+upconv_dgrad3_lds<16,%d>+upconv_wgrad<16,16,0,%d>%s" % (o, d, 1 - d, "+upconv_bwd3_fused" if d else "")


def _id(case):
    return case.id + "-" + _kernel_names(case)


def _x_tensor(case, x):
    return x.float() if case.x_mode in ("pre_f32", "f32") else x.to(bf)


def _weff(case, inp, use_pack):
    """-> (Weff fp32 [2, 2, 64, 2, 2, cout], pack | None).  pack=None: the fp32 effective weights come from the evaluator (exact tap
    sums) and the kernels build their fragments themselves; otherwise both come from rcb_upconv_weff_build"""
    from recombiner_amd import ops
    if not use_pack:
        return ue.eff_layout(ue.tap_weights(inp.W, case.geo, "f32"), case.geo).float().contiguous(), None
    gen = torch.Generator().manual_seed(9)
    W1 = torch.randint(-7, 8, (64, 128, 5, 5), generator=gen).float().to(DEV)
    b1 = torch.randint(-7, 8, (64,), generator=gen).float().to(DEV)
    other = torch.randint(-7, 8, (16, 64, 3, 3) if case.kernel == "upconv2" else (64, 64, 3, 3), generator=gen).float().to(DEV)
    W2, W3 = (inp.W.float(), other) if case.kernel == "upconv2" else (other, inp.W.float())
    _, _, e2, e3, pack = ops.upconv_weff_build(W1, b1, W2.contiguous(), W3.contiguous(), True)
    return (e2 if case.kernel == "upconv2" else e3), pack


def run_kernels(case, inp, want=("fwd", "dgrad", "wgrad"), use_pack=False, fused=False):
    """the kernels of `case` on `inp` (fp64 tensors on the GPU holding values of the kernels' types) -> namespace of fp64 results"""
    from recombiner_amd import ops
    from types import SimpleNamespace
    r = SimpleNamespace()
    x, W, b = _x_tensor(case, inp.x).contiguous(), inp.W.float().contiguous(), inp.b.float().contiguous()
    dy = (inp.dy.float() if case.dy == "f32" else inp.dy.to(bf)).contiguous()
    if case.kernel == "phaseconv":
        ff, fd = ops.phaseconv_pack(W)
        if "fwd" in want:
            r.y = ops.phaseconv_fwd(x, ff, b, case.cout, case.leaky)
        if "dgrad" in want:
            r.dx = ops.phaseconv_dgrad(dy, fd, x)
        if "wgrad" in want:
            r.dW, r.db = ops.phaseconv_wgrad(x, dy)
    elif case.kernel == "stage1":
        r.wbig = ops.phase_bigweight(W, [4], 5, 2, bf)
        if "fwd" in want:
            r.y = ops.stage1_1d_fwd(x, r.wbig, b)
        if "dgrad" in want:
            r.dx = ops.stage1_1d_dgrad(dy, r.wbig)
        if "wgrad" in want:
            r.dW, r.db = ops.stage1_1d_wgrad(x, dy)
    else:
        weff, pack = _weff(case, inp, use_pack)
        grid = case.shape[1]
        pre = case.kernel == "upconv2"
        if "fwd" in want:
            r.y = ops.upconv_fwd(x, weff, b, grid, case.cout, out_f32=case.out == "f32", preact=pre,
                                 linear_bf16=(not pre) and case.out == "bf16", pack=pack)
        if fused:
            r.dx, r.dW, r.db = ops.upconv_bwd_fused(dy, weff, x, grid, case.cout, pack=pack)
        else:
            if "dgrad" in want:
                if pre:
                    r.dx, part = ops.upconv_dgrad(dy, weff, x, grid, case.cout, preact=True, want_dbias=True, pack=pack)
                    assert part.shape[0] == min(case.shape[0], 256)
                    r.dbx = part.double().sum(0)                    # the partial sums, added up (exact on the lattice)
                    r.dbx_parts = part.shape[0]
                else:
                    r.dx = ops.upconv_dgrad(dy, weff, x, grid, case.cout, pack=pack)
            if "wgrad" in want:
                r.dW, r.db = ops.upconv_wgrad(x, dy, grid, case.cout, preact=pre)
    torch.cuda.synchronize()
    for k, v in list(vars(r).items()):
        if torch.is_tensor(v):
            setattr(r, k, v.double())
    return r


_REFS = {}


def _lattice(case, want=("fwd", "dgrad", "wgrad")):
    """the lattice inputs and the evaluator's results of a case, computed once (on the GPU) and shared by the tests; unchanged"""
    key = (case, tuple(want))
    if key not in _REFS:
        if len(_REFS) > 6:
            _REFS.clear()
        _REFS[key] = ue.lattice(case, DEV, want)
    return _REFS[key]


def assert_bit_equal(case, got, ref, names, tag=""):
    bad = []
    for name in names:
        g, r = getattr(got, name), getattr(ref, name)
        if r is None:
            continue
        assert g.shape == r.shape, (name, g.shape, r.shape)
        if not torch.equal(g, r):
            bad.append("%s %s%s: %s" % (case.id, name, tag, ue.first_difference(g, r, case, name)))
    assert not bad, "\n".join(bad)


# ---- a. rcb_phaseconv_* ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ue.PHASECONV_CASES, ids=[_id(c) for c in ue.PHASECONV_CASES])
def test_phaseconv_kernels_bit_equal_on_the_lattice(case):
    inp, ref = _lattice(case)
    got = run_kernels(case, inp)
    assert_bit_equal(case, got, ref, ("y", "dx", "dW", "db"))
    again = run_kernels(case, inp, want=("wgrad",))
    assert torch.equal(again.dW, got.dW) and torch.equal(again.db, got.db)


# ---- b. rcb_stage1_1d_* ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ue.STAGE1_CASES, ids=[_id(c) for c in ue.STAGE1_CASES])
def test_stage1_1d_kernels_bit_equal_on_the_lattice(case):
    from recombiner_amd import ops
    inp, ref = _lattice(case)
    got = run_kernels(case, inp)
    Wt = ue.tap_weights(inp.W, case.geo, "f32")
    big = ue.big_layout(Wt, case.geo)
    assert torch.equal(got.wbig, ue.bf16(big)), ue.first_difference(got.wbig, ue.bf16(big), case, "Wbig")
    assert torch.equal(ops.phase_bigweight(inp.W.float(), [4], 5, 2, torch.float32).double(), big)
    assert_bit_equal(case, got, ref, ("y", "dx", "dW", "db"))
    reads = ue.big_layout(torch.ones_like(Wt), case.geo) != 0                  # the structure, whatever the tap values
    assert bool((got.dW[~reads] == 0).all()), "dwbig must be exactly zero wherever no phase reads"
    # the adjoint map back onto the conv weight: sums of a few integers
    dW = ops.phase_bigweight_grad(got.dW.float(), tuple(inp.W.shape), [4], 5, 2).double()
    dWp = ue.wgrad_acc(ue.operand(case, inp.x, case.rounding), inp.dy, case.geo)[0]
    assert torch.equal(dW, ue.conv_layout(dWp))


# ---- c. rcb_upconv_* ------------------------------------------------------------------------------------------------------------
UPCONV_CASES = ue.UPCONV2_CASES + ue.UPCONV2_SLOPE_CASES + ue.UPCONV3_CASES


@pytest.mark.parametrize("use_pack", [False, True], ids=["fragments_in_kernel", "weff_build_pack"])
@pytest.mark.parametrize("case", UPCONV_CASES, ids=[_id(c) for c in UPCONV_CASES])
def test_upconv_kernels_bit_equal_on_the_lattice(case, use_pack):
    inp, ref = _lattice(case)
    got = run_kernels(case, inp, use_pack=use_pack)
    names = ("y", "dx", "dW", "db") + (("dbx",) if case.kernel == "upconv2" else ())
    assert_bit_equal(case, got, ref, names)
    if case.kernel == "upconv3" and case.dy == "bf16":
        fused = run_kernels(case, inp, want=(), use_pack=use_pack, fused=True)
        assert_bit_equal(case, fused, ref, ("dx", "dW", "db"), " (upconv_bwd_fused)")


@pytest.mark.parametrize("use_pack", [False, True], ids=["fragments_in_kernel", "weff_build_pack"])
@pytest.mark.parametrize("case", ue.UPCONV2_FWD_ONLY, ids=[c.id + "-upconv_fwd2_reg-second_trip" for c in ue.UPCONV2_FWD_ONLY])
def test_stage2_forward_second_trip(case, use_pack):
    """B = 1027: 257 groups of four on 256 workgroups -- workgroup 0 makes a second trip, and its group holds three datapoints"""
    inp, ref = _lattice(case, ("fwd",))
    assert_bit_equal(case, run_kernels(case, inp, ("fwd",), use_pack=use_pack), ref, ("y",))


def test_weff_build_and_grad_exact_on_lattice_taps():
    """rcb_upconv_weff_build: Weff1 (the dense map of stage 1 on the 2 x 2 latent grid), Weff2, Weff3 are sums of a few integers,
    the bf16 Weff1 their rounding; rcb_upconv_weff_grad: the adjoint, on integer gradients"""
    from recombiner_amd import ops
    gen = torch.Generator().manual_seed(21)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float().to(DEV)       # noqa: E731
    W1, b1, W2, W3 = ri(-7, 7, 64, 128, 5, 5), ri(-7, 7, 64), ri(-7, 7, 64, 64, 3, 3), ri(-7, 7, 16, 64, 3, 3)
    g1, g2 = ue.Geo(4, 5, 2, 2), ue.Geo(2, 3, 1, 2)
    M1 = ue.dense_map(W1.double(), (2, 2), g1)
    E2 = ue.eff_layout(ue.tap_weights(W2.double(), g2, "f32"), g2)
    E3 = ue.eff_layout(ue.tap_weights(W3.double(), g2, "f32"), g2)
    for bf16_out in (False, True):
        e1, b1rep, e2, e3, _ = ops.upconv_weff_build(W1, b1, W2, W3, bf16_out)
        assert torch.equal(e1.double(), ue.bf16(M1) if bf16_out else M1)
        assert torch.equal(e2.double(), E2) and torch.equal(e3.double(), E3)
        assert torch.equal(b1rep.double().view(64, 64), (ue.bf16(b1.double()) if bf16_out else b1.double()).expand(64, 64))
    d1, d2, d3 = ri(-4, 4, 512, 4096), ri(-4, 4, 2, 2, 64, 2, 2, 64), ri(-4, 4, 2, 2, 64, 2, 2, 16)
    part = ri(-4, 4, 261, 64)
    r1 = ue.dense_map_grad(d1.double(), (64, 128, 5, 5), (2, 2), g1)
    r2, r3 = ue.eff_grad_to_conv(d2.double(), g2), ue.eff_grad_to_conv(d3.double(), g2)
    for d1_in in (d1, d1.to(bf)):
        o1, o2, o3, ob = ops.upconv_weff_grad(d1_in, d2, d3, part)
        assert torch.equal(o1.double(), r1) and torch.equal(o2.double(), r2) and torch.equal(o3.double(), r3)
        assert torch.equal(ob.double(), part.double().sum(0))


# ---- d. the half-workgroup instances ----------------------------------------------------------------------------------------------
def _half_wg_child():
    """B = 769 through upconv_fwd3_lds_kernel<16, 0, 4> and <16, 1, 4> (768 four-wave workgroups: one makes a second trip)"""
    assert os.environ.get("RCB_UPCONV_HALF_WG") == "1"
    for case in (ue.HALF_WG_CASE, ue.upconv3_case(769, "bf16", "bf16", seed=61)):
        inp, ref = ue.lattice(case, DEV, ("fwd",))
        for use_pack in (False, True):
            got = run_kernels(case, inp, ("fwd",), use_pack=use_pack)
            d = ue.first_difference(got.y, ref.y, case, "y")
            if d is not None:
                print("MISMATCH %s pack=%s: %s" % (case.id, use_pack, d))
                return 1
    print("half-workgroup instances: bit-equal at B = 769")
    return 0


def test_half_workgroup_instances_bit_equal_in_a_child_process():
    """RCB_UPCONV_HALF_WG is read once per process: one fresh child with the switch on"""
    env = dict(os.environ, RCB_UPCONV_HALF_WG="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "half_wg"], env=env, timeout=240, capture_output=True, text=True)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert "bit-equal at B = 769" in p.stdout


# ---- e. the chains ----------------------------------------------------------------------------------------------------------------
def _chain_weights(inp):
    from recombiner_amd import ops
    gen = torch.Generator().manual_seed(5)
    W1 = torch.randint(0, 2, (64, 128, 5, 5), generator=gen).float().to(DEV)
    b1 = torch.ones(64, device=DEV)
    return W1, b1, ops.upconv_weff_build(W1, b1, inp.W2.float().contiguous(), inp.W3.float().contiguous(), True)


@pytest.mark.parametrize("cc", ue.CIFAR_CHAINS, ids=lambda c: c.id)
def test_cifar_stages_2_3_chain_bit_equal(cc):
    """stage 2 -> stage 3 forward and their backward, as _UpsampleCifarFn strings the kernels together: h2 and dz2 are bf16 roundings
    of exact sums, which the evaluator makes too; every output bit-equal"""
    from recombiner_amd import ops
    inp = ue.chain_inputs(cc, DEV)
    ref = ue.chain23(cc, inp)
    _, _, (_, _, e2, e3, pack) = _chain_weights(inp)
    z1 = inp.z1.float() if cc.z1 == "pre_f32" else inp.z1.to(bf)
    dpe = inp.dpe.float() if cc.pe == "f32" else inp.dpe.to(bf)
    b2, b3 = inp.b2.float(), inp.b3.float()
    h2 = ops.upconv_fwd(z1, e2, b2, 8, 64, out_f32=False, preact=True, pack=pack)
    pe = ops.upconv_fwd(h2, e3, b3, 16, 16, out_f32=cc.pe == "f32", linear_bf16=cc.pe == "bf16", pack=pack)
    if cc.pe == "bf16":
        dz2, dW3, db3 = ops.upconv_bwd_fused(dpe, e3, h2, 16, 16, pack=pack)
    else:
        dz2 = ops.upconv_dgrad(dpe, e3, h2, 16, 16, pack=pack)
        dW3, db3 = ops.upconv_wgrad(h2, dpe, 16, 16)
    dz1, part = ops.upconv_dgrad(dz2, e2, z1, 8, 64, preact=True, want_dbias=True, pack=pack)
    dW2, db2 = ops.upconv_wgrad(z1, dz2, 8, 64, preact=True)
    got = dict(h2=h2, pe=pe, dz2=dz2, dW3=dW3, db3=db3, dz1=dz1, dbx=part.double().sum(0), dW2=dW2, db2=db2)
    bad = [k for k, v in got.items() if not torch.equal(v.double(), getattr(ref, k))]
    assert not bad, bad


@pytest.mark.parametrize("cc", ue.STITCHED_CHAINS, ids=lambda c: c.id)
def test_stitched_2d_chain_has_no_seam(cc):
    """stages 2 / 3 of the stitched 2-D path (overlapping tiles through rcb_tile_gather / _crop / _fold) against the evaluator on
    the WHOLE grid: pe, dW2, db2, dW3, db3 bit-equal -- there is no seam.  dz1: see the module docstring (a-priori bound)."""
    from recombiner_amd.upsample_fast import _UpsampleStitched23Fn
    inp = ue.chain_inputs(cc, DEV)
    ref = ue.chain23(cc, inp)
    assert float(ref.S_dz2.max()) <= 256                      # the bf16 tile sums of dz2 that rcb_tile_fold adds are exact integers
    W1, b1, _ = _chain_weights(inp)
    z1 = inp.z1.to(bf).requires_grad_(True)
    params = [t.float().contiguous().requires_grad_(True) for t in (inp.W2, inp.b2, inp.W3, inp.b3)]
    pe = _UpsampleStitched23Fn.apply(z1, W1, b1, *params)
    assert pe.dtype == bf and torch.equal(pe.double(), ref.pe), ue.first_difference(pe.double(), ref.pe, ue.upconv3_case(1, "bf16", "bf16"), "y")
    dz1, dW2, db2, dW3, db3 = torch.autograd.grad(pe, [z1] + params, inp.dpe.to(bf))
    g2 = ue.Geo(2, 3, 1, 2)
    want = dict(dW2=ue.eff_grad_to_conv(ref.dW2, g2), db2=ref.db2, dW3=ue.eff_grad_to_conv(ref.dW3, g2), db3=ref.db3)
    bad = [k for k, v in dict(dW2=dW2, db2=db2, dW3=dW3, db3=db3).items() if not torch.equal(v.double(), want[k])]
    assert not bad, bad
    lim = ue.bound(ref.dz1, ref.S_dz1, ref.n_dz1, "bf16", roundings=2)          # the tile's rounding and rcb_tile_fold's
    ratio = float(((dz1.double() - ref.dz1).abs() / lim).max())
    print("%s: dz1 of the stitched backward, worst error / bound %.3f; %d of %d elements differ from the whole-grid rounding"
          % (cc.id, ratio, int((dz1.double() != ref.dz1).sum()), dz1.numel()))
    assert ratio <= 1.0


# ---- the a-priori bound on gridded inputs ------------------------------------------------------------------------------------------
GRIDDED_CASES = ([ue.phaseconv_case(s, c, seed=70 + i) for i, s in enumerate([(2, 33), (2, 5, 33), (1, 2, 3, 32)]) for c in (64, 16)]
                 + [ue.stage1_case(2, 33, seed=80)]
                 + [ue.upconv2_case(3, m, seed=81) for m in ("pre_f32", "pre_bf16")]
                 + [ue.upconv3_case(3, o, d, seed=82) for o, d in (("f32", "f32"), ("bf16", "bf16"))])


def _ratios(case, got, ref):
    """worst |got - ref| / bound per output; every element counts"""
    out = {}
    for name, S, n, typ in (("y", "S_y", "n_y", case.out), ("dx", "S_dx_out", "n_dx", case.dx), ("dW", "S_dW", "n_dW", "f32"),
                            ("db", "S_db", "n_db", "f32")):
        if hasattr(got, name) and hasattr(ref, name):
            r = getattr(ref, name)
            # stage 1 stores LeakyReLU(bf16(z)) as bf16: where the slope applies that is a second rounding (upconv_emul.bound)
            twice = (r < 0).to(F64) + 1 if (case.kernel == "stage1" and name == "y") else 1
            lim = ue.bound(r, getattr(ref, S), getattr(ref, n), typ, twice)
            e = (getattr(got, name) - r).abs()
            assert bool((e[lim == 0] == 0).all())
            out[name] = float((e / lim.clamp_min(1e-300)).max())
    if hasattr(got, "dbx") and hasattr(ref, "dbx"):
        # a sum of m stored dx values in any order: their own bounds, plus one ulp of a partial sum per addition
        li = ue.bound(ref.dx, ref.S_dx_out, ref.n_dx, case.dx).reshape(-1, case.cin)
        m = li.shape[0]
        lim = li.sum(0) + m * ue.EPS32 * (ref.dx.abs().reshape(-1, case.cin) + li).sum(0)
        out["dbx"] = float(((got.dbx - ref.dbx).abs() / lim).max())
    return out


@pytest.mark.parametrize("case", GRIDDED_CASES, ids=[_id(c) for c in GRIDDED_CASES])
def test_gridded_inputs_within_the_a_priori_bound(case):
    inp, ref = ue.gridded(case, DEV)
    runs = [("", run_kernels(case, inp))]
    if case.kernel.startswith("upconv"):
        runs.append((" pack", run_kernels(case, inp, use_pack=True)))
        if case.kernel == "upconv3" and case.dy == "bf16":
            runs.append((" fused", run_kernels(case, inp, want=(), fused=True)))
    for tag, got in runs:
        ratios = _ratios(case, got, ref)
        print("%s%s: worst error / bound  %s" % (_id(case), tag, "  ".join("%s %.3f" % kv for kv in ratios.items())))
        assert all(v <= 1.0 for v in ratios.values()), ratios


# ---- 4. the checks discriminate ---------------------------------------------------------------------------------------------------
def test_the_checks_see_what_the_whole_tensor_limits_cannot():
    """The kernels' outputs against deliberately wrong evaluators (upconv_emul.Faults; nothing is injected into a kernel): every one
    must FAIL its check -- bit equality on the lattice, the a-priori bound on gridded inputs -- while the right evaluator passes.
    Beside each: whether the whole-tensor limit of the matching test of test_hip_upsample.py (largest difference over largest
    entry) would have passed."""
    unseen = []
    for name, case, kw, out, old_limit, kind in ue.DISCRIMINATION:
        want = {"y": ("fwd",), "dx": ("dgrad",), "dW": ("wgrad",)}[out]
        if kind == "lattice":
            inp, ref = _lattice(case, want)
            got = getattr(run_kernels(case, inp, want), out)
            wrong = getattr(ue.evaluate(case, inp, faults=ue.Faults(**kw), want=want), out)
            assert torch.equal(got, getattr(ref, out)), name
            seen = not torch.equal(got, wrong)
            detail = "%d elements differ" % int((got != wrong).sum())
        else:
            inp, ref = ue.gridded(case, DEV, want=want)
            _, bad = ue.gridded(case, DEV, faults=ue.Faults(**kw), want=want)
            got = getattr(run_kernels(case, inp, want), out)
            wrong = getattr(bad, out)
            typ = {"y": case.out, "dx": case.dx, "dW": "f32"}[out]
            S, n = getattr(ref, {"dx": "S_dx_out"}.get(out, "S_" + out)), getattr(ref, "n_" + out)
            right = float(((got - getattr(ref, out)).abs() / ue.bound(getattr(ref, out), S, n, typ)).max())
            ratio = float(((got - wrong).abs() / ue.bound(wrong, getattr(bad, {"dx": "S_dx_out"}.get(out, "S_" + out)), n, typ)).max())
            assert right <= 1.0, (name, right)
            seen = ratio > 1.0
            detail = "worst error / bound %.1f (right evaluator: %.3f)" % (ratio, right)
        old = float((got - wrong).abs().max() / wrong.abs().max())
        print("%-75s %s: %s by the new check (%s); the old limit %.0e %s (%.1e)"
              % (name, kind, "SEEN" if seen else "NOT SEEN", detail, old_limit, "would have PASSED" if old < old_limit else "fails too", old))
        if not seen:
            unseen.append(name)
    assert not unseen, "faults the new checks do not see: %s" % unseen


if __name__ == "__main__":
    sys.exit(_half_wg_child() if sys.argv[1:] == ["half_wg"] else 2)
