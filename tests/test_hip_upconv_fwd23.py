"""Stages 2 + 3 of the CIFAR upsampling net's forward as ONE launch (rcb_upconv_fwd23 / upconv_fwd23_kernel) against the fp64
evaluator of tests/upconv_emul.py and against the two rcb_upconv_fwd launches it replaces.  No tolerance anywhere: every check
is bit equality.

The kernel is persistent (256 workgroups at most, each walking INRs blockIdx.x, + gridDim.x, ...), processes ONE image per
barrier interval and role, and pipelines its two roles one iteration apart, so the batch sizes are the ones at which that can go
wrong: 1 (fill and drain only), 2 .. 5 (few workgroups), 255 / 256 / 257 / 258 (no, one, two workgroups on a second trip:
g W + 1 and g W + g + 1 with g = 1 image per interval on W = 256 workgroups), 261, 513 (a third trip), 1027 and 2500 (most
workgroups on trip ten, some not)."""
import numpy as np
import pytest
import torch

import upconv_emul as ue

from recombiner_amd import _lib, config, ops, utils
from recombiner_amd import prior_model as PM
from recombiner_amd.upsample_fast import upsample_cifar_hip

pytestmark = pytest.mark.gpu

DEV = "cuda"
bf = torch.bfloat16
C3 = ue.upconv3_case(1, "bf16", "bf16")          # (geometry for ue.first_difference)
C2 = ue.upconv2_case(1, "pre_bf16")


def _eq(got, ref, case, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(got.double(), ref.double()), "%s: %s" % (what, ue.first_difference(got.double(), ref.double(), case, "y"))


def _pack(W2, W3, seed=9):
    """rcb_upconv_weff_build on (W2, W3) (the stage-1 part is not used here) -> (Weff2, Weff3, pack)"""
    gen = torch.Generator().manual_seed(seed)
    W1 = torch.randint(-7, 8, (64, 128, 5, 5), generator=gen).float().to(DEV)
    b1 = torch.randint(-7, 8, (64,), generator=gen).float().to(DEV)
    _, _, e2, e3, pack = ops.upconv_weff_build(W1, b1, W2.float().contiguous(), W3.float().contiguous(), True)
    return e2, e3, pack


# ---- a. the lattice chain against the evaluator ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 5, 257, 258, 261, 513, 1027])
def test_fused_forward_bit_equal_to_the_evaluator_on_the_lattice_chain(B):
    cc = ue.ChainCase(B, 8, 8, pe="bf16", z1="pre_bf16", seed=1)
    inp = ue.chain_inputs(cc, DEV)
    c2 = ue.Case("upconv2", (B, 8, 8), 64, x_mode="pre_bf16", leaky=True, dx="bf16", sign="nonneg")
    c3 = ue.Case("upconv3", (B, 16, 16), 16, out="bf16", dy="bf16", sign="nonneg")
    none = torch.zeros(1, dtype=ue.F64, device=DEV)
    from types import SimpleNamespace as NS
    f2 = ue.evaluate(c2, NS(x=inp.z1, W=inp.W2, b=inp.b2, dy=none), want=("fwd",))
    f3 = ue.evaluate(c3, NS(x=f2.y, W=inp.W3, b=inp.b3, dy=none), want=("fwd",))
    ue.assert_exact(cc.id + " h2", f2.S_y, inp.z1, ue.tap_weights(inp.W2, c2.geo, "bf16"))
    ue.assert_exact(cc.id + " pe", f3.S_y, f2.y, ue.tap_weights(inp.W3, c3.geo, "bf16"))
    _, _, pack = _pack(inp.W2, inp.W3, seed=5)
    h2, pe = ops.upconv_fwd23(inp.z1.to(bf), inp.b2.float(), inp.b3.float(), pack)
    torch.cuda.synchronize()
    assert h2.dtype == bf and pe.dtype == bf
    _eq(h2, f2.y, c2, "h2")
    _eq(pe, f3.y, c3, "pe")


# ---- b. LeakyReLU: signed lattice stage-2 cases -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 261])
def test_fused_forward_h2_on_signed_lattice_data(B):
    case = ue.upconv2_case(B, "pre_bf16", sign="mixed", amp=2, tap=1, seed=45 + B)
    inp, ref = ue.lattice(case, DEV, ("fwd",))
    assert bool((ref.y < 0).any()) and bool((inp.x < 0).any()), "the case must put values under the slope"
    gen = torch.Generator().manual_seed(3)
    W3 = torch.randint(-1, 2, (16, 64, 3, 3), generator=gen).float().to(DEV)
    b3 = torch.randint(-2, 3, (16,), generator=gen).float().to(DEV)
    _, _, pack = _pack(inp.W, W3)
    h2, _ = ops.upconv_fwd23(inp.x.to(bf), inp.b.float(), b3, pack)
    _eq(h2, ref.y, case, "h2")


# ---- c. against the two launches on signed random data ------------------------------------------------------------------------------
_RANDOM = {}


def _random_net(Bmax=2500):
    """data at the scale of tests/test_hip_upsample.py: z1 ~ N(0, 1) in bf16, conv weights and biases as torch.nn initialises them;
    made once, shared, unchanged"""
    if not _RANDOM:
        torch.manual_seed(0)
        net = PM.Upsample(2, [2, 1, 1], [4, 2, 2]).to(DEV)
        z1 = torch.randn(Bmax, 8, 8, 64, device=DEV).to(bf)
        with torch.no_grad():
            e1, b1rep, e2, e3, pack = ops.upconv_weff_build(net.conv1.weight, net.conv1.bias, net.conv2.weight, net.conv3.weight, True)
        _RANDOM.update(net=net, z1=z1, e2=e2, e3=e3, pack=pack, b2=net.conv2.bias.detach().contiguous(),
                       b3=net.conv3.bias.detach().contiguous())
    return _RANDOM


def _two_launches(r, z1):
    h2 = ops.upconv_fwd(z1, r["e2"], r["b2"], 8, 64, out_f32=False, preact=True, pack=r["pack"])
    pe = ops.upconv_fwd(h2, r["e3"], r["b3"], 16, 16, out_f32=False, linear_bf16=True, pack=r["pack"])
    return h2, pe


@pytest.mark.parametrize("B", [1, 2, 3, 5, 255, 256, 257, 261, 513, 1027, 2500])
def test_fused_forward_equals_the_two_launches(B):
    r = _random_net()
    z1 = r["z1"][:B].contiguous()
    h2_ref, pe_ref = _two_launches(r, z1)
    assert bool((h2_ref < 0).any()) and bool((pe_ref < 0).any())
    h2, pe = ops.upconv_fwd23(z1, r["b2"], r["b3"], r["pack"])
    _eq(h2, h2_ref, C2, "h2")
    _eq(pe, pe_ref, C3, "pe")
    h2b, peb = ops.upconv_fwd23(z1, r["b2"], r["b3"], r["pack"])          # a second launch: the same bits
    assert torch.equal(h2b, h2) and torch.equal(peb, pe)


@pytest.mark.parametrize("B", [1, 5, 261])
def test_fused_forward_writes_nothing_behind_its_outputs(B):
    r = _random_net()
    z1 = r["z1"][:B].contiguous()
    h2_ref, pe_ref = _two_launches(r, z1)
    guard = 3                                                   # rows of canary behind row B - 1
    canary = -1234.0
    h2_buf = torch.full((B + guard, 16, 16, 64), canary, device=DEV, dtype=bf)
    pe_buf = torch.full((B + guard, 32, 32, 16), canary, device=DEV, dtype=bf)
    h2, pe = ops.upconv_fwd23(z1, r["b2"], r["b3"], r["pack"], out=(h2_buf[:B], pe_buf[:B]))
    torch.cuda.synchronize()
    assert h2.data_ptr() == h2_buf.data_ptr() and pe.data_ptr() == pe_buf.data_ptr()
    _eq(h2_buf[:B], h2_ref, C2, "h2")
    _eq(pe_buf[:B], pe_ref, C3, "pe")
    assert bool((h2_buf[B:] == canary).all()), "h2: written behind row B - 1"
    assert bool((pe_buf[B:] == canary).all()), "pe: written behind row B - 1"


# ---- d. the refusals ---------------------------------------------------------------------------------------------------------------
def test_other_combinations_are_refused_and_the_autograd_function_keeps_the_two_launches(monkeypatch):
    r = _random_net()
    B = 5
    z1 = r["z1"][:B].contiguous()
    for kw, args in ((dict(), (z1.float(), r["b2"], r["b3"], r["pack"])),                 # fp32 z1
                     (dict(pe_f32=True), (z1, r["b2"], r["b3"], r["pack"])),              # fp32 pe
                     (dict(), (z1, r["b2"], r["b3"], None))):                             # no pack
        with pytest.raises(_lib.RcbError, match="code -3"):
            ops.upconv_fwd23(*args, **kw)
        assert ops.upconv_fwd23(*args, refuse_ok=True, **kw) is None
    # the autograd function: fp32 z1 (stage1_bf16 = False) and fp32 pe with the switch on give what they give with it off
    fused_calls = []
    real = ops.upconv_fwd23

    def counting(*a, **k):
        out = real(*a, **k)
        fused_calls.append(out is not None)
        return out
    monkeypatch.setattr(ops, "upconv_fwd23", counting)
    torch.manual_seed(1)
    lpe = 0.1 * torch.randn(1, B, 2, 2, 128, device=DEV)
    with torch.no_grad():
        for s1, p16 in ((False, False), (False, True), (True, False)):
            on = upsample_cifar_hip(r["net"], lpe, s1, p16, fwd_fused=True)
            off = upsample_cifar_hip(r["net"], lpe, s1, p16, fwd_fused=False)
            assert on.dtype == off.dtype and torch.equal(on, off)
        assert not any(fused_calls), fused_calls
        on = upsample_cifar_hip(r["net"], lpe, True, True, fwd_fused=True)
        assert fused_calls[-1] is True
        assert torch.equal(on, upsample_cifar_hip(r["net"], lpe, True, True, fwd_fused=False))


# ---- e. the autograd function ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 261])
def test_autograd_function_with_the_switch_on_equals_off(B):
    torch.manual_seed(2)
    net = PM.Upsample(2, [2, 1, 1], [4, 2, 2]).to(DEV)
    lpe0 = 0.1 * torch.randn(1, B, 2, 2, 128, device=DEV)
    g = torch.randn(B, 1, 1024, 16, device=DEV).to(bf)
    res = []
    for fused in (True, False):
        lpe = lpe0.clone().requires_grad_(True)
        pe = upsample_cifar_hip(net, lpe, True, True, fwd_fused=fused)
        grads = torch.autograd.grad(pe, [lpe] + list(net.parameters()), g)
        res.append((pe.detach(), grads))
    (pe_on, g_on), (pe_off, g_off) = res
    assert torch.equal(pe_on, pe_off)
    assert len(g_on) == len(g_off) == 7
    for k, (a, b) in enumerate(zip(g_on, g_off)):
        assert torch.equal(a, b), "gradient %d differs" % k


# ---- f. the training step ----------------------------------------------------------------------------------------------------------
def _set_switch(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("RCB_UPCONV_FWD_FUSED", raising=False)
    else:
        monkeypatch.setenv("RCB_UPCONV_FWD_FUSED", value)


class _Count:
    """counts the fused launches that went out (ops.upconv_fwd23 returning its outputs)"""

    def __init__(self, monkeypatch):
        self.n, self.real, self.mp = 0, ops.upconv_fwd23, monkeypatch
        monkeypatch.setattr(ops, "upconv_fwd23", self)

    def __call__(self, *a, **k):
        out = self.real(*a, **k)
        self.n += int(out is not None)
        return out

    def stop(self):
        self.mp.setattr(ops, "upconv_fwd23", self.real)
        return self.n


def _prior_setup(n, precision, stage1_bf16=True):
    cfg = config.configs["cifar"]
    X, Y = utils.synthetic_inputs(cfg["pixel_sizes"], cfg["fourier_dim"], n, 3, seed=2)
    Xd, Yd = X.to(DEV)[None].expand(n, -1, -1), Y.to(DEV)
    torch.manual_seed(77)                      # (the in-kernel noise seed takes torch.initial_seed() in)
    m = PM.PriorBNNmodel(cfg["input_dim"], cfg["hidden_dims"], cfg["output_dim"], n, cfg["data_dim"], cfg["pixel_sizes"],
                         cfg["upsample_factors"], cfg["latent_dim"], False, None, None, random_seed=42, device=DEV)
    m.precision = precision
    m.stage1_bf16 = stage1_bf16
    torch.manual_seed(123)
    lt = PM.LinearTransform(m.dims).to(DEV)
    torch.manual_seed(124)
    up = PM.Upsample(2, cfg["paddings"], cfg["layerwise_scale_factors"]).to(DEV)
    D, s0 = m._d_net, 0.0211547
    pri = [torch.zeros(D, device=DEV), torch.full((D,), s0, device=DEV), torch.zeros(2, 2, 128, device=DEV),
           torch.full((2, 2, 128), s0, device=DEV)] + [None] * 4
    return m, lt, up, Xd, Yd, pri


def _train(monkeypatch, switches, n=64, steps=12, precision=1, stage1_bf16=True):
    """one train() call per entry of `switches` on ONE model -> (logs, parameters, fused launches per call)"""
    m, lt, up, Xd, Yd, pri = _prior_setup(n, precision, stage1_bf16)
    out, launches = {"elbo": [], "mse": [], "kl": []}, []
    for sw in switches:
        _set_switch(monkeypatch, sw)
        cnt = _Count(monkeypatch)
        mse, kl, elbo = m.train(steps, 2e-4, Xd, Yd, *pri, lt, up, 1e-8, training_mappings=True)
        torch.cuda.synchronize()
        launches.append(cnt.stop())
        out["elbo"] += list(elbo)
        out["mse"].append(mse)
        out["kl"].append(kl)
    params = {"model." + k: v.detach().clone() for k, v in m.named_parameters()}
    params.update({"lt." + k: v.detach().clone() for k, v in lt.named_parameters()})
    params.update({"up." + k: v.detach().clone() for k, v in up.named_parameters()})
    return out, params, launches


def _same(run_a, run_b):
    (out_a, par_a, _), (out_b, par_b, _) = run_a, run_b
    assert out_a["elbo"] == out_b["elbo"] and out_a["mse"] == out_b["mse"] and out_a["kl"] == out_b["kl"]
    assert np.isfinite(out_a["elbo"]).all()
    assert par_a.keys() == par_b.keys() and len(par_a) >= 4 + 4 + 6
    for k in par_a:
        assert torch.equal(par_a[k], par_b[k]), k


def test_training_step_with_the_fused_forward_equals_the_two_launches(monkeypatch):
    """CIFAR preset, 64 INRs, 12 steps (eager warm-up, capture, replay), then a second call on the cached graph"""
    on = _train(monkeypatch, [None, None])
    assert on[2][0] >= 4 and on[2][1] == 0, on[2]        # 3 eager steps + the capture; the second call replays the cached graph
    off = _train(monkeypatch, ["0", "0"])
    assert off[2] == [0, 0]
    _same(on, off)


def test_flipping_the_switch_between_calls_captures_again(monkeypatch):
    """the switch is a field of the step plan, hence of the workspace key: a graph captured under one setting is not replayed
    under the other"""
    on_off = _train(monkeypatch, [None, "0", None])
    assert on_off[2][0] >= 4 and on_off[2][1] == 0 and on_off[2][2] >= 4, on_off[2]
    off_on = _train(monkeypatch, ["0", None, "0"])
    assert off_on[2][0] == 0 and off_on[2][1] >= 4 and off_on[2][2] == 0, off_on[2]
    _same(on_off, off_on)


@pytest.mark.parametrize("precision,stage1_bf16", [(0, True), (1, False)])
def test_fp32_modes_take_no_fused_launch_and_train(monkeypatch, precision, stage1_bf16):
    run = _train(monkeypatch, [None], precision=precision, stage1_bf16=stage1_bf16)
    assert run[2] == [0]
    assert len(run[0]["elbo"]) == 12 and np.isfinite(run[0]["elbo"]).all()


# ---- g. the test-time step ---------------------------------------------------------------------------------------------------------
def _test_time(monkeypatch, switch, steps=12):
    """TestBNNmodel.train on the CIFAR golden's model (bf16 mode, S = 5): warm-up, both captured graphs, a second call.  The
    model reads the switch once, at its first forward, and keeps it for its lifetime (upsample_cifar_hip, frozen cache)"""
    from golden_util import load
    from test_hip_test_model import build, set_post, xdev, ydev
    _set_switch(monkeypatch, switch)
    d = load("test_cifar.npz")
    cfg, n, m = build(d, "cifar")
    m.precision = 1
    set_post(d, cfg, m)
    X, Y = xdev(d, n), ydev(d)
    cnt = _Count(monkeypatch)
    for _ in range(2):
        m.train(X, Y, steps, torch.optim.Adam(m.parameters(), lr=2e-4), False, sample_size=5)
    torch.cuda.synchronize()
    launches = cnt.stop()
    # the model took the setting at its first forward and keeps it (its step graphs were recorded with it): the other
    # setting in the environment changes nothing for this model any more
    _set_switch(monkeypatch, "0" if switch is None else None)
    cnt = _Count(monkeypatch)
    with torch.no_grad():
        y = m.predict(X, random_seed=3, sample_size=5)
    assert cnt.stop() == (1 if switch is None else 0)
    with torch.no_grad():
        loss = float(torch.mean((y - Y[:, None]) ** 2) * n + m.calculate_kl())
    state = {k: v.detach().clone() for k, v in m.named_parameters()}
    state.update({"beta%d" % i: lv.kl_beta.detach().clone() for i, lv in enumerate(m._levels)})
    state["predict"] = y
    return n, loss, state, launches


def test_test_time_step_with_the_fused_forward_equals_the_two_launches(monkeypatch):
    n, loss_on, on, launches_on = _test_time(monkeypatch, None)
    _, loss_off, off, launches_off = _test_time(monkeypatch, "0")
    assert launches_on >= 4 and launches_off == 0, (launches_on, launches_off)     # S x N images through the same function
    assert np.isfinite(loss_on) and loss_on == loss_off
    assert on.keys() == off.keys()
    for k in on:
        assert torch.equal(on[k], off[k]), k
