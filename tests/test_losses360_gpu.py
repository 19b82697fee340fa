"""The mip-NeRF 360 loss terms on the device (-m gpu): `ucn_outer_loss`, `ucn_opacity_loss` and the rawnerf weights of
`ucn_data_loss_ex` behind train_utils.interlevel_loss / opacity_loss / compute_data_loss, against tests/golden/losses360.npz.

Bars (tests/losses360_ref.py): every value and gradient may sit 2 |float32 reference - float64| + 2 ulp from the float64
evaluation, both sides taken from the fixture; nothing here is derived from what the kernels return.  Run with -s for one
LOSSES360 line per quantity (profiles/losses360/parity.txt holds one run's)."""
import math
import types

import numpy as np
import pytest
import torch

import helpers as H
import losses360_ref as R
from oracle import raymarch as rm

pytestmark = pytest.mark.gpu


def _outer_on_device(fx, k):
    from ucnerf_amd.internal import train_utils as tu
    dev = lambda t: t.cuda()
    wp = dev(fx[k + "wp"]).requires_grad_(True)
    loss = tu._OuterLevel.apply(dev(fx[k + "c"]), dev(fx[k + "w"]), dev(fx[k + "cp"]), wp)
    loss.backward()
    return loss.detach(), wp.grad


@pytest.mark.parametrize("case", R.OUTER_CASES)
def test_outer_loss_kernel_value_and_gradient(case):
    fx, k = R.fixture(), f"outer.{case}."
    loss, grad = _outer_on_device(fx, k)
    R.check(f"ucn_outer_loss, {case}", loss, fx, k + "loss")
    R.check(f"ucn_outer_loss, {case}", grad, fx, k + "grad")
    if case == "special":
        assert float(grad[2].abs().max()) == 0.0                  # w <= w_outer on the whole ray: exactly nothing
        assert float(grad[3].min()) * 5 * 32 < -1.9               # wp = 0: slope -2 per covering interval
    loss2, grad2 = _outer_on_device(fx, k)                        # no atomics, fixed order: the same bits
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_interlevel_loss_over_a_ray_history_takes_the_kernel(monkeypatch):
    from ucnerf_amd.internal import train_utils as tu
    fx = R.fixture()
    lead = lambda t: t[:, None, None, :].cuda()
    wps = [lead(fx[f"hist.weights.{i}"]).requires_grad_(True) for i in range(2)]
    hist = [dict(sdist=lead(fx[f"hist.sdist.{i}"]), weights=wps[i]) for i in range(2)]
    hist.append(dict(sdist=lead(fx["hist.sdist.2"]), weights=lead(fx["hist.weights.2"]).requires_grad_(True)))
    monkeypatch.setattr(tu, "_outer_level_torch", lambda *a: pytest.fail("the torch form ran on in-range device tensors"))
    loss = tu.interlevel_loss(hist, types.SimpleNamespace(interlevel_loss_mult=float(fx["hist.mult"])))
    loss.backward()
    R.check("interlevel_loss, history", loss, fx, "hist.loss")
    for i in range(2):
        R.check("interlevel_loss, history", wps[i].grad.reshape(fx[f"hist.grad.{i}"].shape), fx, f"hist.grad.{i}")
    assert hist[-1]['weights'].grad is None


def _random_levels(seed, N, S1, Sp, w_floor=0.0):
    g = torch.Generator().manual_seed(seed)
    post = lambda S: torch.cat([torch.zeros(N, 1), torch.sort(torch.rand(N, S - 1, generator=g), dim=-1).values, torch.ones(N, 1)], dim=-1)
    norm = lambda w, s: s * w / w.sum(-1, keepdim=True)
    return post(S1).cuda(), norm(w_floor + torch.rand(N, S1, generator=g), 0.9).cuda(), post(Sp).cuda(), norm(torch.rand(N, Sp, generator=g) ** 2, 0.95).cuda()


def test_outer_loss_is_deterministic_on_many_workgroups():
    from ucnerf_amd.internal import train_utils as tu
    c, w, cp, wp = _random_levels(7, 301, 32, 128)
    runs = []
    for _ in range(2):
        q = wp.clone().requires_grad_(True)
        loss = tu._OuterLevel.apply(c, w, cp, q)
        loss.backward()
        runs.append((loss.detach(), q.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_outer_level_backward_is_autograd_through_the_torch_form():
    """The node's backward (a scale of the gradient the forward saved) against autograd through `_outer_level_torch` on the same
    device tensors, under a non-trivial upstream gradient.  The two differ by float32's prefix sum of wp on the device: every
    partial sum is <= 1 and a tree scan of S_prop values adds at most log2(S_prop) + 1 times, the envelope's subtraction rounds once
    more: delta = (log2(S_prop) + 2) 2^-24 on w_outer, which moves an interval's -2 max(w - w_outer, 0) / (w + eps) by at most
    2 delta / w_min; a proposal interval collects at most S_nerf of them.  w >= w_min by construction (no division by ~eps)."""
    from ucnerf_amd.internal import train_utils as tu
    N, S1, Sp, up = 67, 32, 128, 3.7
    c, w, cp, wp = _random_levels(11, N, S1, Sp, w_floor=0.5)
    w_min = float(w.min())
    assert w_min > 0.25 * 0.9 / S1
    a, b = wp.clone().requires_grad_(True), wp.clone().requires_grad_(True)
    (up * tu._OuterLevel.apply(c, w, cp, a)).backward()
    (up * tu._outer_level_torch(c, w, cp, b)).backward()
    delta = (math.log2(Sp) + 2) * 2.0 ** -24
    tol = S1 * 2 * delta / w_min * up / (N * S1) + 2 * float(np.spacing(np.float32(float(b.grad.abs().max()))))
    e = float((a.grad - b.grad).abs().max())
    print(f"LOSSES360 {'_OuterLevel.backward vs autograd':44s} {'grad':28s} bar {tol:.3e}  observed {e:.3e}  "
          f"(largest gradient {float(b.grad.abs().max()):.3e})")
    assert float(b.grad.abs().max()) > 100 * tol and e <= tol


@pytest.mark.parametrize("S1,Sp,cp_grad", [(513, 64, False), (32, 1025, False), (32, 64, True)])
def test_interlevel_loss_outside_the_kernel_limits_takes_the_torch_form(monkeypatch, S1, Sp, cp_grad):
    from ucnerf_amd.internal import train_utils as tu
    c, w, cp, wp = _random_levels(S1 + Sp, 9, S1, Sp)
    monkeypatch.setattr(tu._OuterLevel, "apply", lambda *a: pytest.fail("the kernel was handed a shape or graph it does not take"))
    q = wp.clone().requires_grad_(True)
    cpq = cp.clone().requires_grad_(cp_grad)
    got = tu.interlevel_loss([dict(sdist=cpq, weights=q), dict(sdist=c, weights=w)], types.SimpleNamespace(interlevel_loss_mult=0.5))
    want = 0.5 * R.outer_masks(c, w, cp, wp).mean()               # the comparison-table form, on the device
    got.backward()
    assert torch.equal(got.detach(), want) and bool(torch.isfinite(q.grad).all()) and float(q.grad.abs().max()) > 0


def test_interlevel_loss_gate_on_dtype_and_shape(monkeypatch):
    """float64 device tensors must not reach a kernel that reads floats: the torch form, in float64.  Half weights do take the kernel,
    upcast by the node (exactly), and get a half gradient back."""
    from ucnerf_amd.internal import train_utils as tu
    c, w, cp, wp = _random_levels(21, 9, 32, 64)
    cfg = types.SimpleNamespace(interlevel_loss_mult=1.0)
    h = wp.half().requires_grad_(True)
    got = tu.interlevel_loss([dict(sdist=cp, weights=h), dict(sdist=c, weights=w)], cfg)
    got.backward()
    f = wp.half().float().requires_grad_(True)
    want = tu._OuterLevel.apply(c, w, cp, f)
    want.backward()
    assert torch.equal(got.detach(), want.detach()) and h.grad.dtype == torch.float16 and torch.equal(h.grad, f.grad.half())
    monkeypatch.setattr(tu._OuterLevel, "apply", lambda *a: pytest.fail("the kernel was handed float64 tensors"))
    d = [t.double() for t in (c, w, cp, wp)]
    got = tu.interlevel_loss([dict(sdist=d[2], weights=d[3]), dict(sdist=d[0], weights=d[1])], cfg)
    assert got.dtype == torch.float64 and torch.equal(got, R.outer_masks(*d).mean())
    # fenceposts that are not one longer than the weights never reach the kernel either (the patched apply would fail the test)
    tu.interlevel_loss([dict(sdist=cp[:, :-1], weights=wp), dict(sdist=c, weights=w)], cfg)


def test_outer_loss_refuses_sizes_outside_its_limits():
    from ucnerf_amd import _lib
    lib = _lib.load()
    z = torch.zeros(4096, device="cuda")
    assert lib.ucn_outer_loss(z.data_ptr(), z.data_ptr(), 513, z.data_ptr(), z.data_ptr(), 8, 1, z.data_ptr(), z.data_ptr(), _lib.stream()) != 0
    assert lib.ucn_outer_loss(z.data_ptr(), z.data_ptr(), 8, z.data_ptr(), z.data_ptr(), 1025, 1, z.data_ptr(), z.data_ptr(), _lib.stream()) != 0
    assert b"outer_loss" in lib.ucn_last_error()


def test_outer_loss_at_the_largest_sizes():
    """S_nerf = 512, S_prop = 1024: eight intervals per lane, sixteen proposal intervals per lane, 57 440 bytes of LDS"""
    from ucnerf_amd.internal import train_utils as tu
    c, w, cp, wp = _random_levels(3, 6, 512, 1024, w_floor=0.5)
    q = wp.clone().requires_grad_(True)
    got = tu._OuterLevel.apply(c, w, cp, q)
    got.backward()
    d = [t.cpu().double() for t in (c, w, cp, wp)]
    d[3].requires_grad_(True)
    want64 = R.outer_masks(*d, eps=R.EPS32).mean()
    want64.backward()
    f = [t.cpu() for t in (c, w, cp, wp)]
    f[3].requires_grad_(True)
    want32 = R.outer_masks(*f).mean()
    want32.backward()
    R.check_pair("ucn_outer_loss, 512 / 1024", "loss", got, want32.detach(), want64.detach())
    R.check_pair("ucn_outer_loss, 512 / 1024", "grad", q.grad, f[3].grad, d[3].grad)


@pytest.mark.parametrize("case", R.LEVEL_CASES)
def test_opacity_loss_kernel_value_and_gradient(case):
    from ucnerf_amd.internal import train_utils as tu
    fx, k = R.fixture(), f"opacity.{case}."
    cfg = types.SimpleNamespace(opacity_loss_mult=float(fx[k + "mult"]))
    runs = []
    for _ in range(2):
        accs = [a.cuda().requires_grad_(True) for a in R.levels_of(fx, k, "acc")]
        loss = tu.opacity_loss([dict(acc=a) for a in accs], cfg)
        assert "_OpacityLoss" in type(loss.grad_fn).__name__
        loss.backward()
        runs.append([loss.detach()] + [a.grad for a in accs])
    R.check(f"ucn_opacity_loss, {case}", runs[0][0], fx, k + "loss")
    for l in range(len(runs[0]) - 1):
        R.check(f"ucn_opacity_loss, {case}", runs[0][1 + l], fx, k + f"grad.{l}")
    assert all(torch.equal(x, y) for x, y in zip(*runs))


@pytest.mark.parametrize("case", R.LEVEL_CASES)
def test_rawnerf_data_loss_kernel_value_and_gradient(case):
    from ucnerf_amd.internal import train_utils as tu
    fx, k = R.fixture(), f"rawnerf.{case}."
    batch = dict(rgb=fx[k + "target"].cuda(), lossmult=fx[k + "lossmult"].cuda())
    runs = []
    for _ in range(2):
        rgbs = [r.cuda().requires_grad_(True) for r in R.levels_of(fx, k, "rgb")]
        loss, stats = tu.compute_data_loss(batch, [dict(rgb=r) for r in rgbs], R.rawnerf_config(fx[k + "coarse_mult"]))
        assert "_DataLoss" in type(loss.grad_fn).__name__ and stats.pending('mses')
        loss.backward()
        runs.append([loss.detach()] + [r.grad for r in rgbs])
    R.check(f"ucn_data_loss_ex rawnerf, {case}", runs[0][0], fx, k + "loss")
    for l in range(len(runs[0]) - 1):
        R.check(f"ucn_data_loss_ex rawnerf, {case}", runs[0][1 + l], fx, k + f"grad.{l}")
        over = fx[k + f"rgb.{l}"] > 1
        assert float(runs[0][1 + l].cpu()[over].abs().max()) == 0.0
    assert float(runs[0][1][0, 0]) != 0.0                          # rgb == 1: the bound keeps its gradient, like torch's clamp_max
    R.check(f"ucn_data_loss_ex rawnerf, {case}", torch.from_numpy(np.asarray(stats['mses'])), fx, k + "mses")   # the UNCLIPPED residual
    assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_data_loss_entry_points_agree_without_rawnerf_weights():
    """ucn_data_loss is ucn_data_loss_ex with w_raw = NULL: the same bits for the charb / mse weights"""
    import ctypes
    from ucnerf_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(2)
    N = 700
    rgb, tgt, mult = [torch.rand(N, 3, generator=g).cuda() for _ in range(2)], torch.rand(N, 3, generator=g).cuda(), torch.rand(N, generator=g).cuda()
    ptrs = (ctypes.c_void_p * 2)(*[r.data_ptr() for r in rgb])
    wm, wc, wr = (ctypes.c_float * 2)(0.1, 0.0), (ctypes.c_float * 2)(0.0, 1.0), (ctypes.c_float * 2)(0.0, 0.0)
    a, b = torch.empty(6, device="cuda"), torch.empty(6, device="cuda")
    _lib.check(lib.ucn_data_loss(ptrs, 2, wm, wc, tgt.data_ptr(), mult.data_ptr(), N, 0.001, a.data_ptr(), None, None, _lib.stream()))
    _lib.check(lib.ucn_data_loss_ex(ptrs, 2, wm, wc, wr, tgt.data_ptr(), mult.data_ptr(), N, 0.001, b.data_ptr(), None, None, _lib.stream()))
    assert torch.equal(a, b)


@pytest.mark.parametrize("autocast", [False, True])
def test_training_step_with_the_three_terms(autocast, monkeypatch):
    """One step of the tiny model (288 rays) with interlevel, opacity and rawnerf on: finite losses, finite gradients on every
    parameter and non-zero ones where the terms reach (the interlevel term, run backward on its own first, reaches the proposal
    field and nothing of the NeRF field), and each term equal to
    the plain torch forms of tests/losses360_ref.py on detached host copies of the same renderings / ray_history, to the bracket bar."""
    from ucnerf_amd.internal import train_utils as tu
    fx = H.load("train_step.npz")
    spec = rm.make_spec("tiny")
    model, _ = H.hip_model(spec, H.state_for(fx, spec))
    model.train()
    # the fixture's proposal field envelopes its NeRF level everywhere (interlevel loss exactly 0, no gradient): lower its density
    # bias so that it under-estimates the NeRF weights, the situation the term exists for
    model.prop_mlp_0.density_bias = -6.0
    b = {k[4:]: torch.cat([v, v, v]) for k, v in fx.items() if k.startswith("ray_")}
    batch = {k: (v[:, None, None, :] if v.dim() == 2 else v[:, None, None]).cuda() for k, v in b.items()}
    batch['rgb'] = batch['rgb'] * 1.3                                # targets on both sides of the clip
    cfg = types.SimpleNamespace(data_loss_type='rawnerf', data_loss_mult=1.0, data_coarse_loss_mult=0.1, charb_padding=0.001,
                                disable_multiscale_loss=False, interlevel_loss_mult=1.0, opacity_loss_mult=0.01)
    torch.manual_seed(0)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        rend, hist = model(True, batch, 0.5, False, zero_glo=False)
    # the model's own ray_history has to take ucn_outer_loss (fenceposts without a gradient, float weights), not the torch form
    monkeypatch.setattr(tu, "_outer_level_torch", lambda *a: pytest.fail("the training graph's ray_history took the torch form"))
    losses = dict(interlevel=tu.interlevel_loss(hist, cfg), opacity=tu.opacity_loss(rend, cfg))
    losses['data'], stats = tu.compute_data_loss(batch, rend, cfg)
    assert {type(v.grad_fn).__name__ for v in losses.values()} >= {"_OpacityLossBackward", "_DataLossBackward"}, losses
    for k, v in losses.items():
        assert bool(torch.isfinite(v)), (k, v)
    assert float(losses['interlevel'].detach()) > 0
    # the interlevel term alone: the proposal field's gradient is there and finite, the NeRF level is behind a stop-gradient
    losses['interlevel'].backward(retain_graph=True)
    prop = {n: p.grad.clone() for n, p in model.named_parameters() if n.startswith("prop_mlp_0") and p.grad is not None}
    assert prop and all(bool(torch.isfinite(g).all()) for g in prop.values()) and any(float(g.abs().max()) > 0 for g in prop.values())
    assert all(p.grad is None or float(p.grad.abs().max()) == 0 for n, p in model.named_parameters() if n.startswith("nerf_mlp"))
    (losses['opacity'] + losses['data']).backward()
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), n
    for n in ("nerf_mlp.encoder.embeddings", "prop_mlp_0.encoder.embeddings"):
        assert float(dict(model.named_parameters())[n].grad.abs().max()) > 0, n
    # the terms against the plain torch forms on the host: float32 and float64 of the same detached tensors
    host = lambda t, dt: t.detach().to("cpu", dt)
    for tag, got, form in (
            ("interlevel", losses['interlevel'], lambda dt, eps: R.interlevel_masks(
                [dict(sdist=host(h['sdist'], dt), weights=host(h['weights'], dt)) for h in hist], cfg.interlevel_loss_mult, eps)),
            ("opacity", losses['opacity'], lambda dt, eps: R.opacity_torch([host(r['acc'], dt) for r in rend], cfg.opacity_loss_mult)),
            ("rawnerf", losses['data'], lambda dt, eps: R.rawnerf_torch([host(r['rgb'], dt) for r in rend], host(batch['rgb'], dt),
                                                                        host(batch['lossmult'], dt), cfg.data_coarse_loss_mult))):
        R.check_pair(f"training step, autocast={autocast}", tag, got, form(torch.float32, None), form(torch.float64, R.EPS32))
