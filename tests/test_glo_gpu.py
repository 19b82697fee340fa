"""GLO appearance codes on the GPU: the modulation kernels (ucn_ray_film / _backward), the inference forward and one training step
against the reference (tests/golden/model_glo.npz, train_step_glo.npz from make_glo_golden.py), the neutral code against the
non-GLO routes, the per-sample API, and the route render_image takes."""
import contextlib

import pytest
import torch

import helpers as H
from oracle import raymarch as rm
from test_glo_cpu import fixture, glo_model
from test_train_step import check_grad, losses_of, train_batch

pytestmark = pytest.mark.gpu


def glo_hip_model(fx, spec=None, glo=True):
    spec = spec or rm.make_spec("tiny")
    sd = H.state_for(fx, spec)
    if glo:
        model = glo_model(spec)
        sd.update({k[4:]: v.float() for k, v in fx.items() if k.startswith("glo_")})
    else:
        model, _ = H.hip_model(spec, sd, device="cpu")
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".idx") for k in missing), (missing, unexpected)
    return model.cuda().eval()


@contextlib.contextmanager
def f32_engine(name):
    from ucnerf_amd.internal import dense_f32
    prev = dense_f32.set_engine(name)
    try:
        yield
    finally:
        dense_f32.set_engine(prev)


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S", [32, 37, 128])
def test_ray_film_kernels_against_float64(dtype, S):
    from ucnerf_amd import _lib
    lib = _lib.load()
    code = {torch.float32: 0, torch.bfloat16: 2}[dtype]
    N, W = 300, 256                                       # N * S rows, not a multiple of 256 rays
    g = torch.Generator(device="cuda").manual_seed(S)
    x = torch.randn(N * S, W, device="cuda", generator=g).to(dtype)
    a = torch.exp(0.3 * torch.randn(N, W, device="cuda", generator=g))
    b = 0.5 * torch.randn(N, W, device="cuda", generator=g)
    gy = torch.randn(N * S, W, device="cuda", generator=g).to(dtype)
    out = torch.empty_like(x)
    _lib.check(lib.ucn_ray_film(x.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), N, S, W, code, _lib.stream()))
    outs = []
    for _ in range(2):
        gx, ga, gb = torch.empty_like(x), torch.empty(N, W, device="cuda"), torch.empty(N, W, device="cuda")
        _lib.check(lib.ucn_ray_film_backward(gy.data_ptr(), x.data_ptr(), a.data_ptr(), gx.data_ptr(), ga.data_ptr(), gb.data_ptr(),
                                             N, S, W, code, _lib.stream()))
        outs.append((gx, ga, gb))
    torch.cuda.synchronize()
    x64, gy64 = x.double().reshape(N, S, W), gy.double().reshape(N, S, W)
    a64, b64 = a.double()[:, None, :], b.double()[:, None, :]
    want = (x64 * a64 + b64).reshape(N * S, W)
    # fp32 mul and add (each rounded: 2^-24 of |x a| + |b|), then the result rounded to the output type (bf16: 2^-9 of it)
    bound = 2.0 ** -22 * (x64 * a64).abs().reshape(N * S, W) + 2.0 ** -22 * b64.abs().expand(N, S, W).reshape(N * S, W)
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * want.abs()
    assert bool(((out.double() - want).abs() <= bound).all())
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -22          # gx: one rounding of the product
    gx, ga, gb = outs[0]
    want_gx = (gy64 * a64).reshape(N * S, W)
    assert float(((gx.double() - want_gx).abs() / want_gx.abs().clamp_min(1e-3)).max()) <= ulp
    want_ga, want_gb = (gy64 * x64).sum(1), gy64.sum(1)               # fp32 sums of S exact-operand terms
    scale_a, scale_b = (gy64 * x64).abs().sum(1), gy64.abs().sum(1)
    assert float(((ga.double() - want_ga).abs() / scale_a).max()) <= 1e-6
    assert float(((gb.double() - want_gb).abs() / scale_b).max()) <= 1e-6
    for t, u in zip(outs[0], outs[1]):                                 # fixed summation order: bit-identical reruns
        assert torch.equal(t, u)


def test_ray_film_rejects_a_width_off_the_vector_grid():
    from ucnerf_amd import _lib
    lib = _lib.load()
    x = torch.zeros(4, 12, device="cuda")
    a = torch.zeros(2, 12, device="cuda")
    assert lib.ucn_ray_film(x.data_ptr(), a.data_ptr(), a.data_ptr(), x.data_ptr(), 2, 2, 12, 0, _lib.stream()) != 0


# ---------------------------------------------------------------------------------------------------- inference forward
def glo_batch(fx, tag, n):
    batch = H.to_dev(H.batch_of(fx))
    batch["rand_vec"] = torch.cat([fx[f"{tag}noise{l}_rand_vec"].reshape(n, -1) for l in range(2)], -1).cuda()
    return batch


@pytest.mark.parametrize("zero_glo", [True, False])
def test_glo_forward_vs_golden(zero_glo):
    """Model.forward in eval mode against the reference, with the bars of test_model_forward_vs_golden for `tiny`.
    zero_glo=True: the fused march on the folded colour layers; False: the training graph's forward without gradients."""
    fx = fixture("model_glo.npz")
    tag = "Z1_" if zero_glo else "Z0_"
    model = glo_hip_model(fx)
    n = fx["ray_origins"].shape[0]
    with torch.no_grad():
        rend, hist = model(False, glo_batch(fx, tag, n), 1.0, True, zero_glo=zero_glo)
    torch.cuda.synchronize()
    assert model.last_march_route == ("fused" if zero_glo else "train_graph")
    for lvl in range(2):
        g = lambda k: fx[f"{tag}L{lvl}_{k}"]
        last = lvl == 1
        samp = 1e-2 if last else 2e-6
        assert H.maxdiff(hist[lvl]["sdist"].cpu(), g("hist_sdist")) <= (5e-5 if last else 0.0), lvl
        assert H.maxdiff(hist[lvl]["density"].cpu().reshape(-1), g("hist_density").reshape(-1)) <= samp, lvl
        assert H.maxdiff(rend[lvl]["weights"].cpu().reshape(-1), g("weights").reshape(-1)) <= (2e-4 if last else 5e-7), lvl
        assert H.maxdiff(rend[lvl]["rgb"].cpu().reshape(-1), g("rgb").reshape(-1)) <= H.RGB_TOL, lvl
        assert float((rend[lvl]["rgb"].cpu().reshape(-1) - g("rgb").reshape(-1)).abs().mean()) <= 2e-5, lvl
        assert H.maxdiff(rend[lvl]["acc"].cpu().reshape(-1), g("acc").reshape(-1)) <= 1e-4, lvl
        if last:
            assert H.maxdiff(hist[lvl]["rgb"].cpu().reshape(-1), g("hist_rgb").reshape(-1)) <= samp


@pytest.mark.parametrize("zero_glo", [True, False])
def test_glo_forward_vs_golden_under_autocast(zero_glo):
    """The same under bf16 autocast (the reference's render_image context).  zero_glo=True takes the mixed-precision fused march
    (march_infer.mixed_level, folded weights); bars: bf16 through three 256-wide layers, those of
    test_render_under_autocast_runs_the_mixed_precision_path."""
    fx = fixture("model_glo.npz")
    tag = "Z1_" if zero_glo else "Z0_"
    model = glo_hip_model(fx)
    n = fx["ray_origins"].shape[0]
    model._mixed_levels = 0
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        rend, _ = model(False, glo_batch(fx, tag, n), 1.0, True, zero_glo=zero_glo)
    torch.cuda.synchronize()
    if zero_glo:
        assert model.last_march_route == "fused" and model._mixed_levels == 2
    else:
        assert model.last_march_route == "train_graph"
    got, want = rend[1]["rgb"].float().cpu().reshape(-1), fx[f"{tag}L1_rgb"].reshape(-1)
    assert torch.isfinite(got).all()
    d = (got - want).abs()
    assert float(d.max()) <= 3e-2 and float(d.mean()) <= 3e-3, (float(d.max()), float(d.mean()))
    assert H.maxdiff(rend[1]["acc"].float().cpu(), fx[f"{tag}L1_acc"]) <= 3e-2


# ---------------------------------------------------------------------------------------------------- training step
@pytest.mark.parametrize("mode", ["split", "exact", "bf16"])
def test_glo_train_step_matches_reference(mode):
    """One training step with per-image codes against the reference's (train_step_glo.npz): losses and every gradient, GLO
    parameters included.  fp32 on both GEMM engines with the bars of test_hip_train_graph_matches_reference_step; under bf16
    autocast with the bf16-vs-fp32 bars of test_config2_bf16_training_step_end_to_end (the fixture is the fp32 reference)."""
    from ucnerf_amd.internal import train_utils as tu
    fx = fixture("train_step_glo.npz")
    spec = rm.make_spec("tiny")
    model = glo_hip_model(fx)
    model.train()
    batch = H.pin_noise(train_batch(fx, "cuda"), H.noise_of(fx, 2))
    batch["rand_vec"] = batch["rand_vec"][:, None, None, :]
    bf16 = mode == "bf16"
    with f32_engine("split" if bf16 else mode), torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        rend, hist = model(True, batch, float(fx["train_frac"]), False, zero_glo=False)
        assert model.last_march_route == "train_graph" and rend[-1]["rgb"].requires_grad
        losses, _ = losses_of(tu, batch, rend, hist, spec)
        total = sum(losses.values())
    total.backward()
    torch.cuda.synchronize()
    lrel = 3e-2 if bf16 else 2e-4
    for k, v in losses.items():
        assert abs(float(v) - float(fx["loss_" + k])) <= lrel * max(1.0, abs(float(fx["loss_" + k]))), (k, float(v), float(fx["loss_" + k]))
    names = [p for p, _ in model.named_parameters() if f"grad_{p}.abs" in fx]
    assert {"glo_vecs.weight", "nerf_mlp.lin_glo_0.weight", "nerf_mlp.lin_glo_1.bias"} <= set(names)
    for pname, p in model.named_parameters():
        if f"grad_{pname}.abs" not in fx:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), pname
        if bf16:
            want = float(fx[f"grad_{pname}.abs"])
            assert abs(float(p.grad.double().abs().sum()) - want) <= 0.1 * want, pname
        elif pname == "nerf_mlp.encoder.embeddings":
            assert abs(float(p.grad.double().abs().sum()) - float(fx[f"grad_{pname}.abs"])) <= 2e-2 * float(fx[f"grad_{pname}.abs"])
        else:
            check_grad(fx, pname, p.grad, 2e-2)


# ---------------------------------------------------------------------------------------------------- neutral code
@pytest.mark.parametrize("mode", ["exact", "bf16"])
def test_neutral_glo_equals_the_non_glo_route(mode, monkeypatch):
    """lin_glo_last = 0 (a = 1, b = 0): the GLO routes compute what the non-GLO model does on the same weights, bit for bit --
    the fused inference march (fold = identity) and the training step against the uncomposed non-GLO node (_ColourMLP)."""
    monkeypatch.setenv("UCN_F32_COMPOSED", "0")
    monkeypatch.setenv("UCN_FUSED_HEADS", "0")
    fx = fixture("train_step_glo.npz")
    glo, plain = glo_hip_model(fx), glo_hip_model(fx, glo=False)
    with torch.no_grad():
        glo.nerf_mlp.lin_glo_1.weight.zero_()
        glo.nerf_mlp.lin_glo_1.bias.zero_()
    batch = H.pin_noise(train_batch(fx, "cuda"), H.noise_of(fx, 2))
    batch["rand_vec"] = batch["rand_vec"][:, None, None, :]
    bf16 = mode == "bf16"
    with torch.no_grad():
        r_g, _ = glo(False, {k: v for k, v in batch.items() if k != "march_noise"}, 1.0, False)
        r_p, _ = plain(False, {k: v for k, v in batch.items() if k != "march_noise"}, 1.0, False)
    assert glo.last_march_route == "fused"
    assert torch.equal(r_g[-1]["rgb"], r_p[-1]["rgb"])

    def step(model):
        model.train()
        model.zero_grad(set_to_none=True)
        with f32_engine("split" if bf16 else mode):
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
                rend, hist = model(True, batch, 0.4, False, zero_glo=False)
                loss = (rend[-1]["rgb"].float() - batch["rgb"]).square().mean() + sum(h["weights"].float().sum() for h in hist) * 1e-3
            loss.backward()
        return rend[-1]["rgb"].detach(), {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    rgb_g, g_g = step(glo)
    rgb_p, g_p = step(plain)
    torch.cuda.synchronize()
    assert torch.equal(rgb_g, rgb_p)
    for n, gp in g_p.items():
        if n.endswith("encoder.embeddings"):
            # table gradients: rows summed through LDS float adds whose order varies from run to run -- equal to fp32 summation noise
            assert float((g_g[n] - gp).abs().max()) <= 1e-5 * float(gp.abs().max()), n
        else:
            assert torch.equal(g_g[n], gp), n
    assert float(g_g["nerf_mlp.lin_glo_1.weight"].abs().sum()) > 0       # the codes still learn from a neutral start


# ---------------------------------------------------------------------------------------------------- per-sample API, route
def test_nerf_mlp_forward_with_glo_vec_matches_the_reference_formula():
    """NerfMLP.forward(glo_vec=...) (models.py:600-674) against the reference's colour MLP evaluated in float64 on the
    bottleneck predict_density returns; predict_density itself does not see the code."""
    from ucnerf_amd.internal import train_graph as tg
    fx = fixture("model_glo.npz")
    m = glo_hip_model(fx).nerf_mlp
    g = torch.Generator().manual_seed(5)
    R, S = 40, 16
    means = (torch.rand(R, S, 6, 3, generator=g) * 2 - 1).cuda()
    stds = (torch.rand(R, S, 6, generator=g) * 0.01 + 0.001).cuda()
    vd = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).cuda()
    code = torch.randn(R, 4, generator=g).cuda()
    out = m(False, means, stds, viewdirs=vd, glo_vec=code)
    raw, x, _ = m.predict_density(means, stds)
    plain = m(False, means, stds, viewdirs=vd)
    torch.cuda.synchronize()
    d = lambda t: t.detach().double().cpu()
    P = {k: d(v) for k, v in m.named_parameters() if "encoder" not in k}
    h = torch.relu(d(code) @ P["lin_glo_0.weight"].t() + P["lin_glo_0.bias"]) @ P["lin_glo_1.weight"].t() + P["lin_glo_1.bias"]
    scale, shift = h.chunk(2, -1)
    bott = d(x) * torch.exp(scale)[:, None, :] + shift[:, None, :]
    enc = d(tg.view_encoding(vd, m.deg_view))[:, None, :].expand(R, S, -1)
    h1 = torch.relu(torch.cat([bott, enc], -1) @ P["lin_second_stage_0.weight"].t() + P["lin_second_stage_0.bias"])
    h2 = torch.relu(torch.cat([h1, bott, enc], -1) @ P["lin_second_stage_1.weight"].t() + P["lin_second_stage_1.bias"])
    rgb = torch.sigmoid(h2 @ P["rgb_layer.weight"].t() + P["rgb_layer.bias"]) * (1 + 2 * m.rgb_padding) - m.rgb_padding
    assert H.maxdiff(out["rgb"].cpu(), rgb) <= 1e-5
    assert H.maxdiff(out["density"].cpu(), torch.nn.functional.softplus(d(raw) + m.density_bias)) <= 1e-6
    assert float((out["rgb"] - plain["rgb"]).abs().max()) > 1e-3           # the code does act
    assert torch.equal(m.predict_density(means, stds)[1], x)


def test_render_image_on_a_glo_model_runs_the_fused_march(monkeypatch):
    from ucnerf_amd.internal import models, train_graph
    fx = fixture("model_glo.npz")
    model = glo_hip_model(fx)
    model.train()

    def refuse(*a, **k):
        raise AssertionError("render_image took the training graph")
    monkeypatch.setattr(train_graph, "march_train", refuse)
    rays = H.to_dev(rm.synthetic_rays(12 * 16, seed=7))
    batch = {k: v.reshape(12, 16, -1) for k, v in rays.items()}
    cfg = types_ns(render_ray_tile=8, vis_num_rays=16)
    out = models.render_image(model, None, batch, False, 1.0, cfg, verbose=False)
    torch.cuda.synchronize()
    assert model.last_march_route == "fused" and model.training
    assert out["rgb"].shape == (12, 16, 3) and torch.isfinite(out["rgb"]).all()


def types_ns(**kw):
    import types
    return types.SimpleNamespace(**kw)
