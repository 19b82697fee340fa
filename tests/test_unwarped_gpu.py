"""MLP.warp_fn = None on the GPU: the cast probe, the eval forward on both sample orders and both dense arithmetics, the points
API at the cube's faces, a training step in fp32 and under bf16 autocast, exact zeros for what lies outside the cube, and the refusal of
another warp (old against new entry points: tests/test_unwarped_routes_gpu.py).  Reference: tests/golden/unwarped.npz (the
reference's own run, make_unwarped_golden.py); bars: those of the warped tests named at each assert."""
import ctypes

import pytest
import torch

import helpers as H
import unwarped_ref as U
from oracle import raymarch as rm
from test_glo_gpu import f32_engine
from test_train_step import check_grad, losses_of, train_batch
from test_unwarped_cpu import sub

pytestmark = pytest.mark.gpu


def fixture(prefix):
    return sub(H.load("unwarped.npz"), prefix)


def unwarped_model(fx, **kw):
    from ucnerf_amd.internal import models
    spec = rm.make_spec("tiny")
    mlp = {k: kw.pop(k) for k in list(kw) if k in ("mlp_mode", "disable_density_normals")}
    with models.bindings(NerfMLP=dict(warp_fn=None, **mlp), PropMLP=dict(warp_fn=None)):
        model, cfg = H.hip_model(spec, H.state_for(fx, spec), **kw)
    assert model.nerf_mlp.warp == 0 and model.prop_mlp_0.warp == 0
    return model, cfg, spec


def ray_args(fx, tdist, rand_vec, idx=None):
    """(device tensors kept alive, pointer list fenceposts, NULL, NULL, origins, directions, basis, radii, NULL, NULL)"""
    from ucnerf_amd import _lib
    lib = _lib.load()
    f = lambda t: (t if idx is None else t[idx]).cuda().float().contiguous()
    o, d, cam, rad = f(fx["ray_origins"]), f(fx["ray_directions"]), f(fx["ray_cam_dirs"]), f(fx["ray_radii"]).reshape(-1)
    td, rv = tdist.cuda().float().contiguous(), rand_vec.cuda().float().contiguous()
    N = td.shape[0]
    basis = torch.empty(N, 6, device="cuda")
    _lib.check(lib.ucn_cone_basis(cam.data_ptr(), rv.data_ptr(), N, basis.data_ptr(), _lib.stream()))
    keep = (o, d, cam, rad, td, rv, basis)
    return keep, [td.data_ptr(), None, None, o.data_ptr(), d.data_ptr(), basis.data_ptr(), rad.data_ptr(), None, None]


def as_sdist(args, N):
    """ray_args' pointer list read as NORMALISED fenceposts with near = 0 and far = 1 -- the kernels' TD = false instantiations, which
    derive t = s * far + (1 - s) * near = s * 1 + (1 - s) * 0 = s exactly in float32: the same Gaussians as the metric ones, bit for bit."""
    near, far = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
    return (near, far), [args[0], near.data_ptr(), far.data_ptr()] + args[3:]


# ---------------------------------------------------------------------------------------------------- 1. cast probe
def test_cast_probe_unwarped_vs_reference():
    """ucn_cast_probe_warp(warp = 0) against the reference's render.cast_rays: the bars of
    test_cone_cast_and_contraction_vs_reference_golden (4e-6 on the means, 2e-6 on t, 4e-7 relative on std); the grid's inputs
    behind them are the SAME numbers (no contraction), and 1 / sqrt(8 std^2) to the fast rsq's 2e-5 relative (the bar the warped
    probe holds its contracted std to)."""
    from ucnerf_amd import _lib
    lib = _lib.load()
    fx = H.load("unwarped.npz")
    keep, args = ray_args(sub(fx, "eval_"), fx["cast_tdist"], fx["cast_rand_vec"], fx["cast_rays"])
    N, S = fx["cast_tdist"].shape[0], fx["cast_tdist"].shape[1] - 1
    out = torch.full((N, S, 6, 10), float("nan"), device="cuda")
    _lib.check(lib.ucn_cast_probe_warp(*args, 0.5, 0, N, S, out.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    got = out.cpu().double()
    means, stds, t = fx["cast_means"].double(), fx["cast_stds"].double(), fx["cast_t"].double()
    ok = torch.isfinite(stds) & (stds > 0)
    assert H.maxdiff(got[..., 0:3][ok], means[ok]) <= 4e-6
    assert H.maxdiff(got[..., 4][ok], t[ok]) <= 2e-6
    assert float(((got[..., 3] - stds).abs() / stds.abs().clamp_min(1e-30))[ok].max()) <= 4e-7
    assert torch.equal(got[..., 5:8][ok], got[..., 0:3][ok]) and torch.equal(got[..., 8][ok], got[..., 3][ok])
    _, rs = U.grid_inputs(means, stds)
    assert float(((got[..., 9] - rs).abs() / rs)[ok].max()) <= 2e-5
    # k_cast_probe<TD = false, WARP = false>: the same fenceposts as normalised ones of near = 0, far = 1
    keep2, args_sd = as_sdist(args, N)
    out_sd = torch.full((N, S, 6, 10), float("nan"), device="cuda")
    _lib.check(lib.ucn_cast_probe_warp(*args_sd, 0.5, 0, N, S, out_sd.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    assert torch.equal(out_sd.cpu().view(torch.int32), out.cpu().view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 2. eval forward
@pytest.mark.parametrize("mlp_mode", [0, 1])
@pytest.mark.parametrize("rays_fastest", [True, False])
def test_unwarped_forward_vs_reference(rays_fastest, mlp_mode):
    """Model.forward (eval) against the reference's warp_fn = None run, with the bars of test_warped_forward_vs_golden."""
    fx = fixture("eval_")
    model, _, spec = unwarped_model(fx, rays_fastest=rays_fastest, mlp_mode=mlp_mode)
    batch = H.pin_noise(H.to_dev(H.batch_of(fx)), H.noise_of(fx, spec.num_levels))
    with torch.no_grad():
        rend, hist = model(False, batch, float(fx["train_frac"]), True)
    torch.cuda.synchronize()
    assert model.last_march_route == "fused"
    for lvl in range(spec.num_levels):
        g = lambda k: fx[f"L{lvl}_{k}"]
        r = rend[lvl]
        last = lvl == spec.num_levels - 1
        samp = 1e-2 if last else 2e-6
        assert H.maxdiff(hist[lvl]["sdist"].cpu(), g("hist_sdist").reshape(hist[lvl]["sdist"].shape)) <= (5e-5 if last else 0.0), lvl
        d_dens = H.maxdiff(hist[lvl]["density"].cpu().reshape(-1), g("hist_density").reshape(-1))
        d_rgb = H.maxdiff(r["rgb"].cpu().reshape(-1), g("rgb").reshape(-1))
        print(f"UNWARPED level {lvl} rays_fastest {rays_fastest} mlp_mode {mlp_mode}: density {d_dens:.3e} rgb {d_rgb:.3e}")
        assert d_dens <= samp, lvl
        assert H.maxdiff(r["weights"].cpu().reshape(-1), g("weights").reshape(-1)) <= (2e-4 if last else 5e-7), lvl
        assert d_rgb <= H.RGB_TOL, lvl
        assert H.maxdiff(r["acc"].cpu().reshape(-1), g("acc").reshape(-1)) <= 1e-4, lvl
        assert H.maxdiff(hist[lvl]["coord"].cpu().reshape(-1), g("hist_coord").reshape(-1)) <= 5e-6, lvl
        if last:
            assert H.maxdiff(hist[lvl]["rgb"].cpu().reshape(-1), g("hist_rgb").reshape(-1)) <= samp
        stable = (g("acc").reshape(-1) - 0.6).abs() > 1e-3
        assert H.maxdiff(r["depth"].cpu().reshape(-1)[stable], g("depth").reshape(-1)[stable]) <= 1e-3, lvl
        for k in ("distance_mean", "distance_median", "distance_percentile_5", "distance_percentile_95"):
            assert H.maxdiff(r[k].cpu().reshape(-1), g(k).reshape(-1)) <= 2e-3, (lvl, k)
        assert H.maxdiff(r["ray_sdist"].cpu(), g("ray_sdist")) <= 5e-5
        assert H.maxdiff(r["ray_rgbs"].cpu(), g("ray_rgbs")) <= (samp if last else 1e-4)


def outside_samples(fx, lvl, sdist):
    """[N, S] bool: all six multisamples at least 1e-4 outside the cube (the kernel's own points differ from these by < 5e-6)."""
    N = fx["ray_near"].shape[0]
    sd = sdist.reshape(N, -1).cpu()
    tdist = sd * fx["ray_far"] + (1 - sd) * fx["ray_near"]
    means, _, _ = rm.cone_multisamples(tdist, fx["ray_origins"], fx["ray_directions"], fx["ray_cam_dirs"], fx["ray_radii"],
                                       fx[f"noise{lvl}_rand_vec"].reshape(N, -1))
    return (means.abs().amax(dim=-1) > 1 + 1e-4).all(dim=-1), tdist


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_outside_samples_have_zero_features_and_no_gradient(layout):
    from ucnerf_amd import _lib
    lib = _lib.load()
    fx = fixture("eval_")
    model, _, spec = unwarped_model(fx)
    mlp = model.nerf_mlp
    out_mask, tdist = outside_samples(fx, 1, fx["L1_hist_sdist"])
    assert int(out_mask.sum()) >= 100 and int((~out_mask).sum()) >= 100
    keep, args = ray_args(fx, tdist, fx["noise1_rand_vec"].reshape(tdist.shape[0], -1))
    N, S = tdist.shape[0], tdist.shape[1] - 1
    L, C = mlp.encoder.num_levels, mlp.encoder.level_dim
    feat = torch.full((L * N * S * C,), float("nan"), device="cuda")
    d = mlp.grid_field()
    _lib.check(lib.ucn_march_features_warp(ctypes.byref(d), *args, 0.5, 0, N, S, 0, layout, feat.data_ptr(), None, None, _lib.stream()))
    torch.cuda.synchronize()
    if layout == 1:
        f = feat.reshape(N, S, L * C)
    elif layout == 0:
        f = feat.reshape(L, N, S, C).permute(1, 2, 0, 3).reshape(N, S, L * C)
    else:
        f = feat.reshape(L, S, N, C).permute(2, 1, 0, 3).reshape(N, S, L * C)
    f = f.cpu()
    assert bool(torch.isfinite(f).all())
    assert torch.equal(f[out_mask], torch.zeros_like(f[out_mask]))
    assert float(f[~out_mask].abs().max()) > 0
    if layout != 1:
        return
    # the table gradient of a feature gradient that lives on the outside samples only: exactly zero, on both backward routes
    g = torch.zeros(N, S, L * C)
    g[out_mask] = 1.0
    g = g.reshape(N * S, L * C).cuda()
    for lpb, with_ws in ((0, True), (0, False), (1, False)):
        grad = torch.zeros_like(mlp.encoder.embeddings)
        ws = torch.empty(lib.ucn_march_features_backward_ws_floats(ctypes.byref(d), N, S), device="cuda") if with_ws else None
        _lib.check(lib.ucn_march_features_backward_warp(ctypes.byref(d), *args, 0.5, 0, N, S, lpb, 1, g.data_ptr(), grad.data_ptr(),
                                                        _lib.ptr(ws), _lib.stream()))
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(grad)) == 0, (lpb, with_ws)


# ---------------------------------------------------------------------------------------------------- 3. the points API
def test_points_at_the_faces_and_no_warp_is_a_no_op():
    fx = fixture("eval_")
    model, _, _ = unwarped_model(fx)
    mlp = model.nerf_mlp
    eps = 2.0 ** -23
    xs = [1.0, -1.0, 1.0 - eps, -1.0 + eps, 1.0 + 2 * eps, -1.0 - 2 * eps]
    means = torch.tensor([[[x, 0.3, -0.2]] for x in xs] + [[[0.1, x, 0.4]] for x in xs], device="cuda")     # [12, 1, 3]
    stds = torch.full((means.shape[0], 1), 1e-3, device="cuda")
    vd = torch.nn.functional.normalize(torch.tensor([[0.2, -0.5, 0.8]], device="cuda")).expand(means.shape[0], 3).contiguous()
    a = mlp(False, means, stds, viewdirs=vd, no_warp=True)
    b = mlp(False, means, stds, viewdirs=vd, no_warp=False)
    for k in ("coord", "density", "rgb"):
        assert torch.equal(a[k], b[k]), k
    pa, pb = mlp.predict_density(means, stds, no_warp=True), mlp.predict_density(means, stds, no_warp=False)
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert torch.equal(a["coord"], means[:, 0, :])                   # the plain mean, no contraction, no halving
    # bounds inclusive: exactly +-1 and just inside carry grid features, just outside none -- there the density is the bias path's
    empty = mlp(False, torch.tensor([[[5.0, 5.0, 5.0]]], device="cuda"), stds[:1], viewdirs=vd[:1], no_warp=True)["density"]
    dens = a["density"].reshape(2, 6)
    assert bool((dens[:, 4:] == empty).all())
    assert bool((dens[:, :4] != empty).all())


# ---------------------------------------------------------------------------------------------------- 4. training step
_TRUTH_STEP = []


def truth_step():
    """float64 autograd of the restatement's training step on the fixture's rays and draws (computed once, never changed): losses
    and, in the format check_grad reads, every parameter's gradient."""
    if not _TRUTH_STEP:
        from test_unwarped_cpu import train_case
        fx, spec, sd, rays, lo = train_case()
        losses, grads = U.train_step(spec, sd, rays, H.noise_of(fx, 2), float(fx["train_frac"]), lo, torch.float64)
        digest = {}
        for k, g in grads.items():
            digest[f"grad_{k}.abs"], digest[f"grad_{k}.full"] = g.abs().sum(), g
        _TRUTH_STEP.append((losses, digest))
    return _TRUTH_STEP[0]


@pytest.mark.parametrize("mode", ["split", "exact", "bf16", "bf16_fp32_tables"])
def test_unwarped_train_step_matches_reference(mode):
    """One training step against float64 autograd of the restatement (tests/unwarped_ref.py train_step, pinned to the reference's
    own step by tests/test_unwarped_cpu.py) -- the loss terms and the gradient of every parameter -- and against the reference's
    float32 step (train_* of the fixture), both with the bars of test_warped_train_step_matches_reference; two calls agree bit for
    bit where the warped route promises it (the fixed-point table gradient of the autocast step with half tables)."""
    from ucnerf_amd.internal import train_utils as tu
    fx = fixture("train_")
    bf16 = mode.startswith("bf16")
    model, _, spec = unwarped_model(fx, autocast_half_tables=mode != "bf16_fp32_tables")
    model.train()
    batch = H.pin_noise(train_batch(fx, "cuda"), H.noise_of(fx, 2))
    batch["rand_vec"] = batch["rand_vec"][:, None, None, :]
    grads = []
    for rep in range(2 if mode == "bf16" else 1):
        model.zero_grad(set_to_none=True)
        with f32_engine("split" if bf16 else mode), torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            rend, hist = model(True, batch, float(fx["train_frac"]), False)
            assert model.last_march_route == "train_graph" and rend[-1]["rgb"].requires_grad
            losses, _ = losses_of(tu, batch, rend, hist, spec)
            total = sum(losses.values())
        total.backward()
        torch.cuda.synchronize()
        grads.append(model.nerf_mlp.encoder.embeddings.grad.clone())
    if len(grads) == 2:
        assert torch.equal(grads[0], grads[1])
    for lvl in range(spec.num_levels if not bf16 else 0):
        assert H.maxdiff(hist[lvl]["sdist"].detach().cpu().reshape(-1), fx[f"L{lvl}_hist_sdist"].reshape(-1)) <= 5e-5, lvl
    lrel = 3e-2 if bf16 else 2e-4
    for k, v in losses.items():
        print(f"UNWARPED train {mode} loss {k}: {float(v.detach()):.8e} reference {float(fx['loss_' + k]):.8e}")
        assert abs(float(v) - float(fx["loss_" + k])) <= lrel * max(1.0, abs(float(fx["loss_" + k]))), (k, float(v), float(fx["loss_" + k]))
    checked = 0
    for pname, p in model.named_parameters():
        if f"grad_{pname}.abs" not in fx:
            continue
        checked += 1
        assert p.grad is not None and torch.isfinite(p.grad).all(), pname
        if bf16:
            want = float(fx[f"grad_{pname}.abs"])
            assert abs(float(p.grad.double().abs().sum()) - want) <= 0.1 * want, pname
        elif pname == "nerf_mlp.encoder.embeddings":
            assert abs(float(p.grad.double().abs().sum()) - float(fx[f"grad_{pname}.abs"])) <= 2e-2 * float(fx[f"grad_{pname}.abs"])
        else:
            check_grad(fx, pname, p.grad, 2e-2)
    assert checked >= 10
    l64, g64 = truth_step()
    for k, v in losses.items():
        assert abs(float(v.detach()) - l64[k]) <= lrel * max(1.0, abs(l64[k])), (k, float(v.detach()), l64[k])
    checked = 0
    for pname, p in model.named_parameters():
        if f"grad_{pname}.abs" not in g64:
            continue
        checked += 1
        want = float(g64[f"grad_{pname}.abs"])
        got = float(p.grad.double().abs().sum())
        print(f"UNWARPED train {mode} gradient {pname}: |sum| HIP / float64 = {got / want:.6f}")
        if bf16:
            assert abs(got - want) <= 0.1 * want, pname
        elif pname == "nerf_mlp.encoder.embeddings":
            assert abs(got - want) <= 2e-2 * want, pname
        else:
            check_grad(g64, pname, p.grad.double(), 2e-2)
    assert checked >= 10


# ---------------------------------------------------------------------------------------------------- 5. other routes
def test_unwarped_normals_and_outside_normals_are_minus_zero():
    """Density normals of an unwarped field: finite everywhere, and on samples wholly outside the cube what the reference gives
    (zero grid part, zero gradient): raw_grad = +0, normals = -0 / eps = -0."""
    fx = fixture("eval_")
    model, _, spec = unwarped_model(fx, disable_density_normals=False)
    batch = H.pin_noise(H.to_dev(H.batch_of(fx)), H.noise_of(fx, spec.num_levels))
    with torch.no_grad():
        rend, hist = model(False, batch, float(fx["train_frac"]), True)
    torch.cuda.synchronize()
    h = hist[-1]
    out_mask, _ = outside_samples(fx, 1, h["sdist"])
    assert int(out_mask.sum()) >= 100
    raw, nrm = h["raw_grad_density"].cpu().reshape(out_mask.shape + (3,)), h["normals"].cpu().reshape(out_mask.shape + (3,))
    assert bool(torch.isfinite(raw).all()) and bool(torch.isfinite(nrm).all())
    assert torch.equal(raw[out_mask], torch.zeros_like(raw[out_mask])) and not bool(torch.signbit(raw[out_mask]).any())
    assert torch.equal(nrm[out_mask], torch.zeros_like(nrm[out_mask])) and bool(torch.signbit(nrm[out_mask]).all())
    inside = ~out_mask
    assert float((nrm[inside].norm(dim=-1) - 1).abs().median()) <= 1e-5           # unit vectors where the grid has a gradient
    dens = h["density"].cpu().reshape(out_mask.shape)
    assert float(dens[out_mask].max() - dens[out_mask].min()) == 0.0              # zero grid features: one density outside the cube
    # the model above marches normalised fenceposts (k_march_density_grad<C, TD = false, WARP = false>); the metric ones (TD = true) on
    # the entry point itself: the march's fenceposts as metric ones against the same as normalised ones of near = 0, far = 1, bit for bit
    from ucnerf_amd import _lib
    lib = _lib.load()
    mlp = model.nerf_mlp
    N, S = out_mask.shape
    sd = h["sdist"].reshape(N, -1).cpu()
    keep, args = ray_args(fx, sd * fx["ray_far"] + (1 - sd) * fx["ray_near"], fx["noise1_rand_vec"].reshape(N, -1))
    keep_sd, args_sd = as_sdist(args, N)
    L, C = mlp.encoder.num_levels, mlp.encoder.level_dim
    gfeat = torch.randn(L, N * S, C, generator=torch.Generator().manual_seed(3)).cuda()
    d = mlp.grid_field()
    got = []
    for a in (args, args_sd):
        rg, nr = torch.full((N * S, 3), float("nan"), device="cuda"), torch.full((N * S, 3), float("nan"), device="cuda")
        _lib.check(lib.ucn_march_density_grad_warp(ctypes.byref(d), *a, 0.5, 0, N, S, 0, gfeat.data_ptr(), rg.data_ptr(), nr.data_ptr(),
                                                   _lib.stream()))
        torch.cuda.synchronize()
        got.append((rg.cpu(), nr.cpu()))
    assert bool(torch.isfinite(got[0][0]).all()) and float(got[0][0].abs().max()) > 0
    assert torch.equal(got[0][0].view(torch.int32), got[1][0].view(torch.int32))
    assert torch.equal(got[0][1].view(torch.int32), got[1][1].view(torch.int32))
    om = out_mask.reshape(-1)
    assert torch.equal(got[0][0][om], torch.zeros_like(got[0][0][om])) and bool(torch.signbit(got[0][1][om]).all())


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_another_warp_is_refused_with_a_message():
    from ucnerf_amd import _lib
    lib = _lib.load()
    fx = fixture("eval_")
    model, _, _ = unwarped_model(fx)
    d = model.nerf_mlp.grid_field()
    for name, call in (
            ("march_features", lambda w: lib.ucn_march_features_warp(ctypes.byref(d), *[None] * 9, 0.5, w, 0, 4, 0, 1, None, None, None, None)),
            ("march_features_backward", lambda w: lib.ucn_march_features_backward_warp(ctypes.byref(d), *[None] * 9, 0.5, w, 0, 4, 0, 1, None, None, None, None)),
            ("march_scale_features", lambda w: lib.ucn_march_scale_features_warp(ctypes.byref(d), *[None] * 9, 0.5, w, 0, 4, None, 1, None, None)),
            ("march_density_grad", lambda w: lib.ucn_march_density_grad_warp(ctypes.byref(d), *[None] * 9, 0.5, w, 0, 4, 0, None, None, None, None)),
            ("cast_probe", lambda w: lib.ucn_cast_probe_warp(*[None] * 9, 0.5, w, 0, 4, None, None))):
        for w in (2, -1):
            assert call(w) != 0, (name, w)
            msg = lib.ucn_last_error().decode()
            assert name in msg and "warp must be 0" in msg, msg
