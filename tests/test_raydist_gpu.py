"""Warped ray distances (Model.raydist_fn) on the GPU: ucn_s_to_t against float64, the geometry / compositing siblings that
read metric fenceposts, the eval forward and a training step against the reference (tests/golden/raydist_*.npz,
train_step_raydist.npz from make_raydist_golden.py), the other routes of a warped model, and the identity curve through the
siblings against the entry points that read sdist / near / far."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
from oracle import raymarch as rm
from test_glo_gpu import f32_engine, types_ns
from test_raydist_cpu import CURVE_FILES, s_to_t_f64
from test_train_step import check_grad, losses_of, train_batch

pytestmark = pytest.mark.gpu

CURVE_ID = {"piecewise": 1, "power_transformation": 2, "reciprocal": 3, "log": 4, "exp": 5, "sqrt": 6, "square": 7}
MODEL_FN = {"power_transformation": "power_transformation", "piecewise": "piecewise", "reciprocal": torch.reciprocal}


def s_to_t_hip(curve, s, near, far, lam=-1.5):
    from ucnerf_amd import _lib
    lib = _lib.load()
    s, near, far = (x.float().cuda().contiguous() for x in (s, near, far))
    N, S1 = s.shape
    t = torch.full_like(s, float("nan"))
    _lib.check(lib.ucn_s_to_t(s.data_ptr(), near.data_ptr(), far.data_ptr(), N, S1, curve, lam, t.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    return t.cpu()


def curve_name(fx):
    return bytes(fx["raydist"].numpy()).decode().replace("torch.", "")


# ---------------------------------------------------------------------------------------------------- 1. ucn_s_to_t
@pytest.mark.parametrize("name", CURVE_FILES)
def test_s_to_t_against_float64(name):
    """|hip - f64| <= 2 |ref_f32 - f64| + 2 ulp(t), elementwise, on the fixture's (near, far, s) grid: s = 0, s = 1, the last
    fenceposts before 1 (the power curve's saturation) and far up to 1e5.  f64 = the reference's formula in float64 arithmetic with
    its float32 eps.  piecewise / reciprocal: that bar, everywhere.  Power curve: its t comes from (pow - 1) lam_1 / 2, so ulp is
    taken of |t| + lam_1 / 2; where the inverse's slope amplifies an ulp of its argument y (a 1-ulp powf difference in s_far, near
    saturation), that ulp of y is allowed too (2 |dt/ds| 2^-24 s); where it amplifies little and |t| >= 1, the bar is
    2 |ref_f32 - f64| + 4 ulp with no slope allowance."""
    fx = H.load(name)
    curve = curve_name(fx)
    s, near, far = fx["curve_s"], fx["curve_near"], fx["curve_far"]
    got = s_to_t_hip(CURVE_ID[curve], s, near[:, 0], far[:, 0]).double().numpy()
    sd, nd, fd = s.double().numpy(), near.double().numpy(), far.double().numpy()
    exact = s_to_t_f64(curve, sd, nd, fd)
    ref = fx["curve_t_f32"].double().numpy()
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    if curve == "power_transformation":                 # (pow - 1) * lam_1 / 2: an ulp of t + lam_1 / 2
        ulp = np.spacing((np.abs(exact) + 1.25).astype(np.float32)).astype(np.float64)
    h = 1e-7
    hi, lo = np.clip(sd + h, 0, 1), np.clip(sd - h, 0, 1)
    slope = np.abs(s_to_t_f64(curve, hi, nd, fd) - s_to_t_f64(curve, lo, nd, fd)) / (hi - lo)
    err = np.abs(got - exact)
    assert np.isfinite(got).all()
    if curve != "power_transformation":
        # IEEE divisions only: the plain bar, everywhere, no slope term
        bound = 2 * np.abs(ref - exact) + 2 * ulp
        assert (err <= bound).all(), (float((err / bound).max()), np.unravel_index(np.argmax(err / bound), err.shape))
    else:
        amp = slope * 2.0 ** -24 * sd                   # what one ulp of y = s s_far + (1 - s) s_near becomes in t
        bound = 2 * np.abs(ref - exact) + 2 * ulp + 2 * amp
        assert (err <= bound).all(), (float((err / bound).max()), np.unravel_index(np.argmax(err / bound), err.shape))
        # away from saturation (the slope turns an ulp of y into at most 4 ulp of t) and from t ~ 0: no slope allowance
        calm = (amp <= 4 * np.spacing(np.abs(exact).astype(np.float32))) & (np.abs(exact) >= 1)
        assert calm.sum() > 500
        tight = 2 * np.abs(ref - exact) + 4 * ulp
        assert (err <= tight)[calm].all(), float((err / tight)[calm].max())
    ulp0 = np.spacing(np.abs(exact[:, 0]).astype(np.float32) + np.float32(1.25 if curve == "power_transformation" else 0))
    assert (np.abs(got[:, 0] - nd[:, 0]) <= 2 * ulp0).all()                  # s = 0 -> near


@pytest.mark.parametrize("curve", ["log", "exp", "sqrt", "square"])
def test_s_to_t_gin_callables_against_float64(curve):
    """torch.log / exp / sqrt / square (configs.py:13-19) and their inv_mapping partners (coord.py:164-172): the reference's own
    float32 formula (torch on the CPU) against float64, the same bar (the slope term: an ulp of y through fn_inv)."""
    g = torch.Generator().manual_seed(5)
    R = 48
    near = 0.5 + torch.rand(R, generator=g)
    far = near + (1.0 + 4.0 * torch.rand(R, generator=g) if curve == "exp" else 1.0 + 30.0 * torch.rand(R, generator=g))
    s = torch.cat([torch.tensor([0.0, 1.0]), torch.rand(62, generator=g)])[None, :].expand(R, -1).contiguous()
    fwd, inv = {"log": (torch.log, torch.exp), "exp": (torch.exp, torch.log), "sqrt": (torch.sqrt, torch.square),
                "square": (torch.square, torch.sqrt)}[curve]

    def inner(s, n, f):
        sn, sf = fwd(n[:, None]), fwd(f[:, None])
        return s * sf + (1 - s) * sn
    ref = inv(inner(s, near, far)).double()
    y = inner(s.double(), near.double(), far.double())
    exact = inv(y)
    got = s_to_t_hip(CURVE_ID[curve], s, near, far).double()
    spacing = lambda x: torch.from_numpy(np.spacing(x.abs().float().numpy()).astype(np.float64))
    ulp = spacing(exact)
    # an ulp of y (a 1-ulp logf / expf difference in fn(near), fn(far)) moves t by |fn_inv'(y)| ulp(y)
    h = 1e-6 * y.abs().clamp_min(1e-3)
    slope = ((inv(y + h) - inv(y - h)) / (2 * h)).abs()
    bound = 2 * (ref - exact).abs() + 2 * ulp + 2 * slope * spacing(y)
    assert bool(((got - exact).abs() <= bound).all()), float(((got - exact).abs() / bound).max())


# ---------------------------------------------------------------------------------------------------- 2. cast probe
@pytest.mark.parametrize("name", ["raydist_cast.npz", "cast.npz"])
def test_cast_probe_tdist_vs_reference_golden(name):
    """ucn_cast_probe_tdist on the reference's metric fenceposts against its render.cast_rays (what models.py:208-218 does after
    s_to_t): raydist_cast.npz holds the power curve's fenceposts with far from 8 to 1e5 (t up to ~3e4), cast.npz the identity
    curve's (t <= 8).  The bars of test_cone_cast_and_contraction_vs_reference_golden, whose absolute ones (4e-6 on the means,
    2e-6 on t: 2 ulp of 8) scale with the distance beyond 8; the contraction's outputs are bounded (|x| <= 2) and keep theirs."""
    from ucnerf_amd import _lib
    lib = _lib.load()
    fx = H.load(name)
    N, S1 = fx["tdist"].shape
    S = S1 - 1
    f = lambda t: t.cuda().float().contiguous()
    o, d, cam, rad = f(fx["origins"]), f(fx["directions"]), f(fx["cam_dirs"]), f(fx["radii"]).reshape(-1)
    for tag, fl, sp in (("eval", None, None), ("train", f(fx["train_flip"]), f(fx["train_spin"]))):
        basis = torch.empty(N, 6, device="cuda")
        _lib.check(lib.ucn_cone_basis(cam.data_ptr(), f(fx[f"{tag}_rand_vec"]).data_ptr(), N, basis.data_ptr(), _lib.stream()))
        out = torch.full((N, S, 6, 10), float("nan"), device="cuda")
        _lib.check(lib.ucn_cast_probe_tdist(f(fx["tdist"]).data_ptr(), o.data_ptr(), d.data_ptr(), basis.data_ptr(), rad.data_ptr(),
                                            _lib.ptr(fl), _lib.ptr(sp), 0.5, N, S, out.data_ptr(), _lib.stream()))
        torch.cuda.synchronize()
        got = out.cpu().double()
        means, stds, t = fx[f"{tag}_means"].double(), fx[f"{tag}_stds"].double(), fx[f"{tag}_t"].double()
        scale = (t.abs() / 8.0).clamp_min(1.0)                            # [N, S, 6]: the distance beyond 8, per multisample
        ok = torch.isfinite(stds)
        assert torch.equal(torch.isfinite(got[..., 3]), ok)
        dm = (got[..., 0:3] - means).abs().amax(-1)
        assert float((dm / scale)[ok].max()) <= 4e-6, tag
        assert float(((got[..., 4] - t).abs() / scale)[ok].max()) <= 2e-6, tag
        assert float(((got[..., 3] - stds).abs() / stds.abs().clamp_min(1e-30))[ok].max()) <= 4e-7, tag
        okf = ok.reshape(-1)
        cm, cs = rm.contract_points(means.float().reshape(-1, 3)[okf], stds.float().reshape(-1)[okf])
        assert H.maxdiff(got[..., 5:8].reshape(-1, 3)[okf], cm / 2) <= 4e-6, tag
        assert float(((got[..., 8].reshape(-1)[okf] - cs / 2).abs() / (cs / 2).abs().clamp_min(1e-30)).max()) <= 2e-5, tag
    if name == "raydist_cast.npz":
        assert float(fx["tdist"].max()) > 1e4                              # the large distances did reach the geometry


# ---------------------------------------------------------------------------------------------------- 3. eval forward
def warped_model(fx, curve, **kw):
    spec = rm.make_spec("tiny")
    model, cfg = H.hip_model(spec, H.state_for(fx, spec), raydist_fn=MODEL_FN[curve], power_lambda=float(fx["power_lambda"]), **kw)
    return model, cfg, spec


@pytest.mark.parametrize("name", CURVE_FILES)
def test_warped_forward_vs_golden(name):
    """Model.forward (eval, rand=False) against the reference with the same curve, with the bars of test_model_forward_vs_golden
    for `tiny`: every level's sdist, weights, rgb, acc, depth, distance_mean and percentiles."""
    fx = H.load(name)
    curve = curve_name(fx)
    model, _, spec = warped_model(fx, curve)
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
        assert H.maxdiff(hist[lvl]["density"].cpu().reshape(-1), g("hist_density").reshape(-1)) <= samp, lvl
        assert H.maxdiff(r["weights"].cpu().reshape(-1), g("weights").reshape(-1)) <= (2e-4 if last else 5e-7), lvl
        assert H.maxdiff(r["rgb"].cpu().reshape(-1), g("rgb").reshape(-1)) <= H.RGB_TOL, lvl
        assert float((r["rgb"].cpu().reshape(-1) - g("rgb").reshape(-1)).abs().mean()) <= 2e-5, lvl
        assert H.maxdiff(r["acc"].cpu().reshape(-1), g("acc").reshape(-1)) <= 1e-4, lvl
        if last:
            assert H.maxdiff(hist[lvl]["rgb"].cpu().reshape(-1), g("hist_rgb").reshape(-1)) <= samp
            assert H.maxdiff(hist[lvl]["coord"].cpu().reshape(-1), g("hist_coord").reshape(-1)) <= 5e-6
        stable = (g("acc").reshape(-1) - 0.6).abs() > 1e-3
        assert H.maxdiff(r["depth"].cpu().reshape(-1)[stable], g("depth").reshape(-1)[stable]) <= 1e-3, lvl
        for k in ("distance_mean", "distance_median", "distance_percentile_5", "distance_percentile_95"):
            assert H.maxdiff(r[k].cpu().reshape(-1), g(k).reshape(-1)) <= 2e-3, (lvl, k)
        assert H.maxdiff(r["ray_sdist"].cpu(), g("ray_sdist")) <= 5e-5          # s-space, like the reference's
        assert H.maxdiff(r["ray_rgbs"].cpu(), g("ray_rgbs")) <= (samp if last else 1e-4)


# ---------------------------------------------------------------------------------------------------- 4. training step
@pytest.mark.parametrize("mode", ["split", "exact", "bf16"])
def test_warped_train_step_matches_reference(mode):
    """One training step of the power-transformation model against the reference's (train_step_raydist.npz): losses and every
    gradient, with the bars of test_glo_train_step_matches_reference (fp32 on both GEMM engines; bf16 autocast against the fp32
    reference)."""
    from ucnerf_amd.internal import train_utils as tu
    fx = H.load("train_step_raydist.npz")
    model, _, spec = warped_model(fx, "power_transformation")
    model.train()
    batch = H.pin_noise(train_batch(fx, "cuda"), H.noise_of(fx, 2))
    batch["rand_vec"] = batch["rand_vec"][:, None, None, :]
    bf16 = mode == "bf16"
    with f32_engine("split" if bf16 else mode), torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        rend, hist = model(True, batch, float(fx["train_frac"]), False)
        assert model.last_march_route == "train_graph" and rend[-1]["rgb"].requires_grad
        losses, _ = losses_of(tu, batch, rend, hist, spec)
        total = sum(losses.values())
    total.backward()
    torch.cuda.synchronize()
    for lvl in range(spec.num_levels if not bf16 else 0):                # s-space history (the interlevel / distortion losses)
        assert H.maxdiff(hist[lvl]["sdist"].detach().cpu().reshape(-1), fx[f"L{lvl}_hist_sdist"].reshape(-1)) <= 5e-5, lvl
    lrel = 3e-2 if bf16 else 2e-4
    for k, v in losses.items():
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


# ---------------------------------------------------------------------------------------------------- 5. other routes
def test_warped_render_image_and_compaction_match_the_forward():
    """On a warped model: render_image (tiles, fused march) gives the pixels Model.forward gives on the same rays, and the compacted
    march (compact_min_weight > 0) stays within the bound of test_sample_compaction_matches_the_full_evaluation."""
    from ucnerf_amd.internal import models
    spec = rm.make_spec("tiny")
    model, cfg = H.hip_model(spec, rm.init_state(spec, seed=95), raydist_fn="power_transformation", max_chunk_rays=1000)
    H_, W_ = 12, 16
    rays = H.to_dev(rm.synthetic_rays(H_ * W_, seed=7))
    rays["rand_vec"] = torch.randn(H_ * W_, 6, generator=torch.Generator().manual_seed(8)).cuda()     # the same cone bases
    with torch.no_grad():
        want, _ = model(False, dict(rays), 1.0, True)
    batch = {k: v.reshape(H_, W_, -1) for k, v in rays.items()}
    out = models.render_image(model, None, batch, False, 1.0, types_ns(render_ray_tile=8, vis_num_rays=16), verbose=False)
    torch.cuda.synchronize()
    assert model.last_march_route == "fused"
    # render_image walks the frame in tiles (other ray order, other pass boundaries): the per-ray march is the same
    assert H.maxdiff(out["rgb"].reshape(-1, 3).cpu(), want[-1]["rgb"].reshape(-1, 3).cpu()) <= 1e-6
    # compaction on a foggy field (most samples behind an opaque medium), as in the identity test
    model.nerf_mlp.density_bias = 8.0
    n = 2500
    rays = H.to_dev(rm.synthetic_rays(n, seed=96))
    rays["far"] = rays["far"] * (1 + 0.1 * torch.rand(n, 1, generator=torch.Generator().manual_seed(3))).cuda()
    rays["rand_vec"] = torch.randn(n, 6, generator=torch.Generator().manual_seed(97)).cuda()

    def march(thr):
        model.compact_min_weight = thr
        with torch.no_grad():
            r, _ = model._march(False, rays, 1.0, True, None, want_history=False)
        torch.cuda.synchronize()
        return {k: r[-1][k].clone() for k in ("rgb", "depth", "acc", "weights")}
    full, tiny, cut = march(0.0), march(1e-45), march(4e-8)
    for k in full:
        assert torch.equal(full[k], tiny[k]), k
    assert H.maxdiff(cut["rgb"].cpu(), full["rgb"].cpu()) <= 128 * 4e-8 * 1.002 + 1e-7
    for k in ("depth", "acc", "weights"):
        assert torch.equal(cut[k], full[k]), k
    model.compact_min_weight = 0.0


# ---------------------------------------------------------------------------------------------------- 6. identity siblings
def test_identity_curve_through_the_siblings_is_bit_identical():
    """tdist = ucn_s_to_t(identity) is the kernels' own s * far + (1 - s) * near, so every tdist sibling returns what the entry
    point that reads sdist / near / far returns, bit for bit: featurisation (both layouts), its table gradient (fixed-point row
    blocks; the float-row and atomic routes within their run-to-run reassociation), the cast probe, compositing and its backward."""
    from ucnerf_amd import _lib
    lib = _lib.load()
    spec = rm.make_spec("tiny")
    model, _ = H.hip_model(spec, rm.init_state(spec, seed=41))
    g = torch.Generator().manual_seed(42)
    N, S = 300, 64
    rays = H.to_dev(rm.synthetic_rays(N, seed=43))
    near = (0.1 * torch.rand(N, generator=g)).cuda()
    far = (6.0 + 4.0 * torch.rand(N, generator=g)).cuda()
    sdist = torch.sort(torch.rand(N, S + 1, generator=g), dim=-1).values.cuda()
    sdist[:, 0], sdist[:, -1] = 0.0, 1.0
    tdist = torch.full_like(sdist, float("nan"))
    st = _lib.stream()
    _lib.check(lib.ucn_s_to_t(sdist.data_ptr(), near.data_ptr(), far.data_ptr(), N, S + 1, 0, -1.5, tdist.data_ptr(), st))
    o, d, cam = (rays[k].float().contiguous() for k in ("origins", "directions", "cam_dirs"))
    rad = rays["radii"].reshape(-1).contiguous()
    basis = torch.empty(N, 6, device="cuda")
    _lib.check(lib.ucn_cone_basis(cam.data_ptr(), torch.randn(N, 3, generator=g).cuda().data_ptr(), N, basis.data_ptr(), st))
    flip, spin = torch.rand(N, S, generator=g).cuda(), torch.rand(N, S, generator=g).cuda()
    P = lambda *ts: [t.data_ptr() for t in ts]
    old_geom, new_geom = P(sdist, near, far), P(tdist)
    rest = P(o, d, basis, rad, flip, spin)
    mlp = model.nerf_mlp
    L, C = mlp.encoder.num_levels, mlp.encoder.level_dim
    desc = mlp.grid_field()
    for layout in (1, 2):
        outs = []
        for fn, geom in ((lib.ucn_march_features, old_geom), (lib.ucn_march_features_tdist, new_geom)):
            feat, coord, tm = torch.empty(N * S, L * C, device="cuda"), torch.empty(N, S, 3, device="cuda"), torch.empty(N, S, device="cuda")
            _lib.check(fn(ctypes.byref(desc), *geom, *rest, 0.5, N, S, 0, layout, feat.data_ptr(), coord.data_ptr(), tm.data_ptr(), st))
            outs.append((feat, coord, tm))
        for a, b in zip(*outs):
            assert torch.equal(a, b), layout
    gfeat = torch.randn(N * S, L * C, generator=g).cuda()
    # table gradient: the fixed-point row blocks are order-independent, hence bit-reproducible; the float row blocks and the atomic
    # scatter add in a different order on every run (a call against itself differs too): there, within that reassociation
    for lpb, ws, layout in ((0, True, 1 | _lib.BWD_FIXED_POINT), (0, True, 1), (1, False, 1)):
        grads = []
        for fn, geom in ((lib.ucn_march_features_backward, old_geom), (lib.ucn_march_features_backward_tdist, new_geom)):
            grad = torch.zeros_like(mlp.encoder.embeddings)
            w = torch.empty(lib.ucn_march_features_backward_ws_floats(ctypes.byref(desc), N, S), device="cuda") if ws else None
            _lib.check(fn(ctypes.byref(desc), *geom, *rest, 0.5, N, S, lpb, layout, gfeat.data_ptr(), grad.data_ptr(), _lib.ptr(w), st))
            grads.append(grad)
        if layout & _lib.BWD_FIXED_POINT:
            assert torch.equal(grads[0], grads[1]), (lpb, layout)
        else:
            assert torch.allclose(grads[0], grads[1], rtol=1e-5, atol=1e-6 * float(grads[0].abs().max())), (lpb, layout)
    probes = []
    for fn, geom in ((lib.ucn_cast_probe, old_geom), (lib.ucn_cast_probe_tdist, new_geom)):
        out = torch.empty(N, S, 6, 10, device="cuda")
        _lib.check(fn(*geom, *rest, 0.5, N, S, out.data_ptr(), st))
        probes.append(out)
    assert torch.equal(probes[0].nan_to_num(), probes[1].nan_to_num())
    density = torch.rand(N, S, generator=g).cuda() * 3
    rgbs = torch.rand(N, S, 3, generator=g).cuda()
    comp = []
    for fn, geom in ((lib.ucn_composite, old_geom), (lib.ucn_composite_tdist, P(tdist, far))):
        w, main, ex = torch.empty(N, S, device="cuda"), torch.empty(N, 5, device="cuda"), torch.empty(N, 4, device="cuda")
        _lib.check(fn(density.data_ptr(), rgbs.data_ptr(), *geom, d.data_ptr(), 1.0, 0, N, S, w.data_ptr(), main.data_ptr(),
                      ex.data_ptr(), st))
        comp.append((w, main, ex))
    for a, b in zip(*comp):
        assert torch.equal(a, b)
    g_w, g_main = torch.randn(N, S, generator=g).cuda(), torch.randn(N, 5, generator=g).cuda()
    back = []
    for fn, geom in ((lib.ucn_composite_backward, old_geom), (lib.ucn_composite_backward_tdist, P(tdist))):
        gd, gr = torch.empty(N, S, device="cuda"), torch.empty(N, S, 3, device="cuda")
        _lib.check(fn(density.data_ptr(), rgbs.data_ptr(), *geom, d.data_ptr(), 1.0, 0, N, S, g_w.data_ptr(), g_main.data_ptr(),
                      gd.data_ptr(), gr.data_ptr(), st))
        back.append((gd, gr))
    torch.cuda.synchronize()
    for a, b in zip(*back):
        assert torch.equal(a, b)
