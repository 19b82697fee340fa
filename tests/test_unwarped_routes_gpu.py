"""MLP.warp_fn = None on the GPU, second part: the float64 brackets (|HIP - float64| <= 2 |float32 reference - float64| + floor,
helpers.bracket) of the last level's features, densities and colours, of the table gradient, of the density
normals and of the scale features; scale featurization through the inference and the training route; the other routes of an
unwarped model (render_image, compaction, mixed-precision inference, GLO); and every old entry point against the new one with
warp = 1, bit for bit."""
import ctypes

import pytest
import torch

import helpers as H
import normals_ref as NR
import scalefeat_ref as SR
import unwarped_ref as UR
from oracle import raymarch as rm
from oracle import truth64 as t64
from test_glo_gpu import types_ns
from test_unwarped_cpu import sub
from test_unwarped_gpu import as_sdist, fixture, outside_samples, ray_args, unwarped_model

pytestmark = pytest.mark.gpu

K = 2.0


def last_level(fx, spec):
    """The fixture's last level at its own fenceposts: the oracle's cast Gaussians (float32) and the level's noise."""
    noise = H.noise_of(fx, spec.num_levels)[-1]
    batch = H.batch_of(fx)
    N = batch["near"].shape[0]
    sdist = fx["L1_hist_sdist"].reshape(N, -1)
    tdist = sdist * batch["far"] + (1 - sdist) * batch["near"]
    means, stds, _ = rm.cone_multisamples(tdist, batch["origins"], batch["directions"], batch["cam_dirs"], batch["radii"], noise.rand_vec,
                                          spec.std_scale, noise.flip, noise.spin)
    return batch, noise, tdist, means, stds


# ---------------------------------------------------------------------------------------------------- 1. brackets of the forward
@pytest.mark.parametrize("run", ["eval", "rand"])
def test_unwarped_features_density_colour_bracket(run):
    """As test_fine_level_features_density_colour_bracket, on the unwarped field: the gather's features per grid level at the
    fixture's fenceposts, then raw density, density, colour and coord per sample of the field on the oracle's cast Gaussians."""
    from ucnerf_amd import _lib
    lib = _lib.load()
    fx = fixture(run + "_")
    model, _, spec = unwarped_model(fx)
    sd = H.state_for(fx, spec)
    fs, mlp = spec.nerf, model.nerf_mlp
    batch, nz, tdist, means, stds = last_level(fx, spec)
    with torch.no_grad():
        m64, s64, _ = t64.cone_multisamples(tdist, batch["origins"], batch["directions"], batch["cam_dirs"], batch["radii"], nz.rand_vec,
                                            spec.std_scale, nz.flip, nz.spin)
        truth_f, _, _ = t64.sample_features(fs, sd[fs.prefix + ".encoder.embeddings"].double(), m64, s64, no_warp=True)
        ref_f = rm.field_density_features(fs, sd, means, stds, no_warp=True)[3]
    N, S = tdist.shape[0], tdist.shape[1] - 1
    L, C = fs.num_grid_levels, fs.grid_level_dim
    keep, args = ray_args(fx, tdist, nz.rand_vec)
    if nz.flip is not None:
        fl, sp = nz.flip.cuda().contiguous(), nz.spin.cuda().contiguous()
        args[7], args[8] = fl.data_ptr(), sp.data_ptr()
    out = torch.empty(L, N * S, C, device="cuda")
    d = mlp.grid_field()
    _lib.check(lib.ucn_march_features_warp(ctypes.byref(d), *args, 0.5, 0, N, S, 0, 0, out.data_ptr(), None, None, _lib.stream()))
    torch.cuda.synchronize()
    got = out.reshape(L, N, S, C).permute(1, 2, 0, 3).double().cpu()
    ref_f = ref_f.reshape(N, S, L, C).double()
    _, _, grid_sizes, _ = fs.layout()
    for l in range(L):
        H.bracket(f"unwarped {run} features level {l} (side {int(grid_sizes[l])})", (ref_f[:, :, l] - truth_f[:, :, l]).abs(),
                  (got[:, :, l] - truth_f[:, :, l]).abs(), K)
    with torch.no_grad():
        t = t64.field_forward(fs, t64.state64(sd), means, stds, batch["viewdirs"], no_warp=True)
        r32 = rm.field_forward(fs, sd, means, stds, batch["viewdirs"], no_warp=True)
        raw32 = rm.field_density_features(fs, sd, means, stds, no_warp=True)[0]
        dm, ds, vd = means.cuda().contiguous(), stds.cuda().contiguous(), batch["viewdirs"].cuda().contiguous()
        res = mlp(False, dm, ds, viewdirs=vd)
        raw, _, coord = mlp.predict_density(dm, ds)
    H.bracket(f"unwarped {run} raw density", (raw32.double() - t["raw_density"]).abs(), (raw.cpu().double() - t["raw_density"]).abs(), K)
    H.bracket(f"unwarped {run} density", (r32["density"].double() - t["density"]).abs(), (res["density"].cpu().double() - t["density"]).abs(), K)
    H.bracket(f"unwarped {run} rgb", (r32["rgb"].double() - t["rgb"]).abs(), (res["rgb"].cpu().double() - t["rgb"]).abs(), K)
    H.bracket(f"unwarped {run} coord", (r32["coord"].double() - t["coord"]).abs(), (coord.cpu().double() - t["coord"]).abs(), K)


@pytest.mark.parametrize("run", ["eval", "rand"])
def test_unwarped_renderings_bracket_every_level(run):
    """The remaining keys of renderings and history, at both levels: weights (history and rendering; ray_weights / ray_sdist /
    ray_rgbs are their first rows and the fenceposts handed in), rgb, acc, depth (away from the acc = 0.6 sentinel switch),
    distance_mean and the three percentiles -- as test_pixels_bracket_config_B_full_tables brackets the warped model's: Model.forward on
    the training-graph route, truth = oracle/truth64.level_forward on the unwarped field at the march's fenceposts, float32 side = the
    oracle's formulation at the same fenceposts.  Distances relative to far."""
    fx = fixture(run + "_")
    model, _, spec = unwarped_model(fx)
    sd = H.state_for(fx, spec)
    rays, noise = H.batch_of(fx), H.noise_of(fx, spec.num_levels)
    n = rays["near"].shape[0]
    rand = run == "rand"
    sdists = [fx[f"L{lvl}_hist_sdist"].reshape(n, -1).contiguous() for lvl in range(spec.num_levels)]
    batch = H.pin_noise({k: v[:, None, None, :].cuda() for k, v in rays.items()}, noise)
    if "march_noise" not in batch:
        batch["march_noise"] = [dict() for _ in sdists]
    for lvl, sdist in enumerate(sdists):
        batch["march_noise"][lvl]["sdist"] = sdist.cuda()
    batch["rand_vec"] = batch["rand_vec"][:, None, None, :]
    model.train()
    rend, hist = model(rand, batch, float(fx["train_frac"]), True)
    torch.cuda.synchronize()
    assert model.last_march_route == "train_graph"
    far = float(rays["far"].max())
    for lvl in range(spec.num_levels):
        fs, nz = spec.field_for_level(lvl), noise[lvl]
        # every side is evaluated at the fenceposts the march used: the pinned ones on the training pattern (the route pins them only
        # with rand), its own resampled ones on the eval pattern (within 5e-5 of the fixture's, test_unwarped_gpu.py)
        sdist = hist[lvl]["sdist"].detach().reshape(n, -1).cpu().contiguous()
        if rand:
            assert float((sdist - sdists[lvl]).abs().max()) == 0.0
        else:
            assert float((sdist - sdists[lvl]).abs().max()) <= 5e-5
        with torch.no_grad(), UR.unwarped_truth():
            truth, _ = t64.level_forward(spec, fs, t64.state64(sd), rays, sdist, nz)
        with torch.no_grad():
            tdist = sdist * rays["far"] + (1 - sdist) * rays["near"]
            means, stds, _ = rm.cone_multisamples(tdist, rays["origins"], rays["directions"], rays["cam_dirs"], rays["radii"], nz.rand_vec,
                                                  spec.std_scale, nz.flip, nz.spin)
            res = rm.field_forward(fs, sd, means, stds, rays["viewdirs"], no_warp=True)
            w = rm.alpha_weights(res["density"], tdist, rays["directions"], spec.opaque_background)
            ref = rm.composite(res["rgb"], w, tdist, spec.bg_intensity, rays["far"], True)
            ref["weights"] = w
        got = {k: rend[lvl][k].detach().double().cpu().reshape(n, -1).squeeze(-1) for k in truth}
        tag = f"unwarped {run} level {lvl}"
        assert H.maxdiff(hist[lvl]["weights"].detach().reshape(n, -1).cpu(), rend[lvl]["weights"].detach().reshape(n, -1).cpu()) == 0.0
        for k in ("weights", "acc") + (("rgb",) if lvl == spec.num_levels - 1 else ()):
            H.bracket(f"{tag} {k}", (ref[k].double() - truth[k]).abs(), (got[k] - truth[k]).abs(), K)
        stable = (truth["acc"] - 0.6).abs() > 1e-3
        assert torch.equal((got["depth"] == 300)[stable], (truth["depth"] == 300)[stable])
        H.bracket(f"{tag} depth / far", (ref["depth"].double() - truth["depth"]).abs()[stable] / far,
                  (got["depth"] - truth["depth"]).abs()[stable] / far, K)
        for k in ("distance_mean", "distance_median", "distance_percentile_5", "distance_percentile_95"):
            H.bracket(f"{tag} {k} / far", (ref[k].double() - truth[k]).abs() / far, (got[k] - truth[k]).abs() / far, K)


def test_unwarped_table_gradient_bracket():
    """Part 1 of test_table_gradient_bracket_full_size on the unwarped field (float rows; the compacted row-block route, the plain
    row-block kernel re-deriving its own geometry -- levels_per_block 0 without a workspace -- and the atomic one; each on metric
    fenceposts, TD = true, and on the same fenceposts as normalised ones of near = 0 and far = 1, TD = false): per level, the
    relative L2 distance of the table gradient of a random upstream gradient to float64 autograd, against the float32 oracle's own."""
    from ucnerf_amd import _lib
    lib = _lib.load()
    fx = fixture("rand_")
    model, _, spec = unwarped_model(fx)
    sd = H.state_for(fx, spec)
    fs, mlp = spec.nerf, model.nerf_mlp
    key = fs.prefix + ".encoder.embeddings"
    batch, nz, tdist, means, stds = last_level(fx, spec)
    N, S = tdist.shape[0], tdist.shape[1] - 1
    L, C = fs.num_grid_levels, fs.grid_level_dim
    grad = torch.randn(N * S, L, C, generator=torch.Generator().manual_seed(5))
    emb = sd[key].clone().requires_grad_(True)
    state = dict(sd)
    state[key] = emb
    f32 = rm.field_density_features(fs, state, means, stds, no_warp=True)[3]
    (f32.reshape(N * S, -1) * grad.reshape(N * S, -1)).sum().backward()
    table = sd[key].double().requires_grad_(True)
    m64, s64, _ = t64.cone_multisamples(tdist, batch["origins"], batch["directions"], batch["cam_dirs"], batch["radii"], nz.rand_vec,
                                        spec.std_scale, nz.flip, nz.spin)
    f64, _, _ = t64.sample_features(fs, table, m64, s64, no_warp=True)
    (f64.reshape(grad.shape) * grad.double()).sum().backward()
    keep, args = ray_args(fx, tdist, nz.rand_vec)
    fl, sp = nz.flip.cuda().contiguous(), nz.spin.cuda().contiguous()
    args[7], args[8] = fl.data_ptr(), sp.data_ptr()
    d = mlp.grid_field()
    g = grad.reshape(N * S, L * C).cuda().contiguous()
    _, offsets, grid_sizes, _ = fs.layout()
    off = [int(o) for o in offsets]
    keep_sd, args_sd = as_sdist(args, N)
    for lpb, with_ws, td in ((0, True, True), (0, False, True), (1, False, True), (0, True, False), (0, False, False), (1, False, False)):
        gt = torch.zeros_like(mlp.encoder.embeddings.detach())
        ws = torch.empty(lib.ucn_march_features_backward_ws_floats(ctypes.byref(d), N, S), device="cuda") if with_ws else None
        _lib.check(lib.ucn_march_features_backward_warp(ctypes.byref(d), *(args if td else args_sd), 0.5, 0, N, S, lpb, 1, g.data_ptr(),
                                                        gt.data_ptr(), _lib.ptr(ws), _lib.stream()))
        torch.cuda.synchronize()
        hip = gt.double().cpu()
        for l in range(L):
            a, b, c = (x[off[l]:off[l + 1]] for x in (hip, emb.grad.double(), table.grad))
            H.bracket(f"unwarped table gradient lpb {lpb} workspace {with_ws} metric {td} level {l} (side {int(grid_sizes[l])}) rel L2",
                      [float((b - c).norm() / c.norm())], [float((a - c).norm() / c.norm())], K, floor=(1e-6, 1e-6))


# ---------------------------------------------------------------------------------------------------- 2. density normals
@pytest.mark.parametrize("field", ["nerf", "prop"])
def test_unwarped_normals_bracket(field):
    """raw_grad_density and normals of MLP.forward on the fixture's cast Gaussians (inside, straddling and outside the cube) against
    float64 autograd of tests/normals_ref.py (no_warp), with the REFERENCE's own float32 values (its autograd reaches `means`
    directly without the warp) as the float32 side; bar and exclusions of tests/test_normals_gpu.py: samples where the float32 and
    float64 runs put a point into different cells, or a hidden unit lies inside the float32 error bound of its own sum."""
    full = H.load("unwarped.npz")
    fx = sub(full, "eval_")
    model, _, spec = unwarped_model(fx, disable_density_normals=False)
    sd = H.state_for(fx, spec)
    fs = spec.nerf if field == "nerf" else spec.props[0]
    mlp = model.nerf_mlp if field == "nerf" else model.prop_mlp_0
    mlp.disable_density_normals = False
    stride = int(full["normals_stride"])
    means, stds = full["cast_means"][:, ::stride].contiguous(), full["cast_stds"][:, ::stride].contiguous()
    B, G = means.shape[0] * means.shape[1], means.shape[2]
    o32 = NR.normals(fs, sd, means, stds, torch.float32, no_warp=True)
    o64 = NR.normals(fs, sd, means, stds, torch.float64, no_warp=True)
    with torch.no_grad():
        res = mlp(False, means.cuda().contiguous(), stds.cuda().contiguous(), viewdirs=None)
    torch.cuda.synchronize()
    keep = NR.cells_agree(o32["cells"], o64["cells"], B, G) & NR.h_clear(o64["h"].reshape(B, -1), o32["bound"].reshape(B, -1))
    keep &= ((o32["h"] > 0) == (o64["h"] > 0)).reshape(B, -1).all(dim=-1)
    print(f"unwarped normals {field}: kept {float(keep.float().mean()):.3f} of {B} samples")
    assert float(keep.float().mean()) >= 0.9
    g64 = o64["raw_grad_density"].reshape(B, 3)[keep]
    scale = float(g64.abs().max())
    want_g = full[f"normals_{field}_raw_grad_density"].reshape(B, 3).double()[keep]
    got_g = res["raw_grad_density"].reshape(B, 3).double().cpu()[keep]
    H.bracket(f"unwarped {field} raw_grad_density", (want_g - g64).abs(), (got_g - g64).abs(), K, floor=(1e-6 * scale, 1e-7 * scale))
    # normals: where the gradient is not within rounding of zero (the unit vector of a zero vector is -0, asserted in test_unwarped_gpu.py)
    alive = g64.norm(dim=-1) > 1e-3 * scale
    n64 = o64["normals"].reshape(B, 3)[keep][alive]
    want_n = full[f"normals_{field}_normals"].reshape(B, 3).double()[keep][alive]
    got_n = res["normals"].reshape(B, 3).double().cpu()[keep][alive]
    H.bracket(f"unwarped {field} normals", (want_n - n64).abs(), (got_n - n64).abs(), K)
    dead = ~UR.inside_cube(means).reshape(B, G).any(dim=-1)
    assert int(dead.sum()) > 0
    assert torch.equal(res["raw_grad_density"].reshape(B, 3).cpu()[dead], torch.zeros(int(dead.sum()), 3))


# ---------------------------------------------------------------------------------------------------- 3. scale featurization
def scale_model(fx, **kw):
    from ucnerf_amd.internal import models
    spec = rm.make_spec("tiny")
    sd = SR.state_for(fx, spec)
    with models.bindings(NerfMLP=dict(warp_fn=None), PropMLP=dict(warp_fn=None)):
        model, cfg = SR.hip_model(spec, sd, **kw)
    assert model.nerf_mlp.warp == 0 and model.nerf_mlp.scale_featurization
    return model, cfg, spec, sd


def test_unwarped_scale_features_bracket_and_outside_weight():
    """ucn_march_scale_features_warp(warp = 0) against float64: (2 mean_j erf(1 / sqrt(8 std_j^2 gs^2)) - 1) k on the CAST std, all
    six points counted wherever they lie (models.py:505) -- a sample wholly outside the cube has the scale features of its stds,
    not zeros.  float32 side: tests/scalefeat_ref.py on the same stds."""
    from ucnerf_amd import _lib
    lib = _lib.load()
    fx = fixture("scale_")
    model, _, spec, sd = scale_model(fx)
    fs, mlp = spec.nerf, model.nerf_mlp
    batch, nz, tdist, means, stds = last_level(fx, spec)
    N, S = tdist.shape[0], tdist.shape[1] - 1
    L = fs.num_grid_levels
    emb = sd[fs.prefix + ".encoder.embeddings"]
    ref = SR.scale_features(fs, emb, stds).reshape(N * S, L).double()
    _, _, grid_sizes, idx = fs.layout()
    e64 = emb.double()
    sq = (e64 ** 2).sum(-1)
    acc = torch.zeros(L, dtype=torch.float64).index_add_(0, idx.long(), sq)
    cnt = torch.zeros(L, dtype=torch.float64).index_add_(0, idx.long(), torch.ones_like(sq)).clamp_min(1)
    k64 = (SR.INIT_STD ** 2 + acc / cnt).sqrt()
    _, s64, _ = t64.cone_multisamples(tdist, batch["origins"], batch["directions"], batch["cam_dirs"], batch["radii"], nz.rand_vec, spec.std_scale)
    truth = ((2 * t64.level_damping(s64, grid_sizes).mean(dim=-2) - 1) * k64).reshape(N * S, L)
    keep, args = ray_args(fx, tdist, nz.rand_vec)
    out = torch.full((N * S, L), float("nan"), device="cuda")
    d = mlp.grid_field()
    _lib.check(lib.ucn_march_scale_features_warp(ctypes.byref(d), *args, 0.5, 0, N, S, mlp.level_scale().data_ptr(), 1, out.data_ptr(),
                                                 _lib.stream()))
    torch.cuda.synchronize()
    got = out.double().cpu()
    H.bracket("unwarped scale features", (ref - truth).abs(), (got - truth).abs(), K)
    out_mask, _ = outside_samples(fx, 1, fx["L1_hist_sdist"])
    om = out_mask.reshape(-1)
    assert int(om.sum()) >= 100
    assert float(got[om].abs().amax(dim=-1).min()) > 0                      # the erf weights of outside points are there
    H.bracket("unwarped scale features, samples wholly outside", (ref[om] - truth[om]).abs(), (got[om] - truth[om]).abs(), K)


def test_unwarped_scale_featurization_inference_and_training_routes():
    """Model.forward with scale_featurization on an unwarped model against the reference's run (bars of
    test_warped_forward_vs_golden), and the training graph's forward (march_nodes.scale_features with warp = 0) against the fused
    march on the same draws; its backward runs and is finite."""
    fx = fixture("scale_")
    model, _, spec, _ = scale_model(fx)
    batch = H.pin_noise(H.to_dev(H.batch_of(fx)), H.noise_of(fx, spec.num_levels))
    with torch.no_grad():
        rend, hist = model(False, batch, 1.0, True)
    torch.cuda.synchronize()
    assert model.last_march_route == "fused"
    for lvl in range(spec.num_levels):
        g = lambda k: fx[f"L{lvl}_{k}"]
        last = lvl == spec.num_levels - 1
        assert H.maxdiff(hist[lvl]["sdist"].cpu(), g("hist_sdist").reshape(hist[lvl]["sdist"].shape)) <= (5e-5 if last else 0.0), lvl
        assert H.maxdiff(hist[lvl]["density"].cpu().reshape(-1), g("hist_density").reshape(-1)) <= (1e-2 if last else 2e-6), lvl
        assert H.maxdiff(rend[lvl]["weights"].cpu().reshape(-1), g("weights").reshape(-1)) <= (2e-4 if last else 5e-7), lvl
        assert H.maxdiff(rend[lvl]["rgb"].cpu().reshape(-1), g("rgb").reshape(-1)) <= H.RGB_TOL, lvl
        assert H.maxdiff(rend[lvl]["acc"].cpu().reshape(-1), g("acc").reshape(-1)) <= 1e-4, lvl
    model.train()
    model.march_route = "train"
    rend_t, _ = model(False, batch, 1.0, False)
    assert model.last_march_route == "train_graph"
    assert H.maxdiff(rend_t[-1]["rgb"].detach().reshape(-1, 3).cpu(), rend[-1]["rgb"].reshape(-1, 3).cpu()) <= H.RGB_TOL
    rend_t[-1]["rgb"].square().sum().backward()
    torch.cuda.synchronize()
    for name in ("nerf_mlp.encoder.embeddings", "nerf_mlp.density_layer.0.weight"):
        gr = dict(model.named_parameters())[name].grad
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, name
    L, C = model.nerf_mlp.encoder.num_levels, model.nerf_mlp.encoder.level_dim
    assert float(model.nerf_mlp.density_layer[0].weight.grad[:, L * C:].abs().max()) > 0        # the scale columns learn


# ---------------------------------------------------------------------------------------------------- 4. other routes
def test_unwarped_render_image_compaction_and_mixed_precision():
    """test_warped_render_image_and_compaction_match_the_forward on an unwarped model, then the mixed-precision inference
    (march_infer.mixed_level under bf16 autocast) against the fp32-class march with the bars of
    test_glo_forward_vs_golden_under_autocast (bf16 through three 256-wide layers: 3e-2 max, 3e-3 mean)."""
    from ucnerf_amd.internal import models
    spec = rm.make_spec("tiny")
    with models.bindings(NerfMLP=dict(warp_fn=None), PropMLP=dict(warp_fn=None)):
        model, cfg = H.hip_model(spec, rm.init_state(spec, seed=95), max_chunk_rays=1000)
    assert model.nerf_mlp.warp == 0
    H_, W_ = 12, 16
    rays = H.to_dev(rm.synthetic_rays(H_ * W_, seed=7))
    rays["far"] = torch.full_like(rays["far"], 2.5)
    rays["rand_vec"] = torch.randn(H_ * W_, 6, generator=torch.Generator().manual_seed(8)).cuda()
    with torch.no_grad():
        want, _ = model(False, dict(rays), 1.0, True)
    batch = {k: v.reshape(H_, W_, -1) for k, v in rays.items()}
    out = models.render_image(model, None, batch, False, 1.0, types_ns(render_ray_tile=8, vis_num_rays=16), verbose=False)
    torch.cuda.synchronize()
    assert model.last_march_route == "fused"
    assert H.maxdiff(out["rgb"].reshape(-1, 3).cpu(), want[-1]["rgb"].reshape(-1, 3).cpu()) <= 1e-6
    model._mixed_levels = 0
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        mixed, _ = model(False, dict(rays), 1.0, True)
    torch.cuda.synchronize()
    assert model._mixed_levels == spec.num_levels                             # both levels did take the bf16 kernels
    dm = (mixed[-1]["rgb"].float().reshape(-1, 3).cpu() - want[-1]["rgb"].reshape(-1, 3).cpu()).abs()
    print(f"unwarped mixed precision: rgb max {float(dm.max()):.3e} mean {float(dm.mean()):.3e}")
    assert float(dm.max()) <= 3e-2 and float(dm.mean()) <= 3e-3
    model.nerf_mlp.density_bias = 8.0
    n = 2500
    rays = H.to_dev(rm.synthetic_rays(n, seed=96))
    rays["far"] = torch.full_like(rays["far"], 2.5)
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


def test_unwarped_glo_field():
    """A GLO field with warp_fn = None: with zero codes the fused march (folded colour layers) and the training graph's forward
    (per-ray codes, _ColourMLPGlo) give the same pixels, as on a warped GLO model; MLP.forward with glo_vec runs _forward_glo."""
    from ucnerf_amd.internal import models
    from test_glo_gpu import glo_hip_model
    with models.bindings(NerfMLP=dict(warp_fn=None), PropMLP=dict(warp_fn=None)):
        model = glo_hip_model(H.load("model_glo.npz"))
    assert model.nerf_mlp.warp == 0 and model.nerf_mlp.uses_glo()
    G_ = model.num_glo_features
    n = 96
    rays = H.to_dev(rm.synthetic_rays(n, seed=11))
    rays["far"] = torch.full_like(rays["far"], 2.5)
    rays["rand_vec"] = torch.randn(n, 6, generator=torch.Generator().manual_seed(12)).cuda()
    with torch.no_grad():
        fused, _ = model(False, dict(rays), 1.0, False, zero_glo=True)
        assert model.last_march_route == "fused"
        model.march_route = "train"
        graph, _ = model(False, dict(rays), 1.0, False, zero_glo=True)
        assert model.last_march_route == "train_graph"
        model.march_route = "auto"
        means = (torch.rand(n, 5, 6, 3, generator=torch.Generator().manual_seed(13)) * 2.4 - 1.2).cuda()
        stds = torch.full((n, 5, 6), 1e-3, device="cuda")
        res = model.nerf_mlp(False, means, stds, viewdirs=rays["viewdirs"], glo_vec=torch.zeros(n, G_, device="cuda"))
        plain = model.nerf_mlp(False, means, stds, viewdirs=rays["viewdirs"], glo_vec=None, no_warp=True)
    torch.cuda.synchronize()
    assert H.maxdiff(graph[-1]["rgb"].reshape(-1, 3).cpu(), fused[-1]["rgb"].reshape(-1, 3).cpu()) <= H.RGB_TOL
    assert torch.equal(res["coord"], plain["coord"])
    assert H.maxdiff(res["coord"].cpu(), means.mean(dim=-2).cpu()) <= 4 * 2.0 ** -23       # the plain mean of six (|x| <= 1.2; the sum's order differs)
    assert H.maxdiff(res["density"].cpu(), plain["density"].cpu()) <= 1e-4
    assert bool(torch.isfinite(res["rgb"]).all())


# ---------------------------------------------------------------------------------------------------- 5. old against new, bit for bit
def test_every_old_entry_point_is_the_new_one_with_warp_1():
    """The shape of test_identity_curve_through_the_siblings_is_bit_identical: ucn_march_features / _backward / _scale_features /
    _density_grad / ucn_cast_probe and their _tdist siblings against the *_warp entry points with warp = 1, torch.equal.  The table
    gradient on its order-independent route (fixed-point row blocks); the float routes differ between two calls of ONE entry point."""
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
    P = lambda *ts: [None if t is None else t.data_ptr() for t in ts]
    rest = P(o, d, basis, rad, flip, spin)
    # (old entry point or None, its fencepost arguments, the new entry point's fencepost arguments)
    kinds = (("", P(sdist, near, far), P(sdist, near, far)), ("_tdist", P(tdist), P(tdist, None, None)))
    mlp = model.nerf_mlp
    L, C = mlp.encoder.num_levels, mlp.encoder.level_dim
    desc = mlp.grid_field()
    F = ctypes.byref(desc)
    gfeat = torch.randn(N * S, L * C, generator=g).cuda()
    level_scale = torch.rand(L, generator=g).cuda() + 0.5
    assert lib.ucn_march_features_backward_row_blocks(F, N, S) == 1
    for sib, og, ng in kinds:
        for layout in (1, 2):
            outs = []
            for fn, geom, warp in ((getattr(lib, "ucn_march_features" + sib), og, ()), (lib.ucn_march_features_warp, ng, (1,))):
                feat, coord, tm = torch.empty(N * S, L * C, device="cuda"), torch.empty(N, S, 3, device="cuda"), torch.empty(N, S, device="cuda")
                _lib.check(fn(F, *geom, *rest, 0.5, *warp, N, S, 0, layout, feat.data_ptr(), coord.data_ptr(), tm.data_ptr(), st))
                outs.append((feat, coord, tm))
            for a, b in zip(*outs):
                assert torch.equal(a, b), (sib, layout)
        grads = []
        for fn, geom, warp in ((getattr(lib, "ucn_march_features_backward" + sib), og, ()), (lib.ucn_march_features_backward_warp, ng, (1,))):
            grad = torch.zeros_like(mlp.encoder.embeddings)
            w = torch.empty(lib.ucn_march_features_backward_ws_floats(F, N, S), device="cuda")
            _lib.check(fn(F, *geom, *rest, 0.5, *warp, N, S, 0, 1 | _lib.BWD_FIXED_POINT, gfeat.data_ptr(), grad.data_ptr(), w.data_ptr(), st))
            grads.append(grad)
        assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0, sib
        scales = []
        for fn, geom, warp in ((getattr(lib, "ucn_march_scale_features" + sib), og, ()), (lib.ucn_march_scale_features_warp, ng, (1,))):
            out = torch.empty(N * S, L, device="cuda")
            _lib.check(fn(F, *geom, *rest, 0.5, *warp, N, S, level_scale.data_ptr(), 1, out.data_ptr(), st))
            scales.append(out)
        assert torch.equal(scales[0], scales[1]), sib
        probes = []
        for fn, geom, warp in ((getattr(lib, "ucn_cast_probe" + sib), og, ()), (lib.ucn_cast_probe_warp, ng, (1,))):
            out = torch.empty(N, S, 6, 10, device="cuda")
            _lib.check(fn(*geom, *rest, 0.5, *warp, N, S, out.data_ptr(), st))
            probes.append(out)
        assert torch.equal(probes[0].nan_to_num(), probes[1].nan_to_num()), sib
        # the density gradient has one old entry point for both kinds of fenceposts
        nrm = []
        gl = torch.randn(L, N * S, C, generator=g).cuda()
        for fn, warp in ((lib.ucn_march_density_grad, ()), (lib.ucn_march_density_grad_warp, (1,))):
            raw, nn_ = torch.empty(N, S, 3, device="cuda"), torch.empty(N, S, 3, device="cuda")
            _lib.check(fn(F, *ng, *rest, 0.5, *warp, N, S, 0, gl.data_ptr(), raw.data_ptr(), nn_.data_ptr(), st))
            nrm.append((raw, nn_))
        torch.cuda.synchronize()
        for a, b in zip(*nrm):
            assert torch.equal(a, b), sib
