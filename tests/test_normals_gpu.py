"""Density normals (MLP.disable_density_normals = False) on the GPU: csrc/march_normals.hip and the routes that fill
`raw_grad_density` / `normals`, against the autograd restatement tests/normals_ref.py.

Bar (everywhere): helpers.bracket with e_ref = |restatement float32 - restatement float64|, e_hip = |HIP - restatement float64|,
k = 2 and a floor of (1e-6, 1e-7) * max|value| (helpers.bracket's default floor, scaled from O(1) quantities to the gradient's
size).  Left out, at most 5 % of the samples each: samples where the two restatements put some (multisample, level) into
different cells; samples with a hidden unit inside the float32 error bound of its own sum (the ReLU mask is undecided); and, for
`normals` only, samples with |g| below 1e-3 of the median (normalising them amplifies without bound: finite and |n| <= 1 there).

Both discrete choices are made on the gradient kernels' INPUTS, the forward's grid coordinates and features, and the forward
rounds the contraction in another order than torch's float32 (contracted FMAs): on 0.1-0.3 % of the points its u is one ulp off the
float32 restatement's, which at 8192 moves about 1 sample in 2000 into the neighbouring cell although the two restatements agree
(a gradient error of O(1), where the bracket allows 1e-2), or moves a feature by 1e-4 and with it an h across zero; the float32
restatement's own h crosses zero the same way, which would only widen the bracket.  So the tests take further evaluations of the two
choices -- the float32 restatement's ReLU signs, and the forward kernels' own outputs (ucn_cast_probe / ucn_contract_probe,
ucn_march_features / ucn_points_features: not the kernels under test, normals_ref.forward_choices) -- and leave out the samples where
one of them disagrees with the float64 restatement's.  What these leave out beyond the two exclusions above is asserted to stay
below EXTRA_CAP = 0.5 % of the samples (observed: 0 - 0.22 %, cells and masks together, against the ~0.1 % expected from the rate of
one-ulp differences): a kernel that mislocates or mis-masks more samples than that fails."""
import ctypes
import functools

import pytest
import torch

import helpers as H
import normals_ref as nr
from oracle import raymarch as rm

pytestmark = pytest.mark.gpu
CAP = 0.05
EXTRA_CAP = 0.005


def _spec():
    """A colour field whose finest level is 8192 on a hashed table (2^12 rows) and a density-only field that is tiled throughout."""
    nerf = rm.FieldSpec('nerf_mlp', grid_desired_resolution=8192, grid_level_dim=2, grid_log2_hashmap_size=12, bottleneck_width=64,
                        net_width_viewdirs=64)
    prop = rm.FieldSpec('prop_mlp_0', grid_desired_resolution=64, grid_level_dim=2, grid_log2_hashmap_size=19, disable_rgb=True)
    return rm.PathSpec(num_levels=2, num_prop_samples=32, num_nerf_samples=32, prop_desired_grid_size=[64, 2048], nerf=nerf, props=[prop])


def _model(spec, sd, normals=True, **kw):
    from ucnerf_amd.internal import models
    on = dict(disable_density_normals=not normals)
    with models.bindings(NerfMLP=on, PropMLP=on):
        return H.hip_model(spec, sd, **kw)


@functools.lru_cache(maxsize=None)
def _setup():
    spec = _spec()
    sd = rm.init_state(spec, seed=3)
    model, cfg = _model(spec, sd)
    return spec, sd, model, cfg


def _bracket(name, hip, r32, r64, keep, cap_ok=True):
    hip, r32, r64 = hip.double().cpu()[keep], r32.double()[keep], r64.double()[keep]
    scale = float(r64.abs().max())
    return H.bracket(name, (r32 - r64).abs(), (hip - r64).abs(), k=2.0, floor=(1e-6 * scale, 1e-7 * scale))


def _check_sample_normals(name, hip_g, hip_n, o32, o64, B, G, fs, sd, u_fwd, feat_fwd):
    """The per-sample bar of the module docstring on raw_grad_density [B, 3] and normals [B, 3].  u_fwd [B*G, 3] / feat_fwd [B, L*C]: the
    forward kernels' own grid coordinates and features (nr.forward_choices), a third evaluation of the two discrete choices."""
    h32, h64 = o32['h'].reshape(B, -1), o64['h'].reshape(B, -1)
    same_cell = nr.cells_agree(o32['cells'], o64['cells'], B, G)                   # the issue's exclusions, at its cap
    clear = nr.h_clear(h64, o32['bound'].reshape(B, -1))
    c_fwd, h_fwd, b_fwd = nr.forward_choices(fs, sd, u_fwd.cpu(), feat_fwd.cpu())
    agree = nr.cells_agree(c_fwd, o64['cells'], B, G) & ((h32 > 0) == (h64 > 0)).all(dim=-1)
    agree &= nr.h_clear(h_fwd, b_fwd) & ((h_fwd > 0) == (h64 > 0)).all(dim=-1)
    extra = same_cell & clear & ~agree                                             # what only the further evaluations leave out
    print(f"{name}: cell disagreement {1 - same_cell.float().mean():.4f}, undecided mask {1 - clear.float().mean():.4f}, "
          f"further evaluations {extra.float().mean():.4f}")
    assert 1 - same_cell.float().mean() <= CAP and 1 - clear.float().mean() <= CAP
    assert extra.float().mean() <= EXTRA_CAP
    same_cell, clear = same_cell & agree, clear
    keep = same_cell & clear
    g64 = o64['raw_grad_density'].reshape(B, 3)
    _bracket(name + ' raw_grad', hip_g.reshape(B, 3), o32['raw_grad_density'].reshape(B, 3), g64, keep)
    norm = g64.norm(dim=-1)
    tiny = norm < 1e-3 * norm[keep].median()
    assert (tiny & keep).float().mean() <= CAP
    hn = hip_n.reshape(B, 3).cpu()
    assert torch.isfinite(hn).all() and (hn.norm(dim=-1) <= 1 + 1e-6).all()
    _bracket(name + ' normals', hn, o32['normals'].reshape(B, 3), o64['normals'].reshape(B, 3), keep & ~tiny)
    return keep, tiny


# ------------------------------------------------------------------ (a) ucn_density_feature_grad
@pytest.mark.parametrize("which", ["prop", "nerf"])
def test_density_feature_grad(which):
    from ucnerf_amd import _lib
    spec, sd, model, _ = _setup()
    fs, mlp = (spec.props[0], model.prop_mlp_0) if which == "prop" else (spec.nerf, model.nerf_mlp)
    B, L, C = 4096, fs.num_grid_levels, fs.grid_level_dim
    feat = torch.rand(B, L * C, generator=torch.Generator().manual_seed(1)) * 2 - 1
    out = {}
    for dt in (torch.float32, torch.float64):
        f = feat.to(dt).requires_grad_(True)
        raw, h, bound = nr.density_layers(fs, sd, f, dt)
        (g,) = torch.autograd.grad(raw.sum(), f)
        out[dt] = (g.detach(), h.detach(), bound.detach())
    keep = nr.h_clear(out[torch.float64][1], out[torch.float32][2])
    print(f"undecided mask {1 - keep.float().mean():.4f}")
    assert 1 - keep.float().mean() <= CAP
    planes = feat.reshape(B, L, C).permute(1, 0, 2).contiguous().cuda()
    got = torch.empty_like(planes)
    d = mlp.normals_field()
    _lib.check(_lib.load().ucn_density_feature_grad(ctypes.byref(d), planes.data_ptr(), B, got.data_ptr(), _lib.stream()))
    inplace = planes.clone()
    _lib.check(_lib.load().ucn_density_feature_grad(ctypes.byref(d), inplace.data_ptr(), B, inplace.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    assert torch.equal(got, inplace)                       # gfeat may be the feature buffer itself
    got = got.permute(1, 0, 2).reshape(B, L * C)
    _bracket(f"feature_grad {which}", got, out[torch.float32][0], out[torch.float64][0], keep)


# ------------------------------------------------------------------ (b) ucn_points_density_grad through MLP.forward
def _points(B=4096, G=6, seed=2):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(B, 1, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    r = torch.cat([torch.rand(B // 2, generator=g) * 0.98, 1.02 + 28.98 * torch.rand(B - B // 2, generator=g)])
    means = d * r[:, None, None] + 0.003 * torch.randn(B, G, 3, generator=g)
    means[0] = 0.0                                          # the origin exactly (the clamp of coord.py:64)
    stds = 10 ** (-4 + 4 * torch.rand(B, G, generator=g))   # saturated and active erf
    return means, stds


@functools.lru_cache(maxsize=None)
def _points_ref(which, warp):
    spec, sd, _, _ = _setup()
    fs = spec.props[0] if which == "prop" else spec.nerf
    means, stds = _points()
    if not warp:
        means = means / 31                                  # inside the grid's cube without the contraction
    return means, stds, nr.normals(fs, sd, means, stds, torch.float32, not warp), nr.normals(fs, sd, means, stds, torch.float64, not warp)


def _points_forward(mlp, means, stds, warp):
    """The forward's own grid coordinates [B*G, 3] (ucn_contract_probe) and features [B, L*C] (ucn_points_features) of these Gaussians."""
    from ucnerf_amd import _lib
    lib, st = _lib.load(), _lib.stream()
    B, G = stds.shape
    L, C = mlp.encoder.num_levels, mlp.encoder.level_dim
    feat, coord = torch.empty(L, B, C, device='cuda'), torch.empty(B, 3, device='cuda')
    _lib.check(lib.ucn_points_features(ctypes.byref(mlp.grid_field()), means.data_ptr(), stds.data_ptr(), B, G, warp, 1, feat.data_ptr(),
                                       coord.data_ptr(), st))
    c = means.reshape(B * G, 3).contiguous()
    if warp:
        c, sd_c = torch.empty(B * G, 3, device='cuda'), torch.empty(B * G, device='cuda')
        _lib.check(lib.ucn_contract_probe(means.data_ptr(), stds.data_ptr(), B * G, c.data_ptr(), sd_c.data_ptr(), st))
    torch.cuda.synchronize()
    return (c + 1.0) / 2.0, feat.permute(1, 0, 2).reshape(B, L * C)


@pytest.mark.parametrize("warp", [1, 0])
@pytest.mark.parametrize("which", ["nerf", "prop"])
def test_points_density_grad(which, warp):
    spec, sd, model, _ = _setup()
    mlp, fs = (model.prop_mlp_0, spec.props[0]) if which == "prop" else (model.nerf_mlp, spec.nerf)
    means, stds, o32, o64 = _points_ref(which, warp)
    B, G = stds.shape
    res = mlp(False, means.cuda(), stds.cuda(), no_warp=not warp)
    torch.cuda.synchronize()
    assert res['raw_grad_density'].shape == (B, 3) and res['normals'].shape == (B, 3)
    assert H.maxdiff(res['coord'].cpu(), o32['coord']) <= 1e-6
    u_fwd, feat_fwd = _points_forward(mlp, means.cuda(), stds.cuda(), warp)
    _check_sample_normals(f"points {which} warp={warp}", res['raw_grad_density'], res['normals'], o32, o64, B, G, fs, sd, u_fwd, feat_fwd)


# ------------------------------------------------------------------ (c) ucn_march_density_grad
def _march_inputs(N=64, S=32):
    from ucnerf_amd import _lib
    from ucnerf_amd.internal import march_level as ml
    lib, st = _lib.load(), _lib.stream()
    batch = H.to_dev(rm.synthetic_rays(N, seed=5))          # origin inside the unit ball, far = 8: every ray crosses the sphere
    rays = ml.Rays(batch, 2)
    g = torch.Generator().manual_seed(9)
    sdist = torch.sort(torch.rand(N, S + 1, generator=g), dim=-1).values.cuda()
    basis = torch.empty(N, 6, device='cuda')
    rvec = torch.randn(N, 3, generator=g).cuda()
    _lib.check(lib.ucn_cone_basis(rays.cam.data_ptr(), rvec.data_ptr(), N, basis.data_ptr(), st))
    flip, spin = torch.rand(N, S, generator=g).cuda(), torch.rand(N, S, generator=g).cuda()
    return rays, sdist, basis, flip, spin


def _march_hip(mlp, posts, rays, flip, spin, N, S, layout):
    from ucnerf_amd import _lib
    from ucnerf_amd.internal import march_level as ml
    lib, st = _lib.load(), _lib.stream()
    L, C = mlp.encoder.num_levels, mlp.encoder.level_dim
    feat = torch.empty(L * N * S * C, device='cuda')
    _lib.check(posts.entry(lib, 'ucn_march_features')(ctypes.byref(mlp.grid_field()), *posts.geometry(rays, flip, spin), 0.5, N, S, 0, layout,
                                                      feat.data_ptr(), None, None, st))
    fwd = feat.clone()                                      # density_normals turns `feat` into d raw / d features in place
    g, n = torch.empty(N, S, 3, device='cuda'), torch.empty(N, S, 3, device='cuda')
    ml.density_normals(mlp, posts, rays, flip, spin, slice(None), N, S, 0.5, layout, feat, g, n, st)
    probe = torch.empty(N, S, 6, 10, device='cuda')
    if posts.tdist is None:
        _lib.check(lib.ucn_cast_probe(*posts.geometry(rays, flip, spin), 0.5, N, S, probe.data_ptr(), st))
    else:
        _lib.check(lib.ucn_cast_probe_tdist(*posts.geometry(rays, flip, spin), 0.5, N, S, probe.data_ptr(), st))
    torch.cuda.synchronize()
    fwd = fwd.reshape(L, S, N, C).permute(0, 2, 1, 3) if layout == 2 else fwd.reshape(L, N, S, C)
    return g, n, probe[..., 0:3].cpu(), probe[..., 3].cpu(), (probe[..., 5:8].reshape(-1, 3) + 1.0) / 2.0, fwd.permute(1, 2, 0, 3).reshape(N * S, L * C)


@pytest.mark.parametrize("layout,pinned,warped", [(0, False, False), (2, True, False), (0, True, True), (2, False, True)])
def test_march_density_grad(layout, pinned, warped):
    from ucnerf_amd import _lib
    from ucnerf_amd.internal import march_level as ml
    spec, sd, model, _ = _setup()
    mlp, fs = model.nerf_mlp, spec.nerf
    N, S = 64, 32
    rays, sdist, basis, flip, spin = _march_inputs(N, S)
    if not pinned:
        flip = spin = None
    tdist = None
    if warped:
        tdist = torch.empty_like(sdist)
        _lib.check(_lib.load().ucn_s_to_t(sdist.data_ptr(), rays.near.data_ptr(), rays.far.data_ptr(), N, S + 1, 2, -1.5, tdist.data_ptr(),
                                          _lib.stream()))
    posts = ml.Fenceposts(sdist, rays.near, rays.far, tdist, basis)
    g, n, means, stds, u_fwd, feat_fwd = _march_hip(mlp, posts, rays, flip, spin, N, S, layout)
    o32 = nr.normals(fs, sd, means.reshape(N * S, 6, 3), stds.reshape(N * S, 6), torch.float32)
    o64 = nr.normals(fs, sd, means.reshape(N * S, 6, 3), stds.reshape(N * S, 6), torch.float64)
    _check_sample_normals(f"march layout={layout} pinned={pinned} warped={warped}", g, n, o32, o64, N * S, 6, fs, sd, u_fwd, feat_fwd)
    if not warped:
        # the identity curve's metric fenceposts give the same bits (near = 0: sdist * far is the kernels' own t)
        td = sdist * rays.far + (1 - sdist) * rays.near
        g2, n2 = _march_hip(mlp, ml.Fenceposts(sdist, rays.near, rays.far, td, basis), rays, flip, spin, N, S, layout)[:2]
        assert torch.equal(g, g2) and torch.equal(n, n2)


# ------------------------------------------------------------------ (d) end to end
def _frame(n, seed=5, train=False):
    spec, sd, model, cfg = _setup()
    rays = rm.synthetic_rays(n, seed=seed)
    noise = [rm.draw_level_noise(spec, n, lvl, train, torch.Generator().manual_seed(7 + lvl)) for lvl in range(2)]
    return spec, sd, model, cfg, rays, noise


def _reference_last_level(spec, sd, rays, noise, sdist):
    """The restatement on the NeRF level's samples, from the march's own fenceposts (the resampling is not under test here)."""
    tdist = sdist * rays['far'] + (1 - sdist) * rays['near']
    nz = noise[-1]
    means, stds, _ = rm.cone_multisamples(tdist, rays['origins'], rays['directions'], rays['cam_dirs'], rays['radii'], nz.rand_vec,
                                          spec.std_scale, nz.flip, nz.spin)
    N, S = sdist.shape[0], sdist.shape[1] - 1
    m, s = means.reshape(N * S, 6, 3), stds.reshape(N * S, 6)
    return nr.normals(spec.nerf, sd, m, s, torch.float32), nr.normals(spec.nerf, sd, m, s, torch.float64)


@pytest.mark.parametrize("mode", [1, 0])
def test_model_forward_inference_and_training_route(mode):
    n = 256
    spec, sd, model, cfg, rays, noise = _frame(n, train=True)            # pinned jitter / flip / spin
    model.nerf_mlp.mlp_mode = mode
    batch = H.pin_noise(H.to_dev(rays), noise)
    model.eval()
    with torch.no_grad():
        rend, hist = model(True, batch, 1.0, True)
    torch.cuda.synchronize()
    S = spec.num_nerf_samples
    for lvl in range(2):
        assert hist[lvl]['normals'].shape == hist[lvl]['raw_grad_density'].shape == (n, hist[lvl]['weights'].shape[-1], 3)
        assert rend[lvl]['normals'].shape == (n, 3)
    o32, o64 = _reference_last_level(spec, sd, rays, noise, hist[-1]['sdist'].cpu())
    # the forward's own grid coordinates and features on these samples: the level's pinned draws and fenceposts through the same entries
    from ucnerf_amd import _lib
    from ucnerf_amd.internal import march_level as ml
    mrays = ml.Rays(batch, 2)
    _, flip, spin, rvec = ml.draws(mrays, 1, S, True, model.single_jitter)
    basis = torch.empty(n, 6, device='cuda')
    _lib.check(_lib.load().ucn_cone_basis(mrays.cam.data_ptr(), rvec.data_ptr(), n, basis.data_ptr(), _lib.stream()))
    posts = ml.Fenceposts(hist[-1]['sdist'].reshape(n, S + 1).contiguous(), mrays.near, mrays.far, None, basis)
    g_k, n_k, _, _, u_fwd, feat_fwd = _march_hip(model.nerf_mlp, posts, mrays, flip, spin, n, S, 0)
    assert torch.equal(g_k, hist[-1]['raw_grad_density']) and torch.equal(n_k, hist[-1]['normals'])      # the same samples
    keep, tiny = _check_sample_normals(f"model mode={mode}", hist[-1]['raw_grad_density'], hist[-1]['normals'], o32, o64, n * S, 6, spec.nerf,
                                       sd, u_fwd, feat_fwd)
    # the composite, per ray: the bracket on sum_s w_s n_s plus twice the weight of the ray's flagged samples (a flagged sample
    # can move the composite by at most twice its weight: |n| <= 1 on both sides); no ray is left out
    w = hist[-1]['weights'].double().cpu()
    n32, n64 = o32['normals'].double().reshape(n, S, 3), o64['normals'].double().reshape(n, S, 3)
    flagged = ~(keep & ~tiny).reshape(n, S)
    wk = torch.where(flagged, torch.zeros_like(w), w)
    e_ref = ((wk[..., None] * (n32 - n64)).sum(dim=-2)).abs().amax(dim=-1)
    hip_n = hist[-1]['normals'].double().cpu()
    want = (wk[..., None] * n64).sum(dim=-2) + (torch.where(flagged, w, torch.zeros_like(w))[..., None] * hip_n).sum(dim=-2)
    e_hip = (rend[-1]['normals'].double().cpu() - want).abs().amax(dim=-1)
    allow = 2 * torch.where(flagged, w, torch.zeros_like(w)).sum(dim=-1)
    print(f"composite: e_ref max {e_ref.max():.3e} e_hip max {e_hip.max():.3e} flagged weight max {allow.max():.3e}")
    assert (e_hip <= 2 * e_ref.max() + 1e-6 + allow).all()
    # the training route on the same pinned draws: the same normals, detached.  The fenceposts are pinned too: the two routes' dense
    # layers round the proposal density differently, and the next level's resampling would carry that into the sample positions
    model.train()
    batch['march_noise'] = [dict(nz, sdist=hist[lvl]['sdist']) for lvl, nz in enumerate(batch['march_noise'])]
    rend_t, hist_t = model(True, batch, 1.0, True)
    torch.cuda.synchronize()
    assert model.last_march_route == 'train_graph'
    for lvl in range(2):
        for k in ('normals', 'raw_grad_density'):
            assert not hist_t[lvl][k].requires_grad
            assert torch.equal(hist_t[lvl][k], hist[lvl][k]), (lvl, k)
        assert not rend_t[lvl]['normals'].requires_grad
        assert H.maxdiff(rend_t[lvl]['normals'].cpu(), rend[lvl]['normals'].cpu()) <= 1e-5
    model.eval()


def test_model_routes_fill_the_same_normals():
    """The other inference routes with the flag on, against the default route (rays fastest, no compaction, fp32-class) on the same pinned
    draws: ray-major passes (layout 0), sample compaction (normals for ALL samples), and bf16 autocast (a field with normals renders on
    the fp32-class path: the same colours too).  The last level's fenceposts come from the same proposal level, so the samples are the
    same; the gradient kernels see the same points and the same features."""
    n = 256
    spec, sd, model, cfg, rays, noise = _frame(n, train=True)
    batch = H.pin_noise(H.to_dev(rays), noise)
    model.eval()
    S = spec.num_nerf_samples

    def run(autocast=False):
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
            rend, hist = model(True, batch, 1.0, True)
        torch.cuda.synchronize()
        return rend, hist
    rend0, hist0 = run()
    saved = model.rays_fastest, model.compact_min_weight
    try:
        model.rays_fastest = False
        rend1, hist1 = run()
        model.rays_fastest = saved[0]
        model.compact_min_weight = 1e-3
        rend2, hist2 = run()
        model.compact_min_weight = saved[1]
        rend3, hist3 = run(autocast=True)
    finally:
        model.rays_fastest, model.compact_min_weight = saved
    for tag, rend, hist in (('ray-major', rend1, hist1), ('compacted', rend2, hist2), ('autocast', rend3, hist3)):
        for lvl in range(2):
            assert torch.equal(hist[lvl]['sdist'], hist0[lvl]['sdist']), (tag, lvl)
            for k in ('raw_grad_density', 'normals'):
                assert hist[lvl][k].shape == hist0[lvl][k].shape and torch.equal(hist[lvl][k], hist0[lvl][k]), (tag, lvl, k)
        assert rend[-1]['normals'].shape == (n, 3)
    assert torch.equal(rend3[-1]['rgb'], rend0[-1]['rgb'])              # autocast: the fp32-class path, not the bf16 one
    assert H.maxdiff(rend1[-1]['normals'].cpu(), rend0[-1]['normals'].cpu()) <= 1e-6
    assert torch.isfinite(rend2[-1]['normals']).all() and (rend2[-1]['normals'].norm(dim=-1) <= 1 + 1e-5).all()


def test_render_image_returns_normals():
    from ucnerf_amd.internal import models
    spec, sd, model, cfg, rays, noise = _frame(256, seed=6)
    batch = {k: v.reshape(16, 16, -1).cuda() for k, v in rays.items()}
    batch["rand_vec"] = torch.cat([nz.rand_vec for nz in noise], dim=-1).reshape(16, 16, -1).cuda()

    class OneProc:
        num_processes, process_index, is_main_process = 1, 0, True
    out = models.render_image(model, OneProc(), batch, False, 1.0, cfg, verbose=False)
    model.eval()
    assert out['normals'].shape == (16, 16, 3) and torch.isfinite(out['normals']).all()
    with torch.no_grad():
        rend, _ = model(False, H.pin_noise(H.to_dev(rays), noise), 1.0, True)
    # the frame is marched in tile order: the same rays, the same kernels
    assert H.maxdiff(out['normals'].reshape(256, 3).cpu(), rend[-1]['normals'].cpu()) <= 1e-6
    assert (out['normals'].norm(dim=-1) <= 1 + 1e-5).all()


# ------------------------------------------------------------------ (e) the flag at its shipped value
def test_flag_off_is_unchanged():
    """The existing golden of the tiny spec still holds bit for bit what a flag-off model gives beside a flag-on one (same library,
    same weights), and its normals keys are None."""
    fx = H.load("model_tiny.npz")
    spec = rm.make_spec("tiny")
    sd = H.state_for(fx, spec)
    off, _ = H.hip_model(spec, sd)
    batch = H.pin_noise(H.to_dev(H.batch_of(fx)), H.noise_of(fx, 2))
    with torch.no_grad():
        rend, hist = off(False, batch, 1.0, True)
        on, _ = _model(spec, sd)
        rend_on, hist_on = on(False, batch, 1.0, True)
        rend2, hist2 = off(False, batch, 1.0, True)
    for lvl in range(2):
        assert hist[lvl]['normals'] is None and hist[lvl]['raw_grad_density'] is None and 'normals' not in rend[lvl]
        for k in ('rgb', 'depth', 'acc', 'weights'):
            assert torch.equal(rend[lvl][k], rend_on[lvl][k]) and torch.equal(rend[lvl][k], rend2[lvl][k]), (lvl, k)
        for k in ('density', 'rgb', 'coord', 'sdist', 'weights'):
            assert torch.equal(hist[lvl][k], hist_on[lvl][k]), (lvl, k)
    assert H.maxdiff(rend[-1]['rgb'].cpu(), fx['L1_rgb']) <= H.RGB_TOL
