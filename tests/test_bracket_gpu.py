"""Brackets (-m gpu): for a quantity q on identical inputs, e_ref = |q of the float32 oracle - q of oracle/truth64.py| and
e_hip = |q of the HIP kernel - truth|.  Each test asserts that e_ref is really nonzero at the scale the loose absolute bars of
test_gpu_parity / test_train_full_size talk about, and that e_hip <= k e_ref + floor, worst case and on average, with the
project's k = 2 and the floors of test_fine_level_per_sample_error_is_bracketed_by_the_float32_reference_itself
(helpers.bracket).  k is not chosen from what the HIP side measures.  Run with -s for the report lines
(profiles/bracket/bracket_report.txt holds one run's).

Covered here: the cone cast and the contraction (eval and training pattern, fenceposts up to 3e4), the per-level features /
raw density / colour on the L = 16 specs and field.npz, and the table gradient of the featurisation per level at FULL table
size (config B and the waymo.gin grid; float and fixed-point rows) with the no-flip subset and the position-independent level
sums.  Then the pixels of config B at full table size at pinned fenceposts (both dense engines, identity and
power curve) and the table gradient through the whole float32 training step (both engines)."""
import ctypes
import time

import numpy as np
import pytest
import torch

import helpers as H
from oracle import raymarch as rm
from oracle import truth64 as t64

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K = 2.0
# Deliberate trades, each named in DESIGN.md "Parity analysis" with its measured ratio e_hip / e_ref; the bar is 1.5 x the largest
# ratio measured (margin for seed-to-seed spread):
#   * the contracted std feeds only the erf damping and is formed with exp2(log2(.) / 3) on the fast transcendental units
#     instead of powf (csrc/grid_cast.h): largest ratio RATIO_CSTD on the four cast patterns;
#   * UCN_BWD_FIXED_POINT (the autocast training step's table-gradient mode; the float32 step keeps exact float adds) rounds
#     every addend to a 2^-29-class grid of its task's summed |gradient|.  With a random upstream gradient that is an ADDITIVE
#     floor of 6e-6 - 9e-5 (config B) / 1.3e-5 - 8e-4 (waymo.gin grid) in a level's relative L2, far above the float32
#     reference's own 1e-6 - 1e-4 on the coarse and middle levels and invisible beside it from side 16 385 on: the ratio is
#     recorded PER LEVEL (worst of the three seeds; the seeds agree to 3 %).
RATIO_CSTD = 2.418
RATIO_FIXED_POINT = {"B": [3.48, 5.71, 5.31, 17.95, 8.99, 4.67, 2.49, 1.52, 1.15, 1.05, 1.02, 1.01, 1.0, 1.0, 1.0, 1.0],
                     "R": [6.59, 12.95, 13.75, 50.92, 30.24, 16.74, 9.04, 4.70, 2.52, 1.67]}
K_CSTD = max(K, 1.5 * RATIO_CSTD)
# Position error of a faithful float32 evaluation, in units of the unit cube the grid is addressed in, from the roundings alone:
# a cone-cast mean carries <= 24 u relative (tests/test_truth64_cpu.py::test_cast_golden_vs_truth64 asserts it of the reference),
# the contraction z = (2 - 1 / r) m / r has a Jacobian of norm <= 2 / r on |m| = r, so the mean's error arrives as <= 48 u of
# z, / 4 on the way to x = (z / 2 + 1) / 2; the contraction's own chain adds <= 10 u (tests/test_truth64_cpu.py
# _feature_bound): 22 u, rounded up.
DX = 24 * U


def _timed(name, t0):
    print(f"BRACKET-TIME {name}: {time.time() - t0:.1f} s on the host (truth64 + float32 oracle)")


# --------------------------------------------------------------------------------------------- cone cast and contraction
def _probe(fx, rand_vec, flip=None, spin=None, tdist=False):
    from ucnerf_amd import _lib
    lib = _lib.load()
    dev = "cuda"
    N, S = fx["tdist"].shape[0], fx["tdist"].shape[1] - 1
    f = lambda t: t.to(dev).float().contiguous()
    o, d, cam, rad = f(fx["origins"]), f(fx["directions"]), f(fx["cam_dirs"]), f(fx["radii"]).reshape(-1)
    basis = torch.empty(N, 6, device=dev)
    rv = f(rand_vec)
    _lib.check(lib.ucn_cone_basis(cam.data_ptr(), rv.data_ptr(), N, basis.data_ptr(), _lib.stream()))
    out = torch.full((N, S, 6, 10), float("nan"), device=dev)
    fl, sp = (None, None) if flip is None else (f(flip), f(spin))
    td = f(fx["tdist"])
    if tdist:
        _lib.check(lib.ucn_cast_probe_tdist(td.data_ptr(), o.data_ptr(), d.data_ptr(), basis.data_ptr(), rad.data_ptr(), _lib.ptr(fl),
                                            _lib.ptr(sp), 0.5, N, S, out.data_ptr(), _lib.stream()))
    else:                       # near = 0, far = 1: t = s * far + (1 - s) * near = s exactly, the golden's metric fenceposts go in as sdist
        near, far = torch.zeros(N, device=dev), torch.ones(N, device=dev)
        _lib.check(lib.ucn_cast_probe(td.data_ptr(), near.data_ptr(), far.data_ptr(), o.data_ptr(), d.data_ptr(), basis.data_ptr(),
                                      rad.data_ptr(), _lib.ptr(fl), _lib.ptr(sp), 0.5, N, S, out.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    return out.cpu().double()


def cast_sides(fx, tag):
    """truth64 and the float32 oracle on one pattern of a cast fixture: dicts of means / t / stds / contracted halved mean and std."""
    kw = {} if tag == "eval" else dict(flip=fx["train_flip"], spin=fx["train_spin"])
    args = (fx["tdist"], fx["origins"], fx["directions"], fx["cam_dirs"], fx["radii"], fx[f"{tag}_rand_vec"], 0.5)
    m, s, t = t64.cone_multisamples(*args, **kw)
    z, zs = t64.contract_points(m.reshape(-1, 3), s.reshape(-1))
    truth = dict(means=m, t=t, stds=s, cmean=z.reshape(m.shape) / 2, cstd=zs.reshape(s.shape) / 2)
    m32, s32, t32 = rm.cone_multisamples(*args, **kw)
    z32, zs32 = rm.contract_points(m32.reshape(-1, 3), s32.reshape(-1))
    ref = dict(means=m32, t=t32, stds=s32, cmean=z32.reshape(m32.shape) / 2, cstd=zs32.reshape(s32.shape) / 2)
    return truth, ref, torch.isfinite(fx[f"{tag}_stds"])


@pytest.mark.parametrize("name", ["cast.npz", "raydist_cast.npz"])
def test_cone_cast_and_contraction_bracket(name):
    """means and t relative to the element's own scale (|o| + t |d|: fenceposts reach 3e4 on the power curve), stds relative;
    the contracted halved means absolute (|.| <= 1), contracted stds relative."""
    t0 = time.time()
    fx = H.load(name)
    far = name == "raydist_cast.npz"
    for tag in ("eval", "train"):
        truth, ref, ok = cast_sides(fx, tag)
        kw = {} if tag == "eval" else dict(flip=fx["train_flip"], spin=fx["train_spin"])
        got = _probe(fx, fx[f"{tag}_rand_vec"], tdist=far, **kw)
        hip = dict(means=got[..., 0:3], stds=got[..., 3], t=got[..., 4], cmean=got[..., 5:8], cstd=got[..., 8])
        okm = ok[..., None].expand(truth["means"].shape)
        scale = (fx["origins"].double().abs()[:, None, None, :] + truth["t"][..., None] * fx["directions"].double().abs()[:, None, None, :]
                 + 1e-3 * truth["t"][..., None])
        den = dict(means=scale, t=truth["t"].abs().clamp_min(1e-30), stds=truth["stds"].abs().clamp_min(1e-30),
                   cmean=torch.ones_like(scale), cstd=truth["cstd"].abs().clamp_min(1e-30))
        for q in ("means", "t", "stds", "cmean", "cstd"):
            sel = okm if q in ("means", "cmean") else ok
            e_ref = ((ref[q].double() - truth[q]).abs() / den[q])[sel]
            e_hip = ((hip[q] - truth[q]).abs() / den[q])[sel]
            # the reference is off the truth by a good fraction of an ulp somewhere; the floors are half an ulp / a 30th of one
            H.bracket(f"{name} {tag} cast {q}", e_ref, e_hip, K_CSTD if q == "cstd" else K, floor=(U / 2, U / 32), min_ref=U / 2)
        if not far:
            # the existing absolute bars, unchanged: no position further than 2 ulp of 8 from the reference's
            want = fx[f"{tag}_means"].double()
            d = (hip["means"] - want).abs()[okm]
            assert float(d.max()) <= 4e-6, (tag, float(d.max()))
            same = int((hip["means"].float() == fx[f"{tag}_means"])[okm].sum())
            same_pts = int(((hip["means"].float() == fx[f"{tag}_means"]).all(dim=-1))[ok].sum())
            print(f"BRACKET {name} {tag}: {same} of {int(okm.sum())} mean coordinates ({same_pts} of {int(ok.sum())} multisample positions) "
                  f"are bit-identical to the reference's; largest difference {float(d.max()):.3e}")
            if tag == "eval":
                assert same_pts > 0
    _timed(f"test_cone_cast_and_contraction_bracket[{name}]", t0)


# ------------------------------------------------------------------------ per-level features, raw density, colour (L = 16)
def _march_features(model, mlp, rays, rand_vec, sdist, flip, spin):
    """ucn_march_features of one field at given fenceposts -> [N, S, L, C] on the host"""
    from ucnerf_amd import _lib
    lib = _lib.load()
    dev = "cuda"
    n, S = sdist.shape[0], sdist.shape[1] - 1
    enc = mlp.encoder
    L, C = enc.num_levels, enc.level_dim
    g = {k: v.to(dev).contiguous() for k, v in rays.items()}
    basis = torch.empty(n, 6, device=dev)
    rv = rand_vec.to(dev).contiguous()
    _lib.check(lib.ucn_cone_basis(g["cam_dirs"].data_ptr(), rv.data_ptr(), n, basis.data_ptr(), _lib.stream()))
    geom = [sdist.to(dev).contiguous(), g["near"].reshape(-1).contiguous(), g["far"].reshape(-1).contiguous(), g["origins"], g["directions"],
            basis, g["radii"].reshape(-1).contiguous(), None if flip is None else flip.to(dev).contiguous(),
            None if spin is None else spin.to(dev).contiguous()]
    desc = _lib.UcnField.from_buffer_copy(mlp.field())
    out = torch.empty(L, n * S, C, device=dev)
    _lib.check(lib.ucn_march_features(ctypes.byref(desc), *[_lib.ptr(t) for t in geom], float(model.std_scale), n, S, 0, 0, out.data_ptr(),
                                      None, None, _lib.stream()))
    torch.cuda.synchronize()
    return out.reshape(L, n, S, C).permute(1, 2, 0, 3).double().cpu(), geom


def level_sides(fx, spec, sd, lvl):
    """The last level of a model fixture at the GOLDEN's fenceposts: truth64 and the float32 oracle (features per level, raw
    density, colour per sample)."""
    batch, noise = H.batch_of(fx), H.noise_of(fx, spec.num_levels)
    nz = noise[lvl]
    fs = spec.field_for_level(lvl)
    sdist = fx[f"L{lvl}_hist_sdist"].reshape(batch["near"].shape[0], -1)
    with torch.no_grad():
        _, res = t64.level_forward(spec, fs, t64.state64(sd), batch, sdist, nz)
        tdist = sdist * batch["far"] + (1 - sdist) * batch["near"]
        means, stds, _ = rm.cone_multisamples(tdist, batch["origins"], batch["directions"], batch["cam_dirs"], batch["radii"], nz.rand_vec,
                                              spec.std_scale, nz.flip, nz.spin)
        raw32, _, _, feat32 = rm.field_density_features(fs, sd, means, stds)
        out32 = rm.field_forward(fs, sd, means, stds, batch["viewdirs"])
    L, C = fs.num_grid_levels, fs.grid_level_dim
    ref = dict(features=feat32.reshape(feat32.shape[:-1] + (L, C)).double(), raw=raw32.double(), rgb=out32["rgb"].double())
    truth = dict(features=res["features"], raw=res["raw_density"], rgb=res["rgb"], means=res["means"], stds=res["stds"])
    return truth, ref, batch, nz, sdist


@pytest.mark.parametrize("name,kind", [("model_tiny.npz", "tiny"), ("model_tiny64.npz", "tiny64"), ("model_train.npz", "tiny")])
def test_fine_level_features_density_colour_bracket(name, kind):
    """The `1e-2` cases of test_model_forward_vs_golden (eval: model_tiny, model_tiny64; training pattern: model_train), per
    LEVEL of the grid for the features so that a fault on one hashed level is not averaged away."""
    t0 = time.time()
    fx = H.load(name)
    spec = rm.make_spec(kind)
    sd = H.state_for(fx, spec)
    lvl = spec.num_levels - 1
    truth, ref, batch, nz, sdist = level_sides(fx, spec, sd, lvl)
    model, _ = H.hip_model(spec, sd)
    got, _ = _march_features(model, model.nerf_mlp, {k: v for k, v in batch.items() if k in ("near", "far", "origins", "directions", "cam_dirs", "radii")},
                             nz.rand_vec, sdist, nz.flip, nz.spin)
    _, _, grid_sizes, _ = spec.nerf.layout()
    for l in range(got.shape[2]):
        # min_ref: half an ulp of a unit-cube coordinate times the level's side times a typical neighbour difference of the table
        H.bracket(f"{name} features level {l} (side {int(grid_sizes[l])})", (ref["features"][:, :, l] - truth["features"][:, :, l]).abs(),
                  (got[:, :, l] - truth["features"][:, :, l]).abs(), K, min_ref=0.25 * U * int(grid_sizes[l]))
    # raw density and colour of the same samples through the HIP field on the TRUTH's float32-rounded Gaussians would mix two
    # roundings; the field is fed what the oracle's cast produced, as test_field_vs_golden does
    tdist = sdist * batch["far"] + (1 - sdist) * batch["near"]
    means, stds, _ = rm.cone_multisamples(tdist, batch["origins"], batch["directions"], batch["cam_dirs"], batch["radii"], nz.rand_vec,
                                          spec.std_scale, nz.flip, nz.spin)
    with torch.no_grad():
        t = t64.field_forward(spec.nerf, t64.state64(sd), means, stds, batch["viewdirs"])
        r32 = rm.field_forward(spec.nerf, sd, means, stds, batch["viewdirs"])
        raw32 = rm.field_density_features(spec.nerf, sd, means, stds)[0]
        res = model.nerf_mlp(False, means.cuda().contiguous(), stds.cuda().contiguous(), viewdirs=batch["viewdirs"].cuda().contiguous())
        raw, _, _ = model.nerf_mlp.predict_density(means.cuda().contiguous(), stds.cuda().contiguous())
    H.bracket(f"{name} raw density per sample", (raw32.double() - t["raw_density"]).abs(), (raw.cpu().double() - t["raw_density"]).abs(), K, min_ref=1e-4)
    H.bracket(f"{name} density per sample", (r32["density"].double() - t["density"]).abs(), (res["density"].cpu().double() - t["density"]).abs(), K,
              min_ref=1e-5)
    H.bracket(f"{name} rgb per sample", (r32["rgb"].double() - t["rgb"]).abs(), (res["rgb"].cpu().double() - t["rgb"]).abs(), K, min_ref=1e-5)
    _timed(f"test_fine_level_features_density_colour_bracket[{name}]", t0)


def test_field_golden_bracket():
    """field.npz (explicit Gaussians): the reference's OWN float32 values (the golden) are e_ref; features per level, raw
    density, bottleneck, density, colour -- the quantities test_field_vs_golden holds to 1e-3 / 3e-4 / 5e-3."""
    t0 = time.time()
    fx = H.load("field.npz")
    spec = rm.make_spec("tiny")
    sd = H.state_for(fx, spec)
    model, _ = H.hip_model(spec, sd)
    with torch.no_grad():
        t = t64.field_forward(spec.nerf, t64.state64(sd), fx["means"], fx["stds"], fx["viewdirs"])
        m, s, vd = fx["means"].cuda().contiguous(), fx["stds"].cuda().contiguous(), fx["viewdirs"].cuda().contiguous()
        res = model.nerf_mlp(False, m, s, viewdirs=vd)
        raw, x, _ = model.nerf_mlp.predict_density(m, s)
    # per level, through ucn_points_features (the explicit-Gaussian entry of the field module, not ucn_march_features)
    from ucnerf_amd import _lib
    lib = _lib.load()
    mlp = model.nerf_mlp
    L, C = mlp.encoder.num_levels, mlp.encoder.level_dim
    B, G = fx["means"].shape[0] * fx["means"].shape[1], fx["means"].shape[2]
    mm, ss = m.reshape(B * G, 3).contiguous(), s.reshape(B * G, 1).contiguous()
    feat = torch.full((L, B, C), float("nan"), device="cuda")
    coord = torch.empty(B, 3, device="cuda")
    desc = mlp.field(0)
    _lib.check(lib.ucn_points_features(ctypes.byref(desc), mm.data_ptr(), ss.data_ptr(), B, G, 1, 1, feat.data_ptr(), coord.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    got_f = feat.permute(1, 0, 2).double().cpu().reshape(fx["means"].shape[:2] + (L, C))
    want_f = fx["nerf_features"].double().reshape(got_f.shape)
    _, _, grid_sizes, _ = spec.nerf.layout()
    for l in range(L):
        H.bracket(f"field.npz nerf_features level {l} (side {int(grid_sizes[l])})", (want_f[:, :, l] - t["features"][:, :, l]).abs(),
                  (got_f[:, :, l] - t["features"][:, :, l]).abs(), K, min_ref=0.125 * U * int(grid_sizes[l]))     # (96 samples: the
        # largest of 96 position errors is smaller than the largest of the thousands the other brackets see; checked on the golden alone)
    for key, tk, got, floor_ref in (("nerf_raw_density", "raw_density", raw, 1e-4), ("nerf_bottleneck", "bottleneck", x, 1e-4),
                                    ("nerf_density", "density", res["density"], 1e-5), ("nerf_rgb", "rgb", res["rgb"], 1e-5)):
        H.bracket(f"field.npz {key}", (fx[key].double() - t[tk]).abs(), (got.cpu().double() - t[tk]).abs(), K, min_ref=floor_ref)
    _timed("test_field_golden_bracket", t0)


# --------------------------------------------------------------------------- table gradient of the featurisation, full size
SEEDS = (51, 61, 71)
N_GRAD = {"B": 256, "R": 1024}                 # rays: 32 768 samples each (128 / 32 per ray); the tables stay full size


def grad_case(grid, seed, sd):
    """Inputs of one table-gradient bracket on the NeRF field of a full-size state `sd` (bench.build_model's): training-pattern
    rays, fenceposts from the float32 oracle's own forward, a random upstream gradient [N*S, L, C]."""
    spec = rm.make_spec(grid)
    n = N_GRAD[grid]
    rays = rm.synthetic_rays(n, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    noise = [rm.draw_level_noise(spec, n, lvl, True, g) for lvl in range(2)]
    with torch.no_grad():
        _, hist = rm.model_forward(spec, sd, rays, noise, train_frac=0.5, compute_extras=False, training=True)
    sdist = hist[-1]["sdist"].reshape(n, -1).contiguous()
    fs = spec.nerf
    S = sdist.shape[1] - 1
    grad = torch.randn(n * S, fs.num_grid_levels, fs.grid_level_dim, generator=g)
    return spec, rays, noise[-1], sdist, grad


def grad_sides(spec, sd, rays, nz, sdist, grad):
    """float64 truth and the float32 oracle's autograd (oracle/grid_oracle.c's backward) of <grad, features> w.r.t. the table,
    plus the truth's no-flip mask of samples per level [N*S, L]."""
    fs = spec.nerf
    key = fs.prefix + ".encoder.embeddings"
    tdist = sdist * rays["far"] + (1 - sdist) * rays["near"]
    args = (rays["origins"], rays["directions"], rays["cam_dirs"], rays["radii"], nz.rand_vec, spec.std_scale, nz.flip, nz.spin)
    # float32 oracle
    emb = sd[key].clone().requires_grad_(True)
    state = dict(sd)
    state[key] = emb
    means, stds, _ = rm.cone_multisamples(tdist, *args)
    feat32 = rm.field_density_features(fs, state, means, stds)[3]
    (feat32.reshape(grad.shape[0], -1) * grad.reshape(grad.shape[0], -1)).sum().backward()
    # truth
    table = sd[key].double().requires_grad_(True)
    m, s, _ = t64.cone_multisamples(tdist, *args)
    feat, cm, cs = t64.sample_features(fs, table, m, s)
    (feat.reshape(grad.shape) * grad.double()).sum().backward()
    _, _, grid_sizes, _ = fs.layout()
    # no-flip subset: every coordinate of all six multisamples further than tau = DX * side cells from a cell face
    noflip = []
    pts01 = ((cm + 1) / 2).reshape(-1, 3)
    for l, _, _, p, _ in t64.grid_corners(fs, pts01):
        dist = (p - torch.round(p)).abs().reshape(grad.shape[0], 18).amin(dim=1)
        noflip.append(dist > DX * int(grid_sizes[l]))
    return table.grad, emb.grad.double(), torch.stack(noflip, dim=1)


def _per_level(g, offsets):
    return [g[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def _hip_table_gradient(model, rays, nz, sdist, grad, fixed_point):
    from ucnerf_amd import _lib
    lib = _lib.load()
    mlp = model.nerf_mlp
    n, S = sdist.shape[0], sdist.shape[1] - 1
    _, geom = _march_features(model, mlp, {k: rays[k] for k in ("near", "far", "origins", "directions", "cam_dirs", "radii")}, nz.rand_vec, sdist,
                              nz.flip, nz.spin)
    field = mlp.field()
    assert lib.ucn_march_features_backward_row_blocks(ctypes.byref(field), n, S) == 1        # row-block ownership, not the atomic scatter
    ws = torch.empty(lib.ucn_march_features_backward_ws_floats(ctypes.byref(field), n, S), device="cuda")
    gl = grad.permute(1, 0, 2).contiguous().cuda()                                            # layout 0: [L][N*S][C]
    gt = torch.zeros_like(mlp.encoder.embeddings.detach())
    _lib.check(lib.ucn_march_features_backward(ctypes.byref(field), *[_lib.ptr(t) for t in geom], float(model.std_scale), n, S, 0,
                                               _lib.BWD_FIXED_POINT if fixed_point else 0, gl.data_ptr(), gt.data_ptr(), ws.data_ptr(),
                                               _lib.stream()))
    torch.cuda.synchronize()
    return gt.double().cpu()


@pytest.mark.parametrize("fixed_point", [False, True], ids=["float_rows", "fixed_point_rows"])
@pytest.mark.parametrize("grid", ["B", "R"])
def test_table_gradient_bracket_full_size(grid, fixed_point):
    """ucn_march_features_backward at full table size with a random upstream gradient (the featurisation isolated from the MLP),
    per level:

      1. rel-L2 of HIP vs truth64 against rel-L2 of the float32 oracle's autograd vs truth64, k = 2 -- what _table_bar of
         test_train_full_size holds to 3e-2 / 1e-1;
      2. a POSITIVE upstream gradient: the 8 trilinear weights of a multisample sum to 1 wherever it lies, so a level's gradient
         sum is sum_s g_s mean_6 damping -- independent of the positions' last bits.  HIP's sum must equal the truth's to the
         damping's stated float32 error (3e-5 relative on its argument, 1.5e-7 on the erf: <= 2e-5 of the sum) plus float32
         summation over the fullest row (n_max addends: n_max u).  A corner weight scaled by 1 - 2^-6 moves the sum by
         2^-6 / 8 = 2e-3 of it;
      3. the no-flip subset (first seed): the upstream gradient zeroed outside the samples whose six multisamples all lie further
         than tau = DX * side from every cell face (no float32 evaluation within DX of the truth's positions can be in another
         cell).  There (a) the L1 distance to the truth over the level's rows is within the derived
         sum_s |g_s| (8 u side + 32 u + 2e-5 + n_max u), and (b) it is within 2 x the float32 oracle's own L1 distance on the same
         masked gradient.  (b) is the clause that sees weight MOVED between corners: a corner scaled by 1 - 2^-6 adds 2e-3 of
         sum|g|, the oracle's distance is 1e-6 (side 129) ... 4e-4 (side 8193).  Levels 0-9 only (see LIMIT below)."""
    import bench
    t0 = time.time()
    model, _, sd = bench.build_model(torch.device("cuda", 0), grid=grid)
    fs = rm.make_spec(grid).nerf
    _, offsets, grid_sizes, _ = fs.layout()
    off = [int(o) for o in offsets]
    tag = f"table gradient {grid} {'fixed-point' if fixed_point else 'float'} rows"
    host_s, failures = 0.0, []
    # 1. the bracket per level, three seeds (rays, draws, fenceposts, upstream gradient)
    cases = {}
    for seed in SEEDS:
        t1 = time.time()
        cases[seed] = grad_case(grid, seed, sd)
        spec, rays, nz, sdist, grad = cases[seed]
        g_truth, g_ref, noflip = grad_sides(spec, sd, rays, nz, sdist, grad)
        cases[seed] += (noflip,)
        host_s += time.time() - t1
        g_hip = _hip_table_gradient(model, rays, nz, sdist, grad, fixed_point)
        for l, (a, b, c) in enumerate(zip(_per_level(g_hip, off), _per_level(g_ref, off), _per_level(g_truth, off))):
            e_ref, e_hip = float((b - c).norm() / c.norm()), float((a - c).norm() / c.norm())
            k = max(K, 1.5 * RATIO_FIXED_POINT[grid][l]) if fixed_point else K
            try:        # one number per level: the "mean" clause coincides with the "max" one; every level is reported before any fails
                H.bracket(f"{tag} seed {seed} level {l} (side {int(grid_sizes[l])}) rel L2", [e_ref], [e_hip], k, floor=(1e-6, 1e-6),
                          min_ref=0.25 * U * int(grid_sizes[l]))
            except AssertionError as e:
                failures.append(str(e)[:200])
    assert not failures, failures
    # Parts 2 and 3 run on ONE case, the first seed's.
    spec, rays, nz, sdist, grad, noflip = cases[SEEDS[0]]
    key = fs.prefix + ".encoder.embeddings"
    tdist = sdist * rays["far"] + (1 - sdist) * rays["near"]
    cast = (rays["origins"], rays["directions"], rays["cam_dirs"], rays["radii"], nz.rand_vec, spec.std_scale, nz.flip, nz.spin)
    m, s, _ = t64.cone_multisamples(tdist, *cast)

    def truth_gradient(g):
        table = sd[key].double().requires_grad_(True)
        f, cmean, _ = t64.sample_features(fs, table, m, s)
        (f.reshape(g.shape) * g.double()).sum().backward()
        return table.grad, cmean

    # 2. positive upstream gradient: the level sums
    t1 = time.time()
    gpos = grad.abs()
    g_truth, cmean = truth_gradient(gpos)
    rows_max = [int(torch.bincount(rows.reshape(-1) - off[l]).max()) for l, rows, _, _, _ in t64.grid_corners(fs, ((cmean + 1) / 2).reshape(-1, 3))]
    host_s += time.time() - t1
    g_hip = _hip_table_gradient(model, rays, nz, sdist, gpos, fixed_point)
    for l, (a, c) in enumerate(zip(_per_level(g_hip, off), _per_level(g_truth, off))):
        sa, sc = float(a.sum()), float(c.sum())
        bound = (2e-5 + rows_max[l] * U) * sc
        print(f"BRACKET {tag} level {l} sum (positive upstream gradient): truth {sc:.9e} hip {sa:.9e} rel {abs(sa - sc) / sc:.3e} "
              f"(bound {bound / sc:.3e}, fullest row {rows_max[l]} addends)")
        assert float(a.min()) >= 0.0 and abs(float(a.abs().sum()) - sa) <= 1e-9 * sa, l
        assert abs(sa - sc) <= bound, (l, sa, sc, bound)
    # 3. the no-flip subset
    t1 = time.time()
    share = noflip.double().mean(dim=0)
    taken = [l for l in range(len(off) - 1) if float(share[l]) >= 0.5]
    hashed = [l for l in taken if int(grid_sizes[l]) ** 3 > off[l + 1] - off[l]]
    print(f"BRACKET {tag} no-flip share per level: " + " ".join(f"{float(x):.3f}" for x in share) + f"; taken {taken}, hashed among them {hashed}")
    # LIMIT: tau grows with the side, a sample has 18 coordinates: from side 16 385 on fewer than half of the samples are provably
    # flip-free and those levels (the six finest of config B) are NOT in this part; they have parts 1 and 2 only.
    assert taken == list(range(10)) and hashed == list(range(3, 10)), (taken, hashed)
    gsub = grad * noflip[:, :, None].float()
    g_truth, _ = truth_gradient(gsub)
    emb = sd[key].clone().requires_grad_(True)                        # the float32 oracle on the same masked gradient
    state = dict(sd)
    state[key] = emb
    m32, s32, _ = rm.cone_multisamples(tdist, *cast)
    (rm.field_density_features(fs, state, m32, s32)[3].reshape(grad.shape[0], -1) * gsub.reshape(grad.shape[0], -1)).sum().backward()
    g_ref = emb.grad.double()
    host_s += time.time() - t1
    g_hip = _hip_table_gradient(model, rays, nz, sdist, gsub, fixed_point)
    n_addends = grad.shape[0] * 48
    for l in taken:
        a, b, c = (_per_level(g, off)[l] for g in (g_hip, g_ref, g_truth))
        l1, l1_ref = float((a - c).abs().sum()), float((b - c).abs().sum())
        gsum = float(gsub[:, l].abs().sum())
        side = int(grid_sizes[l])
        # (a) derived: 8 corners x ulp x resolution x |g|, + 4 u of rounding per weight, the damping (2e-5), float32 summation over the
        # fullest row; fixed-point rows: + every addend rounded to <= 2^-29 of its task's summed |g| (<= the level's), +- half of it
        bound = gsum * (8 * U * side + 32 * U + 2e-5 + rows_max[l] * U + (n_addends * 2.0 ** -30 if fixed_point else 0.0))
        print(f"BRACKET {tag} level {l} no-flip subset: L1 / sum|g|: oracle {l1_ref / gsum:.3e} hip {l1 / gsum:.3e} ratio {l1 / max(l1_ref, 1e-300):.3f} "
              f"(derived bound {bound / gsum:.3e}, tau {DX * side:.2e} cell)")
        assert l1 <= bound, (l, l1, bound)
        # (b) no cell flip is possible in either float32 evaluation here, so the float32 oracle's own L1 distance is the yardstick:
        # k = 2, floor = float32 summation in another order.  (Fixed-point rows: their quantisation floor is the deliberate trade
        # bracketed per level in part 1; reported here, not asserted twice.)
        if not fixed_point:
            assert l1 <= K * l1_ref + rows_max[l] ** 0.5 * U * gsum, (l, l1, l1_ref)
    print(f"BRACKET-TIME test_table_gradient_bracket_full_size[{grid}-{'fixed' if fixed_point else 'float'}]: {host_s:.1f} s of host work "
          f"(truth64 x 5, float32 oracle x 4), {time.time() - t0:.1f} s in all")


# ---------------------------------------------------------------------------------------- pixels at full table size, config B
def _power32(s, near, far, lam=-1.5):
    """coord.py:137-177 for the power curve, float32 throughout (the float32 side of the bracket; oracle/raymarch.py has no curves)"""
    lam_1 = abs(lam - 1)
    fwd = lambda x: lam_1 / lam * ((2 * x / lam_1 + 1) ** lam - 1)
    inv = lambda y: ((y * lam / lam_1 + 1 + rm.EPS) ** (1 / lam) - 1) * lam_1 / 2
    return inv(s * fwd(far) + (1 - s) * fwd(near))


def pixel_sides(spec, sd, rays, noise, sdists, curve):
    """The NeRF level's pixels at the given fenceposts: truth64 and the float32 oracle's formulation."""
    fs, nz, sdist = spec.nerf, noise[-1], sdists[-1]
    with torch.no_grad():
        truth, _ = t64.level_forward(spec, fs, t64.state64(sd), rays, sdist, nz, curve)
        tdist = sdist * rays["far"] + (1 - sdist) * rays["near"] if curve is None else _power32(sdist, rays["near"], rays["far"])
        means, stds, _ = rm.cone_multisamples(tdist, rays["origins"], rays["directions"], rays["cam_dirs"], rays["radii"], nz.rand_vec,
                                              spec.std_scale, nz.flip, nz.spin)
        res = rm.field_forward(fs, sd, means, stds, rays["viewdirs"])
        w = rm.alpha_weights(res["density"], tdist, rays["directions"], spec.opaque_background)
        ref = rm.composite(res["rgb"], w, tdist, spec.bg_intensity, rays["far"], True)
    return truth, ref


def pixel_case(sd, n=256, seed=81):
    spec = rm.make_spec("B")
    rays = rm.synthetic_rays(n, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    noise = [rm.draw_level_noise(spec, n, lvl, True, g) for lvl in range(2)]
    with torch.no_grad():                                              # fenceposts are an input: the identity curve's, for both curves
        _, hist = rm.model_forward(spec, sd, rays, noise, train_frac=0.5, compute_extras=False, training=True)
    return spec, rays, noise, [h["sdist"].reshape(n, -1).contiguous() for h in hist]


@pytest.mark.parametrize("curve", [None, "power_transformation"])
def test_pixels_bracket_config_B_full_tables(curve):
    """rgb, acc, depth (away from the acc = 0.6 sentinel switch) and median distance of the NeRF level at pinned fenceposts and pinned
    draws, through Model.forward on the training route (the route that accepts pinned fenceposts), split and exact dense engines.
    Distances are bracketed relative to far = 8 (the floors are those of O(1) quantities)."""
    import contextlib
    import bench
    from ucnerf_amd.internal import dense_f32 as D
    from ucnerf_amd.internal import models
    t0 = time.time()
    ctx = models.bindings(Model=dict(raydist_fn=curve)) if curve else contextlib.nullcontext()
    with ctx:
        model, _, sd = bench.build_model(torch.device("cuda", 0))
    assert (model._raydist_curve != 0) == (curve is not None)
    spec, rays, noise, sdists = pixel_case(sd)
    truth, ref = pixel_sides(spec, sd, rays, noise, sdists, curve)
    host_s = time.time() - t0
    n = sdists[0].shape[0]
    batch = {k: v[:, None, None, :].cuda() for k, v in rays.items()}
    batch = H.pin_noise(batch, noise)
    for lvl, sdist in enumerate(sdists):
        batch["march_noise"][lvl]["sdist"] = sdist.cuda()
    batch["rand_vec"] = batch["rand_vec"][:, None, None, :]
    model.train()
    stable = (truth["acc"] - 0.6).abs() > 1e-3
    far = float(rays["far"].max())
    for engine in ("split", "exact"):
        prev = D.set_engine(engine)
        try:
            rend, hist = model(True, batch, 0.5, True, zero_glo=False)
        finally:
            D.set_engine(prev)
        torch.cuda.synchronize()
        assert float((hist[-1]["sdist"].reshape(n, -1).cpu() - sdists[-1]).abs().max()) == 0.0       # the pinned fenceposts were used
        got = {k: rend[-1][k].detach().double().cpu().reshape(n, -1).squeeze(-1) for k in ("rgb", "acc", "depth", "distance_median")}
        tag = f"pixels B {curve or 'identity'} {engine}"
        H.bracket(f"{tag} rgb", (ref["rgb"].double() - truth["rgb"]).abs(), (got["rgb"] - truth["rgb"]).abs(), K, min_ref=1e-6)
        H.bracket(f"{tag} acc", (ref["acc"].double() - truth["acc"]).abs(), (got["acc"] - truth["acc"]).abs(), K, min_ref=1e-7)
        assert int(stable.sum()) >= n // 2
        assert torch.equal((got["depth"] == 300)[stable], (truth["depth"] == 300)[stable])
        H.bracket(f"{tag} depth / far", (ref["depth"].double() - truth["depth"]).abs()[stable] / far,
                  (got["depth"] - truth["depth"]).abs()[stable] / far, K, min_ref=1e-7)
        H.bracket(f"{tag} distance_median / far", (ref["distance_median"].double() - truth["distance_median"]).abs() / far,
                  (got["distance_median"] - truth["distance_median"]).abs() / far, K, min_ref=1e-7)
    print(f"BRACKET-TIME test_pixels_bracket_config_B_full_tables[{curve}]: {host_s:.1f} s of host work, {time.time() - t0:.1f} s in all")


# --------------------------------------------------------------------- table gradient through the whole float32 training step
def truth_step(spec, sd, rays, target, noise, sdists):
    """The step of test_train_full_size.oracle_step in float64 at the oracle's fenceposts: both levels through truth64, the oracle's
    own losses (dtype-generic), autograd.  Returns the two table gradients."""
    from test_train_full_size import _oracle_losses
    s64 = t64.state64(sd)
    keys = [fs.prefix + ".encoder.embeddings" for fs in (spec.props[0], spec.nerf)]
    for k in keys:
        s64[k] = s64[k].clone().requires_grad_(True)
    rend, hist = [], []
    for lvl in range(spec.num_levels):
        fs = spec.field_for_level(lvl)
        r, res = t64.level_forward(spec, fs, s64, rays, sdists[lvl], noise[lvl])
        emb = s64[fs.prefix + ".encoder.embeddings"]
        _, offsets, _, _ = fs.layout()
        decay = torch.stack([(emb[offsets[i]:offsets[i + 1]] ** 2).mean(dim=0) for i in range(fs.num_grid_levels)]).mean()
        rend.append(dict(rgb=r["rgb"][:, None, None], weights=r["weights"][:, None, None]))
        hist.append(dict(sdist=t64.f64(sdists[lvl])[:, None, None], weights=r["weights"][:, None, None], loss_hash_decay=decay))
    batch = {k: t64.f64(v)[:, None, None, :] for k, v in rays.items() if v.is_floating_point()}
    batch["rgb"] = t64.f64(target)[:, None, None, :]
    sum(_oracle_losses(batch, rend, hist).values()).backward()
    return {k: s64[k].grad for k in keys}


def test_training_step_table_gradient_bracket_config_B():
    """The whole float32 training step of test_train_full_size (hip_step: forward, the reference's losses, the hand-written backward
    through heads and featurisation) at the oracle's fenceposts, split and exact engines: per level of both tables, rel-L2 of HIP vs
    truth64 against rel-L2 of the float32 oracle's autograd vs truth64 (k = 2), and the level's sum and sum|.| against the truth's
    to float32 summation error (the float32 oracle's own deviation of the same statistic, x 2, + n u of the level's sum|.| for the
    n rays x samples x 48 addends spread over its rows -- taken as sqrt(n) u)."""
    import test_train_full_size as T
    from ucnerf_amd.internal import dense_f32 as D
    t0 = time.time()
    model, spec, sd, rays, target, noise = T._case("B")
    _, want_g = T.oracle_step(spec, sd, rays, target, noise, 0.5)
    sdists = T.oracle_step.sdist
    truth_g = truth_step(spec, sd, rays, target, noise, sdists)
    host_s = time.time() - t0
    failures = []
    for engine in ("split", "exact"):
        prev = D.set_engine(engine)
        try:
            _, got_g = T.hip_step(model, rays, target, noise, 0.5, bf16=False, sdist=sdists)
        finally:
            D.set_engine(prev)
        for fs in (spec.props[0], spec.nerf):
            key = fs.prefix + ".encoder.embeddings"
            _, offsets, grid_sizes, _ = fs.layout()
            off = [int(o) for o in offsets]
            n_add = T.N_RAYS * (spec.num_prop_samples if fs is spec.props[0] else spec.num_nerf_samples) * 48
            for l, (a, b, c) in enumerate(zip(_per_level(got_g[key].double(), off), _per_level(want_g[key].double(), off), _per_level(truth_g[key], off))):
                e_ref, e_hip = float((b - c).norm() / c.norm()), float((a - c).norm() / c.norm())
                tag = f"training step B {engine} {key} level {l} (side {int(grid_sizes[l])})"
                try:
                    # the NeRF grid's float32 reference is off by 0.3 - 3.5 % on EVERY level here (the hidden state of the heads moves with
                    # the finest features): the scale of _table_bar; the proposal grid's by 1e-7 (no such level), no min_ref there
                    H.bracket(f"{tag} rel L2", [e_ref], [e_hip], K, floor=(1e-6, 1e-6), min_ref=1e-3 if fs is spec.nerf else None)
                except AssertionError as e:
                    failures.append(str(e)[:160])
                sabs = float(c.abs().sum())
                for name, fn in (("sum", lambda g: float(g.sum())), ("sum|.|", lambda g: float(g.abs().sum()))):
                    d_ref, d_hip = abs(fn(b) - fn(c)) / sabs, abs(fn(a) - fn(c)) / sabs
                    print(f"BRACKET {tag} {name} / sum|g|: oracle off by {d_ref:.3e}, hip off by {d_hip:.3e}")
                    if d_hip > K * d_ref + n_add ** 0.5 * U:
                        failures.append(f"{tag} {name}: {d_hip:.3e} vs {d_ref:.3e}")
    print(f"BRACKET-TIME test_training_step_table_gradient_bracket_config_B: {host_s:.1f} s of host work, {time.time() - t0:.1f} s in all")
    assert not failures, failures
