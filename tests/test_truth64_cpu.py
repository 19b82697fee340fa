"""oracle/truth64.py held to account on the CPU, so that a wrong truth cannot bless a wrong kernel:

  * the committed float32 goldens of the reference (field / cast / composite / model_tiny / raydist_*) lie within DERIVED
    float32 bounds of truth64 where such a bound exists -- compositing: S-term sums; the proposal grid (resolution <= 512):
    position error times resolution -- and the measured distance is printed for every key (run with -s);
  * truth64's autograd table gradient equals oracle/grid_numpy.py's float64-accumulated backward_table on the same addends;
  * truth64 is linear in the table and reproduces the closed form on a table of ones.

u = 2^-24 is the float32 unit roundoff throughout."""
import numpy as np
import pytest
import torch

import helpers as H
from oracle import grid_numpy as gn
from oracle import raymarch as rm
from oracle import truth64 as t64
from test_raydist_cpu import CURVE_FILES

U = 2.0 ** -24


def _show(tag, got, want):
    d = (torch.as_tensor(want).double() - got).abs()
    d = d[torch.isfinite(d)]
    print(f"TRUTH64 {tag}: |golden fp32 - truth64| max {float(d.max()):.3e} mean {float(d.mean()):.3e}")
    return d


def _feature_bound(fs, table_range=1.0):
    """Per-level bound on |fp32 feature - truth| for a table in [-range, range]: the contracted, halved, shifted coordinate
    x = (z / 2 + 1) / 2 in [0, 1] carries at most 10 u of absolute error (3 squares + 2 adds, sqrt, 2 root - 1 with root >= 1,
    the division, the product with the mean: <= 8 u relative on |z| / 4 <= 1/2, plus the two roundings of the shift), a level
    scales it by its resolution, the trilinear interpolant moves by at most 2 range per cell along each of 3 axes; the 8-term
    fp32 interpolation (weights: 3 products, one fma each) adds <= 16 u range; the erf damping is <= 1 and its own float32
    error (<= 4 u relative, the std chain included, as the argument's sensitivity x erf'(x) / erf(x) <= 1) is folded into
    the 16 u; the mean of six averages errors."""
    _, _, grid_sizes, _ = fs.layout()
    return torch.as_tensor(grid_sizes).double() * (3 * 2 * table_range * 10 * U) + 16 * U * table_range


def test_field_golden_vs_truth64():
    fx = H.load("field.npz")
    spec = rm.make_spec("tiny")
    sd = H.state_for(fx, spec)
    s64 = t64.state64(sd)
    for name, fs in (("nerf", spec.nerf), ("prop", spec.props[0])):
        with torch.no_grad():
            r = t64.field_forward(fs, s64, fx["means"], fx["stds"], fx["viewdirs"])
        L, C = fs.num_grid_levels, fs.grid_level_dim
        for k in ("raw_density", "density", "rgb", "bottleneck", "coord"):
            if r[k] is not None:
                _show(f"field.npz {name}_{k}", r[k], fx[f"{name}_{k}"])
        want = fx[f"{name}_features"].double().reshape(fx["means"].shape[:2] + (L, C))
        bound = _feature_bound(fs)
        _, _, grid_sizes, _ = fs.layout()
        for l in range(L):
            d = _show(f"field.npz {name}_features level {l} (side {int(grid_sizes[l])}, bound {float(bound[l]):.2e})",
                      r["features"][..., l, :], want[..., l, :])
            if int(grid_sizes[l]) <= 513:                      # the derived bound is only meaningful while it is << the feature
                assert float(d.max()) <= float(bound[l]), (name, l, float(d.max()), float(bound[l]))
        if name == "prop":
            # through the density MLP: |d raw| <= |w2|^T |W0| d feat  +  the float32 MLP's own rounding (n + 2) u sum |w| |h|
            W0, W2 = (s64[f"{fs.prefix}.density_layer.{i}.weight"].abs() for i in (0, 2))
            lip = (W2 @ W0)[0].reshape(L, C).sum(dim=1)                                     # per level, both channels
            mlp = (L * C + 2) * U * float((W2 @ (W0.sum(dim=1) + 1)).max()) + 66 * U * float(W2.sum() + 1)
            b = float((lip * bound).sum()) + mlp
            d = (fx["prop_raw_density"].double() - r["raw_density"]).abs()
            print(f"TRUTH64 field.npz prop_raw_density derived bound {b:.3e}")
            assert float(d.max()) <= b
            assert float((fx["prop_density"].double() - r["density"]).abs().max()) <= b + 4 * U * float(r["density"].max())
    # the float32 reference really is off the truth at the fine levels, and the truth is not the golden in disguise
    d = (fx["nerf_features"].double().reshape(6, 16, 16, 2) - t64.field_forward(
        spec.nerf, s64, fx["means"], fx["stds"], fx["viewdirs"])["features"].detach()).abs()
    assert float(d[:, :, 15].max()) >= 1e-4 and float(d[:, :, 0].max()) <= 4e-6
    # no contraction: the one rounding of (mean + 1) / 2 (<= u of the unit cube = 0.03 cell at the finest level) is all the
    # position error float32 has left, and it is enough for 1e-4-class differences in the raw density: printed, not bounded
    with torch.no_grad():
        r = t64.field_forward(spec.nerf, s64, fx["nowarp_means"], fx["nowarp_stds"], no_warp=True)
    _show("field.npz nowarp_raw_density", r["raw_density"], fx["nowarp_raw_density"])


@pytest.mark.parametrize("name", ["cast.npz", "raydist_cast.npz"])
def test_cast_golden_vs_truth64(name):
    fx = H.load(name)
    far = float(fx["tdist"].max())
    for tag, kw in (("eval", {}), ("train", dict(flip=fx["train_flip"], spin=fx["train_spin"]))):
        m, s, t = t64.cone_multisamples(fx["tdist"], fx["origins"], fx["directions"], fx["cam_dirs"], fx["radii"],
                                        fx[f"{tag}_rand_vec"], 0.5, **kw)
        ok = torch.isfinite(fx[f"{tag}_stds"])                 # the reference's NaN for a zero-width interval at t = 0
        okm = ok[..., None].expand(m.shape)
        # a mean is o + t d + offsets: <= 2 ulp of its magnitude per rounding of t (the t formula: ~8 roundings of
        # O(t) quantities, no cancellation) and of the 3-term sum; per element, against the element's own scale
        scale_m = (fx["origins"].double().abs()[:, None, None, :] + t[..., None] * fx["directions"].double().abs()[:, None, None, :]
                   + 1e-3 * t[..., None])
        dm = ((fx[f"{tag}_means"].double() - m).abs() / scale_m)[okm]
        dt = ((fx[f"{tag}_t"].double() - t).abs() / t.abs().clamp_min(1e-30))[ok]
        ds = ((fx[f"{tag}_stds"].double() - s).abs() / s.abs().clamp_min(1e-30))[ok]
        print(f"TRUTH64 {name} {tag} (t up to {far:.3g}): rel |d means| max {float(dm.max()):.3e}  rel |d t| max {float(dt.max()):.3e}"
              f"  rel |d stds| max {float(ds.max()):.3e}  abs |d means| max {float((fx[f'{tag}_means'].double() - m).abs()[okm].max()):.3e}")
        assert float(dt.max()) <= 16 * U and float(ds.max()) <= 20 * U and float(dm.max()) <= 24 * U
    if "contract_in_mean" in fx:
        z, s = t64.contract_points(fx["contract_in_mean"], fx["contract_in_std"])
        d = _show(f"{name} contract_mean", z, fx["contract_mean"])
        assert float(d.max()) <= 8 * U * 2                     # |z| <= 2, <= 8 u relative (see _feature_bound)
        rel = (s - fx["contract_std"].double()).abs() / s.abs().clamp_min(1e-30)
        print(f"TRUTH64 {name} contract_std: rel max {float(rel.max()):.3e}")
        assert float(rel.max()) <= 32 * U                      # pow(., 1/3) (<= 2 ulp), square, the quotient, 8 u of the norm


def test_composite_golden_vs_truth64():
    """S-term sums: tau = density * delta carries <= 8 u relative (difference of two inputs, the norm of the direction, the
    product); the transmittance exp(-cumsum tau) a relative error <= (S + 8) u cumsum tau + 2 u whatever the order of the
    cumulative sum; alpha = 1 - exp(-tau) an ABSOLUTE error <= 2 u + 8 u tau."""
    fx = H.load("composite.npz")
    S = fx["density"].shape[1]
    w = t64.alpha_weights(fx["density"], fx["tdist"], fx["dirs"])
    tdist, dens = fx["tdist"].double(), fx["density"].double()
    tau = dens * (tdist[:, 1:] - tdist[:, :-1]) * fx["dirs"].double().norm(dim=-1, keepdim=True)
    cum = torch.cat([torch.zeros_like(tau[:, :1]), torch.cumsum(tau[:, :-1], dim=-1)], dim=-1)
    trans = torch.exp(-cum)
    alpha = 1 - torch.exp(-tau)
    bw = alpha * trans * ((S + 8) * U * cum + 2 * U) + trans * (2 * U + 8 * U * tau) + U * w + 2.0 ** -126       # + the product's rounding, + float32 underflow
    d = _show("composite.npz weights", w, fx["weights"])
    assert bool(((fx["weights"].double() - w).abs() <= bw).all()), float(((fx["weights"].double() - w).abs() / bw).max())
    wo = t64.alpha_weights(fx["density"], fx["tdist"], fx["dirs"], True)
    _show("composite.npz weights_opaque", wo, fx["weights_opaque"])
    assert bool(((fx["weights_opaque"].double() - wo).abs()[:, :-1] <= bw[:, :-1]).all())
    assert bool(((fx["weights_opaque"].double() - wo).abs()[:, -1] <= trans[:, -1] * ((S + 8) * U * cum[:, -1] + 4 * U) + 2.0 ** -126).all())      # alpha = 1
    out = t64.composite(fx["rgbs"], w, fx["tdist"], 1.0, fx["far"])
    b_acc = bw.sum(dim=-1) + (S + 1) * U * w.sum(dim=-1)
    c = fx["rgbs"].double().abs()
    b_rgb = (bw[..., None] * c).sum(dim=-2) + (S + 3) * U * (w[..., None] * c).sum(dim=-2) + b_acc[:, None] + 2 * U
    t_mid = 0.5 * (tdist[:, :-1] + tdist[:, 1:])
    acc = out["acc"]
    num = (w * t_mid).sum(dim=-1)
    b_depth = ((bw * t_mid).sum(dim=-1) + (S + 3) * U * num) / acc.clamp_min(1e-30) + out["depth"] * (b_acc / acc.clamp_min(1e-30) + 2 * U)
    for k, b in (("acc", b_acc), ("rgb", b_rgb), ("depth", b_depth)):
        d = (fx["out_" + k].double() - out[k]).abs()
        live = torch.ones_like(d, dtype=torch.bool)
        if k == "depth":
            live = (out["depth"] != 300) & (fx["out_depth"] != 300) & ((acc - 0.6).abs() > 1e-4)
            assert int(live.sum()) >= 10
        print(f"TRUTH64 composite.npz out_{k}: max {float(d[live].max()):.3e} mean {float(d[live].mean()):.3e}; worst share of its derived bound "
              f"{float((d / b)[live].max()):.3f}")
        assert bool((d[live] <= b[live]).all()), (k, float((d / b)[live].max()))
    for k in ("distance_mean", "distance_percentile_5", "distance_median", "distance_percentile_95"):
        d = _show("composite.npz out_" + k, out[k], fx["out_" + k])      # 1 / (cdf slope) amplification: no a-priori bound;
        assert float(d.max()) <= 2e-4, k                                 # the bar test_composite_vs_golden holds HIP to


def _levels_vs_truth(fx, spec, sd, raydist=None, lam=-1.5):
    """every level of a model fixture at the GOLDEN's own fenceposts (hist_sdist): truth64 against the stored float32 values"""
    s64 = t64.state64(sd)
    batch, noise = H.batch_of(fx), H.noise_of(fx, spec.num_levels)
    out = {}
    for lvl in range(spec.num_levels):
        sdist = fx[f"L{lvl}_hist_sdist"].reshape(batch["near"].shape[0], -1)
        with torch.no_grad():
            rend, res = t64.level_forward(spec, spec.field_for_level(lvl), s64, batch, sdist, noise[lvl], raydist, lam)
        out[lvl] = (rend, res)
    return out


def _model_keys(tag, fx, lv, num_levels):
    worst = {}
    for lvl in range(num_levels):
        rend, res = lv[lvl]
        g = lambda k: fx[f"L{lvl}_{k}"].double()
        pairs = [("hist_density", res["density"]), ("hist_coord", res["coord"]), ("weights", rend["weights"]), ("rgb", rend["rgb"]),
                 ("acc", rend["acc"]), ("distance_median", rend["distance_median"]), ("distance_mean", rend["distance_mean"])]
        if res["rgb"] is not None:
            pairs.append(("hist_rgb", res["rgb"]))
        for k, v in pairs:
            worst[(lvl, k)] = float(_show(f"{tag} L{lvl}_{k}", v, g(k).reshape(v.shape)).max())
        stable = ((g("acc").reshape(-1) - 0.6).abs() > 1e-3)
        worst[(lvl, "depth")] = float(_show(f"{tag} L{lvl}_depth (away from the 0.6 switch)", rend["depth"][stable], g("depth").reshape(-1)[stable]).max())
    return worst


def test_model_tiny_golden_vs_truth64():
    fx = H.load("model_tiny.npz")
    spec = rm.make_spec("tiny")
    sd = H.state_for(fx, spec)
    worst = _model_keys("model_tiny.npz", fx, _levels_vs_truth(fx, spec, sd), spec.num_levels)
    # level 0 = the proposal grid (resolution <= 512): position error times resolution, through the density MLP's
    # absolute weights (softplus' <= 1); the same derivation as test_field_golden_vs_truth64
    fs = spec.props[0]
    s64 = t64.state64(sd)
    L, C = fs.num_grid_levels, fs.grid_level_dim
    W0, W2 = (s64[f"{fs.prefix}.density_layer.{i}.weight"].abs() for i in (0, 2))
    b = float(((W2 @ W0)[0].reshape(L, C).sum(dim=1) * _feature_bound(fs)).sum()) + (L * C + 68) * U * float((W2 @ (W0.sum(dim=1) + 1)).max() + 1)
    print(f"TRUTH64 model_tiny.npz L0_hist_density derived bound {b:.3e}")
    assert worst[(0, "hist_density")] <= b
    assert worst[(0, "hist_coord")] <= 16 * U                            # a contracted coordinate / 2, |.| <= 1
    assert worst[(1, "hist_density")] >= 1e-4                            # the fine level: float32 is measurably off the truth
    assert worst[(1, "rgb")] <= H.RGB_TOL                                # ... per sample, while its pixels are within the north-star bar


@pytest.mark.parametrize("name", CURVE_FILES)
def test_raydist_golden_vs_truth64(name):
    fx = H.load(name)
    curve = bytes(fx["raydist"].numpy()).decode().replace("torch.", "")
    lam = float(fx["power_lambda"]) if "power_lambda" in fx else -1.5
    s, near, far = fx["curve_s"], fx["curve_near"], fx["curve_far"]
    t = t64.s_to_t(curve, s, near, far, lam)
    _show(f"{name} curve_t_f32", t, fx["curve_t_f32"])
    _show(f"{name} curve_t_f64", t, fx["curve_t_f64"])
    # the float32 curve: the bound test_raydist_cpu derives (8 ulp of t [+ lam_1 / 2 for the power inverse] + the inverse's
    # slope times the rounding of its argument)
    h = 1e-7
    sp, sm = (s.double() + h).clamp(0, 1), (s.double() - h).clamp(0, 1)
    slope = (t64.s_to_t(curve, sp, near, far, lam) - t64.s_to_t(curve, sm, near, far, lam)).abs() / (sp - sm).clamp_min(1e-300)
    base = t.abs() + (1.25 if curve == "power_transformation" else 0.0)
    bound = 8 * torch.from_numpy(np.spacing(base.numpy().astype(np.float32)).astype(np.float64)) + 4 * slope * U * s.double().clamp_min(1e-3)
    d32 = (fx["curve_t_f32"].double() - t).abs()
    assert bool((d32 <= bound).all()), float((d32 / bound).max())
    if curve != "power_transformation":                                  # (the reference's float64 run adds 2^-52, not the float32 eps)
        assert float(((fx["curve_t_f64"].double() - t).abs() / t.abs().clamp_min(1e-30)).max()) <= 1e-12
    spec = rm.make_spec("tiny")
    sd = H.state_for(fx, spec)
    worst = _model_keys(name, fx, _levels_vs_truth(fx, spec, sd, curve, lam), spec.num_levels)
    assert worst[(0, "hist_coord")] <= 16 * U
    assert worst[(1, "rgb")] <= H.RGB_TOL


# ---------------------------------------------------------------------------------------------------- the table gradient
def _points(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, generator=g)


@pytest.mark.parametrize("kind", ["tiny", "tinyR"])
def test_autograd_table_gradient_equals_grid_numpy_on_the_same_addends(kind):
    """grid_numpy.backward_table accumulates float32-rounded addends fl(w32 * g) in float64; with addends that float32 holds
    EXACTLY (coordinates k / 2^10 on levels whose scale is an integer... are rare), the two can only be compared through their
    own arithmetic: so the comparison is made where both are exact -- the float64 sum of truth64's own addends
    w64 * g scattered with numpy's add.at -- and grid_numpy's float32 weights are held to 4 u relative beside it."""
    fs = rm.make_spec(kind).nerf
    pls, offsets, _, _ = fs.layout()
    off = np.asarray(offsets)
    n_rows = int(off[-1])
    L, C = fs.num_grid_levels, fs.grid_level_dim
    x = _points(3000, 5)
    g = torch.randn(3000, L, C, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    table = torch.zeros(n_rows, C, dtype=torch.float64, requires_grad=True)
    (t64.grid_features(fs, table, x) * g).sum().backward()
    # (a) the same addends, accumulated by numpy in float64
    want = np.zeros((n_rows, C))
    for l, rows, w, _, _ in t64.grid_corners(fs, x):
        np.add.at(want, rows.numpy().reshape(-1), (w[..., None] * g[:, l, None, :]).numpy().reshape(-1, C))
    err = float((table.grad - torch.from_numpy(want)).abs().max())
    scale = float(torch.from_numpy(want).abs().max())
    print(f"TRUTH64 table gradient ({kind}): autograd vs float64 add.at of the same addends: {err:.3e} (scale {scale:.3e})")
    assert err <= 1e-13 * scale and scale > 0.1
    # (b) grid_numpy's backward_table: float32 position / weight arithmetic, float64 accumulation -- the same ROWS, weights to
    # float32 rounding: p = fma(x, scale, .5) (u p, p up to the level's side), fraction, 3 products, one product with g
    gn_g = gn.backward_table(g.permute(1, 0, 2).float().numpy(), x.numpy(), off, float(np.log2(pls)), fs.grid_base_resolution, n_rows)
    _, _, grid_sizes, _ = fs.layout()
    for l in range(L):
        a, b = table.grad[off[l]:off[l + 1]], torch.from_numpy(gn_g[off[l]:off[l + 1]])
        assert torch.equal(a.abs().sum(dim=1) > 0, b.abs().sum(dim=1) > 0) or int(grid_sizes[l]) > 4096, l       # the same rows are touched
        rel = float((a - b).norm() / a.norm())
        bound = 4 * U * int(grid_sizes[l]) + 8 * U                         # u * side: the position's rounding in cell units
        print(f"  level {l} side {int(grid_sizes[l])}: rel L2 vs grid_numpy {rel:.3e} (bound {bound:.2e})")
        assert rel <= bound, (l, rel, bound)
        assert abs(float(a.sum()) - float(b.sum())) <= 8 * U * float(a.abs().sum()), l


def test_linear_in_the_table_and_closed_form_on_ones():
    fx = H.load("field.npz")
    fs = rm.make_spec("tiny").nerf
    _, offsets, grid_sizes, _ = fs.layout()
    n_rows = int(offsets[-1])
    g = torch.Generator().manual_seed(8)
    A = torch.rand(n_rows, 2, generator=g, dtype=torch.float64) * 2 - 1
    B = torch.rand(n_rows, 2, generator=g, dtype=torch.float64) * 2 - 1
    f = lambda T: t64.sample_features(fs, T, fx["means"], fx["stds"])[0]
    assert float((f(2.5 * A - B) - (2.5 * f(A) - f(B))).abs().max()) <= 1e-14
    # a table of ones: the trilinear weights of a cell sum to 1 -> the mean over the six multisamples of the erf damping
    ones, _, cs = t64.sample_features(fs, torch.ones(n_rows, 2, dtype=torch.float64), fx["means"], fx["stds"])
    want = t64.level_damping(cs, grid_sizes).mean(dim=-2)
    assert float((ones - want[..., None]).abs().max()) <= 1e-14
    # ... and the float32 oracle's closed form agrees to float32 rounding (the int32 wrap of grid_sizes ** 2 included:
    # levels 12-15 of this grid have sides >= 46341)
    assert int(grid_sizes[-1]) ** 2 > 2 ** 31
    _, s32 = rm.contract_points(fx["means"].reshape(-1, 3), fx["stds"].reshape(-1))
    d32 = rm.level_damping(s32.reshape(fx["stds"].shape) / 2, grid_sizes).mean(dim=-2)
    assert float((d32.double() - want).abs().max()) <= 32 * U
