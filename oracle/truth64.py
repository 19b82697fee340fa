"""float64 evaluation of the pinned-fencepost path: the TRUTH the float32 oracle and the HIP kernels are both measured against.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py; nothing under ucnerf_amd/ may import it).  Plain torch on the CPU,
dtype=torch.float64 throughout, autograd-capable.  Written against the semantics of oracle/raymarch.py (which the goldens pin
to the reference), not against the HIP code:

  * inputs are the float32 tensors the float32 paths get (rays, fenceposts, rand_vec, flip / spin draws, state dict), converted
    exactly to float64.  Fenceposts are an INPUT: the resampling is chaotic in the last bit and is not restated here;
  * constants that are part of the reference's semantics keep their float32 values: EPS (the float32 eps of the clamps), the
    clip bounds, the 300 depth sentinel, the 1e-12 of F.normalize, the per-level float32 `scale` / integer resolution of the
    grid (gridencoder.cu:107-108) and the int32 wrap of grid_sizes ** 2 in the damping (models.py:495).  Constants that are
    merely ROUNDED in float32 (pi / 3 * k, 2 pi, sqrt 2, 1 / 3) are exact here: their float32 rounding is part of the float32
    evaluation's error, which is what this module exists to measure;
  * the grid lookup is a pure-torch gather (`table[rows]` times float64 trilinear weights), so `loss.backward()` yields the
    float64 table gradient through index_add.  Row indices come from the integer rules of oracle/grid_numpy.py
    (level_geometry, rows_of), the T = 2^19 strided-level quirk included.
"""
import math

import numpy as np
import torch

from . import grid_numpy as gn

F64 = torch.float64
EPS = float(torch.finfo(torch.float32).eps)
_HEX_ORDER = (0, 2, 4, 3, 5, 1)


def f64(t):
    """exact float32 -> float64 (None passes through)"""
    return None if t is None else torch.as_tensor(t).to(F64)


def state64(sd):
    return {k: (v.to(F64) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------------------ ray distances
def s_to_t(curve, s, near, far, power_lambda=-1.5):
    """coord.py:137-177 `construct_ray_warps`' s_to_t for the curves of the fixtures: None (identity), 'piecewise',
    'power_transformation', 'reciprocal'.  The power curve's inverse adds the FLOAT32 eps (coord.py:129), as the float32 paths do."""
    s, near, far = f64(s), f64(near), f64(far)
    if curve is None:
        return s * far + (1 - s) * near
    lam = float(power_lambda)
    lam_1 = abs(lam - 1)
    if curve == "power_transformation":
        fwd = lambda x: lam_1 / lam * ((2 * x / lam_1 + 1) ** lam - 1)
        inv = lambda y: ((y * lam / lam_1 + 1 + EPS) ** (1 / lam) - 1) * lam_1 / 2
    elif curve == "piecewise":
        tiny = float(torch.finfo(torch.float32).tiny)
        fwd = lambda x: torch.where(x < 1, .5 * x, 1 - .5 / x.clamp_min(tiny))
        inv = lambda y: torch.where(y < .5, 2 * y, .5 / (1 - y).clamp_min(tiny))
    elif curve == "reciprocal":
        fwd = inv = lambda x: 1 / x
    else:
        raise ValueError(curve)
    s_near, s_far = fwd(near), fwd(far)
    return inv(s * s_far + (1 - s) * s_near)


# -------------------------------------------------------------------------------------------------------------- ray geometry
def _normalize(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)                    # F.normalize's eps


def cone_multisamples(tdist, origins, directions, cam_dirs, radii, rand_vec, std_scale=0.5, flip=None, spin=None):
    """render.py:94-152 `cast_rays` (oracle/raymarch.py cone_multisamples): means [N,S,6,3], stds [N,S,6], t [N,S,6]."""
    tdist, origins, directions, cam_dirs, radii, rand_vec = map(f64, (tdist, origins, directions, cam_dirs, radii, rand_vec))
    t0 = tdist[..., :-1, None]
    t1 = tdist[..., 1:, None]
    r = radii[..., None]
    t_m = (t0 + t1) / 2
    t_d = (t1 - t0) / 2
    j = torch.arange(6, dtype=F64)
    t = t0 + t_d / (t_d ** 2 + 3 * t_m ** 2) * (
        t1 ** 2 + 2 * t_m ** 2 + 3 / math.sqrt(7.0) * (2 * j / 5 - 1) * ((t_d ** 2 - t_m ** 2) ** 2 + 4 * t_m ** 4).sqrt())
    ang = (math.pi / 3 * torch.tensor(_HEX_ORDER, dtype=F64)).expand(t.shape)
    if flip is not None:
        keep = torch.as_tensor(flip) > 0.5                                        # a comparison of the float32 draw itself
        ang = ang + 2 * math.pi * f64(spin)[..., None]
        ang = torch.where(keep[..., None], ang, math.pi * 5 / 3 - ang)
    else:
        even = (torch.arange(t.shape[-2]) % 2 == 0).expand(t.shape[:-1])
        ang = torch.where(even[..., None], ang, ang + math.pi / 6)
        ang = torch.where(even[..., None], ang, math.pi * 5 / 3 - ang)
    rt = r * t / math.sqrt(2.0)
    local = torch.stack([rt * torch.cos(ang), rt * torch.sin(ang), t], dim=-1)
    stds = std_scale * rt
    e1 = _normalize(torch.cross(cam_dirs, rand_vec, dim=-1))
    e2 = _normalize(torch.cross(cam_dirs, e1, dim=-1))
    axes = torch.stack([e1, e2, directions], dim=-2)                              # [N, k, xyz]
    world = (local[..., :, None] * axes[..., None, None, :, :]).sum(dim=-2)
    return world + origins[..., None, None, :], stds, t


def contract_points(mean, std):
    """coord.py:60-72 `contract_mean_std`: mean [...,3], std [...] -> contracted (NOT yet halved)."""
    mean, std = f64(mean), f64(std)
    m = (mean ** 2).sum(dim=-1, keepdim=True).clamp_min(EPS)
    root = torch.sqrt(m)
    inside = m <= 1
    z = torch.where(inside, mean, ((2 * root - 1) / m) * mean)
    shrink = ((2 * root - 1).clamp_min(0) ** (1.0 / 3) / root) ** 2               # (2 root - 1 > 1 wherever it is selected)
    s = torch.where(inside[..., 0], std, shrink[..., 0] * std)
    return z, s


def view_encoding(d, deg=4):
    """coord.py:214-225 `pos_enc(0, deg, append_identity=True)`."""
    d = f64(d)
    scales = 2.0 ** torch.arange(0, deg, dtype=F64)
    scaled = (d[..., None, :] * scales[:, None]).reshape(d.shape[:-1] + (-1,))
    return torch.cat([d, torch.sin(torch.cat([scaled, scaled + 0.5 * math.pi], dim=-1))], dim=-1)


# ---------------------------------------------------------------------------------------------------------------- hash grid
def level_damping(stds, grid_sizes):
    """models.py:495 with the reference's int32 wrap of grid_sizes ** 2 (65537 ** 2 -> 131073, ...)."""
    gs2 = (torch.as_tensor(grid_sizes).to(torch.int32) ** 2).to(F64)
    return torch.erf(1 / torch.sqrt(8 * f64(stds)[..., None] ** 2 * gs2))


def grid_corners(fs, pts01, levels=None):
    """gridencoder.cu:87-199 locate + index for points in the unit cube, float64 positions: per level the 8 GLOBAL table rows
    [B,8] (int64), the 8 trilinear weights [B,8] (float64), the scaled position p = x * scale + 0.5 [B,3] and the out-of-range
    mask [B] (the kernel writes zeros there, gridencoder.cu:117-130).  `scale` and the resolution are the reference's float32
    constants; cell indices are exact integers."""
    pls, offsets, _, _ = fs.layout()
    off = np.asarray(offsets)
    scale, res, rows = gn.level_geometry(off, float(np.log2(pls)), fs.grid_base_resolution)
    x = f64(pts01).detach()
    xn = x.numpy()
    oob = torch.from_numpy(((xn < 0) | (xn > 1)).any(axis=1))
    out = []
    with np.errstate(over="ignore"):
        for l in (range(len(scale)) if levels is None else levels):
            p = x * float(scale[l]) + 0.5
            fl = torch.floor(p)
            f = p - fl
            cell = fl.numpy().astype(np.int64).astype(np.uint32)
            r8, w8 = [], []
            for k in range(8):
                w = torch.ones(x.shape[0], dtype=F64)
                corner = cell.copy()
                for d in range(3):
                    if k & (1 << d):
                        w = w * f[:, d]
                        corner[:, d] += np.uint32(1)
                    else:
                        w = w * (1 - f[:, d])
                r8.append(torch.from_numpy(gn.rows_of(corner, rows[l], res[l]).astype(np.int64) + int(off[l])))
                w8.append(w)
            out.append((l, torch.stack(r8, dim=1), torch.stack(w8, dim=1), p, oob))
    return out


def grid_features(fs, table, pts01):
    """Interpolated features [B, L, C] (float64); differentiable in `table` ([rows, C] float64)."""
    feats = []
    for _, rows, w, _, oob in grid_corners(fs, pts01):
        v = (table[rows] * w[..., None]).sum(dim=1)                               # [B,8,C] gather: index_add in the backward
        feats.append(torch.where(oob[:, None], torch.zeros_like(v), v))
    return torch.stack(feats, dim=1)


def sample_features(fs, table, means, stds, no_warp=False):
    """models.py:485-496: contraction, / 2, grid lookup, erf damping, mean over the multisample axis.
    means [...,G,3], stds [...,G] -> features [..., L, C] (float64), contracted halved means [...,G,3] and stds [...,G]."""
    means, stds = f64(means), f64(stds)
    if not no_warp:
        z, s = contract_points(means.reshape(-1, 3), stds.reshape(-1))
        means, stds = z.reshape(means.shape) / 2, s.reshape(stds.shape) / 2
    _, _, grid_sizes, _ = fs.layout()
    feat = grid_features(fs, table, ((means + 1) / 2).reshape(-1, 3))
    feat = feat.reshape(means.shape[:-1] + feat.shape[-2:])
    damp = level_damping(stds, grid_sizes)
    return (feat * damp[..., None]).mean(dim=-3), means, stds


# ------------------------------------------------------------------------------------------------------------------- fields
def _lin(x, sd, name):
    return x @ sd[name + ".weight"].T + sd[name + ".bias"]


def field_forward(fs, sd, means, stds, viewdirs=None, no_warp=False):
    """models.py:485-685 `MLP.forward` under waymo.gin.  `sd` is a float64 state (state64).  Returns a dict: features [...,L,C],
    raw_density, bottleneck, density, rgb (None for a PropMLP or without viewdirs), coord."""
    feat, cm, _ = sample_features(fs, sd[fs.prefix + ".encoder.embeddings"], means, stds, no_warp)
    h = torch.relu(_lin(feat.flatten(-2, -1), sd, fs.prefix + ".density_layer.0"))
    x = _lin(h, sd, fs.prefix + ".density_layer.2")
    raw = x[..., 0]
    density = torch.nn.functional.softplus(raw + fs.density_bias)
    rgb = None
    if not fs.disable_rgb and viewdirs is not None:
        enc = view_encoding(viewdirs, fs.deg_view)
        enc = enc[..., None, :].expand(x.shape[:-1] + (enc.shape[-1],))
        h = torch.cat([x, enc], dim=-1)
        skip = h
        for i in range(fs.net_depth_viewdirs):
            h = torch.relu(_lin(h, sd, f"{fs.prefix}.lin_second_stage_{i}"))
            if i == fs.skip_layer_dir:
                h = torch.cat([h, skip], dim=-1)
        rgb = torch.sigmoid(fs.rgb_premultiplier * _lin(h, sd, fs.prefix + ".rgb_layer") + fs.rgb_bias)
        rgb = rgb * (1 + 2 * fs.rgb_padding) - fs.rgb_padding
    return dict(features=feat, raw_density=raw, bottleneck=x, density=density, rgb=rgb, coord=cm.mean(dim=-2))


# ---------------------------------------------------------------------------------------------------------------- rendering
def alpha_weights(density, tdist, dirs, opaque_background=False):
    """render.py:155-174 `compute_alpha_weights`."""
    density, tdist, dirs = f64(density), f64(tdist), f64(dirs)
    delta = (tdist[..., 1:] - tdist[..., :-1]) * torch.norm(dirs[..., None, :], dim=-1)
    tau = density * delta
    if opaque_background:
        tau = torch.cat([tau[..., :-1], torch.full_like(tau[..., -1:], torch.inf)], dim=-1)
    alpha = 1 - torch.exp(-tau)
    trans = torch.exp(-torch.cat([torch.zeros_like(tau[..., :1]), torch.cumsum(tau[..., :-1], dim=-1)], dim=-1))
    return alpha * trans


def _interp_sorted(x, xp, fp):
    """math.py:88-107 `sorted_interp` (oracle/raymarch.py interp_sorted)."""
    n = xp.shape[-1]
    cnt = torch.searchsorted(xp.contiguous(), x.contiguous(), right=True)
    i0, i1 = (cnt - 1).clamp_min(0), cnt.clamp_max(n - 1)
    xp0, xp1, fp0, fp1 = xp.gather(-1, i0), xp.gather(-1, i1), fp.gather(-1, i0), fp.gather(-1, i1)
    frac = torch.nan_to_num((x - xp0) / (xp1 - xp0), 0).clamp(0, 1)
    return fp0 + frac * (fp1 - fp0)


def percentiles(t, w, ps=(5, 50, 95)):
    """stepfun.py:329-339 `weighted_percentile` over stepfun.py:108-128 `integrate_weights`."""
    body = torch.cumsum(w[..., :-1], dim=-1).clamp_max(1)
    edge = body.new_zeros(body.shape[:-1] + (1,))
    cdf = torch.cat([edge, body, edge + 1], dim=-1)
    q = (torch.tensor(ps, dtype=F64) / 100).expand(t.shape[:-1] + (len(ps),))
    return _interp_sorted(q, cdf, t)


def composite(rgbs, weights, tdist, bg, t_far):
    """render.py:177-244 `volumetric_rendering`: rgb, acc, depth (with the acc < 0.6 -> 300 sentinel), distance_mean and the
    three distance percentiles."""
    rgbs, weights, tdist, t_far = f64(rgbs), f64(weights), f64(tdist), f64(t_far)
    out = {}
    acc = weights.sum(dim=-1)
    bg_w = (1 - acc[..., None]).clamp_min(0.)
    out["rgb"] = (weights[..., None] * rgbs).sum(dim=-2) + bg_w * bg
    t_mid = 0.5 * (tdist[..., :-1] + tdist[..., 1:])
    depth = torch.nan_to_num((weights * t_mid).sum(dim=-1) / acc.clamp_min(EPS), torch.inf)
    depth = torch.minimum(torch.maximum(depth, tdist[..., 0]), tdist[..., -1])
    out["depth"] = torch.where(acc < 0.6, torch.full_like(depth, 300.0), depth)
    out["acc"] = acc
    logmean = (weights * torch.log(t_mid)).sum(dim=-1) / acc.clamp_min(EPS)
    dm = torch.nan_to_num(torch.exp(logmean), torch.inf)
    out["distance_mean"] = torch.minimum(torch.maximum(dm, tdist[..., 0]), tdist[..., -1])
    pct = percentiles(torch.cat([tdist, t_far], dim=-1), torch.cat([weights, bg_w], dim=-1))
    out["distance_percentile_5"], out["distance_median"], out["distance_percentile_95"] = pct[..., 0], pct[..., 1], pct[..., 2]
    return out


# --------------------------------------------------------------------------------------------------------------- whole level
def level_forward(spec, fs, sd, rays, sdist, noise, raydist=None, power_lambda=-1.5):
    """One sampling level of models.py:97-365 at GIVEN fenceposts `sdist` [N,S+1]: s_to_t, cone cast, field, weights, compositing.
    `sd` float64 state, `rays` the float32 batch of oracle/raymarch.py, `noise` its LevelNoise.  Returns (rendering, field dict)."""
    tdist = s_to_t(raydist, sdist, rays["near"], rays["far"], power_lambda)
    means, stds, ts = cone_multisamples(tdist, rays["origins"], rays["directions"], rays["cam_dirs"], rays["radii"],
                                        noise.rand_vec, spec.std_scale, noise.flip, noise.spin)
    res = field_forward(fs, sd, means, stds, rays["viewdirs"])
    w = alpha_weights(res["density"], tdist, rays["directions"], spec.opaque_background)
    rgb = res["rgb"] if res["rgb"] is not None else torch.zeros(res["density"].shape + (3,), dtype=F64)
    out = composite(rgb, w, tdist, spec.bg_intensity, f64(rays["far"]))
    out["weights"] = w
    res.update(tdist=tdist, means=means, stds=stds, ts=ts)
    return out, res
