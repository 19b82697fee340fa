"""Autograd restatement of the predicted-normal head and the orientation loss (ref models.py:442-444, :569-578, render.py:155-174,
train_utils.py:282-298) in a chosen dtype, on the fixture's recorded features (tests/golden/pred_normals.npz): the float64 truth the
GPU tests measure against, and -- in float32 -- pinned to the reference's own values on the CPU (tests/test_pred_normals_cpu.py).
Also the helpers the tests share: the fixture, this project's Model built from it, the bracket rule."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pred_normals.npz")
EPS32 = float(torch.finfo(torch.float32).eps)
LEVELS = ("prop_mlp_0", "nerf_mlp")
HEAD_PARAMS = ("normal_layer.weight", "normal_layer.bias", "density_layer.0.weight", "density_layer.0.bias", "density_layer.2.weight",
               "density_layer.2.bias")
NERF = dict(bottleneck_width=64, net_width_viewdirs=64, enable_pred_normals=True, disable_density_normals=True, disable_rgb=False,
            grid_level_dim=4, grid_disired_resolution=128, grid_log2_hashmap_size=9)
PROP = dict(bottleneck_width=64, net_width_viewdirs=64, enable_pred_normals=True, disable_density_normals=True, disable_rgb=False,
            grid_level_dim=2, grid_log2_hashmap_size=8, scale_featurization=True)
MODEL = dict(num_levels=2, num_prop_samples=13, num_nerf_samples=24, prop_desired_grid_size=[64], num_glo_features=4,
             num_glo_embeddings=8)

_fx = None


def fixture():
    global _fx
    if _fx is None:
        with np.load(GOLDEN) as z:
            _fx = {k: z[k] for k in z.files}
    return _fx


def state(fx=None):
    fx = fixture() if fx is None else fx
    return {k[3:]: torch.from_numpy(fx[k].astype(np.float32)) for k in fx if k.startswith("sd_") and k not in ("sd_keys", "sd_ndims", "sd_shapes")}


def sd_layout(fx=None):
    """(keys, shapes) of the reference's state dict, in its order"""
    fx = fixture() if fx is None else fx
    keys = bytes(fx["sd_keys"]).decode().split("\n")
    dims, flat, shapes, at = fx["sd_ndims"].tolist(), fx["sd_shapes"].tolist(), [], 0
    for n in dims:
        shapes.append(tuple(flat[at:at + n]))
        at += n
    return keys, shapes


def build_model(device=None, config=None, flag=True, **model_kw):
    """this project's Model with the fixture's architecture and parameters (flag=False: the same fields without the head)"""
    from ucnerf_amd.internal import configs, models
    nerf, prop = dict(NERF, enable_pred_normals=flag), dict(PROP, enable_pred_normals=flag)
    with models.bindings(NerfMLP=nerf, PropMLP=prop):
        model = models.Model(config=configs.Config() if config is None else config, **dict(MODEL, **model_kw))
    sd = state()
    if not flag:
        sd = {k: v for k, v in sd.items() if "normal_layer" not in k}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("encoder." in k for k in missing), (missing, unexpected)
    return model if device is None else model.to(device)


def batch(device=None, shape=None):
    fx = fixture()
    b = {k[4:]: torch.from_numpy(fx[k]) for k in fx if k.startswith("ray_")}
    b["rand_vec"] = torch.cat([torch.from_numpy(fx[f"noise{l}_rand_vec"]) for l in range(2)], dim=-1)
    if shape is not None:
        b = {k: v.reshape(shape + v.shape[1:]) for k, v in b.items()}
    return b if device is None else {k: v.to(device) for k, v in b.items()}


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def neg_normalize(g):
    """-ref_utils.l2_normalize(g) = -g / max(|g|, float32 eps) (F.normalize)"""
    return -g / g.norm(dim=-1, keepdim=True).clamp_min(EPS32)


def head(feat, p):
    """feat [..., F], p: the six HEAD_PARAMS -> (x [..., NB] the bottleneck, grad_pred [..., 3], normals_pred [..., 3])"""
    h = torch.relu(feat @ p["density_layer.0.weight"].t() + p["density_layer.0.bias"])
    x = h @ p["density_layer.2.weight"].t() + p["density_layer.2.bias"]
    g = x @ p["normal_layer.weight"].t() + p["normal_layer.bias"]
    return x, g, neg_normalize(g)


def alpha_weights(density, tdist, dirs):
    """render.py:155-174 (opaque_background = False)"""
    dd = density * ((tdist[..., 1:] - tdist[..., :-1]) * dirs.norm(dim=-1, keepdim=True))
    trans = torch.exp(-torch.cat([torch.zeros_like(dd[..., :1]), torch.cumsum(dd[..., :-1], dim=-1)], dim=-1))
    return (1 - torch.exp(-dd)) * trans


def orientation_term(w, n, viewdirs):
    """train_utils.py:282-298, one level, per ray"""
    n_dot_v = (n * (-1.0 * viewdirs)[..., None, :]).sum(dim=-1)
    return (w * n_dot_v.clamp_min(0) ** 2).sum(dim=-1)


def restate(dtype, fx=None, density_bias=-1.0, features=None, sdist=None):
    """Both levels from the fixture's features in `dtype`: per level x, grad_pred, normals_pred, weights, the composited normals and
    the loss; 'loss_total' at the fixture's multipliers, 'grad_<level>.<param>' of it for the six head parameters and
    'gfeat_L<level>' for the features.  features / sdist: per level [37, S, F] / [37, S + 1] tensors that stand in for the fixture's --
    what a device march gathered and resampled, so that its head is measured against the float64 truth of ITS inputs."""
    fx = fixture() if fx is None else fx
    sd = state(fx)
    t = lambda k: torch.from_numpy(fx[k]).to(dtype)
    out, total, params = {}, 0.0, {}
    mults = fx["mults"].tolist()
    for lvl, name in enumerate(LEVELS):
        p = {k: sd[f"{name}.{k}"].to(dtype).requires_grad_(True) for k in HEAD_PARAMS}
        params[name] = p
        feat = (t(f"L{lvl}_features") if features is None else features[lvl].detach().cpu().to(dtype)).requires_grad_(True)
        params[f"feat{lvl}"] = feat
        x, g, n = head(feat, p)
        density = torch.nn.functional.softplus(x[..., 0] + density_bias)
        sd_l = t(f"L{lvl}_sdist") if sdist is None else sdist[lvl].detach().cpu().to(dtype).reshape(feat.shape[0], -1)
        tdist = t("ray_near") + sd_l * (t("ray_far") - t("ray_near"))
        w = alpha_weights(density, tdist, t("ray_directions"))
        loss = orientation_term(w, n, t("ray_viewdirs")).mean()
        total = total + mults[lvl] * loss
        out.update({f"L{lvl}_x": x.detach(), f"L{lvl}_grad_pred": g.detach(), f"L{lvl}_normals_pred": n.detach(), f"L{lvl}_weights": w.detach(),
                    f"L{lvl}_render_normals_pred": (w[..., None] * n).sum(dim=-2).detach(), f"L{lvl}_loss": loss.detach()})
    total.backward()
    out["loss_total"] = total.detach()
    for lvl in range(len(LEVELS)):
        out[f"gfeat_L{lvl}"] = params.pop(f"feat{lvl}").grad
    for name, p in params.items():
        for k, v in p.items():
            out[f"grad_{name}.{k}"] = v.grad
    return out


# ---- the bracket (oracle/truth64.py, tests/test_bracket_gpu.py): an error measured against float64, allowed 4x the float32 reference's own
def rel_err(got, truth):
    """max |got - truth| / max |truth|"""
    got, truth = torch.as_tensor(got).double().cpu(), torch.as_tensor(truth).double().cpu()
    return float((got - truth).abs().max() / truth.abs().max().clamp_min(1e-300))


def allowed(ref32, truth, factor=4.0):
    """factor x the float32 reference's own error against the float64 truth, never below factor x float32 eps (a reference value that
    happens to round exactly would otherwise ask for more than the format holds)"""
    return factor * max(rel_err(ref32, truth), EPS32)


# ---- the corners of the heads' shared kernel body (csrc/hidden_rows.h): g = A relu(W0 f + b0) + c on hand-made inputs -----------------
HR_L, HR_N, HR_S = 3, 3, 87            # P * C as small as 3 and as odd as 5; B = 261: two workgroups, the second almost empty


def hidden_rows_case(C, scale_planes):
    """Seeded float32 inputs for a field of HR_L levels of width C, with (scale_planes) or without ceil(L / C) scale planes behind them:
    feat [B, P*C] per sample b, w0 [64, P*C], b0 [64], A [7, 64], c [7], s [N, S, 3] a colour sigmoid.  Some hidden pre-activations are
    exactly 0 or negative in float32 and in float64 alike: unit 5 is 0 and unit 7 is -0.5 for every sample, unit 9 is 1 * 0.25 - 0.25 on
    every fifth sample, and every 17th sample has zero features (h = b0, with b0[11] = 0)."""
    P = HR_L + ((HR_L + C - 1) // C if scale_planes else 0)
    gen = torch.Generator().manual_seed(100 * C + int(scale_planes))
    u = lambda *shape: torch.rand(*shape, generator=gen) * 2 - 1
    feat, w0, b0, A, c = u(HR_N * HR_S, P * C), u(64, P * C), u(64) / 2, u(7, 64) / 4, u(7)
    w0[5], b0[5] = 0.0, 0.0
    w0[7], b0[7] = 0.0, -0.5
    w0[9], b0[9] = 0.0, -0.25
    w0[9, 0], feat[::5, 0] = 1.0, 0.25
    feat[3::17], b0[11] = 0.0, 0.0
    return dict(C=C, P=P, feat=feat, w0=w0, b0=b0, A=A, c=c, s=torch.rand(HR_N, HR_S, 3, generator=gen))


def hidden_rows_planes(case, device):
    """the case's features as the kernels' [P][B][C] buffer"""
    return case["feat"].reshape(-1, case["P"], case["C"]).permute(1, 0, 2).contiguous().to(device)


def hidden_rows_field(case, device):
    """(a hand-filled ucn_field_t with what the heads' entry points read, the device tensors it points to)"""
    from ucnerf_amd import _lib
    w0, b0 = case["w0"].contiguous().to(device), case["b0"].to(device)
    d = _lib.UcnField()
    d.w_d0, d.b_d0, d.num_levels, d.level_dim, d.n_scale_planes = w0.data_ptr(), b0.data_ptr(), HR_L, case["C"], case["P"] - HR_L
    return d, (w0, b0)


def hidden_rows_ref(case, dtype, A, c, layout):
    """A relu(W0 f + b0) + c in `dtype` for the float32 A [R, 64], c [R] the kernel is handed, as [N, S, R]: sample b is ray * S + s
    (layout 0) or s * N + ray (layout 2)"""
    feat, w0, b0 = (case[n].to(dtype) for n in ("feat", "w0", "b0"))
    g = torch.relu(feat @ w0.t() + b0) @ A.to(dtype).t() + c.to(dtype)
    return g.reshape(HR_N, HR_S, -1) if layout == 0 else g.reshape(HR_S, HR_N, -1).transpose(0, 1)


def unplanes(fb, L, C, F, N, S, layout):
    """a kernel feature buffer [L + scale planes][N*S][C] (layout 0: b = ray*S + s, 2: b = s*N + ray) as [N, S, F] features in
    density_layer's column order: L*C grid features, then (F > L*C) the L scale features out of their ceil(L / C) planes"""
    p = fb.reshape(-1, N, S, C) if layout == 0 else fb.reshape(-1, S, N, C).permute(0, 2, 1, 3)
    p = p.permute(1, 2, 0, 3)                                           # [N, S, P, C]
    grid = p[:, :, :L].reshape(N, S, L * C)
    if F == L * C:
        return grid.contiguous()
    return torch.cat([grid, p[:, :, L:].reshape(N, S, -1)[..., :L]], dim=-1).contiguous()
