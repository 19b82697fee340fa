"""Plain-torch restatement, in the dtype of its inputs (float32 or float64), of what Model.forward does with the RawNeRF exposure,
a two-valued bg_intensity_range and near_anneal_rate (ref models.py:137-146, :158-159, :168-200, :245-269, render.py:155-216,
stepfun.py:64-128, :154-218, :251-294).  Pinned to tests/golden/exposure.npz (made from the imported reference by
tests/golden/make_exposure_golden.py) in tests/test_exposure_cpu.py; the float64 run on the same float32 inputs is the truth of the
brackets in tests/test_exposure_gpu.py.

EPS is float32's in BOTH dtypes: the u grid of the inverse-CDF lookup and the pdf's width clamp are inputs of the computation (the
kernels hold them as float32 constants), not roundings of it."""
import numpy as np
import torch

EPS = float(torch.finfo(torch.float32).eps)


# ------------------------------------------------------------------ near_anneal_rate (models.py:137-146, :158-159)
def init_s_near(train_frac, near_anneal_rate, near_anneal_init=0.95):
    if near_anneal_rate is None:
        return 0.
    return float(np.clip(1 - train_frac / near_anneal_rate, 0, near_anneal_init))


def dilations(bias, multiplier, s_near, samples_per_level):
    """models.py:158-162 for every level: bias + multiplier * (init_s_far - init_s_near) / prod_num_samples."""
    out, prod = [], 1
    for S in samples_per_level:
        out.append(bias + multiplier * (1. - s_near) / prod)
        prod *= S
    return out


# ------------------------------------------------------------------ exposure (models.py:258-269)
def exposure_scaling(exposure_idx, offsets):
    """models.py:263-268: 1 + (exposure_idx > 0) * exposure_scaling_offsets(exposure_idx); exposure_idx [N, 1], offsets [E, 3]."""
    idx = exposure_idx[..., 0]
    return 1 + (idx > 0)[..., None] * offsets[idx.long()]


def exposure_block(rgb, exposure_values, exposure_idx=None, offsets=None):
    """models.py:259-269 on rgb [N, S, 3]: the colours the reference leaves in ray_results['rgb'].  offsets None: no learned scaling."""
    rgb = rgb * exposure_values[..., None, :]
    if offsets is not None:
        rgb = rgb * exposure_scaling(exposure_idx, offsets)[..., None, :]
    return rgb


def exposure_gain(exposure_values, exposure_idx=None, offsets=None, N=None):
    """The same as one per-ray factor [N, 3] (what the compositing kernel takes)."""
    gain = exposure_values.expand(exposure_values.shape[0], 3)
    if offsets is not None:
        gain = gain * exposure_scaling(exposure_idx, offsets)
    return gain


# ------------------------------------------------------------------ background (models.py:245-256)
def background(bg_range, rand, N, device='cpu'):
    """The scalar -- the one value, or the midpoint for `rand is None` alone (models.py:249) -- else, rand = False included, one
    torch.rand(N, 3) from the global generator."""
    lo, hi = bg_range
    if lo == hi:
        return lo
    if rand is None:
        return (lo + hi) / 2
    return torch.rand(N, 3, device=device) * (hi - lo) + lo


def level_draws(N, S, single_jitter, bg_range, device='cpu', rand=True):
    """The draws of one level in the reference's order: stepfun.py:216, render.py:123, :124 (these three with a true `rand` only), :140,
    models.py:256 (unless rand is None)."""
    out = {}
    if rand:
        out.update(jitter=torch.rand(N, 1 if single_jitter else S, device=device), flip=torch.rand(N, S, device=device),
                   spin=torch.rand(N, S, device=device))
    out['rvec'] = torch.randn(N, 3, device=device)
    if bg_range[0] != bg_range[1] and rand is not None:
        out['bg'] = background(bg_range, rand, N, device)
    return out


# ------------------------------------------------------------------ compositing (render.py:155-174, :199-216)
def alpha_weights(density, tdist, dirs, opaque_background=False):
    delta = (tdist[..., 1:] - tdist[..., :-1]) * torch.norm(dirs[..., None, :], dim=-1)
    dd = density * delta
    if opaque_background:
        dd = torch.cat([dd[..., :-1], torch.full_like(dd[..., -1:], torch.inf)], dim=-1)
    alpha = 1 - torch.exp(-dd)
    trans = torch.exp(-torch.cat([torch.zeros_like(dd[..., :1]), torch.cumsum(dd[..., :-1], dim=-1)], dim=-1))
    return alpha * trans


def render(rgbs, weights, tdist, bg_rgbs):
    """rgb [N, 3] (the colour line, render.py:203-205), depth [N], acc [N]; bg_rgbs a scalar or [N, 3]."""
    acc = weights.sum(dim=-1)
    bg_w = (1 - acc[..., None]).clamp_min(0.)
    rgb = (weights[..., None] * rgbs).sum(dim=-2) + bg_w * bg_rgbs
    t_mids = 0.5 * (tdist[..., :-1] + tdist[..., 1:])
    depth = torch.clip(torch.nan_to_num((weights * t_mids).sum(dim=-1) / acc.clamp_min(EPS), torch.inf), tdist[..., 0], tdist[..., -1])
    depth = torch.where(acc < 0.6, torch.full_like(depth, 300.), depth)
    return rgb, depth, acc


def composite(density, rgbs, tdist, dirs, bg_rgbs, opaque_background=False, gain=None):
    """weights, rgb, depth, acc, scaled colours of rays whose colours are scaled by a per-ray gain [N, 3] first."""
    scaled = rgbs if gain is None else rgbs * gain[..., None, :]
    weights = alpha_weights(density, tdist, dirs, opaque_background)
    rgb, depth, acc = render(scaled, weights, tdist, bg_rgbs)
    return weights, rgb, depth, acc, scaled


def s_to_t(sdist, near, far):
    """coord.py:176 with the identity curve."""
    return sdist * far + (1 - sdist) * near


# ------------------------------------------------------------------ resampling on a domain (stepfun.py, models.py:168-200)
def interp_sorted(x, xp, fp):
    """math.py:88-107 sorted_interp: its O(n m) masks pick the last knot <= x and the first knot > x; a binary search finds the same."""
    n = xp.shape[-1]
    cnt = torch.searchsorted(xp.contiguous(), x.contiguous(), right=True)
    i0, i1 = (cnt - 1).clamp_min(0), cnt.clamp_max(n - 1)
    xp0, xp1, fp0, fp1 = xp.gather(-1, i0), xp.gather(-1, i1), fp.gather(-1, i0), fp.gather(-1, i1)
    frac = torch.nan_to_num((x - xp0) / (xp1 - xp0), 0).clamp(0, 1)
    return fp0 + frac * (fp1 - fp0)


def max_dilate_weights(t, w, dilation, domain):
    """stepfun.py:75-105 with renormalize=True."""
    pdf = w / (t[..., 1:] - t[..., :-1]).clamp_min(EPS)
    t0, t1 = t[..., :-1] - dilation, t[..., 1:] + dilation
    knots = torch.sort(torch.cat([t, t0, t1], dim=-1), dim=-1).values.clamp(*domain)
    covers = (t0[..., None, :] <= knots[..., None]) & (t1[..., None, :] > knots[..., None])
    env = torch.where(covers, pdf[..., None, :], torch.zeros_like(pdf[..., None, :])).amax(dim=-1)[..., :-1]
    wd = env * (knots[..., 1:] - knots[..., :-1])
    return knots, wd / wd.sum(dim=-1, keepdim=True).clamp_min(EPS)


def u_grid(S, jitter, dtype):
    """stepfun.py:203-216 (deterministic_center=True): the float32 grid, jittered in float32 as the reference does, then cast."""
    if jitter is None:
        pad = 1 / (2 * S)
        u = torch.linspace(pad, 1. - pad - EPS, S)[None, :]
    else:
        u_max = EPS + (1 - EPS) / S
        max_jitter = (1 - u_max) / (S - 1) - EPS
        u = torch.linspace(0, 1 - u_max, S) + jitter.float().cpu() * max_jitter
    return u.to(dtype)


def sample_intervals(t, logits, S, domain, jitter=None):
    """stepfun.py:251-294 through sample and invert_cdf: [N, S + 1] fenceposts."""
    u = u_grid(S, jitter, t.dtype).to(t.device).expand(t.shape[:-1] + (S,))
    w = torch.softmax(logits, dim=-1)
    body = torch.cumsum(w[..., :-1], dim=-1).clamp_max(1)
    edge = body.new_zeros(body.shape[:-1] + (1,))
    centers = interp_sorted(u, torch.cat([edge, body, edge + 1], dim=-1), t)
    mid = (centers[..., 1:] + centers[..., :-1]) / 2
    first = (2 * centers[..., :1] - mid[..., :1]).clamp_min(domain[0])
    last = (2 * centers[..., -1:] - mid[..., -1:]).clamp_max(domain[1])
    return torch.cat([first, mid, last], dim=-1)


def resample(sdist_prev, weights_prev, dilation, anneal, padding, S, s_near, jitter=None, N=None, dtype=torch.float32):
    """One level's fenceposts (models.py:143-147, :168-200).  sdist_prev None: the first level, the interval [s_near, 1] of weight 1."""
    domain = (s_near, 1.)
    if sdist_prev is None:
        sdist = torch.tensor([s_near, 1.], dtype=dtype).expand(N, 2)
        weights = torch.ones(N, 1, dtype=dtype)
    else:
        sdist, weights = sdist_prev, weights_prev
        if dilation > 0:
            sdist, weights = max_dilate_weights(sdist, weights, dilation, domain)
            sdist, weights = sdist[..., 1:-1], weights[..., 1:-1]
    logits = torch.where(sdist[..., 1:] > sdist[..., :-1], anneal * torch.log(weights + padding),
                         torch.full_like(sdist[..., :-1], -torch.inf))
    return sample_intervals(sdist, logits, S, domain, jitter)
