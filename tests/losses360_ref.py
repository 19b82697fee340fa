"""Shared by tests/test_losses360_cpu.py and tests/test_losses360_gpu.py: the fixture tests/golden/losses360.npz
(tests/golden/make_losses360_golden.py), its bars, and plain torch forms of the three terms for inputs the fixture does not hold
(the outer measure from one [S_prop+1, S_nerf+1] comparison table, quadratic like the reference's and independent of the binary
searches under test; the fixture pins all of them to the reference's values).

The bar of a quantity q: with q32 the reference's float32 result and q64 the float64 evaluation of the same formula, both
from the fixture, an implementation may sit at most  2 max|q32 - q64| + 2 ulp  from q64 in the largest element, ulp being
float32's spacing at max|q64|: twice as far from the truth as the float32 reference itself, plus the last-place rounding
every float32 result carries whatever produced it (a reference that happens to hit the truth exactly leaves that much)."""
import types

import numpy as np
import torch

import helpers as H

OUTER_CASES = ["waymo", "s32_64", "odd", "big_nerf", "one", "special"]
LEVEL_CASES = ["l1", "l2", "l3", "blocks"]

_fx = None


def fixture():
    """loaded once and shared; callers do not modify it"""
    global _fx
    if _fx is None:
        _fx = H.load("losses360.npz")
    return _fx


def bar(q32, q64):
    q32, q64 = torch.as_tensor(q32).double(), torch.as_tensor(q64).double()
    ulp = float(np.spacing(np.float32(float(q64.abs().max()))))
    return 2.0 * float((q32 - q64).abs().max()) + 2.0 * ulp


def err(got, q64):
    return float((torch.as_tensor(got).detach().cpu().double() - torch.as_tensor(q64).double()).abs().max())


def levels_of(fx, prefix, key):
    out = []
    while f"{prefix}{key}.{len(out)}" in fx:
        out.append(fx[f"{prefix}{key}.{len(out)}"])
    return out


def _report(name, what, b, e, e_ref):
    line = f"{name:44s} {what:28s} bar {b:.3e}  observed {e:.3e}  (reference's own error {e_ref:.3e})"
    print("LOSSES360 " + line)
    return line


def check(name, got, fx, key):
    """|got - f64| <= bar, both sides of the bar from the fixture; prints the bar and the observed error first"""
    b, e = bar(fx[key], fx[key + ".f64"]), err(got, fx[key + ".f64"])
    line = _report(name, key, b, e, err(fx[key], fx[key + ".f64"]))
    assert e <= b, line


def check_pair(name, what, got, q32, q64):
    """the same bar from a float32 / float64 pair computed on the spot (inputs the fixture does not hold)"""
    b, e = bar(q32, q64), err(got, q64)
    line = _report(name, what, b, e, err(q32, q64))
    assert e <= b, line


# ---------------------------------------------------------------- an independent quadratic form of the outer measure
EPS32 = float(torch.finfo(torch.float32).eps)


def envelope_indices(cp, c):
    """For every fencepost v of c, from ONE comparison table [.., S_prop+1, S_nerf+1]: lo = the last proposal fencepost that is
    not above v (0 when all are above), hi = the first proposal fencepost above v (the last one when none is).  No search and no
    sortedness assumed: what train_utils' binary searches are checked against."""
    n = cp.shape[-1]
    not_above = cp.unsqueeze(-1) <= c.unsqueeze(-2)
    k = torch.arange(n, device=cp.device).unsqueeze(-1)
    return (not_above * k).amax(dim=-2), torch.where(not_above, n - 1, k).amin(dim=-2)


def outer_masks(c, w, cp, wp, eps=None):
    """per NeRF interval: max(w - envelope, 0)^2 / (w + eps), envelope = proposal mass between lo(left end) and hi(right end)"""
    mass = torch.nn.functional.pad(wp.cumsum(dim=-1), (1, 0))              # mass to the left of each proposal fencepost
    lo, hi = envelope_indices(cp, c)
    envelope = mass.gather(-1, hi[..., 1:]) - mass.gather(-1, lo[..., :-1])
    excess = (w - envelope).clamp_min(0)
    return excess * excess / (w + (torch.finfo(c.dtype).eps if eps is None else eps))


def interlevel_masks(ray_history, mult, eps=None):
    c, w = ray_history[-1]['sdist'].detach(), ray_history[-1]['weights'].detach()
    return mult * sum(outer_masks(c, w, h['sdist'], h['weights'], eps).mean() for h in ray_history[:-1])


def opacity_torch(accs, mult):
    return sum(mult * (-o * torch.log(o + 1e-5)).mean() for o in accs)


def rawnerf_torch(rgbs, target, lossmult, coarse, fine=1.0):
    m = torch.broadcast_to(lossmult, target.shape)
    per = []
    for r in rgbs:
        clip = r.clamp_max(1)
        per.append((m * ((clip - target) ** 2 * (1. / (1e-3 + clip.detach())) ** 2)).sum() / m.sum())
    return coarse * sum(per[:-1]) + fine * per[-1]


def rawnerf_config(coarse):
    return types.SimpleNamespace(data_loss_type='rawnerf', data_loss_mult=1.0, data_coarse_loss_mult=float(coarse), charb_padding=0.001,
                                 disable_multiscale_loss=False)
