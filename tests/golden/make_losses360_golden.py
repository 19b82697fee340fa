"""Generate tests/golden/losses360.npz: the REFERENCE's mip-NeRF 360 loss terms on CPU.

    python tests/golden/make_losses360_golden.py          (authoring container only)

Same harness as make_golden.py (ref_import: the reference's own Python).  Three terms of train.py:173-216:

  * `stepfun.lossfun_outer(c, w, cp, wp).mean()` per proposal level and `train_utils.interlevel_loss` over a ray history
    (train_utils.py:233-244), value and autograd gradient d / d wp;
  * `train_utils.opacity_loss` (:308-313), value and d / d acc per level;
  * `train_utils.compute_data_loss` with data_loss_type = 'rawnerf' (:195-202), value, the mses statistic and d / d rgb per level.

Next to every float32 result of the reference sits `.f64`: the same formula evaluated in float64 on the same float32 inputs
(FLT_EPSILON stays float32's: it is part of the formula, stepfun.py:54).  The outer measure's float64 form is the reference's
own `stepfun.inner_outer` on float64 tensors (masks and all), not the binary-search form under test.  The tests hold the
kernels to 2 |float32 reference - float64| + 2 ulp.

Cases of the outer loss (key prefix `outer.<case>.`): (S_nerf, S_prop) = (32, 128) [waymo.gin], (32, 64), (33, 65),
(130, 70) [`big_nerf`: three NeRF intervals per lane], (1, 1); N = 5
(the second workgroup of four rays is partly filled) and N = 1; `special` (32, 64) holds one ray each with NeRF fenceposts that
coincide with proposal fenceposts in the interior, with zero-width NeRF and proposal intervals, with w <= w_outer everywhere (loss
and gradient exactly 0), with wp = 0 (the constant-gradient regime) and a random one.  Both histograms span [0, 1] on every ray.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import ref_import  # noqa: E402

EPS32 = float(torch.finfo(torch.float32).eps)


def fenceposts(g, N, S):
    t = torch.sort(torch.rand(N, S + 1, generator=g), dim=-1).values
    t[:, 0], t[:, -1] = 0.0, 1.0
    return t


def weights(g, N, S, power, total=1.0):
    w = torch.rand(N, S, generator=g) ** power
    return (total * w / w.sum(-1, keepdim=True)).float()


def outer_inputs():
    g = torch.Generator().manual_seed(360)
    cases = {}
    for name, N, S1, Sp in (("waymo", 5, 32, 128), ("s32_64", 5, 32, 64), ("odd", 5, 33, 65), ("big_nerf", 5, 130, 70)):
        cases[name] = [fenceposts(g, N, S1), weights(g, N, S1, 6, 0.9), fenceposts(g, N, Sp), weights(g, N, Sp, 2, 0.95)]
    cases["one"] = [torch.tensor([[0.0, 1.0]]), torch.tensor([[0.7]]), torch.tensor([[0.0, 1.0]]), torch.tensor([[0.4]])]
    N, S1, Sp = 5, 32, 64
    c, w, cp, wp = fenceposts(g, N, S1), weights(g, N, S1, 6, 0.9), fenceposts(g, N, Sp), weights(g, N, Sp, 2, 0.95)
    c[0] = cp[0, ::2]                                            # ray 0: every NeRF fencepost IS a proposal fencepost
    c[1, 5:9] = c[1, 5]                                          # ray 1: zero-width intervals on both sides, some at the same place
    c[1, 20:22] = c[1, 20]
    cp[1, 10:14] = c[1, 5]
    cp[1, 40:43] = cp[1, 40]
    c[1], cp[1] = torch.sort(c[1]).values, torch.sort(cp[1]).values
    wp[2] = 0.95 / Sp * (0.5 + torch.rand(Sp, generator=g))      # ray 2: an envelope well above float32's rounding of cy (w set below)
    wp[3] = 0.0                                                  # ray 3: w_outer = 0
    cases["special"] = [c, w, cp, wp]
    return cases


def outer_f64(ref, c, w, cp, wp):
    """lossfun_outer(...).mean() and its gradient in float64 with float32's eps"""
    c, w, cp = c.double(), w.double(), cp.double()
    wp = wp.double().requires_grad_(True)
    _, w_outer = ref.stepfun.inner_outer(c, cp, wp)
    loss = ((w - w_outer).clamp_min(0) ** 2 / (w + EPS32)).mean()
    loss.backward()
    return loss.detach(), wp.grad, w_outer.detach()


def gen_outer(ref, out):
    cases = outer_inputs()
    # ray 2 of `special`: the NeRF weights sit under the envelope, w = w_outer / 4 rounded down to float32
    c, w, cp, wp = cases["special"]
    _, _, wo = outer_f64(ref, c, w, cp, wp)
    w[2] = torch.nextafter((wo[2] / 4).float(), torch.zeros(()))
    for name, (c, w, cp, wp) in cases.items():
        wq = wp.clone().requires_grad_(True)
        loss = ref.stepfun.lossfun_outer(c, w, cp, wq).mean()
        loss.backward()
        l64, g64, _ = outer_f64(ref, c, w, cp, wp)
        k = f"outer.{name}."
        out.update({k + "c": c, k + "w": w, k + "cp": cp, k + "wp": wp, k + "loss": loss.detach(), k + "grad": wq.grad,
                    k + "loss.f64": l64, k + "grad.f64": g64})
        print(f"{name}: loss {float(loss.detach()):.6e} (f64 {float(l64):.6e})  |grad| max {float(wq.grad.abs().max()):.3e}")
    s = out["outer.special.grad"]
    assert float(s[2].abs().max()) == 0.0 and float(s[3].min()) * 5 * 32 < -1.9        # the mean's 1 / (N S_nerf) undone
    # train_utils.interlevel_loss over a three-level history
    g = torch.Generator().manual_seed(361)
    N = 37
    hist_in = [(fenceposts(g, N, 64), weights(g, N, 64, 2, 0.95)), (fenceposts(g, N, 128), weights(g, N, 128, 3, 0.95)),
               (fenceposts(g, N, 32), weights(g, N, 32, 6, 0.9))]
    cfg = ref.configs.Config()
    cfg.interlevel_loss_mult = 0.01
    wps = [wp.clone().requires_grad_(True) for _, wp in hist_in[:-1]]
    hist = [dict(sdist=hist_in[i][0], weights=wps[i]) for i in range(2)] + [dict(sdist=hist_in[2][0], weights=hist_in[2][1])]
    loss = ref.train_utils.interlevel_loss(hist, cfg)
    loss.backward()
    l64, g64 = 0.0, []
    for i in range(2):
        l, gr, _ = outer_f64(ref, hist_in[2][0], hist_in[2][1], hist_in[i][0], hist_in[i][1])
        l64 = l64 + 0.01 * l
        g64.append(0.01 * gr)
    out.update({"hist.mult": torch.tensor(0.01), "hist.loss": loss.detach(), "hist.loss.f64": l64})
    for i in range(3):
        out[f"hist.sdist.{i}"], out[f"hist.weights.{i}"] = hist_in[i]
    for i in range(2):
        out[f"hist.grad.{i}"], out[f"hist.grad.{i}.f64"] = wps[i].grad, g64[i]
    print(f"hist: loss {float(loss):.6e} (f64 {float(l64):.6e})")


def gen_opacity(ref, out):
    g = torch.Generator().manual_seed(362)
    cfg = ref.configs.Config()
    cfg.opacity_loss_mult = 0.01
    for name, N, L in (("l1", 1, 1), ("l2", 5, 2), ("l3", 5, 3), ("blocks", 1500, 3)):
        accs = [torch.rand(N, generator=g) for _ in range(L)]
        if N >= 5:
            accs[0][0], accs[0][1] = 0.0, 1.0                   # log(1e-5) and the zero crossing of -o log(o + 1e-5)
            accs[-1][2], accs[-1][3] = 1.0, 0.0
        else:
            accs[0][0] = 1.0
        leaves = [a.clone().requires_grad_(True) for a in accs]
        loss = ref.train_utils.opacity_loss([dict(acc=a) for a in leaves], cfg)
        loss.backward()
        d = [a.double().requires_grad_(True) for a in accs]
        l64 = sum(0.01 * (-o * torch.log(o + 1e-5)).mean() for o in d)
        l64.backward()
        k = f"opacity.{name}."
        out.update({k + "mult": torch.tensor(0.01), k + "loss": loss.detach(), k + "loss.f64": l64.detach()})
        for l in range(L):
            out[k + f"acc.{l}"], out[k + f"grad.{l}"], out[k + f"grad.{l}.f64"] = accs[l], leaves[l].grad, d[l].grad
        print(f"opacity {name}: loss {float(loss):.6e} (f64 {float(l64):.6e})")


def gen_rawnerf(ref, out):
    g = torch.Generator().manual_seed(363)
    cfg = ref.configs.Config()
    cfg.data_loss_type, cfg.data_loss_mult, cfg.data_coarse_loss_mult = 'rawnerf', 1.0, 0.3
    cfg.disable_multiscale_loss, cfg.compute_disp_metrics, cfg.compute_normal_metrics = False, False, False
    for name, N, L in (("l1", 1, 1), ("l2", 5, 2), ("l3", 5, 3), ("blocks", 1500, 3)):
        target = torch.rand(N, 3, generator=g)
        lossmult = 0.25 + torch.rand(N, 1, generator=g)
        rgbs = [torch.rand(N, 3, generator=g) * 1.4 for _ in range(L)]       # both sides of the clip at 1
        rgbs[0][0, 0], rgbs[-1][0, 1], rgbs[-1][0, 2] = 1.0, 1.25, 0.0       # the bound itself (gradient 1, like torch), above, and 0
        leaves = [r.clone().requires_grad_(True) for r in rgbs]
        loss, stats = ref.train_utils.compute_data_loss(dict(rgb=target, lossmult=lossmult), [dict(rgb=r) for r in leaves], cfg)
        loss.backward()
        d = [r.double().requires_grad_(True) for r in rgbs]
        m, t = torch.broadcast_to(lossmult.double(), target.shape), target.double()
        per, mses = [], []
        for r in d:
            clip = r.clamp_max(1)
            per.append((m * ((clip - t) ** 2 * (1. / (1e-3 + clip.detach())) ** 2)).sum() / m.sum())
            mses.append(((m * (r - t) ** 2).sum() / m.sum()).detach())
        l64 = 0.3 * sum(per[:-1]) + 1.0 * per[-1]
        l64.backward()
        k = f"rawnerf.{name}."
        out.update({k + "target": target, k + "lossmult": lossmult, k + "coarse_mult": torch.tensor(0.3), k + "loss": loss.detach(),
                    k + "loss.f64": l64.detach(), k + "mses": torch.from_numpy(np.asarray(stats['mses'], dtype=np.float64)),
                    k + "mses.f64": torch.stack(mses)})
        for l in range(L):
            out[k + f"rgb.{l}"], out[k + f"grad.{l}"], out[k + f"grad.{l}.f64"] = rgbs[l], leaves[l].grad, d[l].grad
        print(f"rawnerf {name}: loss {float(loss):.6e} (f64 {float(l64):.6e})")


if __name__ == '__main__':
    ref = ref_import.load()
    torch.set_num_threads(1)              # fixed reduction order for the generating run
    out = {}
    gen_outer(ref, out)
    gen_opacity(ref, out)
    gen_rawnerf(ref, out)
    mg.save('losses360.npz', **mg.npify(out))
