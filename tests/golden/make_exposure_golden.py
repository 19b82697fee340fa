"""Generate tests/golden/exposure.npz: the REFERENCE's RawNeRF exposure block, random background colours and near_anneal_rate
(models.py:137-146, :158-159, :173, :200, :245-269), on CPU.

    python tests/golden/make_exposure_golden.py          (authoring container only)

Same harness as make_golden.py (ref_import: the reference's own Python, the grid op restated in C).  Data only:

  dom_*    stepfun.max_dilate_weights(domain=(s_near, 1), renormalize=True) and stepfun.sample_intervals(domain=(s_near, 1)) on
           random step functions inside [s_near, 1], s_near = 0.3 and 0.95, eval grid and captured training jitter; and the
           first level (the single interval [s_near, 1])
  comp_*   render.compute_alpha_weights + render.volumetric_rendering with per-ray background colours [N, 3] on colours scaled by
           per-ray exposures, opaque_background 0 / 1
  model_*  Model.forward on the `tiny` spec with learned_exposure_scaling, bg_intensity_range = (0.2, 0.8), near_anneal_rate = 0.1
           at train_frac = 0.03, rand=True: every draw captured (five per level: jitter, flip, spin, rand_vec, bg), per level the
           pixels, the history's density / scaled colours / fenceposts / weights; the same run WITHOUT the exposure keys (same
           seed, so the same draws) for the unscaled colours; the state dict's key order.
  eval_*   Model.forward on `tiny` with bg_intensity_range = (0.2, 0.8) alone, rand = False and rand = None after the same torch seed:
           the draws (rand = False draws the background colours, behind each level's randn_like; rand = None does not), pixels, history
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import ref_import  # noqa: E402
from oracle import raymarch as rm  # noqa: E402

S_NEARS = (0.3, 0.95)
BG_RANGE = (0.2, 0.8)
RATE, TRAIN_FRAC = 0.1, 0.03


def step_function(g, N, n, s_near):
    t = torch.sort(s_near + (1 - s_near) * torch.rand(N, n + 1, generator=g), dim=-1).values
    t[:, 0], t[:, -1] = s_near, 1.0
    w = torch.rand(N, n, generator=g) ** 3
    return t, w / w.sum(dim=-1, keepdim=True)


def gen_domain(ref, out):
    sf = ref.stepfun
    g = torch.Generator().manual_seed(201)
    N, n, S = 6, 16, 8
    for i, s_near in enumerate(S_NEARS):
        dom = (s_near, 1.0)
        t, w = step_function(g, N, n, s_near)
        dilation = 0.0025 + 0.5 * (1 - s_near) / 64
        td, wd = sf.max_dilate_weights(t, w, dilation, domain=dom, renormalize=True)
        td_, wd_ = td[..., 1:-1], wd[..., 1:-1]
        logits = torch.where(td_[..., 1:] > td_[..., :-1], 0.7 * torch.log(wd_), torch.full_like(td_[..., :-1], -torch.inf))
        ev = sf.sample_intervals(None, td_, logits, S, single_jitter=True, domain=dom)
        torch.manual_seed(202 + i)
        with ref_import.capture_rng() as cap:
            tr = sf.sample_intervals(True, td_, logits, S, single_jitter=True, domain=dom)
        first_t = torch.tensor([[s_near, 1.0]]).expand(N, 2)
        with ref_import.capture_rng() as cap0:
            first = sf.sample_intervals(True, first_t, torch.zeros(N, 1), S, single_jitter=False, domain=dom)
        out.update({f'dom{i}_s_near': torch.tensor(s_near), f'dom{i}_t': t, f'dom{i}_w': w, f'dom{i}_dilation': torch.tensor(dilation),
                    f'dom{i}_t_dilate': td, f'dom{i}_w_dilate': wd, f'dom{i}_logits': logits, f'dom{i}_eval': ev,
                    f'dom{i}_jitter': cap.draws[0][1], f'dom{i}_train': tr, f'dom{i}_first_jitter': cap0.draws[0][1],
                    f'dom{i}_first': first})


def gen_composite(ref, out):
    g = torch.Generator().manual_seed(211)
    N, S = 7, 12
    rays = rm.synthetic_rays(N, seed=212)
    sd = torch.sort(torch.rand(N, S + 1, generator=g), dim=-1).values
    tdist = sd * rays['far'] + (1 - sd) * rays['near']
    density = 4 * torch.rand(N, S, generator=g) ** 2
    rgbs = torch.rand(N, S, 3, generator=g)
    ev = 0.25 + 3.75 * torch.rand(N, 3, generator=g)
    bg = torch.rand(N, 3, generator=g)
    scaled = rgbs * ev[..., None, :]
    out.update(comp_density=density, comp_rgbs=rgbs, comp_tdist=tdist, comp_dirs=rays['directions'], comp_gain=ev, comp_bg=bg)
    for opaque in (0, 1):
        w = ref.render.compute_alpha_weights(density, tdist, rays['directions'], opaque_background=bool(opaque))[0]
        r = ref.render.volumetric_rendering(scaled, w, tdist, bg, rays['far'], False)
        out.update({f'comp{opaque}_weights': w, f'comp{opaque}_rgb': r['rgb'], f'comp{opaque}_depth': r['depth'],
                    f'comp{opaque}_acc': r['acc']})


def gen_model(ref, out):
    M = ref.models.Model
    saved = {k: M.__dict__[k] for k in ('learned_exposure_scaling', 'bg_intensity_range', 'near_anneal_rate')}
    M.learned_exposure_scaling, M.bg_intensity_range, M.near_anneal_rate = True, BG_RANGE, RATE
    try:
        spec = rm.make_spec('tiny')
        seed, n = 221, 24
        sd = rm.init_state(spec, seed=seed)
        g = torch.Generator().manual_seed(seed + 1)
        offsets = 0.2 * torch.randn(1000, 3, generator=g)
        sd_ref = dict(sd)
        sd_ref['exposure_scaling_offsets.weight'] = offsets
        model, cfg = ref_import.build_reference_model(ref, spec, sd_ref)
        keys = [k for k in model.state_dict().keys()]
        model.train()
        rays = rm.synthetic_rays(n, seed=seed + 2)
        rays['far'] = rays['far'] * (1 + 0.1 * torch.rand(n, 1, generator=g))
        rays['cam_idx'] = torch.randint(0, spec.training_views, (n, 1), generator=g)
        exposure_idx = torch.randint(0, 4, (n, 1), generator=g)
        exposure_idx[0], exposure_idx[1] = 0, 3                      # both sides of the mask are present
        exposure_values = 0.25 + 3.75 * torch.rand(n, 1, generator=g)
        runs = {}
        for tag, extra in (('plain', {}), ('exp', dict(exposure_idx=exposure_idx, exposure_values=exposure_values))):
            torch.manual_seed(seed + 3)
            with ref_import.capture_rng() as cap, torch.no_grad():
                runs[tag] = model(True, dict(rays, **extra), train_frac=TRAIN_FRAC, compute_extras=False) + (cap.draws,)
        rend, hist, draws = runs['exp']
        assert len(draws) == 5 * spec.num_levels, [d[0] for d in draws]
        out.update(model_seed=torch.tensor(seed), model_checksum=torch.tensor(mg.state_checksum(sd), dtype=torch.float64),
                   model_train_frac=torch.tensor(TRAIN_FRAC), model_rate=torch.tensor(RATE), model_bg_range=torch.tensor(BG_RANGE),
                   model_offsets=offsets, model_exposure_idx=exposure_idx, model_exposure_values=exposure_values,
                   model_state_keys=torch.tensor(np.frombuffer('\n'.join(keys).encode(), dtype=np.uint8).copy()))
        out.update({'model_ray_' + k: v for k, v in rays.items()})
        for lvl in range(spec.num_levels):
            d = draws[5 * lvl: 5 * lvl + 5]
            assert [x[0] for x in d] == ['rand', 'rand_like', 'rand_like', 'randn_like', 'rand'], [x[0] for x in d]
            for name, x in zip(('jitter', 'flip', 'spin', 'rand_vec', 'bg_u'), d):
                out[f'model_noise{lvl}_{name}'] = x[1]
                assert torch.equal(x[1], runs['plain'][2][5 * lvl + ('jitter', 'flip', 'spin', 'rand_vec', 'bg_u').index(name)][1])
            out[f'model_L{lvl}_rgb'] = rend[lvl]['rgb']
            for k in ('sdist', 'weights', 'density', 'rgb'):
                out[f'model_L{lvl}_hist_{k}'] = hist[lvl][k]
            out[f'model_L{lvl}_plain_rgb'] = runs['plain'][1][lvl]['rgb']
            assert torch.equal(hist[lvl]['sdist'], runs['plain'][1][lvl]['sdist'])
    finally:
        for k, v in saved.items():
            setattr(M, k, v)


def gen_model_eval(ref, out):
    """The two deterministic calls with a two-valued range: rand = False (what eval.py / render.py / train.py's test renders pass)
    DRAWS the background like rand = True does (models.py:249 tests `rand is None`), behind the level's one randn_like; rand = None
    takes the midpoint and draws the randn_like alone."""
    M = ref.models.Model
    saved = M.__dict__['bg_intensity_range']
    M.bg_intensity_range = BG_RANGE
    try:
        spec = rm.make_spec('tiny')
        seed, n = 231, 24
        sd = rm.init_state(spec, seed=seed)
        model, cfg = ref_import.build_reference_model(ref, spec, sd)
        model.eval()
        rays = rm.synthetic_rays(n, seed=seed + 2)
        out.update(eval_seed=torch.tensor(seed), eval_checksum=torch.tensor(mg.state_checksum(sd), dtype=torch.float64),
                   eval_torch_seed=torch.tensor(seed + 3))
        out.update({'eval_ray_' + k: v for k, v in rays.items()})
        for tag, rand, per in (('false', False, ['randn_like', 'rand']), ('none', None, ['randn_like'])):
            torch.manual_seed(seed + 3)
            with ref_import.capture_rng() as cap, torch.no_grad():
                rend, hist = model(rand, dict(rays), train_frac=1.0, compute_extras=False)
            assert [d[0] for d in cap.draws] == per * spec.num_levels, [d[0] for d in cap.draws]
            for lvl in range(spec.num_levels):
                d = cap.draws[len(per) * lvl: len(per) * (lvl + 1)]
                out[f'eval_{tag}_noise{lvl}_rand_vec'] = d[0][1]
                if rand is not None:
                    out[f'eval_{tag}_noise{lvl}_bg_u'] = d[1][1]
                out[f'eval_{tag}_L{lvl}_rgb'] = rend[lvl]['rgb']
                for k in ('sdist', 'weights', 'density', 'rgb'):
                    out[f'eval_{tag}_L{lvl}_hist_{k}'] = hist[lvl][k]
    finally:
        M.bg_intensity_range = saved


if __name__ == '__main__':
    ref = ref_import.load()
    torch.set_num_threads(1)              # fixed reduction order for the generating run
    out = {}
    gen_domain(ref, out)
    gen_composite(ref, out)
    gen_model(ref, out)
    gen_model_eval(ref, out)
    mg.save('exposure.npz', **mg.npify(out))
