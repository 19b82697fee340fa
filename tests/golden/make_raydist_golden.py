"""Generate tests/golden/raydist_{power,piecewise,reciprocal,cast}.npz and train_step_raydist.npz: the REFERENCE's Model with a
warped ray-distance curve (Model.raydist_fn, coord.py:137-177), on CPU.

    python tests/golden/make_raydist_golden.py          (authoring container only)

Same harness as make_golden.py (ref_import: the reference's own Python, the grid op restated in C), on the `tiny` spec.
Model.raydist_fn / power_lambda are set as class attributes around the run, the way gin binds them (the reference reads
them in forward, models.py:130).  Every case jitters `far` per ray (make_golden.run_model(far_jitter=True)), so that
s_near / s_far differ between rays.

  raydist_<case>.npz   'curve_*': the reference's s_to_t on a grid of (near, far, s) in float32 and float64 (s = 0, 1
                       and, for the power curve, points within a few ulp of saturation); 'L*' / 'noise*' / 'ray_*': an eval
                       Model.forward (rand=False, compute_extras) as make_golden.run_model records it
  train_step_raydist.npz  one training step of the power-transformation model, rand=True, all draws captured (as
                       make_golden.gen_train_step), loss terms and gradient digests
  raydist_cast.npz     render.cast_rays on the power curve's metric fenceposts (far 8 .. 1e5), eval and train draws, as
                       make_golden.gen_cast records it for the identity curve

Cases: power_transformation (lam = -1.5) and piecewise with near = 0; torch.reciprocal with near > 0.
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

CASES = {
    # name: (raydist_fn, near of the rays)
    'power': ('power_transformation', 0.0),
    'piecewise': ('piecewise', 0.0),
    'reciprocal': (torch.reciprocal, 0.5),
}
LAM = -1.5


def bind(ref, fn):
    M = ref.models.Model
    M.raydist_fn, M.power_lambda = fn, LAM


def curve_samples(ref, fn, near0, out):
    """s_to_t of coord.construct_ray_warps in float32 and in float64 on the same float32 inputs."""
    g = torch.Generator().manual_seed(7)
    R = 64
    near = torch.full((R, 1), near0) + (0.2 * torch.rand(R, 1, generator=g) if near0 > 0 else 0.0)
    far = torch.cat([torch.tensor([[8.0], [1e3], [1e5]]), 2.0 + 30.0 * torch.rand(R - 3, 1, generator=g)])
    s = torch.cat([torch.tensor([0.0, 1.0]), torch.rand(60, generator=g),
                   1.0 - torch.arange(1, 11, dtype=torch.float32) * 2.0 ** -24,       # the last fenceposts before s = 1
                   torch.arange(1, 11, dtype=torch.float32) * 2.0 ** -24])
    s = s[None, :].expand(R, -1).contiguous()
    for dt, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
        _, s_to_t = ref.coord.construct_ray_warps(fn, near.to(dt), far.to(dt), LAM)
        out[f'curve_t_{tag}'] = s_to_t(s.to(dt))
    out.update(curve_near=near, curve_far=far, curve_s=s)


def gen_case(ref, name):
    fn, near0 = CASES[name]
    bind(ref, fn)
    out = dict(raydist=torch.tensor(np.frombuffer((fn if isinstance(fn, str) else 'torch.' + fn.__name__).encode(),
                                                  dtype=np.uint8).copy()),
               power_lambda=torch.tensor(LAM))
    curve_samples(ref, fn, near0, out)
    spec = rm.make_spec('tiny')
    if near0 > 0:
        # run_model draws the rays itself: lift `near` through the synthetic-ray hook the harness reads (near = 0 there)
        orig = rm.synthetic_rays

        def rays_with_near(n, seed):
            b = orig(n, seed)
            b['near'] = b['near'] + near0
            return b
        rm.synthetic_rays = rays_with_near
        try:
            out.update(mg.run_model(ref, spec, 111, 32, 112, False, far_jitter=True))
        finally:
            rm.synthetic_rays = orig
    else:
        out.update(mg.run_model(ref, spec, 111, 32, 112, False, far_jitter=True))
    mg.save(f'raydist_{name}.npz', **mg.npify(out))


def gen_train_step(ref):
    bind(ref, 'power_transformation')
    spec = rm.make_spec('tiny')
    seed = 121
    sd = rm.init_state(spec, seed=seed)
    model, cfg = ref_import.build_reference_model(ref, spec, sd)
    model.train()
    n = 80
    rays = rm.synthetic_rays(n, seed=seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    rays['far'] = rays['far'] * (1 + 0.1 * torch.rand(n, 1, generator=g))
    rays['rgb'] = torch.rand(n, 3, generator=g)
    rays['cam_idx'] = torch.randint(0, spec.training_views, (n, 1), generator=g)
    rays['sky_segs'] = (torch.rand(n, generator=g) > 0.7).float()
    batch = {k: (v[:, None, None, :] if v.dim() == 2 else v[:, None, None]) for k, v in rays.items()}
    train_frac = 0.4
    torch.manual_seed(seed + 3)
    with ref_import.capture_rng() as cap:
        rend, hist = model(True, dict(batch), train_frac=train_frac, compute_extras=False)
    tu = ref.train_utils
    losses = {}
    losses['data'], stats = tu.compute_data_loss(batch, rend, cfg)
    losses['anti_interlevel'] = tu.anti_interlevel_loss(hist, cfg)
    losses['distortion'] = tu.distortion_loss(hist, cfg)
    losses['hash_decay'] = tu.hash_decay_loss(hist, cfg)
    total = sum(losses.values())
    total.backward()
    out = dict(seed=torch.tensor(seed), checksum=torch.tensor(mg.state_checksum(sd), dtype=torch.float64),
               train_frac=torch.tensor(train_frac), mse=torch.tensor(stats['mses']), power_lambda=torch.tensor(LAM))
    out.update({'ray_' + k: v for k, v in rays.items()})
    assert len(cap.draws) == 4 * spec.num_levels
    for lvl in range(spec.num_levels):
        d = cap.draws[4 * lvl: 4 * lvl + 4]
        out[f'noise{lvl}_jitter'], out[f'noise{lvl}_flip'], out[f'noise{lvl}_spin'], out[f'noise{lvl}_rand_vec'] = [x[1] for x in d]
        out[f'L{lvl}_rgb'] = rend[lvl]['rgb']
        out[f'L{lvl}_hist_sdist'] = hist[lvl]['sdist']
    for k, v in losses.items():
        out['loss_' + k] = v.detach().double()
    out['loss_total'] = total.detach().double()
    gg = torch.Generator().manual_seed(seed + 4)
    for pname, p in model.named_parameters():
        if p.grad is not None:
            mg.grad_digest('grad_' + pname, p.grad, out, gg)
    mg.save('train_step_raydist.npz', **mg.npify(out))


def gen_cast(ref):
    """render.cast_rays (render.py:94-152) on the METRIC fenceposts of the power curve, as models.py:208-218 hands them over: far
    from 8 to 1e5, so that the large distances a warped curve produces reach the geometry and the contraction."""
    bind(ref, 'power_transformation')
    N, S = 20, 32
    rays = rm.synthetic_rays(N, seed=131)
    g = torch.Generator().manual_seed(132)
    far = torch.cat([torch.tensor([[8.0], [1e3], [1e5]]), 8.0 * 10.0 ** (3.0 * torch.rand(N - 3, 1, generator=g))])
    near = torch.zeros(N, 1)
    s = torch.sort(torch.rand(N, S + 1, generator=g), dim=-1).values
    s[:, 0], s[:, -1] = 0.0, 1.0
    _, s_to_t = ref.coord.construct_ray_warps('power_transformation', near, far, LAM)
    tdist = s_to_t(s)
    out = dict(tdist=tdist, near=near, far=far, sdist=s, **{k: rays[k] for k in ('origins', 'directions', 'cam_dirs', 'radii')})
    torch.manual_seed(133)
    with ref_import.capture_rng() as cap:
        m, sdev, t = ref.render.cast_rays(tdist, rays['origins'], rays['directions'], rays['cam_dirs'], rays['radii'], False,
                                          std_scale=0.5)
    out.update(eval_rand_vec=cap.draws[0][1], eval_means=m, eval_stds=sdev, eval_t=t)
    with ref_import.capture_rng() as cap:
        m2, s2, t2 = ref.render.cast_rays(tdist, rays['origins'], rays['directions'], rays['cam_dirs'], rays['radii'], True,
                                          std_scale=0.5)
    assert [d[0] for d in cap.draws] == ['rand_like', 'rand_like', 'randn_like']
    out.update(train_flip=cap.draws[0][1], train_spin=cap.draws[1][1], train_rand_vec=cap.draws[2][1],
               train_means=m2, train_stds=s2, train_t=t2)
    mg.save('raydist_cast.npz', **mg.npify(out))


PARTS = dict(cases=lambda ref: [gen_case(ref, name) for name in CASES], train=gen_train_step, cast=gen_cast)

if __name__ == '__main__':
    # python make_raydist_golden.py [cases] [train] [cast]   (default: all)
    ref = ref_import.load()
    torch.set_num_threads(1)              # fixed reduction order for the generating run
    for part in sys.argv[1:] or list(PARTS):
        PARTS[part](ref)
