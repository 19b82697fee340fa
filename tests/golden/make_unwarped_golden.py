"""Generate tests/golden/unwarped.npz: the REFERENCE's Model with MLP.warp_fn = None (a bounded scene: the Gaussians reach the
grid uncontracted, coord.py:93-96 / models.py:488-494), on CPU.

    python tests/golden/make_unwarped_golden.py          (authoring container only)

Same harness as make_raydist_golden.py (ref_import: the reference's own Python, the grid op restated in C), on the `tiny` spec.
MLP.warp_fn is bound as a class attribute around every run, the way gin binds it.  The rays are the synthetic ones with far = 2.5
(they start inside the cube at (0.1, -0.05, 0.2) and leave it on the way), plus rays whose origin lies outside the cube: some
point away from it (every point outside), some through it.  The generator asserts and records how many multisample points of the
last level lie inside [-1, 1]^3.

  'eval_*'   an eval Model.forward (rand=False, compute_extras) as make_golden.run_model records it
  'rand_*'   a rand=True forward with all draws captured
  'train_*'  one training step (rand=True, draws captured): loss terms and gradient digests, as train_step_raydist.npz
  'cast_*'   render.cast_rays on the eval run's last-level fenceposts -> means, stds, t (the unwarped grid sees them as they are)
  'inside_*' counts of the last level's multisample points inside the cube
  'normals_*' MLP.forward of both fields with disable_density_normals = False on every fourth sample of the cast Gaussians: without the
             warp the reference's autograd reaches `means` directly (no track_linearize, hence no no_grad: tests/normals_ref.py:19)
  'scale_*'  an eval Model.forward with scale_featurization = True on both fields (weights and extra columns as
             make_scalefeat_golden.py draws them)
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import make_scalefeat_golden as msf  # noqa: E402
import ref_import  # noqa: E402
from oracle import raymarch as rm  # noqa: E402

FAR = 2.5
N_RAYS = 32          # 24 from inside, 4 outside pointing away, 4 outside pointing through the cube


def bounded_rays(orig):
    def rays(n, seed):
        b = orig(n, seed)
        b['far'] = torch.full_like(b['far'], FAR)
        b['far'][:4] = 0.6                                       # these end before the cube's face: every point inside
        v = b['viewdirs']
        o = b['origins'].clone()
        o[n - 8:n - 4] = 1.6 * v[n - 8:n - 4]                    # outside, marching away: every point outside
        o[n - 4:] = -1.2 * v[n - 4:] + torch.tensor([0.05, 0.1, -0.05])    # outside, through the cube
        b['origins'] = o.contiguous()
        return b
    return rays


class unwarped:
    """MLP.warp_fn = None and the bounded rays, around a run."""

    def __init__(self, ref):
        self.ref = ref

    def __enter__(self):
        self.saved = (self.ref.models.MLP.warp_fn, rm.synthetic_rays)
        self.ref.models.MLP.warp_fn = None
        rm.synthetic_rays = bounded_rays(rm.synthetic_rays)

    def __exit__(self, *exc):
        self.ref.models.MLP.warp_fn, rm.synthetic_rays = self.saved
        return False


def inside_counts(ev):
    """Multisample points of the eval run's last level inside [-1, 1]^3 (bounds inclusive): per ray and in all."""
    lvl = 1
    sd, near, far = ev[f'L{lvl}_hist_sdist'], ev['ray_near'], ev['ray_far']
    sd = sd.reshape(near.shape[0], -1)
    tdist = sd * far + (1 - sd) * near
    means, stds, t = rm.cone_multisamples(tdist, ev['ray_origins'], ev['ray_directions'], ev['ray_cam_dirs'], ev['ray_radii'],
                                          ev[f'noise{lvl}_rand_vec'].reshape(near.shape[0], -1))
    inside = (means.abs() <= 1).all(dim=-1)                         # [N, S, 6]
    return inside, means, stds, t, tdist


def gen_train_step(ref, out):
    spec = rm.make_spec('tiny')
    seed = 221
    sd = rm.init_state(spec, seed=seed)
    model, cfg = ref_import.build_reference_model(ref, spec, sd)
    model.train()
    n = N_RAYS
    rays = rm.synthetic_rays(n, seed=seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
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
    tr = dict(seed=torch.tensor(seed), checksum=torch.tensor(mg.state_checksum(sd), dtype=torch.float64),
              train_frac=torch.tensor(train_frac), mse=torch.tensor(stats['mses']))
    tr.update({'ray_' + k: v for k, v in rays.items()})
    assert len(cap.draws) == 4 * spec.num_levels
    for lvl in range(spec.num_levels):
        d = cap.draws[4 * lvl: 4 * lvl + 4]
        tr[f'noise{lvl}_jitter'], tr[f'noise{lvl}_flip'], tr[f'noise{lvl}_spin'], tr[f'noise{lvl}_rand_vec'] = [x[1] for x in d]
        tr[f'L{lvl}_rgb'] = rend[lvl]['rgb']
        tr[f'L{lvl}_hist_sdist'] = hist[lvl]['sdist']
    for k, v in losses.items():
        tr['loss_' + k] = v.detach().double()
    tr['loss_total'] = total.detach().double()
    gg = torch.Generator().manual_seed(seed + 4)
    for pname, p in model.named_parameters():
        if p.grad is not None:
            mg.grad_digest('grad_' + pname, p.grad, tr, gg)
    out.update({'train_' + k: v for k, v in tr.items()})


def gen_normals(ref, spec, means, stds, out):
    sd = rm.init_state(spec, seed=211)                    # the eval run's weights
    model, _ = ref_import.build_reference_model(ref, spec, sd)
    model.eval()
    inside = (means.abs() <= 1).all(dim=-1)
    assert bool(inside.all(dim=-1).any()) and bool((~inside).all(dim=-1).any())
    for name, mlp in (('nerf', model.nerf_mlp), ('prop', model.prop_mlp_0)):
        assert mlp.warp_fn is None
        mlp.disable_density_normals = False
        res = mlp(False, means.clone(), stds.clone(), viewdirs=None)
        g, n = res['raw_grad_density'].detach(), res['normals'].detach()
        assert g.shape == means.shape[:-2] + (3,) and torch.isfinite(g).all() and torch.isfinite(n).all() and float(g.abs().max()) > 0
        out[f'normals_{name}_raw_grad_density'], out[f'normals_{name}_normals'] = g, n
        out[f'normals_{name}_density'] = res['density'].detach()
    out['normals_stride'] = torch.tensor(4)


def gen_scale(ref, spec, out):
    seed = 231
    batch = rm.synthetic_rays(N_RAYS, seed=seed + 2)
    with msf.binding(ref, True):
        model, cfg, sc, sd = msf.build(ref, spec, seed, seed + 1)
        assert model.nerf_mlp.warp_fn is None and model.nerf_mlp.scale_featurization
        sc.update({'ray_' + k: v for k, v in batch.items()})
        sc['train_frac'] = torch.tensor(1.0)
        model.eval()
        torch.manual_seed(seed + 3)
        with ref_import.capture_rng() as cap, torch.no_grad():
            rend, hist = model(False, dict(batch), train_frac=1.0, compute_extras=True, zero_glo=True)
    for lvl in range(spec.num_levels):
        sc[f'noise{lvl}_rand_vec'] = cap.draws[lvl][1]
        for k in ('rgb', 'acc', 'weights'):
            sc[f'L{lvl}_{k}'] = rend[lvl][k]
        for k in ('sdist', 'density'):
            sc[f'L{lvl}_hist_{k}'] = hist[lvl][k]
    for k in ('sd_keys', 'sd_ndims', 'sd_shapes'):
        sc.pop(k)
    out.update({'scale_' + k: v for k, v in sc.items()})


def main():
    ref = ref_import.load()
    torch.set_num_threads(1)              # fixed reduction order for the generating run
    spec = rm.make_spec('tiny')
    out = {}
    with unwarped(ref):
        ev = mg.run_model(ref, spec, 211, N_RAYS, 212, False)
        inside, means, stds, t, tdist = inside_counts(ev)
        frac = float(inside.float().mean())
        per_ray = inside.reshape(inside.shape[0], -1)
        all_in, all_out = int(per_ray.all(dim=-1).sum()), int((~per_ray).all(dim=-1).sum())
        whole_out = int((~inside).all(dim=-1).sum())               # samples with all six points outside
        print(f'last level: {frac:.3f} of the multisample points inside; rays all inside {all_in}, all outside {all_out}; '
              f'samples wholly outside {whole_out}')
        assert 0.25 <= frac <= 0.75, frac
        assert all_in >= 1 and all_out >= 1, (all_in, all_out)
        out.update({'eval_' + k: v for k, v in ev.items()})
        out.update(inside_points=torch.tensor(int(inside.sum())), inside_total=torch.tensor(inside.numel()),
                   inside_rays_all=torch.tensor(all_in), inside_rays_none=torch.tensor(all_out),
                   inside_samples_none=torch.tensor(whole_out))
        # render.cast_rays itself on those fenceposts: what the unwarped grid is handed
        # (every sixth inside ray and the eight outside ones: the file stays small)
        idx = torch.tensor(list(range(0, N_RAYS - 8, 6)) + list(range(N_RAYS - 8, N_RAYS)))
        torch.manual_seed(215)
        with ref_import.capture_rng() as cap:
            m, s, tt = ref.render.cast_rays(tdist[idx], ev['ray_origins'][idx], ev['ray_directions'][idx], ev['ray_cam_dirs'][idx],
                                            ev['ray_radii'][idx], False, std_scale=0.5)
        out.update(cast_rays=idx, cast_tdist=tdist[idx], cast_rand_vec=cap.draws[0][1], cast_means=m, cast_stds=s, cast_t=tt)
        out.update({'rand_' + k: v for k, v in mg.run_model(ref, spec, 213, N_RAYS, 214, True, train_frac=0.3,
                                                           compute_extras=False).items()})
        gen_train_step(ref, out)
        gen_normals(ref, spec, m[:, ::4].contiguous(), s[:, ::4].contiguous(), out)
        gen_scale(ref, spec, out)
    mg.save('unwarped.npz', **mg.npify(out))


if __name__ == '__main__':
    main()
