"""Generate tests/golden/pred_normals.npz: the REFERENCE's predicted-normal head (MLP.enable_pred_normals) and its orientation
loss, on CPU.

    python tests/golden/make_pred_normals_golden.py          (authoring container only)

Same harness as make_glo_golden.py (ref_import: the reference's own Python, the grid op restated in C).  One two-level Model
whose fields both carry the head (disable_density_normals = True, disable_rgb = False), 64-wide bottleneck and colour layers:

  prop_mlp_0   level_dim 2, L = 3 levels (not a multiple of 2), scale_featurization, T = 2^8
  nerf_mlp     level_dim 4, L = 4 levels, GLO (num_glo_features 4), T = 2^9

37 rays x 13 proposal and 24 NeRF samples.  EVERY parameter is drawn here from a seeded generator as a float16-representable
value and stored in full under 'sd_<state-dict key>' (float16, exact); the tables are U(-1, 1).  normal_layer.bias is large
(|b| ~ 0.8 beside |Wn x| ~ 0.3) so that |grad_pred| stays away from 0: normals_pred is ill-conditioned where |grad_pred| is small, the
tests compare unit vectors only where the reference's |grad_pred| exceeds G_MIN, and this script asserts that at most 5 % of the
samples fall below it (and prints the share).

Contents: the state dict's keys / shapes / order; the rays and the pinned draws (rand = False: the cone basis' randn per level);
per level density_layer's input features, grad_pred, normals_pred, density, rgb, weights, sdist, the composited rgb and the composited normals_pred (compute_extras); the orientation loss per level and in
total at (orientation_coarse_loss_mult, orientation_loss_mult) = (0.3, 0.7), and its gradients with respect to normal_layer,
density_layer and the table of both fields, in full.  Nothing of that depends on the GLO code (the head reads the bottleneck
before the modulation, the weights read the density): the march runs with zero_glo = True.  'F_' keys: MLP.forward of both fields on
explicit Gaussians (the NeRF field with per-ray GLO codes).
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

N_RAYS, S_PROP, S_NERF = 37, 13, 24
G_MIN = 0.05                      # unit vectors are compared where the reference's |grad_pred| exceeds this
MULTS = (0.3, 0.7)                # (orientation_coarse_loss_mult, orientation_loss_mult)
WIDTH = dict(bottleneck_width=64, net_width_viewdirs=64, enable_pred_normals=True, disable_density_normals=True, disable_rgb=False)
NERF = dict(WIDTH, grid_level_dim=4, grid_disired_resolution=128, grid_log2_hashmap_size=9)
PROP = dict(WIDTH, grid_level_dim=2, grid_log2_hashmap_size=8, scale_featurization=True)
MODEL = dict(num_levels=2, num_prop_samples=S_PROP, num_nerf_samples=S_NERF, prop_desired_grid_size=[64],
             num_glo_features=4, num_glo_embeddings=8)


def half(t):
    return t.half().float()


def draw_state(model, seed):
    """Every parameter as a float16-representable draw: tables U(-1, 1), Linear layers U(+-1/sqrt(fan_in)) (the colour layers
    U(+-sqrt(6/fan_in)), the GLO layers small), normal_layer.bias large."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, p in model.named_parameters():
        u = torch.rand(p.shape, generator=g) * 2 - 1
        if k.endswith('embeddings'):
            v = u
        elif k.endswith('normal_layer.bias'):
            v = torch.tensor([0.8, 0.5, -0.25]) + 0.05 * u     # n . (-viewdir) of both signs on the synthetic rays
        elif 'lin_glo' in k or k.startswith('glo_vecs'):
            v = 0.3 * u
        else:
            fan_in = p.shape[-1] if p.dim() == 2 else model.get_parameter(k[:-4] + 'weight').shape[-1]
            v = u * ((6.0 / fan_in) ** 0.5 if 'lin_second_stage' in k and p.dim() == 2 else fan_in ** -0.5)
        sd[k] = half(v)
    return sd


def main():
    ref = ref_import.load()
    torch.set_num_threads(1)              # fixed reduction order for the generating run
    M = ref.models
    for cls, attrs in ((M.NerfMLP, NERF), (M.PropMLP, PROP), (M.Model, MODEL)):
        for k, v in attrs.items():       # bound for the whole generating process, like gin bindings
            setattr(cls, k, v)
    cfg = ref.configs.Config()
    cfg.orientation_coarse_loss_mult, cfg.orientation_loss_mult = MULTS
    assert cfg.orientation_loss_target == 'normals_pred'
    model = M.Model(config=cfg)
    sd = draw_state(model, 2024)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    buffers = {k for k, _ in model.named_buffers()}                  # the encoders' offsets / idx / grid_sizes: derived, not drawn
    assert not unexpected and set(missing) <= buffers, (missing, unexpected)
    keys = list(model.state_dict().keys())
    shapes = [tuple(v.shape) for v in model.state_dict().values()]
    out = dict(sd_keys=torch.tensor(np.frombuffer('\n'.join(keys).encode(), dtype=np.uint8).copy()),
               sd_ndims=torch.tensor([len(s) for s in shapes]),
               sd_shapes=torch.tensor([d for s in shapes for d in s], dtype=torch.long),
               g_min=torch.tensor(G_MIN), mults=torch.tensor(MULTS, dtype=torch.float64))
    out.update({'sd_' + k: v.half() for k, v in sd.items()})

    batch = rm.synthetic_rays(N_RAYS, seed=2025)
    batch['cam_idx'] = torch.randint(0, 8, (N_RAYS, 1), generator=torch.Generator().manual_seed(2026))
    out.update({'ray_' + k: v for k, v in batch.items()})
    model.train()
    torch.manual_seed(2027)
    feats = {}
    hooks = [m.density_layer.register_forward_hook(lambda mod, inp, res, k=k: feats.__setitem__(k, inp[0].detach().clone()))
             for k, m in ((0, model.prop_mlp_0), (1, model.nerf_mlp))]
    with ref_import.capture_rng() as cap:
        rend, hist = model(False, dict(batch), train_frac=1.0, compute_extras=True, zero_glo=True)
    for h in hooks:
        h.remove()
    assert len(cap.draws) == 2
    loss = ref.train_utils.orientation_loss(batch, model, hist, cfg)
    loss.backward()
    small = total = 0
    for lvl in range(2):
        out[f'noise{lvl}_rand_vec'] = cap.draws[lvl][1]
        for k in ('grad_pred', 'normals_pred', 'weights', 'sdist', 'density', 'rgb'):
            out[f'L{lvl}_{k}'] = hist[lvl][k].detach()
        out[f'L{lvl}_features'] = feats[lvl]                   # density_layer's input [37, S, L*C (+ L scale features)]
        out[f'L{lvl}_render_rgb'] = rend[lvl]['rgb'].detach()    # level 0: a proposal field with its colour layers composites them
        out[f'L{lvl}_render_normals_pred'] = rend[lvl]['normals_pred'].detach()
        n, w, v = hist[lvl]['normals_pred'].detach().double(), hist[lvl]['weights'].detach().double(), -batch['viewdirs'].double()
        out[f'L{lvl}_loss'] = (w * (n * v[:, None, :]).sum(-1).clamp_min(0) ** 2).sum(-1).mean()
        norm = hist[lvl]['grad_pred'].detach().norm(dim=-1)
        small, total = small + int((norm <= G_MIN).sum()), total + norm.numel()
        front = ((n * v[:, None, :]).sum(-1) > 0).double().mean()
        print(f'level {lvl}: n . (-viewdir) > 0 on {100 * float(front):.1f} % of the samples, loss {float(out[f"L{lvl}_loss"]):.4e}')
        assert 0.1 < float(front) < 0.9, float(front)                  # the clamp is exercised on both sides
    out['loss_total'] = loss.detach().double()
    share = small / total
    print(f'samples with |grad_pred| <= {G_MIN}: {small} of {total} ({100 * share:.2f} %)')
    assert share <= 0.05, share
    for prefix in ('nerf_mlp', 'prop_mlp_0'):
        for k in ('normal_layer.weight', 'normal_layer.bias', 'density_layer.0.weight', 'density_layer.0.bias', 'density_layer.2.weight',
                  'density_layer.2.bias', 'encoder.embeddings'):
            grad = model.get_parameter(f'{prefix}.{k}').grad
            assert grad is not None and float(grad.abs().sum()) > 0, (prefix, k)
            out[f'grad_{prefix}.{k}'] = grad

    # MLP.forward on explicit Gaussians: [37 rays, 3 samples, 6 Gaussians]
    g = torch.Generator().manual_seed(2028)
    means = torch.rand(N_RAYS, 3, 6, 3, generator=g) * 3 - 1.5
    stds = torch.rand(N_RAYS, 3, 6, generator=g) * 0.09 + 0.01
    glo = half(torch.randn(N_RAYS, 4, generator=g) * 0.5)
    out.update(F_means=means, F_stds=stds, F_glo=glo)
    with torch.no_grad():
        for name, mlp, gv in (('prop', model.prop_mlp_0, None), ('nerf', model.nerf_mlp, glo)):
            res = mlp(False, means, stds, viewdirs=batch['viewdirs'], glo_vec=gv)
            for k in ('grad_pred', 'normals_pred', 'density', 'rgb'):
                out[f'F_{name}_{k}'] = res[k]
    mg.save('pred_normals.npz', **mg.npify(out))


if __name__ == '__main__':
    main()
