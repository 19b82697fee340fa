"""Generate tests/golden/ref_colour.npz: the REFERENCE's Ref-NeRF colour heads (MLP.use_diffuse_color, use_specular_tint,
enable_pred_roughness), on CPU.

    python tests/golden/make_ref_colour_golden.py          (authoring container only)

Same harness as make_pred_normals_golden.py (ref_import: the reference's own Python, the grid op restated in C).  One two-level Model,
64-wide bottleneck and colour layers, disable_rgb = False on both fields:

  prop_mlp_0   level_dim 2, L = 3 levels, scale_featurization, T = 2^8, use_diffuse_color only
  nerf_mlp     level_dim 4, L = 4 levels, GLO (num_glo_features 4), T = 2^9, all three flags plus enable_pred_normals,
               rgb_premultiplier 1.5, rgb_bias 0.25

37 rays x 13 proposal and 24 NeRF samples (N*S no multiple of 64).  EVERY parameter is drawn here from a seeded generator as a
float16-representable value and stored in full under 'sd_<state-dict key>' (float16, exact); the tables are U(-1, 1).  The diffuse and rgb
biases are spread per channel so that the network's own samples reach the clipped region (linear colour above 1) as well as the power part;
the share is printed.

Contents: the state dict's keys / shapes / order; the rays and the pinned draws (rand = False: the cone basis' randn per level); per level
density_layer's input features, the raw head outputs, rgb, roughness, density, weights, sdist, the composited rgb and roughness
(compute_extras); the loss sum_levels <composited rgb, G_level> with stored random cotangents G and its gradients with respect to every
parameter and both tables.  The march runs with zero_glo = True.  'F_' keys: MLP.forward of both fields on explicit Gaussians (the NeRF
field with and without per-ray GLO codes).  'E_' keys: a crafted elementwise set for the colour function -- 512 triples of colour logits,
raw diffuse and raw tint logits covering the toe part (l <= 0.0031308), the power part and the clipped region (l > 1) with at least 10 %
each and no element within 1e-4 of 0.0031308 or 1e-3 of 1 (asserted in float64, with and without the tint) -- with the reference's values and
gradients under a stored cotangent, through the reference's image.linear_to_srgb.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402
import ref_import  # noqa: E402
from oracle import raymarch as rm  # noqa: E402
import ref_colour_ref as rc  # noqa: E402  (the architecture's constants only)

N_RAYS = 37
N_CRAFTED = 512


def half(t):
    return t.half().float()


def draw_state(model, seed):
    """Every parameter as a float16-representable draw: tables U(-1, 1), Linear layers U(+-1/sqrt(fan_in)) (the colour layers
    U(+-sqrt(6/fan_in)), the GLO layers small); the diffuse, tint and rgb biases spread per channel."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, p in model.named_parameters():
        u = torch.rand(p.shape, generator=g) * 2 - 1
        if k.endswith('embeddings'):
            v = u
        elif k.endswith('diffuse_layer.bias'):
            # channel 0 straddles a linear colour of 1 (the clip) on both fields: 0.62 + 0.73 * 0.56 (tint), 0.79 + 0.5 * 0.41 (no tint)
            v = torch.tensor([2.45 if k.startswith('prop') else 1.6, 0.75, -1.5]) + 0.05 * u
        elif k.endswith('specular_layer.bias'):
            v = torch.tensor([1.0, 0.0, -1.0]) + 0.05 * u
        elif k.endswith('rgb_layer.bias'):
            v = torch.tensor([0.0, 0.25, -0.75]) + 0.05 * u
        elif k.endswith('normal_layer.bias'):
            v = torch.tensor([0.8, 0.5, -0.25]) + 0.05 * u
        elif 'lin_glo' in k or k.startswith('glo_vecs'):
            v = 0.3 * u
        else:
            fan_in = p.shape[-1] if p.dim() == 2 else model.get_parameter(k[:-4] + 'weight').shape[-1]
            v = u * ((6.0 / fan_in) ** 0.5 if 'lin_second_stage' in k and p.dim() == 2 else fan_in ** -0.5)
        sd[k] = half(v)
    return sd


def crafted_set(ref, kw):
    """512 x 3 logits in three regimes; elements too close to a branch point are redrawn (float64 decides)"""
    g = torch.Generator().manual_seed(2031)
    shape = (N_CRAFTED, 3)
    regime = torch.randint(0, 10, shape, generator=g)          # 0-1 toe, 2-4 clipped, 5-9 power
    u = lambda: torch.rand(shape, generator=g)
    z = torch.where(regime < 2, -9.0 - 3 * u(), torch.where(regime < 5, 2.0 + 3 * u(), -3.0 + 5 * u()))
    rd = torch.where(regime < 2, -7.5 - 3 * u(), torch.where(regime < 5, 2.5 + 3 * u(), -4.0 + 4.5 * u()))
    rt = torch.where(regime < 2, -2.0 + 4 * u(), torch.where(regime < 5, 2.5 + 3 * u(), -3.0 + 6 * u()))
    z, rd, rt = half(z), half(rd), half(rt)

    def lin64(tint):
        s = torch.sigmoid(kw['premultiplier'] * z.double() + kw['bias'])
        return (torch.sigmoid(rt.double()) if tint else 0.5) * s + torch.sigmoid(rd.double() - math.log(3.0))
    for _ in range(64):
        bad = torch.zeros(shape, dtype=torch.bool)
        for tint in (True, False):
            l = lin64(tint)
            bad |= ((l - rc.TOE).abs() < 1e-4) | ((l - 1.0).abs() < 1e-3)
            # linear_to_srgb(l) = 1 at l = 1 exactly: the clip's edge is the same point
        if not bad.any():
            break
        rd = torch.where(bad, half(rd + 0.25 * (torch.rand(shape, generator=g) - 0.5)), rd)
    assert not bad.any()
    for tint in (True, False):
        l = lin64(tint)
        shares = [float((l <= rc.TOE).double().mean()), float(((l > rc.TOE) & (l < 1)).double().mean()), float((l > 1).double().mean())]
        print(f'crafted set, tint {tint}: toe {shares[0]:.3f} power {shares[1]:.3f} clipped {shares[2]:.3f}')
        assert min(shares) >= 0.10, shares
    G = torch.rand(shape, generator=g) - 0.5
    out = dict(E_logits=z, E_raw_diffuse=rd, E_raw_tint=rt, E_G=G)
    image = ref.models.image
    for tint in (True, False):
        a, b, c = (t.clone().requires_grad_(True) for t in (z, rd, rt))
        # models.py:657-674, literally, on the reference's linear_to_srgb
        rgb = torch.sigmoid(kw['premultiplier'] * a + kw['bias'])
        diffuse_linear = torch.sigmoid(b - np.log(3.0))
        specular_linear = torch.sigmoid(c) * rgb if tint else 0.5 * rgb
        rgb = torch.clip(image.linear_to_srgb(specular_linear + diffuse_linear), 0.0, 1.0)
        rgb = rgb * (1 + 2 * rc.PADDING) - rc.PADDING
        rgb.backward(G)
        tag = 'tint' if tint else 'notint'
        out.update({f'E_{tag}_rgb': rgb.detach(), f'E_{tag}_g_logits': a.grad, f'E_{tag}_g_raw_diffuse': b.grad})
        if tint:
            out['E_tint_g_raw_tint'] = c.grad
    return out


def main():
    ref = ref_import.load()
    torch.set_num_threads(1)              # fixed reduction order for the generating run
    M = ref.models
    for cls, attrs in ((M.NerfMLP, rc.NERF), (M.PropMLP, rc.PROP), (M.Model, rc.MODEL)):
        for k, v in attrs.items():       # bound for the whole generating process, like gin bindings
            setattr(cls, k, v)
    cfg = ref.configs.Config()
    model = M.Model(config=cfg)
    assert model.nerf_mlp.rgb_padding == rc.PADDING and model.nerf_mlp.roughness_bias == rc.ROUGHNESS_BIAS
    sd = draw_state(model, 2030)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    buffers = {k for k, _ in model.named_buffers()}                  # the encoders' offsets / idx / grid_sizes: derived, not drawn
    assert not unexpected and set(missing) <= buffers, (missing, unexpected)
    keys = list(model.state_dict().keys())
    shapes = [tuple(v.shape) for v in model.state_dict().values()]
    out = dict(sd_keys=torch.tensor(np.frombuffer('\n'.join(keys).encode(), dtype=np.uint8).copy()),
               sd_ndims=torch.tensor([len(s) for s in shapes]),
               sd_shapes=torch.tensor([d for s in shapes for d in s], dtype=torch.long))
    out.update({'sd_' + k: v.half() for k, v in sd.items()})

    batch = rm.synthetic_rays(N_RAYS, seed=2025)
    batch['cam_idx'] = torch.randint(0, 8, (N_RAYS, 1), generator=torch.Generator().manual_seed(2026))
    out.update({'ray_' + k: v for k, v in batch.items()})
    model.train()
    torch.manual_seed(2027)
    feats, raws = {}, {}
    hooks = []
    for lvl, m in ((0, model.prop_mlp_0), (1, model.nerf_mlp)):
        hooks.append(m.density_layer.register_forward_hook(lambda mod, inp, res, k=lvl: feats.__setitem__(k, inp[0].detach().clone())))
        for key, name in (('raw_diffuse', 'diffuse_layer'), ('raw_tint', 'specular_layer'), ('raw_roughness', 'roughness_layer')):
            if hasattr(m, name):
                hooks.append(getattr(m, name).register_forward_hook(
                    lambda mod, inp, res, k=(lvl, key): raws.__setitem__(k, res.detach().clone())))
    with ref_import.capture_rng() as cap:
        rend, hist = model(False, dict(batch), train_frac=1.0, compute_extras=True, zero_glo=True)
    for h in hooks:
        h.remove()
    assert len(cap.draws) == 2
    g = torch.Generator().manual_seed(2029)
    loss = 0.0
    for lvl in range(2):
        out[f'G{lvl}'] = torch.rand(N_RAYS, 3, generator=g) - 0.5
        loss = loss + (rend[lvl]['rgb'] * out[f'G{lvl}']).sum()
    loss.backward()
    out['loss'] = loss.detach().double()
    for lvl in range(2):
        out[f'noise{lvl}_rand_vec'] = cap.draws[lvl][1]
        for k in ('weights', 'sdist', 'density', 'rgb', 'roughness'):
            if hist[lvl][k] is not None:
                out[f'L{lvl}_{k}'] = hist[lvl][k].detach()
        for (l, key), v in raws.items():
            if l == lvl:
                out[f'L{lvl}_{key}'] = v
        out[f'L{lvl}_features'] = feats[lvl]                   # density_layer's input [37, S, L*C (+ L scale features)]
        out[f'L{lvl}_render_rgb'] = rend[lvl]['rgb'].detach()
        if 'roughness' in rend[lvl]:
            out[f'L{lvl}_render_roughness'] = rend[lvl]['roughness'].detach()
        unpadded = (hist[lvl]['rgb'].detach().double() + rc.PADDING) / (1 + 2 * rc.PADDING)
        print(f'level {lvl}: clipped (colour at 1) on {100 * float((unpadded >= 1 - 1e-7).double().mean()):.1f} % of the channels, '
              f'median colour {float(unpadded.median()):.3f}')
        share0 = float((unpadded[..., 0] >= 1 - 1e-7).double().mean())
        q = torch.quantile(unpadded[..., 0].reshape(-1), torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64)).tolist()
        print(f'level {lvl}: channel 0 clipped on {100 * share0:.1f} % of the samples (colour quantiles 10/50/90 %: {q[0]:.3f} {q[1]:.3f} {q[2]:.3f})')
        assert 0.1 <= share0 <= 0.9, share0                            # the clip is exercised on both sides
    assert 'L1_roughness' in out and out['L1_roughness'].shape == (N_RAYS, 24, 1) and 'L0_roughness' not in out
    assert out['L1_render_roughness'].shape == (N_RAYS, 1)
    for k, p in model.named_parameters():
        if k.startswith('glo_vecs'):
            continue
        if 'roughness_layer' in k or 'normal_layer' in k:          # no consumer on the path: no gradient from this loss
            assert p.grad is None or float(p.grad.abs().sum()) == 0.0
            continue
        # (lin_glo_0.weight: its input is the zero code, its gradient an exact zero; stored like the others)
        assert p.grad is not None and (float(p.grad.abs().sum()) > 0 or k.endswith('lin_glo_0.weight')), k
        out[f'grad_{k}'] = p.grad

    # MLP.forward on explicit Gaussians: [37 rays, 3 samples, 6 Gaussians]
    g = torch.Generator().manual_seed(2028)
    means = torch.rand(N_RAYS, 3, 6, 3, generator=g) * 3 - 1.5
    stds = torch.rand(N_RAYS, 3, 6, generator=g) * 0.09 + 0.01
    glo = half(torch.randn(N_RAYS, 4, generator=g) * 0.5)
    out.update(F_means=means, F_stds=stds, F_glo=glo)
    with torch.no_grad():
        for name, mlp, gv in (('prop', model.prop_mlp_0, None), ('nerf', model.nerf_mlp, None), ('nerfglo', model.nerf_mlp, glo)):
            feats.clear()
            hook = mlp.density_layer.register_forward_hook(lambda mod, inp, res: feats.__setitem__('F', inp[0].detach().clone()))
            res = mlp(False, means, stds, viewdirs=batch['viewdirs'], glo_vec=gv)
            hook.remove()
            out[f'F_{name}_features'] = feats['F']
            for k in ('density', 'rgb', 'roughness'):
                if res[k] is not None:
                    out[f'F_{name}_{k}'] = res[k]
    out.update(crafted_set(ref, rc.head_kw('nerf_mlp')))
    mg.save('ref_colour.npz', **mg.npify(out))


if __name__ == '__main__':
    main()
