"""Generate tests/golden/{model_scalefeat,model_scalefeat_R,train_step_scalefeat}.npz: the REFERENCE's Model with
`scale_featurization = True` on both fields (models.py:436-437, :495-506), on CPU.

    python tests/golden/make_scalefeat_golden.py          (authoring container only)

Same harness as make_golden.py / make_glo_golden.py (ref_import: the reference's own Python, the grid op restated in C, torch_scatter's
segment_coo restated over index_add).  `NerfMLP.scale_featurization` and `PropMLP.scale_featurization` are set as class attributes the
way gin would bind them; the reference reads them through `self` in predict_density too, so the binding spans the forward.  The field
weights come from oracle.raymarch.init_state (seed + checksum), which draws density_layer.0 with L*C input columns; the L extra columns
of each field are drawn here from a seeded generator and stored IN FULL under 'sf_<field>.density_layer.0.extra' (float16, exact): the
layer's weight is cat([init_state's columns, extra], dim=1).  Every fixture records the reference's state-dict keys, shapes and order.

  model_scalefeat.npz       Model.forward eval (rand=False), spec `tiny`  (NeRF L=16 C=2, proposal L=6 C=2), 32 rays
  model_scalefeat_R.npz     the same on spec `tinyR` (L=10 C=4 and L=6 C=4: L is no multiple of C)
  train_step_scalefeat.npz  one training step on `tiny`, rand=True, all draws captured, loss terms and gradient digests, 80 rays
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import ref_import  # noqa: E402
from oracle import raymarch as rm  # noqa: E402


def fields_of(spec):
    return list(spec.props[:spec.num_levels - 1]) + [spec.nerf]


def extra_columns(spec, seed):
    """Seeded weights of the L scale-feature inputs of every field's density_layer.0: multiples of 2^-9 in [-0.25, 0.25],
    stored as float16 (exact) -- the size of the layer's own initial weights (bound 1/sqrt(L*C) = 0.18 .. 0.29)."""
    g = torch.Generator().manual_seed(seed)
    return {f'{fs.prefix}.density_layer.0.extra': (torch.round((torch.rand(64, fs.num_grid_levels, generator=g) - 0.5) * 256) / 512).half()
            for fs in fields_of(spec)}


def widened(sd, extra):
    out = dict(sd)
    for k, v in extra.items():
        name = k[:-len('extra')] + 'weight'
        out[name] = torch.cat([sd[name], v.float()], dim=1)
    return out


@contextlib.contextmanager
def binding(ref, on):
    classes = (ref.models.NerfMLP, ref.models.PropMLP)
    saved = [c.__dict__.get('scale_featurization') for c in classes]
    for c in classes:
        c.scale_featurization = on
    try:
        yield
    finally:
        for c, old in zip(classes, saved):
            if old is None:
                delattr(c, 'scale_featurization')
            else:
                c.scale_featurization = old


def build(ref, spec, seed, extra_seed):
    """(model, cfg, fixture header); call inside `binding(ref, True)`."""
    sd = rm.init_state(spec, seed=seed)
    extra = extra_columns(spec, extra_seed)
    model, cfg = ref_import.build_reference_model(ref, spec, widened(sd, extra))
    keys = list(model.state_dict().keys())
    shapes = [tuple(v.shape) for v in model.state_dict().values()]
    for fs in fields_of(spec):
        L, C = fs.num_grid_levels, fs.grid_level_dim
        assert shapes[keys.index(fs.prefix + '.density_layer.0.weight')] == (64, L * C + L)
    out = dict(seed=torch.tensor(seed), checksum=torch.tensor(mg.state_checksum(sd), dtype=torch.float64),
               sd_keys=torch.tensor(np.frombuffer('\n'.join(keys).encode(), dtype=np.uint8).copy()),
               sd_ndims=torch.tensor([len(s) for s in shapes]),
               sd_shapes=torch.tensor([d for s in shapes for d in s], dtype=torch.long))
    out.update({'sf_' + k: v for k, v in extra.items()})
    return model, cfg, out, sd


def gen_model(ref, name, kind, seed):
    spec = rm.make_spec(kind)
    n = 32
    batch = rm.synthetic_rays(n, seed=seed + 2)
    with binding(ref, True):
        model, cfg, out, sd = build(ref, spec, seed, seed + 1)
        out.update({'ray_' + k: v for k, v in batch.items()})
        out['train_frac'] = torch.tensor(1.0)
        model.eval()
        torch.manual_seed(seed + 3)
        with ref_import.capture_rng() as cap, torch.no_grad():
            rend, hist = model(False, dict(batch), train_frac=1.0, compute_extras=True, zero_glo=True)
    assert len(cap.draws) == spec.num_levels
    for lvl in range(spec.num_levels):
        out[f'noise{lvl}_rand_vec'] = cap.draws[lvl][1]
        for k in ('rgb', 'depth', 'acc', 'weights'):
            out[f'L{lvl}_{k}'] = rend[lvl][k]
        for k in ('sdist', 'weights', 'density', 'rgb', 'coord'):
            out[f'L{lvl}_hist_{k}'] = hist[lvl][k]
    # the same weights without the feature, on the same draws: the fixture is not vacuous
    with binding(ref, False):
        plain, _ = ref_import.build_reference_model(ref, spec, sd)
        plain.eval()
        torch.manual_seed(seed + 3)
        with torch.no_grad():
            rend0, _ = plain(False, dict(batch), train_frac=1.0, compute_extras=True, zero_glo=True)
    last = spec.num_levels - 1
    d = (rend0[last]['rgb'] - out[f'L{last}_rgb']).abs().max()
    assert d > 1e-2, float(d)
    print(f'{name}: scale features move the last level\'s rgb by {float(d):.3f}')
    mg.save(name, **mg.npify(out))


def gen_train_step(ref):
    spec = rm.make_spec('tiny')
    seed = 131
    n = 80
    rays = rm.synthetic_rays(n, seed=seed + 2)
    g = torch.Generator().manual_seed(seed + 3)
    rays['rgb'] = torch.rand(n, 3, generator=g)
    rays['cam_idx'] = torch.randint(0, spec.training_views, (n, 1), generator=g)
    rays['sky_segs'] = (torch.rand(n, generator=g) > 0.7).float()
    batch = {k: (v[:, None, None, :] if v.dim() == 2 else v[:, None, None]) for k, v in rays.items()}
    train_frac = 0.4
    with binding(ref, True):
        model, cfg, out, _ = build(ref, spec, seed, seed + 1)
        model.train()
        torch.manual_seed(seed + 4)
        with ref_import.capture_rng() as cap:
            rend, hist = model(True, dict(batch), train_frac=train_frac, compute_extras=False, zero_glo=False)
        tu = ref.train_utils
        losses = {}
        losses['data'], stats = tu.compute_data_loss(batch, rend, cfg)
        losses['anti_interlevel'] = tu.anti_interlevel_loss(hist, cfg)
        losses['distortion'] = tu.distortion_loss(hist, cfg)
        losses['hash_decay'] = tu.hash_decay_loss(hist, cfg)
        total = sum(losses.values())
        total.backward()
    out.update(train_frac=torch.tensor(train_frac), mse=torch.tensor(stats['mses']))
    out.update({'ray_' + k: v for k, v in rays.items()})
    assert len(cap.draws) == 4 * spec.num_levels
    for lvl in range(spec.num_levels):
        d = cap.draws[4 * lvl: 4 * lvl + 4]
        out[f'noise{lvl}_jitter'], out[f'noise{lvl}_flip'], out[f'noise{lvl}_spin'], out[f'noise{lvl}_rand_vec'] = [x[1] for x in d]
        out[f'L{lvl}_sdist'] = hist[lvl]['sdist']
        out[f'L{lvl}_weights'] = hist[lvl]['weights']
        out[f'L{lvl}_rgb'] = rend[lvl]['rgb']
    for k, v in losses.items():
        out['loss_' + k] = v.detach().double()
    out['loss_total'] = total.detach().double()
    gg = torch.Generator().manual_seed(seed + 5)
    for pname, p in model.named_parameters():
        if p.grad is not None:
            mg.grad_digest('grad_' + pname, p.grad, out, gg)
    for fs in fields_of(spec):
        gw = dict(model.named_parameters())[fs.prefix + '.density_layer.0.weight'].grad
        assert float(gw[:, fs.num_grid_levels * fs.grid_level_dim:].abs().sum()) > 0      # the extra columns do learn
    mg.save('train_step_scalefeat.npz', **mg.npify(out))


if __name__ == '__main__':
    ref = ref_import.load()
    torch.set_num_threads(1)              # fixed reduction order for the generating run
    gen_model(ref, 'model_scalefeat.npz', 'tiny', 111)
    gen_model(ref, 'model_scalefeat_R.npz', 'tinyR', 121)
    gen_train_step(ref)
