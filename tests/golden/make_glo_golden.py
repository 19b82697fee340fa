"""Generate tests/golden/{model_glo,train_step_glo}.npz: the REFERENCE's Model with GLO appearance codes, on CPU.

    python tests/golden/make_glo_golden.py          (authoring container only)

Same harness as make_golden.py (ref_import: the reference's own Python, the grid op restated in C), on the `tiny` spec
with Model.num_glo_features = 4 and num_glo_embeddings = spec.training_views, set as class attributes around
build_reference_model the way gin would bind them.  The field weights come from oracle.raymarch.init_state (seed +
checksum, like every other fixture); the GLO weights (glo_vecs, nerf_mlp.lin_glo_*) are drawn here from a seeded
generator and stored IN FULL under 'glo_<state-dict key>' (float16, exact).  Both fixtures also record the reference's state-dict keys,
shapes and order ('sd_keys' newline-joined as uint8, 'sd_shapes' flattened with 'sd_ndims').

  model_glo.npz       Model.forward eval (rand=False) on fixed rays with zero_glo=True ('Z1_' keys) and zero_glo=False ('Z0_')
  train_step_glo.npz  one training step, rand=True, zero_glo=False, all draws captured (as make_golden.gen_train_step),
                      loss terms and gradient digests including glo_vecs.weight and nerf_mlp.lin_glo_*
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

NUM_GLO = 4


def glo_weights(spec, seed):
    """Seeded GLO parameters, scaled so that exp(scale) / shift move the bottleneck visibly (|scale| ~ 0.2).  Multiples of
    2^-9 stored as float16 (exact): the 512 x 128 matrix then costs ~60 KB of fixture instead of 240."""
    g = torch.Generator().manual_seed(seed)
    width, nb = 128, spec.nerf.bottleneck_width
    q = lambda t: (torch.round(t * 512) / 512).half()
    return {
        'glo_vecs.weight': q(torch.randn(spec.training_views, NUM_GLO, generator=g)),
        'nerf_mlp.lin_glo_0.weight': q(torch.rand(width, NUM_GLO, generator=g) - 0.5),
        'nerf_mlp.lin_glo_0.bias': q((torch.rand(width, generator=g) - 0.5) * 0.5),
        'nerf_mlp.lin_glo_1.weight': q(torch.randn(2 * nb, width, generator=g) * 0.05),
        'nerf_mlp.lin_glo_1.bias': q(torch.randn(2 * nb, generator=g) * 0.1),
    }


def build(ref, spec, seed, glo_seed):
    sd = rm.init_state(spec, seed=seed)
    glo = glo_weights(spec, glo_seed)
    # the reference reads Model.num_glo_features from the CLASS in forward too (models.py:118): the binding stays for the
    # whole generating process, like a gin binding
    M = ref.models.Model
    M.num_glo_features, M.num_glo_embeddings = NUM_GLO, spec.training_views
    model, cfg = ref_import.build_reference_model(ref, spec, dict(sd, **{k: v.float() for k, v in glo.items()}))
    keys = list(model.state_dict().keys())
    shapes = [tuple(v.shape) for v in model.state_dict().values()]
    out = dict(seed=torch.tensor(seed), checksum=torch.tensor(mg.state_checksum(sd), dtype=torch.float64),
               sd_keys=torch.tensor(np.frombuffer('\n'.join(keys).encode(), dtype=np.uint8).copy()),
               sd_ndims=torch.tensor([len(s) for s in shapes]),
               sd_shapes=torch.tensor([d for s in shapes for d in s], dtype=torch.long))
    out.update({'glo_' + k: v for k, v in glo.items()})
    return model, cfg, out


def gen_model_glo(ref):
    spec = rm.make_spec('tiny')
    model, cfg, out = build(ref, spec, 91, 92)
    n = 32
    batch = rm.synthetic_rays(n, seed=93)
    batch['cam_idx'] = torch.randint(0, spec.training_views, (n, 1), generator=torch.Generator().manual_seed(94))
    out.update({'ray_' + k: v for k, v in batch.items()})
    model.eval()
    for tag, zero_glo in (('Z1_', True), ('Z0_', False)):
        torch.manual_seed(95)
        with ref_import.capture_rng() as cap, torch.no_grad():
            rend, hist = model(False, dict(batch), train_frac=1.0, compute_extras=True, zero_glo=zero_glo)
        assert len(cap.draws) == spec.num_levels
        for lvl in range(spec.num_levels):
            out[f'{tag}noise{lvl}_rand_vec'] = cap.draws[lvl][1]
            for k in ('rgb', 'depth', 'acc', 'weights'):
                out[f'{tag}L{lvl}_{k}'] = rend[lvl][k]
            for k in ('sdist', 'density', 'rgb'):
                out[f'{tag}L{lvl}_hist_{k}'] = hist[lvl][k]
    d = (out['Z1_L1_rgb'] - out['Z0_L1_rgb']).abs().max()
    assert d > 1e-2, float(d)               # the per-image codes do change the pixels
    mg.save('model_glo.npz', **mg.npify(out))


def gen_train_step_glo(ref):
    spec = rm.make_spec('tiny')
    model, cfg, out = build(ref, spec, 101, 102)
    model.train()
    n = 80
    seed = 101
    rays = rm.synthetic_rays(n, seed=seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    rays['rgb'] = torch.rand(n, 3, generator=g)
    rays['cam_idx'] = torch.randint(0, spec.training_views, (n, 1), generator=g)
    rays['sky_segs'] = (torch.rand(n, generator=g) > 0.7).float()
    batch = {k: (v[:, None, None, :] if v.dim() == 2 else v[:, None, None]) for k, v in rays.items()}
    train_frac = 0.4
    torch.manual_seed(seed + 3)
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
        out[f'L{lvl}_rgb'] = rend[lvl]['rgb']
    for k, v in losses.items():
        out['loss_' + k] = v.detach().double()
    out['loss_total'] = total.detach().double()
    gg = torch.Generator().manual_seed(seed + 4)
    for pname, p in model.named_parameters():
        if p.grad is not None:
            mg.grad_digest('grad_' + pname, p.grad, out, gg)
    assert float(model.glo_vecs.weight.grad.abs().sum()) > 0
    mg.save('train_step_glo.npz', **mg.npify(out))


if __name__ == '__main__':
    ref = ref_import.load()
    torch.set_num_threads(1)              # fixed reduction order for the generating run
    gen_model_glo(ref)
    gen_train_step_glo(ref)
