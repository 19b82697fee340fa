"""torch-CPU restatement of `MLP.scale_featurization` (ref models.py:436-437, :495-506), on top of oracle/raymarch.py.

TEST INFRASTRUCTURE ONLY.  Per sample of a field with L grid levels:
    w[j, l]          = erf(1 / sqrt(8 std_j^2 grid_sizes[l]^2))              the damping the gather applies (level_damping)
    k[l]             = sqrt(init_std^2 + mean over level l's rows of sum_c embeddings[row, c]^2)      no_grad, fp32 table
    scale_feature[l] = (2 mean_j w[j, l] - 1) k[l]
    density input    = cat([damped grid features (L*C), scale features (L)])
Pinned against the reference's own Python by tests/golden/{model,train_step}_scalefeat*.npz (make_scalefeat_golden.py).
"""
import contextlib

import torch
import torch.nn.functional as F

import helpers as H
from oracle import raymarch as rm

INIT_STD = 1e-4            # GridEncoder's default (gridencoder/grid.py), which MLP.__init__ does not override


def fields_of(spec):
    return list(spec.props[:spec.num_levels - 1]) + [spec.nerf]


def level_scale(fs, emb, init_std=INIT_STD):
    """k [L] in the reference's arithmetic: torch_scatter.segment_coo(mean) restated as an fp32 index_add and a division by the
    row count (models.py:499-505)."""
    _, _, _, idx = fs.layout()
    L = fs.num_grid_levels
    with torch.no_grad():
        sq = (emb.detach() ** 2).sum(-1)
        acc = torch.zeros(L, dtype=sq.dtype).index_add_(0, idx.long(), sq)
        cnt = torch.zeros(L, dtype=sq.dtype).index_add_(0, idx.long(), torch.ones_like(sq)).clamp_min(1)
        return (init_std ** 2 + acc / cnt).sqrt()


def scale_features(fs, emb, stds):
    """stds [..., G]: the (contracted, halved) Gaussians the gather damps with -> [..., L]."""
    _, _, grid_sizes, _ = fs.layout()
    return (2 * rm.level_damping(stds, grid_sizes).mean(dim=-2) - 1) * level_scale(fs, emb)


def field_density_features(fs, sd, means, stds, no_warp=False):
    """oracle.raymarch.field_density_features with the scale features appended to the density MLP's input; same returns
    (the last one, `feat`, is the widened input [..., L*C + L])."""
    pls, offsets, grid_sizes, _ = fs.layout()
    if not no_warp:
        flat_m, flat_s = rm.contract_points(means.reshape(-1, 3), stds.reshape(-1))
        means = flat_m.reshape(means.shape) / 2
        stds = flat_s.reshape(stds.shape) / 2
    emb = sd[fs.prefix + '.encoder.embeddings']
    pts01 = ((means + 1) / 2).reshape(-1, 3)
    feat = rm._GridEncodeCPU.apply(pts01, emb, offsets, pls, fs.grid_base_resolution)
    feat = feat.reshape(means.shape[:-1] + (fs.num_grid_levels, fs.grid_level_dim))
    damp = rm.level_damping(stds, grid_sizes)
    feat = (feat * damp[..., None]).mean(dim=-3).flatten(-2, -1)
    feat = torch.cat([feat, (2 * damp.mean(dim=-2) - 1) * level_scale(fs, emb)], dim=-1)
    h = F.relu(rm._lin(feat, sd, fs.prefix + '.density_layer.0'))
    x = rm._lin(h, sd, fs.prefix + '.density_layer.2')
    return x[..., 0], x, means.mean(dim=-2), feat


@contextlib.contextmanager
def featurized():
    """Inside the block oracle.raymarch's fields (field_forward, hence model_forward's level loop) run with scale
    featurization: they look `field_density_features` up in their module, which this swaps for the one above."""
    saved = rm.field_density_features
    # this only works while rm.field_forward resolves the name as a module global at call time; if the oracle is ever
    # refactored to bind it differently these tests would silently become flag-off tests, hence the assert
    assert "field_density_features" in rm.field_forward.__code__.co_names and rm.field_forward.__globals__ is vars(rm)
    rm.field_density_features = field_density_features
    try:
        yield
    finally:
        rm.field_density_features = saved


def model_forward(spec, sd, batch, noise, **kw):
    with featurized():
        return rm.model_forward(spec, sd, batch, noise, **kw)


def state_for(fx, spec, extra='stored'):
    """The fixture's state: init_state's weights (seed + checksum) with each field's L extra input columns of density_layer.0
    appended -- extra='stored': the fixture's; 'zero': zero columns; None: not appended (the flag-off model on the same
    remaining weights)."""
    sd = H.state_for(fx, spec)
    if extra is None:
        return sd
    for fs in fields_of(spec):
        name = fs.prefix + '.density_layer.0.'
        cols = fx['sf_' + name + 'extra'].float()
        sd[name + 'weight'] = torch.cat([sd[name + 'weight'], cols if extra == 'stored' else torch.zeros_like(cols)], dim=1)
    return sd


def hip_model(spec, sd, on=True, device='cuda', **model_kw):
    """helpers.hip_model with `scale_featurization` bound on both field classes."""
    from ucnerf_amd.internal import models
    with models.bindings(NerfMLP=dict(scale_featurization=on), PropMLP=dict(scale_featurization=on)):
        return H.hip_model(spec, sd, device=device, **model_kw)
