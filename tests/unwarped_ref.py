"""Plain-torch restatement of the unwarped march (MLP.warp_fn = None, ref models.py:488-494 / coord.py:93-96): the oracle's
Model.forward (oracle/raymarch.py) with every field evaluated on the Gaussians as cast -- no contraction, no halving, grid
coordinate u = (x + 1) / 2, damping from the cast std, `coord` the plain mean of the six means.  Points outside [-1, 1]^3 get zero
grid features from the grid op (bounds inclusive) and still count in the mean of six.

TEST INFRASTRUCTURE ONLY.  The oracle's fields already know `no_warp` (predict_density's flag); its Model.forward does not pass it,
so `field_forward` and `field_density_features` are bound around the call (`unwarped_fields`).  Dtype follows the inputs: a float32
state and batch give the float32 restatement (the oracle's C grid op, as everywhere); a `.double()` state and batch give the float64
one, whose grid is oracle/truth64.py's torch gather -- differentiable in the table, so autograd of a float64 training step reaches
every parameter (`train_step`)."""
import contextlib
import functools

import torch
import torch.nn.functional as F

from oracle import raymarch as rm
from oracle import truth64 as t64


def field_density_features(fs, sd, means, stds, no_warp=True):
    """oracle.raymarch.field_density_features without the warp, in the dtype of the state: (raw density, x, coord, features)."""
    emb = sd[fs.prefix + '.encoder.embeddings']
    if emb.dtype != torch.float64:
        return _ORACLE_FEATURES(fs, sd, means, stds, True)
    feat, _, _ = t64.sample_features(fs, emb, means, stds, no_warp=True)
    feat = feat.flatten(-2, -1)
    h = F.relu(rm._lin(feat, sd, fs.prefix + '.density_layer.0'))
    x = rm._lin(h, sd, fs.prefix + '.density_layer.2')
    return x[..., 0], x, means.mean(dim=-2), feat


_ORACLE_FEATURES = rm.field_density_features


@contextlib.contextmanager
def unwarped_fields():
    # this only works while rm.model_forward / rm.field_forward resolve the two names as module globals at call time; if the oracle
    # is ever refactored to bind them differently these would silently become warped runs, hence the asserts
    assert "field_forward" in rm.model_forward.__code__.co_names and rm.model_forward.__globals__ is vars(rm)
    assert "field_density_features" in rm.field_forward.__code__.co_names and rm.field_forward.__globals__ is vars(rm)
    saved = (rm.field_forward, rm.field_density_features)
    rm.field_forward = functools.partial(saved[0], no_warp=True)
    rm.field_density_features = field_density_features
    try:
        yield
    finally:
        rm.field_forward, rm.field_density_features = saved


@contextlib.contextmanager
def unwarped_truth():
    """oracle/truth64.level_forward (one level at given fenceposts, float64) on an unwarped field."""
    assert "field_forward" in t64.level_forward.__code__.co_names and t64.level_forward.__globals__ is vars(t64)
    saved = t64.field_forward
    t64.field_forward = functools.partial(saved, no_warp=True)
    try:
        yield
    finally:
        t64.field_forward = saved


def model_forward(spec, sd, batch, noise, **kw):
    with unwarped_fields():
        return rm.model_forward(spec, sd, batch, noise, **kw)


def train_step(spec, sd, rays, noise, train_frac, losses_of, dtype=torch.float32):
    """One training step of the restatement in `dtype`, as tests/test_train_step.py::test_oracle_autograd_matches_reference_gradients
    runs the oracle's: forward with training=True, the project's loss functions (`losses_of(batch, rend, hist)` -> dict), backward.
    rays: the flat batch (fixture 'ray_*').  Returns (losses {name: float}, grads {parameter: tensor})."""
    cast = lambda v: v.to(dtype) if v.is_floating_point() else v
    params = {k: cast(v).clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    state = dict(sd)
    state.update(params)
    flat = {k: cast(v) for k, v in rays.items()}
    nz = [rm.LevelNoise(**{f: (None if getattr(n, f) is None else cast(getattr(n, f))) for f in ('rand_vec', 'jitter', 'flip', 'spin')})
          for n in noise]
    rend, hist = model_forward(spec, state, flat, nz, train_frac=train_frac, compute_extras=False, training=True)
    batch = {k: (v[:, None, None, :] if v.dim() == 2 else v[:, None, None]) for k, v in flat.items()}
    rend = [{k: (v[:, None, None] if torch.is_tensor(v) else v) for k, v in r.items()} for r in rend]
    hist = [{k: (v[:, None, None] if torch.is_tensor(v) and v.dim() >= 1 and k != 'loss_hash_decay' else v) for k, v in h.items()}
            for h in hist]
    losses = losses_of(batch, rend, hist)
    sum(losses.values()).backward()
    return {k: float(v.detach()) for k, v in losses.items()}, {k: p.grad.detach() for k, p in params.items() if p.grad is not None}


def inside_cube(means):
    """[..., 3] world-space means -> bool: inside [-1, 1]^3, bounds inclusive (the grid op's own test on u in [0, 1])."""
    u = (means + 1) / 2
    return ((u >= 0) & (u <= 1)).all(dim=-1)


def grid_inputs(means, stds):
    """What the unwarped grid is handed for cast Gaussians: (u [..., 3], 1 / sqrt(8 std^2) [...])."""
    return (means + 1) / 2, 1 / torch.sqrt(8 * stds ** 2)
