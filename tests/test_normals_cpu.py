"""Density normals (MLP.disable_density_normals = False), CPU side: the restatement tests/normals_ref.py against the oracle, its
float64 path against finite differences, and what the host accepts and refuses.

Golden fixture: tests/golden/normals_tiny.npz, the reference's own MLP.forward with no_warp=True (its grid.py backward over
oracle/grid_cpu.py returns the input gradients).  With the warp on the reference has nothing to give: it hands `means` to
coord.track_linearize, which is @torch.no_grad (coord.py:75), so its autograd.grad has no path to `means`; the warped restatement is
held by the forward parity and the gradcheck below."""
import numpy as np
import pytest
import torch

import normals_ref as nr
from oracle import raymarch as rm


def _points(n, seed, G=6):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 1, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    r = torch.cat([torch.rand(n // 2, generator=g), 1 + 29 * torch.rand(n - n // 2, generator=g)])
    means = d * r[:, None, None] + 0.01 * torch.randn(n, G, 3, generator=g)
    means[0] = 0.0
    stds = 10 ** (-4 + 4 * torch.rand(n, G, generator=g))
    return means, stds


def _small_field():
    fs = rm.FieldSpec('prop_mlp_0', grid_desired_resolution=64, grid_level_dim=2, grid_log2_hashmap_size=9, disable_rgb=True)
    spec = rm.make_spec('tiny')
    spec.props = [fs]
    return fs, rm.init_state(spec, seed=11)


@pytest.mark.parametrize("no_warp", [False, True])
def test_restatement_forward_matches_oracle(no_warp):
    spec = rm.make_spec('tiny')
    sd = rm.init_state(spec, seed=3)
    means, stds = _points(64, 1)
    if no_warp:
        means = means / 31
    for fs in (spec.props[0], spec.nerf):
        raw, _, coord, feat = rm.field_density_features(fs, sd, means, stds, no_warp)
        got, aux = nr.predict_density(fs, sd, means, stds, torch.float32, no_warp)
        assert (aux['feat'] - feat).abs().max() <= 1e-6
        assert (got - raw).abs().max() <= 1e-6 * max(1.0, float(raw.abs().max()))
        assert (aux['coord'] - coord).abs().max() <= 1e-6


def test_safe_contraction_is_the_oracles():
    means, stds = _points(256, 2)
    z, s = rm.contract_points(means.reshape(-1, 3), stds.reshape(-1))
    z2, s2 = nr.contract_points(means.reshape(-1, 3), stds.reshape(-1))
    assert torch.equal(z, z2) and torch.equal(s, s2)


def test_gradcheck_float64_interior():
    """autograd of the float64 path against central differences, at points at least 0.05 of a cell away from every lattice plane
    of every level (a perturbation of 1e-6 then stays inside the cell) and away from the unit sphere."""
    fs, sd = _small_field()
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    means, stds = _points(400, 5)
    means, stds = means.double(), stds.double().clamp_min(3e-3)            # keep the erf damping in its active range
    z, _ = nr.contract_points(means.reshape(-1, 3), stds.reshape(-1))
    u = (z / 2 + 1) / 2
    levels, _ = nr.locate(fs, u)
    ok = torch.ones(u.shape[0], dtype=torch.bool)
    for cell, frac, scale, _, _ in levels:
        f = u * scale + 0.5 - torch.from_numpy(cell)
        ok &= ((f > 0.05) & (f < 0.95)).all(dim=-1)
    r = means.reshape(-1, 3).norm(dim=-1)
    ok &= ((r - 1).abs() > 1e-3) & (r > 1e-3)
    keep = ok.reshape(-1, 6).all(dim=-1).nonzero().reshape(-1)[:6]
    assert keep.numel() >= 4, "the seed leaves too few interior samples"
    m = means[keep].clone().requires_grad_(True)
    fn = lambda mm: nr.predict_density(fs, sd, mm, stds[keep], torch.float64, exact_frac=True)[0]
    assert torch.autograd.gradcheck(fn, (m,), eps=1e-6, atol=1e-6, rtol=1e-4)
    # and the straight-through fraction the bracket tests use has the same derivative, up to the float32 rounding of its value:
    # pos <= 65 carries <= 2^-24 * 65 = 4e-6 of a cell, which moves the other two axes' weights by that much relative to 1
    (g1,) = torch.autograd.grad(fn(m).sum(), m)
    (g2,) = torch.autograd.grad(nr.predict_density(fs, sd, m, stds[keep], torch.float64)[0].sum(), m)
    assert (g1 - g2).abs().max() <= 1e-4 * g1.abs().max()


def test_normals_are_finite_at_the_origin_and_unit():
    fs, sd = _small_field()
    means, stds = _points(64, 7)
    out = nr.normals(fs, sd, means, stds)
    assert torch.isfinite(out['raw_grad_density']).all() and torch.isfinite(out['normals']).all()
    assert (out['normals'].norm(dim=-1) <= 1 + 1e-6).all()


# ------------------------------------------------------------------ host: what is accepted and refused
def test_construction_and_state_dict_keys():
    from ucnerf_amd.internal import configs, models
    kw = dict(grid_level_dim=2, grid_log2_hashmap_size=10)
    with models.bindings(NerfMLP=dict(grid_disired_resolution=1024, **kw), PropMLP=dict(**kw)):
        base = models.Model(config=configs.Config(), num_levels=2)
        mlp = models.NerfMLP(disable_density_normals=False)
        assert mlp.disable_density_normals is False
        with models.bindings(NerfMLP=dict(disable_density_normals=False), PropMLP=dict(disable_density_normals=False)):
            model = models.Model(config=configs.Config(), num_levels=2)
    assert model.nerf_mlp.disable_density_normals is False and model.prop_mlp_0.disable_density_normals is False
    assert list(model.state_dict().keys()) == list(base.state_dict().keys())
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in base.state_dict().items()}


def test_refused_combinations():
    from ucnerf_amd.internal import configs, models
    kw = dict(grid_level_dim=2, grid_log2_hashmap_size=10, grid_disired_resolution=256)
    for bad in (dict(enable_pred_normals=True), dict(use_reflections=True), dict(use_n_dot_v=True)):
        with pytest.raises(NotImplementedError):
            models.NerfMLP(disable_density_normals=False, **kw, **bad)
    with pytest.raises(NotImplementedError, match="scale features"):
        models.NerfMLP(disable_density_normals=False, scale_featurization=True, **kw)
    models.NerfMLP(disable_density_normals=True, scale_featurization=True, **kw)           # each alone stays supported
    for k in ('orientation_loss_mult', 'predicted_normal_loss_mult'):
        cfg = configs.Config()
        setattr(cfg, k, 0.1)
        with models.bindings(NerfMLP=kw, PropMLP=kw):
            with pytest.raises(NotImplementedError, match=k):
                models.Model(config=cfg, num_levels=2)
            setattr(cfg, k, 0.0)
            models.Model(config=cfg, num_levels=2)


def test_result_dictionaries_carry_the_normals():
    from ucnerf_amd.internal import march_level as ml
    N, S = 3, 4
    w = torch.rand(N, S)
    nrm = torch.randn(N, S, 3)
    main, extras = torch.rand(N, 5), torch.rand(N, 4)
    r = ml.rendering_entry(main[:, :3], main[:, 3], main[:, 4], w, extras, (N,), torch.rand(N, S + 1), torch.rand(N, S, 3), 2, normals=nrm)
    assert torch.allclose(r['normals'], (w[..., None] * nrm).sum(dim=-2)) and r['normals'].shape == (N, 3)
    assert 'normals' not in ml.rendering_entry(main[:, :3], main[:, 3], main[:, 4], w, None, (N,), normals=nrm)
    assert 'normals' not in ml.rendering_entry(main[:, :3], main[:, 3], main[:, 4], w, extras, (N,), torch.rand(N, S + 1), None, 2)
    h = ml.history_entry(torch.rand(N, S, 3), torch.rand(N, S), None, torch.rand(N, S + 1), w, (N,), nrm * 2, nrm)
    assert torch.equal(h['normals'], nrm) and torch.equal(h['raw_grad_density'], nrm * 2)
    h = ml.history_entry(torch.rand(N, S, 3), torch.rand(N, S), None, torch.rand(N, S + 1), w, (N,))
    assert h['normals'] is None and h['raw_grad_density'] is None


# ------------------------------------------------------------------ the reference's own autograd (no_warp)
def test_restatement_matches_reference_golden():
    """tests/golden/normals_tiny.npz (make_normals_golden.py): the reference's MLP.forward(no_warp=True) with the flag off, through its own
    grid.py backward (`calc_grad_inputs`), mean(-2) and l2_normalize, both fields of spec `tiny`.  The reference is a float32 evaluation, so
    it is held like one: |reference - restatement float64| within k = 2 of |restatement float32 - restatement float64| (helpers.bracket,
    floor scaled to the gradient's size); samples where the float32 and float64 runs disagree on a cell or on a ReLU sign are left out
    (at most 5 %).  The warped path has no golden: coord.track_linearize is @torch.no_grad (coord.py:75)."""
    import helpers as H
    fx = H.load("normals_tiny.npz")
    spec = rm.make_spec('tiny')
    sd = rm.init_state(spec, seed=int(fx['seed']))
    means, stds = torch.as_tensor(fx['means']), torch.as_tensor(fx['stds'])
    B, G = stds.shape
    for name, fs in (('nerf', spec.nerf), ('prop', spec.props[0])):
        o32 = nr.normals(fs, sd, means, stds, torch.float32, True)
        o64 = nr.normals(fs, sd, means, stds, torch.float64, True)
        keep = nr.cells_agree(o32['cells'], o64['cells'], B, G) & ((o32['h'] > 0) == (o64['h'] > 0)).all(dim=-1)
        assert 1 - keep.float().mean() <= 0.05
        assert (torch.as_tensor(fx[name + '_coord']) - o32['coord']).abs().max() <= 1e-6
        for key in ('raw_grad_density', 'normals'):
            want, r32, r64 = torch.as_tensor(fx[f'{name}_{key}']).double()[keep], o32[key].double()[keep], o64[key].double()[keep]
            scale = float(r64.abs().max())
            assert scale > 0
            H.bracket(f"golden {name} {key}", (r32 - r64).abs(), (want - r64).abs(), k=2.0, floor=(1e-6 * scale, 1e-7 * scale))
