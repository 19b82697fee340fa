"""internal/march_level.py without a GPU: the level plan and anneal value against the reference's formulas (models.py:152-184), the
order of the random draws against the literal sequence (stepfun.py:216, render.py:123,124,140), and the result dictionaries."""
from types import SimpleNamespace

import pytest
import torch

from oracle import raymarch as rm
from ucnerf_amd.internal import march_level as ml


def _model(**over):
    spec = rm.make_spec("tiny")
    kw = dict(num_levels=3, num_prop_samples=64, num_nerf_samples=32, dilation_bias=spec.dilation_bias,
              dilation_multiplier=spec.dilation_multiplier, nerf_mlp="nerf")
    kw.update(over)
    return SimpleNamespace(get_submodule=lambda name: name, **kw)


def test_level_plan_equals_the_reference_formula():
    m = _model()
    want, prod = [], 1
    for i in range(3):                                               # models.py:152-162
        is_prop = i < 2
        S = 64 if is_prop else 32
        want.append((i, is_prop, S, f"prop_mlp_{i}" if is_prop else "nerf", m.dilation_bias + m.dilation_multiplier * 1.0 / prod))
        prod *= S
    assert ml.level_plan(m) == want
    assert [p[4] for p in want] == [0.0025 + 0.5, 0.0025 + 0.5 / 64, 0.0025 + 0.5 / 4096]


def test_level_plan_dilation_off_and_refused():
    assert [p[4] for p in ml.level_plan(_model(dilation_bias=0, dilation_multiplier=0))] == [0.0, 0.0, 0.0]
    assert all(type(p[4]) is float for p in ml.level_plan(_model(dilation_bias=0, dilation_multiplier=0)))
    with pytest.raises(NotImplementedError, match="dilation"):
        ml.level_plan(_model(dilation_bias=-1, dilation_multiplier=0.5))


def test_anneal():
    for f in (0.0, 0.5, 1.0):
        assert ml.anneal_of(10, f) == (10 * f) / ((10 - 1) * f + 1)   # models.py:181
    assert ml.anneal_of(10, 0.0) == 0.0 and ml.anneal_of(10, 1.0) == 1.0
    assert ml.anneal_of(0, 0.3) == 1.0


N, S, LEVELS = 5, 4, 3


def _rays(**extra):
    batch = {k: v for k, v in rm.synthetic_rays(N, seed=1).items()}
    batch.update(extra)
    return ml.Rays(batch, LEVELS, on_device=False)


def _sequence(seed, jcols, skip=()):
    torch.manual_seed(seed)
    out = {}
    for name, shape in (("jitter", (N, jcols)), ("flip", (N, S)), ("spin", (N, S))):
        if name not in skip:
            out[name] = torch.rand(*shape)
    out["rvec"] = torch.randn(N, 3)
    return out


@pytest.mark.parametrize("single_jitter", [True, False])
def test_draw_order_unpinned(single_jitter):
    want = _sequence(11, 1 if single_jitter else S)
    torch.manual_seed(11)
    jitter, flip, spin, rvec = ml.draws(_rays(), 1, S, True, single_jitter)
    assert jitter.shape == (N, 1 if single_jitter else S)
    for got, k in ((jitter, "jitter"), (flip, "flip"), (spin, "spin"), (rvec, "rvec")):
        assert torch.equal(got, want[k]), k


def test_draw_order_without_rand_consumes_randn_alone():
    torch.manual_seed(12)
    want = torch.randn(N, 3)
    after = torch.rand(2)
    torch.manual_seed(12)
    jitter, flip, spin, rvec = ml.draws(_rays(), 0, S, False, True)
    assert jitter is None and flip is None and spin is None
    assert torch.equal(rvec, want) and torch.equal(torch.rand(2), after)


def test_draw_order_with_only_flip_pinned():
    pinned = torch.full((N, S), 0.25)
    want = _sequence(13, 1, skip=("flip",))
    torch.manual_seed(13)
    jitter, flip, spin, rvec = ml.draws(_rays(march_noise=[{}, {}, dict(flip=pinned)]), 2, S, True, True)
    assert flip.data_ptr() == pinned.data_ptr() and torch.equal(flip, pinned)
    assert torch.equal(jitter, want["jitter"]) and torch.equal(spin, want["spin"]) and torch.equal(rvec, want["rvec"])


def test_pinned_rand_vec_columns():
    vec = torch.arange(N * 3 * LEVELS, dtype=torch.float64).reshape(N, 3 * LEVELS) / 7
    for lvl in range(LEVELS):
        torch.manual_seed(14)
        before = torch.rand(2)
        torch.manual_seed(14)
        _, _, _, rvec = ml.draws(_rays(rand_vec=vec), lvl, S, False, True)
        assert rvec.dtype == torch.float32 and rvec.is_contiguous() and rvec.shape == (N, 3)
        assert torch.equal(rvec, vec[:, 3 * lvl:3 * lvl + 3].float())
        assert torch.equal(torch.rand(2), before)                     # nothing was drawn


EXTRA_KEYS = {"distance_mean", "distance_percentile_5", "distance_median", "distance_percentile_95"}
RAY_KEYS = {"ray_sdist", "ray_weights", "ray_rgbs"}
HISTORY_KEYS = {"coord", "density", "rgb", "raw_grad_density", "grad_pred", "normals", "normals_pred", "roughness", "sdist", "weights"}


@pytest.mark.parametrize("prefix", [(6,), (2, 3)])
@pytest.mark.parametrize("compute_extras", [False, True])
def test_result_dictionaries(prefix, compute_extras):
    n, s, n_vis = 6, 4, 4
    g = torch.Generator().manual_seed(3)
    main, weights, extras = torch.rand(n, 5, generator=g), torch.rand(n, s, generator=g), torch.rand(n, 4, generator=g)
    sdist, coord, density = torch.rand(n, s + 1, generator=g), torch.rand(n, s, 3, generator=g), torch.rand(n, s, generator=g)
    rgbs = torch.rand(n, s, 3, generator=g)
    r = ml.rendering_entry(main[:, :3], main[:, 3], main[:, 4], weights, extras if compute_extras else None, prefix, sdist, rgbs, n_vis)
    assert set(r) == {"rgb", "depth", "acc", "weights"} | (EXTRA_KEYS | RAY_KEYS if compute_extras else set())
    assert r["rgb"].shape == prefix + (3,) and r["depth"].shape == prefix and r["acc"].shape == prefix
    assert r["weights"].shape == prefix + (s,) and torch.equal(r["weights"].reshape(n, s), weights)
    assert torch.equal(r["rgb"].reshape(n, 3), main[:, :3]) and torch.equal(r["depth"].reshape(n), main[:, 3])
    if compute_extras:
        for j, k in enumerate(("distance_mean", "distance_percentile_5", "distance_median", "distance_percentile_95")):
            assert r[k].shape == prefix and torch.equal(r[k].reshape(n), extras[:, j])
        prop = ml.rendering_entry(main[:, :3], main[:, 3], main[:, 4], weights, extras, prefix, sdist, None, n_vis)   # a proposal level: zero colours
        r = ml.rendering_entry(main[:, :3], main[:, 3], main[:, 4], weights, extras, prefix, sdist, rgbs, n_vis)
        assert set(r) - EXTRA_KEYS - {"rgb", "depth", "acc", "weights"} == RAY_KEYS
        assert r["ray_sdist"].shape == (n_vis, s + 1) and r["ray_weights"].shape == (n_vis, s) and r["ray_rgbs"].shape == (n_vis, s, 3)
        assert prop["ray_rgbs"].shape == (n_vis, s, 3) and not prop["ray_rgbs"].any()
        few = ml.rendering_entry(main[:, :3], main[:, 3], main[:, 4], weights, extras, prefix, sdist, None, 16)   # n_vis > N: [min(n_vis, N), S, 3]
        assert few["ray_rgbs"].shape == (n, s, 3) and few["ray_sdist"].shape == (n, s + 1)
        ml.broadcast_final([prop, r])
        final = (rgbs[:n_vis] * weights[:n_vis, :, None]).sum(dim=-2)
        assert prop["ray_rgbs"].shape == (n_vis, s, 3)
        assert torch.equal(prop["ray_rgbs"], final[:, None, :].expand(n_vis, s, 3)) and torch.equal(r["ray_rgbs"], rgbs[:n_vis])
    for level_rgbs in (rgbs, None):
        h = ml.history_entry(coord, density, level_rgbs, sdist, weights, prefix)
        assert set(h) == HISTORY_KEYS
        assert h["coord"].shape == prefix + (s, 3) and h["density"].shape == prefix + (s,) and h["rgb"].shape == prefix + (s, 3)
        assert h["sdist"].shape == prefix + (s + 1,) and h["weights"].shape == prefix + (s,)
        assert torch.equal(h["rgb"].reshape(n, s, 3), rgbs if level_rgbs is not None else torch.zeros(n, s, 3))
        assert h["sdist"].data_ptr() != sdist.data_ptr() and torch.equal(h["sdist"].reshape(n, s + 1), sdist)
        assert all(h[k] is None for k in ("raw_grad_density", "grad_pred", "normals", "normals_pred", "roughness"))
