"""RawNeRF exposure, random background colours and near_anneal_rate without a GPU: tests/exposure_ref.py (the plain-torch restatement)
against tests/golden/exposure.npz (the imported reference's outputs, make_exposure_golden.py); the Model's construction and its state
dict's key order; init_s_near and the dilation schedule; the order of the random draws through internal/march_level.py."""
from types import SimpleNamespace

import pytest
import torch

import exposure_ref as er
import helpers as H
from oracle import raymarch as rm
from ucnerf_amd.internal import configs, march_level as ml, models

# float32 restatement against the float32 reference: the same operations in the same order, except where the restatement replaces an
# O(n m) mask by a binary search (the same knots) and a sum's blocking may differ -- a few ulp of O(1) quantities
TOL = 8 * 2.0 ** -24


@pytest.fixture(scope="module")
def fx():
    return H.load("exposure.npz")


@pytest.mark.parametrize("i", [0, 1])
def test_restatement_domain_resampling_equals_the_reference(fx, i):
    g = lambda k: fx[f"dom{i}_{k}"]
    s_near, dom = float(g("s_near")), (float(g("s_near")), 1.0)
    td, wd = er.max_dilate_weights(g("t"), g("w"), float(g("dilation")), dom)
    assert H.maxdiff(td, g("t_dilate")) == 0.0 and H.maxdiff(wd, g("w_dilate")) <= TOL
    assert float(td.min()) >= s_near and float(td.max()) <= 1.0
    t_in = g("t_dilate")[..., 1:-1]
    assert H.maxdiff(er.sample_intervals(t_in, g("logits"), 8, dom), g("eval")) <= TOL
    assert H.maxdiff(er.sample_intervals(t_in, g("logits"), 8, dom, jitter=g("jitter")), g("train")) <= TOL
    # the whole level (dilate, trim, logits, sample) and the first level
    got = er.resample(g("t"), g("w"), float(g("dilation")), 0.7, 0.0, 8, s_near, jitter=g("jitter"))
    assert H.maxdiff(got, g("train")) <= TOL
    first = er.resample(None, None, 0.0, 1.0, 0.0, 8, s_near, jitter=g("first_jitter"), N=6)
    assert H.maxdiff(first, g("first")) <= TOL
    for f in (got, first):
        assert float(f.min()) >= s_near and float(f.max()) <= 1.0 and bool((f[:, 1:] >= f[:, :-1]).all())


@pytest.mark.parametrize("opaque", [0, 1])
def test_restatement_compositing_equals_the_reference(fx, opaque):
    w, rgb, depth, acc, scaled = er.composite(fx["comp_density"], fx["comp_rgbs"], fx["comp_tdist"], fx["comp_dirs"], fx["comp_bg"],
                                              bool(opaque), gain=fx["comp_gain"])
    assert H.maxdiff(w, fx[f"comp{opaque}_weights"]) <= TOL and H.maxdiff(acc, fx[f"comp{opaque}_acc"]) <= TOL
    assert H.maxdiff(rgb, fx[f"comp{opaque}_rgb"]) <= 4 * TOL                  # colours up to 4 (the gain)
    assert H.maxdiff(depth, fx[f"comp{opaque}_depth"]) <= 8 * TOL              # distances up to 8


def test_restatement_exposure_block_and_model_levels_equal_the_reference(fx):
    spec = rm.make_spec("tiny")
    idx, ev, off = fx["model_exposure_idx"], fx["model_exposure_values"], fx["model_offsets"]
    rays = {k[len("model_ray_"):]: v for k, v in fx.items() if k.startswith("model_ray_")}
    lo, hi = (float(v) for v in fx["model_bg_range"])
    s_near = er.init_s_near(float(fx["model_train_frac"]), float(fx["model_rate"]))
    assert s_near == pytest.approx(0.7)
    samples = [spec.num_prop_samples] * (spec.num_levels - 1) + [spec.num_nerf_samples]
    dil = er.dilations(spec.dilation_bias, spec.dilation_multiplier, s_near, samples)
    anneal = ml.anneal_of(spec.anneal_slope, float(fx["model_train_frac"]))
    gain = er.exposure_gain(ev, idx, off)
    assert bool((gain[idx[:, 0] == 0] == ev[idx[:, 0] == 0]).all())               # the mask: no learned scaling at exposure_idx 0
    sdist = weights = None
    for lvl, S in enumerate(samples):
        g = lambda k: fx[f"model_L{lvl}_{k}"]
        # the exposure block: the history's colours are the plain run's, scaled
        assert H.maxdiff(er.exposure_block(g("plain_rgb"), ev, idx, off), g("hist_rgb")) <= 4 * TOL
        assert H.maxdiff(g("plain_rgb") * gain[:, None, :], g("hist_rgb")) <= 8 * TOL      # ... as one per-ray factor: one rounding more
        # the fenceposts on the annealed domain, from the previous level's
        sdist = er.resample(sdist, weights, dil[lvl], anneal, spec.resample_padding, S, s_near, jitter=fx[f"model_noise{lvl}_jitter"],
                            N=idx.shape[0])
        assert H.maxdiff(sdist, g("hist_sdist")) <= TOL
        assert float(g("hist_sdist").min()) >= float(torch.tensor(s_near, dtype=torch.float32))      # the float32 domain
        sdist = g("hist_sdist")
        # compositing with the level's background draw
        bg = fx[f"model_noise{lvl}_bg_u"] * (hi - lo) + lo
        tdist = er.s_to_t(sdist, rays["near"], rays["far"])
        weights, rgb, _, _, _ = er.composite(g("hist_density"), g("hist_rgb"), tdist, rays["directions"], bg, spec.opaque_background)
        assert H.maxdiff(weights, g("hist_weights")) <= TOL and H.maxdiff(rgb, g("rgb")) <= 4 * TOL
        weights = g("hist_weights")


def _tiny(**kw):
    spec = rm.make_spec("tiny")
    fkw = lambda fs: dict(grid_disired_resolution=fs.grid_desired_resolution, grid_level_dim=fs.grid_level_dim,
                          grid_log2_hashmap_size=fs.grid_log2_hashmap_size, bottleneck_width=fs.bottleneck_width,
                          net_width_viewdirs=fs.net_width_viewdirs)
    cfg = configs.Config(model_sky=spec.model_sky, brightness_correction=spec.brightness_correction, training_views=spec.training_views)
    with models.bindings(NerfMLP=fkw(spec.nerf), PropMLP=fkw(spec.props[0])):
        return models.Model(config=cfg, num_levels=spec.num_levels, num_prop_samples=spec.num_prop_samples,
                            num_nerf_samples=spec.num_nerf_samples, prop_desired_grid_size=list(spec.prop_desired_grid_size), **kw)


def test_state_dict_keys_and_order_with_learned_exposure_scaling(fx):
    want = bytes(fx["model_state_keys"].numpy()).decode().split("\n")
    model = _tiny(learned_exposure_scaling=True)
    got = [k for k in model.state_dict().keys() if not k.endswith(".idx") or k in want]
    assert got == [k for k in want if k in set(got)] and "exposure_scaling_offsets.weight" in got
    assert set(want) - set(got) <= {k for k in want if k.endswith(".idx")}
    w = model.exposure_scaling_offsets.weight
    assert w.shape == (model.num_glo_embeddings, 3) and not w.any()               # zero-initialised (models.py:82)


@pytest.mark.parametrize("kw", [dict(learned_exposure_scaling=True), dict(bg_intensity_range=(0.2, 0.8)), dict(near_anneal_rate=0.1)])
def test_the_three_options_construct(kw):
    model = _tiny(**kw)
    for k, v in kw.items():
        assert getattr(model, k) == v


def test_single_mlp_is_still_refused():
    for kw in (dict(single_mlp=True), dict(distinct_prop=False), dict(use_viewdirs=False)):
        with pytest.raises(NotImplementedError):
            _tiny(**kw)


def _plan_model(**over):
    kw = dict(num_levels=3, num_prop_samples=64, num_nerf_samples=32, dilation_bias=0.0025, dilation_multiplier=0.5, nerf_mlp="nerf",
              near_anneal_rate=0.1, near_anneal_init=0.95)
    kw.update(over)
    return SimpleNamespace(get_submodule=lambda name: name, **kw)


@pytest.mark.parametrize("train_frac, s_near", [(0.0, 0.95), (0.05, 0.5), (0.1, 0.0), (1.0, 0.0)])
def test_init_s_near_and_the_dilation_schedule(train_frac, s_near):
    m = _plan_model()
    got = ml.s_near_of(m, train_frac)
    assert got == pytest.approx(s_near, abs=1e-15) and got == er.init_s_near(train_frac, 0.1, 0.95)
    assert 0.0 <= got <= 0.95
    plan = ml.level_plan(m, train_frac)
    assert [p[4] for p in plan] == er.dilations(0.0025, 0.5, got, [64, 64, 32])
    assert [p[4] for p in plan] == [0.0025 + 0.5 * (1. - got) / prod for prod in (1, 64, 4096)]      # models.py:158-159
    # without the option train_frac is not read and the schedule is the one of before
    off = _plan_model(near_anneal_rate=None)
    assert ml.s_near_of(off, train_frac) == 0.0 and ml.level_plan(off) == ml.level_plan(off, train_frac)
    with pytest.raises(ValueError):
        ml.level_plan(m)


N, S, LEVELS = 5, 4, 3


def _rays(**extra):
    batch = dict(rm.synthetic_rays(N, seed=1))
    batch.update(extra)
    return ml.Rays(batch, LEVELS, on_device=False)


def _draw_level(model, rays, lvl, rand):
    d = ml.draws(rays, lvl, S, rand, True)
    return d, ml.background(model, rays, lvl, rand)


def test_draw_order_with_a_background_range():
    rng = (0.2, 0.8)
    model = SimpleNamespace(bg_intensity_range=rng)
    torch.manual_seed(21)
    want = [er.level_draws(N, S, True, rng) for _ in range(2)]
    torch.manual_seed(21)
    rays = _rays()
    for lvl in range(2):
        (jitter, flip, spin, rvec), (bg, ray_bg) = _draw_level(model, rays, lvl, True)
        for got, k in ((jitter, "jitter"), (flip, "flip"), (spin, "spin"), (rvec, "rvec"), (ray_bg, "bg")):
            assert torch.equal(got, want[lvl][k]), (lvl, k)
        assert ray_bg.shape == (N, 3) and float(ray_bg.min()) >= 0.2 and float(ray_bg.max()) <= 0.8


def test_background_for_rand_none_pinned_and_one_valued():
    model = SimpleNamespace(bg_intensity_range=(0.2, 0.8))
    torch.manual_seed(22)
    after = torch.rand(2)
    torch.manual_seed(22)
    assert ml.background(model, _rays(), 0, None) == (er.background((0.2, 0.8), None, N), None) == (0.5, None)      # models.py:249: `is None`
    pinned = torch.full((N, 3), 0.25, dtype=torch.float64)
    for rand in (True, False):
        bg, ray_bg = ml.background(model, _rays(march_noise=[{}, dict(bg=pinned), {}]), 1, rand)
        assert ray_bg.dtype == torch.float32 and torch.equal(ray_bg, pinned.float())
        assert ml.background(SimpleNamespace(bg_intensity_range=(1., 1.)), _rays(), 0, rand) == (1.0, None)
    assert torch.equal(torch.rand(2), after)                             # none of these consumed the generator


def test_background_is_drawn_for_rand_false_behind_the_randn():
    """rand = False is not rand = None: the reference draws the colours (models.py:249-256), right behind the level's randn_like."""
    rng = (0.2, 0.8)
    model = SimpleNamespace(bg_intensity_range=rng)
    torch.manual_seed(24)
    want = [er.level_draws(N, S, True, rng, rand=False) for _ in range(2)]
    assert all(set(w) == {"rvec", "bg"} for w in want)
    torch.manual_seed(24)
    rays = _rays()
    for lvl in range(2):
        (jitter, flip, spin, rvec), (bg, ray_bg) = _draw_level(model, rays, lvl, False)
        assert jitter is None and flip is None and spin is None
        assert torch.equal(rvec, want[lvl]["rvec"]) and torch.equal(ray_bg, want[lvl]["bg"])


@pytest.mark.parametrize("tag, rand", [("false", False), ("none", None)])
def test_deterministic_calls_with_a_background_range_equal_the_reference(fx, tag, rand):
    """The reference's Model with bg_intensity_range = (0.2, 0.8), rand = False and rand = None (tests/golden/exposure.npz eval_*): after
    the reference's torch seed, march_level draws what the reference drew, in its order; and the restatement composites the reference's
    per-sample outputs with that background to the reference's pixels."""
    spec = rm.make_spec("tiny")
    rays_fx = {k[len("eval_ray_"):]: v for k, v in fx.items() if k.startswith("eval_ray_")}
    n = rays_fx["origins"].shape[0]
    model = SimpleNamespace(bg_intensity_range=(0.2, 0.8))
    rays = ml.Rays(rays_fx, spec.num_levels, on_device=False)
    torch.manual_seed(int(fx["eval_torch_seed"]))
    for lvl, S_l in enumerate([spec.num_prop_samples] * (spec.num_levels - 1) + [spec.num_nerf_samples]):
        g = lambda k: fx[f"eval_{tag}_L{lvl}_{k}"]
        jitter, flip, spin, rvec = ml.draws(rays, lvl, S_l, rand, True)
        bg, ray_bg = ml.background(model, rays, lvl, rand)
        assert jitter is None and torch.equal(rvec, fx[f"eval_{tag}_noise{lvl}_rand_vec"])
        if rand is None:
            assert (bg, ray_bg) == (0.5, None)
        else:
            assert ray_bg.shape == (n, 3) and torch.equal(ray_bg, fx[f"eval_{tag}_noise{lvl}_bg_u"] * (0.8 - 0.2) + 0.2)
        tdist = er.s_to_t(g("hist_sdist"), rays_fx["near"], rays_fx["far"])
        _, rgb, _, _, _ = er.composite(g("hist_density"), g("hist_rgb"), tdist, rays_fx["directions"], bg if ray_bg is None else ray_bg,
                                       spec.opaque_background)
        assert H.maxdiff(rgb, g("rgb")) <= TOL
    assert H.maxdiff(fx["eval_false_L1_rgb"], fx["eval_none_L1_rgb"]) > 1e-3          # the two calls do differ upstream


def test_ray_gain():
    g = torch.Generator().manual_seed(23)
    ev, idx = 0.25 + 3.75 * torch.rand(N, 1, generator=g), torch.tensor([[0], [1], [2], [0], [3]])
    emb = torch.nn.Embedding(8, 3)
    with torch.no_grad():
        emb.weight.copy_(0.2 * torch.randn(8, 3, generator=g))
    rays = _rays()
    plain = SimpleNamespace(learned_exposure_scaling=False)
    learned = SimpleNamespace(learned_exposure_scaling=True, exposure_scaling_offsets=emb)
    assert ml.ray_gain(plain, {}, rays) is None and ml.ray_gain(plain, dict(exposure_idx=None, exposure_values=ev), rays) is None
    assert torch.equal(ml.ray_gain(plain, dict(exposure_idx=idx, exposure_values=ev), rays), ev.expand(N, 3))
    got = ml.ray_gain(learned, dict(exposure_idx=idx, exposure_values=ev), rays)
    assert torch.equal(got, er.exposure_gain(ev, idx, emb.weight))
    got.sum().backward()
    assert not emb.weight.grad[0].any() and emb.weight.grad[1].any() and not emb.weight.grad[4:].any()
    with pytest.raises(TypeError):                                       # indexing None upstream (models.py:261)
        ml.ray_gain(plain, dict(exposure_idx=idx), rays)
