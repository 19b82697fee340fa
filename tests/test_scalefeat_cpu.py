"""MLP.scale_featurization, host side: the torch-CPU restatement (tests/scalefeat_ref.py) against the reference's own outputs
(tests/golden/*_scalefeat*.npz, make_scalefeat_golden.py) at the bars of tests/test_oracle_golden.py, and the module layout of a
flag-on model against the reference's state dict."""
import pytest
import torch

import helpers as H
import scalefeat_ref as sf
from oracle import raymarch as rm
from test_glo_cpu import fixture, ref_layout
from test_oracle_golden import TOL

MODELS = [("model_scalefeat.npz", "tiny"), ("model_scalefeat_R.npz", "tinyR")]


@pytest.mark.parametrize("name,kind", MODELS)
def test_restatement_reproduces_the_reference_forward(name, kind):
    fx = fixture(name)
    spec = rm.make_spec(kind)
    sd = sf.state_for(fx, spec)
    with torch.no_grad():
        rend, hist = sf.model_forward(spec, sd, H.batch_of(fx), H.noise_of(fx, spec.num_levels), train_frac=1.0, compute_extras=True)
    for lvl in range(spec.num_levels):
        for k in ("rgb", "depth", "acc", "weights"):
            want = fx[f"L{lvl}_{k}"]
            assert H.maxdiff(rend[lvl][k].reshape(want.shape), want) <= (300 * TOL if k == "depth" else 8 * TOL), (lvl, k)
        for k in ("sdist", "weights", "density", "rgb", "coord"):
            want = fx[f"L{lvl}_hist_{k}"]
            assert H.maxdiff(hist[lvl][k].reshape(want.shape), want) <= 8 * TOL, (lvl, k)
    # the fixture is not vacuous: without the feature (same remaining weights) the pixels differ visibly
    with torch.no_grad():
        plain, _ = rm.model_forward(spec, sf.state_for(fx, spec, extra=None), H.batch_of(fx), H.noise_of(fx, spec.num_levels))
    assert H.maxdiff(plain[-1]["rgb"], fx[f"L{spec.num_levels - 1}_rgb"]) > 1e-2


def test_restatement_reproduces_the_reference_training_forward():
    fx = fixture("train_step_scalefeat.npz")
    spec = rm.make_spec("tiny")
    sd = sf.state_for(fx, spec)
    with torch.no_grad():
        rend, hist = sf.model_forward(spec, sd, H.batch_of(fx), H.noise_of(fx, spec.num_levels), train_frac=float(fx["train_frac"]),
                                      compute_extras=False, training=True)
    for lvl in range(spec.num_levels):
        for k, got in (("sdist", hist[lvl]["sdist"]), ("weights", hist[lvl]["weights"]), ("rgb", rend[lvl]["rgb"])):
            want = fx[f"L{lvl}_{k}"]
            assert H.maxdiff(got.reshape(want.shape), want) <= 8 * TOL, (lvl, k)


def test_level_scale_is_computed_without_gradient_and_from_the_whole_level():
    spec = rm.make_spec("tinyR")
    fs = spec.nerf
    emb = rm.init_state(spec, seed=5)[fs.prefix + ".encoder.embeddings"].requires_grad_()
    k = sf.level_scale(fs, emb)
    assert not k.requires_grad and k.shape == (fs.num_grid_levels,)
    _, offsets, _, _ = fs.layout()
    want = torch.stack([(emb[offsets[i]:offsets[i + 1]].detach().double() ** 2).sum(-1).mean() for i in range(fs.num_grid_levels)])
    # a sequential fp32 sum of up to 4096 positive terms: rounding random-walks to ~sqrt(4096) 2^-24 = 4e-6 relative
    assert H.maxdiff(k.double(), (sf.INIT_STD ** 2 + want).sqrt()) <= 1e-5


def sf_model(spec, on=True):
    from ucnerf_amd.internal import configs, models

    def fkw(fs):
        return dict(grid_disired_resolution=fs.grid_desired_resolution, grid_level_dim=fs.grid_level_dim,
                    grid_log2_hashmap_size=fs.grid_log2_hashmap_size, bottleneck_width=fs.bottleneck_width,
                    net_width_viewdirs=fs.net_width_viewdirs, scale_featurization=on)
    with models.bindings(NerfMLP=fkw(spec.nerf), PropMLP=fkw(spec.props[0])):
        return models.Model(config=configs.Config(training_views=spec.training_views), num_levels=spec.num_levels,
                            num_prop_samples=spec.num_prop_samples, num_nerf_samples=spec.num_nerf_samples,
                            prop_desired_grid_size=list(spec.prop_desired_grid_size))


@pytest.mark.parametrize("L,C", [(16, 2), (10, 4)])
def test_mlp_constructs_with_the_wider_density_layer(L, C):
    from ucnerf_amd.internal import models
    mlp = models.MLP(scale_featurization=True, grid_level_dim=C, grid_disired_resolution=16 << (L - 1), grid_log2_hashmap_size=12)
    assert (mlp.encoder.num_levels, mlp.encoder.level_dim) == (L, C)
    assert mlp.density_layer[0].in_features == L * C + L
    assert models.MLP(grid_level_dim=C, grid_disired_resolution=16 << (L - 1), grid_log2_hashmap_size=12).density_layer[0].in_features == L * C
    assert mlp.encoder.init_std == sf.INIT_STD


@pytest.mark.parametrize("name,kind", MODELS + [("train_step_scalefeat.npz", "tiny")])
def test_state_dict_matches_reference(name, kind):
    """Keys, shapes and registration order equal the reference's; its checkpoint loads with strict=True."""
    fx = fixture(name)
    spec = rm.make_spec(kind)
    model = sf_model(spec)
    keys, shapes = ref_layout(fx)
    sd = model.state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    ckpt = {k: v.clone() for k, v in sd.items()}
    ckpt.update(sf.state_for(fx, spec))
    model.load_state_dict(ckpt, strict=True)
    for fs in sf.fields_of(spec):
        w = model.get_submodule(fs.prefix).density_layer[0].weight
        assert torch.equal(w[:, fs.num_grid_levels * fs.grid_level_dim:], fx[f"sf_{fs.prefix}.density_layer.0.extra"].float())
