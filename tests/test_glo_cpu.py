"""GLO appearance codes (Model.num_glo_features > 0), host side: module layout against the reference's state dict
(tests/golden/model_glo.npz, make_glo_golden.py), the zero_glo switches, and the weight fold the fused inference march uses."""
import numpy as np
import pytest
import torch

import helpers as H
from oracle import raymarch as rm


def fixture(name):
    z = np.load(f"{H.GOLDEN}/{name}")
    return {k: torch.from_numpy(z[k]) for k in z.files}


def ref_layout(fx):
    keys = bytes(fx["sd_keys"].numpy()).decode().split("\n")
    dims, flat = fx["sd_ndims"].tolist(), fx["sd_shapes"].tolist()
    shapes, i = [], 0
    for d in dims:
        shapes.append(tuple(flat[i:i + d]))
        i += d
    return keys, shapes


def glo_model(spec, zero_glo=False):
    from ucnerf_amd.internal import configs, models

    def fkw(fs):
        return dict(grid_disired_resolution=fs.grid_desired_resolution, grid_level_dim=fs.grid_level_dim,
                    grid_log2_hashmap_size=fs.grid_log2_hashmap_size, bottleneck_width=fs.bottleneck_width,
                    net_width_viewdirs=fs.net_width_viewdirs)
    cfg = configs.Config(training_views=spec.training_views, zero_glo=zero_glo)
    with models.bindings(NerfMLP=fkw(spec.nerf), PropMLP=fkw(spec.props[0])):
        return models.Model(config=cfg, num_levels=spec.num_levels, num_prop_samples=spec.num_prop_samples,
                            num_nerf_samples=spec.num_nerf_samples, prop_desired_grid_size=list(spec.prop_desired_grid_size),
                            num_glo_features=4, num_glo_embeddings=spec.training_views)


@pytest.mark.parametrize("name", ["model_glo.npz", "train_step_glo.npz"])
def test_glo_state_dict_matches_reference(name):
    """Keys, shapes and registration order equal the reference's; its checkpoint loads with strict=True."""
    fx = fixture(name)
    model = glo_model(rm.make_spec("tiny"))
    keys, shapes = ref_layout(fx)
    sd = model.state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    ckpt = {k: v.clone() for k, v in sd.items()}
    for k in ckpt:
        if "glo_" + k in fx:
            ckpt[k] = fx["glo_" + k].float()
    model.load_state_dict(ckpt, strict=True)
    assert torch.equal(model.glo_vecs.weight, fx["glo_glo_vecs.weight"].float())
    assert torch.equal(model.nerf_mlp.lin_glo_1.weight, fx["glo_nerf_mlp.lin_glo_1.weight"].float())


def test_glo_layer_widths_and_default_init():
    model = glo_model(rm.make_spec("tiny"))
    m = model.nerf_mlp
    assert [type(m.get_submodule(f"lin_glo_{i}")) for i in range(2)] == [torch.nn.Linear] * 2
    assert (m.lin_glo_0.in_features, m.lin_glo_0.out_features) == (4, 128)
    assert (m.lin_glo_1.in_features, m.lin_glo_1.out_features) == (128, 2 * m.bottleneck_width)
    assert tuple(model.glo_vecs.weight.shape) == (model.config.training_views, 4)
    for i in range(model.num_levels - 1):                     # proposal fields carry no GLO layers
        assert not any("glo" in k for k in model.get_submodule(f"prop_mlp_{i}").state_dict())


def test_config_zero_glo_has_no_embedding_and_misuse_raises():
    spec = rm.make_spec("tiny")
    model = glo_model(spec, zero_glo=True)
    assert not hasattr(model, "glo_vecs")
    assert "nerf_mlp.lin_glo_0.weight" in model.state_dict()
    batch = {k: v for k, v in rm.synthetic_rays(8, seed=1).items()}
    with pytest.raises(RuntimeError, match="zero_glo"):
        model(False, batch, 1.0, False, zero_glo=False)


def test_glo_affine_is_the_reference_glo_mlp():
    torch.manual_seed(0)
    m = glo_model(rm.make_spec("tiny")).nerf_mlp.double()
    g = torch.randn(5, 4, dtype=torch.float64)
    a, b = m.glo_affine(g)
    h = m.lin_glo_1(torch.relu(m.lin_glo_0(g)))
    scale, shift = h.chunk(2, dim=-1)
    assert torch.allclose(a.double(), torch.exp(scale), rtol=1e-6) and torch.allclose(b.double(), shift, atol=1e-7)
    assert a.dtype == torch.float32 and a.shape == (5, m.bottleneck_width)


def test_glo_fold_reproduces_the_modulated_colour_layers_float64():
    """models.glo_fold: W0x diag(a), b0 + W0x b, W1x diag(a), b1 + W1x b -- the colour layers on x * a + b, in float64."""
    from ucnerf_amd.internal import models
    g = torch.Generator().manual_seed(3)
    NB, NW, E, M = 256, 256, 27, 64
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    W0, b0, W1, b1 = r(NW, NB + E), r(NW), r(NW, NW + NB + E), r(NW)
    a, b = torch.exp(0.3 * r(NB)), 0.5 * r(NB)
    x, enc = r(M, NB), r(M, E)

    def colour(W0, b0, W1, b1, x):
        h1 = torch.relu(torch.cat([x, enc], -1) @ W0.t() + b0)
        return torch.relu(torch.cat([h1, x, enc], -1) @ W1.t() + b1)
    want = colour(W0, b0, W1, b1, x * a + b)
    got = colour(*models.glo_fold(W0, b0, W1, b1, a, b), x)
    assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max())
    # identity modulation: the fold returns the weights unchanged, bit for bit
    same = models.glo_fold(W0, b0, W1, b1, torch.ones(NB, dtype=torch.float64), torch.zeros(NB, dtype=torch.float64))
    for p, q in zip(same, (W0, b0, W1, b1)):
        assert torch.equal(p, q)
