"""The Ref-NeRF colour heads (MLP.use_diffuse_color, use_specular_tint, enable_pred_roughness), CPU side: the state dict's layout, the
restatement tests/ref_colour_ref.py against the reference's recorded values (tests/golden/ref_colour.npz), the refusals, the training
graph's route decision and the library's exports.  Nothing here touches a GPU."""
import itertools
import os

import pytest
import torch

import ref_colour_ref as rc

KW = dict(grid_level_dim=2, grid_log2_hashmap_size=8, grid_disired_resolution=64)
FLAGS3 = ("use_diffuse_color", "use_specular_tint", "enable_pred_roughness")


def test_state_dict_layout_is_the_references():
    keys, shapes = rc.sd_layout()
    sd = rc.build_model().state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    at = keys.index("nerf_mlp.normal_layer.weight")
    assert keys[at + 2:at + 9:2] == ["nerf_mlp.diffuse_layer.weight", "nerf_mlp.specular_layer.weight", "nerf_mlp.roughness_layer.weight",
                                     "nerf_mlp.lin_glo_0.weight"]
    assert "prop_mlp_0.diffuse_layer.weight" in keys and "prop_mlp_0.specular_layer.weight" not in keys
    # lin_second_stage_0's input is unchanged: bottleneck + 27
    assert sd["nerf_mlp.lin_second_stage_0.weight"].shape[1] == 64 + 27


def test_restatement_agrees_with_the_fixture():
    fx = rc.fixture()
    r32, r64 = rc.restate(torch.float32), rc.restate(torch.float64)
    for k, v in r64.items():
        if k not in fx:
            continue
        # float32 sums of <= 91 O(1) terms in another order (values), of 37 x S samples (gradients): 64 eps / 1e-5 relative to the largest value
        bar = 1e-5 if k.startswith("grad_") else 64 * rc.EPS32
        assert rc.rel_err(fx[k], v) <= bar and rc.rel_err(r32[k], v) <= bar, k
    for k in ("L0_rgb", "L1_rgb", "L1_roughness", "L1_render_roughness", "L0_render_rgb", "grad_nerf_mlp.diffuse_layer.weight",
              "grad_nerf_mlp.specular_layer.weight", "grad_prop_mlp_0.diffuse_layer.weight"):
        assert k in fx and k in r64, k
    assert not any("roughness_layer" in k for k in fx if k.startswith("grad_"))      # no consumer: no gradient in the reference
    for tint in (True, False):
        tag = "tint" if tint else "notint"
        for dtype in (torch.float32, torch.float64):
            got = rc.crafted(dtype, tint)
            for name, v in zip(("rgb", "g_logits", "g_raw_diffuse", "g_raw_tint"), got):
                if v is not None:
                    assert rc.rel_err(fx[f"E_{tag}_{name}"], v) <= 8 * rc.EPS32, (tag, name, dtype)


def test_crafted_set_covers_the_three_regimes():
    for tint, (toe, power, clipped, l) in rc.crafted_regimes().items():
        for m in (toe, power, clipped):
            assert float(m.double().mean()) >= 0.10
        assert float((l - rc.TOE).abs().min()) >= 1e-4 and float((l - 1.0).abs().min()) >= 1e-3
    fx = rc.fixture()
    for lvl in range(2):      # the network's own samples reach the clip and the power part
        at_one = torch.from_numpy(fx[f"L{lvl}_rgb"])[..., 0] >= 1.0
        assert 0.1 <= float(at_one.double().mean()) <= 0.9


def test_refusal_matrix():
    from ucnerf_amd.internal import models
    for n in range(1, 4):
        for on in itertools.combinations(FLAGS3, n):
            flags = {k: True for k in on}
            m = models.NerfMLP(**flags, **KW)
            assert [hasattr(m, l) for l in rc.HEAD_LAYERS] == [k in on for k in FLAGS3]
            models.NerfMLP(enable_pred_normals=True, **flags, **KW)
            models.PropMLP(disable_rgb=False, **flags, **KW)
    every = {k: True for k in FLAGS3}
    m = models.NerfMLP(enable_pred_normals=True, num_glo_features=4, scale_featurization=True, warp_fn=None, **every, **KW)
    assert m.ref_heads_mask() == 7 and m.roughness_bias == -1.0
    keys = list(m.state_dict().keys())
    assert keys.index("normal_layer.bias") < keys.index("diffuse_layer.weight") < keys.index("specular_layer.weight") \
        < keys.index("roughness_layer.weight") < keys.index("lin_glo_0.weight")
    for bad in ("use_reflections", "use_n_dot_v", "use_directional_enc"):
        for extra in ({}, every):
            with pytest.raises(NotImplementedError, match=bad):
                models.NerfMLP(**{bad: True}, **extra, **KW)
    # disable_rgb = True: the flags register nothing and do nothing, as in the reference
    p = models.PropMLP(**every, **KW)
    assert p.disable_rgb and p.ref_heads_mask() == 0 and not any(hasattr(p, l) for l in rc.HEAD_LAYERS)
    assert list(p.state_dict().keys()) == list(models.PropMLP(**KW).state_dict().keys())


def test_heads_route(monkeypatch):
    """A flagged field takes "colour_node" for every argument and switch setting of tests/test_train_graph_split_cpu.py's grid; a field
    without the flags -- also one whose flags do nothing (disable_rgb = True) -- gets the route that file's TABLE records from before
    `heads_route` existed."""
    import test_train_graph_split_cpu as split
    from ucnerf_amd.internal import models
    from ucnerf_amd.internal import train_graph as tg
    every = {k: True for k in FLAGS3}
    unflagged = dict(nerf=models.NerfMLP(), prop=models.PropMLP(**every))         # the reference's widths, like that file's fixture
    assert unflagged["prop"].ref_heads_mask() == 0
    flagged = [models.NerfMLP(**{k: True}) for k in FLAGS3]
    wrong = []
    for e, env in enumerate(split.ENVS):
        for name, value in zip(split.SWITCHES, env):
            monkeypatch.setenv(name, value)
        for (field, autocast, on_device, glo), cells in split.TABLE.items():
            for n, cell in zip(split.N_FEATURES, cells):
                args = (n, on_device, autocast, (None, None) if glo else None)
                got = tg.heads_route(unflagged[field], *args)
                if got != split.ROUTE[cell[e]]:
                    wrong.append((field, args, env, got, split.ROUTE[cell[e]]))
                if field == "nerf":
                    wrong += [(k, args, env, r, "colour_node") for k, m in zip(FLAGS3, flagged) for r in [tg.heads_route(m, *args)]
                              if r != "colour_node"]
    assert not wrong, wrong[:5]
    with pytest.raises(NotImplementedError, match="net_width_viewdirs"):
        tg.heads_route(models.NerfMLP(use_diffuse_color=True, net_width_viewdirs=60, **KW), 20, True, None, None)


def test_result_dictionaries_carry_the_roughness():
    from ucnerf_amd.internal import march_level as ml
    N, S = 5, 4
    w, rough = torch.rand(N, S), torch.rand(N, S, 1)
    args = (torch.zeros(N, 3), torch.zeros(N), torch.zeros(N), w)
    r = ml.rendering_entry(*args, torch.zeros(N, 4), (N,), torch.zeros(N, S + 1), None, roughness=rough)
    assert r["roughness"].shape == (N, 1) and torch.allclose(r["roughness"][:, 0], (w * rough[..., 0]).sum(-1))
    assert "roughness" not in ml.rendering_entry(*args, None, (N,), roughness=rough)              # only with compute_extras
    assert "roughness" not in ml.rendering_entry(*args, torch.zeros(N, 4), (N,), torch.zeros(N, S + 1), None)
    h = ml.history_entry(torch.zeros(N, S, 3), torch.zeros(N, S), None, torch.zeros(N, S + 1), w, (N,), roughness=rough.reshape(N, S))
    assert h["roughness"].shape == (N, S, 1)
    assert ml.history_entry(torch.zeros(N, S, 3), torch.zeros(N, S), None, torch.zeros(N, S + 1), w, (N,))["roughness"] is None


def test_library_exports_the_entry_points_at_abi_32():
    from ucnerf_amd import _lib
    for name in ("ucn_ref_heads", "ucn_ref_colour", "ucn_ref_colour_backward"):
        assert name in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ucnerf_march.h")).read()
    for name in ("ucn_ref_heads", "ucn_ref_colour", "ucn_ref_colour_backward"):
        assert f"int {name}(" in header
    lib = _lib.load()
    assert _lib.ABI_VERSION == 32 and lib.ucn_abi_version() == 32
    for name in ("ucn_ref_heads", "ucn_ref_colour", "ucn_ref_colour_backward"):
        assert getattr(lib, name) is not None
