"""Predicted normals (MLP.enable_pred_normals) and the orientation loss, CPU side: the restatement tests/pred_normals_ref.py against
the reference's recorded values (tests/golden/pred_normals.npz), the state dict's layout, the refusals, the loss's semantics, the result
dictionaries and the overlay's export.  Nothing here touches a GPU."""
import ast
import os
import types

import pytest
import torch

import pred_normals_ref as pr

KW = dict(grid_level_dim=2, grid_log2_hashmap_size=8, grid_disired_resolution=64)


@pytest.fixture(scope="module")
def restated():
    return {torch.float32: pr.restate(torch.float32), torch.float64: pr.restate(torch.float64)}


def test_restatement_agrees_with_the_fixture(restated):
    fx = pr.fixture()
    r32, r64 = restated[torch.float32], restated[torch.float64]
    strong = lambda lvl: torch.from_numpy(fx[f"L{lvl}_grad_pred"]).norm(dim=-1) > float(fx["g_min"])
    for lvl in range(2):
        assert float((~strong(lvl)).double().mean()) <= 0.05
        for k in ("grad_pred", "weights", "render_normals_pred"):
            # float32 sums of <= 64 O(1) terms in another order: 64 eps relative to the largest value
            for r in (r32, r64):
                assert pr.rel_err(r[f"L{lvl}_{k}"], fx[f"L{lvl}_{k}"]) <= 64 * pr.EPS32, (lvl, k)
        m = strong(lvl)
        for r in (r32, r64):
            assert float((r[f"L{lvl}_normals_pred"].double()[m] - torch.from_numpy(fx[f"L{lvl}_normals_pred"]).double()[m]).abs().max()) <= 64 * pr.EPS32 / float(fx["g_min"])
            assert abs(float(r[f"L{lvl}_loss"]) - float(fx[f"L{lvl}_loss"])) <= 1e-5 * float(fx[f"L{lvl}_loss"])
    assert abs(float(r64["loss_total"]) - float(fx["loss_total"])) <= 1e-5 * float(fx["loss_total"])
    # the reference's float32 gradients against the float64 restatement's: sums over 37 x S samples of one-sided terms
    for name in pr.LEVELS:
        for k in pr.HEAD_PARAMS:
            assert pr.rel_err(fx[f"grad_{name}.{k}"], r64[f"grad_{name}.{k}"]) <= 1e-4, (name, k)
            assert pr.rel_err(r32[f"grad_{name}.{k}"], r64[f"grad_{name}.{k}"]) <= 1e-4, (name, k)


def test_state_dict_layout_is_the_references():
    keys, shapes = pr.sd_layout()
    model = pr.build_model()
    sd = model.state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    at = keys.index("nerf_mlp.normal_layer.weight")
    assert keys[at - 1] == "nerf_mlp.density_layer.2.bias" and keys[at + 2] == "nerf_mlp.lin_glo_0.weight"


def test_refusal_matrix():
    from ucnerf_amd.internal import configs, models
    models.NerfMLP(enable_pred_normals=True, **KW)                              # the supported combination
    models.PropMLP(enable_pred_normals=True, disable_rgb=False, **KW)
    models.NerfMLP(enable_pred_normals=True, scale_featurization=True, num_glo_features=4, warp_fn=None, **KW)
    with pytest.raises(NotImplementedError, match="predicted_normal_loss"):
        models.NerfMLP(enable_pred_normals=True, disable_density_normals=False, **KW)
    with pytest.raises(NotImplementedError, match="disable_rgb"):
        models.PropMLP(enable_pred_normals=True, **KW)                          # PropMLP.disable_rgb defaults to True
    for bad in ("use_reflections", "use_n_dot_v"):
        with pytest.raises(NotImplementedError, match=bad):
            models.NerfMLP(enable_pred_normals=True, **{bad: True}, **KW)
    head = dict(KW, enable_pred_normals=True, disable_rgb=False)
    for k in ("orientation_loss_mult", "orientation_coarse_loss_mult"):
        cfg = configs.Config()
        assert getattr(cfg, k) == 0.0
        setattr(cfg, k, 0.1)
        with models.bindings(NerfMLP=head, PropMLP=head):
            models.Model(config=cfg, num_levels=2)                               # every level carries the head
            cfg.orientation_loss_target = "normals"
            with pytest.raises(NotImplementedError, match=k):
                models.Model(config=cfg, num_levels=2)
            cfg.orientation_loss_target = "normals_pred"
        with models.bindings(NerfMLP=head, PropMLP=KW):                          # the proposal field lacks it
            with pytest.raises(NotImplementedError, match=k):
                models.Model(config=cfg, num_levels=2)
    for k in ("predicted_normal_loss_mult", "predicted_normal_coarse_loss_mult"):
        cfg = configs.Config()
        assert getattr(cfg, k) == 0.0
        setattr(cfg, k, 0.1)
        with models.bindings(NerfMLP=head, PropMLP=head):
            with pytest.raises(NotImplementedError, match=k):
                models.Model(config=cfg, num_levels=2)
    assert configs.Config().orientation_loss_target == "normals_pred"


def test_orientation_loss_semantics(restated):
    from ucnerf_amd.internal import train_utils
    fx = pr.fixture()
    t = lambda k: torch.from_numpy(fx[k])
    hist = [dict(weights=t(f"L{l}_weights"), normals_pred=t(f"L{l}_normals_pred"), normals=None) for l in range(2)]
    model = types.SimpleNamespace(num_levels=2)
    coarse, fine = fx["mults"].tolist()
    cfg = types.SimpleNamespace(orientation_loss_target="normals_pred", orientation_coarse_loss_mult=coarse, orientation_loss_mult=fine)
    batch = dict(viewdirs=t("ray_viewdirs"))
    got = train_utils.orientation_loss(batch, model, hist, cfg)
    assert abs(float(got) - float(fx["loss_total"])) <= 1e-5 * float(fx["loss_total"])
    # each multiplier reaches its own levels
    cfg.orientation_coarse_loss_mult = 0.0
    assert abs(float(train_utils.orientation_loss(batch, model, hist, cfg)) - fine * float(fx["L1_loss"])) <= 1e-5 * float(fx["L1_loss"])
    # a training batch: [N, 1, 1, .]
    cfg.orientation_coarse_loss_mult = coarse
    hist4 = [{k: (None if v is None else v[:, None, None]) for k, v in h.items()} for h in hist]
    got4 = train_utils.orientation_loss(dict(viewdirs=batch["viewdirs"][:, None, None, :]), model, hist4, cfg)
    assert abs(float(got4) - float(got)) <= 1e-6 * float(got)
    # a None target raises before the multipliers are looked at
    cfg.orientation_loss_target = "normals"
    cfg.orientation_coarse_loss_mult = cfg.orientation_loss_mult = 0.0
    with pytest.raises(ValueError, match="Normals cannot be None"):
        train_utils.orientation_loss(batch, model, hist, cfg)


def test_nodes_formulas_by_finite_differences():
    """the two nodes' backward formulas (csrc/train_ops.hip) against float64 finite differences of the restatement"""
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(7, 3, generator=g, dtype=torch.float64) - 0.5).requires_grad_(True)
    assert torch.autograd.gradcheck(pr.neg_normalize, (x,), eps=1e-7, atol=1e-6)
    dn = torch.rand(7, 3, generator=g, dtype=torch.float64)
    n = pr.neg_normalize(x.detach())
    r = x.detach().norm(dim=-1, keepdim=True)
    (auto,) = torch.autograd.grad(pr.neg_normalize(x), x, dn)
    assert torch.allclose(-(dn - n * (n * dn).sum(-1, keepdim=True)) / r, auto, rtol=1e-12, atol=1e-12)
    w = torch.rand(5, 6, generator=g, dtype=torch.float64).requires_grad_(True)
    nn_ = pr.neg_normalize(torch.rand(5, 6, 3, generator=g, dtype=torch.float64) - 0.5).requires_grad_(True)
    v = pr.neg_normalize(torch.rand(5, 3, generator=g, dtype=torch.float64) - 0.5)
    assert torch.autograd.gradcheck(lambda a, b: pr.orientation_term(a, b, v), (w, nn_), eps=1e-7, atol=1e-6)
    gl = torch.rand(5, generator=g, dtype=torch.float64)
    aw, an = torch.autograd.grad(pr.orientation_term(w, nn_, v), (w, nn_), gl)
    d = (nn_.detach() * (-v)[:, None, :]).sum(-1).clamp_min(0)
    assert torch.allclose(gl[:, None] * d ** 2, aw) and torch.allclose((gl[:, None] * w.detach() * 2 * d)[..., None] * (-v)[:, None, :], an)
    # the clamp: g = 0 gives 0, not NaN, and a finite backward -dn / eps
    z = torch.zeros(1, 3, dtype=torch.float64, requires_grad=True)
    out = pr.neg_normalize(z)
    (gz,) = torch.autograd.grad(out, z, torch.ones(1, 3, dtype=torch.float64))
    assert torch.equal(out.detach(), torch.zeros(1, 3, dtype=torch.float64)) and torch.allclose(gz, torch.full((1, 3), -1.0 / pr.EPS32, dtype=torch.float64))


def test_result_dictionaries_carry_the_new_keys_only_when_asked():
    from ucnerf_amd.internal import march_level as ml
    N, S = 3, 4
    g = torch.Generator().manual_seed(1)
    w, gp = torch.rand(N, S, generator=g), torch.rand(N, S, 3, generator=g)
    npred = pr.neg_normalize(gp)
    coord, density, sdist = torch.zeros(N, S, 3), torch.zeros(N, S), torch.zeros(N, S + 1)
    h = ml.history_entry(coord, density, None, sdist, w, (N,))
    assert h["grad_pred"] is None and h["normals_pred"] is None
    h = ml.history_entry(coord, density, None, sdist, w, (N, 1), grad_pred=gp, normals_pred=npred)
    assert h["grad_pred"].shape == (N, 1, S, 3) and torch.equal(h["normals_pred"].reshape(N, S, 3), npred)
    assert h["normals"] is None and h["raw_grad_density"] is None
    main, extras = torch.zeros(N, 5), torch.zeros(N, 4)
    r = ml.rendering_entry(main[:, :3], main[:, 3], main[:, 4], w, extras, (N,), sdist)
    assert "normals_pred" not in r and "normals" not in r
    r = ml.rendering_entry(main[:, :3], main[:, 3], main[:, 4], w, None, (N,), sdist, normals_pred=npred)
    assert "normals_pred" not in r                                          # compute_extras off
    r = ml.rendering_entry(main[:, :3], main[:, 3], main[:, 4], w, extras, (N,), sdist, normals_pred=npred)
    assert torch.allclose(r["normals_pred"], (w[..., None] * npred).sum(-2)) and "normals" not in r


def test_overlay_exports_orientation_loss():
    import ucnerf_amd
    path = os.path.join(os.path.dirname(ucnerf_amd.__file__), "compat", "dropin", "internal", "train_utils.py")
    names = {a.name for node in ast.walk(ast.parse(open(path).read())) if isinstance(node, ast.ImportFrom)
             and node.module == "ucnerf_amd.internal.train_utils" for a in node.names}
    assert "orientation_loss" in names
    from ucnerf_amd.internal import train_utils
    assert callable(train_utils.orientation_loss)


def test_flag_off_routes_are_unchanged():
    from ucnerf_amd.internal import models
    from ucnerf_amd.internal import train_graph as tg
    plain, head = models.NerfMLP(**KW), models.NerfMLP(enable_pred_normals=True, **KW)
    assert "normal_layer" not in dict(plain.named_modules())
    assert tg.heads_route(plain, 24, True, None, None) == "field_node_f32"
    for autocast in (None, torch.bfloat16):
        for glo in (None, (None, None)):
            assert tg.heads_route(head, 24, True, autocast, glo) == "colour_node"
    # a colour width the fp32 kernels' 16-byte operand loads do not take: the colour node's own condition holds for the head's route too
    odd = models.NerfMLP(enable_pred_normals=True, net_width_viewdirs=100, **KW)
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        tg.heads_route(odd, 24, True, None, None)
