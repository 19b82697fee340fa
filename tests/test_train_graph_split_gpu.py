"""`field_heads` takes the route `heads_route` names (-m gpu): per case the autograd graph holds that route's node and none of the
others, and one backward leaves a finite gradient on every dense parameter.  Values are held by tests/test_train_step.py."""
import pytest
import torch

from ucnerf_amd.internal import models
from ucnerf_amd.internal import train_graph as tg

pytestmark = pytest.mark.gpu

N, S = 4, 8            # M = 32 rows: one tile of the fused kernels, the smallest shape every route's kernels take
NODES = {"_FusedHeadsBackward", "_PropHeadsBackward", "_FieldMLPComposedBackward", "_ColourMLPComposedBackward", "_ColourMLPBackward",
         "_ColourMLPGloBackward"}
NODE_OF = {"fused_bf16": "_FusedHeadsBackward", "prop_fused": "_PropHeadsBackward", "field_node_f32": "_FieldMLPComposedBackward",
           "composed_f32": "_ColourMLPComposedBackward", "colour_node": "_ColourMLPBackward"}


@pytest.fixture(scope="module")
def fields():
    torch.manual_seed(3)
    # default widths; the proposal field on the reference's first proposal grid (512: 6 levels x 4 = 24 features, what its kernels take)
    return dict(nerf=models.NerfMLP().cuda(), prop=models.PropMLP(grid_disired_resolution=512).cuda())


def _graph_nodes(*outputs):
    seen, names, todo = set(), set(), [t.grad_fn for t in outputs if t.grad_fn is not None]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo += [nxt for nxt, _ in fn.next_functions]
    return names


@pytest.mark.parametrize("field, bf16, glo, env, route", [
    ("nerf", True, False, {}, "fused_bf16"),
    ("nerf", True, True, {}, "colour_node"),
    ("nerf", False, False, {}, "field_node_f32"),
    ("nerf", False, False, {"UCN_FIELD_NODE": "0"}, "composed_f32"),
    ("nerf", False, False, {"UCN_F32_COMPOSED": "0"}, "colour_node"),
    ("nerf", False, False, {"UCN_F32_LIBRARY": "1"}, "colour_node"),
    ("prop", False, False, {}, "prop_fused"),
    ("prop", True, False, {}, "prop_fused"),
])
def test_field_heads_runs_the_node_heads_route_names(fields, monkeypatch, field, bf16, glo, env, route):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mlp = fields[field]
    mlp.zero_grad(set_to_none=True)
    g = torch.Generator(device="cuda").manual_seed(11)
    feat = torch.randn(N * S, mlp.encoder.output_dim, device="cuda", generator=g).requires_grad_()
    vd = torch.nn.functional.normalize(torch.randn(N, 3, device="cuda", generator=g), dim=-1)
    film = None
    if glo:
        film = (torch.exp(0.1 * torch.randn(N, mlp.bottleneck_width, device="cuda", generator=g)).requires_grad_(),
                (0.1 * torch.randn(N, mlp.bottleneck_width, device="cuda", generator=g)).requires_grad_())
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        named = tg.heads_route(mlp, feat.shape[1], True, torch.bfloat16 if bf16 else None, film)
        density, rgb = tg.field_heads(mlp, feat, vd, N, S, None, film)
    assert named == route
    want = "_ColourMLPGloBackward" if (named == "colour_node" and glo) else NODE_OF[named]
    assert _graph_nodes(rgb, density) & NODES == {want}
    assert density.shape == (N, S) and rgb.shape == (N, S, 3)
    (rgb.float().sum() + density.float().sum()).backward()
    torch.cuda.synchronize()
    dense = {k: p for k, p in mlp.named_parameters() if not k.startswith("encoder.")}
    assert dense and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in dense.values()), \
        [k for k, p in dense.items() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert bool(torch.isfinite(feat.grad).all())
    if glo:
        assert all(bool(torch.isfinite(t.grad).all()) for t in film)
