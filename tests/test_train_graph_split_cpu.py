"""The training graph's modules (internal/train_graph.py and the five beside it), without a GPU: the one route decision of the dense
layers against a recorded table, the split-K chunk rule, who imports whom, the colour output activation."""
import ast
import itertools
import os
import types

import pytest
import torch

from ucnerf_amd.internal import head_pack, heads_bf16, heads_f32, models
from ucnerf_amd.internal import train_graph as tg

INTERNAL = os.path.dirname(os.path.abspath(tg.__file__))
BF16, FP16 = torch.bfloat16, torch.float16
SWITCHES = ("UCN_FUSED_HEADS", "UCN_F32_COMPOSED", "UCN_FIELD_NODE", "UCN_F32_LIBRARY")
ENVS = list(itertools.product("10", repeat=4))                 # '1111', '1110', ..., '0000' in the order of SWITCHES
N_FEATURES = (24, 25, 40, 42, 64, 68)
ROUTE = dict(B="fused_bf16", P="prop_fused", N="field_node_f32", C="composed_f32", K="colour_node", G="generic")
# Recorded from the if-ladder `field_heads` had before `heads_route` existed (its node classes stubbed, every combination driven
# through it).  Key: (field, autocast dtype, features float32 on the device, GLO present); value: per n_features of N_FEATURES one
# string with the route letter (ROUTE) of each of the 16 switch settings in the order of ENVS.
TABLE = {
    ("nerf", None, True, False): ('KNKCKKKKKNKCKKKK', 'KCKCKKKKKCKCKKKK', 'KNKCKKKKKNKCKKKK', 'KCKCKKKKKCKCKKKK', 'KNKCKKKKKNKCKKKK', 'KNKCKKKKKNKCKKKK'),
    ("nerf", None, True, True): ('KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK'),
    ("nerf", None, False, False): ('KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK'),
    ("nerf", None, False, True): ('KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK'),
    ("nerf", BF16, True, False): ('BBBBBBBBKKKKKKKK', 'BBBBBBBBKKKKKKKK', 'BBBBBBBBKKKKKKKK', 'BBBBBBBBKKKKKKKK', 'BBBBBBBBKKKKKKKK', 'KKKKKKKKKKKKKKKK'),
    ("nerf", BF16, True, True): ('KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK'),
    ("nerf", BF16, False, False): ('BBBBBBBBKKKKKKKK', 'BBBBBBBBKKKKKKKK', 'BBBBBBBBKKKKKKKK', 'BBBBBBBBKKKKKKKK', 'BBBBBBBBKKKKKKKK', 'KKKKKKKKKKKKKKKK'),
    ("nerf", BF16, False, True): ('KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK'),
    ("nerf", FP16, True, False): ('KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK'),
    ("nerf", FP16, True, True): ('KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK'),
    ("nerf", FP16, False, False): ('KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK'),
    ("nerf", FP16, False, True): ('KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK', 'KKKKKKKKKKKKKKKK'),
    ("prop", None, True, False): ('PPPPPPPPGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG'),
    ("prop", None, True, True): ('PPPPPPPPGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG'),
    ("prop", None, False, False): ('GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG'),
    ("prop", None, False, True): ('GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG'),
    ("prop", BF16, True, False): ('PPPPPPPPGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG'),
    ("prop", BF16, True, True): ('PPPPPPPPGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG'),
    ("prop", BF16, False, False): ('GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG'),
    ("prop", BF16, False, True): ('GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG'),
    ("prop", FP16, True, False): ('GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG'),
    ("prop", FP16, True, True): ('GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG'),
    ("prop", FP16, False, False): ('GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG'),
    ("prop", FP16, False, True): ('GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG', 'GGGGGGGGGGGGGGGG'),
}


@pytest.fixture(scope="module")
def fields():
    return dict(nerf=models.NerfMLP(), prop=models.PropMLP())            # the defaults: the reference's widths


def test_defaults_are_the_reference_widths(fields):
    nerf, prop = fields["nerf"], fields["prop"]
    assert (nerf.density_layer[0].out_features, nerf.density_layer[2].out_features, nerf.net_width_viewdirs) == (64, 256, 256)
    assert tg._heads_shape(nerf, 64, BF16) and not tg._heads_shape(nerf, 65, BF16) and not tg._heads_shape(prop, 24, BF16)
    assert tg._prop_shape(prop, 24, True, None) and not tg._prop_shape(prop, 25, True, None)
    # the wrappers the GPU tests call read the autocast state themselves: none on a machine without a GPU
    feat = torch.zeros(2, 24)
    assert not tg._fusable_heads(nerf, feat) and not tg._fusable_prop(prop, feat)


def test_heads_route_reproduces_the_recorded_table(fields, monkeypatch):
    mlps = fields
    assert len(TABLE) == 2 * 3 * 2 * 2 and all(len(cells) == 6 and all(len(c) == 16 for c in cells) for cells in TABLE.values())
    wrong = []
    for env in ENVS:
        for name, value in zip(SWITCHES, env):
            monkeypatch.setenv(name, value)
        e = ENVS.index(env)
        for (field, autocast, on_device, glo), cells in TABLE.items():
            for n, cell in zip(N_FEATURES, cells):
                got = tg.heads_route(mlps[field], n, on_device, autocast, (None, None) if glo else None)
                if got != ROUTE[cell[e]]:
                    wrong.append((field, autocast, on_device, glo, n, env, got, ROUTE[cell[e]]))
    assert not wrong, wrong[:5]


@pytest.mark.parametrize("autocast, glo", [(None, None), (BF16, None)])
def test_other_colour_topologies_are_generic(autocast, glo):
    deep = models.NerfMLP(grid_log2_hashmap_size=8)
    deep.net_depth_viewdirs = 3               # (the constructor refuses it; the route must not depend on that)
    narrow = models.NerfMLP(grid_log2_hashmap_size=8, net_width_viewdirs=100)
    for mlp in (deep, narrow):
        assert tg.heads_route(mlp, 40, True, autocast, glo) == "generic"
        assert tg.heads_route(mlp, 40, True, autocast, (None, None)) == "generic"


def test_split_k_rule_and_its_users():
    c = 8192
    assert heads_f32.split_k(3 * c) is None and heads_f32.split_k(4 * c + 1) is None
    assert heads_f32.split_k(4 * c) == 4 and heads_f32.split_k(5 * c) == 5
    m, a, b = 4 * c, 3, 8
    g = torch.Generator().manual_seed(0)
    gy, x = torch.rand(m, a, generator=g), torch.rand(m, b, generator=g)          # one sign: the bound below is for such sums
    want = gy.double().t() @ x.double()
    # rtol 1e-5: 32768 fp32 addends of one sign in chunked order
    torch.testing.assert_close(heads_f32._wgrad(gy, x).double(), want, rtol=1e-5, atol=0)
    torch.testing.assert_close(heads_bf16._colsum(gy).double(), gy.double().sum(0), rtol=1e-5, atol=0)
    act = torch.cat([torch.rand(m, 5, generator=g), x, torch.rand(m, 2, generator=g)], dim=1)
    torch.testing.assert_close(heads_bf16._wgrad_cols(gy, act, 5, 5 + b).double(), want, rtol=1e-5, atol=0)
    # short or ragged: the plain product
    assert torch.equal(heads_f32._wgrad(gy[:c + 1], x[:c + 1]), (gy[:c + 1].t() @ x[:c + 1]).float())


NAMES = """tall_linear _ColourMLP _ColourMLPGlo field_heads _fusable_heads _fusable_prop _PropHeads _FieldFeatures _FusedHeads _AffineBlend
sky_forward sky_forward_fused _sky_fusable scale_features hash_decay view_encoding _head_gather_index _weave _pack_fragments _acc_vec
prepare_heads GradientScaler march_train brightness_forward wgrad heads_route""".split()


def _imported(path):
    """module names a file imports, relative ones by their last component"""
    out = set()
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Import):
            out |= {a.name.split(".")[-1] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            out |= {(node.module or "").split(".")[-1]} | {a.name for a in node.names}
    return out


def test_import_discipline():
    family = {"head_pack", "heads_bf16", "heads_f32", "sky_train", "march_nodes"}
    for name in family:
        assert "train_graph" not in _imported(os.path.join(INTERNAL, name + ".py")), name
    assert not _imported(os.path.join(INTERNAL, "head_pack.py")) & (family | {"train_graph"})
    tree = ast.parse(open(os.path.join(INTERNAL, "models.py")).read())
    private = [n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name)
               and n.value.id in ("tg", "train_graph") and n.attr.startswith("_")]
    assert private == []
    glo = [n for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and any(a.name == "_ColourMLPGlo" for a in n.names)]
    assert [n.module for n in glo] == ["heads_f32"]
    missing = [n for n in NAMES if not hasattr(tg, n)]
    assert missing == []
    assert tg.prepare_heads is head_pack.prepare_heads and tg._ColourMLPGlo is heads_f32._ColourMLPGlo


@pytest.mark.parametrize("pre, bias, pad", [(1.0, 0.0, 0.001), (2.0, 0.5, 0.01)])
def test_rgb_activation_is_the_formula(pre, bias, pad):
    mlp = types.SimpleNamespace(rgb_premultiplier=pre, rgb_bias=bias, rgb_padding=pad)
    x = torch.linspace(-6.0, 7.0, 15).reshape(5, 3)
    want = torch.sigmoid(pre * x + bias) * (1 + 2 * pad) - pad
    assert torch.equal(head_pack.rgb_activation(mlp, x), want)
