"""Differentiable (training) form of Model.forward -- SURVEY.md 8(a15/a16).

What carries gradients in the reference's training step (train.py:165-221): the hash tables (through
_grid_encode.backward, grid.py:68-89), the MLP weights, and -- when enabled -- the sky / colour-correction
parameters.  Sample positions do not (`stop_level_grad`, models.py:204-205; `track_linearize` is
@torch.no_grad, coord.py:75).  Here:

* resampling, cone basis and the fused cast/contract/hash-grid/erf featurisation are the same HIP kernels as
  in rendering; the featurisation's backward (`ucn_march_features_backward`: LDS row blocks + compaction, no
  global atomics) is hand-written HIP and replaces kernel_grid_backward + the autograd of the erf/mean glue;
* alpha compositing (weights, rgb, depth, acc) is `ucn_composite` forward and `ucn_composite_backward`;
* the dense layers run as library GEMMs under torch autograd (hipBLASLt; bf16 under autocast like the reference's
  `accelerator.autocast()`), arranged so that nothing of size [N*S, 283] / [N*S, 539] is ever concatenated and the
  weight / bias gradients are split-K batched GEMMs.  A fused MFMA backward on the register-chained engine is the
  next step; until then this is a GPU path through vendor GEMMs, not a fallback to the CPU:
  host tensors still raise.

This file is the wiring: `heads_route` (the ONE place that decides a level's dense route, for `field_heads` and for the mixed-precision
inference march), `field_heads`, `march_train`.  The nodes live in march_nodes.py, heads_bf16.py, heads_f32.py, sky_train.py and
head_pack.py; their names are imported here, `field_heads` and `march_train` call them through this namespace (tests and tools patch it).
"""
import os

import torch
import torch.nn.functional as F

from .. import _lib
from . import dense_f32
from . import march_level as ml
from .head_pack import (_acc_vec, _head_gather_index, _pack_fragments, _weave, prepare_heads,  # noqa: F401  (the packer: tests, tools)
                        rgb_activation, view_encoding)
from .heads_bf16 import _FusedHeads, _PropHeads, wgrad  # noqa: F401
from .heads_f32 import (_ColourMLP, _ColourMLPComposed, _ColourMLPGlo, _FieldMLPComposed, _TallLinear,  # noqa: F401
                        tall_affine, tall_linear, tall_matmul)
from .march_nodes import (GradientScaler, _AffineBlend, _Composite, _CompositeRays, _FieldFeatures, _GradChannel, _NegNormalize, _RefColour, _tail_fusable,  # noqa: F401
                          brightness_forward, hash_decay, scale_features)
from .sky_train import _sky_fusable, sky_forward, sky_forward_fused


# ------------------------------------------------------------------ which dense route a level takes
def _prop_shape(mlp, n_features, on_device, autocast_dtype):
    """what `ucn_prop_train_fwd / _bwd` take: the reference's proposal field (Linear(F <= 24, 64) + ReLU, Linear(64, 1)), fp32 or bf16"""
    l0, l1 = mlp.density_layer[0], mlp.density_layer[2]
    return (mlp.disable_rgb and len(mlp.density_layer) == 3 and on_device and n_features <= 24 and l0.out_features == 64
            and l1.out_features == 1 and l0.bias is not None and l1.bias is not None
            and autocast_dtype in (None, torch.bfloat16))


def _heads_shape(mlp, n_features, autocast_dtype):
    """what `ucn_train_fwd / _bwd` take: the reference's NeRF field (F <= 64 -> 64 -> 256, two 256-wide colour layers, rgb) under bf16"""
    return (autocast_dtype == torch.bfloat16 and not mlp.disable_rgb
            and mlp.net_depth_viewdirs == 2 and mlp.skip_layer_dir == 0 and n_features <= 64
            and mlp.density_layer[0].out_features == 64 and mlp.density_layer[2].out_features == 256
            and mlp.net_width_viewdirs == 256 and mlp.rgb_layer.out_features == 3)


def _autocast_dtype():
    return torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else None


def _fusable_prop(mlp, feat):
    return _prop_shape(mlp, feat.shape[1], feat.is_cuda, _autocast_dtype())


def _fusable_heads(mlp, feat):
    return _heads_shape(mlp, feat.shape[1], _autocast_dtype())


def heads_route(mlp, n_features, on_device_f32, autocast_dtype, glo):
    """The route of `mlp`'s dense layers over [M, n_features] features, from the arguments and the environment (switches read per call):
    "fused_bf16" _FusedHeads | "prop_fused" _PropHeads | "field_node_f32" _FieldMLPComposed | "composed_f32" the same as three nodes |
    "colour_node" _ColourMLP / _ColourMLPGlo between tall_linear layers (csrc/gemm_f32.hip; library GEMMs under autocast or
    UCN_F32_LIBRARY=1) | "generic" layer by layer.  on_device_f32: features and first weight are float32 device tensors;
    autocast_dtype: torch.get_autocast_dtype("cuda") under autocast, else None; glo: the per-ray GLO modulation or None (a per-ray
    diagonal between bottleneck and colour layers: the routes that fuse or compose the two are out)."""
    if getattr(mlp, 'enable_pred_normals', False):
        # the predicted-normal head reads the bottleneck (models.py:570): the one route that materialises it between the density and
        # the colour layers, in fp32 and under autocast, with and without GLO
        # (the colour node's own condition below: the reference's topology at a width the fp32 kernels' 16-byte operand loads take)
        if mlp.disable_rgb or mlp.net_depth_viewdirs != 2 or mlp.skip_layer_dir != 0 or mlp.net_width_viewdirs % 8 != 0:
            raise NotImplementedError("enable_pred_normals in the training graph needs the reference's colour topology (net_depth_viewdirs = 2, "
                                      f"skip_layer_dir = 0) at a net_width_viewdirs that is a multiple of 8, got {mlp.net_width_viewdirs}")
        return "colour_node"
    if getattr(mlp, 'ref_heads_mask', lambda: 0)():
        # the Ref-NeRF colour heads read the bottleneck too (models.py:589-597): the same route, under the same condition
        if mlp.net_depth_viewdirs != 2 or mlp.skip_layer_dir != 0 or mlp.net_width_viewdirs % 8 != 0:
            raise NotImplementedError("use_diffuse_color / use_specular_tint / enable_pred_roughness in the training graph need the reference's "
                                      "colour topology (net_depth_viewdirs = 2, skip_layer_dir = 0) at a net_width_viewdirs that is a multiple "
                                      f"of 8, got {mlp.net_width_viewdirs}")
        return "colour_node"
    fused = os.environ.get("UCN_FUSED_HEADS", "1") == "1"
    if glo is None and fused and _heads_shape(mlp, n_features, autocast_dtype):
        return "fused_bf16"
    if fused and _prop_shape(mlp, n_features, on_device_f32, autocast_dtype):
        return "prop_fused"
    # the reference's colour topology, at a width the fp32 kernels' 16-byte operand loads take
    colour = not mlp.disable_rgb and mlp.net_depth_viewdirs == 2 and mlp.skip_layer_dir == 0 and mlp.net_width_viewdirs % 8 == 0
    if (glo is None and colour and autocast_dtype is None and on_device_f32 and not dense_f32.library_route()
            and os.environ.get("UCN_F32_COMPOSED", "1") == "1"):        # 0: the uncomposed _ColourMLP on the same kernels (A/B, cross-check)
        # r06: one node; 0: three nodes (A/B, cross-check)
        return "field_node_f32" if os.environ.get("UCN_FIELD_NODE", "1") != "0" and n_features % 4 == 0 else "composed_f32"
    return "colour_node" if colour else "generic"


def _heads_fused_bf16(mlp, feat, viewdirs, N, S, chan, glo):
    d0, d1, l0, l1, lr = mlp.density_layer[0], mlp.density_layer[2], mlp.lin_second_stage_0, mlp.lin_second_stage_1, mlp.rgb_layer
    density, rgb = _FusedHeads.apply(feat, view_encoding(viewdirs, mlp.deg_view), d0.weight, d0.bias, d1.weight, d1.bias,
                                     l0.weight, l0.bias, l1.weight, l1.bias, lr.weight, lr.bias, N, S,
                                     (mlp.density_bias, mlp.rgb_premultiplier, mlp.rgb_bias, mlp.rgb_padding), chan)
    return density.reshape(N, S), rgb.reshape(N, S, 3)


def _heads_prop_fused(mlp, feat, viewdirs, N, S, chan, glo):
    l0, l1 = mlp.density_layer[0], mlp.density_layer[2]
    density = _PropHeads.apply(feat, l0.weight, l0.bias, l1.weight, l1.bias, mlp.density_bias, torch.is_autocast_enabled())
    return density.reshape(N, S), torch.zeros(N, S, 3, device=feat.device)


def _heads_composed_f32(mlp, feat, viewdirs, N, S, chan, glo, one_node=False):
    # the fp32 step on hand-written kernels, the bottleneck composed into the colour layers (_ColourMLPComposed)
    lin = dense_f32.hip_linear
    d0l, d1l, l0, l1 = mlp.density_layer[0], mlp.density_layer[2], mlp.lin_second_stage_0, mlp.lin_second_stage_1
    NB = d1l.out_features
    NW = l0.out_features
    enc = view_encoding(viewdirs, mlp.deg_view)                                              # [N, 27], per ray
    Wd1t = d1l.weight.t()                                                                    # [64, NB] (view: autograd transposes back)
    W0x, W0e = l0.weight[:, :NB], l0.weight[:, NB:]
    W1h, W1x, W1e = l1.weight[:, :NW], l1.weight[:, NW:NW + NB], l1.weight[:, NW + NB:]
    A0, A1 = lin(W0x, Wd1t), lin(W1x, Wd1t)                                                  # W_ix Wd1   [NW, 64]
    pr0 = lin(enc, W0e, l0.bias) + lin(d1l.bias[None, :], W0x)                               # [N, NW] + [1, NW]
    pr1 = lin(enc, W1e, l1.bias) + lin(d1l.bias[None, :], W1x)
    if one_node:
        # r06: density layer 0, the density row and the colour MLP as one node (_FieldMLPComposed)
        raw, rgbl = _FieldMLPComposed.apply(feat, d0l.weight, d0l.bias, d1l.weight[:1], d1l.bias[:1], A0, pr0, W1h, A1, pr1,
                                            mlp.rgb_layer.weight, mlp.rgb_layer.bias, N, S)
    else:
        h0 = lin(feat, d0l.weight, d0l.bias, relu=True)                                      # [N*S, 64]
        rgbl = _ColourMLPComposed.apply(h0, A0, pr0, W1h, A1, pr1, mlp.rgb_layer.weight, mlp.rgb_layer.bias, N, S)
        raw = lin(h0, d1l.weight[:1], d1l.bias[:1])                                          # feature 0 of the bottleneck (models.py:508)
    return F.softplus(raw.reshape(N, S) + mlp.density_bias), rgb_activation(mlp, rgbl.reshape(N, S, -1))


def ref_colour_heads(mlp, x, logits):
    """models.py:589-597 and :657-674 on the bottleneck x [B, NB] (before the GLO modulation) and the colour logits [B, 3] of a field with
    Ref-NeRF colour heads: (rgb [B, 3], roughness [B, 1] float32 or None).  The rows of the heads that are READ -- diffuse 3, tint 3 (beside
    the diffuse colour only: models.py:665), roughness 1 -- go through ONE stacked product on x (autograd's cat splits the weight gradient);
    the colour is `_RefColour`, the roughness a softplus on its column.  An unread specular_layer gets no gradient, as in the reference."""
    layers = [mlp.diffuse_layer] if mlp.use_diffuse_color else []
    if mlp.use_diffuse_color and mlp.use_specular_tint:
        layers.append(mlp.specular_layer)
    if mlp.enable_pred_roughness:
        layers.append(mlp.roughness_layer)
    raw = None
    if layers:
        # (the stack is part of the graph: its backward hands each layer its rows of the weight gradient; R x bottleneck floats per step)
        W = torch.cat([l.weight for l in layers], dim=0) if len(layers) > 1 else layers[0].weight
        b = torch.cat([l.bias for l in layers], dim=0) if len(layers) > 1 else layers[0].bias
        raw = tall_affine(x, W, b).float()
    roughness = F.softplus(raw[:, -1:] + mlp.roughness_bias) if mlp.enable_pred_roughness else None
    if not mlp.use_diffuse_color:
        return rgb_activation(mlp, logits), roughness
    raw_tint = raw[:, 3:6] if mlp.use_specular_tint else None
    return _RefColour.apply(logits, raw[:, 0:3], raw_tint, mlp.rgb_premultiplier, mlp.rgb_bias, mlp.rgb_padding), roughness


def _heads_colour_node(mlp, feat, viewdirs, N, S, chan, glo, with_x=False):
    x = tall_linear(mlp.density_layer[2], tall_linear(mlp.density_layer[0], feat, relu=True))    # [N*S, bottleneck]
    enc = view_encoding(viewdirs, mlp.deg_view)                                                  # [N, 27], per ray
    l0, l1 = mlp.lin_second_stage_0, mlp.lin_second_stage_1                                      # the reference's topology
    if glo is not None:
        h, raw = _ColourMLPGlo.apply(x, glo[0], glo[1], enc, l0.weight, l0.bias, l1.weight, l1.bias, N, S)
    else:
        h, raw = _ColourMLP.apply(x, enc, l0.weight, l0.bias, l1.weight, l1.bias, N, S)
    density = F.softplus(raw.reshape(N, S) + mlp.density_bias)
    roughness = None
    if getattr(mlp, 'ref_heads_mask', lambda: 0)():
        rgb, roughness = ref_colour_heads(mlp, x, tall_linear(mlp.rgb_layer, h))
        rgb = rgb.reshape(N, S, -1)
    else:
        rgb = rgb_activation(mlp, tall_linear(mlp.rgb_layer, h).reshape(N, S, -1))
    return (density, rgb, x, roughness) if with_x else (density, rgb)


def _heads_generic(mlp, feat, viewdirs, N, S, chan, glo):
    x = tall_linear(mlp.density_layer[2], tall_linear(mlp.density_layer[0], feat, relu=True))    # [N*S, bottleneck]
    if mlp.disable_rgb:
        return F.softplus(x.reshape(N, S, -1)[..., 0] + mlp.density_bias), torch.zeros(N, S, 3, device=feat.device)
    enc = view_encoding(viewdirs, mlp.deg_view)                                                  # [N, 27], per ray
    if glo is not None:
        raise NotImplementedError("GLO modulation needs the reference's colour topology (net_depth_viewdirs = 2, skip_layer_dir = 0)")
    density = F.softplus(x.reshape(N, S, -1)[..., 0] + mlp.density_bias)
    per_sample, skip, with_enc = [x], [x], True            # column blocks of the next layer's input, in cat order
    for i in range(mlp.net_depth_viewdirs):
        lin = mlp.get_submodule(f"lin_second_stage_{i}")
        col, pre = 0, None
        for blk in per_sample:
            pre = tall_matmul(blk, lin.weight[:, col:col + blk.shape[-1]], pre)
            col += blk.shape[-1]
        per_ray = F.linear(enc, lin.weight[:, col:], lin.bias) if with_enc else lin.bias[None, :]   # [N | 1, width]
        h = F.relu(pre.reshape(N, S, -1) + per_ray[:, None, :].to(pre.dtype)).reshape(N * S, -1)
        with_enc = i == mlp.skip_layer_dir                  # the direction block enters at layer 0 and after the skip
        per_sample = [h] + skip if with_enc else [h]
    assert len(per_sample) == 1, "skip connection into the rgb layer is not part of the reference configs"
    return density, rgb_activation(mlp, tall_linear(mlp.rgb_layer, h).reshape(N, S, -1))


_HEADS = {"fused_bf16": _heads_fused_bf16, "prop_fused": _heads_prop_fused, "field_node_f32": lambda *a: _heads_composed_f32(*a, one_node=True),
          "composed_f32": _heads_composed_f32, "colour_node": _heads_colour_node, "generic": _heads_generic}


def field_heads(mlp, feat, viewdirs, N, S, chan=None, glo=None):
    """models.py:507-674 on [N*S, F] features: density MLP, softplus, colour MLP, on the route `heads_route` names.

    glo = (a, b), float32 [N, bottleneck] (MLP.glo_affine): the GLO modulation of the bottleneck, per ray.  It takes the
    uncomposed route (_ColourMLPGlo); the fused / composed routes fold the bottleneck layer into the colour layers and are
    only taken without it.

    The reference concatenates [bottleneck, dir_enc] (and [h, bottleneck, dir_enc] after the skip layer) per SAMPLE
    and multiplies by one weight.  The same product is formed here column block by column block: per-sample blocks
    as GEMMs that accumulate into one output, the per-RAY direction block (and the layer bias) as one small
    [N, 27] GEMM broadcast over the samples -- no [N*S, 283] / [N*S, 539] concatenations, 7 % fewer flops, and the
    bias / direction-weight gradients reduce over rays instead of samples."""
    route = heads_route(mlp, feat.shape[1], dense_f32.device_f32(feat, mlp.density_layer[0].weight), _autocast_dtype(), glo)
    return _HEADS[route](mlp, feat, viewdirs, N, S, chan, glo)


def field_heads_pred(mlp, feat, viewdirs, N, S, chan=None, glo=None):
    """`field_heads` of a field with MLP.enable_pred_normals, plus its head (models.py:569-578): (density [N, S], rgb [N, S, 3],
    grad_pred [N, S, 3] float32).  grad_pred = normal_layer(x) on the bottleneck x the colour node's route materialises (before the GLO
    modulation), through tall_linear: autograd carries its gradient into normal_layer, the density layers and the tables."""
    route = heads_route(mlp, feat.shape[1], dense_f32.device_f32(feat, mlp.density_layer[0].weight), _autocast_dtype(), glo)
    assert route == "colour_node", route
    density, rgb, x, _ = _heads_colour_node(mlp, feat, viewdirs, N, S, chan, glo, with_x=True)
    return density, rgb, tall_linear(mlp.normal_layer, x).float().reshape(N, S, 3)


def field_heads_ref(mlp, feat, viewdirs, N, S, chan=None, glo=None):
    """`field_heads` of a field with Ref-NeRF colour heads (models.py:589-597, :661-674): (density [N, S], rgb [N, S, 3],
    grad_pred [N, S, 3] or None, roughness [N, S, 1] or None).  The heads read the bottleneck the colour node's route materialises; with
    enable_pred_normals the normal head is a product of its own on the same x, as in `field_heads_pred`."""
    route = heads_route(mlp, feat.shape[1], dense_f32.device_f32(feat, mlp.density_layer[0].weight), _autocast_dtype(), glo)
    assert route == "colour_node", route
    density, rgb, x, roughness = _heads_colour_node(mlp, feat, viewdirs, N, S, chan, glo, with_x=True)
    grad_pred = tall_linear(mlp.normal_layer, x).float().reshape(N, S, 3) if mlp.enable_pred_normals else None
    return density, rgb, grad_pred, None if roughness is None else roughness.reshape(N, S, 1)


def march_train(model, rand, batch, train_frac, compute_extras, eval_camidx, glo_vec=None):
    """Model.forward with an autograd graph (ref models.py:97-365).  glo_vec [N, num_glo_features] (or None): the NeRF level's
    per-ray GLO codes (models.py:118-127); the proposal levels get none (models.py:226)."""
    lib = _lib.load()
    model.last_march_route = 'train_graph'
    rays = ml.Rays(batch, model.num_levels)
    N, dev, prefix = rays.N, rays.dev, rays.prefix
    o, d, vd, cam, far = rays.o, rays.d, rays.vd, rays.cam, rays.far
    st, cfg = _lib.stream(), model.config
    opaque = int(bool(model.opaque_background))
    gain = ml.ray_gain(model, batch, rays)                      # the RawNeRF exposure [N, 3] (None without batch['exposure_idx']); differentiable
    renderings, ray_history = [], []
    posts = weights = None
    # The sky NeRF depends on the rays only, not on the field: with `Model.sky_side_stream` its fused forward is issued FIRST, on
    # a second HIP stream, and joins at the colour-correction step.  Autograd runs a node's backward on the stream of its
    # forward, so the sky's compositing backward, dgrad kernel and weight-gradient passes (HBM-bound: 4.4 GB of stores, 9 GB of
    # reads) run beside the field's featurisation backward (VALU / LDS-bound) as well.
    _sky_pending = None
    if (getattr(cfg, 'model_sky', False) and model.sky_side_stream and model.fused_sky_train and _sky_fusable(model.skynerf, o)):
        if getattr(model, '_sky_stream', None) is None:
            model._sky_stream = torch.cuda.Stream()
        model._sky_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(model._sky_stream):
            _sky_pending = sky_forward_fused(model.skynerf, o, d, cam, far)
        for t in (o, d, cam, far):
            t.record_stream(model._sky_stream)
    for i_level, is_prop, S, mlp, dilation in ml.level_plan(model, train_frac):
        # 'sdist' among the pinned draws (tests/test_train_full_size.py): tells 1-ulp sample positions amplified by 2^19-wide levels from a wrong backward
        posts, flip, spin = ml.fenceposts(model, rays, i_level, S, dilation, train_frac, rand, posts, weights, st,
                                          pinned_sdist=rays.noise[i_level].get('sdist') if rand else None)
        half_table = torch.is_autocast_enabled() and mlp.encoder.level_dim % 2 == 0 and getattr(model, 'autocast_half_tables', True)
        # `feat` has exactly one consumer, the heads below: the two nodes may agree on its gradient's layout.  Not with scale
        # featurization: the heads then read cat([feat, scale features]) and autograd hands gfeat[:, :L*C] back sample-major (layout 1)
        chan = None if mlp.scale_featurization else _GradChannel()
        feat, coord, tmean = _FieldFeatures.apply(mlp.encoder.embeddings, mlp, posts, rays, flip, spin, S, model.std_scale,
                                                  model.levels_per_block, half_table, chan)
        if mlp.scale_featurization:
            feat = torch.cat([feat, scale_features(mlp, posts, rays, flip, spin, S, model.std_scale)], dim=-1)
        glo = None if (is_prop or glo_vec is None) else mlp.glo_affine(glo_vec.reshape(N, -1))
        grad_pred = normals_pred = roughness = None
        if mlp.ref_heads_mask():                                      # models.py:589-597, :661-674 (and :569-578 beside them)
            density, rgbs, grad_pred, roughness = field_heads_ref(mlp, feat, vd, N, S, chan, glo)
            normals_pred = None if grad_pred is None else _NegNormalize.apply(grad_pred)
        elif mlp.enable_pred_normals:                                   # models.py:569-578; normals_pred = -l2_normalize(grad_pred)
            density, rgbs, grad_pred = field_heads_pred(mlp, feat, vd, N, S, chan, glo)
            normals_pred = _NegNormalize.apply(grad_pred)
        else:
            density, rgbs = field_heads(mlp, feat, vd, N, S, chan, glo)
        if getattr(cfg, 'brightness_correction', False):              # models.py:233-235 (gated on this flag)
            rgbs, density = GradientScaler.apply(rgbs, density, tmean)
        bg, ray_bg = ml.background(model, rays, i_level, rand)        # drawn behind the level's MLP (models.py:256)
        level_gain = None if is_prop else gain                        # a proposal level's colours are zeros (models.py:584-585): gain * 0 = 0
        if level_gain is None and ray_bg is None:
            weights, c_rgb, c_depth, c_acc = _Composite.apply(density, rgbs, posts, d, bg, opaque)
        else:
            # models.py:258-269 scales ray_results['rgb'] in place: the scaled colours are what the history and the ray bundles carry
            weights, c_rgb, c_depth, c_acc, scaled = _CompositeRays.apply(density, rgbs, level_gain, posts, d, ray_bg, bg, opaque)
            if level_gain is not None:
                rgbs = scaled
        extras = None
        if compute_extras:
            # render.py:218-242: depth percentiles and the mean distance -- not differentiated by any loss of the path
            # (train_utils.py reads them for metrics only), so they come from the rendering kernel on detached inputs
            with torch.no_grad():
                dn, rg = density.detach().float().contiguous(), rgbs.detach().float().contiguous()
                w_x, main_x, extras = torch.empty(N, S, device=dev), torch.empty(N, 5, device=dev), torch.empty(N, 4, device=dev)
                # (`rg` are the colours as composited -- already scaled by the gain, hence none here; a detached copy, so nothing is overwritten)
                ml.composite(posts, dn, rg, d, None, ray_bg, bg, opaque, w_x, main_x, extras, st)
        raw_grad = normals = None
        if not mlp.disable_density_normals:
            # models.py:550-567, detached (the second-order path of create_graph=True is not built: Model.__init__ refuses its
            # consumers).  A level-major fp32 copy of the features becomes gfeat; the table is the fp32 one
            with torch.no_grad():
                L, C = mlp.encoder.num_levels, mlp.encoder.level_dim
                gfeat = feat.detach()[:, :L * C].float().reshape(N * S, L, C).permute(1, 0, 2).contiguous()
                raw_grad, normals = torch.empty(N, S, 3, device=dev), torch.empty(N, S, 3, device=dev)
                ml.density_normals(mlp, posts, rays, flip, spin, slice(None), N, S, model.std_scale, 0, gfeat, raw_grad, normals, st)
        out = ml.LevelOutputs(density=density, rgbs=rgbs, weights=weights, main=(c_rgb, c_depth, c_acc), extras=extras, coord=coord, raw_grad=raw_grad,
                              normals=normals, grad_pred=grad_pred, normals_pred=normals_pred, roughness=roughness)
        renderings.append(out.rendering(prefix, posts.sdist, getattr(cfg, 'vis_num_rays', 16)))
        hist = out.history(prefix, posts.sdist)
        if model.training:
            hist['loss_hash_decay'] = hash_decay(mlp)
        ray_history.append(hist)
    if compute_extras:
        ml.broadcast_final(renderings)
    with_sky = getattr(cfg, 'model_sky', False)
    if with_sky:
        # under bf16 autocast (what train.py:165 runs): the hand-written sky kernels; else the eager fp32 form (the G10 parity path)
        sky = _sky_pending if _sky_pending is not None else (
            sky_forward_fused if (model.fused_sky_train and _sky_fusable(model.skynerf, o)) else sky_forward)(model.skynerf, o, d, cam, far)
        if _sky_pending is not None:
            torch.cuda.current_stream().wait_stream(model._sky_stream)
            sky.record_stream(torch.cuda.current_stream())
        for r in renderings:
            r['sky_rgbs'] = sky
    if getattr(cfg, 'brightness_correction', False):
        idx = batch['cam_idx'].reshape(N, -1)[:, 0] if eval_camidx is None else torch.as_tensor(eval_camidx).to(dev).reshape(-1)[:1].repeat(N)
        A = brightness_forward(model.brightness_corr, idx)
        A_sky = brightness_forward(model.brightness_corr, idx, 'sky_latent_code') if with_sky else None
        last_w = renderings[-1]['weights'].reshape(N, -1)
        # models.py:350-354's per-ray 3 x 3 products as broadcast multiplies + a 3-term sum: torch.bmm with a batch of 8192
        # tiny matrices costs 1.3 ms of HOST time per call on this stack (12 calls per step forward + backward: the GPU idled
        # 45 ms of a 66 ms step, tools/train_cpu.py)
        affine = lambda M, v: (M[:, :3, :3] * v.reshape(N, 1, 3)).sum(dim=-1, keepdim=True) + M[:, :3, 3:]
        fused_tail = model.fused_heads_tail and _tail_fusable(A, A_sky, renderings[-1]['rgb'])
        acc_last = renderings[-1]['acc'].reshape(N) if (fused_tail and with_sky) else None   # = sum of the last level's weights
        if fused_tail:                       # explicit upcast (differentiable; a no-op for fp32): the kernel reads float32
            A32 = A.float().reshape(N, 12)
            A_sky32 = A_sky.float().reshape(N, 12) if with_sky else None
        for r in renderings:
            if fused_tail:
                # one launch forward + one backward per level (csrc/heads_train.hip); acc of the last level stands for the
                # sum of its weights (render.py:199: the same sum, in the compositing kernel's order)
                rgb = _AffineBlend.apply(r['rgb'].reshape(N, 3).float(), A32, acc_last,
                                         r['sky_rgbs'].reshape(N, 3).float() if with_sky else None, A_sky32)
                r['rgb'] = rgb.reshape(N, 1, 1, 3) if eval_camidx is None else rgb.reshape(N, 3)
                r['affine_trans'] = A
                if with_sky:
                    r['affine_trans_sky'] = A_sky
                continue
            rgb = affine(A, r['rgb'])
            if with_sky:
                opac = 1 - last_w.sum(dim=-1, keepdim=True)
                rgb = rgb + opac[..., None] * affine(A_sky, r['sky_rgbs'])
            r['rgb'] = rgb.reshape(N, 1, 1, 3) if eval_camidx is None else rgb.reshape(N, 3)
            r['affine_trans'] = A
            if with_sky:
                r['affine_trans_sky'] = A_sky
    return renderings, ray_history
