"""Model / NerfMLP / PropMLP / render_image -- host side of the fused HIP ray-march.

Interface mirror of /root/reference/nerf/internal/models.py (Model :31-365, MLP :367-695,
render_image :907-1007): same class names, class-attribute knobs, constructor and forward
signatures, sub-module names (=> identical ``state_dict`` keys) and the
same keys in the returned ``renderings`` / ``ray_history``.  What differs is everything below the
signature: a sampling level is five kernel launches on the caller's HIP stream
(resample -> cone basis -> fused cast/contract/hash-grid/erf features -> MFMA MLP -> wave-per-ray
composite) instead of ~300 eager ops, and nothing of size [N*S*6, .] is ever materialised.

Supported configuration = the reference's shipped one (configs/waymo.gin): disable_density_normals,
no reflections / IDE, plus GLO appearance codes (num_glo_features > 0; DESIGN.md "GLO") and every
ray-distance curve of coord.construct_ray_warps (raydist_fn None, 'piecewise', 'power_transformation' or a gin-bound
torch.reciprocal / log / exp / sqrt / square; DESIGN.md "Ray-distance curves") and the featurized grid scale
(MLP.scale_featurization) and analytic density normals (MLP.disable_density_normals = False) and the
predicted-normal head (MLP.enable_pred_normals) and the Ref-NeRF colour heads (MLP.use_diffuse_color, use_specular_tint,
enable_pred_roughness).
Anything else raises at construction.
In eval mode or with gradients disabled forward is the fused inference march (internal/march_infer.py `march`); a model in training mode
with gradients enabled routes to internal/train_graph.py `march_train` (same kernels for resampling and featurisation, HIP
backward for the tables and the dense layers' dgrad, autograd glue; `Model.march_route`).  Without the HIP library or a GPU every entry point raises.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..gridencoder import GridEncoder
from . import march_level as ml
from .head_pack import rgb_activation, view_encoding
from .extrinsic_optimizer import BrightnessCorrection
from .march_level import _f32, _u_table  # noqa: F401  (_u_table: not used here, kept importable for tests and tools)
from .sky import NeRF, render_rays  # noqa: F401  (names kept importable like upstream)


try:                                    # the reference registers its classes with gin (models.py:30,688,693); so do these,
    import gin                          # when gin is importable, so that configs/waymo.gin:10-20 binds to them unchanged
except ImportError:                     # (without gin: `bindings()` below, or constructor keyword arguments)
    gin = None


def _configurable(cls):
    return gin.configurable(cls) if gin is not None else cls


def set_kwargs(self, kwargs):
    """Instance configuration = the class-level knobs AS THEY ARE NOW (gin bindings set class attributes,
    configs/waymo.gin:10-20; `bindings()` below restores them when its block ends) overridden by the constructor's
    keyword arguments.  Frozen on the instance: a field built as 64-wide must still describe itself as 64-wide after
    the class default is back to 256 (the C descriptor is filled from these attributes on every call)."""
    for klass in reversed(type(self).__mro__):
        if klass in (nn.Module, object):
            continue
        for k, v in vars(klass).items():
            if not k.startswith('_') and not callable(v) and not isinstance(v, (property, classmethod, staticmethod)):
                object.__setattr__(self, k, v) if not isinstance(v, (torch.Tensor, nn.Module)) else None
    for k, v in kwargs.items():
        setattr(self, k, v)


def glo_fold(W0, b0, W1, b1, a, b):
    """The colour layers (lin_second_stage_0 over [bottleneck, dir_enc], lin_second_stage_1 over [h1, bottleneck, dir_enc])
    with a modulation x' = x * a + b of the bottleneck that is the SAME for every ray (a, b [NB]) folded into their weights:
        W0x <- W0x diag(a),  b0 <- b0 + W0x b;   W1x <- W1x diag(a),  b1 <- b1 + W1x b
    Exact in real arithmetic; returns new (W0, b0, W1, b1) in the parameters' dtype."""
    NB, NW = a.numel(), W0.shape[0]
    a, b = a.to(W0.dtype).reshape(-1), b.to(W0.dtype).reshape(-1)
    W0x, W1x = W0[:, :NB], W1[:, NW:NW + NB]
    W0f, W1f = W0.clone(), W1.clone()
    W0f[:, :NB] = W0x * a
    W1f[:, NW:NW + NB] = W1x * a
    return W0f, b0 + W0x @ b, W1f, b1 + W1x @ b


def _cached(obj, slot, params, build, extra=()):
    """build()'s value, kept on `obj` as `slot` = (key, value) and rebuilt only when one of `params` was updated in place or
    replaced, or `extra` (flags the value depends on) changed: key = their (data_ptr, _version), then extra."""
    key = tuple((p.data_ptr(), p._version) for p in params) + tuple(extra)
    hit = getattr(obj, slot, None)
    if hit is None or hit[0] != key:
        hit = (key, build())
        setattr(obj, slot, hit)
    return hit[1]


def _require_f32(params, what):
    """every parameter on the device (`what`: how the message names them), contiguous float32: the kernels read them through raw pointers"""
    for p in params:
        _lib.require_device(p, what)
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError("field parameters must be contiguous float32")


def _field_copy(desc, **members):
    """A copy of the descriptor `desc` with the named members overridden.  The caller keeps it, and what its pointers name, alive for
    the launches it makes with it."""
    d = _lib.UcnField()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc), ctypes.sizeof(_lib.UcnField))
    for k, v in members.items():
        setattr(d, k, v)
    return d


# Model.raydist_fn -> the curve id of include/ucnerf_march.h (UCN_RAYDIST_*).  coord.py:151-172 selects a callable by its
# __name__ and inverts it through `inv_mapping`; the gin-bound callables are configs.py:13-19's torch functions.
RAYDIST_CURVES = {None: _lib.RAYDIST_IDENTITY, 'piecewise': _lib.RAYDIST_PIECEWISE, 'power_transformation': _lib.RAYDIST_POWER}
RAYDIST_TORCH = {name: getattr(_lib, 'RAYDIST_' + name.upper()) for name in ('reciprocal', 'log', 'exp', 'sqrt', 'square')}


def raydist_curve(fn):
    """The curve id of a Model.raydist_fn value, or ValueError for one the reference cannot invert (torch.log1p: missing from
    inv_mapping, coord.py:164-172, a KeyError in its forward) or that is not one of the reference's curves."""
    if fn is None or isinstance(fn, str):
        if fn in RAYDIST_CURVES:
            return RAYDIST_CURVES[fn]
        raise ValueError(f"Model.raydist_fn={fn!r}: expected None, 'piecewise', 'power_transformation' or one of "
                         f"torch.{', torch.'.join(RAYDIST_TORCH)}")
    # gin hands over its configurable wrapper of the torch function (functools.wraps: same __name__, the function itself under
    # __wrapped__), so the reference's selection by __name__ (coord.py:164-172) sees through it; the chain must end at the torch
    # function of that name, because the kernels evaluate the curve themselves rather than call `fn`
    name = getattr(fn, '__name__', None)
    base = fn
    while hasattr(base, '__wrapped__'):
        base = base.__wrapped__
    if name in RAYDIST_TORCH and base is getattr(torch, name):
        return RAYDIST_TORCH[name]
    if base is getattr(torch, str(name), None):
        raise ValueError(f"Model.raydist_fn=torch.{name}: the reference has no inverse for it (coord.py:164-172 inv_mapping "
                         f"holds {', '.join(RAYDIST_TORCH)})")
    raise ValueError(f"Model.raydist_fn={fn!r}: only the reference's curves are supported (None, 'piecewise', "
                     f"'power_transformation', torch.{', torch.'.join(RAYDIST_TORCH)}); the HIP kernels evaluate each "
                     "curve and its inverse themselves (csrc/raydist.h)")


class MLP(nn.Module):
    """One hash-grid field (ref models.py:367-685).  Holds the parameters in the reference's
    layout; evaluation is ucnerf_amd/csrc/{march_features,field_mlp}.hip."""
    bottleneck_width: int = 256
    net_depth_viewdirs: int = 2
    net_width_viewdirs: int = 256
    skip_layer_dir: int = 0
    num_rgb_channels: int = 3
    deg_view: int = 4
    use_reflections: bool = False
    use_directional_enc: bool = False
    enable_pred_roughness: bool = False
    use_diffuse_color: bool = False
    use_specular_tint: bool = False
    use_n_dot_v: bool = False
    bottleneck_noise: float = 0.0
    density_bias: float = -1.
    density_noise: float = 0.
    rgb_premultiplier: float = 1.
    rgb_bias: float = 0.
    rgb_padding: float = 0.001
    roughness_bias: float = -1.
    enable_pred_normals: bool = False
    disable_density_normals: bool = True     # waymo.gin:15,17 (upstream class default is False)
    disable_rgb: bool = False
    warp_fn = 'contract'
    num_glo_features: int = 0
    num_glo_embeddings: int = 1000
    scale_featurization: bool = False
    grid_num_levels: int = 10
    grid_level_interval: int = 2
    grid_level_dim: int = 4
    grid_base_resolution: int = 16
    grid_disired_resolution: int = 8192
    grid_log2_hashmap_size: int = 21
    net_width_glo: int = 128
    net_depth_glo: int = 2
    # ---- knob of this implementation (not in the reference): arithmetic of the dense layers
    #   0 = fp32-input MFMA (exact fp32 products; 157 TF ceiling)
    #   1 = split-f16 MFMA, fp32 accumulate (hi/lo f16 operands, ~3e-7 relative per product; 5.3x rate)
    mlp_mode: int = 1
    bwd_fixed_point: bool = True      # autocast training step: table-gradient row blocks in guaranteed-range fixed point (UCN_BWD_FIXED_POINT)

    def __init__(self, **kwargs):
        super().__init__()
        set_kwargs(self, kwargs)
        # the rest of the reference's Ref-NeRF branch, each refused by name
        if self.use_reflections or self.use_n_dot_v:
            k = 'use_reflections' if self.use_reflections else 'use_n_dot_v'
            raise NotImplementedError(
                f"{type(self).__name__}.{k}=True: the colour layers would read a per-SAMPLE direction term (the reflected direction's "
                "encoding, the normal's dot product with the view direction); the fused field kernels take one direction tile per ray. "
                "Supported of the Ref-NeRF branch: use_diffuse_color, use_specular_tint, enable_pred_roughness, enable_pred_normals "
                "(DESIGN.md 7i)")
        if self.use_directional_enc:
            raise NotImplementedError(
                f"{type(self).__name__}.use_directional_enc=True: the reference's own forward fails on the integrated directional "
                "encoding without use_reflections and enable_pred_roughness together (sigma * None, a per-ray against per-sample "
                "broadcast), and use_reflections is not built (DESIGN.md 7i)")
        unsupported = dict(net_depth_viewdirs=2, skip_layer_dir=0, num_rgb_channels=3,
                           bottleneck_noise=0.0, density_noise=0.0)
        for k, want in unsupported.items():
            if getattr(self, k) != want:
                raise NotImplementedError(
                    f"{type(self).__name__}.{k}={getattr(self, k)!r}: the HIP ray-march implements the shipped "
                    f"waymo.gin configuration only ({k}={want!r})")
        if self.warp_fn not in ('contract', None):
            # ref coord.py:93-96: track_linearize raises for anything else
            raise NotImplementedError(
                f"{type(self).__name__}.warp_fn={self.warp_fn!r}: supported are 'contract' (the unbounded scene contracted into "
                "the grid) and None (a bounded scene inside [-1, 1]^3, the Gaussians reach the grid as they are)")
        # the kernels' `warp` argument, resolved once: 1 = 'contract', 0 = None
        self.warp = 1 if self.warp_fn == 'contract' else 0
        if not self.disable_density_normals and self.scale_featurization:
            raise NotImplementedError(
                f"{type(self).__name__}: disable_density_normals=False with scale_featurization=True: the density gradient's term "
                "through the scale features (their erf damping depends on the position outside the unit ball) is not built "
                "(DESIGN.md 7d)")
        if self.enable_pred_normals and not self.disable_density_normals:
            raise NotImplementedError(
                f"{type(self).__name__}: enable_pred_normals=True with disable_density_normals=False: the only consumer of both at "
                "once is predicted_normal_loss, which differentiates the density normals, and their second-order path is not built "
                "(DESIGN.md 7h)")
        if self.enable_pred_normals and self.disable_rgb:
            raise NotImplementedError(
                f"{type(self).__name__}: enable_pred_normals=True with disable_rgb=True: the reference applies normal_layer = "
                "Linear(bottleneck_width, 3) to the 1-wide density output there (models.py:440-444) and fails in forward; give the "
                "field its colour layers (disable_rgb=False)")
        self.grid_num_levels = int(np.log(self.grid_disired_resolution / self.grid_base_resolution)
                                   / np.log(self.grid_level_interval)) + 1
        self.encoder = GridEncoder(input_dim=3, num_levels=self.grid_num_levels, level_dim=self.grid_level_dim,
                                   base_resolution=self.grid_base_resolution,
                                   desired_resolution=self.grid_disired_resolution,
                                   log2_hashmap_size=self.grid_log2_hashmap_size, gridtype='hash', align_corners=False)
        last_dim = self.encoder.output_dim
        if self.scale_featurization:                 # ref models.py:436-437: one scale feature per grid level
            last_dim += self.encoder.num_levels
        self.density_layer = nn.Sequential(nn.Linear(last_dim, 64), nn.ReLU(),
                                           nn.Linear(64, 1 if self.disable_rgb else self.bottleneck_width))
        if self.enable_pred_normals:                 # ref models.py:442-444: registered here (the state dict's key order)
            self.normal_layer = nn.Linear(self.bottleneck_width, 3)
        self.dim_dir_enc = 3 + 6 * self.deg_view
        if not self.disable_rgb:
            # ref models.py:447-454: the Ref-NeRF colour heads, registered here (after normal_layer, before lin_glo_*); with
            # disable_rgb the flags do nothing, as in the reference
            if self.use_diffuse_color:
                self.diffuse_layer = nn.Linear(self.bottleneck_width, self.num_rgb_channels)
            if self.use_specular_tint:
                self.specular_layer = nn.Linear(self.bottleneck_width, 3)
            if self.enable_pred_roughness:
                self.roughness_layer = nn.Linear(self.bottleneck_width, 1)
            last_dim_rgb = self.bottleneck_width + self.dim_dir_enc
            if self.num_glo_features > 0:           # ref models.py:467-473: registered before the colour layers
                last_dim_glo = self.num_glo_features
                for i in range(self.net_depth_glo - 1):
                    self.register_module(f"lin_glo_{i}", nn.Linear(last_dim_glo, self.net_width_glo))
                    last_dim_glo = self.net_width_glo
                self.register_module(f"lin_glo_{self.net_depth_glo - 1}", nn.Linear(last_dim_glo, self.bottleneck_width * 2))
            input_dim_rgb = last_dim_rgb
            for i in range(self.net_depth_viewdirs):
                lin = nn.Linear(last_dim_rgb, self.net_width_viewdirs)
                torch.nn.init.kaiming_uniform_(lin.weight)
                self.register_module(f"lin_second_stage_{i}", lin)
                last_dim_rgb = self.net_width_viewdirs
                if i == self.skip_layer_dir:
                    last_dim_rgb += input_dim_rgb
            self.rgb_layer = nn.Linear(last_dim_rgb, self.num_rgb_channels)
        self._fields = {}          # (mlp_mode, glo fold) -> (key, ucn_field_t, packed weight stream): one packed buffer each

    _UNPICKLED = ('_fields', '_grid_desc', '_grid_desc_key', '_glo_fold', '_level_scale', '_pred_head', '_ref_head')

    # ---- the Ref-NeRF colour heads (ref models.py:447-454, :589-597, :661-674) ------------
    HEAD_DIFFUSE, HEAD_TINT, HEAD_ROUGHNESS = 1, 2, 4            # ucn_ref_heads' mask (include/ucnerf_march.h)

    def ref_heads_mask(self):
        """The mask of the colour heads this field carries: 0 for a field without them, and with disable_rgb (no layer exists)."""
        if self.disable_rgb:
            return 0
        return ((self.HEAD_DIFFUSE if self.use_diffuse_color else 0) | (self.HEAD_TINT if self.use_specular_tint else 0)
                | (self.HEAD_ROUGHNESS if self.enable_pred_roughness else 0))

    def ref_head_layers(self):
        """The present heads' layers in the row order of `ref_head`: diffuse 3, tint 3, roughness 1."""
        mask = self.ref_heads_mask()
        return [getattr(self, n) for bit, n in ((self.HEAD_DIFFUSE, 'diffuse_layer'), (self.HEAD_TINT, 'specular_layer'),
                                                (self.HEAD_ROUGHNESS, 'roughness_layer')) if mask & bit]

    def ref_head(self):
        """(A = W Wd1 [R, 64], c = W bd1 + b [R]), float32 on the device, W / b the present heads' rows stacked (diffuse 3, tint 3,
        roughness 1: R <= 7): the heads composed with density_layer.2, what ucn_ref_heads applies to the hidden layer."""
        return self._hidden_head('_ref_head', self.ref_head_layers())

    def _hidden_head(self, slot, layers):
        """(A = W Wd1 [R, 64], c = W bd1 + b [R]), float32 on the device, W / b the `layers`' rows stacked: Linear(bottleneck, .) heads
        composed with density_layer.2 (the inference kernels never materialise the bottleneck).  Two small fp32 products, recomputed
        only when one of the parameters changed."""
        d1 = self.density_layer[2]
        ps = [p for lin in layers for p in (lin.weight, lin.bias)] + [d1.weight, d1.bias]
        for p in ps:
            _lib.require_device(p, f"{type(self).__name__} parameter")

        def compose():
            with torch.no_grad(), torch.autocast('cuda', enabled=False):
                W = torch.cat([lin.weight.float() for lin in layers], dim=0)
                b = torch.cat([lin.bias.float() for lin in layers], dim=0)
                return (W @ d1.weight.float()).contiguous(), (W @ d1.bias.float() + b).contiguous()
        return _cached(self, slot, ps, compose)

    def unpadded_field(self, desc):
        """A copy of the descriptor `desc` whose rgb_padding is 0: ucn_field_mlp then leaves the colour MLP's plain sigmoid
        (x * 1 - 0, exact), what ucn_ref_heads takes as the linear specular colour.  The caller keeps it alive for its launches."""
        return _field_copy(desc, rgb_padding=0.0)

    # ---- predicted normals (ref models.py:442-444, :569-578) -------------------------
    def pred_head(self):
        """(A = Wn Wd1 [3, 64], c = Wn bd1 + bn [3]), float32 on the device: normal_layer composed with density_layer.2, what
        ucn_pred_normals applies to the hidden layer."""
        return self._hidden_head('_pred_head', [self.normal_layer])

    # ---- scale featurization (ref models.py:436-437, :497-506) ---------------------
    def scale_planes(self):
        """Pseudo-level planes the scale features occupy behind the grid planes of a level-major feature buffer: ceil(L / C)
        (plane p, channel c = the scale feature of level p*C + c), 0 without scale_featurization."""
        enc = self.encoder
        return (enc.num_levels + enc.level_dim - 1) // enc.level_dim if self.scale_featurization else 0

    @torch.no_grad()
    def level_scale(self):
        """k [L] on the device: sqrt(init_std^2 + per-level mean of sum_c embeddings^2) of the fp32 table (models.py:498-505, no
        gradient), by ucn_level_scale.  Recomputed only when the table changed: once per render, once per training step."""
        emb, enc = self.encoder.embeddings, self.encoder
        _require_f32([emb], f"{type(self).__name__}.encoder.embeddings")

        def launch():
            out = torch.empty(enc.num_levels, device=emb.device)
            ws = torch.empty(_lib.LEVEL_SCALE_WS_FLOATS, device=emb.device)
            _lib.check(_lib.load().ucn_level_scale(emb.data_ptr(), enc._offsets_np.ctypes.data, enc.num_levels, enc.level_dim,
                                                   float(enc.init_std), out.data_ptr(), ws.data_ptr(), _lib.stream()))
            return out
        return _cached(self, '_level_scale', [emb], launch)

    # ---- GLO appearance codes (ref models.py:600-614) ---------------------------------------------
    def uses_glo(self):
        return self.num_glo_features > 0 and not self.disable_rgb

    def _glo_layers(self):
        return [self.get_submodule(f"lin_glo_{i}") for i in range(self.net_depth_glo)]

    def glo_affine(self, glo_vec):
        """glo_vec [N, num_glo_features] -> (a = exp(scale), b = shift), float32 [N, bottleneck_width]: the per-ray GLO MLP
        (lin_glo_0 -> ReLU -> ... -> lin_glo_last, models.py:606-612) in torch, differentiable.  Per ray, not per sample
        (0.1 GFLOP at 8192 rays): not on the hot path."""
        g = glo_vec
        layers = self._glo_layers()
        for i, lin in enumerate(layers):
            g = lin(g)
            if i != len(layers) - 1:
                g = torch.relu(g)
        scale, shift = g.chunk(2, dim=-1)
        return torch.exp(scale).float().contiguous(), shift.float().contiguous()

    def _glo_folded(self):
        """The colour layers with the zero-code modulation folded in (glo_fold), float32 (W0, b0, W1, b1): what the fused
        inference kernels run when every ray's code is zero (zero_glo=True).  Recomputed only when a parameter changed."""
        l0, l1 = self.lin_second_stage_0, self.lin_second_stage_1
        ps = [l0.weight, l0.bias, l1.weight, l1.bias] + [p for lin in self._glo_layers() for p in (lin.weight, lin.bias)]

        def fold():
            with torch.no_grad(), torch.autocast('cuda', enabled=False):
                z = torch.zeros(1, self.num_glo_features, device=l0.weight.device)
                a, b = self.glo_affine(z)
                return tuple(t.contiguous() for t in glo_fold(l0.weight, l0.bias, l1.weight, l1.bias, a[0], b[0]))
        return _cached(self, '_glo_fold', ps, fold)          # (_glo_fold[0], the key, is part of `field`'s)

    def __getstate__(self):
        """copy.deepcopy / torch.save(model): the cached C descriptors hold raw device pointers (ctypes objects with
        pointers cannot be pickled, and would dangle in a copy anyway) -- they are rebuilt on first use."""
        state = self.__dict__.copy()
        for k in self._UNPICKLED:
            state.pop(k, None)
        state['_fields'] = {}
        return state

    # ---- C-ABI descriptor -------------------------------------------------------------------
    def _weights(self, glo_fold=False):
        ws = [self.encoder.embeddings, self.density_layer[0].weight, self.density_layer[0].bias,
              self.density_layer[2].weight, self.density_layer[2].bias]
        if not self.disable_rgb:
            colour = [self.lin_second_stage_0.weight, self.lin_second_stage_0.bias, self.lin_second_stage_1.weight,
                      self.lin_second_stage_1.bias]
            ws += (list(self._glo_folded()) if glo_fold else colour) + [self.rgb_layer.weight, self.rgb_layer.bias]
        return ws

    def field(self, mode=None, glo_fold=False):
        """ucn_field_t for the current parameters and the given arithmetic mode (default: self.mlp_mode); the
        MFMA-ordered weight copy of that mode is refreshed when any parameter was updated in place or moved
        (render: once; train: once per optimiser step).  glo_fold: the colour layers with the zero GLO code's modulation
        folded in (a GLO field marched with zero_glo=True; the key then also covers lin_glo_*)."""
        mode = int(self.mlp_mode if mode is None else mode)
        glo_fold = bool(glo_fold) and self.uses_glo()
        ws = self._weights(glo_fold)
        _require_f32(ws, f"{type(self).__name__} parameter")
        key = tuple((w.data_ptr(), w._version) for w in ws)
        if glo_fold:
            key += self._glo_fold[0]             # the folded copies are new tensors: their source parameters decide
        mode_key = (mode, glo_fold) if glo_fold else mode
        hit = self._fields.get(mode_key)
        if hit is not None and hit[0] == key:
            return hit[1]
        lib = _lib.load()
        enc = self.encoder
        d = _lib.UcnField()
        self._fill_grid(d, ws[0].data_ptr())
        d.w_d0, d.b_d0, d.w_d1, d.b_d1 = (w.data_ptr() for w in ws[1:5])
        d.n_bottleneck = 1 if self.disable_rgb else self.bottleneck_width
        if not self.disable_rgb:
            d.w_c0, d.b_c0, d.w_c1, d.b_c1, d.w_rgb, d.b_rgb = (w.data_ptr() for w in ws[5:11])
        d.n_width = self.net_width_viewdirs
        d.n_dir = self.dim_dir_enc
        d.density_bias, d.rgb_premultiplier = float(self.density_bias), float(self.rgb_premultiplier)
        d.rgb_bias, d.rgb_padding = float(self.rgb_bias), float(self.rgb_padding)
        d.mlp_mode = mode
        w_d0 = None
        if self.scale_featurization:
            # the kernels read [L + ceil(L/C)] planes of C: density_layer.0's [64, L*C + L] right-padded with zero columns to
            # that width (the padding channels of the last scale plane), rebuilt with the packed copy under the same key
            d.n_scale_planes, d.scale_init_std = self.scale_planes(), float(enc.init_std)
            with torch.no_grad():
                w_d0 = torch.zeros(ws[1].shape[0], (enc.num_levels + d.n_scale_planes) * enc.level_dim, device=ws[1].device)
                w_d0[:, :ws[1].shape[1]] = ws[1]
            d.w_d0 = w_d0.data_ptr()
        n = lib.ucn_field_packed_floats(ctypes.byref(d))
        if n == 0:
            raise RuntimeError(lib.ucn_last_error().decode())
        packed = hit[2] if hit is not None else None
        if packed is None or packed.numel() != n or packed.device != ws[0].device:
            packed = torch.empty(n, dtype=torch.float32, device=ws[0].device)
        d.packed = packed.data_ptr()
        _lib.check(lib.ucn_field_pack(ctypes.byref(d), _lib.stream()))
        self._fields[mode_key] = (key, d, packed, w_d0)        # (w_d0: kept alive for mode 0, whose kernels are not its only readers)
        return d

    def _fill_grid(self, d, emb_ptr):
        """the hash-grid members of the descriptor `d`, reading the table at `emb_ptr`"""
        enc = self.encoder
        d.embeddings = emb_ptr
        d.offsets_host = enc._offsets_np.ctypes.data
        d.grid_sizes_host = enc._sizes_np.ctypes.data
        d.num_levels, d.level_dim, d.base_resolution = enc.num_levels, enc.level_dim, enc.base_resolution
        d.log2_per_level_scale = float(np.log2(enc.per_level_scale))

    def grid_field(self):
        """ucn_field_t with only the hash-grid part filled in: all the featurisation kernels read.  The training graph
        uses it so that an optimiser step does not trigger a re-pack of the RENDERING engine's weight stream."""
        emb = self.encoder.embeddings
        _lib.require_device(emb, f"{type(self).__name__}.encoder.embeddings")
        key = (emb.data_ptr(),)
        if getattr(self, "_grid_desc_key", None) != key:
            d = _lib.UcnField()
            self._fill_grid(d, emb.data_ptr())
            self._grid_desc, self._grid_desc_key = d, key
        return self._grid_desc

    def normals_field(self):
        """A copy of `grid_field()` with the unpacked density_layer pointers: what the density-normal kernels read
        (ucn_density_feature_grad recomputes the hidden layer in fp32 from them).  No packed stream: the training
        route uses it every step.  The caller keeps it alive for the launches it makes with it."""
        grid = self.grid_field()
        ws = [self.density_layer[0].weight, self.density_layer[0].bias, self.density_layer[2].weight, self.density_layer[2].bias]
        _require_f32(ws, f"{type(self).__name__} parameter")
        return _field_copy(grid, **{k: w.data_ptr() for k, w in zip(('w_d0', 'b_d0', 'w_d1', 'b_d1'), ws)})

    def grid_field_with(self, embeddings):
        """A copy of `grid_field()` that reads another table of the same layout: the half-precision copy of an autocast pass
        (gridencoder/grid.py:41-44).  The caller keeps `embeddings` alive for as long as it uses the descriptor."""
        return _field_copy(self.grid_field(), embeddings=embeddings.data_ptr())

    # ---- reference API on explicit Gaussians (extract.py:56-57,96) ---------------------------
    @torch.no_grad()
    def predict_density(self, means, stds, rand=False, no_warp=False):
        """ref models.py:485-512.  means [..., G, 3], stds [..., G] -> (raw_density [...],
        x [..., n_out], mean contracted coordinate [..., 3]).  A warp_fn = None field never warps: no_warp changes nothing there."""
        raw, x, coord, _, _, _ = self._evaluate(means, stds, None, no_warp, want_x=True, want_normals=False)
        return raw, x, coord

    @torch.no_grad()
    def forward(self, rand, means, stds, viewdirs=None, imageplane=None, glo_vec=None, exposure=None,
                no_warp=False):
        """ref models.py:514-685 (keys of the returned dict identical).  With glo_vec [..., num_glo_features] (one code per
        ray) on a GLO field, the colour layers read the modulated bottleneck (models.py:606-614): the training graph's colour
        node (_ColourMLPGlo) on the fp32 kernel's bottleneck, without gradients."""
        if glo_vec is not None and self.uses_glo() and viewdirs is not None:
            return self._forward_glo(means, stds, viewdirs, glo_vec, no_warp)
        _, _, coord, density, rgb, (raw_grad, normals, grad_pred, normals_pred, roughness) = self._evaluate(means, stds, viewdirs, no_warp,
                                                                                                           want_x=False)
        if self.disable_rgb or viewdirs is None:
            rgb = torch.zeros(density.shape + (3,), device=density.device)
        return dict(coord=coord, density=density, rgb=rgb, raw_grad_density=raw_grad, grad_pred=grad_pred, normals=normals,
                    normals_pred=normals_pred, roughness=roughness)

    def _forward_glo(self, means, stds, viewdirs, glo_vec, no_warp):
        from .heads_f32 import _ColourMLPGlo
        raw, x, coord, _, _, (raw_grad, normals, grad_pred, normals_pred, _) = self._evaluate(means, stds, None, no_warp, want_x=True)
        prefix = raw.shape
        vd = _f32(viewdirs, -1, 3)
        N = vd.shape[0]
        B = raw.numel()
        if B % N:
            raise RuntimeError("viewdirs do not divide the sample count")
        density = torch.nn.functional.softplus(raw + self.density_bias)
        with torch.autocast('cuda', enabled=False):
            a, b = self.glo_affine(glo_vec.reshape(N, -1).float())
            l0, l1 = self.lin_second_stage_0, self.lin_second_stage_1
            h, _ = _ColourMLPGlo.apply(x.reshape(B, -1), a, b, view_encoding(vd, self.deg_view), l0.weight, l0.bias,
                                       l1.weight, l1.bias, N, B // N)
            logits = torch.nn.functional.linear(h, self.rgb_layer.weight, self.rgb_layer.bias)
        roughness = None
        if self.ref_heads_mask():
            # models.py:589-597, :661-674 on the bottleneck before the modulation: the training graph's heads and colour node, without gradients
            from .train_graph import ref_colour_heads
            with torch.autocast('cuda', enabled=False):
                rgb, roughness = ref_colour_heads(self, x.reshape(B, -1), logits)
            roughness = None if roughness is None else roughness.reshape(prefix + (1,))
        else:
            rgb = rgb_activation(self, logits)
        return dict(coord=coord, density=density, rgb=rgb.reshape(prefix + (3,)), raw_grad_density=raw_grad, grad_pred=grad_pred,
                    normals=normals, normals_pred=normals_pred, roughness=roughness)

    def _evaluate(self, means, stds, viewdirs, no_warp, want_x, want_normals=True):
        # the split-f16 kernel composes the bottleneck away; the API that returns it uses the fp32 kernel's packed copy
        mode = 0 if (want_x and not self.disable_rgb) else int(self.mlp_mode)
        no_warp = bool(no_warp) or not self.warp           # ref models.py:488: `if self.warp_fn is not None and not no_warp`
        lib = _lib.load()
        _lib.require_device(means, "means")
        prefix = means.shape[:-2]
        G = means.shape[-2]
        if not 1 <= G <= 6:
            raise RuntimeError(f"predict_density: 1..6 Gaussians per feature supported, got {G}")
        B = int(np.prod(prefix)) if len(prefix) else 1
        d = self.field(mode)
        dev = means.device
        m = _f32(means, B * G, 3)
        s = _f32(stds, B * G, 1)
        L, C = self.encoder.num_levels, self.encoder.level_dim
        feat = torch.empty((L + self.scale_planes()) * B * C, device=dev)
        coord = torch.empty(B, 3, device=dev)
        st = _lib.stream()
        _lib.check(lib.ucn_points_features(ctypes.byref(d), m.data_ptr(), s.data_ptr(), B, G, 0 if no_warp else 1, 1,
                                           feat.data_ptr(), coord.data_ptr(), st))
        if self.scale_featurization:               # the scale planes, behind the grid planes
            _lib.check(lib.ucn_points_scale_features(ctypes.byref(d), m.data_ptr(), s.data_ptr(), B, G, 0 if no_warp else 1,
                                                     self.level_scale().data_ptr(), 0, feat[L * B * C:].data_ptr(), st))
        density = torch.empty(B, device=dev)
        n_out = 1 if self.disable_rgb else self.bottleneck_width
        x = torch.empty(B, n_out, device=dev) if (want_x and not self.disable_rgb) else None
        rgb = None
        dirb = None
        spr = 1
        if viewdirs is not None and not self.disable_rgb:
            # viewdirs [..., 3] broadcast over the sample axis: samples per ray = B / #rays
            vd = _f32(viewdirs, -1, 3)
            n_rays = vd.shape[0]
            if B % n_rays:
                raise RuntimeError("viewdirs do not divide the sample count")
            spr = B // n_rays
            dirb = torch.empty(lib.ucn_field_dir_floats(ctypes.byref(d), n_rays), device=dev)
            _lib.check(lib.ucn_field_dir_bias(ctypes.byref(d), vd.data_ptr(), n_rays, dirb.data_ptr(), st))
            rgb = torch.empty(B, 3, device=dev)
        ref_mask = self.ref_heads_mask() if rgb is not None else 0           # models.py:587: the heads are evaluated beside the colours only
        d_mlp = self.unpadded_field(d) if ref_mask & self.HEAD_DIFFUSE else d  # (the diffuse head: the plain sigmoid, finished below)
        _lib.check(lib.ucn_field_mlp(ctypes.byref(d_mlp), feat.data_ptr(), B, spr, 0, _lib.ptr(dirb), density.data_ptr(),
                                     _lib.ptr(rgb), _lib.ptr(x), st))
        roughness = None
        if ref_mask & (self.HEAD_DIFFUSE | self.HEAD_ROUGHNESS):
            roughness = torch.empty(B, device=dev) if ref_mask & self.HEAD_ROUGHNESS else None
            ml.ref_heads(self, d, self.ref_head(), feat, slice(None), B, 1, 0, rgb, roughness, st)
            roughness = None if roughness is None else roughness.reshape(prefix + (1,))
        nrm = (None, None, None, None)
        if want_normals and self.enable_pred_normals:
            # models.py:569-578: the head on the hidden layer, before any GLO modulation; the MLP left the features as they were
            grad_pred, normals_pred = torch.empty(B, 1, 3, device=dev), torch.empty(B, 1, 3, device=dev)
            ml.pred_normals(d, self.pred_head(), feat, slice(None), B, 1, 0, grad_pred, normals_pred, st)
            nrm = (None, None, grad_pred.reshape(prefix + (3,)), normals_pred.reshape(prefix + (3,)))
        if want_normals and not self.disable_density_normals:
            # models.py:550-567: after the field MLP, on the same stream; the feature buffer is free and becomes gfeat in place
            nd = self.normals_field()
            raw_grad, normals = torch.empty(B, 3, device=dev), torch.empty(B, 3, device=dev)
            _lib.check(lib.ucn_density_feature_grad(ctypes.byref(nd), feat.data_ptr(), B, feat.data_ptr(), st))
            _lib.check(lib.ucn_points_density_grad(ctypes.byref(nd), m.data_ptr(), s.data_ptr(), B, G, 0 if no_warp else 1,
                                                   feat.data_ptr(), raw_grad.data_ptr(), normals.data_ptr(), st))
            nrm = (raw_grad.reshape(prefix + (3,)), normals.reshape(prefix + (3,)), None, None)
        # raw (pre-activation) density: softplus is inverted only for API parity of predict_density
        raw = None
        if want_x:
            if self.disable_rgb:
                raise NotImplementedError("predict_density on a disable_rgb field: use forward()['density']")
            raw = x[:, 0].reshape(prefix)
            x = x.reshape(prefix + (n_out,))
        return (raw, x, coord.reshape(prefix + (3,)), density.reshape(prefix),
                None if rgb is None else rgb.reshape(prefix + (3,)), nrm + (roughness,))


@_configurable
class NerfMLP(MLP):
    pass


@_configurable
class PropMLP(MLP):
    disable_rgb: bool = True      # waymo.gin:16


@_configurable
class Model(nn.Module):
    """ref models.py:31-365."""

    def __getstate__(self):
        state = self.__dict__.copy()
        for k in ('_side_stream', '_sky_stream', '_prof', '_alive_idx', '_alive_cnt', '_alive_stats', '_mixed_cache'):
            state.pop(k, None)
        return state

    num_prop_samples: int = 64
    num_nerf_samples: int = 32
    num_levels: int = 3
    bg_intensity_range = (1., 1.)
    anneal_slope: float = 10
    stop_level_grad: bool = True
    use_viewdirs: bool = True
    raydist_fn = None
    single_jitter: bool = True
    dilation_multiplier: float = 0.5
    dilation_bias: float = 0.0025
    num_glo_features: int = 0
    num_glo_embeddings: int = 1000
    learned_exposure_scaling: bool = False
    near_anneal_rate = None
    near_anneal_init: float = 0.95
    single_mlp: bool = False
    distinct_prop: bool = True
    resample_padding: float = 0.0
    opaque_background: bool = False
    power_lambda: float = -1.5
    std_scale: float = 0.5
    prop_desired_grid_size = [512, 2048]
    # ---- knobs of this implementation (not in the reference) ----
    max_chunk_rays: int = 10240          # rays per internal pass.  At S=128, F=32 the feature workspace is 168 MB: with
    #                                      the tables (64 + 24 MB) it stays inside the 256 MB Infinity Cache between the
    #                                      featurisation that writes it and the MLP that reads it (65 536: 5 % slower)
    levels_per_block: int = 0            # hash-grid levels per thread: 0 = auto (every fine level its own group, the coarse levels dealt out over them)
    overlap_streams: bool = False        # featurisation of pass i+1 beside the MLP of pass i on a second HIP stream:
    #                                      measured +1 % only (both kernels want every CU), so off by default
    rays_fastest: bool = True            # wave lanes = neighbouring rays at one sample index (L1/L2 locality)
    compact_min_weight: float = 0.0      # > 0: early-termination sample compaction at the last level of inference marches
    #                                      that return no per-sample history (render_image): density head first, then the
    #                                      colour layers only for samples whose compositing weight alpha * T reaches this
    #                                      value (pixel error <= num_nerf_samples * compact_min_weight).  The reference
    #                                      evaluates every sample (models.py:221-243).  0 = off: on a field whose samples all
    #                                      carry weight (random initialisation) the extra density pass is pure overhead

    autocast_half_tables: bool = True     # training under autocast gathers a HALF copy of the tables, like the reference's
    #                                      _grid_encode (grid.py:41-44); False keeps the fp32 tables (more exact, 2x the bytes)
    autocast_bf16_features: bool = True   # (with autocast_render) the NeRF level's features leave the gather as bf16 pairs -- what
    #                                      its bf16 MLP would round the floats to anyway: bit-identical pixels, half the
    #                                      workspace traffic
    autocast_render: bool = True          # inference marches called under bf16 autocast (the reference's render_image wraps the
    #                                      model call in accelerator.autocast(), models.py:957) run in the reference's mixed
    #                                      precision: half tables in the gather, dense layers as bf16 MFMAs (the training
    #                                      forward kernels without their stores), fp32 compositing.  False: fp32-class always
    sky_side_stream: bool = True         # (with fused_sky_train) the sky branch of a training step on a second HIP stream
    fused_sky_train: bool = True         # training under bf16 autocast runs the sky NeRF on csrc/sky_train.hip (False: eager torch)
    _warned_eval_route = False
    fused_heads_tail: bool = True        # training: per-ray colour correction + sky blend as one HIP node per level (False: eager torch)
    march_route: str = 'auto'            # which march Model.forward runs: 'auto' = the training graph iff self.training and
    #                                      autograd is enabled, else the fused inference march; 'train' / 'inference' force it
    sky_min_background: float = 0.0      # > 0: inference marches evaluate the sky layer only for rays whose background
    #                                      weight 1 - sum(weights of the last level) reaches this value; the others get
    #                                      sky_rgbs = 0 (their pixel moves by < sky_min_background * |A_sky| through
    #                                      models.py:352-354).  The reference evaluates the sky for every ray
    #                                      (models.py:326-337) and RETURNS sky_rgbs, so 0 = off is the default

    def __init__(self, config=None, **kwargs):
        super().__init__()
        set_kwargs(self, kwargs)
        self.config = config
        self._raydist_curve = raydist_curve(self.raydist_fn)         # resolved once (coord.py:151-172); 0 = identity
        for k, want in dict(single_mlp=False, distinct_prop=True, use_viewdirs=True).items():
            if getattr(self, k) != want:
                raise NotImplementedError(f"Model.{k}={getattr(self, k)!r} is outside the shipped waymo.gin path")
        for k in ('predicted_normal_loss_mult', 'predicted_normal_coarse_loss_mult'):
            # the consumer of the density normals' own gradient (the reference's create_graph=True, models.py:559): not built,
            # the normals are returned detached; both default to 0 (configs.py:85,87)
            if getattr(config, k, 0):
                raise NotImplementedError(f"config.{k}={getattr(config, k)!r}: the second-order path through the density normals "
                                          "is not built (normals are returned detached)")
        self.nerf_mlp = NerfMLP(num_glo_features=self.num_glo_features, num_glo_embeddings=self.num_glo_embeddings)
        for i in range(self.num_levels - 1):
            self.register_module(f'prop_mlp_{i}', PropMLP(grid_disired_resolution=self.prop_desired_grid_size[i]))
        for k in ('orientation_loss_mult', 'orientation_coarse_loss_mult'):
            # train_utils.orientation_loss reads every level's target (train_utils.py:282-298).  On 'normals_pred' (the default,
            # configs.py:84) it needs first-order gradients only and every level's field must carry the head; on 'normals' it would
            # differentiate the density normals, which are returned detached
            if not getattr(config, k, 0):
                continue
            target = getattr(config, 'orientation_loss_target', 'normals_pred')
            if target != 'normals_pred':
                raise NotImplementedError(f"config.{k}={getattr(config, k)!r} with orientation_loss_target={target!r}: the second-order "
                                          "path through the density normals is not built (normals are returned detached); the "
                                          "supported target is 'normals_pred'")
            fields = [self.nerf_mlp] + [self.get_submodule(f'prop_mlp_{i}') for i in range(self.num_levels - 1)]
            missing = [type(m).__name__ for m in fields if not m.enable_pred_normals]
            if missing:
                raise NotImplementedError(f"config.{k}={getattr(config, k)!r}: the orientation loss reads normals_pred of every level, "
                                          f"but {', '.join(missing)} were built without enable_pred_normals (for a proposal level: "
                                          "PropMLP.disable_rgb = False, PropMLP.enable_pred_normals = True)")
        if self.num_glo_features > 0 and not getattr(config, 'zero_glo', False):
            # ref models.py:73-75: one appearance code per training image, looked up by batch['cam_idx']
            self.glo_vecs = nn.Embedding(self.num_glo_embeddings, self.num_glo_features)
        if self.learned_exposure_scaling:
            # ref models.py:77-82 (registered here, before skynerf: the state dict's key order): a learned per-exposure colour
            # scaling, an offset from 1 that starts at 0; row 0 stays unused (march_level.ray_gain masks exposure_idx == 0)
            self.exposure_scaling_offsets = nn.Embedding(self.num_glo_embeddings, 3)
            torch.nn.init.zeros_(self.exposure_scaling_offsets.weight)
        if getattr(self.config, 'model_sky', False):
            self.skynerf = NeRF(D=8, d_in_view=3, W=256, multires_view=4, output_ch=4, skips=[4])
        if getattr(self.config, 'brightness_correction', False):
            self.brightness_corr = BrightnessCorrection(self.config.training_views,
                                                        model_sky=getattr(self.config, 'model_sky', False))

    # ------------------------------------------------------------------------------------------
    def forward(self, rand, batch, train_frac, compute_extras, zero_glo=True, eval_camidx=None):
        """ref models.py:97-365.  `batch` may carry two optional extra keys that pin the random
        draws (the reference draws them from torch's global RNG, render.py:123-124,140 and
        stepfun.py:216): 'rand_vec' [..., num_levels*3] and 'march_noise' (list of per-level dicts
        with 'jitter', 'flip', 'spin', and 'bg' [..., 3] for the random background colours of a two-valued bg_intensity_range).

        Route (`Model.march_route`): 'auto' builds the differentiable graph of train_graph.py (HIP featurisation
        forward / backward, MFMA train kernels, autograd glue) only for a model in TRAINING mode with autograd enabled
        -- what train.py:160-167 does; a model in eval mode, or any call under torch.no_grad(), runs the fully fused
        inference march, whose outputs carry no graph (an eval-mode call outside no_grad used to allocate the training
        graph's activation buffers, 2.1 GB at 8192 x 128 samples).  'train' / 'inference' force one route."""
        route = self.march_route
        if route not in ('auto', 'train', 'inference'):
            raise ValueError(f"Model.march_route={route!r}: expected 'auto', 'train' or 'inference'")
        glo_vec = self._glo_vec(batch, zero_glo)
        if route == 'train' or (route == 'auto' and self.training and torch.is_grad_enabled()):
            from . import train_graph
            return train_graph.march_train(self, rand, batch, train_frac, compute_extras, eval_camidx, glo_vec)
        if glo_vec is not None and not zero_glo:
            # per-ray codes differ: no call-wide fold exists, so the inference route is the training graph's forward without
            # gradients (correct, slower than the fused march: the fused field kernels cannot take a per-ray scale; DESIGN.md GLO)
            from . import train_graph
            with torch.no_grad():
                return train_graph.march_train(self, rand, batch, train_frac, compute_extras, eval_camidx, glo_vec)
        if route == 'auto' and torch.is_grad_enabled() and not self.training and not Model._warned_eval_route:
            Model._warned_eval_route = True
            import warnings
            warnings.warn("ucnerf_amd Model: eval-mode call with autograd enabled takes the inference route (detached outputs); "
                          "call model.train() before a training step, or set Model.march_route = 'train'", stacklevel=2)
        with torch.no_grad():
            return self._march(rand, batch, train_frac, compute_extras, eval_camidx, want_history=True)

    def _glo_vec(self, batch, zero_glo):
        """ref models.py:118-127: the NeRF level's per-ray GLO codes [N, num_glo_features] (zeros with zero_glo), or None."""
        if not self.num_glo_features > 0:
            return None
        origins = batch['origins']
        N = origins.numel() // origins.shape[-1]
        if zero_glo:
            return torch.zeros(N, self.num_glo_features, device=origins.device)
        if not hasattr(self, 'glo_vecs'):
            raise RuntimeError("Model.forward(zero_glo=False) on a model built with config.zero_glo=True: it has no glo_vecs "
                               "(per-image GLO codes); pass zero_glo=True or build the model with config.zero_glo=False")
        cam_idx = batch['cam_idx'][..., 0]
        return self.glo_vecs(cam_idx.long()).reshape(N, self.num_glo_features)

    def _march(self, rand, batch, train_frac, compute_extras, eval_camidx, want_history):
        from . import march_infer          # the fused inference march (imported on first use, like train_graph)
        return march_infer.march(self, rand, batch, train_frac, compute_extras, eval_camidx, want_history)


import contextlib


@contextlib.contextmanager
def bindings(**per_class):
    """The gin-binding mechanism of the reference (`NerfMLP.grid_level_dim = 2` in a .gin file sets a
    class attribute, configs/waymo.gin:10-20) as a context manager:
        with bindings(NerfMLP=dict(grid_level_dim=2), PropMLP=dict(grid_level_dim=2)):
            model = Model(config=cfg, num_levels=2, ...)"""
    classes = dict(Model=Model, NerfMLP=NerfMLP, PropMLP=PropMLP, MLP=MLP)
    saved = []
    try:
        for cname, attrs in per_class.items():
            cls = classes[cname]
            for k, v in attrs.items():
                saved.append((cls, k, cls.__dict__.get(k, _MISSING)))
                setattr(cls, k, v)
        yield
    finally:
        for cls, k, old in reversed(saved):
            if old is _MISSING:
                delattr(cls, k)
            else:
                setattr(cls, k, old)


_MISSING = object()


def unwrap_model(model):
    """The bare Model behind DistributedDataParallel / DataParallel / accelerate wrappers (anything whose `.module`
    is the wrapped nn.Module), as `accelerator.unwrap_model` would return it."""
    seen = 0
    while not hasattr(model, '_march') and isinstance(getattr(model, 'module', None), nn.Module) and seen < 8:
        model = model.module
        seen += 1
    if not hasattr(model, '_march'):
        raise TypeError(f"render_image: expected a ucnerf_amd Model (possibly DDP-wrapped), got {type(model).__name__}")
    return model


_TILE_ORDER = {}


def _tile_order(height, width, tile, device):
    """(perm, inv) int64 [H*W]: the frame's pixels in tile-major order (tile x tile pixel blocks, row-major inside a block
    and over the blocks; ragged blocks at the right / bottom edge) and the inverse permutation."""
    key = (height, width, tile, str(device))
    hit = _TILE_ORDER.get(key)
    if hit is None:
        r = torch.arange(height).reshape(-1, 1).expand(height, width)
        c = torch.arange(width).reshape(1, -1).expand(height, width)
        block = (r // tile) * ((width + tile - 1) // tile) + c // tile
        inside = (r % tile) * tile + c % tile
        perm = torch.argsort((block * (tile * tile) + inside).reshape(-1), stable=True)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(perm.numel())
        if len(_TILE_ORDER) > 8:
            _TILE_ORDER.clear()
        hit = _TILE_ORDER[key] = (perm.to(device), inv.to(device))
    return hit


def render_image(model, accelerator, batch, rand, train_frac, config, verbose=True, return_weights=False,
                 eval_camidx=0):
    """ref models.py:907-1007: render every pixel of an [H, W, .] ray batch.

    Same signature and returned dict (2-D buffers of the LAST level reshaped to [H, W, ...], and the
    'ray_*' visualisation bundles of every level).  The reference walks the frame in
    `render_chunk_size` pieces, pads, slices this rank's rows and all-gathers every tensor of every
    level per chunk (O(10^3) small collectives per frame).  Here each rank marches ONE contiguous
    row range of the frame in a single Model call and the finished buffers are exchanged with one
    packed all-gather per frame (ucnerf_amd/internal/dist.py) -- rays are independent, weights are
    replicated, so no other communication exists on the path."""
    from . import dist as udist
    model.eval()
    try:      # the mode is restored on EVERY exit: a failed render must not leave the next training step on the inference route
        # the reference hands over the `accelerator.prepare`d model (train.py:95,330, render.py:119,146, eval.py:103,140):
        # a DistributedDataParallel wrapper when num_processes > 1.  The march itself is a method of the bare Model.
        core = unwrap_model(model)
        height, width = batch['origins'].shape[:2]
        num_rays = height * width
        flat = {k: v.reshape((num_rays, -1)) for k, v in batch.items() if v is not None and torch.is_tensor(v)}
        # Rays are marched in TILE-major order (8 x 8 pixel blocks): a wave's 64 lanes are then the rays of one block, whose
        # samples at one depth index sit within ~8 pixel footprints of each other in BOTH image directions -- on the hash
        # grid's coarse and middle levels they share lattice cells, i.e. cache lines, and the gather's requests coalesce
        # (a 64 x 1 pixel row spreads 8x further).  Pixels do not depend on the order; the outputs are put back below.
        tile = int(getattr(config, 'render_ray_tile', 8))
        perm = inv = None
        if tile > 1 and height > 1 and width > 1 and flat['origins'].is_cuda:
            perm, inv = _tile_order(height, width, tile, flat['origins'].device)
            flat = {k: v.index_select(0, perm) for k, v in flat.items()}
        world = getattr(accelerator, 'num_processes', 1)
        rank = getattr(accelerator, 'process_index', 0)
        lo, hi = udist.shard_bounds(num_rays, world, rank)
        shard = {k: v[lo:hi] for k, v in flat.items()}
        with torch.no_grad():
            renderings, history = core._march(rand, shard, train_frac, True, eval_camidx, want_history=return_weights)
        last = renderings[-1]
        keys = [k for k in last if not k.startswith('ray_')]
        # rendering['weights'] ([H, W, S] of the last level) is 27x the pixels' payload.  The reference gathers it with
        # everything else (models.py:965-968) and so does this function by default -- the returned key set never depends
        # on the world size.  None of the reference's callers reads it unless return_weights=True (where models.py:977
        # overwrites it with the history's copy): `config.render_gather_weights = False` is the explicit opt-out that drops
        # the key at EVERY world size.
        if not return_weights and not getattr(config, 'render_gather_weights', True):
            keys = [k for k in keys if k != 'weights']
        local = {k: last[k].reshape(hi - lo, -1) for k in keys}
        if return_weights:
            local['weights'] = history[-1]['weights'].reshape(hi - lo, -1)
            local['coord'] = history[-1]['coord'].reshape(hi - lo, -1)
        shapes = {k: tuple(last[k].shape[1:]) for k in keys}
        if return_weights:
            shapes['weights'] = tuple(history[-1]['weights'].shape[1:])
            shapes['coord'] = tuple(history[-1]['coord'].shape[1:])
        gathered = udist.all_gather_rows(local, num_rays, world, rank)
        if inv is not None:
            gathered = {k: v.index_select(0, inv) for k, v in gathered.items()}
        rendering = {k: gathered[k].reshape((height, width) + shapes[k]) for k in gathered}
        # 'ray_*' bundles: vis_num_rays rays per level, drawn like the reference's final randperm subset
        bundle_keys = [k for k in last if k.startswith('ray_')]
        if bundle_keys:
            n_vis = getattr(config, 'vis_num_rays', 16)
            per_level = [{k: r[k] for k in bundle_keys} for r in renderings]
            per_level = udist.all_gather_bundles(per_level, world, rank)
            n_have = per_level[0][bundle_keys[0]].shape[0]
            pick = torch.randperm(n_have)[:n_vis].to(per_level[0][bundle_keys[0]].device)
            for k in bundle_keys:
                rendering[k] = [lvl[k][pick] for lvl in per_level]
    finally:
        model.train()                   # ref models.py:1006 (unconditional)
    return rendering
