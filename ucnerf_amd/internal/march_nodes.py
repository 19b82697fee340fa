"""Autograd nodes of the training march around the dense layers: featurisation, compositing, hash decay, `GradientScaler` and the
colour-correction tail -- rendering kernels and their hand-written backwards; `march_train` (train_graph.py) wires them."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib
from . import dense_f32


class _GradChannel:
    """What the featurisation node and the ONE consumer of its features agree on about the feature gradient's layout (r06).  A plain object,
    not a dict: torch.amp.custom_fwd(cast_inputs=...) rebuilds every container argument, a dict would arrive as a copy."""
    __slots__ = ("feat_ptr", "levels", "level_dim", "lm")

    def __init__(self):
        self.feat_ptr = self.levels = self.level_dim = self.lm = None


class _FieldFeatures(torch.autograd.Function):
    """features[N*S, L*C] = HIP featurisation of one level; backward scatters into the table gradient.  `posts` (march_level.Fenceposts)
    with `rays`, `flip` and `spin` is the geometry, and picks the entry points (the metric-fencepost siblings for a warped Model.raydist_fn)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, embeddings, mlp, posts, rays, flip, spin, S, std_scale, lpb, half_table=False, chan=None):
        lib = _lib.load()
        desc = mlp.grid_field()
        N, L, C = rays.N, mlp.encoder.num_levels, mlp.encoder.level_dim
        ctx.chan = chan
        layout = 1 | _lib.RAYS_INCOHERENT               # a training batch is random rays (datasets.py:278): see include/ucnerf_march.h
        if half_table:
            # gridencoder/grid.py:41-44: under autocast (and C even) the reference gathers `embeddings.to(torch.half)`.
            # Same here -- half the bytes per corner, a 2 MiB level slice per XCD L2 -- with fp32 interpolation arithmetic
            # (the reference's is half); the table gradient stays fp32 (grid.py:77-89 converts it back as well)
            emb16 = embeddings.detach().to(torch.half)
            desc, layout = mlp.grid_field_with(emb16), layout | _lib.TABLE_F16
        feat = torch.empty(N * S, L * C, device=embeddings.device)
        coord = torch.empty(N, S, 3, device=embeddings.device)
        tmean = torch.empty(N, S, device=embeddings.device)
        _lib.check(posts.ray_call(
            lib, 'ucn_march_features', ctypes.byref(desc), rays, flip, spin, slice(None), std_scale, mlp.warp, N, S, int(lpb), layout,
            feat.data_ptr(), coord.data_ptr(), tmean.data_ptr(), _lib.stream()))
        ctx.mlp, ctx.posts, ctx.cones, ctx.dims = mlp, posts, (rays, flip, spin), (N, S, float(std_scale), int(lpb))
        # the autocast step (half tables): the table gradient's row blocks accumulate in guaranteed-range fixed point (order-
        # independent, one LDS add per channel pair); the fp32 step keeps exact fp32 adds (include/ucnerf_march.h UCN_BWD_FIXED_POINT)
        ctx.fixed = bool(half_table) and bool(getattr(mlp, 'bwd_fixed_point', True))
        ctx.mark_non_differentiable(coord, tmean)
        if chan is not None:
            # r06 (VERDICT r05 item 2 c): tell the node that consumes `feat` -- and nothing else does, see train_graph.march_train -- that its feature
            # gradient may come back LEVEL-MAJOR and already divided by 6 (ucn_march_features_backward's layout 4: no copy, no division in
            # the mask pass), if the table gradient of this call runs on the row-block kernel
            chan.feat_ptr = chan.lm = None
            if C in (2, 4) and lib.ucn_march_features_backward_row_blocks(ctypes.byref(mlp.grid_field()), N, S) == 1:
                chan.feat_ptr, chan.levels, chan.level_dim = feat.data_ptr(), L, C
        return feat, coord, tmean

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_feat, _g_coord, _g_tmean):
        lib = _lib.load()
        N, S, std_scale, lpb = ctx.dims
        mlp = ctx.mlp
        emb = mlp.encoder.embeddings
        grad = torch.zeros_like(emb)                                   # dense, like grid.py:77
        # the feature gradient is consumed where autograd left it: [N*S][L*C] (layout 1) or, if a producer hands a
        # transposed view of [L*C][N*S] (_TallLinear grad_t; measured no faster than layout 1), layout 3 -- no
        # permuted level-major copy
        B = N * S
        lm_ptr = None
        if ctx.chan is not None:
            lm_ptr, ctx.chan.lm = ctx.chan.lm, None
        if lm_ptr is not None:
            # the consumer wrote [L][B][C] / 6 into this very buffer: anything else arriving here (a sum with another consumer's gradient,
            # a cast) would be read in the wrong layout -- fail loudly
            if g_feat.data_ptr() != lm_ptr or g_feat.dtype != torch.float32 or not g_feat.is_contiguous():
                raise RuntimeError("_FieldFeatures.backward: a level-major feature gradient was announced but another tensor arrived")
            g, layout = g_feat, 4
        else:
            g = g_feat if g_feat.dtype == torch.float32 else g_feat.float()
            if g.dim() == 2 and g.stride() == (1, B):
                layout = 3
            else:
                g, layout = g.contiguous(), 1
        ws = torch.empty(lib.ucn_march_features_backward_ws_floats(ctypes.byref(mlp.grid_field()), N, S), device=g.device)
        _lib.check(ctx.posts.ray_call(
            lib, 'ucn_march_features_backward', ctypes.byref(mlp.grid_field()), *ctx.cones, slice(None), std_scale, mlp.warp, N, S, 0,
            layout | (_lib.BWD_FIXED_POINT if ctx.fixed else 0), g.data_ptr(), grad.data_ptr(), ws.data_ptr(), _lib.stream()))
        return (grad,) + (None,) * 10


@torch.no_grad()
def scale_features(mlp, posts, rays, flip, spin, S, std_scale):
    """[N*S, L] float32: the scale features of a level's samples (MLP.scale_featurization, ref models.py:497-506) from
    ucn_march_scale_features, sample-major.  A constant of the graph, as in the reference: k is taken under no_grad, the
    Gaussians carry no gradient (coord.py:75), so nothing flows to the table or the positions through it."""
    lib = _lib.load()
    N, L = rays.N, mlp.encoder.num_levels
    out = torch.empty(N * S, L, device=rays.dev)
    _lib.check(posts.ray_call(
        lib, 'ucn_march_scale_features', ctypes.byref(mlp.grid_field()), rays, flip, spin, slice(None), std_scale, mlp.warp, N, S,
        mlp.level_scale().data_ptr(), 1, out.data_ptr(), _lib.stream()))
    return out


class GradientScaler(torch.autograd.Function):
    """ref train_utils.py:101-111: identity forward, grads scaled by clamp(ray_dist^2, 0, 1)."""

    @staticmethod
    def forward(ctx, colors, sigmas, ray_dist):
        ctx.save_for_backward(ray_dist)
        return colors, sigmas

    @staticmethod
    def backward(ctx, g_colors, g_sigmas):
        (ray_dist,) = ctx.saved_tensors
        k = torch.square(ray_dist).clamp(0, 1)
        return g_colors * k[..., None], g_sigmas * k, None


_ZEROS_RO = {}


def _zeros_ro(n, k, device):
    """A cached [n, k] fp32 block of zeros that kernels only READ (never hand it to anything that writes)."""
    key = (int(n), int(k), str(device))
    z = _ZEROS_RO.get(key)
    if z is None:
        if len(_ZEROS_RO) > 16:
            _ZEROS_RO.clear()
        z = _ZEROS_RO[key] = torch.zeros(n, k, device=device)
    return z


class _Composite(torch.autograd.Function):
    """render.py:155-174 + :203-216 as the rendering kernel `ucn_composite` (forward) and `ucn_composite_backward`:
    weights, rgb, depth, acc of N rays from density [N,S] and rgbs [N,S,3]; sample positions carry no gradient.
    `posts` (march_level.Fenceposts) picks the entry points (the siblings on the metric fenceposts of a warped Model.raydist_fn)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, density, rgbs, posts, dirs, bg, opaque):
        lib = _lib.load()
        N, S = density.shape
        density, rgbs = density.contiguous(), rgbs.contiguous()
        weights = torch.empty(N, S, device=density.device)
        main = torch.empty(N, 5, device=density.device)
        ctx.consts = (float(bg), int(bool(opaque)))
        _lib.check(posts.entry(lib, 'ucn_composite')(density.data_ptr(), rgbs.data_ptr(), *posts.compositing(), dirs.data_ptr(),
                                                     *ctx.consts, N, S, weights.data_ptr(), main.data_ptr(), None, _lib.stream()))
        ctx.save_for_backward(density, rgbs, dirs)
        ctx.posts = posts
        # outputs nobody differentiates (depth and acc always, rgb at a proposal level) arrive as None in backward instead of as
        # zero tensors autograd fills first: 12 launches per step less (tools/train_launch_sites.py)
        ctx.set_materialize_grads(False)
        return weights, main[:, :3].contiguous(), main[:, 3].contiguous(), main[:, 4].contiguous()

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_w, g_rgb, g_depth, g_acc):
        lib = _lib.load()
        density, rgbs, dirs = ctx.saved_tensors
        N, S = density.shape
        if g_w is None and g_rgb is None and g_depth is None and g_acc is None:
            return None, None, None, None, None, None
        if g_depth is None and g_acc is None:
            # the usual case: one cat against a cached block of zeros (read-only) instead of a fill and up to three strided copies
            g_main = _zeros_ro(N, 5, density.device) if g_rgb is None else torch.cat([g_rgb.float(), _zeros_ro(N, 2, density.device)], dim=1)
        else:
            g_main = torch.zeros(N, 5, device=density.device)
            if g_rgb is not None:
                g_main[:, :3] = g_rgb
            if g_depth is not None:
                g_main[:, 3] = g_depth
            if g_acc is not None:
                g_main[:, 4] = g_acc
        g_w = None if g_w is None else g_w.float().contiguous()
        g_density = torch.empty_like(density)
        g_rgbs = torch.empty_like(rgbs)
        posts = ctx.posts
        _lib.check(posts.entry(lib, 'ucn_composite_backward')(
            density.data_ptr(), rgbs.data_ptr(), *posts.compositing(backward=True), dirs.data_ptr(), *ctx.consts, N, S,
            _lib.ptr(g_w), g_main.data_ptr(), g_density.data_ptr(), g_rgbs.data_ptr(), _lib.stream()))
        return g_density, g_rgbs, None, None, None, None


class _CompositeRays(torch.autograd.Function):
    """`_Composite` with the per-ray colour gain [N, 3] (models.py:258-269, differentiable: its gradient reaches the exposure
    embedding) and / or per-ray background colours [N, 3] (models.py:253-256, no gradient), each None or a tensor:
    `ucn_composite_rays` and `ucn_composite_rays_backward`.  Fifth output: the colours as composited, gain * rgbs (what the reference's
    in-place scaling leaves in ray_results['rgb']); None with no gain."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, density, rgbs, gain, posts, dirs, ray_bg, bg, opaque):
        lib = _lib.load()
        N, S = density.shape
        density, rgbs = density.contiguous(), rgbs.contiguous()
        gain = None if gain is None else gain.contiguous()
        ray_bg = None if ray_bg is None else ray_bg.contiguous()
        weights = torch.empty(N, S, device=density.device)
        main = torch.empty(N, 5, device=density.device)
        scaled = torch.empty_like(rgbs) if gain is not None else None         # the backward reads the unscaled colours: a second buffer
        ctx.consts = (float(bg), int(bool(opaque)))
        _lib.check(posts.entry(lib, 'ucn_composite_rays')(
            density.data_ptr(), rgbs.data_ptr(), *posts.compositing(), dirs.data_ptr(), _lib.ptr(gain), _lib.ptr(ray_bg), *ctx.consts,
            N, S, weights.data_ptr(), main.data_ptr(), None, _lib.ptr(scaled), _lib.stream()))
        ctx.save_for_backward(density, rgbs, dirs, gain, ray_bg)
        ctx.posts = posts
        ctx.set_materialize_grads(False)
        return weights, main[:, :3].contiguous(), main[:, 3].contiguous(), main[:, 4].contiguous(), scaled

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_w, g_rgb, g_depth, g_acc, g_scaled):
        lib = _lib.load()
        density, rgbs, dirs, gain, ray_bg = ctx.saved_tensors
        N, S = density.shape
        if g_w is None and g_rgb is None and g_depth is None and g_acc is None and g_scaled is None:
            return (None,) * 8
        g_main = torch.zeros(N, 5, device=density.device)
        if g_rgb is not None:
            g_main[:, :3] = g_rgb
        if g_depth is not None:
            g_main[:, 3] = g_depth
        if g_acc is not None:
            g_main[:, 4] = g_acc
        g_w = None if g_w is None else g_w.float().contiguous()
        g_scaled = None if g_scaled is None else g_scaled.float().contiguous()
        g_density = torch.empty_like(density)
        g_rgbs = torch.empty_like(rgbs)
        g_gain = torch.empty(N, 3, device=density.device) if (gain is not None and ctx.needs_input_grad[2]) else None
        posts = ctx.posts
        _lib.check(posts.entry(lib, 'ucn_composite_rays_backward')(
            density.data_ptr(), rgbs.data_ptr(), *posts.compositing(backward=True), dirs.data_ptr(), _lib.ptr(gain), _lib.ptr(ray_bg),
            *ctx.consts, N, S, _lib.ptr(g_w), g_main.data_ptr(), _lib.ptr(g_scaled), g_density.data_ptr(), g_rgbs.data_ptr(),
            _lib.ptr(g_gain), _lib.stream()))
        return g_density, g_rgbs, g_gain, None, None, None, None, None


class _NegNormalize(torch.autograd.Function):
    """models.py:574 `-ref_utils.l2_normalize(grad_pred)`: n = -g / max(|g|, float32 eps) over [..., 3] as one HIP launch each way
    (`ucn_neg_normalize`); backward -(dn - n (n . dn)) / |g| above the clamp, -dn / eps below it."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, g):
        g = g.contiguous()
        out = torch.empty_like(g)
        _lib.check(_lib.load().ucn_neg_normalize(g.data_ptr(), g.numel() // 3, None, out.data_ptr(), _lib.stream()))
        ctx.save_for_backward(g)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dn):
        (g,) = ctx.saved_tensors
        dn = dn.float().contiguous()
        out = torch.empty_like(g)
        _lib.check(_lib.load().ucn_neg_normalize(g.data_ptr(), g.numel() // 3, dn.data_ptr(), out.data_ptr(), _lib.stream()))
        return out


class _RefColour(torch.autograd.Function):
    """models.py:657-674 with use_diffuse_color, in place of `rgb_activation`: the final colour from the colour logits [..., 3], the raw
    diffuse logits and the raw tint logits (or None: the factor 0.5) as one HIP launch each way (`ucn_ref_colour`, `ucn_ref_colour_backward`;
    csrc/ref_colour.hip).  float32 inside, whatever the autocast dtype of its inputs."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, logits, raw_diffuse, raw_tint, premultiplier, bias, padding):
        logits, raw_diffuse = logits.contiguous(), raw_diffuse.contiguous()
        raw_tint = None if raw_tint is None else raw_tint.contiguous()
        for name, t in (("logits", logits), ("raw_diffuse", raw_diffuse), ("raw_tint", raw_tint)):
            if t is not None:
                _lib.require_device(t, f"_RefColour {name}")
                if t.shape != logits.shape or t.shape[-1] != 3:
                    raise RuntimeError(f"_RefColour: {name} {tuple(t.shape)} against logits {tuple(logits.shape)}: expected equal [..., 3] shapes")
        out = torch.empty_like(logits)
        ctx.head = (float(premultiplier), float(bias), float(padding))
        _lib.check(_lib.load().ucn_ref_colour(logits.data_ptr(), raw_diffuse.data_ptr(), _lib.ptr(raw_tint), logits.numel() // 3, *ctx.head,
                                              out.data_ptr(), _lib.stream()))
        ctx.save_for_backward(logits, raw_diffuse, raw_tint)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        logits, raw_diffuse, raw_tint = ctx.saved_tensors
        g = g.float().contiguous()
        g_logits, g_diffuse = torch.empty_like(logits), torch.empty_like(raw_diffuse)
        g_tint = None if raw_tint is None else torch.empty_like(raw_tint)
        _lib.check(_lib.load().ucn_ref_colour_backward(logits.data_ptr(), raw_diffuse.data_ptr(), _lib.ptr(raw_tint), g.data_ptr(),
                                                       logits.numel() // 3, *ctx.head, g_logits.data_ptr(), g_diffuse.data_ptr(),
                                                       _lib.ptr(g_tint), _lib.stream()))
        return g_logits, g_diffuse, g_tint, None, None, None


class _HashDecay(torch.autograd.Function):
    """models.py:297-306 as one pass over the table forward and one backward (`ucn_hash_decay`); the per-level slices of
    the reference's formulation cost 16 full-table zero-fills and adds in autograd, the torch form of the weighted sum
    (pow, per-row sum, dot with a [rows] weight vector) 150 us per table and step."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, emb, offsets_np):
        lib = _lib.load()
        emb = emb.contiguous()
        out = torch.empty(1, device=emb.device)
        ws = torch.empty(1024, device=emb.device)
        off = np.ascontiguousarray(offsets_np, dtype=np.int32)
        _lib.check(lib.ucn_hash_decay(emb.data_ptr(), off.ctypes.data, len(off) - 1, emb.shape[1], None, out.data_ptr(), ws.data_ptr(),
                                      _lib.stream()))
        ctx.save_for_backward(emb)
        ctx.off = off
        return out[0]

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        lib = _lib.load()
        (emb,) = ctx.saved_tensors
        grad = torch.empty_like(emb)
        g = g.reshape(1).float().contiguous()
        _lib.check(lib.ucn_hash_decay(emb.data_ptr(), ctx.off.ctypes.data, len(ctx.off) - 1, emb.shape[1], g.data_ptr(), grad.data_ptr(),
                                      None, _lib.stream()))
        return grad, None


def hash_decay(mlp):
    """models.py:297-306: mean over levels and channels of the per-level mean of embeddings^2
    (torch_scatter.segment_coo(reduce='mean') over the sorted level index), restated as one weighted sum with
    w[row] = 1 / (rows_of_its_level * L * C)."""
    enc = mlp.encoder
    if not enc.embeddings.is_cuda:
        # host tensors (CPU debugging of a loss): the same weighted sum as plain torch ops
        off = torch.as_tensor(enc._offsets_np.astype('int64'))
        rows = (off[1:] - off[:-1]).double()
        w = torch.repeat_interleave(1.0 / (rows * rows.numel() * enc.embeddings.shape[1]), off[1:] - off[:-1])
        return (enc.embeddings.double() ** 2 * w[:, None]).sum().to(enc.embeddings.dtype)
    return _HashDecay.apply(enc.embeddings, enc._offsets_np)


def _ptr_array(tensors):
    """host array of device pointers (kept alive by the caller for the duration of the call)"""
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


def _tail_fusable(*tensors):
    """the fused tail kernels (csrc/heads_train.hip) take contiguous float32 device tensors; bf16 affine maps (what the
    colour-correction nn.Linear layers return under train.py:165's autocast) are upcast by the caller -- exact, and what the eager
    form's bf16 * fp32 type promotion does"""
    return all(t is None or (t.is_cuda and t.dtype in (torch.float32, torch.bfloat16, torch.float16)) for t in tensors)


class _AffineBlend(torch.autograd.Function):
    """models.py:339-363 for one level: rgb' = A rgb + t (+ (1 - acc_last) (A_sky sky + t_sky)) with per-ray maps [N, 3, 4]:
    one launch forward, one backward (`ucn_affine_blend`) where the broadcast-multiply form took ~12 + ~25 eager launches per level."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rgb, A, acc_last, sky, A_sky):
        lib = _lib.load()
        N = rgb.shape[0]
        rgb, A = rgb.contiguous(), A.contiguous()
        with_sky = sky is not None
        if with_sky:
            acc_last, sky, A_sky = acc_last.contiguous(), sky.contiguous(), A_sky.contiguous()
        out = torch.empty(N, 3, device=rgb.device)
        _lib.check(lib.ucn_affine_blend(None, rgb.data_ptr(), A.data_ptr(), _lib.ptr(acc_last) if with_sky else None,
                                        _lib.ptr(sky) if with_sky else None, _lib.ptr(A_sky) if with_sky else None, N, 0,
                                        out.data_ptr(), None, None, None, None, _lib.stream()))
        ctx.save_for_backward(rgb, A, *( (acc_last, sky, A_sky) if with_sky else () ))
        ctx.with_sky = with_sky
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        lib = _lib.load()
        saved = ctx.saved_tensors
        rgb, A = saved[0], saved[1]
        N = rgb.shape[0]
        g = g.float().contiguous()
        g_rgb, g_A = torch.empty_like(rgb), torch.empty_like(A)
        if ctx.with_sky:
            acc_last, sky, A_sky = saved[2:]
            g_acc, g_sky, g_As = torch.empty_like(acc_last), torch.empty_like(sky), torch.empty_like(A_sky)
            _lib.check(lib.ucn_affine_blend(g.data_ptr(), rgb.data_ptr(), A.data_ptr(), acc_last.data_ptr(), sky.data_ptr(),
                                            A_sky.data_ptr(), N, 0, g_rgb.data_ptr(), g_A.data_ptr(), g_acc.data_ptr(), g_sky.data_ptr(),
                                            g_As.data_ptr(), _lib.stream()))
            return g_rgb, g_A, g_acc, g_sky, g_As
        _lib.check(lib.ucn_affine_blend(g.data_ptr(), rgb.data_ptr(), A.data_ptr(), None, None, None, N, 0, g_rgb.data_ptr(),
                                        g_A.data_ptr(), None, None, None, _lib.stream()))
        return g_rgb, g_A, None, None, None


def brightness_forward(bc, idx, which="latent_code"):
    """extrinsic_optimizer.py:4-48 as models.py:341-349 calls it: the reference looks the latent code up per RAY and runs the
    4 -> 256 -> 256 -> 256 -> 12 MLP on 8192 rows that repeat at most `training_views` distinct codes.  A row's result depends
    only on its code, so the MLP runs on the code table (210 rows) and the rays gather their affine map: same values, same
    gradients (autograd's gather backward sums a code's rays), 40x fewer rows through six GEMMs forward + backward."""
    codes = getattr(bc, which)
    idx = idx.reshape(-1).long()
    mlp = bc.brightness_MLP
    if codes.is_cuda and codes.dtype == torch.float32 and mlp.output_linear.weight.dtype == torch.float32 and not dense_f32.library_route():
        # csrc/gemm_f32.hip, with or without autocast (r06: under autocast the reference runs these four 210-row layers in bf16 on the
        # library; fp32 products here are the higher precision, and the step holds no library GEMM)
        out_dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else None

        def run(x):
            with torch.autocast("cuda", enabled=False):
                for lin in mlp.pts_linears:
                    x = dense_f32.hip_linear(x, lin.weight, lin.bias, relu=True)
                y = dense_f32.hip_linear(x, mlp.output_linear.weight, mlp.output_linear.bias).view(-1, 3, 4)
            return y if out_dt is None else y.to(out_dt)          # the dtype the reference's nn.Linear returns under autocast
    else:
        def run(x):
            for lin in mlp.pts_linears:
                x = F.relu(lin(x))
            return mlp.output_linear(x).view(-1, 3, 4)
    if codes.shape[0] > 2 * idx.shape[0]:                           # more codes than rays: the per-ray form is the smaller one
        return run(codes[idx])
    return run(codes)[idx]
