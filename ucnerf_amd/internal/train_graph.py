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
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib
from . import dense_f32
from . import march_level as ml

EPS = float(torch.finfo(torch.float32).eps)


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
            d16 = _lib.UcnField()
            ctypes.memmove(ctypes.byref(d16), ctypes.byref(desc), ctypes.sizeof(_lib.UcnField))
            d16.embeddings = emb16.data_ptr()
            desc, layout = d16, layout | _lib.TABLE_F16
        feat = torch.empty(N * S, L * C, device=embeddings.device)
        coord = torch.empty(N, S, 3, device=embeddings.device)
        tmean = torch.empty(N, S, device=embeddings.device)
        _lib.check(posts.entry(lib, 'ucn_march_features')(
            ctypes.byref(desc), *posts.geometry(rays, flip, spin), float(std_scale), N, S, int(lpb), layout,
            feat.data_ptr(), coord.data_ptr(), tmean.data_ptr(), _lib.stream()))
        ctx.mlp, ctx.posts, ctx.cones, ctx.dims = mlp, posts, (rays, flip, spin), (N, S, float(std_scale), int(lpb))
        # the autocast step (half tables): the table gradient's row blocks accumulate in guaranteed-range fixed point (order-
        # independent, one LDS add per channel pair); the fp32 step keeps exact fp32 adds (include/ucnerf_march.h UCN_BWD_FIXED_POINT)
        ctx.fixed = bool(half_table) and bool(getattr(mlp, 'bwd_fixed_point', True))
        ctx.mark_non_differentiable(coord, tmean)
        if chan is not None:
            # r06 (VERDICT r05 item 2 c): tell the node that consumes `feat` -- and nothing else does, see field_level -- that its feature
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
        _lib.check(ctx.posts.entry(lib, 'ucn_march_features_backward')(
            ctypes.byref(mlp.grid_field()), *ctx.posts.geometry(*ctx.cones), std_scale, N, S, 0, layout | (_lib.BWD_FIXED_POINT if ctx.fixed else 0),
            g.data_ptr(), grad.data_ptr(), ws.data_ptr(), _lib.stream()))
        return (grad,) + (None,) * 10


@torch.no_grad()
def scale_features(mlp, posts, rays, flip, spin, S, std_scale):
    """[N*S, L] float32: the scale features of a level's samples (MLP.scale_featurization, ref models.py:497-506) from
    ucn_march_scale_features, sample-major.  A constant of the graph, as in the reference: k is taken under no_grad, the
    Gaussians carry no gradient (coord.py:75), so nothing flows to the table or the positions through it."""
    lib = _lib.load()
    N, L = rays.N, mlp.encoder.num_levels
    out = torch.empty(N * S, L, device=rays.dev)
    _lib.check(posts.entry(lib, 'ucn_march_scale_features')(
        ctypes.byref(mlp.grid_field()), *posts.geometry(rays, flip, spin), float(std_scale), N, S, mlp.level_scale().data_ptr(), 1,
        out.data_ptr(), _lib.stream()))
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


class _TallLinear(torch.autograd.Function):
    """x @ weight.T (+ bias | + acc) for a tall activation matrix [M ~ 1e6, K] and a small weight [N <= 256, K].

    * The library's weight-gradient GEMM dY^T X (N x K output, reduction over the M samples) gets a single
      64x64 macro-tile grid -- 36 workgroups on a 256-CU part, 1.75 ms per call -- because nothing splits the
      reduction.  Here the reduction is cut into chunks that run as one batched GEMM and are summed afterwards
      (the same addends in a different order; fp32 accumulation inside each chunk and across chunks).
    * The bias gradient (column sums of dY) is a batched ones-row GEMM over the same chunks instead of an fp32
      copy of dY plus a reduction kernel.
    * `extra` is either a bias [N] or an accumulator [M, N] (the partial sum of another GEMM of the same layer:
      the concatenations of the reference's colour MLP are never materialised, see field_heads)."""
    CHUNK = 8192

    @staticmethod
    def forward(ctx, x, weight, extra, grad_t=False):
        ctx.grad_t = grad_t
        dt = torch.get_autocast_dtype("cuda")                      # bf16 under the reference's accelerator.autocast()
        xb, wb = x.to(dt), weight.to(dt)
        ctx.save_for_backward(xb, wb)
        ctx.dtypes = (x.dtype, weight.dtype, None if extra is None else extra.dtype)
        ctx.extra_is_acc = extra is not None and extra.dim() == 2
        with torch.autocast("cuda", enabled=False):
            if ctx.extra_is_acc:
                return torch.addmm(extra.to(dt), xb.reshape(-1, xb.shape[-1]), wb.t())
            return F.linear(xb, wb, None if extra is None else extra.to(dt))

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        x_dt, w_dt, e_dt = ctx.dtypes
        with torch.autocast("cuda", enabled=False):
            gy2 = gy.reshape(-1, gy.shape[-1]).to(x.dtype)
            x2 = x.reshape(-1, x.shape[-1])
            if not ctx.needs_input_grad[0]:
                gx = None
            elif ctx.grad_t:                                     # [K, M] written by the GEMM, handed on as its transpose
                gx = (weight.t() @ gy2.t()).to(x_dt).t()
            else:
                gx = (gy2 @ weight).reshape(x.shape).to(x_dt)
            m, c = x2.shape[0], _TallLinear.CHUNK
            chunked = m >= 4 * c and m % c == 0
            if chunked:
                gyc = gy2.reshape(m // c, c, -1)
            if gy2.shape[1] == 1:
                # a single output row (PropMLP's density head): every library route for it (bmm with one row, mv)
                # takes an 11 ms HOST-side path in bf16 on this stack, which made the whole step CPU-bound
                gw = (gy2 * x2).float().sum(0, keepdim=True)
            elif chunked:
                gw = torch.bmm(gyc.transpose(1, 2), x2.reshape(m // c, c, -1)).float().sum(0)
            else:
                gw = (gy2.t() @ x2).float()
            if e_dt is None:
                ge = None
            elif ctx.extra_is_acc:
                ge = gy2.to(e_dt)
            elif chunked:
                ge = torch.bmm(gy2.new_ones(m // c, 1, c), gyc).float().sum(dim=(0, 1)).to(e_dt)
            else:
                ge = gy2.float().sum(0).to(e_dt)
        return gx, gw.to(w_dt), ge, None


def tall_linear(lin, x, grad_t=False, relu=False):
    """nn.Linear `lin` (+ ReLU) applied through _TallLinear (autocast: operands in bf16 like F.linear under autocast).
    grad_t: the input gradient comes back as the transpose of a contiguous [K, M] matrix (for _FieldFeatures).
    relu: on the fp32 route the ReLU is the GEMM's epilogue (and its output keeps the recorded maximum the next product scales by:
    the waymo.gin proposal level -- 1.9 M rows x 64 -- paid an elementwise pass and an amax pass for a separate F.relu)."""
    if torch.is_autocast_enabled():
        y = _TallLinear.apply(x, lin.weight, lin.bias, grad_t)
        return F.relu(y) if relu else y
    if dense_f32.usable(x, lin.weight):            # the fp32 step (train_waymo.sh:3): hand-written fp32 MFMA GEMMs (csrc/gemm_f32.hip)
        return dense_f32.hip_linear(x, lin.weight, lin.bias, relu=relu)
    y = F.linear(x, lin.weight, lin.bias)
    return F.relu(y) if relu else y


def tall_matmul(x, weight, acc=None):
    """x @ weight.T (+ acc [M, N]) through _TallLinear under autocast."""
    if torch.is_autocast_enabled():
        return _TallLinear.apply(x, weight, acc)
    y = dense_f32.hip_linear(x, weight) if dense_f32.usable(x, weight) else x @ weight.t()
    return y if acc is None else y + acc


def view_encoding(d, deg):
    """coord.py:214-225 pos_enc(min_deg=0, max_deg=deg, append_identity=True)."""
    scales = 2 ** torch.arange(0, deg, device=d.device)
    scaled = (d[..., None, :] * scales[:, None]).reshape(d.shape[:-1] + (-1,))
    return torch.cat([d, torch.sin(torch.cat([scaled, scaled + 0.5 * torch.pi], dim=-1))], dim=-1)


def _wgrad(gy, x):
    """gy^T @ x for tall operands [M, a], [M, b] -> [a, b] float32, the reduction over M cut into batched chunks
    (see _TallLinear)."""
    m, c = x.shape[0], _TallLinear.CHUNK
    if m >= 4 * c and m % c == 0:
        return torch.bmm(gy.reshape(m // c, c, -1).transpose(1, 2), x.reshape(m // c, c, -1)).float().sum(0)
    return (gy.t() @ x).float()


def _colsum(g):
    """Column sums of a tall [M, a] matrix as float32 [a]: a batched ones-row GEMM over 8192-row chunks (an fp32 copy +
    reduce_kernel over [1M, 3] costs 0.35 ms; this is 0.06 ms)."""
    m, c = g.shape[0], _TallLinear.CHUNK
    if m >= 4 * c and m % c == 0:
        return torch.bmm(g.new_ones(m // c, 1, c), g.reshape(m // c, c, -1)).float().sum(dim=(0, 1))
    return g.float().sum(0)


class _ColourMLP(torch.autograd.Function):
    """The two hidden layers of the colour MLP in the reference's topology (models.py:615-640: net_depth_viewdirs = 2,
    skip connection after layer 0) as ONE autograd node:

        h1 = relu(x W0x^T + [enc W0e^T + b0]_ray),   h2 = relu(h1 W1h^T + x W1x^T + [enc W1e^T + b1]_ray)

    (second output: column 0 of x, the raw density, so that its gradient joins d x inside the node instead of through
    a zero-filled [N*S, 256] tensor and an add)

    with W0 = [W0x | W0e], W1 = [W1h | W1x | W1e] the reference's weights over its concatenated inputs
    [bottleneck, dir_enc] and [h1, bottleneck, dir_enc].  The GEMMs are library GEMMs (bf16 under autocast); the
    broadcast-add + ReLU and its backward (mask + per-ray reduction) are the HIP kernels ucn_bias_relu /
    ucn_relu_backward_reduce, in place; the two contributions to d x accumulate inside the second GEMM (addmm), so
    no activation-sized tensor is added, concatenated or re-read by an elementwise kernel."""

    @staticmethod
    def forward(ctx, x, enc, W0, b0, W1, b1, N, S):
        h2, xb, saved, meta = _colour_mlp_forward(x, enc, W0, b0, W1, b1, N, S)
        ctx.save_for_backward(*saved)
        ctx.meta = meta
        return h2, xb[:, 0].clone()                       # raw density = column 0 of the bottleneck (models.py:508)

    @staticmethod
    def backward(ctx, g_h2, g_raw):
        gx, gW0, gb0, gW1, gb1 = _colour_mlp_backward(ctx.saved_tensors, ctx.meta, g_h2, g_raw)
        return gx, None, gW0, gb0, gW1, gb1, None, None


def _colour_mlp_forward(x, enc, W0, b0, W1, b1, N, S, film=None):
    """_ColourMLP's forward: (h2, the bottleneck operand as the GEMMs read it, tensors to save, meta).  film = (a, b), float32 [N, NB]:
    the GEMMs read x * a[ray] + b[ray] (ucn_ray_film, the GLO modulation) instead of x."""
    lib = _lib.load()
    dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else torch.float32
    code = {torch.float32: 0, torch.bfloat16: 2}[dt]
    NB, NW = x.shape[1], W0.shape[0]
    hip = code == 0 and x.is_cuda and not dense_f32.library_route()      # fp32: csrc/gemm_f32.hip instead of the library GEMMs
    with torch.autocast("cuda", enabled=False):
        xb, eb = x.to(dt).contiguous(), enc.to(dt)
        if film is not None:
            y = torch.empty_like(xb)
            _lib.check(lib.ucn_ray_film(xb.data_ptr(), film[0].data_ptr(), film[1].data_ptr(), y.data_ptr(), N, S, NB, code,
                                        _lib.stream()))
            xb = y
        W0x, W0e = W0[:, :NB].to(dt), W0[:, NB:].to(dt)
        W1h, W1x, W1e = W1[:, :NW].to(dt), W1[:, NW:NW + NB].to(dt), W1[:, NW + NB:].to(dt)
        if hip:
            R, G = dense_f32._rows, dense_f32.gemm
            xb, eb = R(xb), R(eb)
            W0x, W1h, W1x = R(W0x), R(W1h), R(W1x)
            pr0 = G(eb, R(W0e), b0.contiguous())                                     # [N, NW] per ray
            h1 = G(xb, W0x)
            _lib.check(lib.ucn_bias_relu(h1.data_ptr(), pr0.data_ptr(), N, S, NW, code, _lib.stream()))
            dense_f32.forget(h1)                                                     # written through its raw pointer
            pr1 = G(eb, R(W1e), b1.contiguous())
            h2 = G(h1, W1h)
            G(xb, W1x, flags=dense_f32.ACCUMULATE, out=h2)                           # accumulate in place: no copy
            _lib.check(lib.ucn_bias_relu(h2.data_ptr(), pr1.data_ptr(), N, S, NW, code, _lib.stream()))
            dense_f32.forget(h2)
        else:
            pr0 = torch.addmm(b0.to(dt), eb, W0e.t()).contiguous()                   # [N, NW] per ray
            h1 = xb @ W0x.t()
            _lib.check(lib.ucn_bias_relu(h1.data_ptr(), pr0.data_ptr(), N, S, NW, code, _lib.stream()))
            pr1 = torch.addmm(b1.to(dt), eb, W1e.t()).contiguous()
            h2 = (h1 @ W1h.t()).addmm_(xb, W1x.t())                                  # accumulate in place: no copy
            _lib.check(lib.ucn_bias_relu(h2.data_ptr(), pr1.data_ptr(), N, S, NW, code, _lib.stream()))
    return h2, xb, (xb, eb, h1, h2, W0x, W1h, W1x), (N, S, NB, NW, code, x.dtype, W0.dtype, b0.dtype, hip, enc.shape[1])


def _colour_mlp_backward(saved, meta, g_h2, g_raw):
    """_ColourMLP's backward: (d bottleneck operand, gW0, gb0, gW1, gb1); g_raw (or None) joins column 0 of the first."""
    lib = _lib.load()
    xb, eb, h1, h2, W0x, W1h, W1x = saved
    N, S, NB, NW, code, x_dt, w_dt, b_dt, hip, E = meta
    dt = xb.dtype
    with torch.autocast("cuda", enabled=False):
        g = g_h2.to(dt).contiguous()
        d1 = torch.empty_like(g)
        r1 = torch.empty(N, NW, device=g.device, dtype=dt)
        _lib.check(lib.ucn_relu_backward_reduce(g.data_ptr(), h2.data_ptr(), d1.data_ptr(), r1.data_ptr(), N, S, NW, code,
                                                _lib.stream()))
        if hip:
            # the same node on the hand-written fp32 kernels: dgrad = the forward kernel on the transposed weight; every
            # weight gradient one pass of ucn_wgrad_f32 (fixed-order partial sums); both paths into x accumulate in one output
            R, G, WG = dense_f32._rows, dense_f32.gemm, dense_f32.wgrad
            d0 = G(d1, R(W1h.t()))                                                    # d h1, masked in place below
            r0 = torch.empty(N, NW, device=g.device, dtype=dt)
            _lib.check(lib.ucn_relu_backward_reduce(d0.data_ptr(), h1.data_ptr(), d0.data_ptr(), r0.data_ptr(), N, S, NW, code,
                                                    _lib.stream()))
            dense_f32.forget(d0)                                                      # masked in place through its raw pointer
            gW0 = torch.cat([WG(d0, xb)[0][:, :NB], WG(r0, eb)[0][:, :E]], dim=1)
            gW1 = torch.cat([WG(d1, h1)[0], WG(d1, xb)[0][:, :NB], WG(r1, eb)[0][:, :E]], dim=1)
            gb0, gb1 = r0.sum(0), r1.sum(0)
            gx = G(d1, R(W1x[:, :NB].t()))
            G(d0, R(W0x[:, :NB].t()), flags=dense_f32.ACCUMULATE, out=gx)
            if g_raw is not None:
                gx[:, 0] += g_raw.reshape(-1)
            return gx[:, :NB].to(x_dt), gW0.to(w_dt), gb0.to(b_dt), gW1.to(w_dt), gb1.to(b_dt)
        d_h1 = d1 @ W1h
        d0 = d_h1                                                                     # masked in place
        r0 = torch.empty(N, NW, device=g.device, dtype=dt)
        _lib.check(lib.ucn_relu_backward_reduce(d_h1.data_ptr(), h1.data_ptr(), d0.data_ptr(), r0.data_ptr(), N, S, NW, code,
                                                _lib.stream()))
        gW0 = torch.cat([_wgrad(d0, xb), (r0.t() @ eb).float()], dim=1)
        gW1 = torch.cat([_wgrad(d1, h1), _wgrad(d1, xb), (r1.t() @ eb).float()], dim=1)
        gb0, gb1 = r0.float().sum(0), r1.float().sum(0)
        gx = (d1 @ W1x).addmm_(d0, W0x)                                               # both paths into x in one output
        if g_raw is not None:
            gx[:, 0] += g_raw.reshape(-1).to(dt)                                      # the density head's column
    return gx.to(x_dt), gW0.to(w_dt), gb0.to(b_dt), gW1.to(w_dt), gb1.to(b_dt)


class _ColourMLPGlo(torch.autograd.Function):
    """_ColourMLP with the GLO appearance modulation of the bottleneck (models.py:606-614) in front of it:

        x' = x * a[ray] + b[ray],   a = exp(scale), b = shift  (float32 [N, NB], from the per-ray GLO MLP)

    x' replaces x in both colour layers (skip input included); the raw density stays column 0 of the UNmodulated x
    (models.py:508).  Forward and backward of the modulation are the HIP kernels ucn_ray_film / ucn_ray_film_backward; the
    backward hands d a = sum_s d x' * x and d b = sum_s d x' (float32 [N, NB]) to ordinary autograd (exp, the GLO MLP,
    glo_vecs).  The per-ray scale is why this is not the composed / fused route: those fold the bottleneck layer into the
    colour layers' weights, which a per-ray diagonal between them breaks."""

    @staticmethod
    def forward(ctx, x, a, b, enc, W0, b0, W1, b1, N, S):
        a, b = a.float().contiguous(), b.float().contiguous()
        h2, _, saved, meta = _colour_mlp_forward(x, enc, W0, b0, W1, b1, N, S, film=(a, b))
        xb = x.to(saved[0].dtype).contiguous()                                   # the unmodulated bottleneck, as the film read it
        ctx.save_for_backward(xb, a, *saved)
        ctx.meta = meta
        return h2, xb[:, 0].clone()

    @staticmethod
    def backward(ctx, g_h2, g_raw):
        lib = _lib.load()
        xb, a, *saved = ctx.saved_tensors
        N, S, NB, NW, code, x_dt, w_dt, b_dt, hip, E = ctx.meta
        gy, gW0, gb0, gW1, gb1 = _colour_mlp_backward(saved, ctx.meta, g_h2, None)
        with torch.autocast("cuda", enabled=False):
            gy = gy.to(xb.dtype).contiguous()
            gx = torch.empty_like(xb)
            ga = torch.empty(N, NB, device=xb.device)
            gb = torch.empty(N, NB, device=xb.device)
            _lib.check(lib.ucn_ray_film_backward(gy.data_ptr(), xb.data_ptr(), a.data_ptr(), gx.data_ptr(), ga.data_ptr(), gb.data_ptr(),
                                                 N, S, NB, code, _lib.stream()))
            if g_raw is not None:
                gx[:, 0] += g_raw.reshape(-1).to(gx.dtype)                         # the density head's column
        return gx.to(x_dt), ga, gb, None, gW0, gb0, gW1, gb1, None, None


def _colour_forward(h0, A0, pr0, W1h, A1, pr1, Wr, br, S):
    """h1, h2, colour logits of the composed colour MLP (see _ColourMLPComposed) from the 64-wide hidden layer h0 [M, 64]; operands as
    dense_f32._rows returns them."""
    G = dense_f32.gemm
    # r05: the per-ray terms are the GEMMs' row-group bias, the ReLUs their epilogue, and the rgb row (models.py:663) sits inside the
    # node so that its d X GEMM can carry h2's ReLU derivative as a mask epilogue (r04: ucn_bias_relu / ucn_relu_backward_reduce passes)
    pr0, pr1 = pr0.contiguous(), pr1.contiguous()
    # layer 1's two products as ONE over the concatenated input [h1 | h0] (K = 256 + 64): h1 is written straight into its column block
    # of the buffer; a second, accumulating pass re-read the whole [M, 256] output (0.65 + 0.69 ms -> 0.82 + a 0.1 ms copy)
    M = h0.shape[0]
    cat = torch.empty(M, W1h.shape[1] + h0.shape[1], device=h0.device, dtype=torch.float32)
    cat[:, W1h.shape[1]:] = h0      # (before the kernel writes h1 into its view: an in-place torch op bumps the shared version
    h1 = G(h0, A0, None, dense_f32.RELU, out=cat[:, :W1h.shape[1]], rowbias=pr0, rgroup=S)  # counter and h1's records would go stale)
    dense_f32.tag_amax_of_parts(cat, h1, h0)
    h2 = G(cat, torch.cat([W1h, A1], dim=1), None, dense_f32.RELU, out=dense_f32.rows_buffer(M, W1h.shape[0], h0.device), rowbias=pr1, rgroup=S)
    del cat
    rgbl = G(h2, Wr, br.float().contiguous())
    return h1, h2, rgbl


def _colour_backward(g_rgbl, h0, h1, h2, A0, A1, W1h, Wr, N, S):
    """gradients of _colour_forward: (d h0 [M, 64] -- a buffer the caller may keep accumulating into --, d A0, d pr0, d W1h, d A1, d pr1,
    d Wr, d br)."""
    R, G, WG = dense_f32._rows, dense_f32.gemm, dense_f32.wgrad
    NW, n_rgb = W1h.shape[0], Wr.shape[0]
    g4 = R(g_rgbl.float())                                                     # [M, 3 -> 4]
    gWr4, gbr4 = WG(g4, h2, True)
    E = lambda: dense_f32.rows_buffer(g4.shape[0], NW, g4.device)
    d1 = G(g4, R(Wr.t()), mask=h2, out=E())                                    # d (layer 1 pre-activation)
    r1 = d1.unflatten(0, (N, S)).sum(dim=1)                                    # (strided views: no copy)
    d0 = G(d1, R(W1h.t()), mask=h1, out=E())
    r0 = d0.unflatten(0, (N, S)).sum(dim=1)
    gA0, gA1, gW1h = WG(d0, h0)[0], WG(d1, h0)[0], WG(d1, h1)[0]
    gh0 = G(d0, R(A0.t()))
    G(d1, R(A1.t()), flags=dense_f32.ACCUMULATE, out=gh0)
    return gh0, gA0, r0, gW1h, gA1, r1, gWr4[:n_rgb], gbr4[:n_rgb]


class _ColourMLPComposed(torch.autograd.Function):
    """fp32 route (r04): the colour MLP's two hidden layers with the activation-free bottleneck COMPOSED into them, on csrc/gemm_f32.hip.

    The bottleneck x = h0 Wd1^T + bd1 (models.py:508) has no activation, so x W0x^T = h0 (W0x Wd1)^T + W0x bd1: with
    A0 = W0x Wd1, A1 = W1x Wd1 ([256, 64], formed OUTSIDE this node with differentiable ops so that autograd carries
    d A_i back to W_ix and Wd1) the 256-wide x is never materialised:

        h1 = relu(h0 A0^T + pr0_ray),      h2 = relu(h1 W1h^T + h0 A1^T + pr1_ray)

    pr_i [N, 256] = the per-ray terms (direction block, layer bias, W_ix bd1), also formed outside.  Against the uncomposed node:
    two forward GEMMs of K = 256 become K = 64, the bottleneck GEMM disappears, the backward's two 256 x 256 dgrads into x and
    the 256 -> 64 dgrad behind them become two 256 -> 64 dgrads, two 256 x 256 weight gradients become 256 x 64."""

    @staticmethod
    def forward(ctx, h0, A0, pr0, W1h, A1, pr1, Wr, br, N, S):
        R = dense_f32._rows
        h0, A0, A1, W1h, Wr = R(h0), R(A0), R(A1), R(W1h), R(Wr)
        h1, h2, rgbl = _colour_forward(h0, A0, pr0, W1h, A1, pr1, Wr, br, S)
        ctx.save_for_backward(h0, h1, h2, A0, A1, W1h, Wr)
        dense_f32.stash_amax(ctx, (h0, h1, h2))
        ctx.meta = (N, S)
        return rgbl

    @staticmethod
    def backward(ctx, g_rgbl):
        h0, h1, h2, A0, A1, W1h, Wr = ctx.saved_tensors
        dense_f32.restore_amax(ctx, (h0, h1, h2))
        N, S = ctx.meta
        return _colour_backward(g_rgbl, h0, h1, h2, A0, A1, W1h, Wr, N, S) + (None, None)


class _FieldMLPComposed(torch.autograd.Function):
    """fp32 route (r06): the NeRF field's whole dense part as ONE node -- density layer 0 (+ ReLU), the density row of the bottleneck
    (feature 0 of density layer 1: models.py:508-510), the composed colour MLP of _ColourMLPComposed -- so that the 64-wide hidden layer's
    gradient is formed in one buffer: the colour branch's two products accumulate into it, the density row's rank-1 term is a third
    accumulating product whose epilogue applies the layer's ReLU derivative (the mask is linear: masking the sum = masking the parts).
    As three nodes autograd added the two branches' [M, 64] gradients, ran threshold_backward over the sum and copied it once more
    (0.36 ms of elementwise passes per step at M = 2^20).  Returns (raw density [M, 1], colour logits [M, 3])."""

    @staticmethod
    def forward(ctx, feat, Wd0, bd0, wrow, brow, A0, pr0, W1h, A1, pr1, Wr, br, N, S):
        R, G = dense_f32._rows, dense_f32.gemm
        feat, Wd0, wrow, A0, A1, W1h, Wr = R(feat), R(Wd0), R(wrow), R(A0), R(A1), R(W1h), R(Wr)
        h0 = G(feat, Wd0, bd0.float().contiguous(), dense_f32.RELU)                # [M, 64]
        raw = G(h0, wrow, brow.float().contiguous())                              # [M, 1]
        h1, h2, rgbl = _colour_forward(h0, A0, pr0, W1h, A1, pr1, Wr, br, S)
        ctx.save_for_backward(feat, h0, h1, h2, Wd0, wrow, A0, A1, W1h, Wr)
        dense_f32.stash_amax(ctx, (feat, h0, h1, h2))
        ctx.meta = (N, S)
        return raw, rgbl

    @staticmethod
    def backward(ctx, g_raw, g_rgbl):
        feat, h0, h1, h2, Wd0, wrow, A0, A1, W1h, Wr = ctx.saved_tensors
        dense_f32.restore_amax(ctx, (feat, h0, h1, h2))
        N, S = ctx.meta
        R, G, WG = dense_f32._rows, dense_f32.gemm, dense_f32.wgrad
        gh0, gA0, r0, gW1h, gA1, r1, gWr, gbr = _colour_backward(g_rgbl, h0, h1, h2, A0, A1, W1h, Wr, N, S)
        g4 = torch.zeros(h0.shape[0], 4, device=h0.device)
        g4[:, :1] = g_raw
        gwrow4, gbrow4 = WG(g4, h0, True)                                          # [4, 64], [4]
        w4 = torch.zeros(wrow.shape[1], 4, device=h0.device)
        w4[:, :1] = wrow[:1].t()                                                   # [64, 4]: the row as the product's weight
        dp0 = G(g4, w4, flags=dense_f32.ACCUMULATE, out=gh0, mask=h0)              # d (layer 0 pre-activation): the sum, masked
        gWd0, gbd0 = WG(dp0, feat, True)                                           # [64, F]
        gfeat = G(dp0, R(Wd0.t()))                                                 # [M, F]
        return (gfeat, gWd0, gbd0, gwrow4[:1], gbrow4[:1], gA0, r0, gW1h, gA1, r1, gWr, gbr, None, None)


# ------------------------------------------------------------------ fused bf16 forward of the NeRF field's dense layers
_FRAG_CACHE = {}


def _perm(r, g):
    """Feature (within a 32-wide tile) held by accumulator register r of wave half g (csrc/mfma_chain.h acc_row)."""
    return (r & 3) + 8 * (r >> 2) + 4 * g


def _fragment_index(rows, cols, natural):
    """(row, col) of every element of a [rows, cols] weight's MFMA A-fragments in consumption order
    [out tile pair][in tile][k-step][tile of the pair][lane][8] (a single output tile: [in tile][k-step][lane][8]):
    lane (row = lane & 31, g = lane >> 5) element e is W[32 ot + row][32 it + k], k = 16 s + 8 g + e for the first
    layer (features arrive in natural order) and perm(8 s + e, g) for the others (the producing layer's accumulator
    order).  Positions beyond the matrix (tile padding) come back as row = -1."""
    nto, nti = (rows + 31) // 32, (cols + 31) // 32
    p = 1 if nto == 1 else 2                                  # output tiles in pairs, the pair innermost (csrc/field_train.hip)
    assert nto % p == 0
    otp, it, s_, o2, lane, e = torch.meshgrid(torch.arange(nto // p), torch.arange(nti), torch.arange(2), torch.arange(p),
                                              torch.arange(64), torch.arange(8), indexing="ij")
    row, g = 32 * (p * otp + o2) + (lane & 31), lane >> 5
    col = 32 * it + (16 * s_ + 8 * g + e if natural else _perm(8 * s_ + e, g))
    valid = (row < rows) & (col < cols)
    return torch.where(valid, row, torch.full_like(row, -1)).reshape(-1), col.reshape(-1)


def _pack_fragments(weights, device, total=0):
    """bf16 fragment stream of [(W, natural_k_order), ...]: ONE gather from the concatenated matrices (+ a zero slot
    for the tile padding and the stream's tail); the gather index depends only on the shapes and is cached."""
    key = ("pack", tuple((tuple(W.shape), tuple(W.stride()), nat) for W, nat in weights), total, str(device))
    idx = _FRAG_CACHE.get(key)
    if idx is None:
        parts, off = [], 0
        for W, nat in weights:
            r, c = _fragment_index(W.shape[0], W.shape[1], nat)
            parts.append(torch.where(r >= 0, off + r * W.shape[1] + c, torch.full_like(r, -1)))
            off += W.numel()
        flat = torch.cat(parts)
        if total * 512 > flat.numel():
            flat = torch.cat([flat, flat.new_full((total * 512 - flat.numel(),), -1)])
        idx = torch.where(flat >= 0, flat, torch.full_like(flat, off)).to(device)      # `off` = the zero slot
        _FRAG_CACHE[key] = idx
    src = torch.cat([W.reshape(-1) for W, _ in weights] + [weights[0][0].new_zeros(1)])
    return src[idx]


def _acc_order(width, device):
    """Column permutation that puts a [.., width] vector into accumulator order [tile][wave half][16]."""
    key = ("acc", width, str(device))
    hit = _FRAG_CACHE.get(key)
    if hit is None:
        t, g, r = torch.meshgrid(torch.arange((width + 31) // 32), torch.arange(2), torch.arange(16), indexing="ij")
        hit = (32 * t + _perm(r, g)).reshape(-1).to(device)
        _FRAG_CACHE[key] = hit
    return hit


def _acc_vec(v, width, device):
    pad = torch.zeros(v.shape[:-1] + (32 * ((width + 31) // 32),), device=device, dtype=torch.float32)
    pad[..., :v.shape[-1]] = v
    return pad[..., _acc_order(width, device)].contiguous()


# Column layout of the one activation buffer ucn_train_fwd writes per sample (bf16 [M, ACT_LD]): adjacent blocks are the
# concatenated inputs of the reference's layers, so each layer's whole weight gradient -- per-sample blocks, the per-ray
# direction block AND the bias (the constant-1 column of `aux`) -- is ONE split-K GEMM on a strided view:
#   [ h2 | h1 | x | aux = (dir_enc(27), 1, 0, 0, 0, 0) | h0 | bf16 copy of the features (<= 64) | pad ]     rows of 2 KiB:
#   a row that does not start on a 128-byte line (864 columns) costs the forward kernel 15 %
#     d1^T [h1 | x | aux] = [gW1h | gW1x | gW1e | gb1]  (models.py:620-640: lin_second_stage_1 over cat([h1, x, enc]))
#     d0^T [x | aux]      = [gW0x | gW0e | gb0],      gx^T [aux | h0] -> gb_d1 (column 27), gW_d1 (columns 32..95)
_ACT_H2, _ACT_H1, _ACT_X, _ACT_AUX, _ACT_H0, _ACT_FB, ACT_LD = 0, 256, 512, 768, 800, 864, 1024


def _weave(parts, producer, consumer):
    """Fragment lists of consecutive layers -> the same lists with parts[producer] (4 output-tile PAIRS) and
    parts[consumer] (whose 8 input tiles are those output tiles) cut into quarters and alternated: pair 0 of the
    producer, the consumer's fragments for input tiles 0-1, pair 1, input tiles 2-3, ..."""
    a, b = parts[producer], parts[consumer]
    assert a.numel() % 4 == 0 and b.numel() % 4 == 0 and consumer == producer + 1
    qa, qb = a.reshape(4, -1), b.reshape(4, -1)
    woven = torch.cat([torch.cat([qa[p], qb[p]]) for p in range(4)])
    return parts[:producer] + [woven] + parts[consumer + 1:]


def _head_gather_index(F_in, NB, NW, E, total, device, dir_in_stream=False):
    """ONE gather index over the flat bf16 copy of (Wd0, Wd1, W0, W1, Wr, bd0, bd1, b0', b1', br, W0x Wd1, W1x Wd1, 0) -- the
    colour layers composed with the activation-free bottleneck and W bd1 folded into their biases -- that yields, in this
    order: the forward fragment stream, the dgrad (transposed) fragment stream, the direction blocks of W0 / W1 with
    rows in accumulator order [2 NW, E], their biases [2 NW], and bd0 / bd1 / br in accumulator order (64 + NB + 32).
    A logical matrix is a list of column blocks (base, row_stride, col_stride, ncols) of the flat source."""
    key = ("heads", F_in, NB, NW, E, total, str(device), dir_in_stream)
    hit = _FRAG_CACHE.get(key)
    if hit is not None:
        return hit
    k0, k1 = NB + E, NW + NB + E
    oWd0 = 0
    oWd1 = oWd0 + 64 * F_in
    oW0 = oWd1 + NB * 64
    oW1 = oW0 + NW * k0
    oWr = oW1 + NW * k1
    obd0 = oWr + 3 * NW
    obd1, ob0, ob1, obr = obd0 + 64, obd0 + 64 + NB, obd0 + 64 + NB + NW, obd0 + 64 + NB + 2 * NW
    oWc0 = obr + 3
    oWc1 = oWc0 + NW * 64
    zero = oWc1 + NW * 64

    def stream(mats, weave):
        parts = []
        for rows, blocks, nat in mats:
            cols = sum(b[3] for b in blocks)
            r, c = _fragment_index(rows, cols, nat)
            off = torch.full_like(r, -1)
            start = 0
            for base, rs, cs, nc in blocks:
                inside = (r >= 0) & (c >= start) & (c < start + nc)
                off = torch.where(inside, base + r * rs + (c - start) * cs, off)
                start += nc
            parts.append(off)
        parts = _weave(parts, *weave)
        flat = torch.cat(parts)
        assert flat.numel() <= total * 512
        return torch.cat([flat, flat.new_full((total * 512 - flat.numel(),), -1)])

    # forward: the rgb layer's fragments ride behind each pair of the last hidden layer's output tiles; backward: the
    # density layer's behind each pair of bottleneck-gradient tiles (field_train.hip: the consumer layer runs on every
    # finished pair, so that only one pair of accumulators is live and two workgroups fit a CU)
    # dir_in_stream (inference with rays-fastest lanes): the direction block, the layer bias (against the constant-1 column of
    # the ray's tile) and zero padding form one more 32-column input tile of the two colour layers
    aux0 = [(oW0 + NB, k0, 1, E), (ob0, 1, 0, 1), (zero, 0, 0, 31 - E)] if dir_in_stream else []
    aux1 = [(oW1 + NW + NB, k1, 1, E), (ob1, 1, 0, 1), (zero, 0, 0, 31 - E)] if dir_in_stream else []
    fwd = stream([(64, [(oWd0, F_in, 1, F_in)], True), (NB, [(oWd1, 64, 1, 64)], False), (NW, [(oWc0, 64, 1, 64)] + aux0, False),
                  (NW, [(oW1, k1, 1, NW), (oWc1, 64, 1, 64)] + aux1, False), (3, [(oWr, NW, 1, NW)], False)], weave=(3, 4))
    bwd = stream([(NW, [(oWr, 1, NW, 3)], True), (NW, [(oW1, 1, k1, NW)], False),
                  (NB, [(oW1 + NW, 1, k1, NW), (oW0, 1, k0, NW)], False), (64, [(oWd1, 1, 64, NB)], False),
                  (F_in, [(oWd0, 1, F_in, 64)], False)], weave=(2, 3))
    acc_w, acc_b, acc_64 = _acc_order(NW, "cpu"), _acc_order(NB, "cpu"), _acc_order(64, "cpu")
    e = torch.arange(E)
    we = torch.cat([(oW0 + acc_w[:, None] * k0 + NB + e[None, :]).reshape(-1),
                    (oW1 + acc_w[:, None] * k1 + NW + NB + e[None, :]).reshape(-1)])
    be = torch.cat([ob0 + acc_w, ob1 + acc_w])
    a32 = _acc_order(32, "cpu")
    bv = torch.cat([obd0 + acc_64, obd1 + acc_b, torch.where(a32 < 3, obr + a32, torch.full_like(a32, -1))])
    idx = torch.cat([fwd, bwd, we, be, bv])
    hit = (torch.where(idx >= 0, idx, torch.full_like(idx, zero)).to(device), zero + 1)
    _FRAG_CACHE[key] = hit
    return hit


_WGRAD_WS = {}


def wgrad(A, B1, B2=None):
    """A^T [B1 | B2] as float32 [A columns, B columns] by the hand-written kernel (csrc/wgrad.hip: LDS transpose reads + bf16
    MFMA, every operand element read once, fixed-order split-K): A, B1, B2 are column-slice views [M, k] of bf16 buffers
    (k a multiple of 32; A <= 256 columns, B1 + B2 <= 288)."""
    lib = _lib.load()
    M, KA = A.shape
    kb1, kb2 = B1.shape[1], (0 if B2 is None else B2.shape[1])
    for t in (A, B1) + ((B2,) if B2 is not None else ()):
        assert t.dtype == torch.bfloat16 and t.stride(1) == 1 and t.shape[0] == M and t.shape[1] % 32 == 0, (t.dtype, t.stride(), t.shape)
    n = lib.ucn_wgrad_ws_floats(KA, kb1 + kb2, M)
    # one split-K workspace per stream (the sky branch runs beside the field), keyed by the Stream OBJECT kept alive in the entry:
    # a raw handle value can be recycled by a later stream and would alias a workspace still in flight
    st = torch.cuda.current_stream()
    key = (str(A.device), st.cuda_stream)
    hit = _WGRAD_WS.get(key)
    if hit is None or hit[0] != st or hit[1].numel() < n:
        if len(_WGRAD_WS) > 8:
            _WGRAD_WS.clear()
        hit = _WGRAD_WS[key] = (st, torch.empty(n, device=A.device))
    ws = hit[1]
    out = torch.empty(KA, kb1 + kb2, device=A.device)
    _lib.check(lib.ucn_wgrad_bf16(A.data_ptr(), A.stride(0), KA, B1.data_ptr(), B1.stride(0), kb1, _lib.ptr(B2),
                                  0 if B2 is None else B2.stride(0), kb2, M, ws.data_ptr(), out.data_ptr(), _lib.stream()))
    return out


def _wgrad_cols(gy, act, lo, hi):
    """gy^T @ act[:, lo:hi] as float32 [gy columns, hi - lo]: split-K batched GEMM over 8192-row chunks on a strided
    column view of the activation buffer (no copy; see _TallLinear for why the reduction is cut)."""
    m, c = gy.shape[0], _TallLinear.CHUNK
    if m >= 4 * c and m % c == 0:
        return torch.bmm(gy.reshape(m // c, c, -1).transpose(1, 2), act.reshape(m // c, c, -1)[:, :, lo:hi]).float().sum(0)
    return (gy.t() @ act[:, lo:hi]).float()


def prepare_heads(Wd0, bd0, Wd1, bd1, W0, b0, W1, b1, Wr, br, dir_in_stream=False):
    """Everything ucn_train_fwd / ucn_train_bwd need from the NeRF field's dense parameters, as ONE cat + ONE cast + ONE gather:
    (forward fragment stream, dgrad fragment stream, direction blocks [2 NW, E] and their biases [2 NW] in accumulator
    order (bf16), bd0 / bd1 / br in accumulator order (fp32)).  The colour layers enter the forward stream composed with
    the activation-free bottleneck (models.py:508): (W0x Wd1), [W1h | W1x Wd1], W bd1 folded into the biases."""
    lib = _lib.load()
    dev, dt = Wd0.device, torch.bfloat16
    NB, NW, F_in = Wd1.shape[0], W0.shape[0], Wd0.shape[1]
    E = W0.shape[1] - NB
    T = lib.ucn_train_fwd_fragments()
    idx, n_src = _head_gather_index(F_in, NB, NW, E, T, dev, dir_in_stream)
    zero = _FRAG_CACHE.get(("zero1", str(dev)))
    if zero is None:
        zero = _FRAG_CACHE[("zero1", str(dev))] = torch.zeros(1, device=dev)
    W0x32, W1x32, Wd132, bd132 = W0.detach()[:, :NB].float(), W1.detach()[:, NW:NW + NB].float(), Wd1.detach().float(), bd1.detach().float()
    Wd1t = Wd132.t().contiguous()                                    # (csrc/gemm_f32.hip: no library GEMM in the autocast step, r06)
    Wc0, Wc1 = dense_f32.gemm(W0x32.contiguous(), Wd1t), dense_f32.gemm(W1x32.contiguous(), Wd1t)
    b0c, b1c = torch.addmv(b0.detach().float(), W0x32, bd132), torch.addmv(b1.detach().float(), W1x32, bd132)
    src = torch.cat([t.detach().reshape(-1).float() for t in (Wd0, Wd1, W0, W1, Wr, bd0, bd1, b0c, b1c, br, Wc0, Wc1)] + [zero]).to(dt)
    assert src.numel() == n_src
    got = src[idx]
    packed, packed_t = got[:T * 512], got[T * 512:2 * T * 512]
    o = 2 * T * 512
    We = got[o:o + 2 * NW * E].view(2 * NW, E)
    be = got[o + 2 * NW * E:o + 2 * NW * E + 2 * NW]
    bv = got[o + 2 * NW * E + 2 * NW:].float()
    return packed, packed_t, We, be, bv[:64], bv[64:64 + NB], bv[64 + NB:]


class _FusedHeads(torch.autograd.Function):
    """Density MLP + colour MLP + rgb layer + output activations of the NeRF field (models.py:507-674, the reference's
    topology and widths) under bf16 autocast: the forward is ONE HIP kernel (`ucn_train_fwd`: activations stay in
    registers from the feature row to density / rgb, each hidden activation and its ReLU mask is stored once, into one
    [M, 864] buffer); the backward's dgrad chain is ONE HIP kernel too (`ucn_train_bwd`: transposed weight fragments, the
    forward's masks, the activation derivatives from the saved outputs), and every layer's weight + bias gradient is one
    split-K library GEMM on the pre-activation gradients it stores (column layout above).  All weight preparation (bf16
    copies, both fragment streams, accumulator-order biases) is one cat + one cast + one gather per step."""

    @staticmethod
    def forward(ctx, feat, enc, Wd0, bd0, Wd1, bd1, W0, b0, W1, b1, Wr, br, N, S, head, chan=None):
        lib = _lib.load()
        # the feature gradient goes back level-major (see _FieldFeatures) when `feat` is that node's own output buffer
        ctx.chan = chan if (chan is not None and chan.feat_ptr == feat.data_ptr() and feat.dtype == torch.float32 and feat.is_contiguous()
                            and feat.shape[1] == chan.levels * chan.level_dim and feat.shape[1] % 4 == 0
                            and os.environ.get("UCN_FEAT_GRAD_LM", "1") == "1") else None
        dev, dt = feat.device, torch.bfloat16
        NB, NW, F_in = Wd1.shape[0], W0.shape[0], Wd0.shape[1]
        E = W0.shape[1] - NB
        T = lib.ucn_train_fwd_fragments()
        with torch.autocast("cuda", enabled=False):
            packed, packed_t, We, be, bias0, bias1, biasr = prepare_heads(Wd0, bd0, Wd1, bd1, W0, b0, W1, b1, Wr, br)
            eb = enc.to(dt)
            # what the bf16 GEMM + bias would hold (operands rounded to bf16, fp32 accumulation, the sum rounded to bf16), acc order --
            # on csrc/gemm_f32.hip instead of the library's bf16 kernel (r06)
            eb4, We4 = dense_f32._rows(eb.float()), dense_f32._rows(We.float())
            pr = dense_f32.gemm(eb4, We4, be.float().contiguous()).to(dt).float()
            pr0, pr1 = pr[:, :NW].contiguous(), pr[:, NW:].contiguous()
            M = N * S
            f = feat.float().contiguous()
            act = torch.empty(M, ACT_LD, device=dev, dtype=dt)
            aux = torch.zeros(N, 32, device=dev, dtype=dt)
            aux[:, :E] = eb
            aux[:, E] = 1.0
            fb_in_act = F_in % 8 == 0                                   # the kernel writes the bf16 feature copy into the row
            density, rgb = torch.empty(M, device=dev), torch.empty(M, 3, device=dev)
            m0 = torch.empty(M, 2, device=dev, dtype=torch.int32)
            m1, m2 = (torch.empty(M, 2, 4, device=dev, dtype=torch.int32) for _ in range(2))
            hd = (ctypes.c_float * 4)(*[float(v) for v in head])
            base = act.data_ptr()
            # r04: with the reference's widths the bottleneck x is neither stored nor read back -- it is linear in h0 (models.py:508 has
            # no activation there), so every weight gradient that had x or d x as an operand is formed from the [256, 64] products
            # d0^T h0, d1^T h0 instead (backward below): 0.5 GB less stored here, 0.5 GB less in the backward, 1.5 GB less read by wgrad
            # UCN_HEADS_STORED_X=1 keeps the r03 route (x stored, d x written by the backward, three more ucn_wgrad_bf16 passes)
            # selectable: the A/B DESIGN cites and the cross-check of tests/test_train_step.py
            lean = NW == 256 and NB == 256 and os.environ.get("UCN_HEADS_STORED_X", "0") != "1"
            _lib.check(lib.ucn_train_fwd(f.data_ptr(), F_in, packed.data_ptr(), bias0.data_ptr(), bias1.data_ptr(),
                                         biasr.data_ptr(), pr0.data_ptr(), pr1.data_ptr(), N, S, base + 2 * _ACT_H0, None if lean else base + 2 * _ACT_X,
                                         base + 2 * _ACT_H1, base + 2 * _ACT_H2, ACT_LD, aux.data_ptr(), base + 2 * _ACT_AUX,
                                         base + 2 * _ACT_FB if fb_in_act else None, hd, density.data_ptr(),
                                         rgb.data_ptr(), m0.data_ptr(), m1.data_ptr(), m2.data_ptr(), 0, _lib.stream()))
            if not fb_in_act:
                act[:, _ACT_FB:_ACT_FB + F_in] = f
        ctx.save_for_backward(act, m0, m1, m2, packed_t, density, rgb, Wd1, bd1, W0, W1)
        ctx.meta = (N, S, NB, NW, E, F_in, feat.dtype, Wd0.dtype, bd0.dtype, tuple(float(v) for v in head), lean)
        return density, rgb

    @staticmethod
    def backward(ctx, g_density, g_rgb):
        lib = _lib.load()
        act, m0, m1, m2, packed_t, density, rgb, Wd1, bd1, W0, W1 = ctx.saved_tensors
        N, S, NB, NW, E, F_in, f_dt, w_dt, b_dt, head, lean = ctx.meta
        dt, dev, M = torch.bfloat16, act.device, act.shape[0]
        with torch.autocast("cuda", enabled=False):
            g_rgb = torch.zeros(M, 3, device=dev) if g_rgb is None else g_rgb.reshape(M, 3).float().contiguous()
            g_density = None if g_density is None else g_density.reshape(-1).float().contiguous()
            d1, d0 = (torch.empty(M, NW, device=dev, dtype=dt) for _ in range(2))
            gx = None if lean else torch.empty(M, NW, device=dev, dtype=dt)
            gh0 = torch.empty(M, 64, device=dev, dtype=dt)
            # dy: colour-logit gradients (columns 0-2) + the density head's gradient at the bottleneck (column 3); lean: as a zero-filled
            # 32-wide tile, the A operand of ucn_wgrad_bf16 (the rgb layer's and the bottleneck row's weight gradients without a library GEMM)
            dy = torch.zeros(M, 32 if lean else 4, device=dev, dtype=dt)
            gfeat = torch.empty(M, F_in, device=dev)
            lm = ctx.chan is not None and f_dt == torch.float32
            if lm:
                ctx.chan.lm = gfeat.data_ptr()                        # the same bytes as [levels][M][level_dim], every value / 6
            hd = (ctypes.c_float * 4)(*head)
            _lib.check(lib.ucn_train_bwd(g_rgb.data_ptr(), _lib.ptr(g_density), hd, density.data_ptr(), rgb.data_ptr(),
                                         packed_t.data_ptr(), m0.data_ptr(), m1.data_ptr(), m2.data_ptr(), N, S, F_in | ((_lib.GFEAT_LEVEL_MAJOR if ctx.chan.level_dim == 2 else _lib.GFEAT_LEVEL_MAJOR4) if lm else 0),
                                         d1.data_ptr(), d0.data_ptr(), _lib.ptr(gx), gh0.data_ptr(), dy.data_ptr(), dy.shape[1], gfeat.data_ptr(),
                                         _lib.stream()))
            # [NW, NW + NB] and [NW, 32]: as ONE 544-column GEMM the library picks a kernel twice as slow (602 us against
            # 302 + 119 us, tools/wgrad_bench.py); the 288-column GEMM of layer 0 is fine (255 us)
            if lean:
                # hand-written weight-gradient kernel (csrc/wgrad.hip), each pass reads its operands once.  x = h0 Wd1^T + bd1 and
                # d x = d0 W0x + d1 W1x (+ the density head's column) never touch memory: with P_i = d_i^T h0 [NW, 64] and
                # s_i = d_i^T 1 [NW] (the constant-1 column of the aux tile),
                #   d_i^T x = P_i Wd1^T + s_i bd1^T,     (d x)^T h0 = W0x^T P0 + W1x^T P1 (+ e0 g_raw^T h0),   (d x)^T 1 likewise
                # -- four [256, 64] x [64, 256] products in fp32 on the weights as the kernels saw them (bf16-rounded) instead of
                # 2.5 GB of activation traffic; exact where the stored route rounded x and d x to bf16
                rb = lambda w: w.detach().to(dt).float()
                Wd1b, bd1b, W0xb, W1xb = rb(Wd1), rb(bd1), rb(W0[:, :NB]), rb(W1[:, NW:NW + NB])
                h0a = act[:, _ACT_AUX:_ACT_FB]                                  # [aux tile (32) | h0 (64)]
                P1h = wgrad(d1, act[:, _ACT_H1:_ACT_H1 + NW])                  # [NW, NW]
                Q1, Q0 = wgrad(d1, h0a), wgrad(d0, h0a)                       # [NW, 32 + 64] each
                P1, P0, s1, s0 = Q1[:, 32:].contiguous(), Q0[:, 32:].contiguous(), Q1[:, E], Q0[:, E]
                G = dense_f32.gemm
                d1x = torch.addr(G(P1, Wd1b), s1, bd1b)                       # d1^T x   [NW, NB]
                d0x = torch.addr(G(P0, Wd1b), s0, bd1b)                       # d0^T x
                G1 = torch.cat([P1h, d1x, Q1[:, :32]], dim=1)                 # [NW, NW + NB + 32]
                G0 = torch.cat([d0x, Q0[:, :32]], dim=1)                      # [NW, NB + 32]
                gWd1_ = G(W0xb.t().contiguous(), P0.t().contiguous())         # W0x^T P0   [NB, 64]
                G(W1xb.t().contiguous(), P1.t().contiguous(), flags=dense_f32.ACCUMULATE, out=gWd1_)
                gbd1_ = (W0xb * s0[:, None]).sum(0) + (W1xb * s1[:, None]).sum(0)        # W0x^T s0 + W1x^T s1   [NB]
                Gy = wgrad(dy, act[:, _ACT_H2:_ACT_H2 + NW], act[:, _ACT_AUX:_ACT_AUX + 32])     # dy^T [h2 | aux]   [32, NW + 32]
                if g_density is not None:                                     # the density head: feature 0 of the bottleneck
                    gWd1_[0] += wgrad(dy, act[:, _ACT_H0:_ACT_H0 + 64])[3]    # dy[:, 3]^T h0
                    gbd1_[0] += Gy[3, NW + E]                                 # dy[:, 3]^T 1
                Gd1 = torch.cat([torch.zeros(NB, E, device=dev), gbd1_[:, None], torch.zeros(NB, 31 - E, device=dev), gWd1_], dim=1)   # the stored route's [NB, 32 + 64] layout
            elif NW == 256 and NB == 256:
                aux = act[:, _ACT_AUX:_ACT_AUX + 32]
                G1 = torch.cat([wgrad(d1, act[:, _ACT_H1:_ACT_H1 + NW]), wgrad(d1, act[:, _ACT_X:_ACT_X + NB], aux)], dim=1)   # [NW, NW + NB + 32]
                G0 = wgrad(d0, act[:, _ACT_X:_ACT_X + NB], aux)                # [NW, NB + 32]
                Gd1 = wgrad(gx, act[:, _ACT_AUX:_ACT_FB])                     # [NB, 32 + 64]
            else:
                G1a, G1b = _wgrad_cols(d1, act, _ACT_H1, _ACT_AUX), _wgrad_cols(d1, act, _ACT_AUX, _ACT_AUX + 32)
                G1 = torch.cat([G1a, G1b], dim=1)
                G0 = _wgrad_cols(d0, act, _ACT_X, _ACT_AUX + 32)                  # [NW, NB + 32]
                Gd1 = _wgrad_cols(gx, act, _ACT_AUX, _ACT_FB)                     # [NB, 32 + 64]
            gW1, gb1 = G1[:, :NW + NB + E], G1[:, NW + NB + E]
            gW0, gb0 = G0[:, :NB + E], G0[:, NB + E]
            gWd1, gbd1 = Gd1[:, 32:], Gd1[:, E]
            if lean:
                gWr, gbr = Gy[:3, :NW], Gy[:3, NW + E]
                fb_cols = (F_in + 31) // 32 * 32 if F_in % 8 == 0 else 1 << 30          # (F_in % 8 != 0: the feature copy is not in the row)
                if fb_cols <= 64:
                    # gh0^T [features | aux]: the feature block rounded up to whole 32-column tiles (the waymo.gin grid has 10 levels x 4 = 40
                    # features) -- the columns behind F_in are whatever the row holds; an output column depends on ITS operand column only
                    G00 = wgrad(gh0, act[:, _ACT_FB:_ACT_FB + fb_cols], act[:, _ACT_AUX:_ACT_AUX + 32])          # [64, fb_cols + 32]
                    gWd0, gbd0 = G00[:, :F_in], G00[:, fb_cols + E]
                else:
                    gWd0, gbd0 = _wgrad_cols(gh0, act, _ACT_FB, _ACT_FB + F_in), _colsum(gh0)
            else:
                Gr = _wgrad_cols(dy, act, _ACT_H2, _ACT_H2 + NW)              # [4, NW]
                gWr, gbr = Gr[:3], _colsum(dy)[:3]
                gWd0, gbd0 = _wgrad_cols(gh0, act, _ACT_FB, _ACT_FB + F_in), _colsum(gh0)
        return (gfeat.to(f_dt), None, gWd0.to(w_dt), gbd0.to(b_dt), gWd1.to(w_dt), gbd1.to(b_dt), gW0.to(w_dt), gb0.to(b_dt),
                gW1.to(w_dt), gb1.to(b_dt), gWr.to(w_dt), gbr.to(b_dt), None, None, None, None)


class _PropHeads(torch.autograd.Function):
    """The proposal field's dense part (models.py:507-516, disable_rgb: Linear(F,64) + ReLU, Linear(64,1), softplus) as
    three HIP launches forward + backward (`ucn_prop_train_fwd / _bwd`, prop_train.hip) instead of ~45 library ones.
    Under autocast the kernels round operands and layer outputs to bf16 like the library GEMMs would."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, feat, W0, b0, W1, b1, density_bias, bf16):
        lib = _lib.load()
        feat, W0, b0, W1, b1 = (t.contiguous() for t in (feat, W0, b0, W1, b1))
        M, F_in = feat.shape
        density = torch.empty(M, device=feat.device)
        _lib.check(lib.ucn_prop_train_fwd(feat.data_ptr(), F_in, W0.shape[0], W0.data_ptr(), b0.data_ptr(), W1.data_ptr(), b1.data_ptr(),
                                          float(density_bias), int(bf16), M, density.data_ptr(), 0, 0, _lib.stream()))
        ctx.save_for_backward(feat, W0, b0, W1, b1, density)
        ctx.consts = (float(density_bias), int(bf16))
        return density

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_density):
        lib = _lib.load()
        feat, W0, b0, W1, b1, density = ctx.saved_tensors
        M, F_in = feat.shape
        g = g_density.reshape(-1).float().contiguous()
        gfeat = torch.empty_like(feat) if ctx.needs_input_grad[0] else None
        gW0, gb0, gW1, gb1 = torch.empty_like(W0), torch.empty_like(b0), torch.empty_like(W1), torch.empty_like(b1)
        ws = torch.empty(lib.ucn_prop_train_bwd_ws_floats(F_in, M), device=feat.device)
        _lib.check(lib.ucn_prop_train_bwd(feat.data_ptr(), F_in, W0.shape[0], W0.data_ptr(), b0.data_ptr(), W1.data_ptr(), b1.data_ptr(),
                                          *ctx.consts, M, density.data_ptr(), g.data_ptr(), _lib.ptr(gfeat), gW0.data_ptr(),
                                          gb0.data_ptr(), gW1.data_ptr(), gb1.data_ptr(), ws.data_ptr(), _lib.stream()))
        return gfeat, gW0, gb0, gW1, gb1, None, None


def _fusable_prop(mlp, feat):
    l0, l1 = mlp.density_layer[0], mlp.density_layer[2]
    return (mlp.disable_rgb and len(mlp.density_layer) == 3 and feat.is_cuda and feat.shape[1] <= 24 and l0.out_features == 64
            and l1.out_features == 1 and l0.bias is not None and l1.bias is not None
            and (not torch.is_autocast_enabled() or torch.get_autocast_dtype("cuda") == torch.bfloat16))


def _fusable_heads(mlp, feat):
    return (torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16 and not mlp.disable_rgb
            and mlp.net_depth_viewdirs == 2 and mlp.skip_layer_dir == 0 and feat.shape[1] <= 64
            and mlp.density_layer[0].out_features == 64 and mlp.density_layer[2].out_features == 256
            and mlp.net_width_viewdirs == 256 and mlp.rgb_layer.out_features == 3)


def field_heads(mlp, feat, viewdirs, N, S, chan=None, glo=None):
    """models.py:507-674 on [N*S, F] features: density MLP, softplus, colour MLP (torch GEMMs).

    glo = (a, b), float32 [N, bottleneck] (MLP.glo_affine): the GLO modulation of the bottleneck, per ray.  It takes the
    uncomposed route (_ColourMLPGlo); the fused / composed routes fold the bottleneck layer into the colour layers and are
    only taken without it.

    The reference concatenates [bottleneck, dir_enc] (and [h, bottleneck, dir_enc] after the skip layer) per SAMPLE
    and multiplies by one weight.  The same product is formed here column block by column block: per-sample blocks
    as GEMMs that accumulate into one output, the per-RAY direction block (and the layer bias) as one small
    [N, 27] GEMM broadcast over the samples -- no [N*S, 283] / [N*S, 539] concatenations, 7 % fewer flops, and the
    bias / direction-weight gradients reduce over rays instead of samples."""
    if glo is None and _fusable_heads(mlp, feat) and os.environ.get("UCN_FUSED_HEADS", "1") == "1":
        d0, d1, l0, l1, lr = mlp.density_layer[0], mlp.density_layer[2], mlp.lin_second_stage_0, mlp.lin_second_stage_1, mlp.rgb_layer
        density, rgb = _FusedHeads.apply(feat, view_encoding(viewdirs, mlp.deg_view), d0.weight, d0.bias, d1.weight, d1.bias,
                                         l0.weight, l0.bias, l1.weight, l1.bias, lr.weight, lr.bias, N, S,
                                         (mlp.density_bias, mlp.rgb_premultiplier, mlp.rgb_bias, mlp.rgb_padding), chan)
        return density.reshape(N, S), rgb.reshape(N, S, 3)
    if _fusable_prop(mlp, feat) and os.environ.get("UCN_FUSED_HEADS", "1") == "1":
        l0, l1 = mlp.density_layer[0], mlp.density_layer[2]
        density = _PropHeads.apply(feat, l0.weight, l0.bias, l1.weight, l1.bias, mlp.density_bias, torch.is_autocast_enabled())
        return density.reshape(N, S), torch.zeros(N, S, 3, device=feat.device)
    if (glo is None and not mlp.disable_rgb and mlp.net_depth_viewdirs == 2 and mlp.skip_layer_dir == 0 and mlp.net_width_viewdirs % 8 == 0
            and dense_f32.usable(feat, mlp.density_layer[0].weight) and not dense_f32.library_route()
            and os.environ.get("UCN_F32_COMPOSED", "1") == "1"):        # 0: the uncomposed _ColourMLP on the same kernels (A/B, cross-check)
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
        if os.environ.get("UCN_FIELD_NODE", "1") != "0" and feat.shape[1] % 4 == 0:
            # r06: density layer 0, the density row and the colour MLP as one node (_FieldMLPComposed); 0: three nodes (A/B, cross-check)
            raw, rgbl = _FieldMLPComposed.apply(feat, d0l.weight, d0l.bias, d1l.weight[:1], d1l.bias[:1], A0, pr0, W1h, A1, pr1,
                                                mlp.rgb_layer.weight, mlp.rgb_layer.bias, N, S)
        else:
            h0 = lin(feat, d0l.weight, d0l.bias, relu=True)                                      # [N*S, 64]
            rgbl = _ColourMLPComposed.apply(h0, A0, pr0, W1h, A1, pr1, mlp.rgb_layer.weight, mlp.rgb_layer.bias, N, S)
            raw = lin(h0, d1l.weight[:1], d1l.bias[:1])                                          # feature 0 of the bottleneck (models.py:508)
        density = F.softplus(raw.reshape(N, S) + mlp.density_bias)
        rgb = torch.sigmoid(mlp.rgb_premultiplier * rgbl.reshape(N, S, -1) + mlp.rgb_bias)
        return density, rgb * (1 + 2 * mlp.rgb_padding) - mlp.rgb_padding
    x = tall_linear(mlp.density_layer[2], tall_linear(mlp.density_layer[0], feat, relu=True))    # [N*S, bottleneck]
    if mlp.disable_rgb:
        return F.softplus(x.reshape(N, S, -1)[..., 0] + mlp.density_bias), torch.zeros(N, S, 3, device=feat.device)
    enc = view_encoding(viewdirs, mlp.deg_view)                                                  # [N, 27], per ray
    if mlp.net_depth_viewdirs == 2 and mlp.skip_layer_dir == 0 and mlp.net_width_viewdirs % 8 == 0:
        l0, l1 = mlp.lin_second_stage_0, mlp.lin_second_stage_1                                  # the reference's topology
        if glo is not None:
            h, raw = _ColourMLPGlo.apply(x, glo[0], glo[1], enc, l0.weight, l0.bias, l1.weight, l1.bias, N, S)
        else:
            h, raw = _ColourMLP.apply(x, enc, l0.weight, l0.bias, l1.weight, l1.bias, N, S)
        density = F.softplus(raw.reshape(N, S) + mlp.density_bias)
        rgb = torch.sigmoid(mlp.rgb_premultiplier * tall_linear(mlp.rgb_layer, h).reshape(N, S, -1) + mlp.rgb_bias)
        return density, rgb * (1 + 2 * mlp.rgb_padding) - mlp.rgb_padding
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
    rgb = torch.sigmoid(mlp.rgb_premultiplier * tall_linear(mlp.rgb_layer, h).reshape(N, S, -1) + mlp.rgb_bias)
    return density, rgb * (1 + 2 * mlp.rgb_padding) - mlp.rgb_padding


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


class _SkyTrunkF32(torch.autograd.Function):
    """The sky NeRF's dense layers (models.py:743-820) of the fp32 training step as ONE autograd node over csrc/gemm_f32.hip (r05): the
    eight 256-wide layers (skip into layer 5 as a second accumulating GEMM on the padded points), the density row, the view layer with
    feature_linear composed in (Mv) and its per-RAY direction term as the GEMM's row-group bias, the rgb row.  Every bias + ReLU is a
    GEMM epilogue, and every ReLU derivative is the MASK epilogue of the d X GEMM that produces the layer's output gradient (mask = the
    layer's stored output) -- no elementwise pass over an [M, 256] tensor is left (r04: threshold_backward 4.4 ms, adds 1.3 ms, ReLU /
    bias kernels 2.0 ms of the 60 ms step).  Each activation is stored once (fp32, [M, 256]); two [M, 256] gradient buffers ping-pong.
    Inputs: pts4 [M, 4] (points padded with a zero column; no gradient), per_ray [n, 128], the layer parameters."""

    @staticmethod
    def forward(ctx, pts4, per_ray, Mv, bv, Wa, ba, Wr, br, *wb):
        G = dense_f32.gemm
        Ws, bs = wb[0::2], wb[1::2]
        M, n = pts4.shape[0], per_ray.shape[0]
        group = M // n
        pad4 = lambda w: torch.nn.functional.pad(w, (0, 4 - w.shape[1] % 4)) if w.shape[1] % 4 else w
        hs = []
        E = lambda n_: dense_f32.rows_buffer(M, n_, pts4.device)          # (row strides off the powers of two: rows_buffer)
        h = G(pts4, pad4(Ws[0].detach()).contiguous(), bs[0].detach(), dense_f32.RELU, out=E(256))
        hs.append(h)
        for i in range(1, 8):
            W = Ws[i].detach()
            if i == 5:                                                      # [pts | h] -> two column blocks of the weight: the 3-d block
                h = G(h, W[:, 3:].contiguous(), bs[i].detach(), dense_f32.RELU,       # rides in the wide product's epilogue (r06)
                      out=E(256), x2=pts4, w2=pad4(W[:, :3]).contiguous())
            else:
                h = G(h, W.contiguous(), bs[i].detach(), dense_f32.RELU, out=E(256))
            hs.append(h)
        sigma = G(h, Wa.detach().contiguous(), ba.detach())                                    # [M, 1]
        hv = G(h, Mv.detach().contiguous(), bv.detach(), dense_f32.RELU, out=E(128), rowbias=per_ray.detach().contiguous(), rgroup=group)    # [M, 128]
        rgbl = G(hv, Wr.detach().contiguous(), br.detach())                                    # [M, 3] logits
        ctx.save_for_backward(pts4, Mv, Wa, Wr, hv, *hs, *Ws)
        dense_f32.stash_amax(ctx, (pts4, hv, *hs))
        ctx.group = group
        return sigma, rgbl

    @staticmethod
    def backward(ctx, g_sigma, g_rgbl):
        # (no gradient into the sample points: the reference's rays are data.  A caller that makes them differentiable -- pose refinement --
        #  must take the layer-by-layer route, UCN_SKY_F32_CHAIN=0, which propagates it)
        assert not ctx.needs_input_grad[0], "_SkyTrunkF32 does not propagate a gradient into the sample points (use UCN_SKY_F32_CHAIN=0)"
        G, WG = dense_f32.gemm, dense_f32.wgrad
        saved = ctx.saved_tensors
        pts4, Mv, Wa, Wr, hv = saved[:5]
        hs, Ws = saved[5:13], saved[13:21]
        dense_f32.restore_amax(ctx, (pts4, hv, *hs))
        M, dev = pts4.shape[0], pts4.device
        n = M // ctx.group
        g4 = torch.zeros(M, 4, device=dev)
        g4[:, :3] = g_rgbl
        gs4 = torch.zeros(M, 4, device=dev)
        gs4[:, :1] = g_sigma
        padT = lambda w: torch.nn.functional.pad(w.detach().t(), (0, 4 - w.shape[0] % 4)).contiguous() if w.shape[0] % 4 else w.detach().t().contiguous()
        # rgb row
        gWr4, gbr4 = WG(g4, hv, True)
        gWr, gbr = gWr4[:3], gbr4[:3]
        E = lambda n_: dense_f32.rows_buffer(M, n_, dev)
        dv = G(g4, padT(Wr), mask=hv, out=E(128))                                              # d (view layer pre-activation) [M, 128]
        gMv, gbv = WG(dv, hs[7], True)
        g_per_ray = dv.unflatten(0, (n, ctx.group)).sum(dim=1)                                 # (a strided view: no copy)
        # into h7: view layer + density row, masked by h7 > 0 after the sum
        gWa4, gba4 = WG(gs4, hs[7], True)
        gWa, gba = gWa4[:1], gba4[:1]
        d = G(dv, Mv.detach().t().contiguous(), mask=hs[7], out=E(256), x2=gs4, w2=padT(Wa))    # (the density row's rank-1 term in the epilogue, r06)
        del dv
        spare = E(256)                                                                         # two gradient buffers ping-pong
        gW, gb = [None] * 8, [None] * 8
        for i in range(7, 0, -1):
            W = Ws[i].detach()
            if i == 5:
                gWh, gb[i] = WG(d, hs[4], True)
                gWp = WG(d, pts4, False)[0]
                gW[i] = torch.cat([gWp[:, :3], gWh], dim=1)
                d, spare = G(d, W[:, 3:].t().contiguous(), mask=hs[4], out=spare), d
            else:
                gW[i], gb[i] = WG(d, hs[i - 1], True)
                d, spare = G(d, W.t().contiguous(), mask=hs[i - 1], out=spare), d
        gW0, gb[0] = WG(d, pts4, True)
        gW[0] = gW0[:, :3]
        out = [None, g_per_ray, gMv, gbv, gWa, gba, gWr, gbr]
        for i in range(8):
            out += [gW[i], gb[i]]
        return tuple(out)


def sky_forward(net, origins, directions, cam_dirs, far):
    """models.py:852-904 + :743-850 with torch ops (training only; rendering uses csrc/sky.hip)."""
    n = origins.shape[0]
    near = far.reshape(n, 1)
    sky_far = (near[0:1].detach() * 1.5).expand_as(near)        # 1.5 x the first ray's far plane (models.py:856-858), on the device:
    tv = torch.linspace(0., 1., steps=120, device=origins.device)   # (r06: was float(near[0].item()) -- a host sync in every step)
    z = (near * (1. - tv) + 1. / sky_far * tv).expand(n, 120)
    pts = origins[:, None, :] + directions[:, None, :] * z[:, :, None]
    freqs = 2. ** torch.linspace(0., 3., 4, device=origins.device)
    embed = lambda v: torch.cat([v] + [fn(v * f) for f in freqs for fn in (torch.sin, torch.cos)], dim=-1)
    on_kernels = dense_f32.usable(pts, net.pts_linears[0].weight) and not dense_f32.library_route()
    # the view encoding is the same for a ray's 120 samples: the kernel route needs it per RAY only (r06: it was formed per sample --
    # nine elementwise passes and a 27-wide concatenation over [n, 120, .] -- and read back as venc[:, 0])
    venc = embed(cam_dirs)[:, None, :] if on_kernels else embed(cam_dirs[:, None, :].expand(-1, 120, -1))
    if on_kernels:
        # the fp32 step: every layer on csrc/gemm_f32.hip.  The reference's two concatenations (models.py:790-795: [pts | h] into
        # layer 5, [feature | view encoding] into the views layer) are products by column blocks of the weight instead -- the
        # direction block is per RAY ([n, 27] against [n * 120, 283] rows)
        lin = dense_f32.hip_linear
        Lv, Lf = net.views_linears[0], net.feature_linear
        Wf_in = Lf.out_features
        # feature_linear has no activation (models.py:806): composed into the views layer, Mv = Wv[:, :256] Wf -- formed with
        # differentiable ops, autograd carries d Mv back to both weights -- one 256 x 256 layer less forward and backward
        Mv = lin(Lv.weight[:, :Wf_in], Lf.weight.t())                                      # [128, 256]
        cb = lin(Lf.bias[None, :], Lv.weight[:, :Wf_in])                                   # Wv[:, :256] b_f   [1, 128]
        per_ray = lin(venc[:, 0, :], Lv.weight[:, Wf_in:]) + cb                            # the same encoding for a ray's 120 samples
        if os.environ.get("UCN_SKY_F32_CHAIN", "1") == "1":
            # r05: one autograd node, bias / ReLU / ReLU-derivative / per-ray term as GEMM epilogues (_SkyTrunkF32)
            pts4 = F.pad(pts.reshape(-1, 3), (0, 1))
            wb = [t for L in net.pts_linears for t in (L.weight, L.bias)]
            sigma, rgbl = _SkyTrunkF32.apply(pts4, per_ray, Mv, Lv.bias, net.alpha_linear.weight, net.alpha_linear.bias,
                                             net.rgb_linear.weight, net.rgb_linear.bias, *wb)
            sigma, rgb = sigma.reshape(n, 120, 1), torch.sigmoid(rgbl.reshape(n, 120, 3))
        else:                                                                              # r04: layer by layer (A/B, cross-check)
            h = pts
            for i in range(8):
                L = net.pts_linears[i]
                if i == 5:
                    h = torch.relu(lin(h, L.weight[:, 3:], L.bias) + lin(pts, L.weight[:, :3]))
                else:
                    h = lin(h, L.weight, L.bias, relu=True)
            sigma = lin(h, net.alpha_linear.weight, net.alpha_linear.bias)
            h = torch.relu(lin(h, Mv, Lv.bias) + per_ray[:, None, :])
            rgb = torch.sigmoid(lin(h, net.rgb_linear.weight, net.rgb_linear.bias))
    else:
        h = pts
        for i in range(8):
            h = F.relu(net.pts_linears[i](h))
            if i == 4:
                h = torch.cat([pts, h], dim=-1)
        sigma = net.alpha_linear(h)
        h = F.relu(net.views_linears[0](torch.cat([net.feature_linear(h), venc], dim=-1)))
        rgb = torch.sigmoid(net.rgb_linear(h))
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], dim=-1)
    dists = dists * torch.norm(directions[:, None, :], dim=-1)
    alpha = 1. - torch.exp(-F.relu(sigma[..., 0]) * dists)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + 1e-10], dim=-1), dim=-1)[:, :-1]
    return ((alpha * trans)[..., None] * rgb).sum(dim=-2)


class _SkyFused(torch.autograd.Function):
    """The sky NeRF of a training step under bf16 autocast (models.py:326-337, :743-904) as hand-written kernels
    (csrc/sky_train.hip): forward = `ucn_sky_train_fwd` (one MFMA kernel through all ten layers + the compositing; every
    hidden activation stored once as bf16, ReLU masks as bits), backward = `ucn_sky_train_bwd` (compositing backward +
    one dgrad MFMA kernel on transposed fragments) and ONE pass of the weight-gradient kernel (`wgrad`, csrc/wgrad.hip) per layer
    for weight + bias gradient over [h_{l-1} | aux] of the activation buffer.  The two 9-tile layers arrive composed (M5, Mv: see
    `sky_forward_fused`), so autograd carries their gradients on to pts_linears.5 / views_linears.0 / feature_linear."""

    @staticmethod
    def forward(ctx, o, d, cam, far, W0, b0, W1, b1, W2, b2, W3, b3, W4, b4, W6, b6, W7, b7, M5, Mv, wa, ba, Wr, br):
        from .sky import _t_vals
        lib = _lib.load()
        dev, N = o.device, o.shape[0]
        ws = [t.detach().float().contiguous() for t in (W0, b0, W1, b1, W2, b2, W3, b3, W4, b4, W6, b6, W7, b7, M5, Mv, wa, ba, Wr, br)]
        W0_, b0_, W1_, b1_, W2_, b2_, W3_, b3_, W4_, b4_, W6_, b6_, W7_, b7_, M5_, Mv_, wa_, ba_, Wr_, br_ = ws
        desc = _lib.UcnSkyTrain()
        for i, (w, b) in {0: (W0_, b0_), 1: (W1_, b1_), 2: (W2_, b2_), 3: (W3_, b3_), 4: (W4_, b4_), 6: (W6_, b6_), 7: (W7_, b7_)}.items():
            desc.w_pts[i], desc.b_pts[i] = w.data_ptr(), b.data_ptr()
        desc.m5, desc.mv = M5_.data_ptr(), Mv_.data_ptr()
        desc.w_alpha, desc.b_alpha, desc.w_rgb, desc.b_rgb = wa_.data_ptr(), ba_.data_ptr(), Wr_.data_ptr(), br_.data_ptr()
        packed = torch.empty(lib.ucn_sky_train_packed_bytes(), dtype=torch.uint8, device=dev)
        desc.packed = packed.data_ptr()
        st = _lib.stream()
        _lib.check(lib.ucn_sky_train_pack(ctypes.byref(desc), st))
        M = N * 120
        act_ld, g_ld = lib.ucn_sky_train_act_ld(), lib.ucn_sky_train_grad_ld()
        o_, d_, cam_ = (t.detach().float().contiguous() for t in (o, d, cam))
        far_ = far.detach().float().reshape(N).contiguous()
        act = torch.empty(M, act_ld, device=dev, dtype=torch.bfloat16)
        mask = torch.empty(8, M, 2, 4, device=dev, dtype=torch.int32)
        mask_v = torch.empty(M, 2, 2, device=dev, dtype=torch.int32)
        raw = torch.empty(M, 4, device=dev)
        aux = torch.empty(N, 32, device=dev)
        sky = torch.empty(N, 3, device=dev)
        tv = _t_vals(dev)
        _lib.check(lib.ucn_sky_train_fwd(packed.data_ptr(), o_.data_ptr(), d_.data_ptr(), cam_.data_ptr(), far_.data_ptr(), tv.data_ptr(),
                                         N, aux.data_ptr(), raw.data_ptr(), act.data_ptr(), mask.data_ptr(), mask_v.data_ptr(),
                                         sky.data_ptr(), st))
        ctx.save_for_backward(packed, raw, d_, far_, act, mask, mask_v)
        ctx.meta = (N, act_ld, g_ld, tuple(t.dtype for t in (W0, b0, M5, Mv, wa, ba, Wr, br)))
        return sky

    @staticmethod
    def backward(ctx, g_sky):
        from .sky import _t_vals
        lib = _lib.load()
        packed, raw, d_, far_, act, mask, mask_v = ctx.saved_tensors
        N, act_ld, g_ld, dts = ctx.meta
        dev, M = act.device, act.shape[0]
        with torch.autocast("cuda", enabled=False):
            g = g_sky.reshape(N, 3).float().contiguous()
            g_raw = torch.empty(M, 4, device=dev)
            dl = torch.empty(M, g_ld, device=dev, dtype=torch.bfloat16)
            _lib.check(lib.ucn_sky_train_bwd(packed.data_ptr(), g.data_ptr(), raw.data_ptr(), d_.data_ptr(), far_.data_ptr(),
                                             _t_vals(dev).data_ptr(), N, mask.data_ptr(), mask_v.data_ptr(), g_raw.data_ptr(),
                                             dl.data_ptr(), _lib.stream()))
            AUX, HV = 2048, 2080
            aux = act[:, AUX:AUX + 32]
            G0 = wgrad(dl[:, 0:256], aux)                                                   # d0^T aux: [256, 32] = [dW0 (3) | db0 | .]
            out = {0: (G0[:, :3], G0[:, 3])}
            for l in (1, 2, 3, 4, 5, 6, 7):
                G = wgrad(dl[:, 256 * l:256 * (l + 1)], act[:, 256 * (l - 1):256 * l], aux)   # d_l^T [h_{l-1} | aux]: [256, 288]
                out[l] = G if l == 5 else (G[:, :256], G[:, 259])
            Gv = wgrad(dl[:, 2048:2048 + 160], act[:, 256 * 7:256 * 8], aux)                # [dv | g]^T [h7 | aux]: [160, 288]
            gMv, gwa, gba = Gv[:128], Gv[131:132, :256], Gv[131, 259].reshape(1)
            gbr = Gv[128:131, 259]
            gWr = wgrad(dl[:, 2048 + 128:2048 + 160], act[:, HV:HV + 128])[:3]              # g^T hv: [3, 128]
        w_dt, b_dt, m5_dt, mv_dt, wa_dt, ba_dt, wr_dt, br_dt = dts
        # (contiguous: these are column blocks of the weight-gradient kernel's [., 288] outputs; autograd's accumulation would
        #  clone a strided gradient anyway, and DistributedDataParallel's bucket views warn about the stride mismatch)
        c = lambda t, dt: t.to(dt).clone(memory_format=torch.contiguous_format)      # (clone: a [1, 256] view keeps its row stride through .contiguous())
        res = [None, None, None, None, c(out[0][0], w_dt), c(out[0][1], b_dt)]
        for l in (1, 2, 3, 4, 6, 7):
            res += [c(out[l][0], w_dt), c(out[l][1], b_dt)]
        res += [c(out[5], m5_dt), c(gMv, mv_dt), c(gwa, wa_dt), c(gba, ba_dt), c(gWr, wr_dt), c(gbr, br_dt)]
        return tuple(res)


def sky_forward_fused(net, origins, directions, cam_dirs, far):
    """sky_forward through the hand-written training kernels.  The two layers with 9 input tiles are handed over composed,
    formed HERE with differentiable torch ops (fp32) so that autograd maps their gradients back to the parameters:
        M5 = [W5[:, 3:] | W5[:, :3] | b5 | 0]                  (the skip layer, its input [pts, h] reordered to [h | pts, 1])
        Mv = [Wv[:, :256] Wf | 0 | bv + Wv[:, :256] bf | Wv[:, 256:] | 0]   (feature_linear has no activation behind it)"""
    P = net.pts_linears
    with torch.autocast("cuda", enabled=False):
        W5, b5 = P[5].weight.float(), P[5].bias.float()
        Wv, bv = net.views_linears[0].weight.float(), net.views_linears[0].bias.float()
        Wf, bf = net.feature_linear.weight.float(), net.feature_linear.bias.float()
        z = W5.new_zeros
        M5 = torch.cat([W5[:, 3:], W5[:, :3], b5[:, None], z(256, 28)], dim=1)
        Wvf = Wv[:, :256]
        lin = dense_f32.hip_linear                                    # (differentiable, csrc/gemm_f32.hip: no library GEMM, r06)
        Mv = torch.cat([lin(Wvf.contiguous(), Wf.t()), z(128, 3), (bv + lin(bf[None, :], Wvf)[0])[:, None], Wv[:, 256:], z(128, 1)], dim=1)
        args = [origins, directions, cam_dirs, far, P[0].weight, P[0].bias]
        for l in (1, 2, 3, 4, 6, 7):
            args += [P[l].weight, P[l].bias]
        args += [M5, Mv, net.alpha_linear.weight, net.alpha_linear.bias, net.rgb_linear.weight, net.rgb_linear.bias]
        return _SkyFused.apply(*args)


def _sky_fusable(net, origins):
    return (origins.is_cuda and torch.is_autocast_enabled() and torch.get_autocast_dtype('cuda') == torch.bfloat16
            and origins.shape[0] > 0 and all(p.dtype == torch.float32 for p in net.parameters()))


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


def march_train(model, rand, batch, train_frac, compute_extras, eval_camidx, glo_vec=None):
    """Model.forward with an autograd graph (ref models.py:97-365).  glo_vec [N, num_glo_features] (or None): the NeRF level's
    per-ray GLO codes (models.py:118-127); the proposal levels get none (models.py:226)."""
    lib = _lib.load()
    model.last_march_route = 'train_graph'
    rays = ml.Rays(batch, model.num_levels)
    N, dev, prefix = rays.N, rays.dev, rays.prefix
    o, d, vd, cam, far = rays.o, rays.d, rays.vd, rays.cam, rays.far
    st, cfg = _lib.stream(), model.config
    bg, opaque = float(model.bg_intensity_range[0]), int(bool(model.opaque_background))
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
    for i_level, is_prop, S, mlp, dilation in ml.level_plan(model):
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
        density, rgbs = field_heads(mlp, feat, vd, N, S, chan, glo)
        if getattr(cfg, 'brightness_correction', False):              # models.py:233-235 (gated on this flag)
            rgbs, density = GradientScaler.apply(rgbs, density, tmean)
        weights, c_rgb, c_depth, c_acc = _Composite.apply(density, rgbs, posts, d, bg, opaque)
        extras = None
        if compute_extras:
            # render.py:218-242: depth percentiles and the mean distance -- not differentiated by any loss of the path
            # (train_utils.py reads them for metrics only), so they come from the rendering kernel on detached inputs
            with torch.no_grad():
                dn, rg = density.detach().float().contiguous(), rgbs.detach().float().contiguous()
                w_x, main_x, extras = torch.empty(N, S, device=dev), torch.empty(N, 5, device=dev), torch.empty(N, 4, device=dev)
                _lib.check(posts.entry(lib, 'ucn_composite')(dn.data_ptr(), rg.data_ptr(), *posts.compositing(), d.data_ptr(), bg,
                                                             opaque, N, S, w_x.data_ptr(), main_x.data_ptr(), extras.data_ptr(), st))
        renderings.append(ml.rendering_entry(c_rgb, c_depth, c_acc, weights, extras, prefix, posts.sdist, rgbs, getattr(cfg, 'vis_num_rays', 16)))
        hist = ml.history_entry(coord, density, rgbs, posts.sdist, weights, prefix)
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
