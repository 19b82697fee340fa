"""The fields' dense layers outside the fused bf16 kernels (train_graph.heads_route picks): `_TallLinear` (library GEMMs under autocast,
split-K weight gradients), `_ColourMLP` / `_ColourMLPGlo` (the colour layers as one node), `_ColourMLPComposed` / `_FieldMLPComposed` (fp32,
the bottleneck composed into the colour layers, csrc/gemm_f32.hip)."""
import torch
import torch.nn.functional as F

from .. import _lib
from . import dense_f32


CHUNK = 8192


def split_k(m):
    """Into how many CHUNK-row pieces the reduction over m rows of a library weight-gradient GEMM is cut (they run as one batched
    GEMM and are summed afterwards, see _TallLinear); None: m is short or no whole number of chunks, one GEMM."""
    return m // CHUNK if m >= 4 * CHUNK and m % CHUNK == 0 else None


class _TallLinear(torch.autograd.Function):
    """x @ weight.T (+ bias | + acc) for a tall activation matrix [M ~ 1e6, K] and a small weight [N <= 256, K].

    * The library's weight-gradient GEMM dY^T X (N x K output, reduction over the M samples) gets a single
      64x64 macro-tile grid -- 36 workgroups on a 256-CU part, 1.75 ms per call -- because nothing splits the
      reduction.  Here the reduction is cut into chunks that run as one batched GEMM and are summed afterwards
      (the same addends in a different order; fp32 accumulation inside each chunk and across chunks).
    * The bias gradient (column sums of dY) is a batched ones-row GEMM over the same chunks instead of an fp32
      copy of dY plus a reduction kernel.
    * `extra` is either a bias [N] or an accumulator [M, N] (the partial sum of another GEMM of the same layer:
      the concatenations of the reference's colour MLP are never materialised, see train_graph.field_heads)."""

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
            chunked = split_k(x2.shape[0])
            if chunked:
                gyc = gy2.reshape(chunked, -1, gy2.shape[1])
            if gy2.shape[1] == 1:
                # a single output row (PropMLP's density head): every library route for it (bmm with one row, mv)
                # takes an 11 ms HOST-side path in bf16 on this stack, which made the whole step CPU-bound
                gw = (gy2 * x2).float().sum(0, keepdim=True)
            elif chunked:
                gw = torch.bmm(gyc.transpose(1, 2), x2.reshape(chunked, -1, x2.shape[1])).float().sum(0)
            else:
                gw = (gy2.t() @ x2).float()
            if e_dt is None:
                ge = None
            elif ctx.extra_is_acc:
                ge = gy2.to(e_dt)
            elif chunked:
                ge = torch.bmm(gy2.new_ones(chunked, 1, gyc.shape[1]), gyc).float().sum(dim=(0, 1)).to(e_dt)
            else:
                ge = gy2.float().sum(0).to(e_dt)
        return gx, gw.to(w_dt), ge, None


def tall_affine(x, weight, bias, grad_t=False, relu=False):
    """x @ weight.T + bias (+ ReLU) through _TallLinear (autocast: operands in bf16 like F.linear under autocast), on the fp32 step through the
    hand-written fp32 MFMA GEMMs (csrc/gemm_f32.hip), else F.linear: the ONE place that picks among the three.  weight / bias need not be
    parameters (a stack of several heads' rows).  grad_t, relu: see `tall_linear`."""
    if torch.is_autocast_enabled():
        y = _TallLinear.apply(x, weight, bias, grad_t)
        return F.relu(y) if relu else y
    if dense_f32.usable(x, weight):               # the fp32 step (train_waymo.sh:3)
        return dense_f32.hip_linear(x, weight, bias, relu=relu)
    y = F.linear(x, weight, bias)
    return F.relu(y) if relu else y


def tall_linear(lin, x, grad_t=False, relu=False):
    """nn.Linear `lin` (+ ReLU) applied through `tall_affine`.
    grad_t: the input gradient comes back as the transpose of a contiguous [K, M] matrix (for _FieldFeatures).
    relu: on the fp32 route the ReLU is the GEMM's epilogue (and its output keeps the recorded maximum the next product scales by:
    the waymo.gin proposal level -- 1.9 M rows x 64 -- paid an elementwise pass and an amax pass for a separate F.relu)."""
    return tall_affine(x, lin.weight, lin.bias, grad_t, relu)


def tall_matmul(x, weight, acc=None):
    """x @ weight.T (+ acc [M, N]) through _TallLinear under autocast."""
    if torch.is_autocast_enabled():
        return _TallLinear.apply(x, weight, acc)
    y = dense_f32.hip_linear(x, weight) if dense_f32.usable(x, weight) else x @ weight.t()
    return y if acc is None else y + acc


def _wgrad(gy, x):
    """gy^T @ x for tall operands [M, a], [M, b] -> [a, b] float32, the reduction over M cut into batched chunks
    (see _TallLinear)."""
    k = split_k(x.shape[0])
    if k:
        return torch.bmm(gy.reshape(k, -1, gy.shape[1]).transpose(1, 2), x.reshape(k, -1, x.shape[1])).float().sum(0)
    return (gy.t() @ x).float()


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
