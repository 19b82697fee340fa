"""The fields' dense layers under bf16 autocast on the hand-written MFMA kernels: `_FusedHeads` (csrc/field_train.hip + csrc/wgrad.hip),
`_PropHeads` (csrc/prop_train.hip) and the weight-gradient helpers over the bf16 activation buffer."""
import ctypes
import os

import torch

from .. import _lib
from . import dense_f32
from .head_pack import _ACT_AUX, _ACT_FB, _ACT_H0, _ACT_H1, _ACT_H2, _ACT_X, ACT_LD, prepare_heads
from .heads_f32 import split_k


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
    ws = dense_f32.stream_workspace(n, A.device, "bf16")
    out = torch.empty(KA, kb1 + kb2, device=A.device)
    _lib.check(lib.ucn_wgrad_bf16(A.data_ptr(), A.stride(0), KA, B1.data_ptr(), B1.stride(0), kb1, _lib.ptr(B2),
                                  0 if B2 is None else B2.stride(0), kb2, M, ws.data_ptr(), out.data_ptr(), _lib.stream()))
    return out


def _wgrad_cols(gy, act, lo, hi):
    """gy^T @ act[:, lo:hi] as float32 [gy columns, hi - lo]: split-K batched GEMM over 8192-row chunks on a strided
    column view of the activation buffer (no copy; see _TallLinear for why the reduction is cut)."""
    k = split_k(gy.shape[0])
    if k:
        return torch.bmm(gy.reshape(k, -1, gy.shape[1]).transpose(1, 2), act.reshape(k, -1, act.shape[1])[:, :, lo:hi]).float().sum(0)
    return (gy.t() @ act[:, lo:hi]).float()


def _colsum(g):
    """Column sums of a tall [M, a] matrix as float32 [a]: a batched ones-row GEMM over 8192-row chunks (an fp32 copy +
    reduce_kernel over [1M, 3] costs 0.35 ms; this is 0.06 ms)."""
    k = split_k(g.shape[0])
    if k:
        return torch.bmm(g.new_ones(k, 1, g.shape[0] // k), g.reshape(k, -1, g.shape[1])).float().sum(dim=(0, 1))
    return g.float().sum(0)


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
