"""The sky NeRF of a training step (models.py:326-337, :743-904): `sky_forward` (fp32: one node over csrc/gemm_f32.hip, or eager layers)
and `sky_forward_fused` (bf16 autocast: csrc/sky_train.hip + csrc/wgrad.hip).  Rendering uses csrc/sky.hip (sky.py)."""
import ctypes
import os

import torch
import torch.nn.functional as F

from .. import _lib
from . import dense_f32
from .heads_bf16 import wgrad


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
