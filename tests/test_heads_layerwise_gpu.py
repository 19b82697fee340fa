"""ucn_train_fwd / ucn_train_bwd (csrc/field_train.hip) and ucn_sky_train_fwd / ucn_sky_train_bwd (csrc/sky_train.hip) held to float64
LAYER BY LAYER through the C ABI: every tensor the kernels store is compared, element by element, with the float64 layer formed from the
tensor they stored in front of it (heads_layerwise_ref.py; the bound is derived there and proven on a CPU emulation by
test_heads_layerwise_cpu.py).  Every output is allocated with extra rows behind a NaN / sentinel pattern that must survive."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import heads_layerwise_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu
BF, PAD, SENT = torch.bfloat16, 40, 0x5A5A5A5A
REPORT = H.Report()


def _nan(rows, cols, dtype=BF):
    return torch.full((rows, cols), float("nan"), device="cuda", dtype=dtype)


def _untouched(t, what):
    assert bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t == SENT).all()), f"{what}: written outside its rows / blocks"


@functools.lru_cache(maxsize=None)
def _field_setup(F, seed):
    from ucnerf_amd.internal import dense_f32
    from ucnerf_amd.internal.head_pack import prepare_heads
    P = H.field_params(F, seed)
    Pc = {k: v.cuda() for k, v in P.items()}
    packed, packed_t, _, _, b0a, b1a, bra = prepare_heads(*(Pc[k] for k in ("Wd0", "bd0", "Wd1", "bd1", "W0", "b0", "W1", "b1", "Wr", "br")))
    Wd1t = Pc["Wd1"].t().contiguous()
    composed = tuple(dense_f32.gemm(w.contiguous(), Wd1t).cpu() for w in (Pc["W0"][:, :256], Pc["W1"][:, 256:512]))
    exact = ((P["W0"][:, :256].double() @ P["Wd1"].double()), (P["W1"][:, 256:512].double() @ P["Wd1"].double()))
    for c, e in zip(composed, exact):                         # the host's fp32 composition is the fp32 GEMM of the float64 one
        assert float((c.double() - e).abs().max()) <= 65 * H.U32 * float(e.abs().max())
    bias = dict(bd0=H.from_acc(b0a.cpu(), 64), bd1=H.from_acc(b1a.cpu(), 256), br=H.from_acc(bra.cpu(), 32)[:3])
    for k, v in bias.items():                                 # prepare_heads rounds the biases to bf16
        assert torch.equal(v.double(), H.rb(P[k])), k
    return P, H.field_weights(P, composed), packed, packed_t, (b0a.contiguous(), b1a.contiguous(), bra.contiguous()), bias


def run_field(c, x_null=False, side=True, split=None, pr_rows=None):
    """One forward (+ the head = NULL forward for the logits) and one backward of case c -> (inp, out) on the CPU."""
    from ucnerf_amd import _lib
    lib = _lib.load()
    (N, S), F = split or (c["N"], c["S"]), c["F"]
    seed = H.case_seed(c)
    P, Wb, packed, packed_t, (b0a, b1a, bra), bias = _field_setup(F, seed)
    inp = H.field_inputs(c["N"], c["S"], F, seed, head=c["head"], graw=c["graw"])
    inp.update(bias, lm=c["lm"], S=S, N=N)
    if pr_rows is not None:                                   # the same per-ray terms for every ray: any N x S split is the same problem
        inp["pr0"], inp["pr1"] = inp["pr0"][:1].expand(N, -1).contiguous(), inp["pr1"][:1].expand(N, -1).contiguous()
        inp["ray_cols"] = inp["ray_cols"][:1].expand(N, -1).contiguous()
    M = N * S
    assert M == c["N"] * c["S"]
    feat = inp["feat"].cuda()

    def per_ray(v):                                           # accumulator order; off by 4 bytes = the entry point takes the non-SIDE route
        a = H.to_acc(v, 256).reshape(-1)
        buf = torch.zeros(a.numel() + 4, device="cuda")
        view = buf[0 if side else 1:][:a.numel()]
        view.copy_(a)
        assert (view.data_ptr() % 16 == 0) == side
        return buf, view
    k0, pr0 = per_ray(inp["pr0"])
    k1, pr1 = per_ray(inp["pr1"])
    ld = c["act_ld"]
    rows = M + PAD
    if ld:
        act = _nan(rows, ld)
        blk = {k: act[:, lo:hi] for k, (lo, hi) in H.ACT_BLOCKS.items()}
    else:
        blk = dict(h0=_nan(rows, 64), x=_nan(rows, 256), h1=_nan(rows, 256), h2=_nan(rows, 256), fb=_nan(rows, F))
    use_fb = F % 8 == 0
    use_rc = c["ray_cols"]
    rc = inp["ray_cols"].cuda() if use_rc else None
    hd = (ctypes.c_float * 4)(*inp["head"]) if inp["head"] is not None else None
    st = _lib.stream()
    fwd = {}
    for head in ([None, hd] if hd is not None else [None]):
        for t in ([act] if ld else list(blk.values())):
            t.fill_(float("nan"))
        raw, y = _nan(rows, 1, torch.float32), _nan(rows, 3, torch.float32)
        m0 = torch.full((rows, 2), SENT, device="cuda", dtype=torch.int32)
        m1, m2 = (torch.full((rows, 2, 4), SENT, device="cuda", dtype=torch.int32) for _ in range(2))
        _lib.check(lib.ucn_train_fwd(feat.data_ptr(), F, packed.data_ptr(), b0a.data_ptr(), b1a.data_ptr(), bra.data_ptr(), pr0.data_ptr(),
                                     pr1.data_ptr(), N, S, blk["h0"].data_ptr(), None if x_null else blk["x"].data_ptr(), blk["h1"].data_ptr(),
                                     blk["h2"].data_ptr(), ld, _lib.ptr(rc), blk["aux"].data_ptr() if use_rc else None,
                                     blk["fb"].data_ptr() if use_fb else None, head, raw.data_ptr(), y.data_ptr(), m0.data_ptr(),
                                     m1.data_ptr(), m2.data_ptr(), 0, st))
        torch.cuda.synchronize()
        for t, what in ((raw, "raw"), (y, "y"), (m0, "m0"), (m1, "m1"), (m2, "m2")):
            _untouched(t[M:], what)
        if ld:
            _untouched(act[M:], "activation rows")
            written = [(0, 512), (800, 864)] + ([] if x_null else [(512, 768)]) + ([(768, 800)] if use_rc else []) + ([(864, 864 + F)] if use_fb else [])
            keep = torch.ones(ld, dtype=torch.bool)
            for lo, hi in written:
                keep[lo:hi] = False
            _untouched(act[:M][:, keep.cuda()], "activation columns outside the documented blocks")
        else:
            for k, t in blk.items():
                _untouched(t[M:], k)
                if (k == "fb" and not use_fb) or (k == "x" and x_null):
                    _untouched(t, k)
        cur = dict(h0=blk["h0"][:M], h1=blk["h1"][:M], h2=blk["h2"][:M], m0=m0[:M], m1=m1[:M], m2=m2[:M])
        if not x_null:
            cur["x"] = blk["x"][:M]
        if use_fb:
            cur["feat_bf16"] = blk["fb"][:M, :F]
        if use_rc:
            cur["ray_dst"] = blk["aux"][:M]
        cur = {k: v.cpu().clone() for k, v in cur.items()}
        if head is None:
            fwd = dict(cur, raw=raw[:M, 0].cpu(), y=y[:M].cpu())
        else:
            for k, v in cur.items():                          # the head only changes what raw / y hold
                assert torch.equal(v.view(torch.int16) if v.dtype == BF else v, fwd[k].view(torch.int16) if v.dtype == BF else fwd[k]), k
            fwd.update(density=raw[:M, 0].cpu(), rgb=y[:M].cpu())
            dens_dev, rgb_dev = raw[:M, 0].contiguous(), y[:M].contiguous()
    if use_rc:
        assert torch.equal(fwd["ray_dst"].view(torch.int16), inp["ray_cols"][torch.arange(M) // S].view(torch.int16)), "ray_dst block"
    # ---- backward
    gy, graw = inp["gy"].cuda().contiguous(), (inp["graw"].cuda().contiguous() if inp["graw"] is not None else None)
    dyl = c["dy_ld"] or 4
    d1, d0, gx, gh0 = _nan(rows, 256), _nan(rows, 256), _nan(rows, 256), _nan(rows, 64)
    dy = _nan(rows, dyl)
    dy[:M] = 0                                                # the caller's zero-filled tile; the kernel writes columns 0 .. 3
    gfeat = _nan(rows * F, 1, torch.float32)
    m0, m1, m2 = (fwd[k].cuda() for k in ("m0", "m1", "m2"))
    flag = {0: 0, 1: _lib.GFEAT_LEVEL_MAJOR, 2: _lib.GFEAT_LEVEL_MAJOR4}[c["lm"]]
    _lib.check(lib.ucn_train_bwd(gy.data_ptr(), _lib.ptr(graw), hd, dens_dev.data_ptr() if hd is not None else None,
                                 rgb_dev.data_ptr() if hd is not None else None, packed_t.data_ptr(), m0.data_ptr(), m1.data_ptr(), m2.data_ptr(),
                                 N, S, F | flag, d1.data_ptr(), d0.data_ptr(), None if x_null else gx.data_ptr(), gh0.data_ptr(), dy.data_ptr(),
                                 c["dy_ld"], gfeat.data_ptr(), st))
    torch.cuda.synchronize()
    for t, what in ((d1, "d1"), (d0, "d0"), (gx, "gx"), (gh0, "gh0"), (dy, "dy")):
        _untouched(t[M:], what)
    if x_null:
        _untouched(gx, "gx = NULL")
    _untouched(gfeat[M * F:], "gfeat")
    assert bool((dy[:M, 4:] == 0).all())
    out = dict(fwd, d1=d1[:M].cpu(), d0=d0[:M].cpu(), gh0=gh0[:M].cpu(), dy=dy[:M].cpu(), gfeat=gfeat[:M * F, 0].cpu() if c["lm"] else gfeat[:M * F, 0].reshape(M, F).cpu())
    if not x_null:
        out["gx"] = gx[:M].cpu()
    return inp, out, Wb


@functools.lru_cache(maxsize=None)
def judged_field(i):
    c = H.field_cases()[i]
    inp, out, Wb = run_field(c)
    rep = H.Report()
    for r in (rep, REPORT):
        H.field_forward_check(r, H.case_id(c), Wb, inp, out)
        H.field_backward_check(r, H.case_id(c), Wb, inp, out)
    return rep


@pytest.mark.parametrize("i", range(len(H.field_cases())), ids=[H.case_id(c) for c in H.field_cases()])
def test_field_kernels_layer_by_layer(i):
    rep = judged_field(i)
    print(rep.text())
    assert not rep.failures(), rep.failures()


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t


def _same(a, b, skip=()):
    for k in a:
        if k in b and k not in skip:
            assert torch.equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize("N,S", [(2, 32), (3, 96)])
def test_side_route_equals_the_global_route(N, S):
    """EXACT: both routes start each accumulator from the same fp32 values (LDS side table against global loads) and run the same MFMAs."""
    c = dict(H.BASE, N=N, S=S, F=32)
    _same(run_field(c, side=True)[1], run_field(c, side=False)[1])


@pytest.mark.parametrize("N,S,F", [(3, 96, 32), (5, 100, 40)])
def test_null_x_and_gx_change_nothing_else(N, S, F):
    """EXACT: x / gx are stores only; two runs of the stored form are bit-identical as well."""
    c = dict(H.BASE, N=N, S=S, F=F)
    a, b, lean = run_field(c)[1], run_field(c)[1], run_field(c, x_null=True)[1]
    _same(a, b)
    _same(a, lean)
    assert "x" not in lean and "gx" not in lean


def test_the_same_rows_under_different_ray_splits():
    """EXACT: 96 rows as 3 x 32 (SIDE), 1 x 96 (SIDE) and 2 x 48 (waves spanning two rays) with every ray's terms the same."""
    c = dict(H.BASE, N=3, S=32, F=32)
    outs = [run_field(c, split=s, pr_rows=1)[1] for s in ((3, 32), (1, 96), (2, 48))]
    _same(outs[0], outs[1])
    _same(outs[0], outs[2])


# ------------------------------------------------------------------ sky
@functools.lru_cache(maxsize=None)
def run_sky(N):
    from ucnerf_amd import _lib
    lib = _lib.load()
    P = H.sky_params(7)
    inp = H.sky_inputs(N, P, 8)
    M = N * H.SKY_S
    dev = {k: [t.cuda().contiguous() for t in v] if isinstance(v, list) else v.cuda().contiguous() for k, v in P.items()}
    desc = _lib.UcnSkyTrain()
    for l in (0, 1, 2, 3, 4, 6, 7):
        desc.w_pts[l], desc.b_pts[l] = dev["W"][l].data_ptr(), dev["b"][l].data_ptr()
    desc.m5, desc.mv = dev["m5"].data_ptr(), dev["mv"].data_ptr()
    desc.w_alpha, desc.b_alpha, desc.w_rgb, desc.b_rgb = (dev[k].data_ptr() for k in ("wa", "ba", "wr", "br"))
    packed = torch.empty(lib.ucn_sky_train_packed_bytes(), dtype=torch.uint8, device="cuda")
    desc.packed = packed.data_ptr()
    st = _lib.stream()
    _lib.check(lib.ucn_sky_train_pack(ctypes.byref(desc), st))
    ld, gld = lib.ucn_sky_train_act_ld(), lib.ucn_sky_train_grad_ld()
    assert ld == H.SKY_LD == gld
    o, d, cam, far, tv, g_sky = (inp[k].cuda().contiguous() for k in ("o", "d", "cam", "far", "tv", "g_sky"))
    rows = M + PAD
    runs = []
    for _ in range(2):
        act, grad = _nan(rows, ld), _nan(rows, gld)
        mask = torch.full((8 * M * 8 + 64,), SENT, device="cuda", dtype=torch.int32)
        mask_v = torch.full((rows, 2, 2), SENT, device="cuda", dtype=torch.int32)
        raw, g_raw = _nan(rows, 4, torch.float32), _nan(rows, 4, torch.float32)
        aux, sky = _nan(N + 2, 32, torch.float32), _nan(N + 2, 3, torch.float32)
        _lib.check(lib.ucn_sky_train_fwd(packed.data_ptr(), o.data_ptr(), d.data_ptr(), cam.data_ptr(), far.data_ptr(), tv.data_ptr(), N,
                                         aux.data_ptr(), raw.data_ptr(), act.data_ptr(), mask.data_ptr(), mask_v.data_ptr(), sky.data_ptr(), st))
        _lib.check(lib.ucn_sky_train_bwd(packed.data_ptr(), g_sky.data_ptr(), raw.data_ptr(), d.data_ptr(), far.data_ptr(), tv.data_ptr(), N,
                                         mask.data_ptr(), mask_v.data_ptr(), g_raw.data_ptr(), grad.data_ptr(), st))
        torch.cuda.synchronize()
        for t, what in ((act[M:], "act rows"), (grad[M:], "grad rows"), (act[:M, 2208:], "act pad"), (grad[:M, 2208:], "grad pad"), (mask[8 * M * 8:], "mask"),
                        (mask_v[M:], "mask_v"), (raw[M:], "raw"), (g_raw[M:], "g_raw"), (aux[N:], "aux"), (sky[N:], "sky_rgb")):
            _untouched(t, what)
        runs.append(dict(act=act[:M, :2208].cpu(), grad=grad[:M, :2208].cpu(), raw=raw[:M].cpu(), g_raw=g_raw[:M].cpu(), sky_rgb=sky[:N].cpu(),
                         mask=mask[:8 * M * 8].reshape(8, M, 2, 4).cpu(), mask_v=mask_v[:M].cpu()))
    _same(runs[0], runs[1])                                    # two runs bit-identical
    out = runs[0]
    pad = lambda t: torch.cat([t, torch.zeros(M, H.SKY_LD - t.shape[1], dtype=t.dtype)], dim=1)
    out["act"], out["grad"] = pad(out["act"]), pad(out["grad"])
    rep = H.Report()
    for r in (rep, REPORT):
        H.sky_forward_check(r, f"sky N={N}", P, inp, out)
        H.sky_backward_check(r, f"sky N={N}", P, inp, out)
    return rep, inp, out


@pytest.mark.parametrize("N", H.SKY_RAYS)
def test_sky_kernels_layer_by_layer(N):
    rep, inp, out = run_sky(N)
    print(rep.text())
    assert not rep.failures(), rep.failures()
    if N >= 3:
        raw = out["raw"].reshape(N, H.SKY_S, 4)
        assert float(raw[1, :, 3].max()) < 0 and float(out["sky_rgb"][1].abs().max()) == 0      # all-zero alpha
        assert float(out["g_raw"].reshape(N, H.SKY_S, 4)[1].abs().max()) == 0
        assert float(raw[2, 0, 3]) > 1.0 and bool(torch.isfinite(out["sky_rgb"]).all()) and bool(torch.isfinite(out["g_raw"]).all())


def test_activation_and_compositing_errors_and_the_report():
    """softplus / padded sigmoid and the sky compositing forward / backward against float64 on the kernel's own logits / raw: within 4 x
    the error of a float32 torch-CPU evaluation of the same formula, pooled over every case (worst against worst).  Writes the report
    when UCN_HEADS_LAYERWISE_REPORT names a file."""
    for i in range(len(H.field_cases())):
        judged_field(i)
    for N in H.SKY_RAYS:
        run_sky(N)
    text = REPORT.text()
    print(text)
    path = os.environ.get("UCN_HEADS_LAYERWISE_REPORT")
    if path:
        with open(path, "w") as f:
            f.write(text)
    assert not REPORT.failures(), REPORT.failures()
    assert set(REPORT.measured) >= {"field fwd density", "field fwd rgb", "sky fwd sky_rgb", "sky bwd g_raw d logits", "sky bwd g_raw d sigma"}
    for what, (ref, got) in REPORT.measured.items():
        assert got <= 4 * ref, (what, ref, got)
