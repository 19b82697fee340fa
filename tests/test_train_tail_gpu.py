"""The HIP nodes that close a training step -- ucn_hash_decay, ucn_affine_blend, ucn_data_loss(_ex), ucn_sky_loss,
ucn_identity_loss (csrc/heads_train.hip), ucn_adam_step(_many), ucn_nan_to_num_many (csrc/train_ops.hip) -- through the C ABI
against the float64 restatement of tests/train_tail_ref.py, at the shapes and edges where such kernels go wrong.

Every output and workspace is pre-filled with NaN, every buffer is PAD elements longer than the length passed and the spare
elements are checked afterwards.  Bars: a rounding count next to the kernel expression it counts (train_tail_ref.ROUNDINGS)
times the float64 sum of absolute terms, or helpers.bracket with k = 2, its default floors and a min_ref; none is taken from
what a kernel returns, and tests/test_train_tail_cpu.py holds the float32 eager forms to the same bars on the same inputs.
`pytest -s` prints the report lines of profiles/train_tail/report.txt."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
import train_tail_ref as R
from train_tail_ref import PAD, U32, U64, gamma

pytestmark = pytest.mark.gpu
NAN = float("nan")
POISON = 7.25


def _lib():
    from ucnerf_amd import _lib as L
    return L, L.load(), L.stream()


def put(t, fill=NAN):
    """device copy of a host tensor, flat, with PAD spare elements of `fill` behind it"""
    buf = torch.full((t.numel() + PAD,), fill, dtype=t.dtype, device="cuda")
    buf[:t.numel()] = t.reshape(-1).cuda()
    return buf


def blank(n, fill=NAN, dtype=torch.float32):
    return torch.full((n + PAD,), fill, dtype=dtype, device="cuda")


def spare_ok(buf, n, fill=NAN):
    tail = buf[n:].cpu()
    return bool(torch.isnan(tail).all()) if fill != fill else bool((tail == fill).all())


def untouched(buf, fill=NAN):
    return spare_ok(buf, 0, fill)


def ptrs(bufs):
    return (ctypes.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs])


def floats(vals):
    return (ctypes.c_float * len(vals))(*vals)


def within(name, got, want, bar, note="", quiet=False):
    """|got - want| <= bar element by element; prints the largest share of the bar used"""
    got = torch.as_tensor(got).detach().cpu().double().reshape(-1)
    want, bar = torch.as_tensor(want, dtype=torch.float64).reshape(-1), torch.as_tensor(bar, dtype=torch.float64).reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), (name, "an element was not written or is not finite", int((~torch.isfinite(got)).sum()))
    diff = (got - want).abs()
    share = float((diff / bar.clamp_min(1e-300)).max()) if diff.numel() else 0.0
    if not quiet:
        print(f"TAIL {name}: max |hip - float64| {float(diff.max()) if diff.numel() else 0.0:.3e}, largest share of the derived bar {share:.3f} {note}")
    bad = diff > bar
    assert not bool(bad.any()), (name, int(bad.sum()), float(diff.max()), share)
    return share


# ================================================================== ucn_hash_decay
def _hash_forward(case):
    L_, lib, st = _lib()
    L, C, rows = R.HASH_CASES[case]
    emb, off = R.hash_inputs(case)
    e, out, ws = put(emb), blank(1), blank(1024)
    assert lib.ucn_hash_decay(e.data_ptr(), off.ctypes.data, L, C, None, out.data_ptr(), ws.data_ptr(), st) == 0, case
    assert bool(torch.isfinite(ws[:1024]).all().cpu()), (case, "a block left its partial unwritten")
    assert spare_ok(out, 1) and spare_ok(ws, 1024) and spare_ok(e, emb.numel())
    return emb, off, e, float(out[0].cpu())


@pytest.mark.parametrize("case", list(R.HASH_CASES))
def test_hash_decay_forward_bound_and_backward(case):
    L_, lib, st = _lib()
    L, C, rows = R.HASH_CASES[case]
    emb, off, e, val = _hash_forward(case)
    want = R.hash_decay(emb, rows)
    bound = R.hash_decay_fwd_bound(emb.numel(), L)
    print(f"TAIL ucn_hash_decay forward {case}: hip {val:.9e} float64 {want:.9e} rel {abs(val - want) / want:.3e} (derived bound {bound:.3e}, {emb.numel()} floats)")
    assert abs(val - want) <= bound * want, (case, val, want)
    for g in (1.0, -0.37):
        gd, grad = torch.tensor([g], device="cuda"), blank(emb.numel())
        assert lib.ucn_hash_decay(e.data_ptr(), off.ctypes.data, L, C, gd.data_ptr(), grad.data_ptr(), None, st) == 0
        gw = R.hash_decay_grad(emb, rows, np.float32(g))
        within(f"ucn_hash_decay backward {case} g={g}", grad[:emb.numel()], gw, gamma(R.ROUNDINGS["hash_decay_bwd"]) * gw.abs())
        assert spare_ok(grad, emb.numel())


def test_hash_decay_forward_bracket():
    """all cases as one vector: the host branch of hash_decay rounds a double sum once, so a single case's e_ref is one rounding"""
    e_ref, e_hip, truth = [], [], []
    for case, (L, C, rows) in R.HASH_CASES.items():
        emb, off, _, val = _hash_forward(case)
        want = R.hash_decay(emb, rows)
        e_ref.append(abs(float(R.eager_hash_decay(emb, off)) - want)); e_hip.append(abs(val - want)); truth.append(want)
    H.bracket("ucn_hash_decay forward, all cases", e_ref, e_hip, min_ref=R.min_ref(truth))


def test_hash_decay_refusals():
    L_, lib, st = _lib()
    emb = torch.rand(8, 2)
    e, out, ws, grad = put(emb), blank(1), blank(1024), blank(16)
    g = torch.ones(1, device="cuda")
    off = lambda *v: np.asarray(v, dtype=np.int32)
    o2, o33, oe = off(0, 3, 8), off(*range(34)), off(0, 3, 3, 8)
    assert lib.ucn_hash_decay(e.data_ptr(), o2.ctypes.data, 0, 2, None, out.data_ptr(), ws.data_ptr(), st) != 0, "L = 0"
    assert lib.ucn_hash_decay(e.data_ptr(), o33.ctypes.data, 33, 2, None, out.data_ptr(), ws.data_ptr(), st) != 0, "L = 33"
    assert lib.ucn_hash_decay(e.data_ptr(), oe.ctypes.data, 3, 2, None, out.data_ptr(), ws.data_ptr(), st) != 0, "an empty level"
    assert lib.ucn_hash_decay(e.data_ptr(), oe.ctypes.data, 3, 2, g.data_ptr(), grad.data_ptr(), None, st) != 0, "an empty level, backward"
    assert lib.ucn_hash_decay(e.data_ptr(), o2.ctypes.data, 2, 2, None, out.data_ptr(), None, st) != 0, "forward with a NULL workspace"
    torch.cuda.synchronize()
    assert untouched(out) and untouched(ws) and untouched(grad)


def test_hash_decay_node_under_autocast_and_on_the_host():
    from ucnerf_amd.internal import march_nodes as tg
    L_, lib, st = _lib()
    case = "L16_C8_geometric_5_to_3000"
    L, C, rows = R.HASH_CASES[case]
    emb, off, e, val = _hash_forward(case)
    grad = blank(emb.numel())
    assert lib.ucn_hash_decay(e.data_ptr(), off.ctypes.data, L, C, torch.ones(1, device="cuda").data_ptr(), grad.data_ptr(), None, st) == 0
    leaf = emb.cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        v = tg._HashDecay.apply(leaf, off)
    v.backward()
    assert v.dtype == torch.float32 and float(v) == val, "the node under autocast(bfloat16) returns the C ABI's value"
    assert torch.equal(leaf.grad.reshape(-1), grad[:emb.numel()]), "and its gradient"
    host, want = float(R.eager_hash_decay(emb, off)), R.hash_decay(emb, rows)
    assert abs(float(v) - host) <= (R.hash_decay_fwd_bound(emb.numel(), L) + U32) * want, (float(v), host)


# ================================================================== ucn_affine_blend
BLEND_GRADS = ("g_affine", "g_acc", "g_sky", "g_affine_sky")


@pytest.mark.parametrize("sky", [False, True], ids=["no_sky", "sky"])
@pytest.mark.parametrize("N", R.BLEND_N)
def test_affine_blend(N, sky):
    L_, lib, st = _lib()
    t = R.blend_inputs(N)
    dv = {k: put(v) for k, v in t.items()}
    opt_h = (t["acc"], t["sky"], t["A_sky"]) if sky else ()
    opt_d = [dv[k].data_ptr() if sky else None for k in ("acc", "sky", "A_sky")]
    tag = f"N={N} {'sky' if sky else 'no sky'}"
    out = blank(3 * N)
    assert lib.ucn_affine_blend(None, dv["rgb"].data_ptr(), dv["A"].data_ptr(), *opt_d, N, 0, out.data_ptr(), None, None, None, None, st) == 0
    want, mag = R.affine_blend_fwd(t["rgb"], t["A"], *opt_h)
    n = R.ROUNDINGS["blend_fwd_sky" if sky else "blend_fwd"]
    within(f"ucn_affine_blend forward {tag}", out[:3 * N], want, gamma(n) * mag, f"({n} roundings)")
    assert spare_ok(out, 3 * N)

    sizes = dict(g_rgb=3 * N, g_affine=12 * N, g_acc=N, g_sky=3 * N, g_affine_sky=12 * N)

    def backward(go, bufs, accumulate):
        return lib.ucn_affine_blend(dv[go].data_ptr(), dv["rgb"].data_ptr(), dv["A"].data_ptr(), *opt_d, N, accumulate,
                                    *[bufs[k].data_ptr() for k in ("g_rgb", "g_affine", "g_acc", "g_sky", "g_affine_sky")], st)
    # without a sky the three sky gradients are handed poisoned buffers: they must come back untouched
    bufs = {k: blank(n_, NAN if (sky or k in ("g_rgb", "g_affine")) else POISON) for k, n_ in sizes.items()}
    assert backward("g_out", bufs, 0) == 0
    ref = R.affine_blend_bwd(t["g_out"], t["rgb"], t["A"], *opt_h)
    for k, (val, mg) in ref.items():
        within(f"ucn_affine_blend backward {tag} {k}", bufs[k][:sizes[k]], val, gamma(R.ROUNDINGS[k]) * mg, f"({R.ROUNDINGS[k]} roundings)")
        assert spare_ok(bufs[k], sizes[k])
    if not sky:
        assert all(untouched(bufs[k], POISON) for k in ("g_acc", "g_sky", "g_affine_sky")), "no sky: the sky gradients are not written"

    # accumulate = 1, twice, into known values: prefill + both contributions; g_rgb is overwritten each time
    gen = torch.Generator().manual_seed(77 + N)
    pre = {k: torch.randn(sizes[k], generator=gen) for k in BLEND_GRADS}
    bufs = {k: (put(pre[k]) if (sky or k == "g_affine") else blank(sizes[k], POISON)) for k in BLEND_GRADS}
    bufs["g_rgb"] = blank(3 * N)
    assert backward("g_out", bufs, 1) == 0 and backward("g_out2", bufs, 1) == 0
    ref2 = R.affine_blend_bwd(t["g_out2"], t["rgb"], t["A"], *opt_h)
    within(f"ucn_affine_blend accumulate {tag} g_rgb (overwritten)", bufs["g_rgb"][:3 * N], ref2["g_rgb"][0], gamma(R.ROUNDINGS["g_rgb"]) * ref2["g_rgb"][1])
    for k in BLEND_GRADS:
        if k in ref:
            n = R.ROUNDINGS[k] + R.ROUNDINGS["accumulate"]
            want = pre[k].double() + ref[k][0].reshape(-1) + ref2[k][0].reshape(-1)
            mag = pre[k].double().abs() + ref[k][1].reshape(-1) + ref2[k][1].reshape(-1)
            within(f"ucn_affine_blend accumulate {tag} {k}", bufs[k][:sizes[k]], want, gamma(n) * mag, f"({n} roundings)")
            assert spare_ok(bufs[k], sizes[k])
        else:
            assert untouched(bufs[k], POISON), k
    for k in ("rgb", "A", "acc", "sky", "A_sky", "g_out"):
        assert torch.equal(dv[k][:t[k].numel()].cpu(), t[k].reshape(-1)) and spare_ok(dv[k], t[k].numel()), ("an input changed", k)


def test_affine_blend_refusals():
    L_, lib, st = _lib()
    t = R.blend_inputs(255)
    dv = {k: put(v) for k, v in t.items()}
    out, gA = blank(3 * 255), blank(12 * 255)
    a = lambda k: dv[k].data_ptr()
    assert lib.ucn_affine_blend(None, a("rgb"), a("A"), None, a("sky"), a("A_sky"), 255, 0, out.data_ptr(), None, None, None, None, st) != 0, "sky without acc"
    assert lib.ucn_affine_blend(a("g_out"), a("rgb"), a("A"), None, None, None, 255, 0, out.data_ptr(), None, None, None, None, st) != 0, "backward without g_affine"
    torch.cuda.synchronize()
    assert untouched(out) and untouched(gA)


# ================================================================== ucn_data_loss / ucn_data_loss_ex
def _data_call(lib, st, ex, lv, L, w, tgt, mult, N, fwd_out, g=None, grads=None):
    wm, wc, wr = (floats(x) for x in w)
    mp = None if mult is None else mult.data_ptr()
    gp, gl = (None, None) if g is None else (g.data_ptr(), ptrs(grads))
    if ex:
        return lib.ucn_data_loss_ex(ptrs(lv), L, wm, wc, wr, tgt.data_ptr(), mp, N, R.CHARB_PAD, fwd_out.data_ptr(), gp, gl, st)
    return lib.ucn_data_loss(ptrs(lv), L, wm, wc, tgt.data_ptr(), mp, N, R.CHARB_PAD, fwd_out.data_ptr(), gp, gl, st)


@pytest.mark.parametrize("with_mult", [False, True], ids=["lossmult_null", "lossmult"])
@pytest.mark.parametrize("N", R.DATA_N)
@pytest.mark.parametrize("L", R.DATA_L)
def test_data_loss(L, N, with_mult):
    L_, lib, st = _lib()
    levels, target, mult = R.data_inputs(L, N)
    mult = mult if with_mult else None
    lv, tgt, md = [put(x) for x in levels], put(target), (put(mult) if with_mult else None)          # exactly L level pointers
    seq = (3 * N + 1023) // 1024                                              # elements one of the 1024 threads adds
    e_ref, e_hip, truth = [], [], []
    for pattern in R.DATA_PATTERNS:
        tag = f"L={L} N={N} {'lossmult' if with_mult else 'lossmult NULL'} {pattern}"
        w = R.data_weights(pattern, L)
        out = blank(2 * L + 2)
        assert _data_call(lib, st, True, lv, L, w, tgt, md, N, out) == 0, tag
        res = out[:2 * L + 2].cpu().double()
        assert bool(torch.isfinite(res).all()) and spare_ok(out, 2 * L + 2), tag
        ref = R.data_loss(levels, target, mult, *w, R.CHARB_PAD)
        den_bar = R.sum_bound(seq, 0, 10)                                     # den: 1.0f or mult[i / 3] added as they are
        if pattern in R.FLOAT_PATTERNS:
            # k_data_loss_fwd: a += m * r2 (r, r2, the product: 3), c += m * sqrtf(r2 + pad2) (r, r2, the sum, pad2's own, sqrtf, the
            # product: 6); per thread `seq` adds, 10 tree levels, the division by den
            out2 = blank(2 * L + 2)
            assert _data_call(lib, st, False, lv, L, w, tgt, md, N, out2) == 0
            assert torch.equal(out2.cpu()[:2 * L + 2], out.cpu()[:2 * L + 2]), "ucn_data_loss is ucn_data_loss_ex with w_raw = NULL"
            stat_bar = R.sum_bound(seq, 6, 10, extra=1) + den_bar
            within(f"ucn_data_loss forward {tag} mse statistics", res[0:2 * L:2], ref["mses"], stat_bar * torch.tensor(ref["mses"], dtype=torch.float64))
            within(f"ucn_data_loss forward {tag} charb statistics", res[1:2 * L:2], ref["charbs"], stat_bar * torch.tensor(ref["charbs"], dtype=torch.float64))
            within(f"ucn_data_loss forward {tag} denominator", res[2 * L], ref["den"], den_bar * ref["den"])
            loss, mses, _ = R.eager_data_pattern(levels, target, mult, pattern)
            want = R.data_vector(ref["loss"], ref["mses"])
            e_ref.append((R.data_vector(loss, mses) - want).abs()); e_hip.append((R.data_vector(res[2 * L + 1], res[0:2 * L:2]) - want).abs())
            truth.append(want)
        else:
            # k_data_loss_fwd_raw: every sum in double -- up to 8 roundings to form a term, `seq` adds, 10 tree levels, the division,
            # the weighting and the per-level adds -- then ONE float32 rounding where it stores a float
            bar64 = gamma(8 + seq + 10 + 2 + 3 * L, U64) + U32
            within(f"ucn_data_loss_ex forward {tag} mse statistics", res[0:2 * L:2], ref["mses"], bar64 * torch.tensor(ref["mses"], dtype=torch.float64))
            charb = [ref["charbs"][l] if w[1][l] != 0 else 0.0 for l in range(L)]               # summed only where its weight is not 0
            within(f"ucn_data_loss_ex forward {tag} charb statistics", res[1:2 * L:2], charb, bar64 * torch.tensor(charb, dtype=torch.float64))
            within(f"ucn_data_loss_ex forward {tag} denominator", res[2 * L], ref["den"], bar64 * ref["den"])
            within(f"ucn_data_loss_ex forward {tag} loss", res[2 * L + 1], ref["loss"], bar64 * ref["loss"])
        for g in (1.0, 0.25):
            gd, grads = torch.tensor([g], device="cuda"), [blank(3 * N) for _ in range(L)]
            assert _data_call(lib, st, True, lv, L, w, tgt, md, N, out, gd, grads) == 0
            rb = R.data_loss(levels, target, mult, *w, R.CHARB_PAD, g=g, den=float(res[2 * L]))
            n = R.ROUNDINGS["data_bwd"]
            shares = []
            for l in range(L):
                got = grads[l][:3 * N]
                shares.append(within(f"ucn_data_loss_ex backward {tag} g={g} level {l}", got, rb["grads"][l], (gamma(n) + gamma(8, U64)) * rb["mags"][l], quiet=True))
                assert spare_ok(grads[l], 3 * N)
                x, tg_ = levels[l].view(-1), target.view(-1)
                same = (x == tg_).nonzero().view(-1)
                if pattern in ("charb_only", "mse_only") and same.numel():
                    assert bool((got.cpu()[same] == 0).all()), (tag, "rgb == target: gradient exactly 0")
                if pattern == "rawnerf_only" and N > 1:
                    above, one = (x > 1.0), (x == 1.0) & (torch.repeat_interleave(mult, 3) != 0 if mult is not None else True)
                    assert bool((got.cpu()[above] == 0).all()) and bool((got.cpu()[one] != 0).all()), (tag, "clamp gradient: 1 at the bound, 0 above")
            print(f"TAIL ucn_data_loss_ex backward {tag} g={g}: largest share of the derived bar over the levels {max(shares):.3f} ({n} roundings)")
        assert torch.equal(out[:2 * L + 2].cpu().double(), res), "the backward leaves the forward's record alone"
    e_ref, e_hip, truth = torch.cat(e_ref), torch.cat(e_hip), torch.cat(truth)
    H.bracket(f"k_data_loss_fwd L={L} N={N} {'lossmult' if with_mult else 'lossmult NULL'}: mse statistics and loss, charb_only + mse_only",
              e_ref, e_hip, min_ref=R.min_ref(truth))
    for b, x in zip(lv + [tgt], levels + [target]):
        assert torch.equal(b[:x.numel()].cpu(), x.reshape(-1)) and spare_ok(b, x.numel()), "an input changed"


def test_data_loss_refusals():
    L_, lib, st = _lib()
    levels, target, mult = R.data_inputs(4, 341)
    lv, tgt = [put(x) for x in levels] + [put(levels[0])], put(target)
    out, g = blank(12), torch.ones(1, device="cuda")
    w5 = ([0.0] * 5, [1.0] * 5, [0.0] * 5)
    assert _data_call(lib, st, True, lv[:1], 0, R.data_weights("charb_only", 1), tgt, None, 341, out) != 0, "L = 0"
    assert _data_call(lib, st, True, lv, 5, w5, tgt, None, 341, out) != 0, "L = 5"
    assert _data_call(lib, st, False, lv, 5, w5, tgt, None, 341, out) != 0, "L = 5, ucn_data_loss"
    wm, wc, wr = (floats(x) for x in R.data_weights("charb_only", 2))
    assert lib.ucn_data_loss_ex(ptrs(lv[:2]), 2, wm, wc, wr, tgt.data_ptr(), None, 341, R.CHARB_PAD, out.data_ptr(), g.data_ptr(), None, st) != 0, \
        "g without gradient pointers"
    torch.cuda.synchronize()
    assert untouched(out)


# ================================================================== ucn_sky_loss
@pytest.mark.parametrize("N", R.SKY_N)
def test_sky_loss(N):
    L_, lib, st = _lib()
    e_ref, e_hip, truth = [], [], []
    for L in R.SKY_L:
        for segs, seed in (("binary", 0), ("binary", 1), ("fractional", 2)):
            tag = f"L={L} N={N} {segs} sky_segs (draw {seed})"
            accs, s = R.sky_inputs(L, N, segs, seed)
            av, sv, out = [put(a) for a in accs], put(s), blank(1)
            assert lib.ucn_sky_loss(ptrs(av), L, sv.data_ptr(), N, out.data_ptr(), None, None, st) == 0, tag
            val = float(out[0].cpu())
            assert val == val and spare_ok(out, 1), tag
            gd, grads = torch.tensor([0.7], device="cuda"), [blank(N) for _ in range(L)]
            assert lib.ucn_sky_loss(ptrs(av), L, sv.data_ptr(), N, None, gd.data_ptr(), ptrs(grads), st) == 0, tag
            want, gw, mags = R.sky_loss(accs, s, g=np.float32(0.7))
            n = R.ROUNDINGS["sky_bwd"]
            shares = []
            for l in range(L):
                got = grads[l][:N].cpu()
                shares.append(within(f"ucn_sky_loss backward {tag} level {l}", got, gw[l], gamma(n) * mags[l], quiet=True))
                raw = accs[l].double()
                outside, on = (raw < R.CLIP_LO) | (raw > R.CLIP_HI), (raw == R.CLIP_LO) | (raw == R.CLIP_HI)
                assert bool((got[outside] == 0).all()), (tag, "0 outside the clip bounds")
                assert bool((got[on] != 0).all()), (tag, "the clip bounds are inside")
                assert spare_ok(grads[l], N) and spare_ok(av[l], N)
            print(f"TAIL ucn_sky_loss backward {tag}: largest share of the derived bar over the levels {max(shares):.3f} ({n} roundings)")
            e_ref.append(abs(float(R.eager_sky_loss(accs, s)[0]) - want)); e_hip.append(abs(val - want)); truth.append(want)
    H.bracket(f"k_sky_loss_fwd N={N}: L in (1, 4) x binary, binary, fractional sky_segs", e_ref, e_hip, min_ref=R.min_ref(truth))


# ================================================================== ucn_identity_loss
@pytest.mark.parametrize("sky", [False, True], ids=["no_sky", "sky"])
@pytest.mark.parametrize("N", R.IDENTITY_N)
def test_identity_loss(N, sky):
    L_, lib, st = _lib()
    A, B = R.identity_inputs(N)
    B = B if sky else None
    av, bv = put(A), (put(B) if sky else None)
    bp = bv.data_ptr() if sky else None
    out = blank(1, dtype=torch.float64)
    assert lib.ucn_identity_loss(av.data_ptr(), bp, N, out.data_ptr(), None, None, None, st) == 0
    want, _ = R.identity_loss(A, B)
    # k_identity_loss_fwd: s += fabs(eye - a) + fabs(eye - b) in double: up to 4 roundings per element (the two differences, the inner
    # sum, the add), ceil(12 N / 1024) elements per thread, 10 tree levels, the division
    n64 = 4 * ((12 * N + 1023) // 1024) + 10 + 1
    tag = f"N={N} {'with' if sky else 'without'} the sky map"
    within(f"ucn_identity_loss forward {tag}", out[:1], want, gamma(n64, U64) * want, f"({n64} double roundings)")
    assert spare_ok(out, 1)
    g = torch.tensor([0.3], dtype=torch.float64, device="cuda")
    gA, gB = blank(12 * N), blank(12 * N, NAN if sky else POISON)
    assert lib.ucn_identity_loss(av.data_ptr(), bp, N, None, g.data_ptr(), gA.data_ptr(), gB.data_ptr(), st) == 0
    _, eager = R.eager_identity_loss(A, B, g=0.3)                            # float64 eager form, its gradient cast to float32 by autograd
    equal = True
    for name, got, ref, M in (("affine", gA, eager[0], A),) + ((("affine_sky", gB, eager[1], B),) if sky else ()):
        got = got[:12 * N].cpu()
        assert bool(torch.isfinite(got).all()), name
        ulps = (got.double() - ref.reshape(-1).double()).abs() / torch.from_numpy(R.ulp32(ref.reshape(-1).numpy())).clamp_min(1e-300)
        assert float(ulps.max()) <= 1.0, (name, float(ulps.max()))
        equal = equal and torch.equal(got, ref.reshape(-1))
        on = (M == torch.eye(4)[:3].reshape(1, 12).expand(N, 12)).reshape(-1)
        assert int(on.sum()) >= 2 and bool((got[on] == 0).all()) and bool((got[~on] != 0).all()), (name, "gradient exactly 0 on the identity")
    print(f"TAIL ucn_identity_loss backward {tag}: within one float32 ulp of the float64 eager gradient, bit-equal: {equal}")
    assert spare_ok(gA, 12 * N) and (spare_ok(gB, 12 * N) if sky else untouched(gB, POISON))


# ================================================================== ucn_adam_step
def _adam(lib, st, bufs, n, step, sanitize):
    h = R.ADAM_HYPER
    return lib.ucn_adam_step(*[b if isinstance(b, int) or b is None else b.data_ptr() for b in bufs], n, h["lr"], h["betas"][0], h["betas"][1],
                             h["eps"], step, sanitize, st)


def _adam_check(name, hip, host, want, p, e_ref, e_hip, truth):
    """non-finite entries agree exactly with the host's; where the float32 second moment overflowed (+-FLT_MAX gradients) the
    parameter is the host's, bit for bit, and exp_avg within its two roundings of the float64 value; the rest goes to the bracket"""
    fin = R.adam_masks(host, hip)
    over = ~fin
    if bool(over.any()):
        assert torch.equal(hip[0][over], host[0][over]) and torch.equal(hip[0][over], p[over]), (name, "overflowed second moment: no update")
        assert bool(((hip[1].double() - want[1]).abs()[over] <= 2 * torch.from_numpy(R.ulp32(want[1].float().numpy()))[over]).all()), name
    for k in range(3):
        e_ref[k].append((host[k].double() - want[k]).abs()[fin]); e_hip[k].append((hip[k].double() - want[k]).abs()[fin])
        truth[k].append(want[k][fin])


@pytest.mark.parametrize("sanitize", [0, 1])
@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam_step(n, sanitize):
    L_, lib, st = _lib()
    for step in R.ADAM_STEPS:
        e_ref, e_hip, truth = [[], [], []], [[], [], []], [[], [], []]
        for seed in range(R.ADAM_SEEDS(n)):
            p, g, m, v = R.adam_inputs(n, seed, nonfinite=bool(sanitize))
            bufs = [put(x, POISON) for x in (p, g, m, v)]
            assert _adam(lib, st, bufs, n, step, sanitize) == 0
            hp, hg, hm, hv = (b.cpu() for b in bufs)
            assert all(bool((b[n:] == POISON).all()) for b in (hp, hg, hm, hv)), (n, step, "the elements after the n-th changed")
            if sanitize:
                assert torch.equal(hg[:n], torch.nan_to_num(g)), "the stored gradient is nan_to_num of the gradient"
            else:
                assert torch.equal(hg[:n].view(torch.int32), g.view(torch.int32)), "the gradient is untouched"
            want = R.adam_step(p, g, m, v, step=step, sanitize=bool(sanitize), **R.ADAM_HYPER)
            _adam_check(f"n={n} step={step}", (hp[:n], hm[:n], hv[:n]), R.eager_adam(p, g, m, v, step, sanitize), (want[0], want[2], want[3]), p,
                        e_ref, e_hip, truth)
        for k, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
            H.bracket(f"ucn_adam_step n={n} step={step} sanitize={sanitize} {name}", torch.cat(e_ref[k]), torch.cat(e_hip[k]),
                      min_ref=R.min_ref(torch.cat(truth[k])))


def test_adam_step_tail_element_has_the_bits_of_a_body_element():
    L_, lib, st = _lib()
    p, g, m, v = R.adam_inputs(4, 3, nonfinite=True)
    res = {}
    for n in (3, 4):                                                          # n = 3: all three in the tail loop; n = 4: one float4
        bufs = [put(x[:n], POISON) for x in (p, g, m, v)]
        assert _adam(lib, st, bufs, n, 2, 1) == 0
        res[n] = [b.cpu()[:3].view(torch.int32) for b in bufs]
    for a, b, name in zip(res[3], res[4], ("p", "grad", "exp_avg", "exp_avg_sq")):
        assert torch.equal(a, b), name


def test_adam_step_refusals():
    L_, lib, st = _lib()
    p, g, m, v = R.adam_inputs(64, 0)
    bufs = [put(x, POISON) for x in (p, g, m, v)]
    before = [b.clone() for b in bufs]
    assert _adam(lib, st, bufs, 64, 0, 1) != 0, "step = 0"
    assert _adam(lib, st, [bufs[0].data_ptr() + 4] + bufs[1:], 60, 1, 1) != 0, "a pointer offset by 4 bytes"
    assert _adam(lib, st, [bufs[0], None] + bufs[2:], 64, 1, 1) != 0, "a NULL pointer"
    assert _adam(lib, st, bufs, 0, 1, 1) == 0 and _adam(lib, st, [None] * 4, 0, 1, 1) == 0, "n = 0 returns 0"
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(bufs, before)), "and nothing was written"


# ================================================================== ucn_adam_step_many
BIG_MEMBER = 512 * 256 * 2 + 5                                              # more than 512 blocks x 256 threads: the grid-stride loop


@pytest.mark.parametrize("count", [0, 1, 24, 25, 49])
def test_adam_step_many(count):
    L_, lib, st = _lib()
    h, step = R.ADAM_HYPER, 7
    hyper = (h["lr"], h["betas"][0], h["betas"][1], h["eps"], step, 1, st)
    if count == 0:
        assert lib.ucn_adam_step_many(None, None, None, None, None, 0, *hyper) == 0
        return
    lens = [[0, 1, 5, 33, 1000, 7][i % 6] for i in range(count)]
    lens[{1: 0, 24: 3, 25: 24, 49: 48}[count]] = BIG_MEMBER                   # alone in the launch, inside the first chunk, in the second, the third
    assert 0 in lens or count == 1
    host_in = [R.adam_inputs(n, seed=i, nonfinite=True) if n else [torch.zeros(0)] * 4 for i, n in enumerate(lens)]
    # every member starts one float into its buffer: 4-byte aligned, not 16-byte aligned
    members = [[torch.full((n + 1 + PAD,), POISON, device="cuda") for _ in range(4)] for n in lens]
    for mem, src, n in zip(members, host_in, lens):
        for b, x in zip(mem, src):
            b[1:1 + n] = x.cuda()
            assert (b.data_ptr() + 4) % 16 == 4
    arr = lambda j: (ctypes.c_void_p * count)(*[mem[j].data_ptr() + 4 for mem in members])
    assert lib.ucn_adam_step_many(arr(0), arr(1), arr(2), arr(3), (ctypes.c_uint64 * count)(*lens), count, *hyper) == 0
    e_ref, e_hip, truth = [[], [], []], [[], [], []], [[], [], []]
    for i, (mem, src, n) in enumerate(zip(members, host_in, lens)):
        got = [b.cpu() for b in mem]
        assert all(float(b[0]) == POISON and bool((b[1 + n:] == POISON).all()) for b in got), (i, n, "a neighbour of the member changed")
        if n == 0:
            continue
        single = [put(x, POISON) for x in src]                                 # the same data, 16-byte aligned, through ucn_adam_step
        assert _adam(lib, st, single, n, step, 1) == 0
        for b, s, name in zip(got, single, ("p", "grad", "exp_avg", "exp_avg_sq")):
            assert torch.equal(b[1:1 + n].view(torch.int32), s.cpu()[:n].view(torch.int32)), (i, n, name, "not the bits of ucn_adam_step")
        p, g, m, v = src
        want = R.adam_step(p, g, m, v, step=step, sanitize=True, **h)
        _adam_check(f"member {i}", (got[0][1:1 + n], got[2][1:1 + n], got[3][1:1 + n]), R.eager_adam(p, g, m, v, step, 1), (want[0], want[2], want[3]),
                    p, e_ref, e_hip, truth)
    for k, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
        H.bracket(f"ucn_adam_step_many count={count} {name}", torch.cat(e_ref[k]), torch.cat(e_hip[k]), min_ref=R.min_ref(torch.cat(truth[k])))


# ================================================================== ucn_nan_to_num_many
def test_nan_to_num_many_long_member_and_empty_members():
    L_, lib, st = _lib()
    stride, n = 2048 * 1024, 2048 * 1024 + 7
    x = torch.randn(n, generator=torch.Generator().manual_seed(9))
    bad = [0, n - 1, stride - 1, stride, stride + 1] + [k * 2048 * 256 + o for k in (1, 2, 3) for o in (-1, 0, 1)]
    for j, i in enumerate(bad):
        x[i] = (NAN, float("inf"), float("-inf"))[j % 3]
    small = torch.tensor([NAN, 1.0, float("-inf")])
    bufs = [blank(0), put(x), blank(0), put(small)]                           # NaN behind every member: a write past the end turns it into 0
    lens = [0, n, 0, 3]
    assert lib.ucn_nan_to_num_many(None, None, 0, st) == 0, "count = 0"
    assert lib.ucn_nan_to_num_many(ptrs(bufs), (ctypes.c_uint64 * 4)(*lens), 4, st) == 0
    assert torch.equal(bufs[1].cpu()[:n], torch.nan_to_num(x)) and torch.equal(bufs[3].cpu()[:3], torch.nan_to_num(small))
    assert all(spare_ok(b, k) for b, k in zip(bufs, lens))


# ================================================================== an empty batch
def test_empty_batch_losses_are_the_eager_nan(monkeypatch):
    """N = 0: the C ABI returns without writing, so the three loss functions must take their eager branches, which return NaN like the
    reference; neither they nor their backward reach the library"""
    import types
    from ucnerf_amd.internal import train_utils as tu

    def boom():
        raise AssertionError("an empty batch reached the HIP library")
    dev = torch.device("cuda", 0)
    z = lambda *s: torch.zeros(*s, device=dev).requires_grad_(True)
    rend = [dict(rgb=z(0, 3), acc=z(0), weights=z(0, 4), affine_trans=z(0, 3, 4), affine_trans_sky=z(0, 3, 4)) for _ in range(2)]
    batch = dict(rgb=torch.zeros(0, 3, device=dev), lossmult=torch.zeros(0, 1, device=dev), sky_segs=torch.zeros(0, device=dev))
    cfg = types.SimpleNamespace(data_loss_type="charb", charb_padding=0.001, data_loss_mult=1.0, data_coarse_loss_mult=0.3, disable_multiscale_loss=False)
    monkeypatch.setattr(tu._lib, "load", boom)
    for name, fn in (("compute_data_loss", lambda: tu.compute_data_loss(batch, rend, cfg)[0]), ("sky_loss", lambda: tu.sky_loss(batch, rend)),
                     ("transformIdentityLoss", lambda: tu.transformIdentityLoss(rend))):
        loss = fn()
        assert bool(torch.isnan(loss)), (name, float(loss))
        loss.backward()
    assert rend[0]["rgb"].grad is None or rend[0]["rgb"].grad.shape == (0, 3)
