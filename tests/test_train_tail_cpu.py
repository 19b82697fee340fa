"""The float64 restatement of the training tail (tests/train_tail_ref.py) against the project's own eager float32 forms on host
tensors -- the non-HIP branches of compute_data_loss, sky_loss and transformIdentityLoss, the host branch of hash_decay,
torch.optim.Adam(foreach=False), all pinned to the reference's goldens elsewhere -- and every bar that
tests/test_train_tail_gpu.py places on a kernel applied to those eager forms on the same inputs: a bar the reference arithmetic
cannot meet is a wrong bar, and an e_ref below its bracket's min_ref shows here without a GPU.

One exception, stated where it is made: the rawnerf terms.  The kernels form them in double (a deliberate departure);
the float32 eager form loses digits in `1e-3 + clip` near clip = -1e-3 and cannot meet a bar counted in double roundings, so
their bars are applied to the eager form evaluated on the float64 upcast of the inputs."""
import numpy as np
import pytest
import torch

import train_tail_ref as R
from train_tail_ref import U32, U64, gamma


def within(name, got, want, bar):
    diff = (torch.as_tensor(got).double() - torch.as_tensor(want, dtype=torch.float64)).abs()
    bar = torch.as_tensor(bar, dtype=torch.float64)
    bad = diff > bar
    assert not bool(bad.any()), (name, int(bad.sum()), float(diff.max()), float((diff / bar.clamp_min(1e-300)).max()))
    return float((diff / bar.clamp_min(1e-300)).max()) if diff.numel() else 0.0


def test_hash_decay_restatement_and_bars():
    e_ref, truth = [], []
    for name, (L, C, rows) in R.HASH_CASES.items():
        emb, off = R.hash_inputs(name)
        assert emb.shape == (sum(rows), C) and all(r > 0 for r in rows)
        want = R.hash_decay(emb, rows)
        for g in (1.0, -0.37):
            val, grad = R.eager_hash_decay(emb, off, g)
            gw = R.hash_decay_grad(emb, rows, g)
            within(f"{name} gradient g={g}", grad, gw, gamma(R.ROUNDINGS["hash_decay_bwd"]) * gw.abs())
        assert abs(float(val) - want) <= R.hash_decay_fwd_bound(emb.numel(), L) * want, name
        per_level = torch.stack([(emb.double()[off[i]:off[i + 1]] ** 2).mean(dim=0) for i in range(L)]).mean()    # models.py:297-306 as written
        assert abs(float(per_level) - want) <= 1e-13 * want, name
        e_ref.append(abs(float(val) - want)); truth.append(want)
    assert max(e_ref) >= R.min_ref(truth), (e_ref, truth)
    total = {k: sum(v[2]) * v[1] for k, v in R.HASH_CASES.items()}
    assert total["total_below_4096_floats"] < 4096 and 550000 < total["total_near_600000_floats"] < 650000, total
    assert all(r % 4 for k in ("L16_C2_geometric_7_to_40000",) for r in R.HASH_CASES[k][2])


@pytest.mark.parametrize("sky", [False, True], ids=["no_sky", "sky"])
@pytest.mark.parametrize("N", R.BLEND_N)
def test_affine_blend_restatement_and_bars(N, sky):
    t = R.blend_inputs(N)
    opt = (t["acc"], t["sky"], t["A_sky"]) if sky else ()
    out, grads = R.eager_affine_blend(t, sky, t["g_out"])
    want, mag = R.affine_blend_fwd(t["rgb"], t["A"], *opt)
    within("forward", out, want, gamma(R.ROUNDINGS["blend_fwd_sky" if sky else "blend_fwd"]) * mag)
    ref = R.affine_blend_bwd(t["g_out"], t["rgb"], t["A"], *opt)
    assert set(ref) == set(grads)
    for k, (val, mg) in ref.items():
        within(k, grads[k], val, gamma(R.ROUNDINGS[k]) * mg)
    # the written-out gradients are the float64 autograd of the written-out forward
    leaves = [x.double().requires_grad_(True) for x in (t["rgb"], t["A"]) + opt]
    R.affine_blend_fwd(*leaves)[0].backward(t["g_out"].double())
    for k, leaf in zip(("g_rgb", "g_affine", "g_acc", "g_sky", "g_affine_sky"), leaves):
        assert float((leaf.grad - ref[k][0]).abs().max()) <= 1e-14 * max(1.0, float(ref[k][0].abs().max())), k
    assert float(t["acc"][0]) in (0.0, 1.0) and (N == 1 or float(t["acc"][N // 2]) == 1.0)


@pytest.mark.parametrize("with_mult", [False, True], ids=["lossmult_null", "lossmult"])
@pytest.mark.parametrize("N", R.DATA_N)
@pytest.mark.parametrize("L", R.DATA_L)
def test_data_loss_restatement_and_bars(L, N, with_mult):
    levels, target, mult = R.data_inputs(L, N)
    mult = mult if with_mult else None
    e_ref, truth = [], []
    for pattern in ("charb_only", "mse_only", "rawnerf_only"):
        wm, wc, wr = R.data_weights(pattern, L)
        if L == 1:
            assert (wm + wc + wr).count(1.0) == 1
        for g in (1.0, 0.25):
            ref = R.data_loss(levels, target, mult, wm, wc, wr, R.CHARB_PAD, g=g)
            # the rawnerf exception of the module docstring: eager on the float64 upcast
            dtype = torch.float64 if pattern == "rawnerf_only" else torch.float32
            loss, mses, grads = R.eager_data_pattern(levels, target, mult, pattern, g=g, dtype=dtype)
            u = U64 if dtype == torch.float64 else U32
            # a sum of 3 N non-negative terms in any order, six roundings to form a term, the division and the weighting
            sum_bar = gamma(3 * N + 10, u)
            assert abs(float(loss) - ref["loss"]) <= sum_bar * ref["loss"], (pattern, float(loss), ref["loss"])
            # the statistics come back through LazyStats as float32 whatever the inputs' type: one more float32 rounding
            within(f"{pattern} mses", mses, ref["mses"], (sum_bar + U32) * torch.tensor(ref["mses"], dtype=torch.float64))
            for l in range(L):
                bar = gamma(R.ROUNDINGS["data_bwd"]) * ref["mags"][l] + gamma(8, U64) * ref["mags"][l]
                if mult is not None and pattern != "rawnerf_only":
                    # the eager denominator is a float32 sum of the multipliers where the restatement's is exact
                    bar = bar + sum_bar * ref["mags"][l]
                within(f"{pattern} gradient level {l} g={g}", grads[l], ref["grads"][l], bar)
                if pattern == "charb_only":
                    assert float(grads[l].view(-1)[(l * 5) % (3 * N)]) == 0.0 or N == 1, l       # rgb == target: exactly 0
        if pattern in R.FLOAT_PATTERNS:
            e_ref.append((R.data_vector(loss, mses) - R.data_vector(ref["loss"], ref["mses"])).abs())
            truth.append(R.data_vector(ref["loss"], ref["mses"]))
    e_ref, truth = torch.cat(e_ref), torch.cat(truth)
    assert float(e_ref.max()) >= R.min_ref(truth), (e_ref, truth)
    # the mixed pattern is linear in the pure ones: per level and kind through the eager branch in float64
    wm, wc, wr = R.data_weights("mixed_per_level", L)
    ref = R.data_loss(levels, target, mult, wm, wc, wr, R.CHARB_PAD, g=1.0)
    tot, grads = 0.0, []
    for l in range(L):
        gl = torch.zeros(N, 3, dtype=torch.float64)
        for kind, w in (("mse", wm[l]), ("charb", wc[l]), ("rawnerf", wr[l])):
            loss, _, gr = R.eager_data_loss([levels[l]], target, mult, kind, 0.0, 1.0, R.CHARB_PAD, g=1.0, dtype=torch.float64)
            w = float(np.float32(w))                                          # the weights reach the kernels as floats
            tot += w * float(loss)
            gl += w * gr[0]
        grads.append(gl)
    assert abs(tot - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    for l in range(L):
        assert float((grads[l] - ref["grads"][l]).abs().max()) <= 1e-12 * max(1e-30, float(ref["grads"][l].abs().max())), l
    # the planted edges are there: rgb == 1 keeps the rawnerf gradient, one ulp above loses it
    x = levels[0].view(-1)
    one, above = (1 * 5) % x.numel(), (2 * 5) % x.numel()
    if N > 1:
        wr1 = R.data_weights("rawnerf_only", L)
        gr = R.data_loss(levels, target, mult, *wr1, R.CHARB_PAD, g=1.0)["grads"][0].view(-1)
        assert float(x[one]) == 1.0 and float(x[above]) > 1.0 and float(gr[above]) == 0.0
        assert float(gr[one]) != 0.0 or float(mult[one // 3]) == 0.0


@pytest.mark.parametrize("N", R.SKY_N)
def test_sky_loss_restatement_and_bars(N):
    e_ref, truth = [], []
    for L in R.SKY_L:
        for segs, seed in (("binary", 0), ("binary", 1), ("fractional", 2)):
            accs, s = R.sky_inputs(L, N, segs, seed)
            want, grads, mags = R.sky_loss(accs, s, g=0.7)
            loss, eg = R.eager_sky_loss(accs, s, g=0.7)
            # N non-negative terms per level in any order, the logarithms and the products of a term
            assert abs(float(loss) - want) <= gamma(N + 16) * want, (L, segs, float(loss), want)
            for l in range(L):
                within(f"gradient L={L} {segs} level {l}", eg[l], grads[l], gamma(R.ROUNDINGS["sky_bwd"]) * mags[l])
                raw = accs[l].double()
                outside = (raw < R.CLIP_LO) | (raw > R.CLIP_HI)
                assert bool((eg[l][outside] == 0).all()) and bool((grads[l][outside] == 0).all())
                on = (raw == R.CLIP_LO) | (raw == R.CLIP_HI)
                assert bool((eg[l][on] != 0).all()) and bool((grads[l][on] != 0).all())                # the bounds are inside
            e_ref.append(abs(float(loss) - want)); truth.append(want)
    assert max(e_ref) >= R.min_ref(truth), (e_ref, truth)
    if N >= len(R.SKY_EDGES):
        accs, _ = R.sky_inputs(1, N)
        assert all(bool((accs[0] == e).any()) for e in R.SKY_EDGES)


@pytest.mark.parametrize("sky", [False, True], ids=["no_sky", "sky"])
@pytest.mark.parametrize("N", R.IDENTITY_N)
def test_identity_loss_restatement(N, sky):
    A, B = R.identity_inputs(N)
    B = B if sky else None
    want, grads = R.identity_loss(A, B, g=0.3)
    loss, eg = R.eager_identity_loss(A, B, g=0.3)
    assert loss.dtype == torch.float64 and abs(float(loss) - want) <= gamma(24 * N + 4, U64) * want
    for a, b in zip(eg, grads):
        assert a.dtype == torch.float32 and torch.equal(a, b.float())
    eye = torch.eye(4)[:3].reshape(1, 12).expand(N, 12)
    on = A == eye
    assert int(on.sum()) >= 2 and bool((grads[0][on] == 0).all()) and bool((A[~on] > eye[~on]).any()) and bool((A[~on] < eye[~on]).any())


def adam_mags(p, g, m, v, step, sanitize):
    """float64 sums of the absolute terms of the three results"""
    tp, tg, tm, tv = R.adam_step(p, g, m, v, step=step, sanitize=sanitize, **R.ADAM_HYPER)
    b1, b2 = R.ADAM_HYPER["betas"]
    mag_m = m.double().abs() + (1 - b1) * (tg.abs() + m.double().abs())
    upd = (tp - p.double()).abs()
    # the update is proportional to exp_avg: where m + (1 - b1)(g - m) cancels, its relative error is mag_m / |exp_avg| times larger
    return (tp, tm, tv), (p.double().abs() + upd * (1.0 + mag_m / tm.abs().clamp_min(1e-300)), mag_m, b2 * v.double() + (1 - b2) * tg * tg)


@pytest.mark.parametrize("sanitize", [0, 1])
@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam_restatement_and_bars(n, sanitize):
    for step in R.ADAM_STEPS:
        e_ref = [[], [], []]
        truth = [[], [], []]
        for seed in range(R.ADAM_SEEDS(n)):
            p, g, m, v = R.adam_inputs(n, seed, nonfinite=bool(sanitize))
            host = R.eager_adam(p, g, m, v, step, sanitize)
            want, mags = adam_mags(p, g, m, v, step, sanitize)
            fin = R.adam_masks(host, host)
            assert bool(torch.isfinite(host[0]).all()) and bool(torch.isfinite(host[1]).all())
            # eight float32 roundings cover either form: lerp / addcmul / sqrt / div / add / addcdiv in torch, the fused forms here
            for k in range(3):
                within(f"adam n={n} step={step} result {k}", host[k][fin], want[k][fin], gamma(8) * mags[k][fin] + 1e-45)
                e_ref[k].append((host[k].double() - want[k]).abs()[fin]); truth[k].append(want[k][fin].abs())
            over = ~fin                                                        # a +-FLT_MAX gradient: the float32 second moment overflows
            assert bool(torch.isinf(host[2][over]).all()) and torch.equal(host[0][over], p[over])
        for k in range(3):
            e, t = torch.cat(e_ref[k]), torch.cat(truth[k])
            assert e.numel() > 0 and float(e.max()) >= R.min_ref(t), (n, step, k, float(e.max()), R.min_ref(t))


def test_adam_inputs_hold_the_special_gradients():
    for n in (1023, 1024 * 256 + 3):
        g = R.adam_inputs(n, 0, nonfinite=True)[1]
        body, tail = g[:(n // 4) * 4], g[(n // 4) * 4:]
        assert tail.numel() == 3
        for part in (body, tail):
            assert bool(torch.isnan(part).any()) and bool((part == float("inf")).any()) and bool((part == float("-inf")).any())
        assert bool((body == 0).any()) and bool((body == R.FLT_MAX).any()) and bool((body == -R.FLT_MAX).any())
        assert bool(((body != 0) & (body.abs() < np.finfo(np.float32).tiny)).any())                     # a float32 subnormal
    seen = torch.stack([R.adam_inputs(1, s, nonfinite=True)[1] for s in range(7)]).view(-1)
    assert len({repr(float(x)) for x in seen}) >= 4
