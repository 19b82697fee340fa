"""float64 restatement of the small HIP nodes that close a training step (csrc/heads_train.hip and the optimiser half of
csrc/train_ops.hip), the generators of the inputs they are tested on, and the project's own float32 eager forms run on host
tensors.  Host only: tests/test_train_tail_cpu.py holds the restatement to the eager forms, tests/test_train_tail_gpu.py the
kernels to the restatement, both on the inputs drawn here from the same seeds.

Inputs arrive as float32 tensors and are upcast exactly; every function returns float64.  Functions that feed a derived bound
also return `mag`, the float64 sum of the ABSOLUTE terms of the same expression: a kernel that evaluates the expression with n
roundings is within gamma(n) * mag of the value."""
import types

import numpy as np
import torch

U32, U64 = 2.0 ** -24, 2.0 ** -53
FLT_MAX = float(np.finfo(np.float32).max)
CLIP_LO, CLIP_HI = float(np.float32(1e-3)), float(np.float32(0.999))      # the float32 bounds of clip(acc, 1e-3, 1 - 1e-3)
PAD = 5                                                                     # spare elements behind every in / out buffer


def gamma(n, u=U32):
    """n roundings of unit u: |computed - exact| <= gamma * sum |terms| (Higham, Accuracy and Stability, lemma 3.1)"""
    return n * u / (1.0 - n * u)


def ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def d(t):
    return None if t is None else t.double()


# ------------------------------------------------------------------ hash decay (models.py:297-306)
def hash_decay_weights(rows, C):
    rows = np.asarray(rows, dtype=np.float64)
    return torch.from_numpy(np.repeat(1.0 / (rows * len(rows) * C), np.asarray(rows, dtype=np.int64)))      # [total rows]


def hash_decay(emb, rows):
    """sum over levels of sum e^2 / (rows_l L C)"""
    w = hash_decay_weights(rows, emb.shape[1])
    return float((d(emb) ** 2 * w[:, None]).sum())


def hash_decay_grad(emb, rows, g):
    """2 g e / (rows_l L C); the expression is one product chain, so mag = |value|"""
    w = hash_decay_weights(rows, emb.shape[1])
    return 2.0 * float(g) * d(emb) * w[:, None]


# ------------------------------------------------------------------ affine blend (models.py:339-363)
def _dot4(M, v, absolute):
    """[N,12] per-ray [3,4] maps applied to [N,3]: M[:, :, :3] v + M[:, :, 3]"""
    M = M.reshape(-1, 3, 4)
    if absolute:
        M, v = M.abs(), v.abs()
    return (M[:, :, :3] * v[:, None, :]).sum(-1) + M[:, :, 3]


def affine_blend_fwd(rgb, A, acc=None, sky=None, A_sky=None):
    """rgb' = A rgb + t (+ (1 - acc) (A_sky sky + t_sky)) -> (value, mag), each [N,3]"""
    rgb, A, acc, sky, A_sky = d(rgb), d(A), d(acc), d(sky), d(A_sky)
    out, mag = _dot4(A, rgb, False), _dot4(A, rgb, True)
    if sky is not None:
        opac = (1.0 - acc)[:, None]
        out = out + opac * _dot4(A_sky, sky, False)
        mag = mag + opac.abs() * _dot4(A_sky, sky, True)
    return out, mag


def affine_blend_bwd(g_out, rgb, A, acc=None, sky=None, A_sky=None):
    """all five gradients written out -> dict name -> (value, mag); the sky entries only with a sky"""
    go, rgb, A, acc, sky, A_sky = d(g_out), d(rgb), d(A).reshape(-1, 3, 4), d(acc), d(sky), d(A_sky)
    N = rgb.shape[0]
    ones = torch.ones(N, 1, dtype=torch.float64)
    t = go[:, :, None] * A[:, :, :3]                                           # [N, c, k]
    out = {"g_rgb": (t.sum(1), t.abs().sum(1))}
    gA = (go[:, :, None] * torch.cat([rgb, ones], -1)[:, None, :]).reshape(N, 12)
    out["g_affine"] = (gA, gA.abs())
    if sky is not None:
        B = A_sky.reshape(-1, 3, 4)
        opac = 1.0 - acc
        out["g_acc"] = (-(go * _dot4(B, sky, False)).sum(-1), (go.abs() * _dot4(B, sky, True)).sum(-1))
        ts = go[:, :, None] * B[:, :, :3]
        out["g_sky"] = (opac[:, None] * ts.sum(1), opac.abs()[:, None] * ts.abs().sum(1))
        gB = (opac[:, None, None] * go[:, :, None] * torch.cat([sky, ones], -1)[:, None, :]).reshape(N, 12)
        out["g_affine_sky"] = (gB, gB.abs())
    return out


# ------------------------------------------------------------------ data loss (train_utils.py:171-230)
def data_loss(levels, target, mult, w_mse, w_charb, w_raw, pad, g=None, den=None):
    """-> dict(loss, mses [L], charbs [L], raws [L], den); with g also grads / mags: the gradient w.r.t. every level's rgb for an
    upstream gradient g.  `den` replaces the denominator in the gradient (the backward kernel divides by the float32 value the
    forward stored; upcast exactly it is one of its inputs).  rawnerf: the 1 / (1e-3 + clip) factor is detached, clamp_max's
    gradient is 1 where rgb <= 1 (the bound included)."""
    w_mse, w_charb, w_raw = ([float(np.float32(x)) for x in w] for w in (w_mse, w_charb, w_raw))      # the C ABI takes float weights
    tgt = d(target)
    m = torch.ones(tgt.shape[0], dtype=torch.float64) if mult is None else d(mult)
    m3 = m[:, None].expand_as(tgt)
    denom = float(m3.sum())
    pad2 = float(pad) ** 2
    res = dict(mses=[], charbs=[], raws=[], den=denom, grads=[], mags=[])
    loss = 0.0
    for l, x in enumerate(levels):
        x = d(x)
        r = x - tgt
        clip = x.clamp_max(1.0)
        scale = 1.0 / (1e-3 + clip) ** 2
        mse = float((m3 * r * r).sum()) / denom
        charb = float((m3 * torch.sqrt(r * r + pad2)).sum()) / denom
        raw = float((m3 * (clip - tgt) ** 2 * scale).sum()) / denom
        res["mses"].append(mse); res["charbs"].append(charb); res["raws"].append(raw)
        loss += float(w_mse[l]) * mse + float(w_charb[l]) * charb + float(w_raw[l]) * raw
        if g is not None:
            k = float(g) * m3 / (denom if den is None else float(den))
            t_mse = float(w_mse[l]) * 2.0 * r
            t_charb = float(w_charb[l]) * r / torch.sqrt(r * r + pad2)
            t_raw = float(w_raw[l]) * 2.0 * (clip - tgt) * scale * (x <= 1.0)
            res["grads"].append(k * (t_mse + t_charb + t_raw))
            res["mags"].append(k.abs() * (t_mse.abs() + t_charb.abs() + t_raw.abs()))
    res["loss"] = loss
    return res


# ------------------------------------------------------------------ sky loss (train_utils.py:149-157)
def sky_loss(accs, sky_segs, g=None):
    """sum over levels of mean BCE(clip(acc, 1e-3, 1 - 1e-3), 1 - sky_segs) -> (value, grads, mags); the gradient is 0 outside
    the float32 bounds and includes them"""
    t = 1.0 - d(sky_segs)
    N = t.numel()
    tot, grads, mags = 0.0, [], []
    for acc in accs:
        raw = d(acc)
        a = raw.clamp(CLIP_LO, CLIP_HI)
        tot += float(-(t * torch.log(a) + (1.0 - t) * torch.log1p(-a)).sum()) / N
        if g is not None:
            inside = (raw >= CLIP_LO) & (raw <= CLIP_HI)
            k = float(g) / N / (a * (1.0 - a))
            grads.append(torch.where(inside, k * (a - t), torch.zeros_like(a)))
            mags.append(torch.where(inside, abs(float(g)) / N / (a * (1.0 - a)) * (a.abs() + t.abs()), torch.zeros_like(a)))
    return tot, grads, mags


# ------------------------------------------------------------------ identity loss (train_utils.py:159-169)
def _eye(N):
    return torch.eye(4, dtype=torch.float64)[:3].reshape(1, 12).expand(N, 12)


def identity_loss(A, A_sky=None, g=None):
    """mean over [N, 12] of |eye - A| (+ |eye - A_sky|) -> (value, [gradient per map]); gradient -sign(eye - a) g / (12 N)"""
    maps = [d(A).reshape(-1, 12)] + ([d(A_sky).reshape(-1, 12)] if A_sky is not None else [])
    N = maps[0].shape[0]
    val = float(sum((_eye(N) - M).abs().sum() for M in maps)) / (12.0 * N)
    grads = None if g is None else [-torch.sign(_eye(N) - M) * float(g) / (12.0 * N) for M in maps]
    return val, grads


# ------------------------------------------------------------------ Adam (torch/optim/adam.py, amsgrad = False, no weight decay)
def adam_step(p, g, m, v, lr, betas, eps, step, sanitize=False):
    """one step -> (p, g as stored, exp_avg, exp_avg_sq); the bias corrections are Python doubles as torch.optim.Adam forms them"""
    p, g, m, v = d(p), d(g), d(m), d(v)
    if sanitize:
        g = torch.nan_to_num(g, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX)    # float32's nan_to_num
    b1, b2 = float(betas[0]), float(betas[1])
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (float(lr) / bc1) * m / (torch.sqrt(v) / bc2 ** 0.5 + float(eps))
    return p, g, m, v


# ================================================================== inputs (identical in both test files: same seeds)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


HASH_CASES = {          # name -> (L, C, rows per level)
    "L1_C1_one_row": (1, 1, [1]),
    "L2_C2_rows_3_5": (2, 2, [3, 5]),
    "L16_C2_geometric_7_to_40000": (16, 2, [r + (r % 4 == 0) for r in (int(round(7 * (40000 / 7) ** (i / 15))) for i in range(16))]),
    "L32_C4_mixed_small_rows": (32, 4, [(i * 7) % 13 + 1 + 30 * (i % 5 == 2) for i in range(32)]),
    "L16_C8_geometric_5_to_3000": (16, 8, [int(round(5 * (3000 / 5) ** (i / 15))) for i in range(16)]),
    "total_below_4096_floats": (8, 2, [3, 5, 9, 17, 31, 61, 123, 251]),               # 1000 floats: 250 of the 1024 blocks hold any
    "total_near_600000_floats": (16, 2, [r + (r % 4 == 0) for r in (int(round(11 * (131000 / 11) ** (i / 15))) for i in range(16))]),
}


def hash_inputs(name):
    """table whose levels alternate between two scales (1e-4, and 10 on every eighth level), so a level that took its
    neighbour's weight shows -> (emb [rows, C] float32, offsets int32 [L + 1])"""
    L, C, rows = HASH_CASES[name]
    g = _gen(100 + len(name) + L)
    emb = torch.cat([(torch.rand(r, C, generator=g) * 2 - 1) * (10.0 if l % 8 == 1 else 1e-4) for l, r in enumerate(rows)]).float()
    return emb, np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)


def blend_inputs(N):
    """per-ray maps near the identity, acc_last with exact 0 and 1 among the rays"""
    g = _gen(200 + N)
    eye = torch.eye(4)[:3].reshape(1, 12)
    r = lambda *s: torch.rand(*s, generator=g)
    t = dict(rgb=r(N, 3), sky=r(N, 3), A=eye + 0.2 * torch.randn(N, 12, generator=g), A_sky=eye + 0.2 * torch.randn(N, 12, generator=g),
             acc=r(N) * 1.2 - 0.1, g_out=torch.randn(N, 3, generator=g), g_out2=torch.randn(N, 3, generator=g))
    t["acc"][0] = 1.0 if N == 1 else 0.0
    if N > 1:
        t["acc"][N // 2] = 1.0
    return {k: v.float().contiguous() for k, v in t.items()}


DATA_PATTERNS = {       # name -> (w_mse, w_charb, w_raw) for up to four levels, the last entry being the final level's
    "charb_only": ([0, 0, 0, 0], [0.3, 0.3, 0.3, 1.0], [0, 0, 0, 0]),
    "mse_only": ([0.3, 0.3, 0.3, 1.0], [0, 0, 0, 0], [0, 0, 0, 0]),
    "rawnerf_only": ([0, 0, 0, 0], [0, 0, 0, 0], [0.3, 0.3, 0.3, 1.0]),
    "mixed_per_level": ([0.5, 0.0, 0.25, 0.0], [0.0, 0.7, 0.1, 0.0], [0.0, 0.0, 0.05, 1.0]),
}


def data_weights(pattern, L):
    return tuple([float(x) for x in w[4 - L:]] for w in DATA_PATTERNS[pattern])


def data_inputs(L, N):
    """-> (levels [L x [N,3]], target [N,3], lossmult [N]) with the edges planted in every level: rgb == target exactly, rgb of
    exactly 1.0f and one ulp above it, rgb near -1e-3 (a small rawnerf denominator); some rays weigh 0"""
    g = _gen(300 + 10 * L + N)
    target = torch.rand(N, 3, generator=g).float()
    mult = (torch.rand(N, generator=g) + 0.5).float()
    if N > 2:
        mult[1::7] = 0.0
    levels = []
    for l in range(L):
        x = (target + 0.1 * torch.randn(N, 3, generator=g)).float()
        flat, tf = x.view(-1), target.view(-1)
        edges = [None, 1.0, float(np.nextafter(np.float32(1.0), np.float32(2.0))), -1e-3 + 3e-5]
        for j, e in enumerate(edges):
            i = ((j + l) * 5) % flat.numel()                                   # N = 1 holds three of them, a different set per level
            flat[i] = tf[i] if e is None else e
        levels.append(x.contiguous())
    return levels, target, mult


SKY_EDGES = [np.float32(1e-3), np.float32(0.999)]
SKY_EDGES = [float(v) for b in SKY_EDGES for v in (b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(1)))] + [-0.25, 1.5]


def sky_inputs(L, N, segs="binary", seed=0):
    """acc per level with values exactly at the two float32 bounds, one ulp inside and outside each, below 0 and above 1"""
    g = _gen(400 + 10 * L + N + 1000 * seed)
    accs = []
    for l in range(L):
        a = (torch.rand(N, generator=g) * 1.2 - 0.1).float()
        for j, e in enumerate(SKY_EDGES):
            if N >= len(SKY_EDGES) or j == (l + seed) % len(SKY_EDGES):
                a[(j * 3 + l) % N] = e
        accs.append(a)
    s = torch.rand(N, generator=g)
    return accs, ((s > 0.6).float() if segs == "binary" else s.float())


def identity_inputs(N):
    """maps around the identity, entries exactly equal to the identity's 0 and 1 planted in both"""
    g = _gen(500 + N)
    eye = torch.eye(4)[:3].reshape(1, 12)
    A, B = (eye + 0.2 * torch.randn(N, 12, generator=g)).float(), (eye + 0.2 * torch.randn(N, 12, generator=g)).float()
    for M in (A, B):
        M.view(-1)[0::5] = eye.expand(N, 12).reshape(-1)[0::5]                # every fifth entry sits on the identity: gradient 0
    return A.contiguous(), B.contiguous()


ADAM_HYPER = dict(lr=float(np.float32(0.01)), betas=(float(np.float32(0.9)), float(np.float32(0.99))), eps=float(np.float32(1e-8)))
# the C ABI takes the hyper-parameters as floats: float32 values here, so that the restatement, torch.optim.Adam and the kernels
# are handed the same numbers
ADAM_SPECIAL = [0.0, 1e-41, FLT_MAX, -FLT_MAX]
ADAM_NONFINITE = [float("nan"), float("inf"), float("-inf")]


def adam_inputs(n, seed=0, nonfinite=False):
    """p, g, m, v of n elements with non-zero starting moments; the special gradients sit at the head (the float4 body from n = 8)
    and at the tail (the up-to-three elements after the last float4)"""
    g = _gen(600 + n % 1000 + 7 * seed)
    p, grad = torch.randn(n, generator=g), torch.randn(n, generator=g) * 10.0 ** float(torch.randint(-3, 2, (1,), generator=g))
    m, v = 0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g)
    special = (ADAM_NONFINITE if nonfinite else []) + ADAM_SPECIAL       # the first three also land in the tail
    for j in range(len(special)):
        if n > 2 * len(special):
            grad[j] = grad[n - 1 - j] = special[j]
        elif j < n:
            grad[j] = special[(j + seed) % len(special)]                      # short tensors: a different selection per seed
    return [t.float().contiguous() for t in (p, grad, m, v)]


# ================================================================== the project's eager float32 forms on host tensors
def eager_hash_decay(emb, offsets, g=None):
    from ucnerf_amd.internal import train_graph
    e = emb.clone().requires_grad_(g is not None)
    mlp = types.SimpleNamespace(encoder=types.SimpleNamespace(embeddings=e, _offsets_np=np.asarray(offsets)))
    val = train_graph.hash_decay(mlp)
    if g is None:
        return val.detach()
    (val * g).backward()
    return val.detach(), e.grad


def eager_affine_blend(t, with_sky, g_out=None):
    """models.py:339-363 in the broadcast-multiply form (the eager side of test_fused_heads_tail_matches_the_eager_form)"""
    N = t["rgb"].shape[0]
    leaves = {k: t[k].clone().requires_grad_(True) for k in (("rgb", "A", "acc", "sky", "A_sky") if with_sky else ("rgb", "A"))}
    affine = lambda M, v: (M.reshape(N, 3, 4)[:, :3, :3] * v.reshape(N, 1, 3)).sum(dim=-1, keepdim=True) + M.reshape(N, 3, 4)[:, :3, 3:]
    out = affine(leaves["A"], leaves["rgb"])
    if with_sky:
        out = out + (1 - leaves["acc"])[:, None, None] * affine(leaves["A_sky"], leaves["sky"])
    out = out.reshape(N, 3)
    if g_out is None:
        return out.detach()
    out.backward(g_out)
    names = dict(rgb="g_rgb", A="g_affine", acc="g_acc", sky="g_sky", A_sky="g_affine_sky")
    return out.detach(), {names[k]: v.grad for k, v in leaves.items()}


def eager_data_loss(levels, target, mult, kind, coarse, final, pad, g=None, dtype=torch.float32):
    """the non-HIP branch of compute_data_loss (host tensors never take the HIP node) -> (loss, mses, grads)"""
    from ucnerf_amd.internal import train_utils as tu
    N = target.shape[0]
    lv = [x.to(dtype).clone().requires_grad_(g is not None) for x in levels]
    cfg = types.SimpleNamespace(data_loss_type=kind, charb_padding=pad, data_loss_mult=final, data_coarse_loss_mult=coarse,
                                disable_multiscale_loss=mult is None)
    batch = dict(rgb=target.to(dtype), lossmult=(torch.ones(N, 1) if mult is None else mult.reshape(N, 1)).to(dtype))
    loss, stats = tu.compute_data_loss(batch, [dict(rgb=x) for x in lv], cfg)
    if g is not None:
        (loss * g).backward()
    return loss.detach(), torch.as_tensor(np.asarray(stats["mses"])), [x.grad for x in lv]


def eager_sky_loss(accs, sky_segs, g=None):
    from ucnerf_amd.internal import train_utils as tu
    lv = [a.clone().requires_grad_(g is not None) for a in accs]
    loss = tu.sky_loss(dict(sky_segs=sky_segs), [dict(weights=a[:, None]) for a in lv])       # one sample per ray: acc = its weight
    if g is not None:
        (loss * g).backward()
    return loss.detach(), [a.grad for a in lv]


def eager_identity_loss(A, A_sky=None, g=None):
    from ucnerf_amd.internal import train_utils as tu
    maps = [M.reshape(-1, 3, 4).clone().requires_grad_(g is not None) for M in ([A] + ([A_sky] if A_sky is not None else []))]
    r = dict(affine_trans=maps[0])
    if A_sky is not None:
        r["affine_trans_sky"] = maps[1]
    loss = tu.transformIdentityLoss([r])
    if g is not None:
        (loss * g).backward()
    return loss.detach(), [M.grad.reshape(-1, 12) if M.grad is not None else None for M in maps]


def eager_adam(p, g, m, v, step, sanitize):
    """torch.optim.Adam(foreach=False) on host tensors, its state set to (m, v, step - 1) -> (p, exp_avg, exp_avg_sq)"""
    q = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], foreach=False, **ADAM_HYPER)
    opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    q.grad = torch.nan_to_num(g) if sanitize else g.clone()
    opt.step()
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]


def adam_masks(host, other):
    """entries whose three results are finite on both sides (a +-FLT_MAX gradient overflows the float32 second moment, which
    the float64 step does not: no truth to bracket there), after asserting that the non-finite entries agree exactly"""
    fin = torch.ones_like(host[0], dtype=torch.bool)
    for a, b in zip(host, other):
        assert torch.equal(torch.isfinite(a), torch.isfinite(b)) and torch.equal(a[~torch.isfinite(a)].nan_to_num(1.5), b[~torch.isfinite(b)].nan_to_num(1.5))
        fin &= torch.isfinite(a)
    return fin


# ================================================================== the derived bars (shared by the host and the device tests)
# Roundings on the longest path of each kernel expression (csrc/heads_train.hip, csrc/train_ops.hip); the bar on an element is
# gamma(count) * mag, mag the float64 sum of the expression's absolute terms.  No count is taken from what a kernel returns.
ROUNDINGS = {
    # o[c] = ((A0 r + A1 g) + A2 b) + A3: a product and three adds
    "blend_fwd": 4,
    # o[c] += opac * (((B0 sr + B1 sg) + B2 sb) + B3), opac = 1 - acc: the 4-term dot (4), opac (1), the product (1), the blend (1)
    # come to 7; the issue's own count for "a 4-term dot plus the blend" is 8
    "blend_fwd_sky": 8,
    # g_rgb[k] = (go0 A0k + go1 A1k) + go2 A2k
    "g_rgb": 3,
    # gA[c][k] = go[c] * v[k]
    "g_affine": 1,
    # dot += go[c] * (((B0 s0 + B1 s1) + B2 s2) + B3) over c (the first add is to 0.0f: exact), g_acc = -dot: 4 + 1 + 2
    "g_acc": 7,
    # g_sky[k] = opac * ((go0 B0k + go1 B1k) + go2 B2k): 3, opac 1, the product 1
    "g_sky": 5,
    # gB[c][k] = opac * go[c] * s[k]: opac 1 and two products
    "g_affine_sky": 3,
    # accumulate = 1: prefill + t, twice
    "accumulate": 2,
    # out[i] = e * (g2 * w), g2 = 2 g exact, w = (float)(1 / (rows L C)): three roundings
    "hash_decay_bwd": 3,
    # gl = g[0] * m * (w_mse * 2 * r + w_charb * r / sqrtf(r2 + pad2)), m = mult / den, r = rgb - target.  On the Charbonnier
    # path: r (1; both terms are monotone in r with relative condition <= 1), r2 (1), + pad2 (1) and pad2 = fl(fl(pad)^2) itself (3), all
    # halved by the square root (2.5), sqrtf (1), w_charb * r (1), the division (1), the sum (1), m (1), g m (1), the last product (1): 10.5,
    # and with a rawnerf weight the float cast of the double term and `gl +=` (the term itself is formed in double): 11
    "data_bwd": 11,
    # go * (a - t) / (a * (1 - a)), go = g / N, t = 1 - seg: go (1), t (1), a - t (1), 1 - a (1), a (1 - a) (1), the product (1),
    # the division (1)
    "sky_bwd": 7,
}


def sum_bound(per_thread, per_term, tree, extra=0, u=U32):
    """relative bound on a fixed-order sum of non-negative terms: `per_term` roundings to form a term, `per_thread` sequential
    adds, `tree` levels of pairwise adds, `extra` roundings after the sum"""
    return gamma(per_term + per_thread + tree + extra, u)


def hash_decay_fwd_bound(total, L):
    """k_hash_decay<false> + k_decay_finish: a thread squares-and-adds its elements with fmaf (one rounding each; at most
    ceil(per / 256) of them, one more per level its block meets), folds each level in with fmaf(w, part, acc) (one rounding, w's
    own another), then 8 tree levels; the finish kernel adds 4 partials per thread and 8 tree levels"""
    per = ((total + 1023) // 1024 + 3) & ~3
    seq = (per + 255) // 256 + 2 * L + 1
    return gamma(seq + 8 + 4 + 8)


# ================================================================== the cases (section by section the same in both test files)
BLEND_N = [1, 255, 256, 257, 15000]
DATA_L, DATA_N = [1, 2, 3, 4], [1, 341, 1025, 15000]
SKY_L, SKY_N = [1, 4], [1, 1023, 1024, 1025, 15000]
IDENTITY_N = [1, 85, 15000]
ADAM_N = [1, 2, 3, 4, 5, 7, 1023, 1024 * 256 + 1, 1024 * 256 + 3]
ADAM_STEPS = [1, 2, 1000, 100000]
ADAM_SEEDS = lambda n: 16 if n < 64 else 1                                # short tensors: enough draws for a bracket to mean something
CHARB_PAD = 0.001
FLOAT_PATTERNS = {"charb_only": "charb", "mse_only": "mse"}                 # the patterns k_data_loss_fwd (float sums) serves
MIN_REF = 2.0 ** -26


def min_ref(truth):
    """min_ref of every bracket: a quarter of a float32 ulp of the typical (median) entry of the bracketed vector.  A float32
    evaluation that is closer than that to the float64 value EVERYWHERE says nothing about float32 arithmetic."""
    return MIN_REF * float(torch.as_tensor(truth, dtype=torch.float64).abs().reshape(-1).median())


def eager_data_pattern(levels, target, mult, pattern, g=None, dtype=torch.float32):
    """one of the three pure weight patterns through compute_data_loss's eager branch (coarse 0.3, final 1.0)"""
    kind = dict(charb_only="charb", mse_only="mse", rawnerf_only="rawnerf")[pattern]
    return eager_data_loss(levels, target, mult, kind, float(np.float32(0.3)), 1.0, CHARB_PAD, g=g, dtype=dtype)


def data_vector(loss, mses):
    return torch.cat([torch.as_tensor(mses, dtype=torch.float64).reshape(-1), torch.as_tensor([float(loss)], dtype=torch.float64)])
