"""Float64 layer models of the four fused bf16 training kernels (csrc/field_train.hip: ucn_train_fwd / ucn_train_bwd,
csrc/sky_train.hip: ucn_sky_train_fwd / ucn_sky_train_bwd), written from the contract in include/ucnerf_march.h.

Both forwards store every hidden activation once, as the bf16 operand the next layer consumed, and both backwards every
pre-activation gradient.  So each layer is checked ALONE: its input is the tensor the kernel stored, the layer is formed in
float64 from the bf16-rounded logical weights, and the result is compared with the tensor the kernel stored behind it,
element by element.  No drift accumulates, and the bar is derived, not measured (`bound`).

Everything here is torch on the CPU; the same functions judge the GPU kernels (test_heads_layerwise_gpu.py) and a float32
emulation of them with planted faults (test_heads_layerwise_cpu.py)."""
import numpy as np
import torch

F64 = torch.float64
U32 = 2.0 ** -23     # ONE fp32 ulp (relative): twice the unit roundoff, so an MFMA that truncates its internal adds is covered
UBF = 2.0 ** -8      # half a bf16 ulp relative to the value: bf16 carries 8 significant bits (7 stored), so a value in
#                      [2^e, 2^(e+1)) has ulp 2^(e-7) and round-to-nearest moves it by at most 2^(e-8) <= 2^-8 |v|.  (2^-9 is
#                      half of that: 1 + 2^-8 - eps rounds to 1 and is 2^-8 away; test_heads_layerwise_cpu.py shows the case.)
SKY_S = 120
ACT_BLOCKS = dict(h2=(0, 256), h1=(256, 512), x=(512, 768), aux=(768, 800), h0=(800, 864), fb=(864, 928))   # head_pack._ACT_*
SKY_AUX, SKY_HV, SKY_DV, SKY_G, SKY_LD = 2048, 2080, 2048, 2176, 2240


def rb(t):
    """fp32 -> bf16, round to nearest even, as float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def rz(t):
    """fp32 -> bf16 by truncation (the planted rounding fault), as float32."""
    return (t.to(torch.float32).contiguous().view(torch.int32) & -65536).view(torch.float32)


def perm(r, g):
    """Feature (within a 32-wide tile) held by accumulator register r of wave half g."""
    return (r & 3) + 8 * (r >> 2) + 4 * g


def acc_order(width):
    """natural index of every accumulator-order slot [tile][wave half][16]."""
    t, g, r = np.meshgrid(np.arange((width + 31) // 32), np.arange(2), np.arange(16), indexing="ij")
    return torch.from_numpy((32 * t + perm(r, g)).reshape(-1))


def from_acc(v, width):
    """[.., tiles * 32] in accumulator order -> natural order [.., width]."""
    out = torch.zeros(v.shape[:-1] + (32 * ((width + 31) // 32),), dtype=v.dtype)
    out[..., acc_order(width)] = v
    return out[..., :width]


def to_acc(v, width):
    pad = torch.zeros(v.shape[:-1] + (32 * ((width + 31) // 32),), dtype=v.dtype)
    pad[..., :v.shape[-1]] = v
    return pad[..., acc_order(width)].contiguous()


# ------------------------------------------------------------------ ReLU mask bit layouts
def decode_mask(words):
    """int32 words [M, 2 (wave half), P] (m0: [M, 2] = P 1; m1 / m2 and the sky's per-layer mask: P 4; mask_v: P 2) -> bool
    [M, 64 P]: bit 16 o + r of word p of half h is feature 32 (2 p + o) + perm(r, h)."""
    w = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    if w.ndim == 2:
        w = w[:, :, None]
    M, _, P = w.shape
    out = np.zeros((M, 64 * P), dtype=bool)
    r = np.arange(16)
    for h in range(2):
        for p in range(P):
            for o in range(2):
                out[:, 32 * (2 * p + o) + perm(r, h)] = ((w[:, h, p, None] >> (16 * o + r)) & 1).astype(bool)
    return torch.from_numpy(out)


def encode_mask(bits):
    """The inverse of decode_mask: bool [M, 64 P] -> int32 [M, 2, P]."""
    b = np.asarray(bits).astype(np.int64)
    M, P = b.shape[0], b.shape[1] // 64
    w = np.zeros((M, 2, P), dtype=np.int64)
    r = np.arange(16)
    for h in range(2):
        for p in range(P):
            for o in range(2):
                w[:, h, p] |= (b[:, 32 * (2 * p + o) + perm(r, h)] << (16 * o + r)).sum(axis=1)
    return torch.from_numpy(w.astype(np.uint32).view(np.int32))


# ------------------------------------------------------------------ the per-element bound
def bound(exact, sum_abs, K, bf16, extra=0.0):
    """|got - exact| allowed for an output formed as a K-term dot product with terms t_k (sum_abs = sum |t_k|, the bias /
    accumulator start among them): delta = (K + 1) 2^-23 sum |t_k| is the worst-case fp32 summation error in ANY order
    (unit 2^-23, a truncating MFMA included; bf16 x bf16 products are exact in fp32); `extra` = what the layer's inputs were
    already off by (stated at each use).  Stored as fp32: delta.  Stored as bf16: plus half a bf16 ulp of the fp32 value,
    UBF (|exact| + delta).  Derived, not tuned."""
    delta = (K + 1) * U32 * sum_abs + extra
    return UBF * (exact.abs() + delta) + delta if bf16 else delta


def lin(x, W, b=None):
    """x W^T (+ b) and the sum of the absolute terms, float64."""
    e, s = x @ W.t(), x.abs() @ W.abs().t()
    if b is not None:
        e, s = e + b, s + b.abs()
    return e, s


class Report:
    """worst error / bound per (kernel, layer) over every case judged, and the case it came from."""

    def __init__(self):
        self.rows, self.measured = {}, {}

    def judge(self, case, layer, got, exact, bnd):
        got, exact = got.to(F64), exact.to(F64)
        assert got.shape == exact.shape, (layer, got.shape, exact.shape)
        if got.numel() == 0:
            return 0.0, 0
        err = (got - exact).abs()
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
        bnd = torch.as_tensor(bnd, dtype=F64).expand_as(err)
        ratio = torch.where(err <= bnd, err / bnd.clamp_min(1e-300), torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.full_like(err, float("inf"))))
        ratio = torch.where(err == 0, torch.zeros_like(err), ratio)
        worst, outside = float(ratio.max()), int((err > bnd).sum())
        if layer not in self.rows or worst > self.rows[layer][0]:
            self.rows[layer] = (worst, case, outside if layer not in self.rows else max(outside, self.rows[layer][2]))
        elif outside > self.rows[layer][2]:
            self.rows[layer] = self.rows[layer][:2] + (outside,)
        return worst, outside

    def exact(self, case, layer, got, want):
        same = bool(torch.equal(got, want))
        self.judge(case, layer, got.to(F64), want.to(F64), 0.0) if not same and got.shape == want.shape else None
        if same and layer not in self.rows:
            self.rows[layer] = (0.0, case, 0)
        return same

    def mask(self, case, layer, words, stored, pre, delta):
        """A mask bit is the SIGN of the fp32 accumulator (clear sign = 1, a pre-activation of exactly +0 included: relu'(0) = 1, a valid
        subgradient where torch picks 0).  So: bit == (stored > 0) wherever the exact pre-activation is further than the fp32 summation
        error `delta` from zero; inside that band a set bit over a stored 0 is the accumulator landing on +0 (F = 1: feat w = -bias happens
        with bf16 operands), nothing else is allowed."""
        bit, pos = decode_mask(words), stored.float() > 0
        ok = (bit == pos) | (bit & ~pos & (pre.abs() <= delta))
        return self.exact(case, layer, ~ok, torch.zeros_like(ok))

    def measure(self, what, ref_err, got_err):
        r, g = self.measured.get(what, (0.0, 0.0))
        self.measured[what] = (max(r, float(ref_err)), max(g, float(got_err)))

    def failures(self):
        return {k: v for k, v in self.rows.items() if v[2] > 0 or not v[0] <= 1.0}

    def text(self):
        lines = ["layer-wise float64 check of the fused bf16 training kernels: worst |got - exact| / bound per stored tensor",
                 "(bound: tests/heads_layerwise_ref.py `bound`; 0 = bit-exact; every row must stay <= 1)", ""]
        lines += [f"{k:<34s} {v[0]:8.4f}   outside {v[2]:d}   worst case: {v[1]}" for k, v in sorted(self.rows.items())]
        lines += ["", "activations / compositing: max abs error against float64 on the kernel's own logits / raw",
                  "(fp32 torch-CPU evaluation of the same formula | kernel | kernel / fp32; allowed: 4)"]
        lines += [f"{k:<34s} {r:.3e} | {g:.3e} | {g / max(r, 1e-300):6.2f}" for k, (r, g) in sorted(self.measured.items())]
        return "\n".join(lines) + "\n"


# ------------------------------------------------------------------ NeRF field: ucn_train_fwd / ucn_train_bwd
def field_weights(P, composed=None):
    """The bf16-rounded matrices the kernels multiply by, float64, from the LOGICAL fp32 parameters P = dict(Wd0 [64,F], bd0,
    Wd1 [256,64], bd1, W0 [256,256+E], b0, W1 [256,512+E], b1, Wr [3,256], br), rounded where head_pack.prepare_heads rounds:
    each plain matrix as it is, the composed ones (W0x Wd1), (W1x Wd1) AFTER the fp32 composition (`composed` = those two fp32
    products as the host formed them; default: float64 products rounded to fp32)."""
    NB, NW = P["Wd1"].shape[0], P["W0"].shape[0]
    W0x, W1h, W1x = P["W0"][:, :NB], P["W1"][:, :NW], P["W1"][:, NW:NW + NB]
    if composed is None:
        composed = ((W0x.to(F64) @ P["Wd1"].to(F64)).float(), (W1x.to(F64) @ P["Wd1"].to(F64)).float())
    return dict(Wd0=rb(P["Wd0"]), Wd1=rb(P["Wd1"]), W0x=rb(W0x), W1h=rb(W1h), W1x=rb(W1x), Wr=rb(P["Wr"]), Wc0=rb(composed[0]), Wc1=rb(composed[1]))


def softplus64(z):
    return torch.where(z > 20, z, torch.log1p(torch.exp(torch.clamp(z, max=20.0))))


def head_density(raw, head, dt):
    """models.py:515 softplus(raw + density_bias), beta 1 / threshold 20, in dtype dt."""
    z = raw.to(dt) + torch.tensor(head[0], dtype=dt)
    return torch.where(z > 20, z, torch.log1p(torch.exp(z)))


def head_rgb(y, head, dt):
    """models.py:667-672 sigmoid(premult y + bias) (1 + 2 pad) - pad in dtype dt."""
    c = lambda v: torch.tensor(v, dtype=dt)
    return torch.sigmoid(c(head[1]) * y.to(dt) + c(head[2])) * (1 + 2 * c(head[3])) - c(head[3])


def field_forward_check(rep, case, Wb, inp, out):
    """Judge every tensor ucn_train_fwd stored, one layer at a time.  inp: feat [M,F] fp32, bd0 / bd1 / br (fp32, natural order,
    the values handed to the kernel), pr0 / pr1 [N,256] fp32 natural order, S, head (4 floats | None).  out: h0, x, h1, h2 (bf16),
    raw, y (fp32: the logits of the head = NULL launch), m0, m1, m2 (int32 words), feat_bf16 | None, density / rgb (the head launch) | None."""
    f64 = lambda t: t.to(F64)
    M, F = inp["feat"].shape
    ray = torch.arange(M) // inp["S"]
    fb = rb(inp["feat"])
    if out.get("feat_bf16") is not None:
        rep.exact(case, "fwd feat_bf16", f64(out["feat_bf16"]), fb)
    e, s = lin(fb, Wb["Wd0"], f64(inp["bd0"]))
    rep.mask(case, "fwd mask of h0", out["m0"], out["h0"], e, (F + 1) * U32 * s)
    rep.judge(case, "fwd h0", out["h0"], e.clamp_min(0), bound(e.clamp_min(0), s, F, True))
    h0 = f64(out["h0"])
    e, s = lin(h0, Wb["Wd1"], f64(inp["bd1"]))
    rep.judge(case, "fwd x", out["x"], e, bound(e, s, 64, True))
    rep.exact(case, "fwd raw = x[:,0]", f64(out["raw"]), f64(out["x"])[:, 0])
    e, s = lin(h0, Wb["Wc0"])
    p0 = f64(inp["pr0"])[ray]
    e, s = e + p0, s + p0.abs()
    rep.mask(case, "fwd mask of h1", out["m1"], out["h1"], e, 65 * U32 * s)
    rep.judge(case, "fwd h1", out["h1"], e.clamp_min(0), bound(e.clamp_min(0), s, 64, True))
    h1 = f64(out["h1"])
    e1, s1 = lin(h1, Wb["W1h"])
    e2, s2 = lin(h0, Wb["Wc1"])
    p1 = f64(inp["pr1"])[ray]
    e, s = e1 + e2 + p1, s1 + s2 + p1.abs()
    rep.mask(case, "fwd mask of h2", out["m2"], out["h2"], e, 321 * U32 * s)
    rep.judge(case, "fwd h2", out["h2"], e.clamp_min(0), bound(e.clamp_min(0), s, 320, True))
    e, s = lin(f64(out["h2"]), Wb["Wr"], f64(inp["br"]))
    rep.judge(case, "fwd y", out["y"], e, bound(e, s, 256, False))
    if out.get("density") is not None:
        head = inp["head"]
        for what, got, fn, logit in (("density", out["density"], head_density, out["raw"]), ("rgb", out["rgb"], head_rgb, out["y"])):
            truth = fn(logit, head, F64)
            rep.measure(f"field fwd {what}", (fn(logit, head, torch.float32).to(F64) - truth).abs().max(), (f64(got) - truth).abs().max())


def field_backward_check(rep, case, Wb, inp, out):
    """Judge every tensor ucn_train_bwd stored.  inp: gy [M,3], graw [M] | None (bf16 without head, fp32 with), head | None, lm (0 row-major, 1 / 2 level-major pairs / quads).  out: dy [M,>=4] bf16, d1, d0, gx, gh0 bf16,
    gfeat fp32 (as written), m0 / m1 / m2, density / rgb (the forward's outputs, head mode)."""
    f64 = lambda t: t.to(F64)
    M = out["d1"].shape[0]
    dy = f64(out["dy"])[:, :4]
    if inp.get("head") is None:
        want = torch.cat([f64(inp["gy"]), f64(inp["graw"])[:, None] if inp.get("graw") is not None else torch.zeros(M, 1, dtype=F64)], dim=1)
        rep.exact(case, "bwd dy (bf16 in)", dy, want)
    else:
        # activation derivatives in fp32 from the saved outputs: sg = (rgb + pad) / k, v = gy k premult sg (1 - sg).  Roundings: k (1),
        # sg (2 + k's), 1 - sg (1, and it inherits sg's 3 ulp scaled by sg / (1 - sg)), four products: relative (9 + 3 sg / (1 - sg)) ulp
        _, pm, _, pad = inp["head"]
        k = 1 + 2 * pad
        sg = (f64(out["rgb"]) + pad) / k
        e = f64(inp["gy"]) * k * pm * sg * (1 - sg)
        rep.judge(case, "bwd dy[:, :3] (head)", dy[:, :3], e, bound(e, 0 * e, 0, True, extra=e.abs() * U32 * (9 + 3 * sg / (1 - sg).clamp_min(1e-30))))
        if inp.get("graw") is not None:
            # graw * (-expm1f(-density)): one product, expm1f within 2 ulp, the negation exact
            e = f64(inp["graw"]) * (-torch.expm1(-f64(out["density"])))
            rep.judge(case, "bwd dy[:, 3] (head)", dy[:, 3], e, bound(e, 0 * e, 0, True, extra=4 * U32 * e.abs()))
        else:
            rep.exact(case, "bwd dy[:, 3] (head)", dy[:, 3], torch.zeros(M, dtype=F64))
    m0, m1, m2 = (decode_mask(out[k]).to(F64) for k in ("m0", "m1", "m2"))
    e, s = lin(dy[:, :3], Wb["Wr"].t())
    rep.judge(case, "bwd d1", out["d1"], m2 * e, m2 * bound(e, s, 3, True))
    d1 = f64(out["d1"])
    e, s = lin(d1, Wb["W1h"].t())
    rep.judge(case, "bwd d0", out["d0"], m1 * e, m1 * bound(e, s, 256, True))
    d0 = f64(out["d0"])
    ea, sa = lin(d1, Wb["W1x"].t())
    eb, sb = lin(d0, Wb["W0x"].t())
    e, s = ea + eb, sa + sb
    e[:, 0] += dy[:, 3]
    s[:, 0] += dy[:, 3].abs()
    rep.judge(case, "bwd gx", out["gx"], e, bound(e, s, 513, True))
    e, s = lin(f64(out["gx"]), Wb["Wd1"].t())
    rep.judge(case, "bwd gh0", out["gh0"], m0 * e, m0 * bound(e, s, 256, True))
    e, s = lin(f64(out["gh0"]), Wb["Wd0"].t())
    F = e.shape[1]
    lm = inp.get("lm", 0)
    if lm:
        C = 2 * lm                                   # [F / C][M][C], every value / 6: one more fp32 rounding (the IEEE division)
        got = out["gfeat"].reshape(F // C, M, C).permute(1, 0, 2).reshape(M, F)
        d = bound(e, s, 64, False)
        rep.judge(case, f"bwd gfeat (level-major {C})", got, e / 6, d / 6 + 0.5 * U32 * (e.abs() + d) / 6)
    else:
        rep.judge(case, "bwd gfeat", out["gfeat"], e, bound(e, s, 64, False))


# ------------------------------------------------------------------ sky NeRF: ucn_sky_train_fwd / ucn_sky_train_bwd
def sky_points(inp, dt):
    """models.py:870-873: z = far (1 - t) + t / (1.5 far[0]), pts = o + d z, in dtype dt from the fp32 inputs."""
    far, tv = inp["far"].to(dt).reshape(-1, 1), inp["tv"].to(dt)
    z = far * (1 - tv) + 1 / (1.5 * far[0:1]) * tv
    return z, inp["o"].to(dt)[:, None, :] + inp["d"].to(dt)[:, None, :] * z[:, :, None]


def sky_embed(cam):
    return torch.cat([cam] + [fn(cam * f) for f in (1.0, 2.0, 4.0, 8.0) for fn in (torch.sin, torch.cos)], dim=-1)


def sky_composite(raw, inp, dt):
    """models.py:822-850 raw2outputs on raw [N,120,4] = (colour logits, sigma) in dtype dt -> rgb_map [N,3]."""
    z, _ = sky_points(inp, dt)
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], dim=-1) * torch.norm(inp["d"].to(dt), dim=-1, keepdim=True)
    alpha = 1 - torch.exp(-torch.relu(raw[..., 3]) * dists)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha + 1e-10], dim=-1), dim=-1)[:, :-1]
    return ((alpha * trans)[..., None] * torch.sigmoid(raw[..., :3])).sum(dim=-2)


def sky_composite_backward(raw, g, inp, dt=F64):
    """The compositing backward as csrc/sky_train.hip states it: d / d y = g w c (1 - c), d / d alpha_s = g . (T_s c_s) -
    (sum_{k > s} g . (w_k c_k)) / (1 - alpha_s + 1e-10), d / d sigma = d / d alpha dist exp(-sigma dist) for sigma > 0."""
    z, _ = sky_points(inp, dt)
    raw, g = raw.to(dt), g.to(dt)
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], dim=-1) * torch.norm(inp["d"].to(dt), dim=-1, keepdim=True)
    ex = torch.exp(-torch.relu(raw[..., 3]) * dists)
    alpha = 1 - ex
    keep = 1 - alpha + 1e-10
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), keep], dim=-1), dim=-1)[:, :-1]
    w, c = alpha * T, torch.sigmoid(raw[..., :3])
    gc = (g[:, None, :] * c).sum(-1)
    wg = w * gc
    after = wg.sum(-1, keepdim=True) - torch.cumsum(wg, dim=-1)
    dalpha = T * gc - after / keep
    dsig = torch.where(raw[..., 3] > 0, dalpha * dists * ex, torch.zeros_like(dalpha))
    return torch.cat([g[:, None, :] * w[..., None] * c * (1 - c), dsig[..., None]], dim=-1)


def sky_weights(P):
    """bf16-rounded matrices of the MFMA layers (float64) from the logical fp32 parameters P = dict(W = 8 weights (W[5] unused), b,
    m5 [256,288], mv [128,288], wa [1,256], ba [1], wr [3,128], br [3]); layer 0 and the two heads stay fp32."""
    return dict(W={l: rb(P["W"][l]) for l in (1, 2, 3, 4, 6, 7)}, m5=rb(P["m5"]), mv=rb(P["mv"]), wr=rb(P["wr"]), wa=rb(P["wa"]))


def sky_forward_check(rep, case, P, inp, out):
    """out: act [M,2240] bf16 (h_0 .. h_7 | aux | hv), raw [M,4], mask [8,M,2,4], mask_v [M,2,2], sky_rgb [N,3]."""
    f64 = lambda t: t.to(F64)
    Wb = sky_weights(P)
    N = inp["o"].shape[0]
    M = N * SKY_S
    z, pts = sky_points(inp, F64)
    p = pts.reshape(M, 3)
    # the kernel forms the point in fp32: 1.5 far0, its reciprocal, 1 - t, two products and the sum give z to 4 ulp of (|a| + |b|),
    # then d z and the sum with o: 8 ulp of (|o| + |d| (|a| + |b|)) covers it
    far, tv = f64(inp["far"]).reshape(-1, 1), f64(inp["tv"])
    zabs = (far * (1 - tv)).abs() + (1 / (1.5 * far[0:1]) * tv).abs()
    dp = (8 * U32 * (f64(inp["o"]).abs()[:, None, :] + f64(inp["d"]).abs()[:, None, :] * zabs[:, :, None])).reshape(M, 3)
    act = out["act"]
    ray = torch.arange(M) // SKY_S
    # aux = (p, 1, embed(cam_dir) (27), 0): sinf / cosf of |x| <= 8 within 4 ulp absolute
    aux = torch.cat([p, torch.ones(M, 1, dtype=F64), sky_embed(f64(inp["cam"]))[ray], torch.zeros(M, 1, dtype=F64)], dim=1)
    daux = torch.cat([dp, torch.zeros(M, 1, dtype=F64), torch.full((M, 27), 4 * U32, dtype=F64), torch.zeros(M, 1, dtype=F64)], dim=1)
    rep.judge(case, "sky fwd aux", act[:, SKY_AUX:SKY_AUX + 32], aux, bound(aux, 0 * aux, 0, True, extra=daux))
    W0, b0 = f64(P["W"][0]), f64(P["b"][0])
    e, s = lin(p, W0, b0)
    rep.mask(case, "sky fwd masks", out["mask"][0], act[:, 0:256], e, 4 * U32 * s + dp @ W0.abs().t())
    e = e.clamp_min(0)
    rep.judge(case, "sky fwd h_0", act[:, 0:256], e, bound(e, s, 3, True, extra=dp @ W0.abs().t()))
    auxs = f64(act[:, SKY_AUX:SKY_AUX + 32])
    for l in range(1, 8):
        hin = f64(act[:, 256 * (l - 1):256 * l])
        if l == 5:
            e, s = lin(torch.cat([hin, auxs], dim=1), Wb["m5"])
            K = 288
        else:
            e, s = lin(hin, Wb["W"][l], f64(P["b"][l]))
            K = 256
        rep.mask(case, "sky fwd masks", out["mask"][l], act[:, 256 * l:256 * (l + 1)], e, (K + 1) * U32 * s)
        e = e.clamp_min(0)
        rep.judge(case, f"sky fwd h_{l}", act[:, 256 * l:256 * (l + 1)], e, bound(e, s, K, True))
    h7 = f64(act[:, 1792:2048])
    e, s = lin(torch.cat([h7, auxs], dim=1), Wb["mv"])
    rep.mask(case, "sky fwd mask_v", out["mask_v"], act[:, SKY_HV:SKY_HV + 128], e, 289 * U32 * s)
    e = e.clamp_min(0)
    rep.judge(case, "sky fwd hv", act[:, SKY_HV:SKY_HV + 128], e, bound(e, s, 288, True))
    hv = f64(act[:, SKY_HV:SKY_HV + 128])
    # the two heads read the fp32 ReLU output, the buffer holds its bf16 rounding: |a - stored| <= UBF stored per input
    wa, wr = f64(P["wa"]), f64(P["wr"])
    e, s = lin(h7, wa, f64(P["ba"]))
    rep.judge(case, "sky fwd raw sigma", out["raw"][:, 3:4], e, bound(e, s, 256, False, extra=UBF * (h7 @ wa.abs().t())))
    e, s = lin(hv, wr, f64(P["br"]))
    rep.judge(case, "sky fwd raw logits", out["raw"][:, :3], e, bound(e, s, 128, False, extra=UBF * (hv @ wr.abs().t())))
    raw = out["raw"].reshape(N, SKY_S, 4)
    truth = sky_composite(f64(raw), inp, F64)
    scale = truth.abs().amax(dim=1, keepdim=True).clamp_min(1.0)      # (negative dists let the transmittance grow: errors relative to the ray's scale)
    rep.measure("sky fwd sky_rgb", ((sky_composite(raw.float(), inp, torch.float32).to(F64) - truth).abs() / scale).max(),
                ((f64(out["sky_rgb"]) - truth).abs() / scale).max())


def sky_backward_check(rep, case, P, inp, out):
    """out: raw [M,4] (what ucn_sky_train_bwd was given), g_raw [M,4] fp32, grad [M,2240] bf16 (d0 .. d7 | dv | g), mask, mask_v."""
    f64 = lambda t: t.to(F64)
    Wb = sky_weights(P)
    N = inp["o"].shape[0]
    M = N * SKY_S
    raw = out["raw"].reshape(N, SKY_S, 4)
    truth = sky_composite_backward(raw, inp["g_sky"], inp).reshape(M, 4)
    r32 = raw.float().clone().requires_grad_(True)
    (sky_composite(r32, inp, torch.float32) * inp["g_sky"].float()).sum().backward()
    ref = r32.grad.reshape(M, 4).to(F64)
    for what, cols in (("d logits", slice(0, 3)), ("d sigma", slice(3, 4))):
        t = truth.reshape(N, SKY_S, 4)[..., cols]
        scale = t.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-30)                 # per ray: their scales differ by orders of magnitude
        err = lambda v: ((v.reshape(N, SKY_S, 4)[..., cols] - t).abs() / scale).max()
        rep.measure(f"sky bwd g_raw {what}", err(ref), err(f64(out["g_raw"])))
    grad = out["grad"]
    g = torch.cat([rb(out["g_raw"]), torch.zeros(M, 28, dtype=F64)], dim=1)
    rep.exact(case, "sky bwd g tile", f64(grad[:, SKY_G:SKY_G + 32]), g)
    mv_ = decode_mask(out["mask_v"]).to(F64)
    e, s = lin(g[:, :3], Wb["wr"].t())
    rep.judge(case, "sky bwd dv", grad[:, SKY_DV:SKY_DV + 128], mv_ * e, mv_ * bound(e, s, 3, True))
    dv = f64(grad[:, SKY_DV:SKY_DV + 128])
    m = decode_mask(out["mask"][7]).to(F64)
    e, s = lin(torch.cat([dv, g[:, 3:4]], dim=1), torch.cat([Wb["mv"][:, :256], Wb["wa"]], dim=0).t())
    rep.judge(case, "sky bwd d7", grad[:, 1792:2048], m * e, m * bound(e, s, 129, True))
    for l in range(6, -1, -1):
        W = Wb["m5"][:, :256] if l + 1 == 5 else Wb["W"][l + 1]
        m = decode_mask(out["mask"][l]).to(F64)
        e, s = lin(f64(grad[:, 256 * (l + 1):256 * (l + 2)]), W.t())
        rep.judge(case, f"sky bwd d{l}", grad[:, 256 * l:256 * (l + 1)], m * e, m * bound(e, s, 256, True))


# ------------------------------------------------------------------ inputs shared by the GPU test and the CPU emulation
def field_params(F, seed, E=27):
    """Logical fp32 parameters with unit-scale layer outputs and biases off zero (about half of every ReLU layer active)."""
    g = torch.Generator().manual_seed(seed)
    w = lambda o, i: torch.randn(o, i, generator=g) / i ** 0.5
    b = lambda o: torch.randn(o, generator=g) * 0.5
    return dict(Wd0=w(64, F), bd0=b(64), Wd1=w(256, 64), bd1=b(256), W0=w(256, 256 + E), b0=b(256), W1=w(256, 512 + E) * 0.8, b1=b(256),
                Wr=w(3, 256), br=b(3))


def field_inputs(N, S, F, seed, head=True, graw=True):
    g = torch.Generator().manual_seed(seed + 1)
    M = N * S
    inp = dict(feat=torch.randn(M, F, generator=g), pr0=torch.randn(N, 256, generator=g) * 0.7, pr1=torch.randn(N, 256, generator=g) * 0.7,
               S=S, N=N, head=(-0.5, 1.0, 0.0, 0.001) if head else None)
    gy, gr = torch.randn(M, 3, generator=g), torch.randn(M, generator=g)
    inp["gy"] = gy if head else gy.to(torch.bfloat16)
    inp["graw"] = None if not graw else (gr if head else gr.to(torch.bfloat16))
    inp["ray_cols"] = torch.randn(N, 32, generator=g).to(torch.bfloat16)
    return inp


def sky_params(seed):
    g = torch.Generator().manual_seed(seed)
    w = lambda o, i: torch.randn(o, i, generator=g) * (2.0 / i) ** 0.5
    b = lambda o: torch.randn(o, generator=g) * 0.3
    W = [w(256, 3)] + [w(256, 256) for _ in range(4)] + [w(256, 259)] + [w(256, 256) for _ in range(2)]
    bs = [b(256) for _ in range(8)]
    Wf, bf, Wv, bv = w(256, 256), b(256), w(128, 283), b(128)
    P = dict(W=W, b=bs, wa=w(1, 256), ba=b(1) - 0.3, wr=w(3, 128), br=b(3), Wf=Wf, bf=bf, Wv=Wv, bv=bv)
    z = torch.zeros
    P["m5"] = torch.cat([W[5][:, 3:], W[5][:, :3], bs[5][:, None], z(256, 28)], dim=1).contiguous()
    Wvf = Wv[:, :256].to(F64)
    P["mv"] = torch.cat([(Wvf @ Wf.to(F64)).float(), z(128, 3), (bv.to(F64) + Wvf @ bf.to(F64)).float()[:, None], Wv[:, 256:], z(128, 1)], dim=1).contiguous()
    return P


def sky_trunk64(P, pts, cam):
    """The sky NeRF in float64, unrounded, the reference's own formulation (models.py:786-815): raw [.., 4]."""
    f = lambda t: t.to(F64)
    h = pts
    for i in range(8):
        h = torch.relu(h @ f(P["W"][i]).t() + f(P["b"][i]))
        if i == 4:
            h = torch.cat([pts, h], dim=-1)
    sigma = h @ f(P["wa"]).t() + f(P["ba"])
    feat = h @ f(P["Wf"]).t() + f(P["bf"])
    hv = torch.relu(torch.cat([feat, sky_embed(cam)], dim=-1) @ f(P["Wv"]).t() + f(P["bv"]))
    return torch.cat([hv @ f(P["wr"]).t() + f(P["br"]), sigma], dim=-1)


def sky_inputs(N, P, seed):
    """N rays with `far` varied per ray.  The reference's z runs from `far` DOWN to 1 / (1.5 far[0]) (models.py:872 with near = far),
    so an ordinary ray has negative dists and slightly negative alphas; the kernels mirror that.  For N >= 3, ray 1's sigma logits
    are all negative (alpha = 0 everywhere) and ray 2 saturates (alpha = 1 from the first sample: its far lies below 1 / sky_far,
    so its z increases, and its direction is long): both are picked among candidates with the float64 network."""
    g = torch.Generator().manual_seed(seed)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    inp = dict(o=torch.randn(N, 3, generator=g) * 0.3, d=unit(N), cam=unit(N), far=2.0 + 6.0 * torch.rand(N, generator=g),
               tv=torch.linspace(0., 1., SKY_S), g_sky=torch.randn(N, 3, generator=g))
    if N >= 3:
        inp["far"][2] = 1e-3
        cand, cand_o = unit(256), torch.randn(256, 3, generator=g) * 0.5
        for r, want_neg in ((1, True), (2, False)):
            cd = cand if want_neg else cand * 1e5
            trial = dict(inp, o=cand_o, d=cd, far=torch.cat([inp["far"][0:1], inp["far"][r].expand(255)]))
            _, pts = sky_points(trial, F64)
            sig = sky_trunk64(P, pts, cand.to(F64)[:, None, :].expand(-1, SKY_S, -1))[..., 3]
            # clear of the bf16 chain's drift: 5 % of the ray's own sigma scale / half the candidates' typical first-sample sigma
            score = -sig.max(dim=1).values / sig.abs().max(dim=1).values if want_neg else sig[:, 0] / sig[:, 0].abs().median() / 10
            best = int(score[1:].argmax()) + 1
            assert float(score[best]) > 0.05, (r, float(score[best]))
            inp["d"][r], inp["o"][r] = cd[best], cand_o[best]
    return inp


def sky_composed(P, dt=F64):
    """The two 9-tile layers as the host hands them over (sky_train.sky_forward_fused): m5 = [W5[:, 3:] | W5[:, :3] | b5 | 0 (28)],
    mv = [Wv[:, :256] Wf | 0 (3) | bv + Wv[:, :256] bf | Wv[:, 256:] | 0], columns = [h (256) | aux = (p, 1, embed (27), 0)]."""
    f = lambda t: t.to(dt)
    z = lambda *s: torch.zeros(*s, dtype=dt)
    W5, Wvf = f(P["W"][5]), f(P["Wv"])[:, :256]
    m5 = torch.cat([W5[:, 3:], W5[:, :3], f(P["b"][5])[:, None], z(256, 28)], dim=1)
    mv = torch.cat([Wvf @ f(P["Wf"]), z(128, 3), (f(P["bv"]) + Wvf @ f(P["bf"]))[:, None], f(P["Wv"])[:, 256:], z(128, 1)], dim=1)
    return m5, mv


def sky_chain64(P, inp):
    """The kernels' formulation (composed layers, aux tile) chained in float64 without any rounding: raw [N,120,4], rgb_map [N,3]."""
    f = lambda t: t.to(F64)
    N = inp["o"].shape[0]
    _, pts = sky_points(inp, F64)
    m5, mv = sky_composed(P)
    aux = torch.cat([pts, torch.ones(N, SKY_S, 1, dtype=F64), sky_embed(f(inp["cam"]))[:, None, :].expand(-1, SKY_S, -1), torch.zeros(N, SKY_S, 1, dtype=F64)], dim=-1)
    h = torch.relu(pts @ f(P["W"][0]).t() + f(P["b"][0]))
    for l in range(1, 8):
        h = torch.relu(torch.cat([h, aux], dim=-1) @ m5.t()) if l == 5 else torch.relu(h @ f(P["W"][l]).t() + f(P["b"][l]))
    sigma = h @ f(P["wa"]).t() + f(P["ba"])
    hv = torch.relu(torch.cat([h, aux], dim=-1) @ mv.t())
    raw = torch.cat([hv @ f(P["wr"]).t() + f(P["br"]), sigma], dim=-1)
    return raw, sky_composite(raw, inp, F64)


def field_chain64(P, inp, enc):
    """The kernels' formulation of the field (composed colour layers, per-ray terms) chained in float64 without rounding, forward and
    backward: density, rgb and d (sum density cd + sum rgb cr) / d feat for the output gradients inp['graw'], inp['gy']."""
    f = lambda t: t.to(F64)
    NB, NW = 256, 256
    Wd0, Wd1, W0, W1, Wr = (f(P[k]) for k in ("Wd0", "Wd1", "W0", "W1", "Wr"))
    W0x, W0e, W1h, W1x, W1e = W0[:, :NB], W0[:, NB:], W1[:, :NW], W1[:, NW:NW + NB], W1[:, NW + NB:]
    ray = torch.arange(inp["feat"].shape[0]) // inp["S"]
    pr0 = (f(enc) @ W0e.t() + f(P["b0"]) + W0x @ f(P["bd1"]))[ray]
    pr1 = (f(enc) @ W1e.t() + f(P["b1"]) + W1x @ f(P["bd1"]))[ray]
    h0 = torch.relu(f(inp["feat"]) @ Wd0.t() + f(P["bd0"]))
    x = h0 @ Wd1.t() + f(P["bd1"])
    h1 = torch.relu(h0 @ (W0x @ Wd1).t() + pr0)
    h2 = torch.relu(h1 @ W1h.t() + h0 @ (W1x @ Wd1).t() + pr1)
    y = h2 @ Wr.t() + f(P["br"])
    head = inp["head"]
    density, rgb = head_density(x[:, 0], head, F64), head_rgb(y, head, F64)
    k = 1 + 2 * head[3]
    sg = (rgb + head[3]) / k
    dy = f(inp["gy"]) * k * head[1] * sg * (1 - sg)
    d1 = (h2 > 0) * (dy @ Wr)
    d0 = (h1 > 0) * (d1 @ W1h)
    gx = d1 @ W1x + d0 @ W0x
    gx[:, 0] += f(inp["graw"]) * (-torch.expm1(-density))
    gh0 = (h0 > 0) * (gx @ Wd1)
    return density, rgb, gh0 @ Wd0


def field_host(P, inp):
    """The bias vectors as head_pack.prepare_heads hands them to the kernel: rounded to bf16, fp32."""
    for k in ("bd0", "bd1", "br"):
        inp[k] = rb(P[k]).float()
    return inp


# ------------------------------------------------------------------ the cases (test_heads_layerwise_gpu.py runs them on the kernels)
SHAPES = [(1, 31), (2, 32), (3, 96), (5, 100), (7, 37)]     # one partial wave | SIDE, < one workgroup | SIDE, full + ragged | two rays per wave, ragged | 259 rows
BASE = dict(head=True, graw=True, act_ld=1024, dy_ld=32, ray_cols=True, lm=0)


def field_cases():
    cases, seen = [], set()
    for F in (32, 40, 64, 12, 33, 1):
        for N, S in ((3, 96), (5, 100)):
            cases.append(dict(BASE, N=N, S=S, F=F))
    for N, S in SHAPES:
        for F in (32, 40):
            cases.append(dict(BASE, N=N, S=S, F=F))
    for N, S in ((3, 96), (5, 100)):
        for over in (dict(head=False), dict(graw=False), dict(act_ld=0, ray_cols=False), dict(dy_ld=0), dict(ray_cols=False), dict(lm=1),
                     dict(lm=2, F=40)):
            cases.append(dict(dict(BASE, N=N, S=S, F=32), **over))
    out = []
    for c in cases:
        key = tuple(sorted(c.items()))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def case_id(c):
    extra = [f"{k}={c[k]}" for k in ("head", "graw", "act_ld", "dy_ld", "ray_cols", "lm") if c[k] != BASE[k]]
    return f"{c['N']}x{c['S']}-F{c['F']}" + ("-" + "-".join(extra) if extra else "")


def case_seed(c):
    return 1000 * c["N"] + 10 * c["S"] + c["F"]


SKY_RAYS = (1, 2, 17)      # 120 samples each: < one 128-sample workgroup | one full + one ragged | 15 full + a ragged one with dead waves
