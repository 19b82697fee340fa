"""The layer-wise float64 check of the fused bf16 training kernels (heads_layerwise_ref.py) proven to bite, without a GPU: a float32
torch emulation of each chain (bf16 rounding at the stated points, masks packed by the inverse of the decoders) stays inside the
derived bound with ZERO elements outside on the GPU test's inputs, every planted fault is caught, and the float64 restatements
reproduce the oracle's / the eager graph's formulations to 1e-12."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import heads_layerwise_ref as H  # noqa: E402
from oracle import raymarch as rm  # noqa: E402

BF = torch.bfloat16
b16 = lambda t: t.to(BF).float()


def emulate_field(P, inp, lm=0, fault=None):
    """ucn_train_fwd + ucn_train_bwd in float32 on the CPU, storing what the kernels store."""
    Wb = {k: v.float() for k, v in H.field_weights(P).items()}
    M = inp["feat"].shape[0]
    ray = torch.arange(M) // inp["S"]
    bd1 = inp["bd1"]
    if fault == "bias_shift":                                    # tile 0 of the bottleneck's bias lands 16 accumulator slots off
        a = H.to_acc(bd1, 256)
        a[:32] = a[:32].roll(16)
        bd1 = H.from_acc(a, 256)
    W1h = Wb["W1h"].clone()
    if fault == "swap_k":
        W1h[:, [5, 70]] = W1h[:, [70, 5]]
    fb = b16(inp["feat"])
    a0 = fb @ Wb["Wd0"].t() + inp["bd0"]
    h0 = b16(a0.clamp_min(0))
    ax = h0 @ Wb["Wd1"].t() + bd1
    x = H.rz(ax) if fault == "rtz" else b16(ax)
    a1 = h0 @ Wb["Wc0"].t() + inp["pr0"][ray]
    h1 = b16(a1.clamp_min(0))
    a2 = h1 @ W1h.t() + inp["pr1"][ray]
    if fault != "drop_skip":
        a2 = a2 + h0 @ Wb["Wc1"].t()
    h2 = b16(a2.clamp_min(0))
    y = h2 @ Wb["Wr"].t() + inp["br"]
    raw = x[:, 0].clone()
    pos = lambda a: ~torch.signbit(a)
    out = dict(h0=h0.to(BF), x=x.to(BF), h1=h1.to(BF), h2=h2.to(BF), raw=raw, y=y, feat_bf16=fb.to(BF),
               m0=H.encode_mask(pos(a0)).reshape(M, 2), m1=H.encode_mask(pos(a1)), m2=H.encode_mask(pos(a2)))
    head = inp["head"]
    if head is not None:
        out["density"], out["rgb"] = H.head_density(raw, head, torch.float32), H.head_rgb(y, head, torch.float32)
        k = torch.tensor(1 + 2 * head[3], dtype=torch.float32)
        sg = (out["rgb"] + head[3]) / k
        dy3 = inp["gy"] * k * head[1] * sg * (1 - sg)
        gr = inp["graw"] * (-torch.expm1(-out["density"])) if inp["graw"] is not None else torch.zeros(M)
    else:
        dy3, gr = inp["gy"].float(), (inp["graw"].float() if inp["graw"] is not None else torch.zeros(M))
    dy = b16(torch.cat([dy3, gr[:, None]], dim=1))
    m0, m1, m2 = pos(a0).float(), pos(a1).float(), pos(a2).float()
    d1 = b16(m2 * (dy[:, :3] @ Wb["Wr"]))
    d0 = b16(m1 * (d1 @ Wb["W1h"]))
    gx = d1 @ Wb["W1x"] + d0 @ Wb["W0x"]
    if fault != "no_dy3":
        gx[:, 0] += dy[:, 3]
    gx = b16(gx)
    gh0 = b16(m0 * (gx @ Wb["Wd1"]))
    gfeat = gh0 @ Wb["Wd0"]
    if lm:
        C, F = 2 * lm, gfeat.shape[1]
        gfeat = (gfeat / 6.0).reshape(M, F // C, C).permute(1, 0, 2).contiguous()
    out.update(dy=dy.to(BF), d1=d1.to(BF), d0=d0.to(BF), gx=gx.to(BF), gh0=gh0.to(BF), gfeat=gfeat)
    if fault == "mask_bit":
        out["m1"] = out["m1"].clone()
        out["m1"][M // 2, 1, 2] ^= 1 << 9
    if fault == "stale_rows":                                    # the ragged last wave keeps the row in front of it
        n = M % 32
        assert n
        out["h2"] = out["h2"].clone()
        out["h2"][M - n:] = out["h2"][M - n - 1]
    return out


def judge_field(c, fault=None):
    P = H.field_params(c["F"], H.case_seed(c))
    inp = H.field_host(P, H.field_inputs(c["N"], c["S"], c["F"], H.case_seed(c), head=c["head"], graw=c["graw"]))
    inp["lm"] = c["lm"]
    out = emulate_field(P, inp, lm=c["lm"], fault=fault)
    rep = H.Report()
    Wb = H.field_weights(P)
    H.field_forward_check(rep, H.case_id(c), Wb, inp, out)
    H.field_backward_check(rep, H.case_id(c), Wb, inp, out)
    return rep


@pytest.mark.parametrize("c", H.field_cases(), ids=H.case_id)
def test_field_emulation_is_inside_the_bound_everywhere(c):
    """The reference alone stays inside the bar: zero elements outside, on every input the GPU test uses."""
    rep = judge_field(c)
    assert not rep.failures(), rep.failures()
    for what, (ref, got) in rep.measured.items():
        assert got <= 4 * ref, (what, ref, got)


RAGGED = dict(H.BASE, N=5, S=100, F=32)


@pytest.mark.parametrize("fault,layer", [("swap_k", "fwd h2"), ("drop_skip", "fwd h2"), ("bias_shift", "fwd x"), ("no_dy3", "bwd gx"),
                                         ("mask_bit", "fwd mask of h1"), ("stale_rows", "fwd h2"), ("rtz", "fwd x")])
def test_each_planted_fault_fails_the_check(fault, layer):
    """Faults that sit inside the end-to-end bars (8e-2 relative L2): each is caught, at the layer it was planted in."""
    bad = judge_field(RAGGED, fault).failures()
    assert layer in bad, (fault, bad)
    assert set(judge_field(RAGGED).failures()) == set()


def test_half_a_bf16_ulp_is_two_to_the_minus_eight():
    """The bar's first term: a correctly rounded store is up to 2^-8 |v| off (8 significant bits), not 2^-9."""
    v = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20], dtype=torch.float64)
    err = float((H.rb(v) - v).abs())
    assert float(H.rb(v)) == 1.0 and 2.0 ** -9 * float(v) < err <= float(H.bound(v, v, 0, True))
    assert H.UBF == 2.0 ** -8


def test_mask_codecs_are_inverse():
    g = torch.Generator().manual_seed(3)
    for P in (1, 2, 4):
        bits = torch.rand(37, 64 * P, generator=g) > 0.5
        assert torch.equal(H.decode_mask(H.encode_mask(bits)), bits)
    # one bit, by hand: word 2 of wave half 1, bit 16 + 9 -> tile 5, register 9: feature 160 + (9 & 3) + 8 (9 >> 2) + 4 = 181
    w = torch.zeros(1, 2, 4, dtype=torch.int32)
    w[0, 1, 2] = 1 << 25
    assert H.decode_mask(w).nonzero().tolist() == [[0, 181]]


def test_float64_field_model_reproduces_the_oracle_formulation():
    """field_chain64 (composed colour layers, per-ray terms, masks) against oracle/raymarch.py's dense formulation with the
    reference's concatenations, both float64, no rounding: values and the feature gradient to 1e-12."""
    import torch.nn.functional as Fn
    N, S, Fin = 3, 17, 40
    P = H.field_params(Fin, 5)
    inp = H.field_inputs(N, S, Fin, 5)
    vd = Fn.normalize(torch.randn(N, 3, generator=torch.Generator().manual_seed(9)), dim=-1).double()
    enc = rm.view_encoding(vd, 4)
    names = {"density_layer.0": ("Wd0", "bd0"), "density_layer.2": ("Wd1", "bd1"), "lin_second_stage_0": ("W0", "b0"),
             "lin_second_stage_1": ("W1", "b1"), "rgb_layer": ("Wr", "br")}
    sd = {}
    for n, (w, b) in names.items():
        sd[f"nerf_mlp.{n}.weight"], sd[f"nerf_mlp.{n}.bias"] = P[w].double(), P[b].double()
    f0 = inp["feat"].double().requires_grad_(True)
    head = inp["head"]
    h0 = Fn.relu(rm._lin(f0, sd, "nerf_mlp.density_layer.0"))
    x = rm._lin(h0, sd, "nerf_mlp.density_layer.2")
    dens = Fn.softplus(x[:, 0] + head[0])
    e = enc[:, None, :].expand(N, S, 27).reshape(N * S, 27)
    skip = torch.cat([x, e], dim=-1)
    h1 = Fn.relu(rm._lin(skip, sd, "nerf_mlp.lin_second_stage_0"))
    h2 = Fn.relu(rm._lin(torch.cat([h1, skip], dim=-1), sd, "nerf_mlp.lin_second_stage_1"))
    rgb = torch.sigmoid(head[1] * rm._lin(h2, sd, "nerf_mlp.rgb_layer") + head[2]) * (1 + 2 * head[3]) - head[3]
    ((dens * inp["graw"].double()).sum() + (rgb * inp["gy"].double()).sum()).backward()
    d64, c64, g64 = H.field_chain64(P, inp, enc)
    for got, want in ((d64, dens), (c64, rgb), (g64, f0.grad)):
        assert float((got - want.detach()).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_float64_sky_model_reproduces_the_eager_graph():
    """sky_chain64 (composed m5 / mv over the aux tile) and the explicit compositing backward against train_graph.sky_forward
    and autograd, all float64: 1e-12."""
    from ucnerf_amd.internal import train_graph as tg
    from ucnerf_amd.internal.sky import NeRF
    P = H.sky_params(7)
    inp = H.sky_inputs(5, P, 8)
    net = NeRF(D=8, d_in_view=3, W=256, multires_view=4, output_ch=4, skips=[4]).double()
    with torch.no_grad():
        for l in range(8):
            net.pts_linears[l].weight.copy_(P["W"][l])
            net.pts_linears[l].bias.copy_(P["b"][l])
        for mod, (w, b) in ((net.alpha_linear, ("wa", "ba")), (net.feature_linear, ("Wf", "bf")), (net.views_linears[0], ("Wv", "bv")),
                            (net.rgb_linear, ("wr", "br"))):
            mod.weight.copy_(P[w])
            mod.bias.copy_(P[b])
    torch.set_default_dtype(torch.float64)          # sky_forward makes its own linspace: float64 like the model's, for the pin only
    try:
        inp["tv"] = torch.linspace(0., 1., H.SKY_S)
        with torch.no_grad():
            want = tg.sky_forward(net, inp["o"].double(), inp["d"].double(), inp["cam"].double(), inp["far"].double())
    finally:
        torch.set_default_dtype(torch.float32)
    raw, got = H.sky_chain64(P, inp)
    scale = want.abs().amax(dim=1, keepdim=True).clamp_min(1.0)
    assert float(((got - want) / scale).abs().max()) <= 1e-12
    r = raw.clone().requires_grad_(True)
    (H.sky_composite(r, inp, torch.float64) * inp["g_sky"].double()).sum().backward()
    g = H.sky_composite_backward(raw, inp["g_sky"], inp)
    assert float((g - r.grad).abs().max()) <= 1e-12 * float(r.grad.abs().max())


def emulate_sky(P, inp, fault=None):
    """ucn_sky_train_fwd + ucn_sky_train_bwd in float32 on the CPU."""
    Wb = H.sky_weights(P)
    f = lambda t: t.float()
    N = inp["o"].shape[0]
    M = N * H.SKY_S
    ray = torch.arange(M) // H.SKY_S
    _, pts = H.sky_points(inp, torch.float32)
    p = pts.reshape(M, 3)
    aux = b16(torch.cat([p, torch.ones(M, 1), H.sky_embed(inp["cam"])[ray], torch.zeros(M, 1)], dim=1))
    act = torch.zeros(M, H.SKY_LD)
    act[:, H.SKY_AUX:H.SKY_AUX + 32] = aux
    masks = []
    a = p @ P["W"][0].t() + P["b"][0]
    for l in range(8):
        if l:
            hin = act[:, 256 * (l - 1):256 * l]
            a = torch.cat([hin, aux], dim=1) @ f(Wb["m5"]).t() if l == 5 else hin @ f(Wb["W"][l]).t() + P["b"][l]
        act[:, 256 * l:256 * (l + 1)] = H.rz(a.clamp_min(0)) if (fault == "rtz" and l == 3) else b16(a.clamp_min(0))
        masks.append(~torch.signbit(a))
    sigma = a.clamp_min(0) @ P["wa"].t() + P["ba"]
    v = torch.cat([act[:, 1792:2048], aux], dim=1) @ f(Wb["mv"]).t()
    act[:, H.SKY_HV:H.SKY_HV + 128] = b16(v.clamp_min(0))
    raw = torch.cat([v.clamp_min(0) @ P["wr"].t() + P["br"], sigma], dim=1)
    r = raw.reshape(N, H.SKY_S, 4).clone().requires_grad_(True)
    rgb = H.sky_composite(r, inp, torch.float32)
    (rgb * inp["g_sky"]).sum().backward()
    g_raw = r.grad.reshape(M, 4)
    grad = torch.zeros(M, H.SKY_LD)
    g = b16(g_raw)
    grad[:, H.SKY_G:H.SKY_G + 4] = g
    mv_ = (~torch.signbit(v)).float()
    dv = b16(mv_ * (g[:, :3] @ f(Wb["wr"])))
    grad[:, H.SKY_DV:H.SKY_DV + 128] = dv
    d = b16(masks[7].float() * (dv @ f(Wb["mv"])[:, :256] + g[:, 3:4] @ f(Wb["wa"])))
    grad[:, 1792:2048] = d
    for l in range(6, -1, -1):
        W = f(Wb["m5"])[:, :256] if l + 1 == 5 else f(Wb["W"][l + 1])
        d = b16(masks[l].float() * (d @ W))
        if fault == "stale_rows" and l == 2:
            d[M - M % 32:] = d[M - M % 32 - 1]
        grad[:, 256 * l:256 * (l + 1)] = d
    mask = torch.stack([H.encode_mask(m) for m in masks])
    return dict(act=act.to(BF), raw=raw, mask=mask, mask_v=H.encode_mask(~torch.signbit(v)), sky_rgb=rgb.detach(), g_raw=g_raw, grad=grad.to(BF))


def judge_sky(N, fault=None):
    P = H.sky_params(7)
    inp = H.sky_inputs(N, P, 8)
    out = emulate_sky(P, inp, fault)
    rep = H.Report()
    H.sky_forward_check(rep, f"N={N}", P, inp, out)
    H.sky_backward_check(rep, f"N={N}", P, inp, out)
    return rep, inp, out


@pytest.mark.parametrize("N", H.SKY_RAYS)
def test_sky_emulation_is_inside_the_bound_everywhere(N):
    rep, inp, out = judge_sky(N)
    assert not rep.failures(), rep.failures()
    for what, (ref, got) in rep.measured.items():
        assert got <= 4 * ref, (what, ref, got)
    if N >= 3:                                                   # the two special rays are what they are meant to be
        raw = out["raw"].reshape(N, H.SKY_S, 4)
        assert float(raw[1, :, 3].max()) < 0 and float(out["sky_rgb"][1].abs().max()) == 0
        assert float(raw[2, 0, 3]) > 1.0


@pytest.mark.parametrize("fault,layer", [("rtz", "sky fwd h_3"), ("stale_rows", "sky bwd d2")])
def test_planted_sky_faults_fail_the_check(fault, layer):
    bad = judge_sky(2, fault)[0].failures()
    assert layer in bad, (fault, bad)
