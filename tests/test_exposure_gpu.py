"""RawNeRF exposure, random background colours and near_anneal_rate on the device (-m gpu): the new C-ABI entry points
(ucn_composite_rays[_tdist], ucn_composite_rays_backward[_tdist], ucn_resample_domain) and Model.forward on both routes, against
tests/exposure_ref.py.

Tolerances are brackets (tests/test_bracket_gpu.py, helpers.bracket): e_ref = |float32 restatement - its own float64 run| on the same
float32 inputs, e_hip = |HIP - float64 run|, asserted e_hip <= K e_ref + floor with the project's K = 2 and helpers.bracket's floors
for O(1) quantities (1e-6 worst case, 1e-7 on average).  Quantities that are not O(1) are divided by a scale known before anything runs:
distances by far, a gradient by the largest magnitude of its float64 value.  Run with -s for the report lines
(profiles/exposure/parity.txt holds one run's)."""
import numpy as np
import pytest
import torch

import exposure_ref as er
import helpers as H
from oracle import raymarch as rm
from ucnerf_amd import _lib
from ucnerf_amd.internal import march_level as ml
from ucnerf_amd.internal import models

pytestmark = pytest.mark.gpu

K = 2.0
N = 5                    # a partial workgroup: one full wave-quad of rays and one with three dead waves


def _ptr(t):
    return None if t is None else t.data_ptr()


def _case(S, seed):
    """float32 inputs on the host: gains in [0.25, 4], backgrounds in [0, 1], upstream gradients on rgb, depth, acc, weights and (for
    the autograd node's fifth output) the scaled colours."""
    g = torch.Generator().manual_seed(seed)
    rays = rm.synthetic_rays(N, seed=seed + 1)
    c = dict(dirs=rays["directions"], near=rays["near"] + 0.05, far=rays["far"] * (1 + 0.1 * torch.rand(N, 1, generator=g)))
    sd = torch.sort(torch.rand(N, S + 1, generator=g), dim=-1).values
    sd[:, 0], sd[:, -1] = 0.0, 1.0
    # optical depths that leave some rays transparent (acc < 0.6: depth = 300, constant) and some opaque
    c.update(sdist=sd, density=(3.0 * torch.rand(N, 1, generator=g)) * torch.rand(N, S, generator=g) ** 2 * (3.0 / 8.0),
             rgbs=torch.rand(N, S, 3, generator=g), gain=0.25 + 3.75 * torch.rand(N, 3, generator=g), bg=torch.rand(N, 3, generator=g),
             g_rgb=torch.randn(N, 3, generator=g), g_depth=torch.randn(N, generator=g), g_acc=torch.randn(N, generator=g),
             g_w=torch.randn(N, S, generator=g), g_hist=torch.randn(N, S, 3, generator=g))
    c["tdist"] = er.s_to_t(c["sdist"], c["near"], c["far"])                     # float32: the `_tdist` siblings' input
    return c


def _reference(c, dtype, tdist_given, opaque, with_hist):
    """values and autograd gradients of the restatement in `dtype` on the float32 inputs."""
    t = {k: v.to(dtype) for k, v in c.items()}
    leaves = [t[k].requires_grad_() for k in ("density", "rgbs", "gain")]
    tdist = t["tdist"] if tdist_given else er.s_to_t(t["sdist"], t["near"], t["far"])
    w, rgb, depth, acc, scaled = er.composite(t["density"], t["rgbs"], tdist, t["dirs"], t["bg"], bool(opaque), gain=t["gain"])
    loss = (rgb * t["g_rgb"]).sum() + (depth * t["g_depth"]).sum() + (acc * t["g_acc"]).sum() + (w * t["g_w"]).sum()
    if with_hist:
        loss = loss + (scaled * t["g_hist"]).sum()
    gd, gc, gg = torch.autograd.grad(loss, leaves)
    return {k: v.detach() for k, v in dict(weights=w, rgb=rgb, depth=depth, acc=acc, scaled=scaled, g_density=gd, g_rgbs=gc, g_gain=gg).items()}


def _hip_composite(c, tdist_given, opaque, gain=True, bg=True, with_hist=False, alias=False, legacy=False, extras=False):
    """forward + backward through the C ABI; legacy: the entry points of before (ucn_composite[_tdist], ucn_composite_backward[_tdist])."""
    lib, st = _lib.load(), _lib.stream()
    d = {k: v.cuda().contiguous() for k, v in c.items()}
    S = d["density"].shape[1]
    fence = (d["tdist"], d["far"]) if tdist_given else (d["sdist"], d["near"], d["far"])
    fence_b = (d["tdist"],) if tdist_given else (d["sdist"], d["near"], d["far"])
    sfx = "_tdist" if tdist_given else ""
    w, main = torch.empty(N, S, device="cuda"), torch.empty(N, 5, device="cuda")
    ex = torch.empty(N, 4, device="cuda") if extras else None
    g_main = torch.cat([d["g_rgb"], d["g_depth"][:, None], d["g_acc"][:, None]], dim=1).contiguous()
    g_density, g_rgbs = torch.empty(N, S, device="cuda"), torch.empty(N, S, 3, device="cuda")
    rgbs_in = d["rgbs"].clone()
    out = dict(weights=w, main=main, extras=ex, g_density=g_density, g_rgbs=g_rgbs)
    if legacy:
        _lib.check(getattr(lib, "ucn_composite" + sfx)(d["density"].data_ptr(), rgbs_in.data_ptr(), *[t.data_ptr() for t in fence],
                                                      d["dirs"].data_ptr(), 0.5, opaque, N, S, w.data_ptr(), main.data_ptr(), _ptr(ex), st))
        _lib.check(getattr(lib, "ucn_composite_backward" + sfx)(
            d["density"].data_ptr(), rgbs_in.data_ptr(), *[t.data_ptr() for t in fence_b], d["dirs"].data_ptr(), 0.5, opaque, N, S,
            d["g_w"].data_ptr(), g_main.data_ptr(), g_density.data_ptr(), g_rgbs.data_ptr(), st))
    else:
        pg, pb = (d["gain"] if gain else None), (d["bg"] if bg else None)
        scaled = rgbs_in if alias else (torch.empty(N, S, 3, device="cuda") if gain else None)
        g_gain = torch.empty(N, 3, device="cuda") if gain else None
        _lib.check(getattr(lib, "ucn_composite_rays" + sfx)(
            d["density"].data_ptr(), rgbs_in.data_ptr(), *[t.data_ptr() for t in fence], d["dirs"].data_ptr(), _ptr(pg), _ptr(pb), 0.5,
            opaque, N, S, w.data_ptr(), main.data_ptr(), _ptr(ex), _ptr(scaled), st))
        _lib.check(getattr(lib, "ucn_composite_rays_backward" + sfx)(
            d["density"].data_ptr(), d["rgbs"].data_ptr(), *[t.data_ptr() for t in fence_b], d["dirs"].data_ptr(), _ptr(pg), _ptr(pb), 0.5,
            opaque, N, S, d["g_w"].data_ptr(), g_main.data_ptr(), d["g_hist"].data_ptr() if with_hist else None, g_density.data_ptr(),
            g_rgbs.data_ptr(), _ptr(g_gain), st))
        out.update(scaled=scaled, g_gain=g_gain)
    torch.cuda.synchronize()
    out.update(rgb=main[:, :3], depth=main[:, 3], acc=main[:, 4])
    return {k: (None if v is None else v.cpu()) for k, v in out.items()}


def _bracket_all(tag, got, r32, r64, far):
    for q in ("weights", "rgb", "depth", "acc", "scaled", "g_density", "g_rgbs", "g_gain"):
        scale = 1.0
        if q == "depth":
            # 300 where acc < 0.6 on every side (asserted: the float32 sides took the float64 side's branch), else a distance: / far
            assert torch.equal(got[q] == 300, r64[q] == 300) and torch.equal(r32[q] == 300, r64[q] == 300), (tag, "depth branch")
            scale = far.reshape(-1).double()
        elif q.startswith("g_"):
            scale = max(float(r64[q].abs().max()), 1.0)
        H.bracket(f"{tag} {q}", (r32[q].double() - r64[q]).abs() / scale, (got[q].double() - r64[q]).abs() / scale, K)


@pytest.mark.parametrize("opaque", [0, 1])
@pytest.mark.parametrize("tdist_given", [False, True], ids=["sdist", "tdist"])
@pytest.mark.parametrize("S", [5, 64, 65])
def test_composite_rays_forward_and_backward_bracket(S, tdist_given, opaque):
    """S = 5: a partial wave; 64: a full wave, one sample per lane; 65: the first two-samples-per-lane shape.  A per-ray gain and a
    per-ray background, upstream gradients on rgb, depth, acc and weights: values and gradients (density, unscaled colours, gain) inside
    the float32 restatement's own bracket; then the same with a gradient on the returned scaled colours."""
    c = _case(S, 300 + S)
    for with_hist in (False, True):
        r64 = _reference(c, torch.float64, tdist_given, opaque, with_hist)
        r32 = _reference(c, torch.float32, tdist_given, opaque, with_hist)
        got = _hip_composite(c, tdist_given, opaque, with_hist=with_hist)
        tag = f"composite_rays S={S} {'tdist' if tdist_given else 'sdist'} opaque={opaque}{' +g_hist' if with_hist else ''}"
        _bracket_all(tag, got, r32, r64, c["far"])
    if opaque:
        assert not got["g_density"][:, -1].any()                  # the last interval's optical depth is the constant inf


@pytest.mark.parametrize("opaque", [0, 1])
@pytest.mark.parametrize("tdist_given", [False, True], ids=["sdist", "tdist"])
@pytest.mark.parametrize("S", [5, 64, 65])
def test_null_pointers_give_the_bits_of_the_entry_points_of_before(S, tdist_given, opaque):
    c = _case(S, 400 + S)
    old = _hip_composite(c, tdist_given, opaque, legacy=True, extras=True)
    new = _hip_composite(c, tdist_given, opaque, gain=False, bg=False, extras=True)
    for k in ("weights", "main", "extras", "g_density", "g_rgbs"):
        assert torch.equal(old[k], new[k]), k
    assert new["scaled"] is None and new["g_gain"] is None
    # one pointer at a time moves only what it should: the background moves no weight, no gain moves no colour gradient's sign
    only_bg = _hip_composite(c, tdist_given, opaque, gain=False, bg=True)
    assert torch.equal(only_bg["weights"], old["weights"]) and torch.equal(only_bg["acc"], old["acc"])
    assert torch.equal(only_bg["g_rgbs"], old["g_rgbs"])
    if not opaque:                                                # (an opaque last interval leaves the background no weight)
        assert not torch.equal(only_bg["rgb"], old["rgb"])


@pytest.mark.parametrize("S", [5, 65])
def test_scaled_colours_written_over_their_input_give_the_same_pixels(S):
    c = _case(S, 500 + S)
    apart = _hip_composite(c, False, 0)
    alias = _hip_composite(c, False, 0, alias=True)
    for k in ("weights", "main", "scaled", "g_density", "g_rgbs", "g_gain"):
        assert torch.equal(apart[k], alias[k]), k
    assert torch.equal(apart["scaled"], c["rgbs"] * c["gain"][:, None, :])          # one float32 product per colour


# ------------------------------------------------------------------ ucn_resample_domain
def _resample_case(S, n_prev, s_near, jitter, seed):
    g = torch.Generator().manual_seed(seed)
    c = dict(jitter=torch.rand(N, 1, generator=g) if jitter else None, sdist=None, weights=None)
    if n_prev:
        t = torch.sort(s_near + (1 - s_near) * torch.rand(N, n_prev + 1, generator=g), dim=-1).values
        t[:, 0], t[:, -1] = s_near, 1.0
        w = 0.05 + torch.rand(N, n_prev, generator=g)
        c.update(sdist=t, weights=0.9 * w / w.sum(dim=-1, keepdim=True))
    c["dilation"] = float(np.float32(0.0025 + 0.5 * (1 - s_near) / 8)) if n_prev else 0.0
    return c


def _hip_resample(c, S, n_prev, s_near, domain_entry):
    lib, st = _lib.load(), _lib.stream()
    u_tab, max_jitter = ml._u_table(S, c["jitter"] is not None, torch.device("cuda", torch.cuda.current_device()))
    sd, w, jit = (None if c[k] is None else c[k].cuda().contiguous() for k in ("sdist", "weights", "jitter"))
    out = torch.empty(N, S + 1, device="cuda")
    head = (_ptr(sd), _ptr(w), n_prev, c["dilation"], float(np.float32(0.7)), 0.0)
    tail = (u_tab.data_ptr(), _ptr(jit), 0 if jit is None else 1, max_jitter, N, S, out.data_ptr(), st)
    if domain_entry:
        _lib.check(lib.ucn_resample_domain(*head, s_near, *tail))
    else:
        _lib.check(lib.ucn_resample(*head, *tail))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("jitter", [False, True], ids=["eval", "jitter"])
@pytest.mark.parametrize("n_prev", [0, 8])
@pytest.mark.parametrize("S", [8, 64])
@pytest.mark.parametrize("s_near", [0.0, 0.3, 0.95])
def test_resample_domain(s_near, S, n_prev, jitter):
    s_near = float(np.float32(s_near))                          # the float the kernel receives, on every side
    c = _resample_case(S, n_prev, s_near, jitter, 600 + S + n_prev)
    got = _hip_resample(c, S, n_prev, s_near, True)
    assert float(got.min()) >= s_near and float(got.max()) <= 1.0 and bool((got[:, 1:] >= got[:, :-1]).all())
    if s_near == 0.0:
        assert torch.equal(got, _hip_resample(c, S, n_prev, s_near, False))
        return
    anneal = float(np.float32(0.7))
    ref = {}
    for dt in (torch.float32, torch.float64):
        sd, w = (None if c[k] is None else c[k].to(dt) for k in ("sdist", "weights"))
        ref[dt] = er.resample(sd, w, c["dilation"], anneal, 0.0, S, s_near, jitter=c["jitter"], N=N, dtype=dt)
    H.bracket(f"resample_domain s_near={s_near:.2f} S={S} n_prev={n_prev} {'jitter' if jitter else 'eval'}",
              (ref[torch.float32].double() - ref[torch.float64]).abs(), (got.double() - ref[torch.float64]).abs(), K)


# ------------------------------------------------------------------ Model.forward
RAYS = 64
TRAIN_FRAC, RATE, BG_RANGE = 0.03, 0.1, (0.2, 0.8)


@pytest.fixture(scope="module")
def tiny():
    """The `tiny` model of tests/golden/model_tiny.npz with the three options on, non-zero learned offsets, 64 rays with exposures, and every
    draw pinned (the background colours too)."""
    spec = rm.make_spec("tiny")
    sd = dict(H.state_for(H.load("model_tiny.npz"), spec))
    g = torch.Generator().manual_seed(71)
    sd["exposure_scaling_offsets.weight"] = 0.2 * torch.randn(1000, 3, generator=g)
    model, _ = H.hip_model(spec, sd, learned_exposure_scaling=True, bg_intensity_range=BG_RANGE, near_anneal_rate=RATE)
    rays = rm.synthetic_rays(RAYS, seed=72)
    idx = torch.randint(0, 4, (RAYS, 1), generator=g)
    idx[0], idx[1] = 0, 3
    ev = 0.25 + 3.75 * torch.rand(RAYS, 1, generator=g)
    noise = [rm.draw_level_noise(spec, RAYS, lvl, True, g) for lvl in range(spec.num_levels)]
    bgs = [BG_RANGE[0] + (BG_RANGE[1] - BG_RANGE[0]) * torch.rand(RAYS, 3, generator=g) for _ in range(spec.num_levels)]
    batch = H.pin_noise(H.to_dev(rays), noise)
    for lvl, bg in enumerate(bgs):
        batch["march_noise"][lvl]["bg"] = bg.cuda()
    return dict(spec=spec, model=model, rays=rays, idx=idx, ev=ev, noise=noise, bgs=bgs, batch=batch, offsets=sd["exposure_scaling_offsets.weight"])


def _levels(spec):
    return [spec.num_prop_samples] * (spec.num_levels - 1) + [spec.num_nerf_samples]


@pytest.mark.parametrize("route", ["inference", "train"])
def test_model_forward_with_the_three_options(tiny, route):
    """Model.forward with exposure, learned offsets, pinned background colours and near_anneal_rate = 0.1 at train_frac = 0.03 against the
    restatement composed with the project's own per-sample outputs (the history's density, colours, fenceposts, weights): per level the
    fenceposts on [s_near, 1] from the previous level's, the scaled colours from the colours of a run without exposure, the pixels.  On
    the training route also the gradient on exposure_scaling_offsets.weight and on the NeRF field's first density layer, against the
    restatement's float64 gradients pushed through the same graph."""
    spec, model, rays = tiny["spec"], tiny["model"], tiny["rays"]
    model.march_route = route
    model.train(route == "train")
    try:
        with_exp = dict(tiny["batch"], exposure_idx=tiny["idx"].cuda(), exposure_values=tiny["ev"].cuda())
        with torch.set_grad_enabled(route == "train"):
            rend, hist = model(True, with_exp, TRAIN_FRAC, False)
            with torch.no_grad():
                _, hist_plain = model(True, dict(tiny["batch"]), TRAIN_FRAC, False)
        assert model.last_march_route == ("train_graph" if route == "train" else "fused")
        s_near = er.init_s_near(TRAIN_FRAC, RATE)
        s_near32 = float(np.float32(s_near))
        dil = er.dilations(spec.dilation_bias, spec.dilation_multiplier, s_near, _levels(spec))
        anneal = float(np.float32(ml.anneal_of(spec.anneal_slope, TRAIN_FRAC)))
        cpu = lambda t: t.detach().cpu().reshape((RAYS,) + tuple(t.shape[len(rays["origins"].shape) - 1:]))
        prev = None
        for lvl, S in enumerate(_levels(spec)):
            h = {k: cpu(hist[lvl][k]) for k in ("density", "rgb", "sdist", "weights")}
            tag = f"model {route} L{lvl}"
            assert float(h["sdist"].min()) >= s_near32 and float(h["sdist"].max()) <= 1.0
            if lvl == 0:
                assert float(h["sdist"].min()) < s_near32 + 0.05            # the first level starts at the annealed near bound
            plain = cpu(hist_plain[lvl]["rgb"])
            assert torch.equal(cpu(hist_plain[lvl]["sdist"]), h["sdist"])
            sides = {}
            for dt in (torch.float32, torch.float64):
                f = lambda t: None if t is None else t.to(dt)
                sdist = er.resample(f(prev and prev["sdist"]), f(prev and prev["weights"]), float(np.float32(dil[lvl])), anneal,
                                    spec.resample_padding, S, s_near32, jitter=tiny["noise"][lvl].jitter, N=RAYS, dtype=dt)
                scaled = er.exposure_block(f(plain), f(tiny["ev"]), tiny["idx"], f(tiny["offsets"]))
                tdist = er.s_to_t(f(h["sdist"]), f(rays["near"]), f(rays["far"]))
                w, rgb, _, acc, _ = er.composite(f(h["density"]), f(h["rgb"]), tdist, f(rays["directions"]), f(tiny["bgs"][lvl]),
                                                 spec.opaque_background)
                sides[dt] = dict(sdist=sdist, scaled=scaled, weights=w, rgb=rgb, acc=acc)
            got = dict(sdist=h["sdist"], scaled=h["rgb"], weights=h["weights"], rgb=cpu(rend[lvl]["rgb"]), acc=cpu(rend[lvl]["acc"]))
            for q in ("sdist", "scaled", "weights", "rgb", "acc"):
                if q == "scaled" and lvl < spec.num_levels - 1:
                    assert not h["rgb"].any() and not plain.any()          # a proposal level: zero colours, scaled or not
                    continue
                H.bracket(f"{tag} {q}", (sides[torch.float32][q].double() - sides[torch.float64][q]).abs(),
                          (got[q].double() - sides[torch.float64][q]).abs(), K)
            prev = h
        if route != "train":
            return
        # ---- gradients: L = sum(G * rgb of the last level), through the project's backward and through the restatement's
        G = torch.randn(RAYS, 3, generator=torch.Generator().manual_seed(73))
        params = [model.exposure_scaling_offsets.weight, model.nerf_mlp.density_layer[0].weight]
        loss = (rend[-1]["rgb"].reshape(RAYS, 3) * G.cuda()).sum()
        grads = [g.detach().cpu() for g in torch.autograd.grad(loss, params, retain_graph=True)]
        assert not grads[0][0].any() and grads[0][1:4].any() and not grads[0][4:].any()       # row 0 is masked: exactly zero
        h = {k: cpu(hist[-1][k]) for k in ("density", "rgb", "sdist")}
        through = {}
        for dt in (torch.float32, torch.float64):
            f = lambda t: t.to(dt)
            density, scaled = f(h["density"]).requires_grad_(), f(h["rgb"]).requires_grad_()
            tdist = er.s_to_t(f(h["sdist"]), f(rays["near"]), f(rays["far"]))
            _, rgb, _, _, _ = er.composite(density, scaled, tdist, f(rays["directions"]), f(tiny["bgs"][-1]), spec.opaque_background)
            gd, gs = torch.autograd.grad((rgb * f(G)).sum(), [density, scaled])
            # ... pushed through the project's graph from the history's density and scaled colours (the scaled colours' own gradient
            # path of the compositing node: g_rgbs += gain * g, g_gain += sum g * c)
            through[dt] = [g.detach().cpu() for g in torch.autograd.grad(
                [hist[-1]["density"], hist[-1]["rgb"]], params,
                grad_outputs=[gd.float().reshape(hist[-1]["density"].shape).cuda(), gs.float().reshape(hist[-1]["rgb"].shape).cuda()],
                retain_graph=True)]
        for name, got_g, g32, g64 in zip(("exposure_scaling_offsets.weight", "nerf_mlp.density_layer.0.weight"), grads,
                                         through[torch.float32], through[torch.float64]):
            assert not g64[0].any() or name != "exposure_scaling_offsets.weight"
            scale = max(float(g64.abs().max()), 1.0)
            H.bracket(f"model train grad {name}", (g32.double() - g64.double()).abs() / scale, (got_g.double() - g64.double()).abs() / scale, K)
    finally:
        model.march_route = "auto"
        model.eval()


def test_render_image_carries_the_exposure_keys_through_its_chunks(tiny):
    """8 x 8 pixels with a different exposure per pixel, marched in passes of 24 rays (max_chunk_rays; three passes per level):
    render_image's tiling, sharding, passes and un-tiling keep exposure_idx and exposure_values beside their rays -- the frame equals the
    flat batch through Model.forward in ONE pass, and differs from a frame without the keys.  rand = None: the background is the range's
    midpoint, nothing but the pinned rand_vec is random."""
    model, cfg = tiny["model"], tiny["model"].config
    as_frame = lambda t: t.reshape((8, 8) + tuple(t.shape[1:]))
    flat = dict(H.to_dev(tiny["rays"]), rand_vec=tiny["batch"]["rand_vec"], exposure_idx=tiny["idx"].cuda(), exposure_values=tiny["ev"].cuda())
    frame = {k: as_frame(v) for k, v in flat.items()}
    one_pass = model.max_chunk_rays
    assert one_pass >= RAYS
    try:
        model.max_chunk_rays = 24
        got = models.render_image(model, None, frame, None, 1.0, cfg, verbose=False)
        plain = models.render_image(model, None, {k: v for k, v in frame.items() if not k.startswith("exposure")}, None, 1.0, cfg, verbose=False)
    finally:
        model.max_chunk_rays = one_pass
        model.eval()
    with torch.no_grad():
        want, _ = model(None, flat, 1.0, True, eval_camidx=0)
    assert torch.equal(got["rgb"].reshape(RAYS, 3), want[-1]["rgb"].reshape(RAYS, 3))
    assert torch.equal(got["acc"].reshape(RAYS), plain["acc"].reshape(RAYS)) and not torch.equal(got["rgb"], plain["rgb"])


# ------------------------------------------------------------------ rand = False / rand = None with a two-valued background range
def _eval_model(fx):
    spec = rm.make_spec("tiny")
    sd = rm.init_state(spec, seed=int(fx["eval_seed"]))
    assert abs(H.state_checksum(sd) - float(fx["eval_checksum"])) <= 1e-9 * float(fx["eval_checksum"])
    model, _ = H.hip_model(spec, sd, bg_intensity_range=BG_RANGE)
    rays = {k[len("eval_ray_"):]: v for k, v in fx.items() if k.startswith("eval_ray_")}
    return spec, model, rays


@pytest.mark.parametrize("route", ["inference", "train"])
def test_rand_false_draws_the_background_like_the_reference(route):
    """models.py:249 takes the midpoint for `rand is None` alone; rand = False -- what every evaluation caller of the reference passes --
    draws rand(N, 3) per level behind the level's randn(N, 3).  (a) the reference's own rand = False run (exposure.npz eval_false_*): with
    its draws pinned the pixels agree to the project's fp32 parity bar (helpers.RGB_TOL); (b) unpinned after a seed = the same draws
    made here in that order and pinned, bit for bit; (c) rand = None = a model whose range is the midpoint, bit for bit, and the
    reference's rand = None pixels."""
    fx = H.load("exposure.npz")
    spec, model, rays = _eval_model(fx)
    model.march_route = route
    n = rays["origins"].shape[0]
    batch = H.to_dev(rays)
    lo, hi = BG_RANGE
    try:
        with torch.no_grad():
            # (a)
            pinned = dict(batch, rand_vec=torch.cat([fx[f"eval_false_noise{l}_rand_vec"] for l in range(spec.num_levels)], dim=-1).cuda(),
                          march_noise=[dict(bg=(fx[f"eval_false_noise{l}_bg_u"] * (hi - lo) + lo).cuda()) for l in range(spec.num_levels)])
            rend, _ = model(False, pinned, 1.0, False)
            for l in range(spec.num_levels):
                err = H.maxdiff(rend[l]["rgb"].cpu(), fx[f"eval_false_L{l}_rgb"])
                print(f"rand=False {route} L{l}: rgb L-inf vs the reference {err:.3e} (bar {H.RGB_TOL:g})")
                assert err <= H.RGB_TOL
            # (b)
            torch.manual_seed(4321)
            free, _ = model(False, dict(batch), 1.0, False)
            torch.manual_seed(4321)
            vecs, noise = [], []
            for l in range(spec.num_levels):
                vecs.append(torch.randn(n, 3, device="cuda"))
                noise.append(dict(bg=torch.rand(n, 3, device="cuda") * (hi - lo) + lo))
            again, _ = model(False, dict(batch, rand_vec=torch.cat(vecs, dim=-1), march_noise=noise), 1.0, False)
            for l in range(spec.num_levels):
                assert torch.equal(free[l]["rgb"], again[l]["rgb"]), l
            # (c)
            none_batch = dict(batch, rand_vec=torch.cat([fx[f"eval_none_noise{l}_rand_vec"] for l in range(spec.num_levels)], dim=-1).cuda())
            mid, _ = model(None, none_batch, 1.0, False)
            model.bg_intensity_range = ((lo + hi) / 2, (lo + hi) / 2)
            one, _ = model(None, none_batch, 1.0, False)
            for l in range(spec.num_levels):
                assert torch.equal(mid[l]["rgb"], one[l]["rgb"]), l
                assert H.maxdiff(mid[l]["rgb"].cpu(), fx[f"eval_none_L{l}_rgb"]) <= H.RGB_TOL
    finally:
        model.bg_intensity_range = BG_RANGE
        model.march_route = "auto"
