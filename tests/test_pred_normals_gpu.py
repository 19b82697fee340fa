"""Predicted normals (MLP.enable_pred_normals) on the device: ucn_pred_normals through the C ABI, the inference routes (Model.forward in
one and in several passes, MLP.forward, render_image), the training graph with the orientation loss in fp32 and under bf16 autocast, the
two training nodes, and a flag-off render that must never reach the new entry point.

Tolerances (the scheme of oracle/truth64.py and tests/test_bracket_gpu.py): an error is measured against the float64 restatement
(tests/pred_normals_ref.py) as max |got - truth| / max |truth| and may reach 4x the float32 reference's own error against the same float64
values (pred_normals_ref.allowed).  The composed A h + c sums 64 terms where the reference sums 64 and then 64: another order, the same
conditioning.  Quantities computed from the DEVICE's own gather (Model.forward, MLP.forward, the training graph) see features that differ from the
fixture's (the CPU restatement of the grid op) in the last digits, and a level-1 march its own resampled fenceposts: their float64 truth is
formed from the features and fenceposts the device itself produced (captured at the head's call), and the allowed error stays 4x the
float32 reference's own error on the fixture's inputs -- no constant is added.  The bracket was taken on the fixture's 64-wide bottleneck;
the shipped 256-wide one was not bracketed.  Unit vectors are compared where the reference's |grad_pred| exceeds
the generator's threshold g_min: |dn| <= 2 |dg| / |g|.  Under bf16 autocast the gradients are compared to the same reference gradients by
cosine >= 0.99 and norm ratio within 5e-2 per tensor: the bars of tests/test_train_full_size.py's bf16 case."""
import ctypes
import functools

import pytest
import torch

import pred_normals_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def truth():
    return pr.restate(torch.float64)


@functools.lru_cache(maxsize=None)
def model_on_device():
    return pr.build_model(DEV).eval()


def t(k):
    return torch.from_numpy(pr.fixture()[k])


def check(name, got, lvl_key, extra=0.0):
    """got against the float64 truth, bracketed by the fixture's float32 value; prints the figures before it asserts"""
    ref64, ref32 = truth()[lvl_key], t(lvl_key)
    err, bar = pr.rel_err(got, ref64), pr.allowed(ref32, ref64) + extra
    print(f"{name}: measured {err:.3e} allowed {bar:.3e} (float32 reference's own {pr.rel_err(ref32, ref64):.3e})")
    assert err <= bar, (name, err, bar)
    return err, bar


def check_units(name, got, lvl, bar_g):
    strong = t(f"L{lvl}_grad_pred").norm(dim=-1) > float(pr.fixture()["g_min"])
    assert float((~strong).double().mean()) <= 0.05
    ref64 = truth()[f"L{lvl}_normals_pred"]
    err = float((got.double().cpu() - ref64)[strong].abs().max())
    bar = 2 * bar_g * float(truth()[f"L{lvl}_grad_pred"].abs().max()) / float(pr.fixture()["g_min"])
    print(f"{name}: unit vectors measured {err:.3e} allowed {bar:.3e}")
    assert err <= bar, (name, err, bar)


def planes(feat, L, C, layout):
    """the fixture's [N, S, L*C (+ L)] features as the kernels' [L + scale planes][B][C] buffer, layout 0 (b = ray*S + s) or 2 (b = s*N + ray)"""
    N, S, F = feat.shape
    parts = [feat[..., :L * C].reshape(N, S, L, C)]
    if F > L * C:
        nsp = (L + C - 1) // C
        pad = torch.zeros(N, S, nsp * C)
        pad[..., :L] = feat[..., L * C:]
        parts.append(pad.reshape(N, S, nsp, C))
    p = torch.cat(parts, dim=2)
    p = p.permute(2, 0, 1, 3) if layout == 0 else p.permute(2, 1, 0, 3)
    return p.contiguous().to(DEV)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("layout", [0, 2])
def test_kernel_through_the_c_abi(layout, mode):
    from ucnerf_amd import _lib
    lib = _lib.load()
    model = model_on_device()
    for lvl, mlp in enumerate((model.prop_mlp_0, model.nerf_mlp)):
        feat = t(f"L{lvl}_features")
        N, S, _ = feat.shape
        fb = planes(feat, mlp.encoder.num_levels, mlp.encoder.level_dim, layout)
        A, c = mlp.pred_head()
        g, n = torch.full((N, S, 3), float("nan"), device=DEV), torch.full((N, S, 3), float("nan"), device=DEV)
        _lib.check(lib.ucn_pred_normals(ctypes.byref(mlp.field(mode)), A.data_ptr(), c.data_ptr(), fb.data_ptr(), N, S, layout,
                                        g.data_ptr(), n.data_ptr(), _lib.stream()))
        torch.cuda.synchronize()
        _, bar = check(f"ucn_pred_normals level {lvl} layout {layout} mode {mode}", g, f"L{lvl}_grad_pred")
        check_units(f"ucn_pred_normals level {lvl}", n, lvl, bar)


def test_kernel_clamp_and_empty_call():
    """a hand-made sample with grad_pred = 0 (zero weights and bias): normals_pred is 0, not NaN; an empty call launches nothing"""
    from ucnerf_amd import _lib
    from ucnerf_amd.internal import models
    lib = _lib.load()
    mlp = models.NerfMLP(enable_pred_normals=True, grid_level_dim=2, grid_log2_hashmap_size=8, grid_disired_resolution=64).to(DEV)
    L, C = mlp.encoder.num_levels, mlp.encoder.level_dim
    fb = torch.rand(L, 300, C, device=DEV)
    A, c = torch.zeros(3, 64, device=DEV), torch.zeros(3, device=DEV)
    g, n = torch.full((300, 1, 3), float("nan"), device=DEV), torch.full((300, 1, 3), float("nan"), device=DEV)
    d = mlp.field()
    _lib.check(lib.ucn_pred_normals(ctypes.byref(d), A.data_ptr(), c.data_ptr(), fb.data_ptr(), 300, 1, 0, g.data_ptr(), n.data_ptr(), _lib.stream()))
    assert torch.equal(g.cpu(), torch.zeros(300, 1, 3)) and torch.equal(n.abs().cpu(), torch.zeros(300, 1, 3))
    _lib.check(lib.ucn_pred_normals(ctypes.byref(d), None, None, None, 0, 1, 0, None, None, _lib.stream()))
    assert lib.ucn_pred_normals(ctypes.byref(d), A.data_ptr(), c.data_ptr(), fb.data_ptr(), 300, 1, 1, g.data_ptr(), n.data_ptr(), _lib.stream()) != 0


def hidden_rows_outputs(C, scale_planes, layout):
    """ucn_pred_normals on pred_normals_ref.hidden_rows_case: (the case, A, c as handed over, grad_pred, normals_pred on the host).  c is
    moved away from 0 so that no |grad_pred| is small: the unit vectors are then as well conditioned as grad_pred itself."""
    from ucnerf_amd import _lib
    case = pr.hidden_rows_case(C, scale_planes)
    A, c = case["A"][:3].contiguous(), case["c"][:3] + torch.tensor([2.0, -2.0, 2.0])
    d, keep = pr.hidden_rows_field(case, DEV)
    fb, Ad, cd = pr.hidden_rows_planes(case, DEV), A.to(DEV), c.to(DEV)
    g, n = (torch.full((pr.HR_N, pr.HR_S, 3), float("nan"), device=DEV) for _ in range(2))
    _lib.check(_lib.load().ucn_pred_normals(ctypes.byref(d), Ad.data_ptr(), cd.data_ptr(), fb.data_ptr(), pr.HR_N, pr.HR_S, layout,
                                            g.data_ptr(), n.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    return case, A, c, g.cpu(), n.cpu()


@pytest.mark.parametrize("layout", [0, 2])
@pytest.mark.parametrize("scale_planes", [False, True])
@pytest.mark.parametrize("C", [1, 2, 4, 8])
def test_shared_body_corners(C, scale_planes, layout):
    """the kernel body the heads share (csrc/hidden_rows.h) where the fixtures do not reach: every level width, P * C from 3, scale planes
    in a hand-filled descriptor, a second workgroup that is almost empty, hidden units at exactly 0; bracketed like the tests above"""
    case, A, c, g, n = hidden_rows_outputs(C, scale_planes, layout)
    g32, g64 = (pr.hidden_rows_ref(case, dt, A, c, layout) for dt in (torch.float32, torch.float64))
    for name, got, r32, r64 in (("grad_pred", g, g32, g64), ("normals_pred", n, pr.neg_normalize(g32), pr.neg_normalize(g64))):
        err, bar = pr.rel_err(got, r64), pr.allowed(r32, r64)
        print(f"shared body C {C} P {case['P']} layout {layout} {name}: measured {err:.3e} allowed {bar:.3e}")
        assert err <= bar, (name, err, bar)


class captured:
    """While active, every call of march_level.pred_normals (the fused march, MLP.forward) also leaves a copy of the feature buffer it
    read: `.calls` = [(buffer, rays slice, n, S, layout)] in call order."""

    def __enter__(self):
        from ucnerf_amd.internal import march_level as ml
        self.ml, self.orig, self.calls = ml, ml.pred_normals, []

        def spy(desc, head, feat, sl, n, S, layout, grad_pred, normals_pred, stream):
            self.calls.append((feat.clone(), sl, n, S, layout))
            return self.orig(desc, head, feat, sl, n, S, layout, grad_pred, normals_pred, stream)
        ml.pred_normals = spy
        return self

    def __exit__(self, *exc):
        self.ml.pred_normals = self.orig
        return False

    def features(self, i, mlp):
        """call i's buffer as [n, S, F] features in density_layer's column order"""
        fb, _, n, S, layout = self.calls[i]
        L, C = mlp.encoder.num_levels, mlp.encoder.level_dim
        return pr.unplanes(fb.cpu(), L, C, mlp.density_layer[0].in_features, n, S, layout)


@functools.lru_cache(maxsize=None)
def marched(chunk=10240, rays_fastest=True, compact=0.0, overlap=False, history=True):
    """(renderings, history, the float64 truth of the march's OWN features and fenceposts -- single-pass marches with a history only)"""
    model = model_on_device()
    model.max_chunk_rays, model.rays_fastest, model.compact_min_weight, model.overlap_streams = chunk, rays_fastest, compact, overlap
    try:
        with torch.no_grad(), captured() as cap:
            if history:
                rend, hist = model(False, pr.batch(DEV), 1.0, True)
            else:
                rend, hist = model._march(False, pr.batch(DEV), 1.0, True, None, want_history=False)
        torch.cuda.synchronize()
    finally:
        model.max_chunk_rays, model.rays_fastest, model.compact_min_weight, model.overlap_streams = 10240, True, 0.0, False
    own = None
    if history and chunk >= 37:
        assert len(cap.calls) == 2
        feats = [cap.features(i, m) for i, m in enumerate((model.prop_mlp_0, model.nerf_mlp))]
        own = pr.restate(torch.float64, features=feats, sdist=[h["sdist"] for h in hist])
    return rend, hist, own


def check_own(name, got, key, own, ref_key=None):
    """got against the float64 truth of the device's OWN inputs; allowed: 4x the float32 reference's error against the float64 truth of ITS
    inputs (the fixture's) -- the same function, the same weights, inputs that differ in the last digits"""
    ref_key = key if ref_key is None else ref_key
    err, bar = pr.rel_err(got, own[key]), pr.allowed(t(ref_key), truth()[ref_key])
    print(f"{name}: measured {err:.3e} allowed {bar:.3e} (against the truth of the device's own features)")
    assert err <= bar, (name, err, bar)
    return bar


def test_model_forward_single_and_multi_pass():
    import helpers as H
    rend, hist, own = marched()
    assert model_on_device().last_march_route == "fused"
    for lvl in range(2):
        bar = check_own(f"Model.forward level {lvl} grad_pred", hist[lvl]["grad_pred"], f"L{lvl}_grad_pred", own)
        strong = t(f"L{lvl}_grad_pred").norm(dim=-1) > float(pr.fixture()["g_min"])
        nerr = float((hist[lvl]["normals_pred"].double().cpu() - own[f"L{lvl}_normals_pred"])[strong].abs().max())
        nbar = 2 * bar * float(own[f"L{lvl}_grad_pred"].abs().max()) / float(pr.fixture()["g_min"])
        print(f"Model.forward level {lvl}: unit vectors measured {nerr:.3e} allowed {nbar:.3e}")
        assert nerr <= nbar
        check_own(f"Model.forward level {lvl} composited", rend[lvl]["normals_pred"], f"L{lvl}_render_normals_pred", own)
        # the levels' colours -- level 0 is a proposal field with its colour layers, composited like the last level's -- at the project's
        # fp32 parity bar (helpers.RGB_TOL), against the reference's recorded values
        for got, key in ((hist[lvl]["rgb"], f"L{lvl}_rgb"), (rend[lvl]["rgb"], f"L{lvl}_render_rgb")):
            err = float((got.cpu() - t(key)).abs().max())
            print(f"Model.forward {key}: L-inf {err:.3e} allowed {H.RGB_TOL:.0e}")
            assert err <= H.RGB_TOL and float(t(key).abs().max()) > 0.1
    # 37 rays in passes of 16 (also with the gather of the next pass on a second stream), and the sample-fastest layout: the same samples
    # through the same arithmetic
    for kw in (dict(chunk=16), dict(chunk=16, rays_fastest=False), dict(rays_fastest=False), dict(chunk=16, overlap=True)):
        rend2, hist2, _ = marched(**kw)
        for lvl in range(2):
            for k in ("grad_pred", "normals_pred"):
                assert torch.equal(hist2[lvl][k], hist[lvl][k]), (kw, lvl, k)
            assert torch.equal(rend2[lvl]["normals_pred"], rend[lvl]["normals_pred"]), kw
    # render_image's march (no history) with the colour layers compacted: the head still runs for every sample
    for kw in (dict(history=False), dict(history=False, compact=1e-3), dict(history=False, compact=1e-3, chunk=16)):
        rend3, _, _ = marched(**kw)
        for lvl in range(2):                 # 8 eps of an O(1) value: the compacted route's weights come from its own density-only pass
            assert float((rend3[lvl]["normals_pred"] - rend[lvl]["normals_pred"]).abs().max()) <= 8 * pr.EPS32, (kw, lvl)


def test_mlp_forward():
    import helpers as H
    model = model_on_device()
    vd = t("ray_viewdirs").to(DEV)
    means, stds, glo = t("F_means").to(DEV), t("F_stds").to(DEV), t("F_glo").to(DEV)
    sd = pr.state()
    for lvl, (name, mlp, gv) in enumerate((("prop", model.prop_mlp_0, None), ("nerf", model.nerf_mlp, glo))):
        with captured() as cap:
            res = mlp(False, means, stds, viewdirs=vd, glo_vec=gv)
        ref32 = t(f"F_{name}_grad_pred")
        assert res["grad_pred"].shape == ref32.shape and res["normals"] is None and len(cap.calls) == 1
        # the float64 truth of the features the device gathered for these Gaussians; allowed: 4x the reference's own error on the same
        # field's marched samples (the fixture holds no features of these points)
        p64 = {k: sd[f"{pr.LEVELS[lvl]}.{k}"].double() for k in pr.HEAD_PARAMS}
        _, g64, n64 = pr.head(cap.features(0, mlp).double().reshape(ref32.shape[:-1] + (-1,)), p64)
        err, bar = pr.rel_err(res["grad_pred"], g64), pr.allowed(t(f"L{lvl}_grad_pred"), truth()[f"L{lvl}_grad_pred"])
        print(f"MLP.forward {name}: grad_pred measured {err:.3e} allowed {bar:.3e} (against the truth of the device's own features)")
        assert err <= bar
        strong = ref32.norm(dim=-1) > float(pr.fixture()["g_min"])
        assert float((~strong).double().mean()) <= 0.05
        nerr = float((res["normals_pred"].cpu().double() - n64)[strong].abs().max())
        assert nerr <= 2 * bar * float(g64.abs().max()) / float(pr.fixture()["g_min"]), nerr
        # against the reference's recorded values (its own gather): the project's fp32 parity bar
        for k in ("grad_pred", "rgb", "density"):
            e = float((res[k].cpu() - t(f"F_{name}_{k}")).abs().max())
            print(f"MLP.forward {name} {k}: L-inf against the reference {e:.3e} allowed {H.RGB_TOL:.0e}")
            assert e <= H.RGB_TOL


def test_render_image_returns_the_composited_normals():
    from ucnerf_amd.internal import configs, models
    model = model_on_device()
    b = pr.batch(DEV)
    H, W = 8, 6
    idx = torch.arange(H * W, device=DEV) % 37                       # pixel i = the fixture's ray i % 37, its cone-basis draws pinned
    flat = {k: v[idx] for k, v in b.items()}
    frame = {k: v.reshape(H, W, -1) for k, v in flat.items()}
    out = models.render_image(model, None, frame, False, 1.0, configs.Config(), verbose=False)
    model.eval()                                                     # (render_image leaves the model in training mode, like the reference)
    assert out["normals_pred"].shape == (H, W, 3)
    # the frame is marched in tile order, 48 rays at once: per ray the arithmetic of the 37-ray march that test_model_forward brackets
    rend, _, _ = marched()
    got = out["normals_pred"].reshape(H * W, 3)
    for lo in (0, 37):
        part = got[lo:lo + 37]
        assert float((part - rend[-1]["normals_pred"][:part.shape[0]]).abs().max()) <= 8 * pr.EPS32       # 8 eps of an O(1) value


def _train_step(autocast):
    from ucnerf_amd.internal import configs, train_utils
    from ucnerf_amd.internal import train_graph as tg
    cfg = configs.Config()
    cfg.orientation_coarse_loss_mult, cfg.orientation_loss_mult = pr.fixture()["mults"].tolist()
    model = pr.build_model(DEV, config=cfg).train()
    b = pr.batch(DEV)
    feats, orig = [], tg.field_heads_pred

    def spy(mlp, feat, viewdirs, N, S, chan=None, glo=None):         # the features the graph's heads read, [N*S, F]
        feats.append(feat.detach().float().reshape(N, S, -1).cpu())
        return orig(mlp, feat, viewdirs, N, S, chan, glo)
    tg.field_heads_pred = spy
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            rend, hist = model(False, b, 1.0, False)
            loss = train_utils.orientation_loss(b, model, hist, cfg)
    finally:
        tg.field_heads_pred = orig
    assert model.last_march_route == "train_graph" and len(feats) == 2
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}
    return float(loss.detach()), hist, grads, feats, rend


def test_training_graph_fp32():
    import helpers as H
    loss, hist, grads, feats, rend = _train_step(False)
    own = pr.restate(torch.float64, features=feats, sdist=[h["sdist"] for h in hist])
    want, ref_own = float(own["loss_total"]), abs(float(t("loss_total")) - float(truth()["loss_total"])) / float(truth()["loss_total"])
    print(f"orientation loss fp32: got {loss:.8e} truth of the device's features {want:.8e}; measured {abs(loss - want) / want:.3e} "
          f"allowed {4 * max(ref_own, pr.EPS32):.3e}")
    assert abs(loss - want) <= 4 * max(ref_own, pr.EPS32) * want
    for lvl in range(2):
        check_own(f"training level {lvl} grad_pred", hist[lvl]["grad_pred"].detach(), f"L{lvl}_grad_pred", own)
    for name in pr.LEVELS:
        for k in pr.HEAD_PARAMS:
            check_own(f"d loss / d {name}.{k}", grads[f"{name}.{k}"], f"grad_{name}.{k}", own)
    for name in pr.LEVELS:
        # the table: no float64 restatement of the grid op's backward; the reference's float32 gradient (of ITS features, which differ
        # from the device's in the last digits), allowed 4x the reference's own error on density_layer.0.weight -- the same upstream
        # gradients, summed over the samples -- plus the 1e-6 floor tests/test_bracket_gpu.py gives a table gradient
        k = f"{name}.encoder.embeddings"
        kw = f"grad_{name}.density_layer.0.weight"
        err, bar = pr.rel_err(grads[k], t("grad_" + k)), pr.allowed(t(kw), truth()[kw]) + 1e-6
        print(f"d loss / d {k}: measured {err:.3e} allowed {bar:.3e} (both sides float32)")
        assert err <= bar, (k, err)
    for k in ("nerf_mlp.lin_second_stage_0.weight", "nerf_mlp.rgb_layer.weight"):
        assert k not in grads or float(grads[k].abs().max()) == 0.0             # the loss does not read the colours
    # the levels' colours in the training graph, level 0 included (helpers.RGB_TOL, as on the fused march)
    for lvl in range(2):
        for got, key in ((hist[lvl]["rgb"], f"L{lvl}_rgb"), (rend[lvl]["rgb"], f"L{lvl}_render_rgb")):
            err = float((got.detach().cpu() - t(key)).abs().max())
            print(f"training graph {key}: L-inf {err:.3e} allowed {H.RGB_TOL:.0e}")
            assert err <= H.RGB_TOL


def test_training_graph_bf16():
    loss, hist, grads, _, _ = _train_step(True)
    want = float(t("loss_total"))
    print(f"orientation loss bf16: got {loss:.6e} reference {want:.6e}")
    assert abs(loss - want) <= 5e-2 * want
    for name in pr.LEVELS:
        for k in pr.HEAD_PARAMS + ("encoder.embeddings",):
            g, w = grads[f"{name}.{k}"].double().reshape(-1), t(f"grad_{name}.{k}").double().reshape(-1)
            cos, ratio = float((g * w).sum() / (g.norm() * w.norm() + 1e-30)), float(g.norm() / w.norm())
            print(f"bf16 d loss / d {name}.{k}: cosine {cos:.5f} norm ratio {ratio:.4f}")
            assert cos >= 0.99 and abs(ratio - 1.0) <= 5e-2, (name, k, cos, ratio)


def test_nodes_on_the_device():
    from ucnerf_amd.internal import train_utils
    from ucnerf_amd.internal.march_nodes import _NegNormalize
    g = torch.Generator().manual_seed(11)
    x = torch.rand(1000, 3, generator=g) - 0.5
    x[0] = 0.0                                                       # the clamp
    dn = torch.rand(1000, 3, generator=g) - 0.5
    xd = x.to(DEV).requires_grad_(True)
    n = _NegNormalize.apply(xd)
    (gx,) = torch.autograd.grad(n, xd, dn.to(DEV))
    x64 = x.double().requires_grad_(True)
    n64 = pr.neg_normalize(x64)
    (gx64,) = torch.autograd.grad(n64, x64, dn.double())
    assert torch.equal(n[0].cpu(), torch.zeros(3)) and bool(torch.isfinite(gx).all())
    assert torch.allclose(gx[0].cpu().double(), -dn[0].double() / pr.EPS32, rtol=1e-6)
    # one float32 rounding of values formed in double: 2 eps relative to the vector's largest component
    assert float((n.detach().cpu().double() - n64.detach()).abs().max()) <= 2 * pr.EPS32
    scale = gx64[1:].abs().amax(dim=-1, keepdim=True)
    assert float(((gx.cpu().double()[1:] - gx64[1:]).abs() / scale).max()) <= 4 * pr.EPS32
    N, S = 37, 70                                                    # more than one sample per lane, a partial workgroup of rays
    w, nn_ = torch.rand(N, S, generator=g), pr.neg_normalize(torch.rand(N, S, 3, generator=g) - 0.5)
    v, gl = pr.neg_normalize(torch.rand(N, 3, generator=g) - 0.5), torch.rand(N, generator=g)
    wd, nd = w.to(DEV).requires_grad_(True), nn_.to(DEV).requires_grad_(True)
    out = train_utils._Orientation.apply(wd, nd, v.to(DEV))
    gw, gn = torch.autograd.grad(out, (wd, nd), gl.to(DEV))
    w64, n64 = w.double().requires_grad_(True), nn_.double().requires_grad_(True)
    out64 = pr.orientation_term(w64, n64, v.double())
    gw64, gn64 = torch.autograd.grad(out64, (w64, n64), gl.double())
    # forward: float32 dots of three terms (3 eps each, squared: 8 eps), summed in double, rounded once; backward: elementwise float32
    assert pr.rel_err(out.detach(), out64.detach()) <= 16 * pr.EPS32
    assert pr.rel_err(gw, gw64) <= 16 * pr.EPS32 and pr.rel_err(gn, gn64) <= 16 * pr.EPS32


def test_flag_off_never_calls_the_entry_point(monkeypatch):
    from ucnerf_amd import _lib
    lib = _lib.load()
    calls = []

    def trap(*a):
        calls.append(a)
        raise AssertionError("ucn_pred_normals called for a field without enable_pred_normals")
    monkeypatch.setattr(lib, "ucn_pred_normals", trap, raising=True)
    model = pr.build_model(DEV, flag=False).eval()
    with torch.no_grad():
        rend, hist = model(False, pr.batch(DEV), 1.0, True)
    torch.cuda.synchronize()
    assert calls == [] and "normals_pred" not in rend[-1]
    assert hist[-1]["grad_pred"] is None and hist[-1]["normals_pred"] is None
    # the same model's densities are the flagged model's: the head changes nothing else
    _, hist_on, _ = marched()
    assert torch.equal(hist[0]["density"], hist_on[0]["density"]) and torch.equal(hist[1]["density"], hist_on[1]["density"])
