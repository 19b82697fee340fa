"""MLP.scale_featurization on the GPU: the level constants (ucn_level_scale), the scale-feature kernels
(ucn_march_scale_features / _tdist, ucn_points_scale_features), Model.forward and one training step against the reference
(tests/golden/*_scalefeat*.npz, make_scalefeat_golden.py) and predict_density against the restatement (tests/scalefeat_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
import scalefeat_ref as sf
from oracle import raymarch as rm
from test_glo_cpu import fixture
from test_glo_gpu import f32_engine
from test_train_step import check_grad, losses_of, train_batch

pytestmark = pytest.mark.gpu

FIELDS = [("tiny", "nerf"), ("tinyR", "nerf"), ("tinyR", "prop")]          # (L, C) = (16, 2), (10, 4), (6, 4)


def field_of(kind, which):
    spec = rm.make_spec(kind)
    return spec, (spec.nerf if which == "nerf" else spec.props[0])


def grid_desc(fs, emb):
    """ucn_field_t with the grid part filled in (all the scale kernels read), and what keeps its host arrays alive."""
    from ucnerf_amd import _lib
    pls, offsets, sizes, _ = fs.layout()
    off = np.ascontiguousarray(offsets.numpy().astype(np.int32))
    gs = np.ascontiguousarray(sizes.numpy().astype(np.int32))
    d = _lib.UcnField()
    d.embeddings, d.offsets_host, d.grid_sizes_host = emb.data_ptr(), off.ctypes.data, gs.ctypes.data
    d.num_levels, d.level_dim, d.base_resolution = fs.num_grid_levels, fs.grid_level_dim, fs.grid_base_resolution
    d.log2_per_level_scale = float(np.log2(pls))
    return d, (off, gs, emb)


# ---------------------------------------------------------------------------------------------------- 1. level constants
@pytest.mark.parametrize("kind,which", FIELDS)
def test_level_scale_against_float64(kind, which):
    """k[l] against a float64 numpy evaluation; bar: 4 x the error the reference arithmetic (torch's fp32 index_add mean)
    makes against the same float64 on this table, plus 1e-7 relative.  Two calls agree bit for bit (fixed summation order)."""
    from ucnerf_amd import _lib
    lib = _lib.load()
    spec, fs = field_of(kind, which)
    emb = rm.init_state(spec, seed=17)[fs.prefix + ".encoder.embeddings"]             # U(-1, 1)
    _, offsets, _, _ = fs.layout()
    L, C = fs.num_grid_levels, fs.grid_level_dim
    e64 = emb.numpy().astype(np.float64)
    k64 = np.array([np.sqrt(sf.INIT_STD ** 2 + (e64[offsets[l]:offsets[l + 1]] ** 2).sum(-1).mean()) for l in range(L)])
    k_ref = sf.level_scale(fs, emb).double().numpy()
    dev = emb.cuda()
    off = np.ascontiguousarray(offsets.numpy().astype(np.int32))
    outs = []
    for _ in range(2):
        out, ws = torch.full((L,), float("nan"), device="cuda"), torch.empty(_lib.LEVEL_SCALE_WS_FLOATS, device="cuda")
        _lib.check(lib.ucn_level_scale(dev.data_ptr(), off.ctypes.data, L, C, sf.INIT_STD, out.data_ptr(), ws.data_ptr(), _lib.stream()))
        outs.append(out)
    torch.cuda.synchronize()
    e_ref = float(np.abs(k_ref - k64).max())
    e_hip = float(np.abs(outs[0].double().cpu().numpy() - k64).max())
    print(f"LEVEL_SCALE {kind}/{which}: e_ref {e_ref:.3e}  e_hip {e_hip:.3e}")
    assert e_hip <= 4 * e_ref + 1e-7 * float(k64.max()), (e_hip, e_ref)
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------- 2. scale planes
def march_inputs(N, S, seed):
    g = torch.Generator().manual_seed(seed)
    rays = H.to_dev(rm.synthetic_rays(N, seed=seed))
    sdist = torch.sort(torch.rand(N, S + 1, generator=g), dim=-1).values.cuda()
    rvec = torch.randn(N, 3, generator=g).cuda()
    return rays, sdist, rvec


@pytest.mark.parametrize("kind,which", FIELDS)
def test_scale_planes_against_the_restatement(kind, which):
    """N = 37 rays x S = 5 (partial waves): every layout against the restatement on the kernel's OWN Gaussians (ucn_cast_probe's
    contracted stds) and the same k.  Bar per entry 2e-6 k[l]: erf_pos is within 1.5e-7 absolute and the fast rsq moves the
    argument by ~1e-6 relative while |x erf'(x)| < 0.5; together, doubled by 2w - 1, ~1.3e-6."""
    from ucnerf_amd import _lib
    lib, st = _lib.load(), _lib.stream()
    spec, fs = field_of(kind, which)
    emb = rm.init_state(spec, seed=19)[fs.prefix + ".encoder.embeddings"]
    L, C = fs.num_grid_levels, fs.grid_level_dim
    P = (L + C - 1) // C
    N, S = 37, 5
    B = N * S
    rays, sdist, rvec = march_inputs(N, S, 23)
    near, far, o, d, rad = (rays[k].reshape(N, -1).contiguous() for k in ("near", "far", "origins", "directions", "radii"))
    basis = torch.empty(N, 6, device="cuda")
    _lib.check(lib.ucn_cone_basis(rays["cam_dirs"].data_ptr(), rvec.data_ptr(), N, basis.data_ptr(), st))
    probe = torch.empty(N, S, 6, 10, device="cuda")              # UCN_CAST_PROBE_FLOATS
    geom = [sdist, near, far, o, d, basis, rad]
    _lib.check(lib.ucn_cast_probe(*[t.data_ptr() for t in geom], None, None, 0.5, N, S, probe.data_ptr(), st))
    k = sf.level_scale(fs, emb)
    k_dev = k.cuda()
    desc, keep = grid_desc(fs, emb.cuda())
    _, _, grid_sizes, _ = fs.layout()
    torch.cuda.synchronize()
    stds = probe[..., 8].double().cpu()                                        # contracted std / 2, as the damping sees it
    want = (2 * rm.level_damping(stds, grid_sizes).mean(dim=-2) - 1) * k.double()            # [N, S, L]
    bar = 2e-6 * k.double()

    def run(layout, tdist=None):
        n_out = B * L if layout == 1 else P * B * C
        out = torch.full((n_out + 64,), float("nan"), device="cuda")            # + a guard band behind the planes
        if tdist is None:
            _lib.check(lib.ucn_march_scale_features(ctypes.byref(desc), *[t.data_ptr() for t in geom], None, None, 0.5, N, S,
                                                    k_dev.data_ptr(), layout, out.data_ptr(), st))
        else:
            _lib.check(lib.ucn_march_scale_features_tdist(ctypes.byref(desc), tdist.data_ptr(), *[t.data_ptr() for t in geom[3:]],
                                                          None, None, 0.5, N, S, k_dev.data_ptr(), layout, out.data_ptr(), st))
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[n_out:]).all())                             # nothing written past the planes
        return out[:n_out].cpu()

    def as_nsl(flat, layout):
        """-> ([N, S, L] values, padding channels)"""
        if layout == 1:
            return flat.reshape(N, S, L), flat.new_zeros(0)
        planes = flat.reshape(P, S, N, C).permute(2, 1, 0, 3) if layout == 2 else flat.reshape(P, N, S, C).permute(1, 2, 0, 3)
        full = planes.reshape(N, S, P * C)
        return full[..., :L], full[..., L:]

    got = {}
    for layout in (0, 1, 2):
        flat = run(layout)
        got[layout], pad = as_nsl(flat, layout)
        assert bool(torch.isfinite(got[layout]).all())
        err = (got[layout].double() - want).abs()
        print(f"SCALE_PLANES {kind}/{which} layout {layout}: max err / k = {float((err / k.double()).max()):.3e}")
        assert bool((err <= bar).all()), (layout, float((err / k.double()).max()))
        if layout != 1:
            assert pad.numel() == N * S * (P * C - L) and bool((pad == 0).all())          # padding channels: exactly 0
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])           # the same numbers in every layout
    tdist = torch.empty(N, S + 1, device="cuda")
    _lib.check(lib.ucn_s_to_t(sdist.data_ptr(), near.data_ptr(), far.data_ptr(), N, S + 1, 0, -1.5, tdist.data_ptr(), st))
    for layout in (0, 1, 2):
        assert torch.equal(as_nsl(run(layout, tdist), layout)[0], got[layout])   # identity-curve tdist: bit-identical
    del keep


# ---------------------------------------------------------------------------------------------------- 3. Model.forward, eval
def eval_batch(fx, n):
    batch = H.to_dev(H.batch_of(fx))
    batch["rand_vec"] = torch.cat([fx[f"noise{l}_rand_vec"].reshape(n, -1) for l in range(2)], -1).cuda()
    return batch


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,kind", [("model_scalefeat.npz", "tiny"), ("model_scalefeat_R.npz", "tinyR")])
def test_forward_vs_golden(name, kind, mode):
    """Model.forward in eval mode against the reference, with the bars of test_glo_forward_vs_golden / test_model_forward_vs_golden
    for the same keys and spec, in both arithmetic modes of the NeRF field's dense layers."""
    fx = fixture(name)
    spec = rm.make_spec(kind)
    model, _ = sf.hip_model(spec, sf.state_for(fx, spec))
    model.nerf_mlp.mlp_mode = mode
    n = fx["ray_origins"].shape[0]
    with torch.no_grad():
        rend, hist = model(False, eval_batch(fx, n), 1.0, True)
    torch.cuda.synchronize()
    assert model.last_march_route == "fused"
    fine = kind == "tiny"
    for lvl in range(2):
        g = lambda k: fx[f"L{lvl}_{k}"]
        last = lvl == 1
        samp = (1e-2 if fine else 2e-4) if last else 2e-6
        assert H.maxdiff(hist[lvl]["sdist"].cpu(), g("hist_sdist")) <= (5e-5 if last else 0.0), lvl
        assert H.maxdiff(hist[lvl]["density"].cpu().reshape(-1), g("hist_density").reshape(-1)) <= samp, lvl
        assert H.maxdiff(hist[lvl]["weights"].cpu().reshape(-1), g("hist_weights").reshape(-1)) <= (2e-4 if last else 5e-7), lvl
        assert H.maxdiff(rend[lvl]["weights"].cpu().reshape(-1), g("weights").reshape(-1)) <= (2e-4 if last else 5e-7), lvl
        assert H.maxdiff(rend[lvl]["rgb"].cpu().reshape(-1), g("rgb").reshape(-1)) <= H.RGB_TOL, lvl
        assert float((rend[lvl]["rgb"].cpu().reshape(-1) - g("rgb").reshape(-1)).abs().mean()) <= 2e-5, lvl
        assert H.maxdiff(rend[lvl]["acc"].cpu().reshape(-1), g("acc").reshape(-1)) <= 1e-4, lvl
        stable = (g("acc").reshape(-1) - 0.6).abs() > 1e-3                 # away from the 0.6 sentinel switch
        assert H.maxdiff(rend[lvl]["depth"].cpu().reshape(-1)[stable], g("depth").reshape(-1)[stable]) <= 1e-3, lvl
        if last:
            assert H.maxdiff(hist[lvl]["rgb"].cpu().reshape(-1), g("hist_rgb").reshape(-1)) <= samp
            assert H.maxdiff(hist[lvl]["coord"].cpu().reshape(-1), g("hist_coord").reshape(-1)) <= 5e-6


@pytest.mark.parametrize("name,kind", [("model_scalefeat.npz", "tiny"), ("model_scalefeat_R.npz", "tinyR")])
def test_forward_under_autocast_takes_the_fp32_class_path(name, kind):
    """Under bf16 autocast (render_image's context) a flag-on field does not take the mixed-precision kernels (march_infer.mixed_level
    returns None): the fused march on the fp32-class path, pixels within the fp32 bars of test_forward_vs_golden."""
    fx = fixture(name)
    spec = rm.make_spec(kind)
    model, _ = sf.hip_model(spec, sf.state_for(fx, spec))
    n = fx["ray_origins"].shape[0]
    model._mixed_levels = 0
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        rend, _ = model(False, eval_batch(fx, n), 1.0, True)
    torch.cuda.synchronize()
    assert model.last_march_route == "fused" and model._mixed_levels == 0
    for lvl in range(2):
        got, want = rend[lvl]["rgb"].float().cpu().reshape(-1), fx[f"L{lvl}_rgb"].reshape(-1)
        assert H.maxdiff(got, want) <= H.RGB_TOL, lvl
        assert float((got - want).abs().mean()) <= 2e-5, lvl
        assert H.maxdiff(rend[lvl]["acc"].float().cpu().reshape(-1), fx[f"L{lvl}_acc"].reshape(-1)) <= 1e-4, lvl


def test_mode_1_refuses_a_field_wider_than_64_inputs():
    """L = 16, C = 4 with scale features: (16 + 4) * 4 = 80 inputs > 64: the split-f16 kernels refuse with a message."""
    from ucnerf_amd.internal import models
    mlp = models.NerfMLP(scale_featurization=True, grid_level_dim=4, grid_disired_resolution=524288, grid_log2_hashmap_size=12).cuda()
    with pytest.raises(RuntimeError, match="mlp_mode 1 supports"):
        mlp.field(1)
    mlp.field(0)


# ---------------------------------------------------------------------------------------------------- 4. zero columns
@pytest.mark.parametrize("mode", [0, 1])
def test_zero_scale_columns_equal_the_flag_off_model(mode):
    """A flag-on model whose L extra columns of density_layer.0 are zero computes what the flag-off model does on the same
    remaining weights, within test_mlp_modes_agree's bars (pixels 2e-6, per-sample densities 2e-5 relative)."""
    fx = fixture("model_scalefeat.npz")
    spec = rm.make_spec("tiny")
    on, _ = sf.hip_model(spec, sf.state_for(fx, spec, extra="zero"))
    off, _ = sf.hip_model(spec, sf.state_for(fx, spec, extra=None), on=False)
    n = fx["ray_origins"].shape[0]
    out = []
    for model in (on, off):
        model.nerf_mlp.mlp_mode = mode
        with torch.no_grad():
            rend, hist = model(False, eval_batch(fx, n), 1.0, True)
        out.append((rend[-1]["rgb"].cpu(), hist[-1]["density"].cpu(), hist[0]["density"].cpu()))
    torch.cuda.synchronize()
    print(f"ZERO_COLUMNS mode {mode}: bit-identical = {all(torch.equal(a, b) for a, b in zip(*out))}, "
          f"pixel diff {H.maxdiff(out[0][0], out[1][0]):.3e}")
    assert H.maxdiff(out[0][0], out[1][0]) <= 2e-6
    for i in (1, 2):
        rel = (out[0][i] - out[1][i]).abs() / (out[1][i].abs() + 1e-3)
        assert float(rel.max()) <= 2e-5


# ---------------------------------------------------------------------------------------------------- 5. training step
def run_step(model, fx, spec, mode="split"):
    from ucnerf_amd.internal import train_utils as tu
    model.train()
    model.zero_grad(set_to_none=True)
    batch = H.pin_noise(train_batch(fx, "cuda"), H.noise_of(fx, 2))
    batch["rand_vec"] = batch["rand_vec"][:, None, None, :]
    bf16 = mode == "bf16"
    with f32_engine("split" if bf16 else mode):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            rend, hist = model(True, batch, float(fx["train_frac"]), False, zero_glo=False)
            assert model.last_march_route == "train_graph" and rend[-1]["rgb"].requires_grad
            losses, _ = losses_of(tu, batch, rend, hist, spec)
            total = sum(losses.values())
        total.backward()
    torch.cuda.synchronize()
    return losses


@pytest.mark.parametrize("mode", ["split", "exact", "bf16"])
def test_train_step_matches_reference(mode):
    """One training step against the reference's (train_step_scalefeat.npz): loss terms and every gradient digest at the bars
    test_glo_train_step_matches_reference uses -- fp32 on both GEMM engines, and under bf16 autocast (the production route:
    half tables, _FusedHeads / _PropHeads on cat([features, scale features])) its bf16-vs-fp32 bars; density_layer.0's gradient
    is alive in the scale columns."""
    fx = fixture("train_step_scalefeat.npz")
    spec = rm.make_spec("tiny")
    model, _ = sf.hip_model(spec, sf.state_for(fx, spec))
    losses = run_step(model, fx, spec, mode)
    bf16 = mode == "bf16"
    lrel = 3e-2 if bf16 else 2e-4
    for k, v in losses.items():
        assert abs(float(v) - float(fx["loss_" + k])) <= lrel * max(1.0, abs(float(fx["loss_" + k]))), (k, float(v), float(fx["loss_" + k]))
    seen = 0
    for pname, p in model.named_parameters():
        if f"grad_{pname}.abs" not in fx:
            continue
        seen += 1
        assert p.grad is not None and torch.isfinite(p.grad).all(), pname
        if bf16:
            want = float(fx[f"grad_{pname}.abs"])
            assert abs(float(p.grad.double().abs().sum()) - want) <= 0.1 * want, pname
        elif pname == "nerf_mlp.encoder.embeddings":
            assert abs(float(p.grad.double().abs().sum()) - float(fx[f"grad_{pname}.abs"])) <= 2e-2 * float(fx[f"grad_{pname}.abs"])
        else:
            check_grad(fx, pname, p.grad, 2e-2)
    assert seen >= 10
    for fs in sf.fields_of(spec):
        g = model.get_submodule(fs.prefix).density_layer[0].weight.grad
        assert g.shape[1] == fs.num_grid_levels * (fs.grid_level_dim + 1)
        assert float(g[:, fs.num_grid_levels * fs.grid_level_dim:].abs().sum()) > 0


def test_scale_features_add_no_gradient_path(monkeypatch):
    """The table gradient equals the one of the same step with the scale features' forward values kept but supplied as a
    constant input: nothing reaches the table (or anything else) through them."""
    from ucnerf_amd.internal import train_graph as tg
    fx = fixture("train_step_scalefeat.npz")
    spec = rm.make_spec("tiny")
    model, _ = sf.hip_model(spec, sf.state_for(fx, spec))
    real, seen = tg.scale_features, []

    def record(*a, **k):
        seen.append(real(*a, **k))
        assert not seen[-1].requires_grad
        return seen[-1]
    monkeypatch.setattr(tg, "scale_features", record)
    run_step(model, fx, spec)
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert len(seen) == 2
    consts = [t.clone() for t in seen]
    monkeypatch.setattr(tg, "scale_features", lambda *a, **k: consts.pop(0))
    run_step(model, fx, spec)
    for n, p in model.named_parameters():
        if n.endswith("encoder.embeddings"):
            # rows summed through LDS float adds whose order varies from run to run: equal to fp32 summation noise
            # (the bar of test_neutral_glo_equals_the_non_glo_route)
            assert float((p.grad - grads[n]).abs().max()) <= 1e-5 * float(grads[n].abs().max()), n
        elif p.grad is not None:
            assert torch.equal(p.grad, grads[n]), n


# ---------------------------------------------------------------------------------------------------- 6. predict_density
def test_predict_density_against_the_restatement():
    """MLP.predict_density (extract.py, the density lattice) with the flag on, 64 points x 6 Gaussians, against the restatement;
    bar: 2e-4, the per-sample bar test_model_forward_vs_golden holds this spec's NeRF field to."""
    fx = fixture("model_scalefeat_R.npz")
    spec = rm.make_spec("tinyR")
    sd = sf.state_for(fx, spec)
    model, _ = sf.hip_model(spec, sd)
    g = torch.Generator().manual_seed(29)
    means = torch.randn(64, 6, 3, generator=g) * torch.logspace(-1, 0.7, 64)[:, None, None]
    stds = torch.rand(64, 6, generator=g) * 0.02 + 1e-3
    with torch.no_grad():
        raw_w, x_w, coord_w, _ = sf.field_density_features(spec.nerf, sd, means, stds)
        raw_p, x_p, _, _ = rm.field_density_features(spec.nerf, sf.state_for(fx, spec, extra=None), means, stds)
    raw, x, coord = model.nerf_mlp.predict_density(means.cuda(), stds.cuda())
    torch.cuda.synchronize()
    assert H.maxdiff(coord.cpu(), coord_w) <= 5e-6
    assert H.maxdiff(raw.cpu(), raw_w) <= 2e-4 and H.maxdiff(x.cpu(), x_w) <= 2e-4
    assert H.maxdiff(raw_w, raw_p) > 1e-2                                       # the scale features do act on these points
    # no_warp (extract.py:56-57): one Gaussian per point, inside the unit cube
    pm, ps = torch.rand(64, 1, 3, generator=g) * 2 - 1, torch.full((64, 1), 1e-3)
    with torch.no_grad():
        raw_w, _, _, _ = sf.field_density_features(spec.nerf, sd, pm, ps, no_warp=True)
    raw, _, _ = model.nerf_mlp.predict_density(pm.cuda(), ps.cuda(), no_warp=True)
    assert H.maxdiff(raw.cpu(), raw_w) <= 2e-4
