"""The ray-tile variant of the NeRF-level split-f16 MLP (csrc/field_mlp_h.hip comment 6): k_field_mlp_h8<..., MODE = 1>.

CPU part: the ISA of the two 4-wave instantiations (hipcc cross-compiles to text, as tests/test_isa_invariants.py does).
GPU part: the per-ray direction terms against a float64 evaluation, and both kernels against oracle/truth64.py on rays of bench.py's
frame.  `UCN_MLP_RAY_TILE=0` (read per launch) keeps a launch on the [any rays][32] tile: one process holds the two to each other."""
import contextlib
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ucnerf_amd", "csrc")


# ------------------------------------------------------------------------------------------------------------------ ISA (no GPU)
def _mlp_kernels():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "field_mlp_h.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                               "-S", "--cuda-device-only", "-w", "field_mlp_h.hip", "-o", out], cwd=CSRC)
        text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_Z\w*k_field_mlp_h8ILi8ELi4ELi16ELi4ELi2ELi2ELi([012])E\w*):", text, re.M):
        body = [ln.split(";")[0].strip() for ln in text[m.end():text.index(".Lfunc_end", m.end())].split("\n")]
        meta = text[text.index(".amdhsa_kernel " + m.group(1)):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        val = lambda key: int(re.search(key + r"\s+(\d+)", meta).group(1))
        found[int(m.group(2))] = dict(mfma=sum(ln.startswith("v_mfma_f32_32x32x16") for ln in body),
                                      other_mfma=sum(ln.startswith("v_mfma") and not ln.startswith("v_mfma_f32_32x32x16") for ln in body),
                                      branches=sum(ln.startswith("s_cbranch") for ln in body),
                                      vgpr=val(r"\.amdhsa_next_free_vgpr"), scratch=val(r"\.amdhsa_private_segment_fixed_size"))
    return found


def test_ray_tile_kernel_issues_96_fewer_mfmas_without_scratch_at_two_workgroups_per_cu():
    """The stages are fully unrolled (rstatic_for), so the static count of v_mfma_f32_32x32x16 IS the count per wave and tile:
    24 (first layer) + 4 pairs x 6 double steps x 6 (A) + 4 x (6 + 16) x 6 (B) = 696 on the [any rays][32] tile; the ray tile drops
    the direction tile's 2 double steps per pair in A and in B's skip part: 2 x 4 x 2 x 6 = 96 -> 600.  <= 256 registers and no
    scratch: two workgroups per CU as before."""
    k = _mlp_kernels()
    assert set(k) == {0, 1, 2}, k                   # MODE 0: direction tile in the stream; 1: ray tiles; 2: per-lane seeds (same arithmetic as 1)
    print("k_field_mlp_h8<8,4,16,4,2,2,MODE>:", k)
    assert k[0]["mfma"] == 696 and k[1]["mfma"] == 600 and k[2]["mfma"] == 600, k
    assert all(v["other_mfma"] == 0 for v in k.values()), k
    for rt in (0, 1, 2):
        assert k[rt]["scratch"] == 0 and k[rt]["vgpr"] <= 256, (rt, k[rt])


# ------------------------------------------------------------------------------------------------------------------------ GPU
@contextlib.contextmanager
def _old_kernel(force):
    prev = os.environ.get("UCN_MLP_RAY_TILE")
    if force:
        os.environ["UCN_MLP_RAY_TILE"] = "0"
    else:
        os.environ.pop("UCN_MLP_RAY_TILE", None)
    try:
        yield
    finally:
        if prev is None:
            os.environ.pop("UCN_MLP_RAY_TILE", None)
        else:
            os.environ["UCN_MLP_RAY_TILE"] = prev


def _frame_rays(n):
    import bench
    dev = torch.device("cuda", 0)
    rays = bench.frame_rays(dev)
    n_total = bench.H_IMG * bench.W_IMG
    idx = torch.linspace(0, n_total - 1, n).long().to(dev)
    return {k: v.reshape(n_total, -1)[idx].contiguous() for k, v in rays.items()}


@pytest.mark.gpu
def test_direction_terms_against_float64():
    """ucn_field_dir_bias of the 256-wide mode-1 field: floats [32, 32 + 512) of a ray's row are 2^e (W[:, dir] enc(d) + bias) of the two
    composed layers in accumulator-slot order, bias = b_c + W_c[:, x] b_d1.  Truth: numpy float64 from the same weights.  2^e (the layer's
    scale, chosen at pack time) is read off as the power of two nearest the median ratio and must then fit EVERY entry.
    Bound per entry, from the arithmetic: the kernel chains ND + 1 fp32 FMAs (each rounds a partial sum of magnitude <= mag =
    sum |w_k enc_k| + |bias|: (ND + 1) 2^-24 mag), the composed bias was rounded to fp32 once (2^-24 |bias|): together <= (ND + 2) 2^-24
    mag, doubled for the fp32 rounding of the weights' products' order = 2^-23 (ND + 2) mag; and enc itself is fp32: sinf's argument
    sc + pi/2 <= 9.6 rounds by <= 2^-21, sinf adds ~2 ulp, the fp32 pi/2 is 4.4e-8 off: <= 1e-6 per entry of enc, times sum |w_k|."""
    import bench
    from ucnerf_amd import _lib
    from oracle import truth64 as t64
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    model, _, _ = bench.build_model(dev)
    mlp = model.nerf_mlp
    assert mlp.mlp_mode == 1 and mlp.net_width_viewdirs == 256
    n = 1003
    g = torch.Generator().manual_seed(5)
    vd = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    desc = mlp.field()
    stride = int(lib.ucn_field_dir_floats(ctypes.byref(desc), 1))
    assert stride == 32 + 512 and int(lib.ucn_field_dir_floats(ctypes.byref(desc), n)) == n * stride
    buf = torch.full((n * stride + 64,), float("nan"), device=dev)                    # + guard: nothing is written past the rows
    vdd = vd.to(dev).contiguous()
    _lib.check(lib.ucn_field_dir_bias(ctypes.byref(desc), vdd.data_ptr(), n, buf.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[n * stride:]).all())
    rows = buf[:n * stride].reshape(n, stride).double().cpu().numpy()
    NB, NW, ND = mlp.bottleneck_width, 256, mlp.dim_dir_enc
    enc = t64.view_encoding(vd, mlp.deg_view).numpy()                                # [n, ND] float64
    # the direction tile in front: 2^10 [enc, 1, 0...]
    tile = np.concatenate([enc, np.ones((n, 1)), np.zeros((n, 31 - ND))], axis=1) * 1024.0
    assert np.abs(rows[:, :32] - tile).max() <= 1024.0 * 1e-6
    f = lambda t: t.detach().double().cpu().numpy()
    bd1 = f(mlp.density_layer[2].bias)
    slot = np.array([32 * t + (r & 3) + 8 * (r >> 2) + 4 * h for t in range(8) for h in range(2) for r in range(16)])
    report = []
    for layer, (lin, x0) in enumerate(((mlp.lin_second_stage_0, 0), (mlp.lin_second_stage_1, NW))):
        W, b = f(lin.weight), f(lin.bias)
        Wdir, bias = W[:, x0 + NB:x0 + NB + ND], b + W[:, x0:x0 + NB] @ bd1
        want = enc @ Wdir.T + bias                                                   # [n, NW]
        mag = np.abs(enc) @ np.abs(Wdir).T + np.abs(bias)
        tol = 2.0 ** -23 * (ND + 2) * mag + 1e-6 * np.abs(Wdir).sum(axis=1)
        got = rows[:, 32 + layer * NW:32 + (layer + 1) * NW][:, np.argsort(slot)]     # accumulator slot -> neuron
        big = np.abs(want) > 0.1 * np.abs(want).max()
        e = int(round(float(np.median(np.log2(np.abs(got[big]) / np.abs(want[big]))))))
        err = np.abs(got * 2.0 ** -e - want)
        report.append((layer, e, float(err.max()), float((err / tol).max())))
        print(f"direction terms layer {layer}: scale 2^{e}, max |err| {err.max():.3e}, max err / bound {(err / tol).max():.3f}")
        assert (err <= tol).all(), report
    assert len(report) == 2


def _history(model, rays, rand_vec, old):
    batch = dict(rays, rand_vec=rand_vec.cuda())
    with _old_kernel(old), torch.no_grad():
        _, hist = model(False, batch, 1.0, False)
    torch.cuda.synchronize()
    n = rand_vec.shape[0]
    h = hist[-1]
    return h["sdist"].reshape(n, -1).cpu(), h["density"].reshape(n, -1).double().cpu(), h["rgb"].reshape(n, -1, 3).double().cpu()


# margin of "no larger than the old kernel's own error": both kernels read the SAME features (one gather), so their errors against
# the truth share the geometry / table part and differ in the roundings of the colour layers only.  The mean over >= 8 192 samples is a
# stable statistic (5 %); the maximum is an extreme value of two different rounding patterns (25 %).  Floors: one fp32 ulp of an O(1)
# colour / 1e-3 of one for the mean.
MARGIN_MAX, MARGIN_MEAN = 1.25, 1.05


@pytest.mark.gpu
@pytest.mark.parametrize("n,rays_fastest", [(10240, True), (1021, True), (1022, False)])
def test_ray_tile_kernel_is_no_further_from_the_float64_truth_than_the_old_kernel(n, rays_fastest):
    """`n` strided rays of bench.py's frame through Model.forward's inference march twice: ray-tile kernel, and UCN_MLP_RAY_TILE=0.
    n = 10 240 is one whole pass of the headline frame; n = 1021 (rays-fastest: 256 ray groups, the last with ONE live wave) and
    n = 1022 in the [ray][sample] feature layout (plain tile order) cover N % 4 != 0 and a partial last workgroup.  Truth: oracle/truth64.py's float64
    level at the HIP march's own fenceposts, on 64 strided rays plus the LAST 8 rays (where the tail handling acts).  Required: the
    new kernel's error (density relative to max(1, density); rgb absolute) <= MARGIN x the old kernel's own error + floor, maximum
    and mean.  Measured on MI355X (profiles/ray_tile/parity.txt): ratio new / old of the maximum and of the mean error 1.000 in all three
    cases, density and rgb (e.g. n = 10 240 rgb: 3.885e-04 / 3.887e-04 max, 2.459e-05 both means); new vs old density identical, rgb
    within 5.1e-07.  New-vs-old differences are printed, not asserted."""
    import bench
    from oracle import raymarch as rm
    from oracle import truth64 as t64
    dev = torch.device("cuda", 0)
    model, _, sd = bench.build_model(dev)
    model.rays_fastest = rays_fastest
    assert model.max_chunk_rays >= n and model.num_nerf_samples % 32 == 0 and model.compact_min_weight == 0
    rays = _frame_rays(n)
    rand_vec = torch.randn(n, 6, generator=torch.Generator().manual_seed(1))
    sd_new, den_new, rgb_new = _history(model, rays, rand_vec, old=False)
    sd_old, den_old, rgb_old = _history(model, rays, rand_vec, old=True)
    assert torch.equal(sd_new, sd_old)                                               # the proposal level is untouched
    assert bool(torch.isfinite(den_new).all()) and bool(torch.isfinite(rgb_new).all())
    print(f"ray tile n={n} rays_fastest={rays_fastest}: new vs old max |d density| / max(1, density) "
          f"{float(((den_new - den_old).abs() / den_old.clamp_min(1)).max()):.3e}, max |d rgb| {float((rgb_new - rgb_old).abs().max()):.3e}")
    pick = torch.unique(torch.cat([torch.linspace(0, n - 1, 64).long(), torch.arange(n - 8, n)]))
    spec = rm.make_spec("B")
    sub = {k: v[pick.to(dev)].cpu() for k, v in rays.items()}
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        _, res = t64.level_forward(spec, spec.nerf, t64.state64(sd), sub, sd_new[pick], rm.LevelNoise(rand_vec=rand_vec[pick, 3:6]))
    t_den, t_rgb = res["density"].reshape(len(pick), -1), res["rgb"].reshape(len(pick), -1, 3)
    lines = []
    for name, new, old, truth, floor in (("density", den_new[pick], den_old[pick], t_den, (1.2e-7, 1e-10)),
                                         ("rgb", rgb_new[pick], rgb_old[pick], t_rgb, (1.2e-7, 1e-10))):
        den = truth.abs().clamp_min(1) if name == "density" else torch.ones_like(truth)
        e_new, e_old = ((new - truth).abs() / den).reshape(-1), ((old - truth).abs() / den).reshape(-1)
        line = (f"RAYTILE n={n} rays_fastest={int(rays_fastest)} {name}: e_old max {float(e_old.max()):.3e} mean {float(e_old.mean()):.3e} | "
                f"e_new max {float(e_new.max()):.3e} mean {float(e_new.mean()):.3e} | ratio max {float(e_new.max() / e_old.max()):.3f} "
                f"mean {float(e_new.mean() / e_old.mean()):.3f}")
        print(line)
        lines.append((line, e_new, e_old, floor))
    for line, e_new, e_old, floor in lines:
        assert float(e_new.max()) <= MARGIN_MAX * float(e_old.max()) + floor[0], line
        assert float(e_new.mean()) <= MARGIN_MEAN * float(e_old.mean()) + floor[1], line


@pytest.mark.gpu
def test_field_call_tiles_partial_workgroup_and_other_sample_counts():
    """The [ray][sample] entry (MLP.forward on explicit Gaussians).  5 rays x 32 samples: five ray tiles, the second workgroup has
    three dead waves -- held to the old kernel's error against truth64 as above.  5 rays x 48 samples (48 % 32 != 0): the launch
    stays on the old kernel, so the output is bit-identical with and without the switch."""
    import bench
    from oracle import raymarch as rm
    from oracle import truth64 as t64
    dev = torch.device("cuda", 0)
    model, _, sd = bench.build_model(dev)
    spec = rm.make_spec("B")
    g = torch.Generator().manual_seed(11)
    for S in (32, 48):
        means = (torch.rand(5, S, 6, 3, generator=g) * 2 - 1) * 1.5
        stds = torch.rand(5, S, 6, generator=g) * 0.02 + 1e-3
        vd = torch.nn.functional.normalize(torch.randn(5, 3, generator=g), dim=-1)
        out = []
        for old in (False, True):
            with _old_kernel(old), torch.no_grad():
                r = model.nerf_mlp(False, means.cuda().contiguous(), stds.cuda().contiguous(), viewdirs=vd.cuda().contiguous())
            torch.cuda.synchronize()
            out.append((r["density"].double().cpu(), r["rgb"].double().cpu()))
        (den_new, rgb_new), (den_old, rgb_old) = out
        if S % 32:
            assert torch.equal(den_new, den_old) and torch.equal(rgb_new, rgb_old)
            continue
        with torch.no_grad():
            t = t64.field_forward(spec.nerf, t64.state64(sd), means, stds, vd)
        for name, new, old, truth in (("density", den_new, den_old, t["density"]), ("rgb", rgb_new, rgb_old, t["rgb"])):
            den = truth.abs().clamp_min(1) if name == "density" else torch.ones_like(truth)
            e_new, e_old = ((new - truth).abs() / den).reshape(-1), ((old - truth).abs() / den).reshape(-1)
            line = (f"RAYTILE field call 5x32 {name}: e_old max {float(e_old.max()):.3e} mean {float(e_old.mean()):.3e} | e_new max "
                    f"{float(e_new.max()):.3e} mean {float(e_new.mean()):.3e}")
            print(line)
            # 160 samples: the mean is no longer a stable statistic, both are held by the maximum's margin
            assert float(e_new.max()) <= MARGIN_MAX * float(e_old.max()) + 1.2e-7, line
            assert float(e_new.mean()) <= MARGIN_MAX * float(e_old.mean()) + 1e-10, line
