"""On-GPU ray generation for the panorama ('panoroma') and spherical camera models against the reference's golden vectors
(tests/golden/rays_pano.npz; tests/test_rays_pano_cpu.py holds the numpy restatement to them bit for bit) (-m gpu).

The bar (rays_pano_ref.within_bar) is derived, not measured: both sides compute in float64 and round once to float32; the device's
double sin / cos need not be libm's in the last bits, so a result may land on the neighbouring float32.  Vector outputs:
|got - want| <= 2^-23 ||want|| per component (the ray's vector norm); radii: |got - want| <= 2^-23 want.  No element is excluded.
Each test prints how many elements differ from the golden file at all (an observation, DESIGN.md records it)."""
import os

import numpy as np
import pytest
import torch

import rays_pano_ref as R

pytestmark = pytest.mark.gpu
KEYS = ("origins", "directions", "viewdirs", "radii", "imageplane", "cam_dirs")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "rays_pano.npz"))


def _cameras(fx, tag):
    return (torch.from_numpy(fx[f"{tag}.pixtocams"]), torch.from_numpy(fx[f"{tag}.camtoworlds"]), None, None)


def _hold(what, got, want_of, keys=KEYS):
    differ = total = 0
    for k in keys:
        g, w = got[k].cpu().numpy(), want_of(k)
        ok, n, ratio = R.within_bar(k, g, w)
        differ, total = differ + n, total + g.size
        assert ok, (what, k, n, ratio)
    print(f"{what}: {differ} of {total} float32 elements differ from the golden file")


def _same(what, a, b, keys=KEYS[:5]):
    for k in keys:
        assert torch.equal(a[k], b[k]), (what, k)


def test_panorama_frame_and_batch_vs_reference(fx):
    from ucnerf_amd.internal import camera_utils as cu
    cams = _cameras(fx, "pano_frame")
    W, H = int(fx["pano_frame.width"]), int(fx["pano_frame.height"])
    px, py = cu.pixel_coordinates(W, H)
    for cam in range(2):
        want = lambda k: fx[f"pano_frame.{k}"][cam]
        pixels = dict(pix_x_int=px, pix_y_int=py, cam_idx=torch.full((H, W, 1), cam, device="cuda"))
        a = cu.cast_ray_batch(cams, pixels, cu.PANORAMA)
        _hold(f"pano_frame[{cam}] cast_ray_batch", a, want)
        one = dict(zip(KEYS[:5], cu.pixels_to_rays(px, py, cams[0][cam], cams[1][cam], camtype="panoroma")))
        idx = torch.full((H, W), cam, dtype=torch.long)
        per = dict(zip(KEYS[:5], cu.pixels_to_rays(px, py, cams[0][idx], cams[1][idx], camtype=cu.PANORAMA)))
        full = cu.generate_ray_batch(cams, cam, W, H, 0.25, 8.0, camtype=cu.PANORAMA)
        # the four forms run the same kernel on the same pixels: bit for bit
        _same("one camera", one, a)
        _same("per-pixel matrices", per, a)
        _same("generate_ray_batch", full, a, KEYS)
        for k in KEYS:
            assert tuple(full[k].shape) == want(k).shape, k
        for k, v in (("near", 0.25), ("far", 8.0), ("lossmult", 1.0), ("cam_idx", float(cam))):
            assert tuple(full[k].shape) == (H, W, 1) and bool((full[k] == v).all()), k
        assert torch.equal(full["camera_id"], full["cam_idx"][..., 0])
    # a [B, 1] pixel batch of the 8000 x 900 frame with per-ray cameras
    cams = _cameras(fx, "pano_batch")
    px, py = torch.from_numpy(fx["pano_batch.pix_x"]).cuda(), torch.from_numpy(fx["pano_batch.pix_y"]).cuda()
    ci = torch.from_numpy(fx["pano_batch.cam_idx"]).cuda()[..., None]
    a = cu.cast_ray_batch(cams, dict(pix_x_int=px, pix_y_int=py, cam_idx=ci, near=None, far=None, lossmult=None), "panoroma")
    _hold("pano_batch cast_ray_batch", a, lambda k: fx[f"pano_batch.{k}"])
    assert a["near"] is None and a["cam_idx"] is ci
    idx = torch.from_numpy(fx["pano_batch.cam_idx"]).long()
    per = dict(zip(KEYS[:5], cu.pixels_to_rays(px, py, cams[0][idx], cams[1][idx], camtype="panoroma")))
    _same("pano_batch per-pixel matrices", per, a)
    # a pixel batch drawn from a full frame equals the same pixels of the frame
    full = cu.generate_ray_batch(cams, 1, 8000, 900, 0.1, 100.0, camtype="panoroma")
    sub = cu.cast_ray_batch(cams, dict(pix_x_int=px, pix_y_int=py, cam_idx=torch.ones_like(ci)), "panoroma")
    for k in KEYS:
        assert torch.equal(sub[k], full[k][py.long(), px.long()]), k


@pytest.mark.parametrize("tag", ["sph_6x16", "sph_5x7", "sph_big"])
def test_spherical_vs_reference(fx, tag):
    from ucnerf_amd.internal import camera_utils as cu
    H, W = int(fx[f"{tag}.height"]), int(fx[f"{tag}.width"])
    near, far = float(fx[f"{tag}.near"]), float(fx[f"{tag}.far"])
    b = cu.cast_spherical_rays(torch.from_numpy(fx[f"{tag}.camtoworld"]), H, W, near, far)
    assert set(b) == {"origins", "directions", "viewdirs", "radii", "imageplane", "lossmult", "near", "far", "cam_idx", "cam_dirs"}
    for k, v in b.items():
        assert v.is_cuda and v.dtype == torch.float32 and tuple(v.shape[:2]) == (H, W), k
    assert torch.equal(b["viewdirs"], b["directions"])                       # not renormalised
    assert not bool(b["imageplane"].any()) and tuple(b["imageplane"].shape) == (H, W, 2)
    assert bool((b["cam_dirs"] == torch.from_numpy(fx[f"{tag}.cam_dirs"]).cuda()).all())     # a copy of a pose column: exact
    if tag == "sph_big":
        rows, cols = torch.from_numpy(fx["sph_big.rows"]).long().cuda(), torch.from_numpy(fx["sph_big.cols"]).long().cuda()
        sel = {k: v[rows[:, None], cols[None, :]] for k, v in b.items()}
    else:
        sel = b
    _hold(tag, sel, lambda k: fx[f"{tag}.{k}"], KEYS[:5])
    for k, g in (("lossmult", "lossmult"), ("cam_idx", "cam_idx"), ("near", "near_col"), ("far", "far_col")):
        assert np.array_equal(sel[k].cpu().numpy(), fx[f"{tag}.{g}"]), k
    # row 0: sin(phi) = 0, dx vanishes exactly and the radius is |dy| / sqrt(12) alone.  That dx is exactly zero shows as the whole
    # row holding one radius and one direction (asserted bit for bit below); dy still goes through the device's sin / cos of
    # phi_1, so against the golden row the radii get the radii bar, not bit-identity (no sin / cos bound gives that)
    want0 = fx[f"{tag}.radii"][0]
    ok, n, ratio = R.within_bar("radii", sel["radii"][0].cpu().numpy(), want0)
    assert ok, (tag, "row 0 radii", n, ratio)
    assert bool((b["radii"][0] == b["radii"][0, 0]).all()) and bool((b["directions"][0] == b["directions"][0, 0]).all())


def test_refusals_and_empty_batches(fx):
    from ucnerf_amd.internal import camera_utils as cu
    px = torch.zeros(4, dtype=torch.int32, device="cuda")
    cams = _cameras(fx, "pano_frame")
    with pytest.raises(NotImplementedError, match="distortion"):
        cu.pixels_to_rays(px, px, cams[0][0], cams[1][0], distortion_params=dict(k1=0.1), camtype="panoroma")
    with pytest.raises(NotImplementedError, match="NDC"):
        cu.pixels_to_rays(px, px, cams[0][0], cams[1][0], pixtocam_ndc=np.eye(3), camtype="panoroma")
    with pytest.raises(NotImplementedError, match="NDC"):
        cu.generate_ray_batch((cams[0], cams[1], None, np.eye(3)), 0, 4, 4, 0.1, 1.0, camtype="panoroma")
    with pytest.raises(NotImplementedError, match="perspective"):
        cu.pixels_to_rays(px, px, cams[0][0], cams[1][0], camtype=cu.ProjectionType.FISHEYE)
    for bad in ("pano", "fisheye", "Panoroma"):
        with pytest.raises(NotImplementedError, match=repr(bad)):
            cu.pixels_to_rays(px, px, cams[0][0], cams[1][0], camtype=bad)
        with pytest.raises(NotImplementedError, match=repr(bad)):
            cu.cast_ray_batch(cams, dict(pix_x_int=px, pix_y_int=px, cam_idx=torch.zeros(4, 1, device="cuda")), bad)
        with pytest.raises(NotImplementedError, match=repr(bad)):
            cu.generate_ray_batch(cams, 0, 4, 4, 0.1, 1.0, camtype=bad)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        cu.pixels_to_rays(px.cpu(), px.cpu(), cams[0][0], cams[1][0], camtype="panoroma")
    with pytest.raises(RuntimeError, match="CUDA device"):
        cu.cast_spherical_rays(cams[1][0], 4, 4, 0.1, 1.0, device="cpu")
    for H, W in ((1 << 32, 1), (1, 1 << 32), (1 << 16, 1 << 16), (-1, 4)):          # would wrap in the 32-bit C arguments
        with pytest.raises(RuntimeError, match="outside"):
            cu.cast_spherical_rays(cams[1][0], H, W, 0.1, 1.0)
    with pytest.raises(RuntimeError, match="out of range"):
        cu.cast_ray_batch(cams, dict(pix_x_int=px, pix_y_int=px, cam_idx=torch.full((4, 1), 99, device="cuda")), "panoroma")
    from ucnerf_amd import _lib
    lib = _lib.load()
    z = torch.zeros(16, device="cuda")
    p2c, c2w = cams[0].cuda(), cams[1].cuda()
    rc = lib.ucn_generate_rays_model(px.data_ptr(), px.data_ptr(), None, 0, p2c.data_ptr(), c2w.data_ptr(), 2, 0, 0, 4, 0.0, 0.0,
                                     z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, z.data_ptr(), None, None, None,
                                     None, 2, _lib.stream())
    assert rc != 0 and b"camera model 2" in lib.ucn_last_error()
    empty = torch.zeros(0, 5, dtype=torch.int32, device="cuda")
    o, d, v, r, ip = cu.pixels_to_rays(empty, empty, cams[0][0], cams[1][0], camtype="panoroma")
    assert o.shape == (0, 5, 3) and d.shape == (0, 5, 3) and v.shape == (0, 5, 3) and r.shape == (0, 5, 1) and ip.shape == (0, 5, 2)
    for H, W in ((0, 8), (8, 0)):
        b = cu.cast_spherical_rays(cams[1][0], H, W, 0.1, 1.0)
        assert b["origins"].shape == (H, W, 3) and b["radii"].shape == (H, W, 1) and b["imageplane"].shape == (H, W, 2)
        assert b["cam_dirs"].shape == (H, W, 3) and b["near"].shape == (H, W, 1)


def test_one_march_on_each_new_batch(fx):
    """The only check that the new batches carry every key the march reads: the smallest model of the GPU tests, eval mode, no_grad."""
    from oracle import raymarch as rm
    from ucnerf_amd.internal import camera_utils as cu, configs, models
    spec = rm.make_spec("tiny")
    kw = dict(grid_level_dim=2, grid_log2_hashmap_size=12)
    with models.bindings(NerfMLP=dict(grid_disired_resolution=524288, **kw), PropMLP=dict(**kw)):
        model = models.Model(config=configs.Config(), num_levels=2, num_prop_samples=64, num_nerf_samples=128)
    missing, unexpected = model.load_state_dict(rm.init_state(spec, seed=3), strict=False)
    assert not unexpected and all(k.endswith(".idx") for k in missing), (missing, unexpected)
    model = model.cuda().eval()
    K = np.array([[10.0, 0.0, 15.7], [0.0, 10.0, 2.2], [0.0, 0.0, 1.0]])
    pose = torch.from_numpy(fx["sph_6x16.camtoworld"])
    cams = (torch.from_numpy(np.linalg.inv(K)), pose, None, None)
    pano = cu.generate_ray_batch(cams, 0, 32, 4, 0.2, 6.0, camtype=cu.PANORAMA)
    # panorama directions are not the perspective ones: |d| = sqrt(1 + y^2)
    assert torch.allclose(pano["directions"].norm(dim=-1), (1 + pano["imageplane"][..., 1] ** 2).sqrt(), rtol=1e-6, atol=0)
    sph = cu.cast_spherical_rays(pose, 4, 8, 0.2, 6.0)
    for name, batch, shape in (("panorama", pano, (4, 32)), ("spherical", sph, (4, 8))):
        with torch.no_grad():
            renderings, _ = model(False, batch, 1.0, True)
        torch.cuda.synchronize()
        rgb = renderings[-1]["rgb"]
        assert tuple(rgb.shape) == shape + (3,), (name, rgb.shape)
        for r in renderings:
            assert tuple(r["rgb"].shape) == shape + (3,) and bool(torch.isfinite(r["rgb"]).all()), name
            assert tuple(r["acc"].shape) == shape and bool(torch.isfinite(r["acc"]).all()), name
