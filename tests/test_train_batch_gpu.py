"""The device batch assembler (ucnerf_amd/internal/datasets.py, csrc/batch.hip) on the GPU (-m gpu): parity with the reference's
`_make_ray_batch` on given indices (tests/golden/train_batch.npz), the shared ray body, out-of-range look-ups, the sampler's
constraints, the virtual-pose branch, and the DataLoader surface feeding `Model.forward`."""
import json
import os

import numpy as np
import pytest
import torch

import helpers as H
import rays_pano_ref
import train_batch_ref as R
from oracle import raymarch as rm
from oracle import warp as oracle_warp
from test_train_batch_cpu import CASES, restated

pytestmark = pytest.mark.gpu
PLANES = ("rgb", "disps", "sky_segs")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "train_batch.npz"))


def dataset(fx, virtual=False, all_cameras=False, **kw):
    from ucnerf_amd.internal import datasets as D
    n_real = int(fx["scene.n_real"])
    cams = slice(None) if virtual or all_cameras else slice(0, n_real)
    kw.setdefault("batch_size", 64)
    return D.DeviceDataset(fx["scene.images"], fx["scene.camtoworlds"][cams], fx["scene.pixtocams"][cams], float(fx["scene.near"]),
                           float(fx["scene.far"]), disp_images=fx["scene.disp_images"], sky_segments=fx["scene.sky_segments"],
                           virtual_poses=fx["scene.camtoworlds"][n_real:] if virtual else None, cam_num=1,
                           virtual_poses_enabled=virtual, compute_disp_metrics=True, load_sky_segments=True, **kw)


def inputs(fx, case):
    return {k.split(".in.", 1)[1]: torch.from_numpy(fx[k]).cuda() for k in fx.files if k.startswith(f"{case}.in.")}


def run(fx, case, **kw):
    ds = dataset(fx, virtual=case == "c", **kw)
    if case == "d":
        return ds.generate_ray_batch(int(fx["d.in.cam_idx"]))
    return ds.make_ray_batch(**inputs(fx, case))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_layout(got, want):
    assert list(got) == list(want)
    for k, v in got.items():
        if want[k] is None:
            assert v is None, k
            continue
        assert v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == want[k].shape, (k, tuple(v.shape), want[k].shape)


@pytest.mark.parametrize("case", CASES)
def test_perspective_batch_is_the_references(fx, case):
    """Every key of the reference's batch, no element excluded: ray keys and columns by torch.equal, gathered planes bit for bit."""
    got = run(fx, case)
    none = json.loads(str(fx[f"{case}.none"]))
    want = {k: (None if k in none else fx[f"{case}.out.{k}"]) for k in json.loads(str(fx[f"{case}.keys"]))}
    check_layout(got, want)
    for k, w in want.items():
        if w is None:
            continue
        assert torch.equal(got[k].cpu(), torch.from_numpy(w)), (case, k)
        if k in PLANES:
            assert same_bits(got[k].cpu().numpy(), w), (case, k)


@pytest.mark.parametrize("case", CASES)
def test_panorama_batch_within_the_existing_bar(fx, case):
    """camtype='panoroma' against the float64 restatement under rays_pano_ref.within_bar (one float32 unit of the ray's vector
    norm, derived there; no margin added); the gathered planes and the columns stay bit-identical."""
    got = run(fx, case, camtype=rays_pano_ref.PANORAMA)
    want = restated(fx, case, camtype=rays_pano_ref.PANORAMA)
    check_layout(got, want)
    for k, w in want.items():
        if w is None:
            continue
        g = got[k].cpu().numpy()
        if k in rays_pano_ref.VECTOR_KEYS or k == "radii":
            ok, n_diff, ratio = rays_pano_ref.within_bar(k, g, w)
            print(f"TRAIN_BATCH pano case {case} {k}: {n_diff} of {g.size} elements differ, worst = {ratio:.3f} of the bar")
            assert ok, (case, k, ratio)
        else:
            assert same_bits(g, w), (case, k)


@pytest.mark.parametrize("case", ["c", "e"])
def test_rays_are_cast_ray_batchs_bit_for_bit(fx, case):
    """The two kernels share one per-ray body (csrc/rays_core.h)."""
    from ucnerf_amd.internal import camera_utils as cu
    ins = inputs(fx, case)
    got = run(fx, case)
    x, y, cam = ((ins["pixel_x_int_with_src"], ins["pixel_y_int_with_src"], ins["cam_idx_with_src"]) if case == "c" else
                 (ins["pix_x_int"], ins["pix_y_int"], ins["cam_idx"]))
    n_cams = None if case == "c" else int(fx["scene.n_real"])
    cameras = (torch.from_numpy(fx["scene.pixtocams"][:n_cams]), torch.from_numpy(fx["scene.camtoworlds"][:n_cams]), None, None)
    want = cu.cast_ray_batch(cameras, dict(pix_x_int=x, pix_y_int=y, cam_idx=cam[..., None]))
    for k in R.RAY_KEYS:
        assert same_bits(got[k].cpu().numpy(), want[k].cpu().numpy()), (case, k)


@pytest.mark.parametrize("which,value", [("pix_x_int", -1), ("pix_x_int", "W"), ("pix_y_int", "H"), ("cam_idx", "n_images")])
def test_out_of_range_lookups_read_nothing(fx, which, value):
    """The tables hold five cameras and the planes three images, so camera n_images casts a ray but has nothing to gather."""
    ds = dataset(fx, all_cameras=True)
    value = dict(W=int(fx["scene.width"]), H=int(fx["scene.height"]), n_images=int(fx["scene.n_real"])).get(value, value)
    ins = inputs(fx, "e")
    clean = ds.make_ray_batch(**ins)
    bad_rows = [0, 100, 256]                                      # first block, and the one lane of the second
    ins[which] = ins[which].clone()
    ins[which][bad_rows] = value
    with pytest.raises(IndexError, match="look-up"):
        ds.make_ray_batch(**ins)
    got = ds.make_ray_batch(**ins, validate=False)
    keep = torch.ones(257, dtype=torch.bool, device="cuda")
    keep[bad_rows] = False
    for k, v in got.items():
        if v is None:
            continue
        assert torch.equal(v[keep], clean[k][keep]), k
        if k in PLANES:
            assert torch.isnan(v[~keep]).all(), k
        else:
            assert torch.isfinite(v[~keep]).all(), k
    with pytest.raises(IndexError, match="camera index"):
        ins["cam_idx"][3] = 5
        ds.make_ray_batch(**ins)
    assert ds.make_ray_batch(**inputs(fx, "e"))["rgb"].isfinite().all()           # the status word is cleared per call


def seeded(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("patch,border,batching", [(1, 0, "all_images"), (2, 1, "all_images"), (3, 2, "single_image")])
def test_next_train_is_deterministic_and_in_range(fx, patch, border, batching):
    ds = dataset(fx, batch_size=300, patch_size=patch, num_border_pixels_to_mask=border, batching=batching)
    Wd, Ht, n_real = int(fx["scene.width"]), int(fx["scene.height"]), int(fx["scene.n_real"])
    a, b = ds.next_train(seeded(7)), ds.next_train(seeded(7))
    assert list(a) == list(b)
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k
    c = ds.next_train(seeded(8))
    assert not torch.equal(a["rgb"], c["rgb"])
    idx = ds.sample_train_indices(seeded(7))
    x, y, cam = idx["pix_x_int"].long(), idx["pix_y_int"].long(), idx["cam_idx"].long()
    num_patches = 300 // patch ** 2
    assert x.shape == y.shape == (num_patches, patch, patch)
    assert cam.shape == ((num_patches, 1, 1) if batching == "all_images" else (1,))
    x0, y0 = x[:, :1, :1], y[:, :1, :1]
    assert int(x0.min()) >= border and int(x0.max()) < Wd - border - patch + 1
    assert int(y0.min()) >= border and int(y0.max()) < Ht - border - patch + 1
    step = torch.arange(patch, device="cuda")
    assert torch.equal(x, (x0 + step[None, None, :]).expand_as(x))                          # a contiguous patch x patch block
    assert torch.equal(y, (y0 + step[None, :, None]).expand_as(y))
    assert int(cam.min()) >= 0 and int(cam.max()) < n_real
    images = torch.from_numpy(fx["scene.images"]).cuda()
    assert a["rgb"].shape == (num_patches, patch, patch, 3)
    assert torch.equal(a["rgb"], images[cam.expand_as(x) if batching == "all_images" else cam[0], y, x])
    assert torch.equal(a["cam_idx"][..., 0], cam.expand_as(x).float()) and torch.equal(a["camera_id"], a["cam_idx"][..., 0])
    assert (a["lossmult"] == 1).all() and a["lossmult"].shape == (num_patches, patch, patch, 1)


def test_next_train_bayer_mask(fx):
    ds = dataset(fx, batch_size=200, apply_bayer_mask=True)
    batch, idx = ds.next_train(seeded(3)), ds.sample_train_indices(seeded(3))
    want = R.bayer_mask(idx["pix_x_int"].cpu().numpy(), idx["pix_y_int"].cpu().numpy())
    assert same_bits(batch["lossmult"].cpu().numpy(), want)


# ------------------------------------------------------------------ the virtual-pose branch of next_train
N_REAL, CAM_NUM, VH, VW, V_BATCH = 6, 1, 12, 16, 40
FLIP = np.diag([1., -1., -1., 1.])


def virtual_scene(depth_value):
    """Six real cameras side by side looking down +z (OpenCV), nine virtual poses each a few centimetres off their real one, and
    a constant depth plane: every warp the selection loop can pick moves a pixel by less than two pixels."""
    rng = np.random.default_rng(5)
    K = np.array([[17.0, 0.0, 7.6], [0.0, 16.5, 5.7], [0.0, 0.0, 1.0]])
    real = np.stack([np.eye(4) for _ in range(N_REAL)])
    real[:, 0, 3] = 0.02 * np.arange(N_REAL)
    virtual = np.repeat(real, 9, axis=0)
    virtual[:, :3, 3] += rng.uniform(-0.05, 0.05, size=(N_REAL * 9, 3))
    return dict(images=rng.random((N_REAL, VH, VW, 3)).astype(np.float32), K=K,
                disp_images=np.full((N_REAL, VH, VW), depth_value, np.float32),
                real=real @ FLIP, virtual=virtual @ FLIP,                                   # OpenGL, as the loaders store them
                pixtocams=np.repeat(np.linalg.inv(K)[None], N_REAL * 10, axis=0))


def virtual_dataset(scene, **kw):
    from ucnerf_amd.internal import datasets as D
    return D.DeviceDataset(scene["images"], np.concatenate([scene["real"], scene["virtual"]]), scene["pixtocams"], 0.25, 8.0,
                           disp_images=scene["disp_images"], virtual_poses=scene["virtual"], cam_num=CAM_NUM,
                           compute_disp_metrics=True, load_sky_segments=False, batch_size=V_BATCH, **kw)


def test_next_train_virtual_branch():
    scene = virtual_scene(2.0)
    num_virtual = int(0.2 * V_BATCH)
    # the fixture's premise, on the CPU restatement of the warp: every (reference, source) pair keeps enough pixels
    for ref in range(3 * CAM_NUM, N_REAL):
        for src in range(N_REAL * 9):
            _, mask = oracle_warp.img_warping(scene["real"][ref] @ FLIP, scene["virtual"][src] @ FLIP, scene["disp_images"][ref],
                                              scene["K"])
            assert mask.sum() >= num_virtual, (ref, src, int(mask.sum()))
    ds = virtual_dataset(scene)
    assert ds.size == N_REAL and len(ds) == 1000
    idx, batch = ds.sample_train_indices(seeded(11)), ds.next_train(seeded(11))
    n = V_BATCH + num_virtual
    assert all(idx[k].shape == (n, 1, 1) for k in idx if k.endswith(("_src", "_ref")))
    src_cam, ref_cam = idx["cam_idx_with_src"][V_BATCH:, 0, 0], idx["cam_idx_with_ref"][V_BATCH:, 0, 0]
    assert int(ref_cam.min()) >= 3 * CAM_NUM and int(ref_cam.max()) < N_REAL and int(src_cam.min()) >= N_REAL
    assert len(set(src_cam.tolist())) == 1 and len(set(ref_cam.tolist())) == 1
    assert torch.equal(idx["cam_idx_with_src"][:V_BATCH], idx["cam_idx"]) and torch.equal(idx["cam_idx_with_ref"][:V_BATCH], idx["cam_idx"])
    assert torch.equal(idx["pixel_y_int_with_src"][:V_BATCH], idx["pix_x_int"])             # datasets.py:553, reproduced
    # the batch is the reference's on these indices (float64 restatement of _make_ray_batch, virtual branch)
    data = dict(images=scene["images"], disp_images=scene["disp_images"], camtoworlds=np.concatenate([scene["real"], scene["virtual"]])[:, :3],
                pixtocams=scene["pixtocams"], near=0.25, far=8.0, virtual_poses=True, load_disps=True)
    want = R.make_ray_batch(data, **{k: v.cpu().numpy().astype(np.int64) for k, v in idx.items()})
    check_layout(batch, want)
    for k, w in want.items():
        if w is not None:
            assert torch.equal(batch[k].cpu(), torch.from_numpy(w)), k
    assert float(batch["cam_idx"][V_BATCH:].min()) >= 3 * CAM_NUM and batch["cam_idx"].shape == (n, 1, 1)
    # fix_src_rows changes exactly the y of the real rays' cast pixels
    fixed = ds.sample_train_indices(seeded(11), fix_src_rows=True)
    for k in idx:
        if k != "pixel_y_int_with_src":
            assert torch.equal(idx[k], fixed[k]), k
    assert torch.equal(fixed["pixel_y_int_with_src"][:V_BATCH], idx["pix_y_int"])
    assert torch.equal(fixed["pixel_y_int_with_src"][V_BATCH:], idx["pixel_y_int_with_src"][V_BATCH:])
    assert not torch.equal(idx["pix_x_int"], idx["pix_y_int"])


def test_next_train_virtual_gives_up_on_an_empty_depth_plane(monkeypatch):
    """max_virtual_tries counts warps: the draws the `>= 3 * cam_num` condition rejects (half of them here) are not tries."""
    from ucnerf_amd.internal import datasets as D
    ds = virtual_dataset(virtual_scene(0.0))
    warps, warp = [], D.train_utils.img_warping
    monkeypatch.setattr(D.train_utils, "img_warping", lambda *a, **k: warps.append(1) or warp(*a, **k))
    with pytest.raises(RuntimeError, match="8 warps"):
        ds.next_train(seeded(1), max_virtual_tries=8)
    assert len(warps) == 8
    scene = virtual_scene(2.0)
    few = D.DeviceDataset(scene["images"][:3], np.concatenate([scene["real"][:3], scene["virtual"][:27]]), scene["pixtocams"][:30],
                          0.25, 8.0, disp_images=scene["disp_images"][:3], virtual_poses=scene["virtual"][:27], cam_num=CAM_NUM,
                          compute_disp_metrics=True, load_sky_segments=False, batch_size=V_BATCH)
    with pytest.raises(RuntimeError, match="3 \\* cam_num"):
        few.next_train(seeded(1))


# ------------------------------------------------------------------ the test path and the DataLoader surface
def test_dataloader_feeds_model_forward(fx):
    """`DataLoader(np.arange(len(ds)), batch_size=1, collate_fn=ds.collate_fn)` as train.py:75-81 writes it, with num_workers=0;
    the training batch goes through one training-route forward of the tiny model."""
    test_ds = dataset(fx, split="test")
    assert len(test_ds) == test_ds.size == int(fx["scene.n_real"])
    loader = torch.utils.data.DataLoader(np.arange(len(test_ds)), num_workers=0, shuffle=False, batch_size=1, collate_fn=test_ds.collate_fn)
    frames = list(loader)
    assert [int(i) for _, i in frames] == [0, 1, 2]
    for k in ("origins", "rgb", "disps", "camera_id"):
        assert torch.equal(frames[1][0][k].cpu(), torch.from_numpy(fx[f"d.out.{k}"])), k
    train_ds = dataset(fx, batch_size=64, seed=4)
    assert len(train_ds) == 1000
    loader = torch.utils.data.DataLoader(np.arange(len(train_ds)), num_workers=0, shuffle=True, batch_size=1, collate_fn=train_ds.collate_fn)
    batch = next(iter(loader))
    assert batch["origins"].shape == (64, 1, 1, 3) and batch["rgb"].shape == (64, 1, 1, 3)
    spec = rm.make_spec("tiny")
    model, _ = H.hip_model(spec, rm.init_state(spec, seed=21))
    model.train()
    renderings, _ = model(True, batch, 0.5, False)
    assert model.last_march_route == "train_graph"
    rgb = renderings[-1]["rgb"]
    assert rgb.numel() == 64 * 3 and torch.isfinite(rgb).all()


def test_from_dataset_reads_the_references_attributes(fx):
    """The one-line binding, on an object with the attributes the reference's `Dataset` has after its `__init__`."""
    import enum
    import types
    from ucnerf_amd.internal import datasets as D
    n_real = int(fx["scene.n_real"])
    config = types.SimpleNamespace(batch_size=64, world_size=1, patch_size=1, batching="all_images", num_border_pixels_to_mask=0,
                                   apply_bayer_mask=False, virtual_poses=False, compute_disp_metrics=True,
                                   compute_normal_metrics=False, load_sky_segments=True, compute_visibility=False)
    ref = types.SimpleNamespace(images=fx["scene.images"], camtoworlds=fx["scene.camtoworlds"][:n_real],
                                pixtocams=fx["scene.pixtocams"][:n_real], near=float(fx["scene.near"]), far=float(fx["scene.far"]),
                                disp_images=fx["scene.disp_images"], sky_segments=fx["scene.sky_segments"], normal_images=None,
                                alphas=None, distortion_params=None, pixtocam_ndc=None,
                                camtype=enum.Enum("ProjectionType", dict(PERSPECTIVE="perspective", FISHEYE="fisheye")).PERSPECTIVE,
                                split=enum.Enum("DataSplit", dict(TRAIN="train", TEST="test")).TRAIN, width=int(fx["scene.width"]),
                                height=int(fx["scene.height"]), render_path=False, _render_spherical=False, config=config)
    ds = D.DeviceDataset.from_dataset(ref)
    assert ds.size == n_real and len(ds) == 1000 and ds.camtype == "perspective"
    got, want = ds.make_ray_batch(**inputs(fx, "a")), run(fx, "a")
    assert list(got) == list(want)
    for k, w in want.items():
        assert (w is None and got[k] is None) or torch.equal(got[k], w), k
    ref.distortion_params = dict(k1=0.1)
    with pytest.raises(NotImplementedError, match="distortion"):
        D.DeviceDataset.from_dataset(ref)
    ref.distortion_params, ref.camtype = None, type(ref.camtype).FISHEYE
    with pytest.raises(NotImplementedError, match="fisheye"):
        D.DeviceDataset.from_dataset(ref)


def test_default_stream_follows_torchs_global_seed(fx):
    """seed=None: what torch.manual_seed (accelerate's set_seed(seed, device_specific=True), train.py:67) gave this process, so
    the ranks of one run draw different batches and one seed reproduces a run."""
    def first_batch(seed):
        torch.manual_seed(seed)
        return dataset(fx, batch_size=128).next_train()["rgb"]
    a, b, c = first_batch(5), first_batch(5), first_batch(6)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(dataset(fx, batch_size=128, seed=5).next_train()["rgb"], a)


def test_generate_ray_batch_spherical_frame(fx):
    """`render_camtype == 'pano'` (datasets.py:574-578): the frame is camera_utils.cast_spherical_rays of that camera's pose."""
    from ucnerf_amd.internal import camera_utils as cu
    ds = dataset(fx, split="test", render_path=True, render_spherical=True, width=7, height=5)
    got = ds.generate_ray_batch(2)
    want = cu.cast_spherical_rays(fx["scene.camtoworlds"][2], 5, 7, float(fx["scene.near"]), float(fx["scene.far"]))
    assert list(got) == list(want) and "rgb" not in got
    for k, w in want.items():
        assert got[k].shape == w.shape == (5, 7, w.shape[-1]) and same_bits(got[k].cpu().numpy(), w.cpu().numpy()), k
    assert torch.equal(got["origins"][0, 0].cpu(), torch.from_numpy(fx["scene.camtoworlds"][2][:, 3]).float())
