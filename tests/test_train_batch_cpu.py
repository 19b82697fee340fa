"""The device batch assembler (ucnerf_amd/internal/datasets.py), what can be held without a GPU: the numpy restatement the GPU
tests lean on against the reference's own output, the C declaration and its binding, and the host-side refusals and arithmetic."""
import json
import os
import re

import numpy as np
import pytest
import torch

import train_batch_ref as R
from ucnerf_amd import _lib
from ucnerf_amd.internal import datasets as D

CASES = ("a", "b", "c", "d", "e")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "train_batch.npz"))


def scene(fx, **kw):
    data = {k.split(".", 1)[1]: fx[k] for k in fx.files if k.startswith("scene.")}
    data.update(near=float(data["near"]), far=float(data["far"]), load_disps=True, load_segs=True)
    n_real = int(data["n_real"])
    if not kw.get("virtual_poses"):
        data["pixtocams"], data["camtoworlds"] = data["pixtocams"][:n_real], data["camtoworlds"][:n_real]
    data.update(kw)
    return data


def restated(fx, case, **kw):
    ins = {k.split(".in.", 1)[1]: fx[k].astype(np.int64) for k in fx.files if k.startswith(f"{case}.in.")}
    if case == "d":
        return R.generate_ray_batch(scene(fx, **kw), int(ins["cam_idx"]), int(fx["scene.width"]), int(fx["scene.height"]))
    return R.make_ray_batch(scene(fx, virtual_poses=case == "c", **kw), **ins)


@pytest.mark.parametrize("case", CASES)
def test_restatement_is_the_reference_bit_for_bit(fx, case):
    got = restated(fx, case)
    assert list(got) == json.loads(str(fx[f"{case}.keys"]))
    assert [k for k, v in got.items() if v is None] == json.loads(str(fx[f"{case}.none"]))
    for k, v in got.items():
        if v is None:
            continue
        want = fx[f"{case}.out.{k}"]
        assert v.dtype == np.float32 and want.dtype == np.float32
        assert v.shape == want.shape, (case, k, v.shape, want.shape)
        assert np.array_equal(v.view(np.uint32), want.view(np.uint32)), (case, k)


def test_fixture_covers_what_it_says(fx):
    assert fx["a.out.origins"].shape == (37, 1, 1, 3) and fx["e.out.origins"].shape == (257, 1, 1, 3)
    assert fx["b.out.rgb"].shape == (9, 2, 2, 3) and fx["b.out.disps"].shape == (9, 2, 2)
    assert fx["d.out.rgb"].shape == (12, 16, 3) and fx["d.out.camera_id"].shape == (12, 16)
    assert fx["c.out.origins"].shape == (44, 1, 1, 3) and fx["c.out.cam_idx"].shape == (44, 1, 1)       # no trailing axis
    n_real = int(fx["scene.n_real"])
    src, ref = fx["c.in.cam_idx_with_src"][37:], fx["c.in.cam_idx_with_ref"][37:]
    assert (src >= n_real).all() and (ref < n_real).all()                                             # distinct cast / look-up
    assert np.array_equal(fx["c.in.pixel_y_int_with_src"][:37], fx["c.in.pix_x_int"])                  # datasets.py:553
    assert np.any(fx["scene.images"] * 255 != np.round(fx["scene.images"] * 255))
    assert "datasets.py" in json.loads(str(fx["meta"]))["source"]


def test_header_declares_and_loader_binds_the_entry():
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"\bint\s+ucn_train_batch\s*\(", text)
    assert _lib.ABI_VERSION == 32
    args = _lib.SIGNATURES["ucn_train_batch"]
    assert len(args) == 36 and args[1] == _lib.c_i32 and args[-1] == _lib.c_vp and args[-2] == _lib.c_i32
    assert _lib.BATCH_MAX_PLANES == 4 and _lib.BATCH_BAYER_MASK == 1
    assert hasattr(_lib.load(), "ucn_train_batch")


def _bare():
    return object.__new__(D.DeviceDataset)          # the refusals below come before any state is read


def test_host_tensors_are_refused():
    px = torch.zeros(4, 1, 1, dtype=torch.int32)
    ds = _bare()
    ds.virtual_poses_enabled, ds.split = False, "train"
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ds.make_ray_batch(px, px, px)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ds.make_ray_batch(px.numpy(), px.numpy(), 0)
    ds.virtual_poses_enabled = True
    with pytest.raises(RuntimeError, match="pixel_x_int_with_src must be a CUDA tensor"):
        ds.make_ray_batch(px, px, px, pixel_x_int_with_src=px, pixel_y_int_with_src=px, cam_idx_with_src=px)
    with pytest.raises(RuntimeError, match="CUDA device"):
        D.DeviceDataset(np.zeros((1, 2, 2, 3), np.float32), np.eye(4)[None], np.eye(3)[None], 0.0, 1.0, device="cpu")


def test_a_foreign_projection_type_is_read_by_its_value():
    """The reference's `Dataset.camtype` is a member of its own enum class (datasets.py:306), equal to neither this package's
    member nor the string; `from_dataset` hands it over as it is."""
    import enum
    from ucnerf_amd.internal import camera_utils as cu
    foreign = enum.Enum("ProjectionType", dict(PERSPECTIVE="perspective", FISHEYE="fisheye"))
    assert foreign.PERSPECTIVE != cu.ProjectionType.PERSPECTIVE and foreign.PERSPECTIVE != "perspective"
    assert D.camtype_value(foreign.PERSPECTIVE) == "perspective" and D.camtype_value(cu.ProjectionType.PERSPECTIVE) == "perspective"
    assert D.camtype_value("panoroma") == "panoroma"
    assert cu._check_supported(None, None, D.camtype_value(foreign.PERSPECTIVE)) == 0
    assert cu._check_supported(None, None, D.camtype_value("panoroma")) == 1
    with pytest.raises(NotImplementedError, match="fisheye"):
        cu._check_supported(None, None, D.camtype_value(foreign.FISHEYE))


def test_worker_processes_are_refused(monkeypatch):
    ds = _bare()
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(RuntimeError, match="num_workers=0"):
        ds[0]
    with pytest.raises(RuntimeError, match="num_workers=0"):
        ds.collate_fn([0])


@pytest.mark.parametrize("batch_size,world_size,patch,border,width,height,virtual", [
    (8192, 1, 1, 0, 1920, 1280, False), (15000, 1, 1, 0, 1920, 1280, True), (4096, 2, 4, 3, 64, 48, False),
    (37, 1, 2, 1, 16, 12, True), (4, 1, 1, 0, 16, 12, True), (65536, 8, 0, 5, 1600, 900, True)])
def test_sampler_shape_arithmetic(batch_size, world_size, patch, border, width, height, virtual):
    got = D.sampler_shapes(batch_size, world_size, patch, border, width, height, virtual)
    assert got == R.sampler_shapes(batch_size, world_size, patch, border, width, height, virtual)
    p = max(patch, 1)
    num_patches = (batch_size // world_size) // p ** 2                                  # datasets.py:277-278, :483
    assert got["num_patches"] == num_patches and got["patch_size"] == p
    assert got["num_patches_for_virtual"] == (int(0.2 * num_patches) if virtual else 0)  # :485
    lo, hi = got["x_range"]
    assert lo == border and hi - 1 + (p - 1) == width - border - 1                      # the last patch ends inside the border
    lo, hi = got["y_range"]
    assert lo == border and hi - 1 + (p - 1) == height - border - 1
    with pytest.raises(ValueError, match="too large"):
        D.sampler_shapes(8, 1, 3, 0, width, height, virtual)
