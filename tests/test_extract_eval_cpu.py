"""The inputs of tests/test_extract_eval_gpu.py meet the conditions that their tests state, and the restatements the kernels are
held to agree with each other on them -- all on the host (tests/extract_eval_ref.py draws the inputs, oracle/ restates)."""
import time

import numpy as np
import pytest

import extract_eval_ref as R
from oracle import marching
from oracle import warp as owarp


# ================================================================== marching cubes
@pytest.mark.parametrize("name", list(R.SCAN_CASES))
def test_scan_volumes_reach_the_multi_block_loop_and_restate_quickly(name):
    t0 = time.perf_counter()
    vol, level, sp, v, f, n = R.restated(name)
    spent = time.perf_counter() - t0
    nb = (vol.size + 255) // 256
    per = (nb + 1023) // 1024
    sums = R.block_triangle_sums(vol, level)
    print(f"EXTRACT_EVAL scan {name}: {vol.shape} {nb} blocks per {per}, {len(v)} vertices {len(f)} triangles, restated in {spent:.1f} s")
    assert nb > 1024 and per == {"per2_ragged": 2, "per2_clipped": 2, "per3_odd": 3}[name]
    assert (sums[:1024] > 0).any() and (sums[1024:] > 0).any() and int(sums.sum()) == len(f)
    # every [lo, hi) range of k_mc_scan has triangles in its first and in its last block, up to the slab x = X - 1 (no cells)
    lo = np.arange(0, nb, per)
    hi = np.minimum(lo + per, nb)
    cells = hi <= (vol.shape[0] - 1) * vol.shape[1] * vol.shape[2] // 256
    assert cells.sum() >= 0.98 * len(lo) and (sums[lo[cells]] > 0).all() and (sums[hi[cells] - 1] > 0).all()
    assert (nb % per != 0) == (name == "per2_clipped")                     # there the last range is cut by min(lo + per, n_blocks)
    assert (nb + per - 1) // per < 1024                                    # threads with lo >= n_blocks exist
    assert 5000 <= len(f) <= 60000 and spent < 20.0


def test_random_volume_holds_every_cube_case_and_its_mesh_has_no_cracks():
    vol, level, sp, v, f, n = R.restated("all_cases")
    hist = np.bincount(R.cube_cases(vol, level).reshape(-1), minlength=256)
    assert (hist[1:255] > 0).all(), np.nonzero(hist[1:255] == 0)[0] + 1
    assert len(f) == int(marching.tables()[1][R.cube_cases(vol, level)].sum())
    consistent, on_border = R.open_edges_on_border(v, f, vol.shape, sp)
    assert consistent and on_border


@pytest.mark.parametrize("k", range(len(R.TIES_SPACINGS)))
def test_tie_volume_has_collapsed_faces_and_few_undecided_ones(k):
    vol, level, sp, v, f, n = R.restated(f"ties{k}")
    assert 0.25 < float((vol == 0).mean()) < 0.35
    A, B = R.degenerate_sets(v, f, sp)
    undecided = int((~A & ~B).sum())
    print(f"EXTRACT_EVAL ties spacing {sp}: {len(f)} faces, A (two identical vertices) {int(A.sum())}, B (area >= 1e-6 h^2) {int(B.sum())}, "
          f"undecided {undecided}")
    assert A.sum() > 100 and B.sum() > 1000 and undecided <= 0.01 * len(f)
    assert np.array_equal(R.kept_faces(f, f[B]), np.nonzero(B)[0])          # the matcher finds a subsequence where it is


def test_cell_cases_are_what_they_say():
    for name, case in R.CELL_CASES.items():
        vol = R.cell_volume(case)
        assert int(R.cube_cases(vol, 0.0)[0, 0, 0]) == case, name
        assert len(R.restated(name)[4]) == int(marching.tables()[1][case]) > 0
    for name, shape in R.SMALL_CASES.items():
        assert len(R.restated(name)[4]) > 0, name
    assert np.prod(R.SMALL_CASES["256k_points"]) % 256 == 0 and np.prod(R.SMALL_CASES["256k_plus_1"]) % 256 == 1


# ================================================================== TSDF fusion
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("seed", R.TSDF_SEEDS)
@pytest.mark.parametrize("second_has_colour", [True, False])
def test_tsdf_scenes_are_safe_and_the_oracle_is_the_float64_form_there(seed, B, second_has_colour):
    sc, s32, s64, safe = R.tsdf_expected(seed, B, second_has_colour)
    assert R.TSDF_N % 256 != 0 and 0.25 < float((sc["depth"] == 0).mean()) < 0.35
    share = float(safe.mean())
    hit = [int((s32[c][1] > (sc["weights"] if c == 0 else s32[0][1])).sum()) for c in range(2)]
    print(f"EXTRACT_EVAL tsdf seed {seed} B {B}: safe share {share:.4f}, voxels updated per call {hit}")
    assert share >= 0.99 and not safe[:6].any()                           # the voxels on camera 0's plane are marked
    assert min(hit) >= (60 if B == 1 else 250)
    for (v32, w32, c32), (v64, w64, c64) in zip(s32, s64):
        assert np.array_equal(w32[safe], w64[safe])
        assert np.abs(v32[safe] - v64[safe]).max() <= 2e-6 and np.abs(c32[safe] - c64[safe]).max() <= 2e-6
        assert np.abs(v32).max() <= 1.0
    if not second_has_colour:
        assert np.array_equal(s32[1][2], s32[0][2])
    assert (s32[1][1] - s32[0][1]).max() <= B and (s32[0][1] - sc["weights"]).max() <= B


# ================================================================== depth warp
@pytest.mark.parametrize("H,W", [(37, 53), (480, 640)])
def test_scatter_inputs_collide(H, W):
    pts, mask, z = R.scatter_inputs(H, W, 1)
    t0 = time.perf_counter()
    want, writers = R.scatter_expected(pts, mask, z, H, W)
    spent = time.perf_counter() - t0
    m = mask.astype(bool)
    shared = writers[pts[m, 1].astype(np.int64), pts[m, 0].astype(np.int64)] > 1
    assert shared.mean() > 1 / 3 and writers.max() >= 24 and spent < 5.0
    assert 0.4 < m.mean() < 0.6 and (np.diff(mask.astype(int)) != 0).mean() > 0.5
    assert (pts[m, 0] > W - 1).any() and (pts[m, 0] == 0).any() and (pts[m, 1] == 0).any() and (z[m] < 0).any()
    assert (pts[m] != np.floor(pts[m])).mean() > 0.9 and np.isnan(pts[~m]).any()
    # numpy's own indexed assignment (oracle/warp.py) has the same last-writer semantics
    out = np.zeros((H, W), np.float32)
    xy = pts[m].astype(np.int64)
    out[xy[:, 1], xy[:, 0]] = z[m]
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


def test_warp_oracle_against_the_float64_form():
    depth, rel, K = R.warp_scene()
    H, W = depth.shape
    uv64, m64, z64 = R.img_warping64(depth, rel, K)
    uv, m = owarp.img_warping(rel, np.eye(4, dtype=np.float32), depth, K)   # inv(I) @ rel = rel
    ok = depth > 0
    assert 0.15 < float((~ok).mean()) < 0.35 and float(z64[ok].min()) > 1.0
    assert 0.2 < float(m64[ok].mean()) < 0.9                                # part of the frame leaves the source camera
    e = np.abs(uv - uv64)[ok]
    assert 1e-7 < e.max() < 1e-3
    assert not ((m != m64) & ~R.warp_edge(uv64, H, W)).any() and not m[~ok].any()


# ================================================================== image metrics
@pytest.mark.parametrize("kind", R.METRIC_KINDS)
def test_metric_images_sit_on_the_steps(kind):
    assert (22 - 6) * (22 - 6) == 256 and (22 - 6) * (23 - 6) == 272 and (263 - 6) == 257 and 19 * 27 == 513
    for h, w in R.METRIC_SIZES:
        pred, gt = R.metric_images(h, w, kind)
        assert pred.dtype == np.float32 and gt.dtype == np.float32 and pred.shape == (h, w, 3)
        k = np.rint(gt.astype(np.float64) * 255)
        assert np.array_equal((k / 255).astype(np.float32), gt) and gt.max() == 1.0 and gt.min() == 0.0
        psnr, ssim, mse = R.metrics_expected(pred, gt)
        if kind == "identical":
            assert psnr == float("inf") and ssim == 1.0 and mse == 0.0
        else:
            assert np.isfinite(psnr) and mse > 0 and ssim < 1.0


# ================================================================== colour-correction head
def test_dense_and_affine_bars_hold_for_a_float32_evaluation():
    """the derived bars are met by a plain float32 evaluation in the kernels' order of operations"""
    f32 = np.float32
    for M, K, N in R.DENSE_SHAPES:
        x, w, b = R.dense_inputs(M, K, N)
        want, bar = R.dense64(x, w, b, False)
        s = np.zeros((M, N), f32)
        for k in range(K):
            s = (s.astype(np.float64) + x[:, k:k + 1].astype(np.float64) * w[:, k][None].astype(np.float64)).astype(f32)     # fmaf: one rounding
        assert (np.abs((s + b[None]).astype(np.float64) - want) <= bar).all(), (M, K, N)
    assert {M * N for M, K, N in R.DENSE_SHAPES} >= {255, 256, 257}
    for N in (1, 255, 257, 1000):
        for S in (1, 33, 128):
            rgb, A, rows, wts, sky, A_sky = R.affine_inputs(N, S)
            want, bar = R.affine64(rgb, A, rows, wts, sky, A_sky)
            acc = np.zeros(N, f32)
            for s_ in range(S):
                acc = acc + wts[:, s_]
            a, bs = A[rows].reshape(-1, 3, 4), A_sky[rows].reshape(-1, 3, 4)
            dot = lambda m, v: ((m[:, :, 0] * v[:, 0:1] + m[:, :, 1] * v[:, 1:2]) + m[:, :, 2] * v[:, 2:3]) + m[:, :, 3]
            got = dot(a, rgb) + (f32(1) - acc)[:, None] * dot(bs, sky)
            assert got.dtype == f32 and (np.abs(got.astype(np.float64) - want) <= bar).all(), (N, S)
            if N >= 7:
                assert (wts.sum(1) > 1.5).any() and set(rows.tolist()) == set(range(R.AFFINE_ROWS)) and (np.diff(rows) < 0).any()
