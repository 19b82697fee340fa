"""The kernels that consume the field -- ucn_marching_cubes_* (csrc/mesh.hip), ucn_tsdf_integrate (tsdf.hip), ucn_img_warping /
ucn_warp_scatter_depth (warp.hip), ucn_image_metrics (metrics.hip), ucn_dense / ucn_apply_affine (heads.hip) -- at the launch
shapes and input classes their first tests do not reach, against oracle/ and the float64 / exact forms of
tests/extract_eval_ref.py.  tests/test_extract_eval_cpu.py proves on the host that the inputs are what the tests here say.

Through the C ABI where the Python wrapper would hide the case.  Device buffers are PAD elements longer than the length passed,
outputs are pre-filled, and the spare elements are checked afterwards.  `pytest -s` prints the lines of
profiles/extract_eval/report.txt."""
import numpy as np
import pytest
import torch

import extract_eval_ref as R
import helpers as H
from extract_eval_ref import PAD
from oracle import warp as owarp

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _lib():
    from ucnerf_amd import _lib as L
    return L, L.load(), L.stream()


def put(a, fill=0):
    """device copy of a host array, flat, with PAD spare elements of `fill` behind it"""
    t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    buf = torch.full((t.numel() + PAD,), fill, dtype=t.dtype, device="cuda")
    buf[:t.numel()] = t.cuda()
    return buf


def blank(n, fill=NAN, dtype=torch.float32):
    return torch.full((n + PAD,), fill, dtype=dtype, device="cuda")


def spare_ok(buf, n, fill=NAN):
    tail = buf[n:].cpu()
    return bool(torch.isnan(tail).all()) if fill != fill else bool((tail == fill).all())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def within(name, got, want, bar):
    """|got - want| <= bar element by element; returns the largest share of the bar used"""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, np.float64).reshape(-1)
    want, bar = np.asarray(want, np.float64).reshape(-1), np.asarray(bar, np.float64).reshape(-1)
    assert got.shape == want.shape and np.isfinite(got).all(), (name, got.shape, want.shape)
    diff = np.abs(got - want)
    share = float((diff / np.maximum(bar, 1e-300)).max()) if diff.size else 0.0
    assert not (diff > bar).any(), (name, int((diff > bar).sum()), float(diff.max()), share)
    return share


def refused(rc, *words):
    L, lib, st = _lib()
    msg = lib.ucn_last_error().decode()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)
    torch.cuda.synchronize()                                               # nothing was launched that could fault


# ================================================================== 1. marching cubes
def _mesh(vol, level, sp, **kw):
    from ucnerf_amd.internal import mesh
    v, f, n, vals = mesh.marching_cubes(torch.tensor(vol).cuda(), level, sp, **kw)
    assert vals is None
    return v.cpu().numpy(), f.cpu().numpy(), None if n is None else n.cpu().numpy()


def _is_the_restatement(name):
    vol, level, sp, want_v, want_f, want_n = R.restated(name)
    v, f, n = _mesh(vol, level, sp)
    assert v.shape == want_v.shape and f.shape == want_f.shape, (name, v.shape, want_v.shape, f.shape, want_f.shape)   # the two counts
    assert np.array_equal(f, want_f), name
    assert np.array_equal(bits(v), bits(want_v)), name
    if len(want_v):
        assert float(np.abs(n - want_n).max()) <= 2e-6, name
    return vol, level, sp, v, f, n


@pytest.mark.parametrize("name", list(R.SCAN_CASES))
def test_marching_cubes_scan_beyond_1024_blocks(name):
    """k_mc_scan with per = 2 (whole ranges, a range cut by n_blocks, idle threads) and per = 3"""
    vol, level, sp, v, f, n = _is_the_restatement(name)
    nb = (vol.size + 255) // 256
    sums = R.block_triangle_sums(vol, level)
    assert nb > 1024 and (sums[:1024] > 0).any() and (sums[1024:] > 0).any()


def test_marching_cubes_all_256_cases():
    """k_mc_faces' use of the table (edge_first_corner, the vinfo flag / popcount indexing) on every cube case"""
    vol, level, sp, v, f, n = _is_the_restatement("all_cases")
    hist = np.bincount(R.cube_cases(vol, level).reshape(-1), minlength=256)
    assert (hist[1:255] > 0).all()


@pytest.mark.parametrize("k", range(len(R.TIES_SPACINGS)))
def test_marching_cubes_ties_and_degenerate_faces(k):
    """values exactly at the level: equal to the restatement with degenerate faces; without them every face of B (float64 area >=
    1e-6 h^2) is kept in order with its indices and no face of A (two bit-identical vertices) is"""
    vol, level, sp, v, f, n = _is_the_restatement(f"ties{k}")
    A, B = R.degenerate_sets(v, f, sp)
    undecided = int((~A & ~B).sum())
    assert A.sum() > 0 and undecided <= 0.01 * len(f)
    v2, f2, n2 = _mesh(vol, level, sp, allow_degenerate=False)
    assert np.array_equal(bits(v2), bits(v))
    kept = R.kept_faces(f, f2)
    assert kept is not None, "the kept faces are not a subsequence of all faces: an index or the order changed"
    mask = np.zeros(len(f), bool)
    mask[kept] = True
    print(f"EXTRACT_EVAL ties spacing {sp}: {len(f)} faces, A {int(A.sum())} B {int(B.sum())} undecided {undecided}; device kept {len(f2)}, "
          f"of A {int((mask & A).sum())}, dropped of B {int((~mask & B).sum())}")
    assert not (~mask & B).any(), ("a face with area was dropped", int((~mask & B).sum()))
    assert not (mask & A).any(), ("a face with two identical vertices was kept", int((mask & A).sum()))


@pytest.mark.parametrize("name", list(R.CELL_CASES) + list(R.SMALL_CASES))
def test_marching_cubes_minimal_and_thin_volumes(name):
    """2 x 2 x 2, an axis of length 2 (every gradient one-sided), 256 k and 256 k + 1 points; with_normals=False changes nothing"""
    vol, level, sp, v, f, n = _is_the_restatement(name)
    v2, f2, n2 = _mesh(vol, level, sp, with_normals=False)
    assert n2 is None and np.array_equal(bits(v2), bits(v)) and np.array_equal(f2, f)


@pytest.mark.parametrize("fill", [-1.0, 1.0])
def test_marching_cubes_without_a_surface_emits_nothing(fill, monkeypatch):
    L, lib, st = _lib()

    def no_emit(*a):
        raise AssertionError("emit was launched for an empty mesh")
    monkeypatch.setattr(lib, "ucn_marching_cubes_emit", no_emit)
    v, f, n = _mesh(np.full((9, 7, 33), fill, np.float32), 0.0, (1.0, 1.0, 1.0))
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)


def test_marching_cubes_refusals():
    L, lib, st = _lib()
    vol, ws, counts = put(np.ones(64, np.float32)), blank(64 * 8), blank(2, 77, torch.int32)
    for X, Y, Z in ((1, 8, 8), (8, 1, 8), (8, 8, 1)):
        refused(lib.ucn_marching_cubes_count(vol.data_ptr(), X, Y, Z, 0.0, ws.data_ptr(), counts.data_ptr(), st), "at least 2 points")
    refused(lib.ucn_marching_cubes_count(vol.data_ptr(), 1024, 1024, 512, 0.0, ws.data_ptr(), counts.data_ptr(), st), "2^29")
    refused(lib.ucn_marching_cubes_count(vol.data_ptr(), 2048, 2048, 2048, 0.0, ws.data_ptr(), counts.data_ptr(), st), "2^29")
    for args in ((None, ws, counts), (vol, None, counts), (vol, ws, None)):
        p = [None if a is None else a.data_ptr() for a in args]
        refused(lib.ucn_marching_cubes_count(p[0], 4, 4, 4, 0.0, p[1], p[2], st), "null pointer")
    out = blank(64)
    refused(lib.ucn_marching_cubes_emit(None, 4, 4, 4, 0.0, 1.0, 1.0, 1.0, ws.data_ptr(), out.data_ptr(), None, None, st), "null pointer")
    refused(lib.ucn_marching_cubes_emit(vol.data_ptr(), 4, 4, 4, 0.0, 1.0, 1.0, 1.0, None, out.data_ptr(), None, None, st), "null pointer")
    assert bool((counts == 77).all()) and spare_ok(ws, 0) and spare_ok(out, 0)          # nothing ran


# ================================================================== 2. TSDF fusion
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("seed", R.TSDF_SEEDS)
@pytest.mark.parametrize("second_has_colour", [True, False])
def test_tsdf_integrate_two_calls_on_generated_scenes(seed, B, second_has_colour):
    """37 x 53 frames, 3001 voxels (some behind the cameras, on a camera's plane, outside the frusta), 30 % zero depth, a volume
    that already holds values / weights / colours, two calls of B views; weights exact, values and colours 2e-6 on the voxels the
    float64 form marks safe in every view"""
    L, lib, st = _lib()
    sc, s32, s64, safe = R.tsdf_expected(seed, B, second_has_colour)
    N, (Hh, Ww) = R.TSDF_N, R.TSDF_HW
    share = float(safe.mean())
    print(f"EXTRACT_EVAL tsdf seed {seed} B {B} colour on call 2 {second_has_colour}: safe share {share:.4f}")
    assert share >= 0.99
    world, Kd = put(sc["world"][0], NAN), put(sc["K"])
    vals, wts, cols = put(sc["values"], NAN), put(sc["weights"], NAN), put(sc["colors"], NAN)
    before_w = sc["weights"]
    for call in range(2):
        sl = slice(call * B, (call + 1) * B)
        with_colour = call == 0 or second_has_colour
        w2c, depth = put(R.tsdf_w2c(sc["c2w"][sl])), put(sc["depth"][sl], NAN)
        colour = put(sc["color"][sl], NAN) if with_colour else None
        cols_before = cols.clone()
        assert lib.ucn_tsdf_integrate(world.data_ptr(), N, w2c.data_ptr(), Kd.data_ptr(), depth.data_ptr(), L.ptr(colour), B, Hh, Ww,
                                      sc["truncation"], vals.data_ptr(), wts.data_ptr(), cols.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert spare_ok(vals, N) and spare_ok(wts, N) and spare_ok(cols, 3 * N)
        if not with_colour:
            assert torch.equal(cols.view(torch.int32), cols_before.view(torch.int32))   # the colour volume is bit-unchanged
        v, w, c = vals[:N].cpu().numpy(), wts[:N].cpu().numpy(), cols[:3 * N].cpu().numpy().reshape(N, 3)
        v32, w32, c32 = s32[call]
        assert np.array_equal(w[safe], w32[safe])
        ev, ec = float(np.abs(v[safe] - v32[safe]).max()), float(np.abs(c[safe] - c32[safe]).max())
        print(f"EXTRACT_EVAL tsdf seed {seed} B {B} call {call}: max |hip - oracle| values {ev:.2e} colours {ec:.2e} on safe voxels, "
              f"{int((w != w32).sum())} weights differ on unsafe ones")
        assert ev <= 2e-6 and ec <= 2e-6
        # on all voxels
        assert np.array_equal(w, np.rint(w)) and (w - before_w >= 0).all() and (w - before_w <= B).all()
        assert np.isfinite(v).all() and np.abs(v).max() <= 1.0 and np.isfinite(c).all()
        before_w = w


# ================================================================== 3. depth warp
def _scatter(lib, st, pts, mask, z, H, W, owner, out):
    p, m, zz = put(pts, NAN), put(mask, 9), put(z, NAN)
    assert lib.ucn_warp_scatter_depth(p.data_ptr(), m.data_ptr(), zz.data_ptr(), H, W, owner.data_ptr(), out.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert spare_ok(owner, H * W, -1) and spare_ok(out, H * W)
    return out[:H * W].cpu().numpy().reshape(H, W)


@pytest.mark.parametrize("H,W", [(37, 53), (480, 640)])
def test_warp_scatter_is_the_last_writer_bit_for_bit(H, W):
    """ucn_warp_scatter_depth on its own inputs has an exact answer: out[int(v), int(u)] = z of the last masked source in
    row-major order.  Twice into the same owner map / output without clearing: the call clears them itself."""
    L, lib, st = _lib()
    owner, out = blank(H * W, -1, torch.int32), blank(H * W)
    for seed in (1, 2):
        pts, mask, z = R.scatter_inputs(H, W, seed)
        want, writers = R.scatter_expected(pts, mask, z, H, W)
        assert writers.max() >= 24
        got = _scatter(lib, st, pts, mask, z, H, W, owner, out)
        wrong = bits(got) != bits(want)
        assert not wrong.any(), (seed, int(wrong.sum()), "pixels differ; writers there", writers[wrong][:8])


def test_img_warping_bracket_and_mask():
    L, lib, st = _lib()
    depth, rel, K = R.warp_scene()
    Hh, Ww = depth.shape
    n = Hh * Ww
    uv64, m64, z64 = R.img_warping64(depth, rel, K)
    uv32, m32 = owarp.img_warping(rel, np.eye(4, dtype=np.float32), depth, K)
    d, pts, mask, z = put(depth, NAN), blank(2 * n), blank(n, 9, torch.uint8), blank(n)
    rel34 = np.ascontiguousarray(rel[:3], np.float32)
    assert lib.ucn_img_warping(d.data_ptr(), rel34.ctypes.data, K.ctypes.data, Hh, Ww, pts.data_ptr(), mask.data_ptr(), z.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert spare_ok(pts, 2 * n) and spare_ok(mask, n, 9) and spare_ok(z, n)
    uv, m = pts[:2 * n].cpu().numpy().reshape(Hh, Ww, 2), mask[:n].cpu().numpy().reshape(Hh, Ww)
    ok = depth > 0
    H.bracket("ucn_img_warping 37x53 projected pixel, depth > 0", np.abs(uv32 - uv64)[ok], np.abs(uv - uv64)[ok], 2.0)
    # the source depth: X, Y (2 roundings each), the products with d, a 3-term fmaf chain and the translation -- 8 roundings at most
    P = np.abs(np.stack([(np.arange(Ww)[None] - float(K[0, 2])) / float(K[0, 0]) * depth, (np.arange(Hh)[:, None] - float(K[1, 2])) / float(K[1, 1]) * depth,
                         depth.astype(np.float64)], 0))
    zbar = 8 * R.U32 * (np.einsum("c,chw->hw", np.abs(rel[2, :3].astype(np.float64)), P) + abs(float(rel[2, 3])))
    share = within("ucn_img_warping z_src", z[:n], z64, zbar)
    print(f"EXTRACT_EVAL ucn_img_warping 37x53 source depth: largest share of the derived bar {share:.3f}")
    assert set(np.unique(m)) <= {0, 1}
    assert not ((m.astype(bool) != m64) & ~R.warp_edge(uv64, Hh, Ww)).any()
    assert not m[~ok].any() and (~ok).sum() > 100 and 100 < m.sum() < ok.sum()
    # no pixels: returns 0 before looking at any pointer, launches nothing
    assert lib.ucn_img_warping(None, None, None, 0, 53, None, None, None, st) == 0
    assert lib.ucn_img_warping(None, None, None, 37, 0, None, None, None, st) == 0
    assert lib.ucn_warp_scatter_depth(None, None, None, 0, 53, None, None, st) == 0
    torch.cuda.synchronize()


# ================================================================== 4. image metrics
def _metrics(lib, st, pred, gt):
    h, w = pred.shape[:2]
    ws = torch.full((int(lib.ucn_image_metrics_ws_bytes(h, w)) + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((3 + PAD,), NAN, dtype=torch.float64, device="cuda")
    p, g = put(pred, NAN), put(gt, NAN)
    assert lib.ucn_image_metrics(p.data_ptr(), g.data_ptr(), h, w, ws.data_ptr(), out.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool((ws[-PAD:] == 0xA5).all()) and bool(torch.isnan(out[3:]).all())
    return out[:3].cpu().tolist()


@pytest.mark.parametrize("kind", R.METRIC_KINDS)
@pytest.mark.parametrize("h,w", R.METRIC_SIZES)
def test_image_metrics_at_block_boundaries_and_on_quantisation_steps(h, w, kind):
    L, lib, st = _lib()
    pred, gt = R.metric_images(h, w, kind)
    psnr, ssim, mse = R.metrics_expected(pred, gt)
    got = _metrics(lib, st, pred, gt)
    if kind == "identical":
        assert got[0] == float("inf") and got[1] == 1.0 and got[2] == 0.0
    else:
        assert abs(got[0] - psnr) <= 1e-9
        assert abs(got[2] - mse) <= 1e-12 * mse
    assert abs(got[1] - ssim) <= 1e-12


def test_image_metrics_refusals():
    L, lib, st = _lib()
    img, ws, out = put(np.zeros(7 * 7 * 3, np.float32)), blank(1024), torch.full((3,), NAN, dtype=torch.float64, device="cuda")
    for h, w in ((6, 7), (7, 6), (6, 300), (0, 7)):
        refused(lib.ucn_image_metrics(img.data_ptr(), img.data_ptr(), h, w, ws.data_ptr(), out.data_ptr(), st), "7 x 7")
    assert bool(torch.isnan(out).all()) and spare_ok(ws, 0)


# ================================================================== 5. colour-correction head
_SHARES = {}


@pytest.mark.parametrize("M,K,Nout", R.DENSE_SHAPES)
def test_dense_against_float64(M, K, Nout):
    """one thread per output, a k-sequential fmaf chain: (K + 1) 2^-24 (sum |x||w| + |b|) per element"""
    L, lib, st = _lib()
    x, w, b = R.dense_inputs(M, K, Nout)
    xd, wd, bd = put(x, NAN), put(w, NAN), put(b, NAN)
    for relu in (0, 1):
        for bias in (b, None):
            y = blank(M * Nout)
            assert lib.ucn_dense(xd.data_ptr(), wd.data_ptr(), None if bias is None else bd.data_ptr(), M, K, Nout, relu, y.data_ptr(), st) == 0
            torch.cuda.synchronize()
            assert spare_ok(y, M * Nout)
            want, bar = R.dense64(x, w, bias, relu)
            share = within(f"ucn_dense {M}x{K}->{Nout} relu {relu} bias {bias is not None}", y[:M * Nout], want, bar)
            _SHARES["ucn_dense"] = max(_SHARES.get("ucn_dense", 0.0), share)
            if relu:
                assert float(y[:M * Nout].min()) >= 0.0
    print(f"EXTRACT_EVAL ucn_dense up to {M}x{K}->{Nout}: largest share of the derived bar so far {_SHARES['ucn_dense']:.3f}")
    y = blank(8)
    assert lib.ucn_dense(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 0, K, Nout, 1, y.data_ptr(), st) == 0
    assert lib.ucn_dense(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), M, K, 0, 1, y.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert spare_ok(y, 0)


@pytest.mark.parametrize("N", [1, 255, 257, 1000])
@pytest.mark.parametrize("S", [0, 1, 33, 128])
def test_apply_affine_against_float64(N, S):
    """S = 0: no sky blend (sky_rgb = NULL); rows scrambled over 7 cameras, and ray_to_row = NULL (row 0)"""
    L, lib, st = _lib()
    rgb, A, rows, wts, sky, A_sky = R.affine_inputs(N, max(S, 1))
    rd, Ad, rowd, wd, sd, Asd = put(rgb, NAN), put(A, NAN), put(rows, -1), put(wts, NAN), put(sky, NAN), put(A_sky, NAN)
    for use_rows in (True, False):
        out = blank(3 * N)
        assert lib.ucn_apply_affine(rd.data_ptr(), Ad.data_ptr(), rowd.data_ptr() if use_rows else None, wd.data_ptr() if S else None, S,
                                    sd.data_ptr() if S else None, Asd.data_ptr() if S else None, N, out.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert spare_ok(out, 3 * N)
        want, bar = R.affine64(rgb, A, rows if use_rows else None, *((wts, sky, A_sky) if S else ()))
        share = within(f"ucn_apply_affine N {N} S {S} rows {use_rows}", out[:3 * N], want, bar)
        _SHARES["ucn_apply_affine"] = max(_SHARES.get("ucn_apply_affine", 0.0), share)
    print(f"EXTRACT_EVAL ucn_apply_affine up to N {N} S {S}: largest share of the derived bar so far {_SHARES['ucn_apply_affine']:.3f}")


def test_apply_affine_refusals():
    L, lib, st = _lib()
    rgb, A, rows, wts, sky, A_sky = R.affine_inputs(9, 4)
    rd, Ad, wd, sd, Asd, out = put(rgb), put(A), put(wts), put(sky), put(A_sky), blank(27)
    refused(lib.ucn_apply_affine(rd.data_ptr(), Ad.data_ptr(), None, None, 4, sd.data_ptr(), Asd.data_ptr(), 9, out.data_ptr(), st), "sky blend")
    refused(lib.ucn_apply_affine(rd.data_ptr(), Ad.data_ptr(), None, wd.data_ptr(), 4, sd.data_ptr(), None, 9, out.data_ptr(), st), "sky blend")
    refused(lib.ucn_apply_affine(None, Ad.data_ptr(), None, None, 0, None, None, 9, out.data_ptr(), st), "null pointer")
    assert lib.ucn_apply_affine(None, None, None, None, 0, None, None, 0, None, st) == 0
    assert spare_ok(out, 0)
