"""Inputs and float64 / exact reference forms for the extraction and evaluation kernels -- csrc/mesh.hip, tsdf.hip, warp.hip,
metrics.hip, heads.hip -- where oracle/ has no form of its own.  Host only: tests/test_extract_eval_cpu.py proves that the inputs
drawn here meet the conditions their tests state (all cube cases present, safe share, undecided faces, restatement timings),
tests/test_extract_eval_gpu.py holds the kernels to the restatements on the same inputs from the same seeds.

Bounds are rounding counts times the float64 sum of ABSOLUTE terms (`mag`), as in tests/train_tail_ref.py; none is measured."""
import functools

import numpy as np

from oracle import marching
from oracle import tsdf as otsdf

U32 = 2.0 ** -24
PAD = 5                                                                     # spare elements behind every device buffer
F32 = np.float32


# ================================================================== marching cubes: volumes
def _axes(shape):
    return np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")


def scan_volume(shape, seed):
    """A tilted plane plus smooth waves: z = f(x, y) is crossed once in every (x, y) row of the lattice, so every 256-point block
    of k_mc_count (x slowest, z fastest) owns vertices and triangles and every [lo, hi) range of k_mc_scan has non-zero sums on
    both sides of its ends.  About 2 X Y triangles."""
    g = np.random.default_rng(seed)
    X, Y, Z = _axes(shape)
    v = Z - 0.31 * X - 0.17 * Y + 0.12 * np.sin(5.3 * X + 1.1) * np.cos(4.1 * Y - 0.4) + 0.004 * g.normal(size=shape)
    return v.astype(F32)


SCAN_CASES = {"per2_ragged": ((70, 64, 64), 11, 0.0, (1.0, 1.0, 1.0)),       # 1120 blocks: per = 2, threads 560.. idle
              "per2_clipped": ((65, 65, 65), 13, -0.01, (1.0, 1.0, 1.0)),    # 1073 blocks: per = 2, hi clipped to n_blocks in thread 536
              "per3_odd": ((129, 64, 65), 12, 0.02, (0.5, 1.0, 0.25))}      # 2097 blocks: per = 3, rows of 65 straddle the blocks


def random_volume(shape, seed):
    """independent values, random sign, magnitude in [0.5, 1.5]: every cube case is equally likely"""
    g = np.random.default_rng(seed)
    return (g.choice([-1.0, 1.0], size=shape) * g.uniform(0.5, 1.5, size=shape)).astype(F32)


ALL_CASES_SHAPE, ALL_CASES_SEED = (20, 19, 21), 7


def ties_volume(shape=(24, 19, 22), seed=21):
    """small integers with ~30 % exactly at the level 0: t is exactly 0 or 1 on every edge that touches a zero"""
    g = np.random.default_rng(seed)
    v = g.choice([-2.0, -1.0, 1.0, 2.0], size=shape)
    v[g.random(shape) < 0.3] = 0.0
    return v.astype(F32)


TIES_SPACINGS = ((1.0, 1.0, 1.0), (0.3, 0.7, 1.1))

# 2 x 2 x 2: inside corners (corner c = x + 2 y + 4 z) of one cell
CELL_CASES = {"one_corner": 0x01, "edge": 0x03, "face_diagonal_ambiguous": 0x09, "body_diagonal": 0x81, "checkerboard": 0x69,
              "all_but_one": 0xFE, "half": 0x0F, "three_on_a_face": 0x07}


def cell_volume(case, seed=0):
    g = np.random.default_rng(seed + case)
    v = g.uniform(0.5, 1.5, size=8)
    for c in range(8):
        if (case >> c) & 1:
            v[c] = -v[c]
    return np.ascontiguousarray(v.reshape(2, 2, 2).transpose(2, 1, 0)).astype(F32)      # [x, y, z], c = x + 2 y + 4 z


SMALL_CASES = {"2x9x9": (2, 9, 9), "9x2x9": (9, 2, 9), "9x9x2": (9, 9, 2), "256k_points": (8, 8, 8), "256k_plus_1": (3, 9, 19),
               "2x2x300": (2, 2, 300)}


def cube_cases(vol, level):
    """case index of every cell, [X-1, Y-1, Z-1], from vol < level alone (bit c = corner x + 2 y + 4 z)"""
    inside = np.asarray(vol, F32) < F32(level)
    X, Y, Z = inside.shape
    cube = np.zeros((X - 1, Y - 1, Z - 1), np.int64)
    for c in range(8):
        cx, cy, cz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        cube |= inside[cx:X - 1 + cx, cy:Y - 1 + cy, cz:Z - 1 + cz].astype(np.int64) << c
    return cube


def block_triangle_sums(vol, level):
    """triangles per 256-point block of k_mc_count (a cell belongs to the block of its corner 0)"""
    X, Y, Z = vol.shape
    per_point = np.zeros((X, Y, Z), np.int64)
    per_point[:-1, :-1, :-1] = marching.tables()[1][cube_cases(vol, level)]
    flat = per_point.reshape(-1)
    nb = (flat.size + 255) // 256
    return np.pad(flat, (0, nb * 256 - flat.size)).reshape(nb, 256).sum(1)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(volume, level, spacing, verts, faces, normals) of a named case, computed once per process"""
    if name in SCAN_CASES:
        shape, seed, level, sp = SCAN_CASES[name]
        vol = scan_volume(shape, seed)
    elif name == "all_cases":
        vol, level, sp = random_volume(ALL_CASES_SHAPE, ALL_CASES_SEED), 0.0, (1.0, 1.0, 1.0)
    elif name.startswith("ties"):
        vol, level, sp = ties_volume(), 0.0, TIES_SPACINGS[int(name[4:])]
    elif name in CELL_CASES:
        vol, level, sp = cell_volume(CELL_CASES[name]), 0.0, (1.0, 2.0, 0.5)
    else:
        vol, level, sp = random_volume(SMALL_CASES[name], 31 + len(name)), 0.0, (0.5, 1.0, 2.0)
    v, f, n = marching.marching_cubes(vol, level, sp)
    for a in (vol, v, f, n):
        a.setflags(write=False)
    return vol, level, sp, v, f, n


def degenerate_sets(verts, faces, spacing):
    """A = faces with two bit-identical vertex positions (what skimage's allow_degenerate=False removes); B = faces whose float64
    area is at least 1e-6 (smallest spacing)^2.  Boolean masks over the faces; a face in neither may be kept or dropped."""
    p = [verts[faces[:, k]] for k in range(3)]
    same = lambda a, b: (a.view(np.uint32) == b.view(np.uint32)).all(axis=1)
    A = same(p[0], p[1]) | same(p[1], p[2]) | same(p[0], p[2])
    q = [x.astype(np.float64) for x in p]
    area = 0.5 * np.linalg.norm(np.cross(q[1] - q[0], q[2] - q[0]), axis=1)
    B = area >= 1e-6 * min(spacing) ** 2
    assert not (A & B).any()
    return A, B


def kept_faces(all_faces, got):
    """indices into all_faces of the rows of `got`, matched in order (earliest match); None if got is no subsequence"""
    keep, j = [], 0
    for row in got:
        while j < len(all_faces) and not np.array_equal(all_faces[j], row):
            j += 1
        if j == len(all_faces):
            return None
        keep.append(j)
        j += 1
    return np.asarray(keep, np.int64)


def open_edges_on_border(verts, faces, shape, spacing):
    """(every undirected edge at most twice and every directed edge once, every edge used once lies on the volume's border)"""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    _, cd = np.unique(e, axis=0, return_counts=True)
    und, cu = np.unique(np.sort(e, 1), axis=0, return_counts=True)
    pts = verts[und[cu == 1].reshape(-1)].astype(np.float64) / np.asarray(spacing, np.float64)
    on_border = ((pts <= 1e-6) | (pts >= np.asarray(shape) - 1 - 1e-6)).any(axis=1)
    return int(cd.max()) == 1 and int(cu.max()) == 2, bool(on_border.all())


# ================================================================== TSDF fusion
TSDF_N, TSDF_HW, TSDF_TRUNC = 3001, (37, 53), 1.0
TSDF_SEEDS = (3, 4)


def _rot(g, scale):
    w = g.normal(size=3) * scale
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def tsdf_scene(seed, B):
    """Two successive calls of B views each onto a volume that already holds values / weights / colours.  Cameras near the origin
    looking down -z (OpenGL axes, tsdf.py:150-152), points in a box of 2.5 units around them: about half behind a camera, most
    of the rest outside the 37 x 53 frustum of a 50 px focal length; the first points lie ON camera 0's plane (zc = 0)."""
    g = np.random.default_rng(seed)
    H, W = TSDF_HW
    N = TSDF_N
    pts = g.uniform(-2.5, 2.5, size=(3, N))
    pts[:, N // 2:] = pts[:, N // 2:] * np.array([[0.45], [0.3], [1.0]])             # more of them inside the frusta
    pts[2, N // 2:] = -np.abs(pts[2, N // 2:]) - 0.3
    c2w = np.tile(np.eye(4), (2 * B, 1, 1))
    for i in range(2 * B):
        c2w[i, :3, :3] = _rot(g, 0.15)
        c2w[i, :3, 3] = g.uniform(-0.3, 0.3, size=3)
    c2w = c2w.astype(F32)
    plane = c2w[0].astype(np.float64)
    for j in range(6):                                                      # zc = 0 (j < 3) or ~1e-8: on camera 0's plane
        local = np.array([g.uniform(-1, 1), g.uniform(-1, 1), 0.0 if j < 3 else 1e-8])
        pts[:, j] = plane[:3, :3] @ local + plane[:3, 3]
    world = np.concatenate([pts, np.ones((1, N))], axis=0).astype(F32)[None]          # [1, 4, N]
    K = np.array([[50.0, 0.0, 26.1], [0.0, 49.5, 18.3], [0.0, 0.0, 1.0]], F32)
    depth = g.uniform(0.4, 3.5, size=(2 * B, 1, H, W)).astype(F32)
    depth[g.random(depth.shape) < 0.3] = 0.0
    color = g.random((2 * B, 3, H, W)).astype(F32)
    values = g.uniform(-1, 1, size=N).astype(F32)
    weights = g.integers(0, 4, size=N).astype(F32)
    colors = g.random((N, 3)).astype(F32)
    return dict(world=world, c2w=c2w, K=K, depth=depth, color=color, values=values, weights=weights, colors=colors, B=B,
                truncation=TSDF_TRUNC)


def tsdf_w2c(c2w):
    """what the kernel is handed: rows 0..2 of the float32 inverse, formed as oracle/tsdf.py forms it"""
    return np.ascontiguousarray(np.linalg.inv(c2w.astype(np.float64)).astype(F32)[:, :3, :])


def tsdf_integrate64(world, c2w, K, depth, color, truncation, values, weights, colors):
    """tsdf.py:131-219 in float64 on the float32 inputs (the float32 w2c included).  In place on float64 arrays; returns the
    voxels that are UNSAFE in some view: a float32 evaluation may take another branch there.
      - a projection within 1e-4 px of a rounding boundary of the nearest sample (this contains the voxels whose two nearest
        pixels hold different depths there), or not finite
      - |zc| < 1e-6
      - |dist + truncation| < 1e-5 max(1, |zc|): the `dist > -truncation` decision"""
    B, _, H, W = depth.shape
    w2c = np.linalg.inv(c2w.astype(np.float64)).astype(F32).astype(np.float64)
    wd, K = world[0].astype(np.float64), K.astype(np.float64)
    unsafe = np.zeros(wd.shape[1], bool)
    for i in range(B):
        cam = w2c[i] @ wd
        cam[1], cam[2] = -cam[1], -cam[2]
        zc = cam[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            pix = K @ (cam[:3] / zc)
            ux, uy = pix[0] - 0.5, pix[1] - 0.5                          # grid_sample's unnormalised coordinate, align_corners=False
            for u in (ux, uy):
                unsafe |= (np.abs(u - np.floor(u) - 0.5) < 1e-4) | ~np.isfinite(u)
            fx, fy = np.rint(ux), np.rint(uy)
        unsafe |= np.abs(zc) < 1e-6
        inb = (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
        ix, iy = np.where(inb, fx, 0).astype(np.int64), np.where(inb, fy, 0).astype(np.int64)
        sd = np.where(inb, depth[i, 0][iy, ix].astype(np.float64), 0.0)
        dist = sd - zc
        unsafe |= inb & (sd > 0) & (np.abs(dist + truncation) < 1e-5 * np.maximum(1.0, np.abs(zc)))
        tsdf = np.clip(dist / truncation, -1.0, 1.0)
        valid = (zc > 0) & (sd > 0) & (dist > -truncation)
        old_w = weights[valid]
        total = old_w + 1.0
        values[valid] = (values[valid] * old_w + tsdf[valid]) / total
        if color is not None:
            sc = np.where(inb[None], color[i][:, iy, ix].astype(np.float64), 0.0)
            colors[valid] = (colors[valid] * old_w[:, None] + sc[:, valid].T) / total[:, None]
        weights[valid] = total
    return unsafe


@functools.lru_cache(maxsize=None)
def tsdf_expected(seed, B, second_has_colour):
    """the scene, the float32 oracle's state after each of the two calls, the float64 form's, and the safe voxels"""
    sc = tsdf_scene(seed, B)
    o = [sc[k].copy() for k in ("values", "weights", "colors")]
    t = [sc[k].astype(np.float64) for k in ("values", "weights", "colors")]
    unsafe = np.zeros(TSDF_N, bool)
    states32, states64 = [], []
    for call in range(2):
        sl = slice(call * B, (call + 1) * B)
        col = sc["color"][sl] if (call == 0 or second_has_colour) else None
        otsdf.integrate(sc["world"], sc["c2w"][sl], sc["K"], sc["depth"][sl], col, sc["truncation"], *o)
        unsafe |= tsdf_integrate64(sc["world"], sc["c2w"][sl], sc["K"], sc["depth"][sl], col, sc["truncation"], *t)
        states32.append([a.copy() for a in o])
        states64.append([a.copy() for a in t])
    return sc, states32, states64, ~unsafe


# ================================================================== depth warp
def scatter_inputs(H, W, seed, hot=12):
    """pts [H W, 2] (u, v), mask [H W] uint8, z [H W]: hand-made inputs of ucn_warp_scatter_depth.  More than a third of the
    sources land on `hot` shared targets (dozens to thousands of writers each), the rest anywhere in the frame, u up to W - 0.5
    exclusive; unmasked sources carry coordinates that must never be read (NaN, far outside the frame)."""
    g = np.random.default_rng(seed)
    n = H * W
    u = g.uniform(0, W - 0.5, size=n)
    v = g.uniform(0, H - 0.5, size=n)
    hot_u, hot_v = g.integers(0, W, size=hot), g.integers(0, H, size=hot)
    sel = g.random(n) < 0.4
    which = g.integers(0, hot, size=n)
    u[sel] = (hot_u[which] + g.uniform(0, 0.999, size=n) * np.where(hot_u[which] == W - 1, 0.49, 1.0))[sel]
    v[sel] = (hot_v[which] + g.uniform(0, 0.999, size=n) * np.where(hot_v[which] == H - 1, 0.49, 1.0))[sel]
    u[5::97], v[5::89] = 0.0, 0.0                                          # exactly on the first column / row
    u[7::101] = g.uniform(W - 1 + 1e-3, W - 0.5 - 1e-3, size=len(u[7::101]))    # (W - 1, W - 0.5): still column W - 1
    v[9::103] = g.uniform(H - 1 + 1e-3, H - 0.5 - 1e-3, size=len(v[9::103]))
    pts = np.stack([u, v], 1).astype(F32)
    assert (pts[:, 0] < W).all() and (pts[:, 1] < H).all() and (pts >= 0).all()
    mask = ((np.arange(n) % 2 == 0) ^ (g.random(n) < 0.25)).astype(np.uint8)      # interleaved, not periodic
    mask[-1] = 1                                                           # the last thread of the ragged last block writes
    off = mask == 0
    junk = np.stack([g.choice([np.nan, -5.0, 1e9, -1e30], size=n), g.choice([np.nan, 4e9, -0.7, 1e30], size=n)], 1).astype(F32)
    bad = off & (np.arange(n) % 3 == 0)
    pts[bad] = junk[bad]
    z = (g.normal(size=n) * 3).astype(F32)                                 # negative values too
    z[11::107] = -0.0
    return pts, mask, z


def scatter_expected(pts, mask, z, H, W):
    """train_utils.py:93-96: out[int(v), int(u)] = z for the masked sources in row-major order, the last writer winning"""
    out = np.zeros((H, W), F32)
    writers = np.zeros((H, W), np.int64)
    for i in np.nonzero(mask)[0]:
        y, x = int(pts[i, 1]), int(pts[i, 0])
        out[y, x] = z[i]
        writers[y, x] += 1
    return out, writers


def warp_scene(seed=5):
    """a 37 x 53 frame, depth 2..6 with ~25 % holes (zero and negative), a source camera turned and moved so that part of the
    frame leaves it; every projected depth stays above 1, so the pixel error is a rounding error and not a pole"""
    g = np.random.default_rng(seed)
    H, W = 37, 53
    K = np.array([[48.0, 0.0, 26.3], [0.0, 47.0, 18.6], [0.0, 0.0, 1.0]], F32)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (4.0 + 1.5 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 0.5 * g.random((H, W))).astype(F32)
    hole = g.random((H, W))
    depth[hole < 0.2] = 0.0
    depth[hole < 0.05] = -1.0
    a = np.radians(9.0)
    rel = np.eye(4)
    rel[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ _rot(g, 0.05)
    rel[:3, 3] = [0.35, -0.2, 0.15]
    return depth, rel.astype(F32), K


def img_warping64(depth, rel, K):
    """train_utils.py:19-55 in float64 on the float32 inputs: (uv [H, W, 2], mask [H, W], z [H, W])"""
    d, rel, K = depth.astype(np.float64), rel.astype(np.float64), K.astype(np.float64)
    H, W = d.shape
    cols, rows = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    P = np.stack([(cols - K[0, 2]) / K[0, 0] * d, (rows - K[1, 2]) / K[1, 1] * d, d], 0).reshape(3, -1)
    Q = rel[:3, :3] @ P + rel[:3, 3:4]
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = (K @ (Q / Q[2:3]))[:2].T.reshape(H, W, 2)
        inside = (uv[..., 0] >= 0) & (uv[..., 1] >= 0) & (uv[..., 0] < W - 0.5) & (uv[..., 1] < H - 0.5)
    return uv, (d > 0) & inside, Q[2].reshape(H, W)


def warp_edge(uv, H, W, margin=1e-2):
    """pixels whose float64 projection is within `margin` px of a mask boundary (tests/test_warp.py's rule)"""
    return np.minimum.reduce([np.abs(uv[..., 0]), np.abs(uv[..., 0] - (W - 0.5)), np.abs(uv[..., 1]), np.abs(uv[..., 1] - (H - 0.5))]) < margin


# ================================================================== image metrics
# interior (H - 6)(W - 6) of 256 and 272 / 257-like block ends of k_metrics_ssim, strips, H W = 256 k and 256 k + 1 for k_metrics_quant
METRIC_SIZES = ((22, 22), (22, 23), (7, 300), (300, 7), (7, 7), (16, 16), (16, 17), (16, 33), (19, 27), (7, 263), (263, 7))
METRIC_KINDS = ("steps", "overshoot", "identical")


def metric_images(h, w, kind, seed=0):
    """steps: both images made of exact k / 255 values, 0 and 1.0 included, differing in places;  overshoot: pred leaves [0, 1] on
    both sides, gt on k / 255 steps with whole rows of 1.0;  identical: pred == gt (steps)"""
    g = np.random.default_rng(seed + 1000 * h + w)
    steps = (np.arange(256, dtype=F32) / F32(255)).astype(F32)
    gt = steps[g.integers(0, 256, size=(h, w, 3))]
    gt[0], gt[-1, :, 1] = F32(1.0), F32(0.0)
    if kind == "identical":
        return gt.copy(), gt
    if kind == "steps":
        pred = steps[np.clip(g.integers(-6, 7, size=gt.shape) + np.rint(gt * 255).astype(np.int64), 0, 255)]
        pred[1] = F32(1.0)
        pred[:, 0] = F32(0.0)
        return pred.astype(F32), gt
    pred = (gt + 0.3 * g.normal(size=gt.shape)).astype(F32)
    pred[2] = F32(1.5)
    pred[:, 1] = F32(-0.25)
    pred[:, 3] = np.nextafter(gt[:, 3], F32(0))                            # one float32 below a step: the product decides k or k - 1
    pred[:, 4] = np.nextafter(gt[:, 4], F32(2))
    assert pred.min() < 0 and pred.max() > 1
    return pred, gt


def metrics_expected(pred, gt):
    """(psnr, ssim, mse on the uint8 scale) of oracle/metrics.py"""
    from oracle import metrics as om
    p, g = om.quantise(pred, gt)
    mse = float(np.mean((p.astype(np.float64) - g.astype(np.float64)) ** 2))
    return om.psnr(p, g), om.ssim(om.to_gray(p), om.to_gray(g)), mse


# ================================================================== colour-correction head
# (M, K, Nout): the layers of extrinsic_optimizer.py's 4 -> 256 -> 256 -> 256 -> 12 MLP at 1, 5 and 210 cameras, and M Nout = 255, 256, 257
DENSE_SHAPES = tuple((M, K, N) for M in (1, 5, 210) for K, N in ((4, 256), (256, 256), (256, 12))) + (
    (5, 256, 51), (1, 4, 256), (257, 4, 1), (1, 256, 257), (3, 7, 85))


def dense_inputs(M, K, Nout, seed=0):
    g = np.random.default_rng(seed + 7 * M + 11 * K + 13 * Nout)
    x = g.normal(size=(M, K)).astype(F32)
    x[g.random((M, K)) < 0.3] = 0.0                                        # a relu'd layer's input
    w = (g.normal(size=(Nout, K)) / np.sqrt(K)).astype(F32)
    b = (0.1 * g.normal(size=Nout)).astype(F32)
    return x, w, b


def dense64(x, w, b, relu):
    """(y, bar): y = act(x w^T + b) in float64; the kernel is a k-sequential fmaf chain of length K plus the bias add, K + 1
    roundings, so |err| <= (K + 1) 2^-24 (sum |x| |w| + |b|) per element (relu is 1-Lipschitz)"""
    x, w = x.astype(np.float64), w.astype(np.float64)
    y, mag = x @ w.T, np.abs(x) @ np.abs(w).T
    if b is not None:
        y, mag = y + b.astype(np.float64), mag + np.abs(b.astype(np.float64))
    return (np.maximum(y, 0.0) if relu else y), (x.shape[1] + 1) * U32 * mag


AFFINE_ROWS = 7


def affine_inputs(N, S, seed=0):
    """rgb [N,3], A [7,12], rows [N] int64 (every row used once N >= 7, scrambled), weights [N,S] (a third of the rows sum to more
    than 1), sky [N,3], A_sky [7,12]"""
    g = np.random.default_rng(seed + 17 * N + S)
    rgb, sky = g.random((N, 3)).astype(F32), g.random((N, 3)).astype(F32)
    A = (np.tile(np.eye(3, 4).reshape(1, 12), (AFFINE_ROWS, 1)) + 0.2 * g.normal(size=(AFFINE_ROWS, 12))).astype(F32)
    A_sky = (np.tile(np.eye(3, 4).reshape(1, 12), (AFFINE_ROWS, 1)) + 0.2 * g.normal(size=(AFFINE_ROWS, 12))).astype(F32)
    rows = g.permutation(np.arange(N) % AFFINE_ROWS).astype(np.int64)
    wts = g.random((N, S))
    wts = wts / wts.sum(1, keepdims=True) * g.uniform(0.0, 1.0, size=(N, 1))
    wts[::3] *= 1.7 / np.maximum(wts[::3].sum(1, keepdims=True), 1e-3)      # 1 - acc = -0.7: the kernel does not clamp
    return rgb, A, rows, wts.astype(F32), sky, A_sky


def affine64(rgb, A, rows, wts=None, sky=None, A_sky=None):
    """(out, bar): rgb' = A rgb + t (+ (1 - sum w)(B sky + t_sky)) in float64, rows = None -> row 0;
    bar = gamma (sum |A||rgb| + |t| + (1 + sum |w|)(sum |B||sky| + |t_sky|)), gamma = (S + 8) 2^-24"""
    d = lambda a: a.astype(np.float64)
    rows = np.zeros(len(rgb), np.int64) if rows is None else rows

    def dot4(M, v, absolute):
        M = d(M)[rows].reshape(-1, 3, 4)
        v = d(v)
        if absolute:
            M, v = np.abs(M), np.abs(v)
        return (M[:, :, :3] * v[:, None, :]).sum(-1) + M[:, :, 3]
    out, mag, S = dot4(A, rgb, False), dot4(A, rgb, True), 0
    if sky is not None:
        S = wts.shape[1]
        acc, absw = d(wts).sum(1, keepdims=True), np.abs(d(wts)).sum(1, keepdims=True)
        out = out + (1.0 - acc) * dot4(A_sky, sky, False)
        mag = mag + (1.0 + absw) * dot4(A_sky, sky, True)
    return out, (S + 8) * U32 * mag
