"""ucn_march_features in auto mode (levels_per_block = 0) pairs every fine level (resolution > 2048) with coarse levels in one
thread.  Every level's accumulation is independent of every other level's, so features, coordinates and t-means must be
bit-identical to the same library with levels_per_block = 1 (every level a group of its own: the contiguous code path).
The grouping rule itself is checked on the host (ucn_level_groups_probe), without a GPU."""
import ctypes
import functools

import numpy as np
import pytest
import torch

CGRP = 8          # a group holds at most this many levels (make_groups, march_features.hip)
CRES = 2048       # a level is coarse up to this resolution

# name -> GridEncoder arguments
GRIDS = {
    "config_b": dict(num_levels=16, level_dim=2, base_resolution=16, desired_resolution=524288, log2_hashmap_size=19),
    "proposal": dict(num_levels=6, level_dim=2, base_resolution=16, desired_resolution=512, log2_hashmap_size=19),       # no fine level
    "waymo_gin": dict(num_levels=10, level_dim=4, base_resolution=16, desired_resolution=8192, log2_hashmap_size=21),    # 8 coarse + 2 fine
    "all_fine": dict(num_levels=3, level_dim=2, base_resolution=4096, desired_resolution=16384, log2_hashmap_size=14),
    "one_coarse": dict(num_levels=4, level_dim=2, base_resolution=2048, desired_resolution=16384, log2_hashmap_size=14),
}


@functools.lru_cache(maxsize=None)
def _encoder(name):
    from ucnerf_amd.gridencoder.grid import GridEncoder
    return GridEncoder(input_dim=3, gridtype="hash", align_corners=False, **GRIDS[name])


def _field(enc, embeddings_ptr):
    from ucnerf_amd import _lib
    d = _lib.UcnField()
    d.embeddings = embeddings_ptr
    d.offsets_host, d.grid_sizes_host = enc._offsets_np.ctypes.data, enc._sizes_np.ctypes.data
    d.num_levels, d.level_dim, d.base_resolution = enc.num_levels, enc.level_dim, enc.base_resolution
    d.log2_per_level_scale = float(np.log2(enc.per_level_scale))
    return d


def _groups(enc, levels_per_block, layout=2):
    from ucnerf_amd import _lib
    lib = _lib.load()
    L = enc.num_levels
    levels, first = np.full(L, 255, dtype=np.uint32), np.zeros(L + 1, dtype=np.uint32)
    d = _field(enc, 8)                                     # the probe never touches the table
    n = lib.ucn_level_groups_probe(ctypes.byref(d), levels_per_block, layout, levels.ctypes.data, first.ctypes.data)
    assert n >= 1, lib.ucn_last_error()
    assert first[0] == 0 and first[n] == L
    return [[int(v) for v in levels[first[g]:first[g + 1]]] for g in range(n)]


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_grouping_rule(name):
    enc = _encoder(name)
    L = enc.num_levels
    res = [int(s) - 1 for s in enc._sizes_np]                                  # side = resolution + 1
    coarse = [l for l in range(L) if res[l] <= CRES]
    fine = [l for l in range(L) if res[l] > CRES]
    auto = _groups(enc, 0)
    assert len(auto) >= 1 and len(auto[0]) >= 1                               # group 0 exists: it writes coord_out / tmean_out
    assert sorted(l for g in auto for l in g) == list(range(L))               # every level in exactly one group
    assert all(1 <= len(g) <= CGRP for g in auto)
    if coarse and fine:
        assert all(sum(l in fine for l in g) <= 1 for g in auto)              # a fine level never shares its L2 slice with another
        if len(coarse) <= len(fine) * (CGRP - 1):
            assert len(auto) == len(fine)                                      # no coarse-only group remains
            share = [sum(l in coarse for l in g) for g in auto]
            assert max(share) - min(share) <= 1
    elif fine:
        assert auto == [[l] for l in range(L)]
    else:
        assert auto == [list(range(l, min(l + CGRP, L))) for l in range(0, L, CGRP)]
    from ucnerf_amd import _lib
    random_rays = _groups(enc, 0, 1 | _lib.RAYS_INCOHERENT)                   # training rays: coarse levels together, fine alone
    assert random_rays == [coarse[l:l + CGRP] for l in range(0, len(coarse), CGRP)] + [[l] for l in fine]
    for k in (1, 2, 3, 5, 8, L, L + 3):                                        # an explicit count keeps its contiguous meaning
        assert _groups(enc, k) == [list(range(l, min(l + k, L))) for l in range(0, L, k)], k


def test_config_b_pairs_one_coarse_level_with_each_fine_level():
    auto = _groups(_encoder("config_b"), 0)
    assert len(auto) == 8 and all(len(g) == 2 for g in auto)
    assert sorted(min(g) for g in auto) == list(range(8)) and sorted(max(g) for g in auto) == list(range(8, 16))


# ---- GPU: auto mode against levels_per_block = 1, bit for bit

@functools.lru_cache(maxsize=None)
def _rays(n, S):
    """n Waymo-like rays with sorted fenceposts, cone bases and metric distances, on the device"""
    from oracle import raymarch as rm
    from ucnerf_amd import _lib
    lib = _lib.load()
    r = {k: v.cuda() for k, v in rm.synthetic_rays(n, seed=31).items()}
    g = torch.Generator(device="cuda").manual_seed(32)
    sdist = torch.sort(torch.rand(n, S + 1, device="cuda", generator=g), dim=-1).values.contiguous()
    rand = torch.randn(n, 3, device="cuda", generator=g)
    basis = torch.empty(n, 6, device="cuda")
    _lib.check(lib.ucn_cone_basis(r["cam_dirs"].data_ptr(), rand.data_ptr(), n, basis.data_ptr(), _lib.stream()))
    near, far, rad = (r[k].reshape(-1).contiguous() for k in ("near", "far", "radii"))
    tdist = (0.05 + 7.9 * sdist).contiguous()
    torch.cuda.synchronize()
    return dict(sdist=sdist, tdist=tdist, near=near, far=far, origins=r["origins"].contiguous(), directions=r["directions"].contiguous(),
                basis=basis, radii=rad)


@functools.lru_cache(maxsize=None)
def _table(name, half):
    enc = _encoder(name)
    g = torch.Generator(device="cuda").manual_seed(33)
    t = torch.rand(enc.embeddings.shape, device="cuda", generator=g) * 2 - 1
    return t.to(torch.half) if half else t


def _run(name, n, S, layout, levels_per_block, half=False, tdist=False, flags=0):
    from ucnerf_amd import _lib
    lib = _lib.load()
    enc, r = _encoder(name), _rays(n, S)
    L, C = enc.num_levels, enc.level_dim
    d = _field(enc, _table(name, half).data_ptr())
    feat = torch.full((L * n * S * C,), float("nan"), device="cuda")
    coord = torch.full((n, S, 3), float("nan"), device="cuda")
    tmean = torch.full((n, S), float("nan"), device="cuda")
    lay = layout | flags | (_lib.TABLE_F16 if half else 0)
    tail = (None, None, 0.5, n, S, levels_per_block, lay, feat.data_ptr(), coord.data_ptr(), tmean.data_ptr(), _lib.stream())
    if tdist:
        _lib.check(lib.ucn_march_features_tdist(ctypes.byref(d), r["tdist"].data_ptr(), r["origins"].data_ptr(), r["directions"].data_ptr(),
                                                r["basis"].data_ptr(), r["radii"].data_ptr(), *tail))
    else:
        _lib.check(lib.ucn_march_features(ctypes.byref(d), r["sdist"].data_ptr(), r["near"].data_ptr(), r["far"].data_ptr(),
                                          r["origins"].data_ptr(), r["directions"].data_ptr(), r["basis"].data_ptr(), r["radii"].data_ptr(), *tail))
    torch.cuda.synchronize()
    return feat, coord, tmean


def _same(name, n, S, layout, **kw):
    got = _run(name, n, S, layout, 0, **kw)
    want = _run(name, n, S, layout, 1, **kw)
    for a, b, what in zip(got, want, ("features", "coord", "tmean")):
        assert not torch.isnan(b).any(), what                                 # every element written
        assert torch.equal(a, b), (name, n, S, layout, kw, what)
    assert float(want[0].abs().max()) > 0


# 96 x 32: whole waves only; 67 x 33 = 34 waves + 35 lanes: the partial last wave takes the per-lane route, the rest lane pairs
SHAPES = [(96, 32), (67, 33)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,S", SHAPES)
@pytest.mark.parametrize("layout", [0, 2])
@pytest.mark.parametrize("name,half", [("config_b", False), ("config_b", True), ("proposal", False), ("waymo_gin", False),
                                       ("all_fine", False), ("one_coarse", False)])
def test_auto_groups_are_bit_identical_to_one_level_per_group(name, half, layout, n, S):
    _same(name, n, S, layout, half=half)


@pytest.mark.gpu
@pytest.mark.parametrize("n,S", SHAPES)
@pytest.mark.parametrize("layout", [0, 2])
def test_tdist_entry_point(layout, n, S):
    _same("config_b", n, S, layout, tdist=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n,S", SHAPES)
@pytest.mark.parametrize("layout", [0, 2])
def test_coresident_launch_shape(layout, n, S):
    from ucnerf_amd import _lib
    _same("config_b", n, S, layout, flags=_lib.LAUNCH_CORESIDENT)


@pytest.mark.gpu
@pytest.mark.parametrize("n,S", SHAPES)
@pytest.mark.parametrize("name,half", [("config_b", False), ("config_b", True), ("waymo_gin", False)])
@pytest.mark.parametrize("incoherent", [False, True])
def test_sample_major_layout_of_the_training_forward(incoherent, name, half, n, S):
    """layout 1 ([B][L*C]) is what the training forward asks for, with UCN_RAYS_INCOHERENT (which keeps the coarse levels in a group
    of their own); without the flag the groups are paired"""
    from ucnerf_amd import _lib
    _same(name, n, S, 1, half=half, flags=_lib.RAYS_INCOHERENT if incoherent else 0)
