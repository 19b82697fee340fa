"""Where the NeRF-level gather's time goes at the benchmark's own pass shape: k_march_features at 10,240 rays x 128 samples,
rays fastest, the rays of bench.py's frame in 8 x 8 tile order (one pass from the middle of the frame).

Variants, each an explicit level range of the benchmark grid handed over as a field of its own (no switch in the library):
  whole        levels 0-15, levels_per_block = 0 (the product's launch)
  coarse only  levels 0-7 (resolution <= 2048) as one field: one group of eight
  fine only    levels 8-15 as one field: eight groups of one
  per level    levels 0-15, levels_per_block = 1 (sixteen groups, the geometry derived sixteen times)
Medians over --launches launches (HIP events around each), with minimum and maximum.
UCN_LIB_PATH=<libucnerf_march.so> measures another build of the library (ucnerf_amd/_lib.py)."""
import argparse, ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, bench
from ucnerf_amd import _lib
from ucnerf_amd.internal import models

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=10240)
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--incoherent", action="store_true", help="random rays of the frame, layout 1 | UCN_RAYS_INCOHERENT: the training forward")
ap.add_argument("--half", action="store_true", help="half tables (UCN_TABLE_F16), as under autocast")
args = ap.parse_args()

lib = _lib.load()
dev = torch.device("cuda", 0)
model, cfg, sd = bench.build_model(dev)
batch = bench.frame_rays(dev)
H, W = batch["origins"].shape[:2]
flat = {k: v.reshape(H * W, -1) for k, v in batch.items()}
n, S = args.rays, bench.S_NERF
if args.incoherent:
    pick = torch.randperm(H * W, generator=torch.Generator().manual_seed(3))[:n].to(dev)
else:
    perm, _ = models._tile_order(H, W, 8, dev)
    r0 = (H * W // 2) // n * n                   # a pass from the middle of the frame
    pick = perm[r0:r0 + n]
flat = {k: v.index_select(0, pick).contiguous() for k, v in flat.items()}
flat["rand_vec"] = torch.randn(n, 6, generator=torch.Generator().manual_seed(1)).to(dev)
with torch.no_grad():
    _, hist = model(False, flat, 1.0, True)
sdist = hist[-1]["sdist"].contiguous()
enc = model.nerf_mlp.encoder
basis = torch.empty(n, 6, device=dev)
_lib.check(lib.ucn_cone_basis(flat["cam_dirs"].data_ptr(), flat["rand_vec"][:, 3:6].contiguous().data_ptr(), n, basis.data_ptr(), _lib.stream()))
near, far = flat["near"].reshape(-1).contiguous(), flat["far"].reshape(-1).contiguous()
rad = flat["radii"].reshape(-1).contiguous()
L, C = enc.num_levels, enc.level_dim
feat = torch.empty(L * n * S * C, device=dev)
layout = ((1 | _lib.RAYS_INCOHERENT) if args.incoherent else 2) | (_lib.TABLE_F16 if args.half else 0)
table = enc.embeddings.detach().to(torch.half) if args.half else enc.embeddings.detach()
keep = []


def sub_field(l0, l1):
    """levels [l0, l1) of the benchmark grid as a field of its own"""
    d = _lib.UcnField()
    off = (enc._offsets_np[l0:l1 + 1] - enc._offsets_np[l0]).astype(np.int32)
    gs = np.ascontiguousarray(enc._sizes_np[l0:l1])
    keep.extend([off, gs])
    d.embeddings = table.data_ptr() + int(enc._offsets_np[l0]) * C * table.element_size()
    d.offsets_host, d.grid_sizes_host = off.ctypes.data, gs.ctypes.data
    d.num_levels, d.level_dim = l1 - l0, C
    d.base_resolution = int(round(enc.base_resolution * enc.per_level_scale ** l0))
    d.log2_per_level_scale = float(np.log2(enc.per_level_scale))
    return d


def time_launch(d, lpb):
    a = (ctypes.byref(d), sdist.data_ptr(), near.data_ptr(), far.data_ptr(), flat["origins"].data_ptr(), flat["directions"].data_ptr(),
         basis.data_ptr(), rad.data_ptr(), None, None, float(model.std_scale), n, S, lpb, layout, feat.data_ptr(), None, None, _lib.stream())
    for _ in range(3):
        _lib.check(lib.ucn_march_features(*a))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches)]
    for e0, e1 in ev:
        e0.record()
        _lib.check(lib.ucn_march_features(*a))
        e1.record()
    torch.cuda.synchronize()
    t = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
    return float(np.median(t)), float(t.min()), float(t.max())


n_coarse = int(sum(1 for l in range(L) if int(round(enc.base_resolution * enc.per_level_scale ** l)) <= 2048))
rows = [("whole (levels_per_block 0)", sub_field(0, L), 0),
        (f"coarse only (levels 0-{n_coarse - 1})", sub_field(0, n_coarse), 0),
        (f"fine only (levels {n_coarse}-{L - 1})", sub_field(n_coarse, L), 0),
        ("per level (levels_per_block 1)", sub_field(0, L), 1)]
print(f"k_march_features, {n} rays x {S} samples, layout {layout:#x}, {args.launches} launches each, ms: median [min, max]   library {_lib.LIB_PATH}")
res = {}
for rep in range(2):                             # twice over, alternating: drift between the variants would show
    for name, d, lpb in rows:
        res.setdefault(name, []).append(time_launch(d, lpb))
for name, _, _ in rows:
    print(f"  {name:34s} " + "   ".join(f"{m:7.4f} [{lo:7.4f}, {hi:7.4f}]" for m, lo, hi in res[name]))
w, c, f = (np.mean([m for m, _, _ in res[rows[i][0]]]) for i in range(3))
passes = H * W / n
print(f"  whole - fine only = {w - f:7.4f} ms per pass = {100 * (w - f) / w:5.1f} % of the launch, x {passes:.0f} passes = {(w - f) * passes:6.2f} ms per frame"
      f"   (coarse alone {c:7.4f}; coarse alone + fine only = {c + f:7.4f})")
