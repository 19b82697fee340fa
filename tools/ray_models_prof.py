"""Run the three ray-generation kernels on one frame size each, for `rocprofv3 --kernel-trace --stats` (no counters in that run):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o rays -- python tools/ray_models_prof.py [--reps N]

  k_generate_rays<0>   perspective, 8000 x 900 (the parent commit's code, at the panorama frame's ray count)
  k_generate_rays<1>   panorama ('panoroma'), 8000 x 900: the nuScenes render path's frame (datasets.py:872-878)
  k_spherical_rays     spherical, 900 x 8000

Every launch writes all ten outputs of a frame batch: 76 B per ray (origins, directions, viewdirs, cam_dirs 12 B each, imageplane
8 B, radii and the near / far / lossmult / cam_idx columns 4 B each) and reads two small matrices.  Prints that byte count; the
kernel times are the profiler's."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucnerf_amd.internal import camera_utils as cu  # noqa: E402

BYTES_PER_RAY = 4 * (3 + 3 + 3 + 3 + 2 + 1 + 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    W, H = 8000, 900
    K = np.array([[1266.417203, 0.0, 4000.2], [0.0, 1266.417203, 449.7], [0.0, 0.0, 1.0]])
    g = torch.Generator().manual_seed(0)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    pose = torch.cat([q, torch.randn(3, 1, generator=g, dtype=torch.float64)], dim=1)
    cams = (torch.from_numpy(np.linalg.inv(K)), pose, None, None)
    for _ in range(a.reps):                      # alternating, so that the three share whatever the clock does
        b = cu.generate_ray_batch(cams, 0, W, H, 0.1, 100.0)
        b = cu.generate_ray_batch(cams, 0, W, H, 0.1, 100.0, camtype=cu.PANORAMA)
        b = cu.cast_spherical_rays(pose, H, W, 0.1, 100.0)
        del b
    torch.cuda.synchronize()
    print(f"{a.reps} launches each of {W * H} rays, {BYTES_PER_RAY} B written per ray = {W * H * BYTES_PER_RAY / 1e6:.1f} MB per launch")


if __name__ == "__main__":
    main()
