#!/usr/bin/env python
"""Time the device batch assembler (ucnerf_amd/internal/datasets.py) against the numpy restatement of the reference's
`_make_ray_batch` on the same host.  Recorded, not gated.

    python tools/time_train_batch.py --out profiles/train_batch/timing.txt

Two batch shapes, 8192 rays and the reference's literal 15 000, all-images batching, each without and with the virtual-pose
branch on a 1280 x 1920 depth plane.  Device figures are HIP-event times (warm-up, then the median of `--reps` calls, each
call between two events, with min and max as the spread); `next_train` includes its draws, and with virtual poses the warp
of the depth map and the one sync per attempt.  The host column is tests/train_batch_ref.py (float64 numpy, single thread of
the DataLoader worker it stands in for) on the indices the device drew, `time.perf_counter` median; in the virtual rows it
includes oracle/warp.py's numpy warp of the same depth map, the reference's per-batch CPU work at datasets.py:527.  The
reference itself is not timed: it is not on the GPU machine.  A run without a GPU fails; it does not fall back.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

N_REAL, CAM_NUM, H, W = 8, 1, 1280, 1920
FLIP = np.diag([1., -1., -1., 1.])


def scene(rng):
    K = np.array([[2055.556149, 0.0, 939.657470], [0.0, 2055.556149, 641.072182], [0.0, 0.0, 1.0]])
    real = np.stack([np.eye(4) for _ in range(N_REAL)])
    real[:, 0, 3] = 0.05 * np.arange(N_REAL)
    virtual = np.repeat(real, 9, axis=0)
    virtual[:, :3, 3] += rng.uniform(-0.05, 0.05, size=(N_REAL * 9, 3))
    images = torch.rand(N_REAL, H, W, 3, generator=torch.Generator().manual_seed(1))
    depth = torch.rand(N_REAL, H, W, generator=torch.Generator().manual_seed(2)) * 3.0 + 1.0
    sky = (torch.rand(N_REAL, H, W, generator=torch.Generator().manual_seed(3)) < 0.3).float()
    return dict(images=images.numpy(), disp_images=depth.numpy(), sky_segments=sky.numpy(), K=K, real=real @ FLIP,
                virtual=virtual @ FLIP, pixtocams=np.repeat(np.linalg.inv(K)[None], N_REAL * 10, axis=0))


def device_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def host_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_batch", "timing.txt"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_train_batch: needs a GPU")
    import train_batch_ref as R
    from oracle import warp as oracle_warp
    from ucnerf_amd.internal import datasets as D

    sc = scene(np.random.default_rng(5))
    c2w = np.concatenate([sc["real"], sc["virtual"]])
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {N_REAL} images of {H} x {W}, planes rgb + disps + "
             f"sky_segs; device = HIP events, median [min .. max] of {args.reps} calls after {args.warmup}; host = numpy restatement "
             f"(tests/train_batch_ref.py), perf_counter median of {args.host_reps}",
             f"{'case':34s} {'next_train ms':>26s} {'make_ray_batch ms':>26s} {'host numpy ms':>26s} {'host / make_ray_batch':>22s} "
             f"{'host / next_train':>18s}"]
    for rays in (8192, 15000):
        for virtual in (False, True):
            ds = D.DeviceDataset(sc["images"], c2w if virtual else sc["real"], sc["pixtocams"][:len(c2w) if virtual else N_REAL],
                                 0.25, 8.0, disp_images=sc["disp_images"], sky_segments=sc["sky_segments"],
                                 virtual_poses=sc["virtual"] if virtual else None, cam_num=CAM_NUM, compute_disp_metrics=True,
                                 load_sky_segments=True, batch_size=rays, seed=9)
            idx = ds.sample_train_indices(torch.Generator().manual_seed(3))
            t_next = device_ms(lambda: ds.next_train(), args.reps, args.warmup)
            t_make = device_ms(lambda: ds.make_ray_batch(**idx, validate=False), args.reps, args.warmup)
            data = dict(images=sc["images"], disp_images=sc["disp_images"], sky_segments=sc["sky_segments"], camtoworlds=c2w[:, :3],
                        pixtocams=sc["pixtocams"], near=0.25, far=8.0, virtual_poses=virtual, load_disps=True, load_segs=True)
            host_idx = {k: v.cpu().numpy().astype(np.int64) for k, v in idx.items()}
            got, want = ds.make_ray_batch(**idx), R.make_ray_batch(data, **host_idx)
            for k, w in want.items():                      # what is timed computes the same thing
                assert w is None or torch.equal(got[k].cpu(), torch.from_numpy(w)), k

            def host():
                if virtual:
                    ref, src = int(host_idx["cam_idx_with_ref"][-1, 0, 0]), int(host_idx["cam_idx_with_src"][-1, 0, 0]) - N_REAL
                    oracle_warp.img_warping(sc["real"][ref] @ FLIP, sc["virtual"][src] @ FLIP, sc["disp_images"][ref], sc["K"])
                R.make_ray_batch(data, **host_idx)
            t_host = host_ms(host, args.host_reps)
            fmt = lambda t: f"{t[0]:9.3f} [{t[1]:.3f} .. {t[2]:.3f}]"
            n = idx["pixel_x_int_with_src"].shape[0] if virtual else rays
            lines.append(f"{f'{rays} rays' + (f' + virtual ({n} in all)' if virtual else ''):34s} {fmt(t_next):>26s} {fmt(t_make):>26s} "
                         f"{fmt(t_host):>26s} {t_host[0] / t_make[0]:22.1f} {t_host[0] / t_next[0]:18.1f}")
            del ds
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
