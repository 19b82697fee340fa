"""Warped ray distances: what Model.raydist_fn = 'power_transformation' costs (DESIGN.md "Ray-distance curves").

    python tools/raydist_bench.py [--steps K] [--frames F] [--out FILE]

On bench.py's config-B model (NeRF grid L16 / C2 / T = 2^19, 64 + 128 samples), the same field weights with raydist_fn None
and 'power_transformation' (lam -1.5):
  * the 1280 x 1920 frame through render_image (configs[1]: fp32-class);
  * the training step at 8192 rays (bench.train_step_ms: forward, losses, backward, Adam), bf16 autocast;
  * ucn_s_to_t alone, timed with HIP events over 100 launches, at the frame's and the step's fencepost counts.
The warped march also places its samples elsewhere along the rays (that is the point of the curve), so the whole-frame and
whole-step figures move for that reason as well as for the added launch; the kernel's own time is the direct cost.
One JSON line per figure, printed (and appended to --out).  The recorded run with its summary: profiles/raydist/raydist_bench.txt.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402
from ucnerf_amd import _lib  # noqa: E402
from ucnerf_amd.internal import models  # noqa: E402


def build(device, fn):
    base = bench.build_model(device)[0]
    if fn is None:
        return base
    with models.bindings(Model=dict(raydist_fn=fn)):
        model = bench.build_model(device)[0]
    model.load_state_dict(base.state_dict())
    del base
    return model


def frame_ms(model, device, frames):
    rays = bench.frame_rays(device)
    cfg = types.SimpleNamespace(render_ray_tile=8, vis_num_rays=16)
    times = []
    for it in range(frames + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = models.render_image(model, None, rays, False, 1.0, cfg, verbose=False)
        torch.cuda.synchronize()
        if it:
            times.append((time.perf_counter() - t0) * 1e3)
    assert torch.isfinite(out["rgb"]).all()
    model.eval()
    return float(np.median(times)), [round(t, 2) for t in times]


def s_to_t_us(N, S1, device, reps=100):
    lib = _lib.load()
    g = torch.Generator(device=device).manual_seed(0)
    sdist = torch.sort(torch.rand(N, S1, device=device, generator=g), dim=-1).values
    near, far = torch.zeros(N, device=device), torch.full((N,), 8.0, device=device)
    tdist = torch.empty_like(sdist)
    st = _lib.stream()
    call = lambda: _lib.check(lib.ucn_s_to_t(sdist.data_ptr(), near.data_ptr(), far.data_ptr(), N, S1, 2, -1.5, tdist.data_ptr(), st))
    for _ in range(5):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    flat = {k: v.reshape(-1, v.shape[-1]) for k, v in bench.frame_rays(dev).items()}
    for fn in (None, "power_transformation"):
        model = build(dev, fn)
        ms, all_ms = frame_ms(model, dev, args.frames)          # frames first: the training steps below move the weights
        emit(figure="frame_1280x1920", raydist_fn=fn, autocast=False, ms=round(ms, 2), frames=all_ms, route=model.last_march_route)
        r = bench.train_step_ms(model, flat, dev, n_rays=8192, steps=args.steps, autocast=True)
        emit(figure="train_step", raydist_fn=fn, autocast=True, ms=round(r["ms"], 3), rays=8192, steps=args.steps)
        del model
        torch.cuda.empty_cache()
    frame_rays = flat["origins"].shape[0]
    for what, N, S1 in (("frame, proposal level", frame_rays, 65), ("frame, NeRF level", frame_rays, 129),
                        ("step, proposal level", 8192, 65), ("step, NeRF level", 8192, 129)):
        us = s_to_t_us(N, S1, dev)
        emit(figure="ucn_s_to_t", what=what, fenceposts=N * S1, us=round(us, 2),
             gbps=round(N * S1 * 8 / (us * 1e-6) / 1e9, 1))


if __name__ == "__main__":
    main()
