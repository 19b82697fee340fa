"""GLO appearance codes: what they cost (DESIGN.md "GLO").

    python tools/glo_bench.py [--steps K] [--frames F] [--only train|frame]

On bench.py's config-B model (NeRF grid L16 / C2 / T = 2^19, 64 + 128 samples), with and without
Model.num_glo_features = 64 (num_glo_embeddings 1000, the reference's defaults otherwise):
  * the training step at 8192 rays (bench.train_step_ms: forward with zero_glo=False, losses, backward, Adam), bf16
    autocast and fp32 (split engine).  With GLO the NeRF field takes the uncomposed route (_ColourMLPGlo) instead of the
    fused kernels (_FusedHeads / _FieldMLPComposed);
  * the 1280 x 1920 frame through render_image (zero_glo=True: the fused march on the folded colour layers), fp32-class
    and under bf16 autocast.
One JSON line per figure.  ucn_ray_film / _backward per-launch times come from a run of `--only train` under
rocprofv3 --kernel-trace --stats; `film_bytes` prints the bytes each launch moves at 8192 x 128 samples x 256.
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
from ucnerf_amd.internal import dense_f32, models  # noqa: E402


def build(device, glo):
    """bench.py's model; with glo, the same field weights (the GLO layers shift the construction-time RNG: a different field
    would resample other sample positions and change the frame time for reasons that have nothing to do with GLO)."""
    base = bench.build_model(device)[0]
    if not glo:
        return base
    with models.bindings(Model=dict(num_glo_features=64, num_glo_embeddings=1000)):
        model = bench.build_model(device)[0]
    missing, unexpected = model.load_state_dict(base.state_dict(), strict=False)
    assert not unexpected and all("glo" in k for k in missing), (missing, unexpected)
    del base
    return model


def frame_ms(model, device, frames, autocast):
    rays = bench.frame_rays(device)
    cfg = types.SimpleNamespace(render_ray_tile=8, vis_num_rays=16)
    times = []
    for it in range(frames + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            out = models.render_image(model, None, rays, False, 1.0, cfg, verbose=False)
        torch.cuda.synchronize()
        if it:
            times.append((time.perf_counter() - t0) * 1e3)
    assert torch.isfinite(out["rgb"]).all()
    model.eval()
    return float(np.median(times)), [round(t, 2) for t in times]


def film_bytes(M=8192 * 128, N=8192, W=256, elem=2):
    fwd = 2 * M * W * elem + 2 * N * W * 4                   # x read, out write; a, b read
    bwd = 3 * M * W * elem + 3 * N * W * 4                   # gy, x read, gx write; a read, ga, gb write
    return dict(M=M, W=W, elem_bytes=elem, fwd_bytes=fwd, bwd_bytes=bwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--only", choices=("train", "frame"), default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    flat = {k: v.reshape(-1, v.shape[-1]) for k, v in bench.frame_rays(dev).items()}
    for glo in (False, True):
        model = build(dev, glo)
        if args.only != "train":             # frames first: the training steps below move the weights
            for autocast in (False, True):
                ms, all_ms = frame_ms(model, dev, args.frames, autocast)
                print(json.dumps(dict(figure="frame_1280x1920", glo=glo, zero_glo=True, autocast=autocast, ms=round(ms, 2),
                                      frames=all_ms, route=model.last_march_route)), flush=True)
        if args.only != "frame":
            for autocast in (True, False):
                with_engine = dense_f32.engine()
                r = bench.train_step_ms(model, flat, dev, n_rays=8192, steps=args.steps, autocast=autocast)
                print(json.dumps(dict(figure="train_step", glo=glo, autocast=autocast, engine=None if autocast else with_engine,
                                      ms=round(r["ms"], 3), rays=8192, steps=args.steps)), flush=True)
        del model
        torch.cuda.empty_cache()
    print(json.dumps(dict(figure="film_bytes_bf16", **film_bytes())), flush=True)
    print(json.dumps(dict(figure="film_bytes_f32", **film_bytes(elem=4))), flush=True)


if __name__ == "__main__":
    main()
