"""The Ref-NeRF colour heads (NerfMLP.use_diffuse_color, use_specular_tint, enable_pred_roughness): what they cost.

    python tools/ref_colour_bench.py [--steps K] [--frames F] [--only train|frame] [--passes P] [--flag on|off]

On bench.py's config-B model (NeRF grid L16 / C2 / T = 2^19, proposal grid L6, 64 + 128 samples), with the flags off (the shipped
configuration) and with all three on the NeRF field on the SAME weights plus seeded head layers (the proposal field stays as shipped: the
figures are the NeRF level's):
  * the 1280 x 1920 frame through render_image, fp32-class (under bf16 autocast a field with the heads renders on the same path);
    --passes P renders only the first P passes of max_chunk_rays rays (for a run under rocprofv3 --kernel-trace --stats, which gives
    k_ref_heads per launch beside k_field_mlp_h8 and k_march_features in the same run);
  * the training step at 8192 rays (bench.train_step_ms), bf16 autocast and fp32: with the flags the NeRF level's dense layers take the
    colour-node route, which materialises the bottleneck, plus the heads' stacked GEMM and the colour node.
One JSON line per figure.
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

FLAGS = dict(use_diffuse_color=True, use_specular_tint=True, enable_pred_roughness=True)
LAYERS = ("diffuse_layer", "specular_layer", "roughness_layer")


def build(device, heads):
    """bench.py's model; with the heads, the same weights and seeded head layers on the NeRF field."""
    base = bench.build_model(device)[0]
    if not heads:
        return base
    with models.bindings(NerfMLP=FLAGS):
        torch.manual_seed(0)
        model = bench.build_model(device)[0]
    missing, unexpected = model.load_state_dict(base.state_dict(), strict=False)
    assert not unexpected and sorted(missing) == sorted(f"nerf_mlp.{l}.{p}" for l in LAYERS for p in ("bias", "weight")), (missing, unexpected)
    del base
    return model


def frame_ms(model, rays, frames, heads):
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
    assert ("roughness" in out) == heads
    if heads:
        assert torch.isfinite(out["roughness"]).all()
    model.eval()
    return float(np.median(times)), [round(t, 2) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--only", choices=("train", "frame"), default=None)
    ap.add_argument("--passes", type=int, default=0, help="render only the first P passes of the frame (0: the whole frame)")
    ap.add_argument("--flag", choices=("on", "off"), default=None, help="only with the heads on / off (default: both)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rays = bench.frame_rays(dev)
    flat = {k: v.reshape(-1, v.shape[-1]) for k, v in rays.items()}
    for heads in (False, True):
        if args.flag is not None and heads != (args.flag == "on"):
            continue
        model = build(dev, heads)
        if args.only != "train":             # frames first: the training steps below move the weights
            part, n = rays, flat["origins"].shape[0]
            if args.passes:
                n = args.passes * int(model.max_chunk_rays)
                part = {k: v[:n].reshape(args.passes, -1, v.shape[-1]) for k, v in flat.items()}
            ms, all_ms = frame_ms(model, part, args.frames, heads)
            print(json.dumps(dict(figure="frame_1280x1920" if not args.passes else f"frame_first_{args.passes}_passes", ref_colour=heads,
                                  rays=n, ms=round(ms, 2), frames=all_ms, route=model.last_march_route)), flush=True)
        if args.only != "frame":
            for autocast in (True, False):
                engine = dense_f32.engine()
                r = bench.train_step_ms(model, flat, dev, n_rays=8192, steps=args.steps, autocast=autocast)
                print(json.dumps(dict(figure="train_step", ref_colour=heads, autocast=autocast, engine=None if autocast else engine,
                                      ms=round(r["ms"], 3), rays=8192, steps=args.steps)), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
