"""Scale featurization: what it costs.

    python tools/scalefeat_bench.py [--steps K] [--frames F] [--rounds R] [--only train|frame]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/scalefeat_bench.py --only frame --rounds 1     (per-kernel times)

On bench.py's config-B model (NeRF grid L16 / C2 / T = 2^19, 64 + 128 samples), with NerfMLP / PropMLP.scale_featurization off
and on, ALTERNATING (off, on, off, on, ...: clock and temperature drift hits both sides alike):
  * the 1280 x 1920 frame through render_image, fp32-class and under bf16 autocast (where a flag-on field stays on the fp32-class
    path while the flag-off model takes the mixed-precision kernels: that pair shows what a user rendering under autocast pays);
  * the training step at 8192 rays (bench.train_step_ms), bf16 autocast and fp32.
The flag-on model carries the flag-off model's weights, with zero columns for the scale inputs: the samples land where they do
without the feature, so the difference is the extra kernel (k_march_scale_features), the wider first dense layer and, per
training step, the table read of k_level_scale_partial.  One JSON line per figure.  Under rocprofv3 compare
k_march_scale_features with k_march_features in the same run's stats.
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import bench  # noqa: E402
from glo_bench import frame_ms  # noqa: E402
from ucnerf_amd.internal import dense_f32, models  # noqa: E402


def build(device, on):
    base = bench.build_model(device)[0]
    if not on:
        return base
    with models.bindings(NerfMLP=dict(scale_featurization=True), PropMLP=dict(scale_featurization=True)):
        model = bench.build_model(device)[0]
    sd = {k: v.clone() for k, v in base.state_dict().items()}
    for k, v in model.state_dict().items():
        if k.endswith("density_layer.0.weight"):
            wide = torch.zeros_like(v)
            wide[:, :sd[k].shape[1]] = sd[k]
            sd[k] = wide
    model.load_state_dict(sd, strict=True)
    del base
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", choices=("train", "frame"), default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    flat = {k: v.reshape(-1, v.shape[-1]) for k, v in bench.frame_rays(dev).items()}
    model = {on: build(dev, on) for on in (False, True)}
    if args.only != "train":                 # frames first: the training steps below move the weights
        for rnd in range(args.rounds):
            for autocast in (False, True):
                for on in (False, True):
                    model[on]._mixed_levels = 0
                    ms, all_ms = frame_ms(model[on], dev, args.frames, autocast)
                    print(json.dumps(dict(figure="frame_1280x1920", scale_featurization=on, autocast=autocast, round=rnd, ms=round(ms, 2),
                                          frames=all_ms, route=model[on].last_march_route,
                                          mixed_precision=model[on]._mixed_levels > 0)), flush=True)
    if args.only != "frame":
        for rnd in range(args.rounds):
            for autocast in (True, False):
                for on in (False, True):
                    r = bench.train_step_ms(model[on], flat, dev, n_rays=8192, steps=args.steps, autocast=autocast)
                    print(json.dumps(dict(figure="train_step", scale_featurization=on, round=rnd, autocast=autocast,
                                          engine=None if autocast else dense_f32.engine(), ms=round(r["ms"], 3), rays=8192,
                                          steps=args.steps)), flush=True)


if __name__ == "__main__":
    main()
