"""image.color_correct on the device (ucn_colour_correct): what it costs beside the reference's formulation.

    python tools/colour_correct_bench.py [--height H] [--width W] [--calls N] [--only hip|torch]

On one H x W frame (default 1280 x 1920, eval.py's Waymo frame) of seeded inputs (regime b of tests/colour_correct_ref.py: a quadratic
warp plus noise, 15 % of the values clipped), after a warm-up, the median of N >= 20 calls timed with device events:
  * hip: ucnerf_amd.internal.image.color_correct (num_iters + 1 streaming passes and num_iters solves, one status read);
  * torch: the reference's formulation written here in torch on the same device -- the concatenated [H W, 10] design matrix, three masked
    copies of it per iteration, fifteen torch.linalg.lstsq calls, the isfinite assertion after each.
--only hip under rocprofv3 --kernel-trace --stats gives k_cc_pass / k_cc_solve per launch; the bytes a pass must move (36 B read and 12 B
written per pixel; pass 0 reads 24 B and writes none, the last pass reads 12 B) are printed beside it.  One JSON line per figure.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import colour_correct_ref as cc  # noqa: E402
from ucnerf_amd.internal import image  # noqa: E402


def torch_formulation(img, ref, num_iters=5, eps=0.5 / 255):
    """The reference's formulation (image.py:71-111), this tool's own text: design matrix, masked copies, lstsq per channel."""
    x, b = img.reshape(-1, 3), ref.reshape(-1, 3)
    unclipped = lambda z: (z >= eps) & (z <= 1 - eps)  # noqa: E731
    mask0 = unclipped(x)
    for _ in range(num_iters):
        a = torch.cat([x[:, 0:1] * x, x[:, 1:2] * x[:, 1:], x[:, 2:3] * x[:, 2:], x, torch.ones_like(x[:, :1])], dim=-1)
        cols = []
        for c in range(3):
            mask = mask0[:, c] & unclipped(x[:, c]) & unclipped(b[:, c])
            w = torch.linalg.lstsq(torch.where(mask[:, None], a, torch.zeros_like(a)), torch.where(mask, b[:, c], torch.zeros_like(b[:, c])))[0]
            assert torch.all(torch.isfinite(w))
            cols.append(w)
        x = torch.clip(a @ torch.stack(cols, dim=-1), 0, 1)
    return x.reshape(img.shape)


def timed(fn, calls, warmup=3):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return out, float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "colour_correct_bench needs a GPU"
    n = args.height * args.width
    img_np, ref_np = cc.make_inputs("b", args.height, args.width, 5)
    img, ref = torch.from_numpy(img_np).cuda(), torch.from_numpy(ref_np).cuda()
    base = dict(height=args.height, width=args.width, num_iters=5, calls=args.calls)
    outs = {}
    if args.only in (None, "hip"):
        outs["hip"], med, lo, hi = timed(lambda: image.color_correct(img, ref), args.calls)
        moved = n * (24 + 4 * 48 + 24)          # pass 0: img, ref; passes 1..4: cur, img, ref in, cur out; pass 5: cur in, out
        print(json.dumps(dict(base, what="hip color_correct", median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                              bytes_the_passes_must_move=moved, per_pass_bytes=[n * 24] + [n * 48] * 4 + [n * 24])))
    if args.only in (None, "torch"):
        outs["torch"], med, lo, hi = timed(lambda: torch_formulation(img, ref), args.calls, warmup=2)
        print(json.dumps(dict(base, what="torch formulation (cat, where, 15 x lstsq)", median_ms=round(med, 4), min_ms=round(lo, 4),
                              max_ms=round(hi, 4))))
    if len(outs) == 2:
        print(json.dumps(dict(base, what="max |hip - torch|", value=float((outs["hip"] - outs["torch"]).abs().max()))))


if __name__ == "__main__":
    main()
