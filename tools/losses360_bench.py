"""The mip-NeRF 360 interlevel loss: what the HIP node costs per training step.

    python tools/losses360_bench.py [--steps K] [--warmup W]

bench.py's config-B model, the 8192-ray training step under bf16 autocast (forward with rand=True, data + anti-interlevel +
distortion + hash-decay losses, backward, nan_to_num, Adam -- bench.train_step_ms's step) with `interlevel_loss_mult = 1` added,
three ways in ONE process on the same model: without the term, with train_utils.interlevel_loss (`ucn_outer_loss`, one launch
per proposal level; the run fails if the torch form is taken), and with the quadratic formulation of the same loss in eager torch
(comparison tensors of [N, S_prop+1, S_nerf+1], like the reference's stepfun.py:6-61), which is the kind of code the drop-in overlay
handed train.py before.  Warm-up steps, then the median of `steps`
timed steps (device synchronised around each), one JSON line per variant and one with the differences."""
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
from ucnerf_amd.internal import train_utils as tu  # noqa: E402


def interlevel_eager(ray_history, config):
    """The quadratic formulation in eager torch: per proposal level one [N, S_prop+1, S_nerf+1] comparison table, from it the index
    of the last proposal fencepost not above and of the first one above every NeRF fencepost (a masked-index tensor and a reduction
    over S_prop+1 each), then the envelope from the running proposal mass.  The same tensors, sizes and passes as the formulation the
    caller's own train_utils runs under the overlay when this package does not provide the function."""
    c, w = ray_history[-1]['sdist'].detach(), ray_history[-1]['weights'].detach()
    total = 0.
    for h in ray_history[:-1]:
        cp, wp = h['sdist'], h['weights']
        n = cp.shape[-1]
        not_above = cp.unsqueeze(-1) <= c.unsqueeze(-2)
        k = torch.arange(n, device=cp.device).unsqueeze(-1)
        lo, hi = (not_above * k).amax(dim=-2), torch.where(not_above, n - 1, k).amin(dim=-2)
        mass = torch.nn.functional.pad(wp.cumsum(dim=-1), (1, 0))
        excess = (w - (mass.gather(-1, hi[..., 1:]) - mass.gather(-1, lo[..., :-1]))).clamp_min(0)
        total = total + (excess * excess / (w + torch.finfo(c.dtype).eps)).mean()
    return config.interlevel_loss_mult * total


def _no_torch_form(*a):
    raise AssertionError("the 'node' variant took train_utils' torch form, not ucn_outer_loss")


def step_ms(model, flat, device, variant, steps, warmup, n_rays=8192):
    cfg = types.SimpleNamespace(data_loss_type='charb', charb_padding=0.001, data_loss_mult=1.0, data_coarse_loss_mult=0.,
                                anti_interlevel_loss_mult=0.01, pulse_width=[0.03, 0.003], distortion_loss_mult=0.005,
                                hash_decay_mults=0.1, disable_multiscale_loss=False, interlevel_loss_mult=1.0)
    g = torch.Generator(device=device).manual_seed(2)
    opt = tu.FusedAdam(model.parameters(), lr=0.01, betas=(0.9, 0.99), eps=1e-8)
    model.train()
    times, last = [], None
    n_total = flat['origins'].shape[0]
    for it in range(warmup + steps):
        idx = torch.randint(0, n_total, (n_rays,), device=device, generator=g)
        batch = {k: v[idx][:, None, None, :] for k, v in flat.items()}
        batch['rgb'] = torch.rand(n_rays, 1, 1, 3, device=device, generator=g)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.autocast('cuda', dtype=torch.bfloat16):
            rend, hist = model(True, batch, 0.5, False, zero_glo=False)
        loss = (tu.compute_data_loss(batch, rend, cfg)[0] + tu.anti_interlevel_loss(hist, cfg) + tu.distortion_loss(hist, cfg)
                + tu.hash_decay_loss(hist, cfg))
        if variant == "node":
            keep, tu._outer_level_torch = tu._outer_level_torch, _no_torch_form      # the route is asserted, not assumed
            try:
                last = tu.interlevel_loss(hist, cfg)
            finally:
                tu._outer_level_torch = keep
            loss = loss + last
        elif variant == "eager":
            last = interlevel_eager(hist, cfg)
            loss = loss + last
        opt.zero_grad(set_to_none=True)
        loss.backward()
        tu.clip_gradients(model, None, cfg)
        opt.step()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    model.eval()
    shapes = [list(h['weights'].shape[-1:]) for h in hist]
    route = {"none": None, "node": "ucn_outer_loss (asserted)", "eager": "eager torch, comparison tables"}[variant]
    return dict(variant=variant, route=route, ms=round(float(np.median(times)), 3), min_ms=round(min(times), 3), max_ms=round(max(times), 3), steps=steps,
                warmup=warmup, rays=n_rays, samples_per_level=[s[0] for s in shapes],
                interlevel=None if last is None else float(last.detach()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    flat = {k: v.reshape(-1, v.shape[-1]) for k, v in bench.frame_rays(dev).items()}
    state, out = None, {}
    for variant in ("none", "node", "eager", "none"):                # `none` again last: drift of the process over the run
        model = bench.build_model(dev)[0]
        if state is None:
            state = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(state)                                  # every variant starts from the same weights
        r = step_ms(model, flat, dev, variant, args.steps, args.warmup)
        out.setdefault(variant, []).append(r)
        print(json.dumps(r), flush=True)
        del model
        torch.cuda.empty_cache()
    base = float(np.mean([r["ms"] for r in out["none"]]))
    print(json.dumps(dict(figure="interlevel_cost_ms_per_step", node=round(out["node"][0]["ms"] - base, 3),
                          eager=round(out["eager"][0]["ms"] - base, 3), baseline_ms=round(base, 3),
                          baseline_spread_ms=round(abs(out["none"][0]["ms"] - out["none"][1]["ms"]), 3))), flush=True)


if __name__ == "__main__":
    main()
