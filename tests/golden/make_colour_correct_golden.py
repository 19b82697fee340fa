"""Generate tests/golden/colour_correct.npz: the REFERENCE's image.color_correct (image.py:71-111), on CPU in float32.

    python tests/golden/make_colour_correct_golden.py          (authoring container only)

Same harness as the other generators (ref_import: the reference's own Python).  Data only: per case the float32 inputs `img`, `ref`
[H, W, 3], the reference's corrected image `out` with its defaults (num_iters 5, eps 0.5 / 255), its fifteen lstsq solutions as `warps` [5, 10, 3]
(recorded at torch.linalg.lstsq while it runs), and the seed that produced the inputs.

Shapes, the smallest at which each part of the device path can go wrong: 4 x 5 (20 pixels: less than a wave, one partial), 24 x 20 (two
workgroups), 67 x 129 (odd sizes, 34 workgroups, a ragged tail).  Regimes (tests/colour_correct_ref.py make_inputs):

  a   ref = a fixed mild quadratic warp of a uniform random img plus N(0, 0.01) noise, everything inside [eps, 1 - eps]
  b   as a, with 15 % of img's values and 15 % of ref's pushed to exactly 0 or 1: all three mask terms are live
  c   as b, with a warp strong enough that the current-estimate mask term differs between iteration 0 and iteration 4 in at least 1 % of
      the rows; asserted in the stricter form that these rows are unclipped in img and saturated in the fifth estimate

Condition on every case, asserted here from the float64 restatement and again by the tests: no value of img, ref or any iterate lies
within 1e-5 of eps, 1 - eps, 0 or 1 unless it is exactly 0 or 1, so a float32 rounding cannot flip a mask or a clip between
implementations.  Seeds are redrawn until it holds.  Regime c's iterates keep that distance from eps and 1 - eps only: a saturated value
comes back from the next warp arbitrarily close to 0 or 1 (colour_correct_ref.condition_gap), and the clip is continuous.  The 4 x 5 image of regimes b and c would leave fewer than ten unclipped rows in a
channel for most seeds; a seed is also redrawn until every channel keeps at least 12 rows in every iteration.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import colour_correct_ref as cc  # noqa: E402
import ref_import  # noqa: E402


def main():
    ref = ref_import.load()
    image = ref.models.image
    out = {}
    for ri, regime in enumerate(cc.REGIMES):
        for si, (h, w) in enumerate(cc.SHAPES):
            for attempt in range(200):
                seed = 1000 * (ri + 1) + 100 * si + attempt
                img, tgt = cc.make_inputs(regime, h, w, seed)
                res = cc.restate(img, tgt)
                rows = res["masks"].sum(axis=1).min()
                if cc.condition_gap(regime, img, tgt, res) >= cc.MARGIN and rows >= 12 and (regime != "c" or cc.saturating_rows(res) >= 0.01):
                    break
            else:
                raise AssertionError(f"no seed for {regime} {h}x{w}")
            cur_term = [cc.unclipped(res["iterates"][k], cc.EPS_DEFAULT) for k in (0, 4)]
            cur_flipped = float((cur_term[0] != cur_term[1]).any(axis=1).mean())
            if regime == "a":
                assert cc.unclipped(img, cc.EPS_DEFAULT).all() and cc.unclipped(tgt, cc.EPS_DEFAULT).all()
            else:
                for arr in (img, tgt):
                    share = float(((arr == 0) | (arr == 1)).mean())
                    assert 0.08 <= share <= 0.30, share
            if regime == "c":
                assert cc.saturating_rows(res) >= 0.01
            solves, lstsq = [], torch.linalg.lstsq

            def recording(*a, **k):
                r = lstsq(*a, **k)
                solves.append(r[0].clone())
                return r
            torch.linalg.lstsq = recording
            try:
                with torch.no_grad():
                    got = image.color_correct(torch.from_numpy(img), torch.from_numpy(tgt)).numpy()
            finally:
                torch.linalg.lstsq = lstsq
            assert got.dtype == np.float32 and got.shape == img.shape and len(solves) == 15
            warps = torch.stack(solves).reshape(5, 3, 10).permute(0, 2, 1).contiguous().numpy()      # [iteration][term][channel]
            name = f"{regime}_{h}x{w}"
            out[f"{name}_img"], out[f"{name}_ref"], out[f"{name}_out"] = img, tgt, got
            out[f"{name}_warps"] = warps
            out[f"{name}_seed"] = np.int64(seed)
            print(f"{name}: seed {seed}  rows >= {rows}  cur-mask rows changed it0 -> it4 {cur_flipped:.3f} (unclipped -> clipped {cc.saturating_rows(res):.3f})  "
                  f"cond {cc.condition_number(img, tgt, res):.1f}  threshold gap "
                  f"{cc.condition_gap(regime, img, tgt, res):.2e}  "
                  f"reference vs float64 restatement: out {cc.max_err(got, res['out']):.3e} warps {cc.max_err(warps, res['warps']):.3e}")
    np.savez_compressed(cc.GOLDEN, **out)
    print("wrote", cc.GOLDEN, os.path.getsize(cc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
