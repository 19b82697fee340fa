"""`internal.image` of the drop-in overlay: the reference's own module (loaded from the caller's `internal/`, so mse_to_psnr,
linear_to_srgb, downsample, its metric harness ... are there unchanged) with `color_correct` replaced by this repo's device
implementation of the same name and signature (eval.py's step between render_image and the colour-corrected metrics)."""
import importlib.util as _ilu
import os as _os
import sys as _sys

from . import UPSTREAM as _UPSTREAM

_spec = _ilu.spec_from_file_location("internal._upstream_image", _os.path.join(_UPSTREAM, "image.py"))
_up = _ilu.module_from_spec(_spec)
_sys.modules["internal._upstream_image"] = _up
_spec.loader.exec_module(_up)
globals().update({k: v for k, v in vars(_up).items() if not k.startswith("__")})
upstream = _up

from ucnerf_amd.internal.image import color_correct  # noqa: E402,F401
