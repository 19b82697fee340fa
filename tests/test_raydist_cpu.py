"""Warped ray distances (Model.raydist_fn, coord.py:137-177), host side: which curve a Model resolves from every value the
reference accepts (gin binds the torch callables of configs.py:13-19), the values it refuses, the unchanged state dict, and
the reference fixtures' own float32-vs-float64 curve values (tests/golden/raydist_*.npz, make_raydist_golden.py)."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
from oracle import raymarch as rm

CURVE_FILES = ["raydist_power.npz", "raydist_piecewise.npz", "raydist_reciprocal.npz"]


def raydist_model(fn, **kw):
    """A `tiny` Model with Model.raydist_fn bound as a class attribute, the way gin binds it."""
    from ucnerf_amd.internal import models
    spec = rm.make_spec("tiny")
    with models.bindings(Model=dict(raydist_fn=fn, **kw)):
        model, _ = H.hip_model(spec, rm.init_state(spec, seed=3), device="cpu")
    return model


def s_to_t_f64(curve, s, near, far, lam=-1.5):
    """coord.py:137-177 in float64 with the float32 eps of inv_power_transformation (the formula the float32 kernels evaluate)."""
    lam_1, eps = abs(lam - 1), float(np.finfo(np.float32).eps)
    fwd, inv = {
        "power_transformation": (lambda x: lam_1 / lam * ((2 * x / lam_1 + 1) ** lam - 1),
                                 lambda y: ((y * lam / lam_1 + 1 + eps) ** (1 / lam) - 1) * lam_1 / 2),
        "piecewise": (lambda x: np.where(x < 1, .5 * x, 1 - .5 / np.maximum(x, 1e-300)),
                      lambda y: np.where(y < .5, 2 * y, .5 / np.maximum(1 - y, 1e-300))),
        "reciprocal": (lambda x: 1 / x, lambda y: 1 / y),
    }[curve]
    sn, sf = fwd(near), fwd(far)
    return inv(s * sf + (1 - s) * sn)


@pytest.mark.parametrize("fn,want", [(None, 0), ("piecewise", 1), ("power_transformation", 2), (torch.reciprocal, 3),
                                     (torch.log, 4), (torch.exp, 5), (torch.sqrt, 6), (torch.square, 7)])
def test_curve_resolution_from_every_accepted_value(fn, want):
    from ucnerf_amd.internal import models
    assert models.raydist_curve(fn) == want
    model = raydist_model(fn)
    assert model._raydist_curve == want
    # resolved once: the class default coming back after the binding does not change the built model
    assert models.Model.raydist_fn is None and model._raydist_curve == want


def test_power_lambda_binds_like_the_reference():
    model = raydist_model("power_transformation", power_lambda=-2.0)
    assert model._raydist_curve == 2 and model.power_lambda == -2.0


@pytest.mark.parametrize("fn", [torch.log1p, lambda x: x, np.log, "reciprocal", "power", torch.tanh])
def test_values_the_reference_cannot_invert_are_refused_at_construction(fn):
    with pytest.raises(ValueError, match="raydist_fn"):
        raydist_model(fn)


def test_log1p_names_the_missing_inverse():
    with pytest.raises(ValueError, match="no inverse"):
        raydist_model(torch.log1p)


def gin_wrapped(fn):
    """What `Model.raydist_fn = @torch.reciprocal` hands over under gin: the configurable's functools.wraps wrapper, a different
    object with the same __name__ (configs.py:13-19 registers the torch functions with gin.external_configurable)."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        return fn(*args, **kwargs)
    return wrapper


@pytest.mark.parametrize("fn,want", [(torch.reciprocal, 3), (torch.log, 4), (torch.exp, 5), (torch.sqrt, 6), (torch.square, 7)])
def test_gin_wrapped_torch_callables_resolve_by_name(fn, want):
    from ucnerf_amd.internal import models
    wrapped = gin_wrapped(fn)
    assert wrapped is not fn and wrapped.__name__ == fn.__name__
    assert models.raydist_curve(wrapped) == want
    assert models.raydist_curve(gin_wrapped(wrapped)) == want             # a wrapper of a wrapper
    assert raydist_model(wrapped)._raydist_curve == want


def test_gin_wrapped_log1p_and_impostors_are_refused():
    with pytest.raises(ValueError, match="no inverse"):
        raydist_model(gin_wrapped(torch.log1p))

    def reciprocal(x):                                                     # the right name, not the torch function
        return 1 / x
    with pytest.raises(ValueError, match="only the reference's curves"):
        raydist_model(reciprocal)
    with pytest.raises(ValueError, match="only the reference's curves"):
        raydist_model(gin_wrapped(reciprocal))


@pytest.mark.parametrize("fn", ["piecewise", "power_transformation", torch.reciprocal])
def test_state_dict_keys_and_shapes_are_unchanged(fn):
    plain, warped = raydist_model(None).state_dict(), raydist_model(fn).state_dict()
    assert list(plain) == list(warped)
    assert [tuple(v.shape) for v in plain.values()] == [tuple(v.shape) for v in warped.values()]


@pytest.mark.parametrize("name", CURVE_FILES)
def test_fixture_curve_float32_agrees_with_float64(name):
    """The reference's float32 s_to_t against its float64 run: a few ulp of t, plus what the inverse's slope makes of the
    rounding of its argument y = s * s_far + (1 - s) * s_near (power curve near s_far: 1 - 0.6 y + eps cancels), plus, for
    the power curve, the float32 eps it adds (float64 adds 2^-52)."""
    fx = H.load(name)
    curve = bytes(fx["raydist"].numpy()).decode().replace("torch.", "")
    s, near, far = (fx[k].double().numpy() for k in ("curve_s", "curve_near", "curve_far"))
    t32, t64 = fx["curve_t_f32"].double().numpy(), fx["curve_t_f64"].double().numpy()
    assert np.isfinite(t32).all() and np.isfinite(t64).all()
    ulp = np.spacing(np.abs(t64).astype(np.float32)).astype(np.float64)
    exact = s_to_t_f64(curve, s, near, far)                      # float32 eps, float64 arithmetic
    h = 1e-7
    slope = np.abs(s_to_t_f64(curve, np.clip(s + h, 0, 1), near, far) - s_to_t_f64(curve, np.clip(s - h, 0, 1), near, far))
    slope = slope / np.maximum(np.clip(s + h, 0, 1) - np.clip(s - h, 0, 1), 1e-300)    # dt/ds; dt/dy = slope / (s_far - s_near)
    # the power inverse forms t from (pow - 1) * lam_1 / 2 with pow ~ 2 t / lam_1 + 1: its rounding is an ulp of t + lam_1 / 2
    base = np.abs(t64) + (1.25 if curve == "power_transformation" else 0.0)
    bound = 8 * np.spacing(base.astype(np.float32)).astype(np.float64) + 4 * slope * 2.0 ** -24 * np.maximum(s, 1e-3)
    assert (np.abs(t32 - exact) <= bound).all(), float(np.max(np.abs(t32 - exact) / bound))
    if curve == "power_transformation":
        assert (np.abs(t64 - exact) <= np.abs(t32 - t64) + bound).all()
    else:
        assert (np.abs(t64 - exact) <= 4 * ulp).all()
    # endpoints: s = 0 and s = 1 map to near and far, every ray, every curve (float64: the power curve's 2^-52 eps moves t by
    # (2 / 3) 2^-52 / (1 - 0.6 s_far) relative, < 1e-7 up to far = 1e5)
    assert np.abs(t32[:, 0] - near[:, 0]).max() <= 8 * ulp[:, 0].max() + 1e-6
    assert np.allclose(t64[:, 0], near[:, 0], rtol=0, atol=1e-12)
    assert np.allclose(t64[:, 1], far[:, 0], rtol=1e-7, atol=0)
