"""The mip-NeRF 360 loss terms (interlevel, opacity, rawnerf) on the host: the torch forms of
ucnerf_amd.internal.train_utils -- what runs wherever the HIP nodes do not apply -- against the reference's values and autograd
gradients in tests/golden/losses360.npz, to the bars of tests/losses360_ref.py; and the drop-in overlay's exports."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import losses360_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", R.OUTER_CASES)
def test_outer_level_torch_form_matches_the_reference(case):
    from ucnerf_amd.internal import train_utils as tu
    fx, k = R.fixture(), f"outer.{case}."
    wp = fx[k + "wp"].clone().requires_grad_(True)
    cfg = types.SimpleNamespace(interlevel_loss_mult=1.0)
    loss = tu.interlevel_loss([dict(sdist=fx[k + "cp"], weights=wp), dict(sdist=fx[k + "c"], weights=fx[k + "w"])], cfg)
    loss.backward()
    R.check(f"torch form, {case}", loss, fx, k + "loss")
    R.check(f"torch form, {case}", wp.grad, fx, k + "grad")
    if case == "special":
        assert float(wp.grad[2].abs().max()) == 0.0              # w <= w_outer everywhere: exactly nothing
        assert float(wp.grad[3].min()) * 5 * 32 < -1.9           # wp = 0: the half-quadratic's constant slope -2 (per interval, w >> eps)


def test_interlevel_loss_over_a_ray_history_with_leading_batch_dimensions():
    """train_utils.interlevel_loss of the reference on three levels; tensors shaped [N, 1, 1, S] like the training batch's"""
    from ucnerf_amd.internal import train_utils as tu
    fx = R.fixture()
    lead = lambda t: t[:, None, None, :]
    wps = [lead(fx[f"hist.weights.{i}"]).clone().requires_grad_(True) for i in range(2)]
    hist = [dict(sdist=lead(fx[f"hist.sdist.{i}"]), weights=wps[i]) for i in range(2)]
    hist.append(dict(sdist=lead(fx["hist.sdist.2"]), weights=lead(fx["hist.weights.2"]).clone().requires_grad_(True)))
    loss = tu.interlevel_loss(hist, types.SimpleNamespace(interlevel_loss_mult=float(fx["hist.mult"])))
    loss.backward()
    R.check("torch form, history", loss, fx, "hist.loss")
    for i in range(2):
        R.check("torch form, history", wps[i].grad.reshape(fx[f"hist.grad.{i}"].shape), fx, f"hist.grad.{i}")
    assert hist[-1]['weights'].grad is None                      # stop-gradient onto the NeRF level (train_utils.py:235-238)


def test_outer_level_torch_form_is_the_masked_form_on_ties():
    """the two binary searches against the comparison-table form where every value is a tie: fenceposts on a coarse lattice"""
    from ucnerf_amd.internal import train_utils as tu
    g = torch.Generator().manual_seed(5)
    c = torch.sort(torch.randint(0, 9, (64, 20), generator=g).float() / 8, dim=-1).values
    cp = torch.sort(torch.randint(0, 9, (64, 31), generator=g).float() / 8, dim=-1).values
    w, wp = torch.rand(64, 19, generator=g), torch.rand(64, 30, generator=g)
    assert torch.equal(tu._outer_level_torch(c, w, cp, wp), R.outer_masks(c, w, cp, wp).mean())


@pytest.mark.parametrize("case", R.OUTER_CASES)
def test_comparison_table_form_matches_the_reference(case):
    """the quadratic comparator the GPU tests use for inputs outside the fixture is itself held to the reference's values"""
    fx, k = R.fixture(), f"outer.{case}."
    wp = fx[k + "wp"].clone().requires_grad_(True)
    loss = R.outer_masks(fx[k + "c"], fx[k + "w"], fx[k + "cp"], wp).mean()
    loss.backward()
    R.check(f"comparison table, {case}", loss, fx, k + "loss")
    R.check(f"comparison table, {case}", wp.grad, fx, k + "grad")


@pytest.mark.parametrize("case", R.LEVEL_CASES)
def test_opacity_loss_torch_form_matches_the_reference(case):
    from ucnerf_amd.internal import train_utils as tu
    fx, k = R.fixture(), f"opacity.{case}."
    accs = [a.clone().requires_grad_(True) for a in R.levels_of(fx, k, "acc")]
    loss = tu.opacity_loss([dict(acc=a) for a in accs], types.SimpleNamespace(opacity_loss_mult=float(fx[k + "mult"])))
    loss.backward()
    R.check(f"torch form, opacity {case}", loss, fx, k + "loss")
    for l, a in enumerate(accs):
        R.check(f"torch form, opacity {case}", a.grad, fx, k + f"grad.{l}")


@pytest.mark.parametrize("case", R.LEVEL_CASES)
def test_rawnerf_data_loss_torch_form_matches_the_reference(case):
    from ucnerf_amd.internal import train_utils as tu
    fx, k = R.fixture(), f"rawnerf.{case}."
    rgbs = [r.clone().requires_grad_(True) for r in R.levels_of(fx, k, "rgb")]
    loss, stats = tu.compute_data_loss(dict(rgb=fx[k + "target"], lossmult=fx[k + "lossmult"]), [dict(rgb=r) for r in rgbs],
                                       R.rawnerf_config(fx[k + "coarse_mult"]))
    loss.backward()
    R.check(f"torch form, rawnerf {case}", loss, fx, k + "loss")
    R.check(f"torch form, rawnerf {case}", torch.from_numpy(np.asarray(stats['mses'])), fx, k + "mses")   # the UNCLIPPED residual
    for l, r in enumerate(rgbs):
        R.check(f"torch form, rawnerf {case}", r.grad, fx, k + f"grad.{l}")
        over = fx[k + f"rgb.{l}"] > 1
        assert bool(over.any()) and float(r.grad[over].abs().max()) == 0.0        # clamp_max's backward above the bound
    assert float(rgbs[0].grad[0, 0]) != 0.0                                          # ... and 1 AT the bound (rgb == 1, target < 1)


def test_data_loss_type_rawnerf_is_accepted_and_an_unknown_kind_is_not():
    from ucnerf_amd.internal import train_utils as tu
    batch = dict(rgb=torch.rand(4, 3), lossmult=torch.ones(4, 1))
    rend = [dict(rgb=torch.rand(4, 3))]
    cfg = R.rawnerf_config(0.0)
    assert torch.isfinite(tu.compute_data_loss(batch, rend, cfg)[0])
    cfg.data_loss_type = 'huber'
    with pytest.raises(NotImplementedError):
        tu.compute_data_loss(batch, rend, cfg)


def test_dropin_overlay_exports_the_two_losses():
    """`internal.train_utils` as the reference's train.py resolves it under the overlay hands out this package's functions"""
    code = ("from internal import train_utils as t\n"
            "assert t.interlevel_loss.__module__ == 'ucnerf_amd.internal.train_utils', t.interlevel_loss.__module__\n"
            "assert t.opacity_loss.__module__ == 'ucnerf_amd.internal.train_utils', t.opacity_loss.__module__\n"
            "assert t.compute_data_loss.__module__ == 'ucnerf_amd.internal.train_utils'\n"
            "assert t.tree_len.__module__ == 'internal._upstream_train_utils'\n"
            "print('OK')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(REPO, "ucnerf_amd", "compat", "dropin"), REPO]))
    p = subprocess.run([sys.executable, "-B", "-c", code], capture_output=True, text=True, timeout=300, env=env,
                       cwd=os.path.join(REPO, "tests", "stubs", "upstream_internal_standin"))
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
