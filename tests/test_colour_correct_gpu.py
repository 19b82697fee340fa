"""image.color_correct on the device (ucn_colour_correct) against the float64 restatement tests/colour_correct_ref.py, by the
bracket scheme of DESIGN.md 7h / 7i: the device may be off by four times what the reference's own float32 result (recorded in
tests/golden/colour_correct.npz) is off, and never less than four float32 roundings of the largest value.  Reads only tests/golden/."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import colour_correct_ref as cc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def image():
    from ucnerf_amd.internal import image
    return image


@pytest.fixture(scope="module")
def restated():
    fx = cc.fixture()
    return fx, {name: cc.restate(fx[f"{name}_img"], fx[f"{name}_ref"]) for name in cc.CASES}


@pytest.mark.parametrize("name", cc.CASES)
def test_parity_with_the_float64_restatement(image, restated, name):
    fx, res = restated
    img, ref, want = fx[f"{name}_img"], fx[f"{name}_ref"], res[name]
    assert cc.condition_gap(name[0], img, ref, want) >= cc.MARGIN
    out, warps = image.color_correct(torch.from_numpy(img).cuda(), torch.from_numpy(ref).cuda(), return_warps=True)
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == img.shape and warps.shape == (5, 10, 3)
    for what, got, rec, truth in (("out", out, fx[f"{name}_out"], want["out"]), ("warps", warps, fx[f"{name}_warps"], want["warps"])):
        err, ref_err = cc.max_err(got.cpu().numpy(), truth), cc.max_err(rec, truth)
        bar = cc.allowed(ref_err, truth)
        print(f"{name} {what}: device {err:.3e}  reference float32 {ref_err:.3e}  allowed {bar:.3e}")
        assert err <= bar, (name, what, err, bar)


def test_grid_stride_size_against_the_float32_formulation(image):
    """301 x 500 = 150500 pixels: more than the 512 x 256 a launch covers in one stride, and a ragged last stride.  No fixture of that size
    fits the repository; the float32 formulation's own error is the float32 restatement's here."""
    img, ref = cc.make_inputs("b", 301, 500, 77)
    want, f32 = cc.restate(img, ref), cc.restate(img, ref, dtype=np.float32)
    assert cc.condition_gap("b", img, ref, want) >= cc.MARGIN
    out, warps = image.color_correct(img, ref, return_warps=True)                       # numpy arrays are uploaded
    for what, got, rec, truth in (("out", out, f32["out"], want["out"]), ("warps", warps, f32["warps"], want["warps"])):
        err, ref_err = cc.max_err(got.cpu().numpy(), truth), cc.max_err(rec, truth)
        bar = cc.allowed(ref_err, truth)
        print(f"b_301x500 {what}: device {err:.3e}  float32 restatement {ref_err:.3e}  allowed {bar:.3e}")
        assert err <= bar, (what, err, bar)


def test_two_calls_are_bit_identical(image, restated):
    fx, _ = restated
    for name in ("c_67x129", "b_4x5"):
        img, ref = torch.from_numpy(fx[f"{name}_img"]).cuda(), torch.from_numpy(fx[f"{name}_ref"]).cuda()
        a, wa = image.color_correct(img, ref, return_warps=True)
        b, wb = image.color_correct(img, ref, return_warps=True)
        assert torch.equal(a, b) and torch.equal(wa, wb)


def test_iteration_count_eps_and_dtypes(image, restated):
    fx, res = restated
    name = "c_24x20"
    img, ref, want = fx[f"{name}_img"], fx[f"{name}_ref"], res[name]
    floor = 4 * cc.EPS32
    out0 = image.color_correct(torch.from_numpy(img).cuda(), torch.from_numpy(ref).cuda(), num_iters=0)
    assert np.array_equal(out0.cpu().numpy(), img)
    out1, w1 = image.color_correct(img, ref, num_iters=1, return_warps=True)
    assert w1.shape == (1, 10, 3)
    # one iteration from exact inputs: the estimate is ten products of values <= 1 with float32-rounded coefficients, so it is off by at
    # most a few float32 roundings of the largest coefficient (or of 1)
    wmax = max(1.0, float(np.abs(want["warps"][0]).max()))
    assert cc.max_err(out1.cpu().numpy().reshape(-1, 3), want["iterates"][1]) <= floor * wmax
    assert cc.max_err(w1.cpu().numpy()[0], want["warps"][0]) <= floor * wmax
    # eps = 2 / 255 against the default on an image with values between the two: other rows, another result
    img_e, ref_e = fx["b_24x20_img"].copy(), fx["b_24x20_ref"].copy()
    img_e[::7, ::3, 0] = 0.005
    ref_e[::5, ::4, 1] = 0.994
    eps = 2 / 255
    want_d, want_e = cc.restate(img_e, ref_e), cc.restate(img_e, ref_e, eps=eps)
    assert cc.condition_gap("b", img_e, ref_e, want_d) >= cc.MARGIN and cc.condition_gap("b", img_e, ref_e, want_e, eps) >= cc.MARGIN
    assert (want_e["masks"] != want_d["masks"]).any(axis=2).mean() >= 0.05 and cc.max_err(want_e["out"], want_d["out"]) >= 0.01
    for e, truth in ((0.5 / 255, want_d), (eps, want_e)):
        got = image.color_correct(img_e, ref_e, 5, e)
        f32 = cc.restate(img_e, ref_e, eps=e, dtype=np.float32)
        err, bar = cc.max_err(got.cpu().numpy(), truth["out"]), cc.allowed(cc.max_err(f32["out"], truth["out"]), truth["out"])
        print(f"eps {e:.5f}: device {err:.3e}  allowed {bar:.3e}")
        assert err <= bar
    # any float dtype, CPU tensors, leading dimensions
    outd = image.color_correct(torch.from_numpy(img).double().reshape(2, 12, 20, 3), torch.from_numpy(ref).double().reshape(2, 12, 20, 3))
    assert outd.shape == (2, 12, 20, 3) and outd.dtype == torch.float32
    assert torch.equal(outd.reshape(24, 20, 3), image.color_correct(img, ref))
    assert image.color_correct(torch.zeros(0, 3), torch.zeros(0, 3)).shape == (0, 3)


def _status_bits(img, ref, num_iters=5):
    """The status word through the C ABI."""
    from ucnerf_amd import _lib
    lib = _lib.load()
    p, g = torch.from_numpy(img).cuda().reshape(-1, 3).contiguous(), torch.from_numpy(ref).cuda().reshape(-1, 3).contiguous()
    n = p.shape[0]
    ws = torch.empty(lib.ucn_colour_correct_ws_bytes(n), dtype=torch.uint8, device="cuda")
    out, status = torch.empty_like(p), torch.full((1,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.ucn_colour_correct(p.data_ptr(), g.data_ptr(), n, num_iters, 0.5 / 255, ws.data_ptr(), out.data_ptr(), None,
                                      status.data_ptr(), _lib.stream()))
    return int(status.item())


def test_rank_deficiency_raises_and_names_the_channel(image, restated):
    """The design matrix is shared by the three channels (its row holds r, g and b), so an img that is constant in one channel makes all
    three systems singular: the error names that channel among them.  One channel alone is deficient when its MASK leaves too few rows;
    a ref channel that is clipped everywhere does that, and there the other two bits stay clear."""
    fx, _ = restated
    img, ref = fx["a_24x20_img"].copy(), fx["a_24x20_ref"].copy()
    assert _status_bits(img, ref) == 0
    const = img.copy()
    const[..., 1] = 0.5
    with pytest.raises(RuntimeError, match=r"channel .*1 \(g\).* rank deficient"):
        image.color_correct(const, ref)
    for c in range(3):
        clipped = ref.copy()
        clipped[..., c] = 1.0
        assert _status_bits(img, clipped) == 1 << c
        with pytest.raises(RuntimeError, match=rf"channel {c} \({'rgb'[c]}\) is rank deficient"):
            image.color_correct(img, clipped)
    # fewer than ten rows: 3 x 3 pixels
    assert _status_bits(img[:3, :3].copy(), ref[:3, :3].copy()) == 7
    # num_iters = 0 clears the word
    assert _status_bits(img, ref, num_iters=0) == 0


def test_overlay_image_module_has_this_color_correct_and_the_callers_other_names():
    standin = os.path.join(REPO, "tests", "stubs", "upstream_internal_standin")
    code = ("import internal.image as im, ucnerf_amd.internal.image as ours\n"
            "assert im.color_correct is ours.color_correct\n"
            "assert im.MetricHarness.STANDIN and im.MetricHarness is im.upstream.MetricHarness and im.mse_to_psnr is im.upstream.mse_to_psnr\n"
            "import numpy as np\n"
            "x = np.random.default_rng(0).uniform(0.1, 0.9, (8, 8, 3)).astype(np.float32)\n"
            "y = im.color_correct(x, 0.5 * x + 0.2)\n"
            "assert y.is_cuda and float((y.cpu() - (0.5 * x + 0.2)).abs().max()) < 1e-5\n"
            "print('OK')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(REPO, "ucnerf_amd", "compat", "dropin"), REPO]))
    p = subprocess.run([sys.executable, "-B", "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=standin)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
