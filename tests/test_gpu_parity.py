"""HIP path vs the golden fixtures of the reference and vs the CPU oracle (-m gpu).

Everything goes through the C ABI (ctypes -> libucnerf_march.so).  Bars: bit-exact for the hash
grid forward (integer addressing + a fixed fmaf chain); fp32 tolerances stated per quantity for the
rest; 1e-4 L-inf on RGB end to end (BASELINE.json north_star).
"""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
from oracle import grid_cpu
from oracle import raymarch as rm

pytestmark = pytest.mark.gpu


def dev(t):
    return t.cuda().contiguous()


# ------------------------------------------------------------------ a7 / a15: the `_gridencoder` op
@pytest.mark.parametrize("D,C", [(3, 2), (3, 4), (2, 2), (3, 1), (3, 8), (4, 2)])
@pytest.mark.parametrize("interp", [0, 1])
def test_grid_forward_bitexact(D, C, interp):
    from ucnerf_amd.gridencoder import _backend
    rng = np.random.default_rng(D * 10 + C)
    L, T = 9, 12
    pls, offsets, sizes, _ = grid_cpu.table_layout(L, C, 16, 4096, T, input_dim=D)
    table = torch.from_numpy(rng.random((int(offsets[-1]), C), dtype=np.float32) * 2 - 1)
    x = rng.random((5000, D), dtype=np.float32)
    x[:4] = [[0.0] * D, [1.0] * D, [np.nextafter(np.float32(1), np.float32(2))] * D, [-1e-7] * D]
    k = rng.integers(1, 4000, size=(64, D)).astype(np.float32)
    x[4:68] = (k - np.float32(0.5)) / np.float32(4095.0)
    x[68:100] = rng.random((32, D), dtype=np.float32) * 3 - 1
    x = torch.from_numpy(x)
    S = np.log2(pls)
    want = torch.empty(L, len(x), C)
    wjac = torch.empty(len(x), L * D * C)
    grid_cpu.grid_encode_forward(x, table, offsets, want, len(x), D, C, L, S, 16, wjac, 0, False, interp)
    got = torch.empty(L, len(x), C, device="cuda")
    gjac = torch.empty(len(x), L * D * C, device="cuda")
    _backend.grid_encode_forward(dev(x), dev(table), dev(offsets), got, len(x), D, C, L, S, 16, gjac, 0, False, interp)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(gjac.cpu(), wjac)


def test_gridencoder_extension_is_the_same_operator_as_the_ctypes_backend():
    """The `_gridencoder` torch extension (ucnerf_amd/csrc/ext/gridencoder_bindings.cpp, what the reference's grid.py:10
    imports) against the ctypes form of the same three functions: bit-identical forward (fp32 + fp16 tables, with dy_dx),
    backward (table + input gradients) and total variation; launches land on the CURRENT stream; and GridEncoder routed
    through it gives the same forward / backward as through the default backend."""
    from ucnerf_amd.gridencoder import _backend, native, GridEncoder
    ext = native.load()
    rng = np.random.default_rng(11)
    L, C, D, T = 8, 2, 3, 11
    pls, offsets, sizes, _ = grid_cpu.table_layout(L, C, 16, 2048, T)
    B = 3000
    x = dev(torch.from_numpy(rng.random((B, D), dtype=np.float32)))
    S = np.log2(pls)
    off = dev(offsets)
    for dt in (torch.float32, torch.float16):
        table = dev(torch.from_numpy(rng.random((int(offsets[-1]), C), dtype=np.float32) * 2 - 1)).to(dt)
        outs = []
        for be in (_backend, ext):
            o = torch.empty(L, B, C, device="cuda", dtype=dt)
            j = torch.empty(B, L * D * C, device="cuda", dtype=dt)
            be.grid_encode_forward(x, table, off, o, B, D, C, L, S, 16, j, 0, False, 0)
            grad = dev(torch.from_numpy(np.random.default_rng(12).standard_normal((L, B, C)).astype(np.float32))).to(dt)
            ge = torch.zeros_like(table)
            gi = torch.zeros(B, D, device="cuda", dtype=dt)
            be.grid_encode_backward(grad, x, table, off, ge, B, D, C, L, S, 16, j, gi, 0, False, 0)
            outs.append((o, j, ge, gi))
        (o0, j0, ge0, gi0), (o1, j1, ge1, gi1) = outs
        assert torch.equal(o0, o1) and torch.equal(j0, j1) and torch.equal(gi0, gi1)
        # the table gradient is accumulated with atomics: equal up to the order of the additions
        tol = 1e-5 if dt == torch.float32 else 2e-2
        assert float((ge0.float() - ge1.float()).abs().max()) <= tol * max(1.0, float(ge0.float().abs().max())) and float(ge0.abs().max()) > 0
    table = dev(torch.from_numpy(rng.random((int(offsets[-1]), C), dtype=np.float32)))
    tv = []
    for be in (_backend, ext):
        g = torch.zeros_like(table)
        be.grad_total_variation(x, table, g, off, 0.3, B, D, C, L, S, 16, 0, False)
        tv.append(g)
    assert float(tv[0].abs().max()) > 0, 'total variation wrote nothing'
    assert float((tv[0] - tv[1]).abs().max()) <= 1e-5 * max(1.0, float(tv[0].abs().max()))      # atomics again
    # current-stream semantics: a side stream that first waits on a long fill must still see its own ordering
    side = torch.cuda.Stream()
    o = torch.empty(L, B, C, device="cuda")
    with torch.cuda.stream(side):
        tbl = torch.zeros_like(table)
        tbl.copy_(table)                                   # enqueued on `side`; the encode below must run after it
        ext.grid_encode_forward(x, tbl, off, o, B, D, C, L, S, 16, None, 0, False, 0)
    side.synchronize()
    ref = torch.empty(L, B, C, device="cuda")
    _backend.grid_encode_forward(x, table, off, ref, B, D, C, L, S, 16, None, 0, False, 0)
    torch.cuda.synchronize()
    assert torch.equal(o, ref)
    with pytest.raises(RuntimeError, match="C must be 1, 2, 4, or 8"):
        ext.grid_encode_forward(x, table, off, o, B, D, 3, L, S, 16, None, 0, False, 0)
    # the module through the extension
    torch.manual_seed(0)
    enc = GridEncoder(input_dim=3, num_levels=8, level_dim=2, base_resolution=16, desired_resolution=2048, log2_hashmap_size=11).cuda()
    with torch.no_grad():
        enc.embeddings.uniform_(-1, 1)
    xin = (x * 2 - 1).requires_grad_(False)
    res = []
    for use_native in (False, True):
        native.use(use_native)
        try:
            enc.embeddings.grad = None
            y = enc(xin, bound=1.0)
            (y * y).sum().backward()
            res.append((y.detach().clone(), enc.embeddings.grad.clone()))
        finally:
            native.use(False)
    assert torch.equal(res[0][0], res[1][0])
    assert float((res[0][1] - res[1][1]).abs().max()) <= 1e-5 * max(1.0, float(res[0][1].abs().max()))


def test_grid_forward_baseline_layout_quirk_levels():
    """L=16 / T=2^19: levels 12 and 13 fall back to wrapped 'dense' strides (uint32 overflow in
    gridencoder.cu:71-75); the device addressing must follow."""
    from ucnerf_amd.gridencoder import _backend
    pls, offsets, sizes, _ = grid_cpu.table_layout(16, 2, 16, 524288, 19)
    g = torch.Generator().manual_seed(0)
    table = torch.rand(int(offsets[-1]), 2, generator=g) * 2 - 1
    x = torch.rand(20000, 3, generator=g)
    want = torch.empty(16, len(x), 2)
    grid_cpu.grid_encode_forward(x, table, offsets, want, len(x), 3, 2, 16, 1.0, 16, None, 0, False, 0)
    got = torch.empty(16, len(x), 2, device="cuda")
    _backend.grid_encode_forward(dev(x), dev(table), dev(offsets), got, len(x), 3, 2, 16, 1.0, 16, None, 0, False, 0)
    assert torch.equal(got.cpu(), want)


def test_grid_backward_and_tv():
    from ucnerf_amd.gridencoder import _backend
    rng = np.random.default_rng(7)
    L, C, D = 8, 2, 3
    pls, offsets, sizes, _ = grid_cpu.table_layout(L, C, 16, 2048, 11)
    B = 4000
    x = torch.from_numpy(rng.random((B, D), dtype=np.float32))
    x[:50] = x[:50] * 3 - 1
    table = torch.from_numpy(rng.random((int(offsets[-1]), C), dtype=np.float32))
    grad = torch.from_numpy(rng.standard_normal((L, B, C)).astype(np.float32))
    S = np.log2(pls)
    _, jac = grid_cpu.encode(x, table, offsets, pls, 16, want_jacobian=True)
    want_g = torch.zeros_like(table)
    want_gi = torch.zeros(B, D)
    grid_cpu.grid_encode_backward(grad, x, table, offsets, want_g, B, D, C, L, S, 16, jac.contiguous(), want_gi, 0, False, 0)
    got_g = torch.zeros_like(table, device="cuda")
    got_gi = torch.zeros(B, D, device="cuda")
    _backend.grid_encode_backward(dev(grad), dev(x), dev(table), dev(offsets), got_g, B, D, C, L, S, 16, dev(jac), got_gi,
                                  0, False, 0)
    # atomics: same addends, different order -> a few ulp of the largest per-row sums
    assert H.maxdiff(got_g.cpu(), want_g) <= 2e-5 * float(want_g.abs().max())
    assert torch.equal(got_gi.cpu(), want_gi)          # sequential fmaf chain: exact
    wt = torch.zeros_like(table)
    grid_cpu.grad_total_variation(x, table, wt, offsets, 1e-2, B, D, C, L, S, 16, 0, False)
    gt = torch.zeros_like(table, device="cuda")
    _backend.grad_total_variation(dev(x), dev(table), gt, dev(offsets), 1e-2, B, D, C, L, S, 16, 0, False)
    assert H.maxdiff(gt.cpu(), wt) <= 1e-5 * float(wt.abs().max())


@pytest.mark.parametrize("D,C,gridtype,align,interp", [(3, 2, 1, False, 0), (3, 2, 0, True, 0), (3, 4, 1, True, 1),
                                                       (5, 2, 0, False, 0), (5, 1, 1, False, 1), (5, 8, 0, True, 0),
                                                       (2, 8, 1, True, 0), (4, 4, 0, True, 1)])
def test_grid_forward_tiled_aligned_5d_bitexact(D, C, gridtype, align, interp):
    """The dispatch axes the model itself never uses: gridtype 'tiled' (gridencoder.cu:78-82), align_corners
    (:70,:148), D = 5 (:381-385) -- forward, dy_dx and the sequential input gradient bit-exact, table gradient to
    atomic-order noise."""
    from ucnerf_amd.gridencoder import _backend
    rng = np.random.default_rng(500 + D * 10 + C + gridtype)
    L, T = 6, 11
    pls, offsets, sizes, _ = grid_cpu.table_layout(L, C, 16, 512, T, input_dim=D, align_corners=align)
    table = torch.from_numpy(rng.random((int(offsets[-1]), C), dtype=np.float32) * 2 - 1)
    B = 3000
    x = rng.random((B, D), dtype=np.float32)
    x[:4] = [[0.0] * D, [1.0] * D, [np.nextafter(np.float32(1), np.float32(2))] * D, [-1e-7] * D]
    k = rng.integers(1, 500, size=(64, D)).astype(np.float32)
    x[4:68] = (k - np.float32(0.0 if align else 0.5)) / np.float32(511.0)
    x[68:100] = rng.random((32, D), dtype=np.float32) * 3 - 1
    x = torch.from_numpy(x)
    S = np.log2(pls)
    want = torch.empty(L, B, C)
    wjac = torch.empty(B, L * D * C)
    grid_cpu.grid_encode_forward(x, table, offsets, want, B, D, C, L, S, 16, wjac, gridtype, align, interp)
    got = torch.empty(L, B, C, device="cuda")
    gjac = torch.empty(B, L * D * C, device="cuda")
    _backend.grid_encode_forward(dev(x), dev(table), dev(offsets), got, B, D, C, L, S, 16, gjac, gridtype, align, interp)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(gjac.cpu(), wjac)
    grad = torch.from_numpy(rng.standard_normal((L, B, C)).astype(np.float32))
    want_g, want_gi = torch.zeros_like(table), torch.zeros(B, D)
    grid_cpu.grid_encode_backward(grad, x, table, offsets, want_g, B, D, C, L, S, 16, wjac, want_gi, gridtype, align, interp)
    got_g, got_gi = torch.zeros_like(table, device="cuda"), torch.zeros(B, D, device="cuda")
    _backend.grid_encode_backward(dev(grad), dev(x), dev(table), dev(offsets), got_g, B, D, C, L, S, 16, gjac, got_gi,
                                  gridtype, align, interp)
    assert H.maxdiff(got_g.cpu(), want_g) <= 2e-5 * float(want_g.abs().max())
    assert torch.equal(got_gi.cpu(), want_gi)
    wt, gt = torch.zeros_like(table), torch.zeros_like(table, device="cuda")
    grid_cpu.grad_total_variation(x, table, wt, offsets, 1e-2, B, D, C, L, S, 16, gridtype, align)
    _backend.grad_total_variation(dev(x), dev(table), gt, dev(offsets), 1e-2, B, D, C, L, S, 16, gridtype, align)
    assert H.maxdiff(gt.cpu(), wt) <= 1e-5 * float(wt.abs().max())


@pytest.mark.parametrize("D,C,gridtype,align,interp", [(3, 2, 0, False, 0), (3, 4, 0, False, 1), (3, 8, 1, True, 0),
                                                       (2, 2, 0, False, 0), (5, 2, 0, False, 0), (3, 1, 0, False, 0)])
def test_grid_half_tables_vs_oracle(D, C, gridtype, align, interp):
    """scalar_t = at::Half (what grid.py:43-44 selects under autocast when C is even; C = 1 through the raw op):
    forward, dy_dx and the input gradient bit-exact against oracle/grid_oracle.c's half path (whose roundings are
    pinned to the c10::Half header), table gradient to the order noise of half atomics."""
    from ucnerf_amd.gridencoder import _backend
    rng = np.random.default_rng(600 + D * 10 + C)
    L, T = 7, 11
    pls, offsets, sizes, _ = grid_cpu.table_layout(L, C, 16, 1024, T, input_dim=D, align_corners=align)
    table = torch.from_numpy((rng.random((int(offsets[-1]), C), dtype=np.float32) * 2 - 1).astype(np.float16))
    B = 2000
    x = rng.random((B, D), dtype=np.float32)
    x[:4] = [[0.0] * D, [1.0] * D, [np.nextafter(np.float32(1), np.float32(2))] * D, [-1e-7] * D]
    x[4:36] = rng.random((32, D), dtype=np.float32) * 3 - 1
    x = torch.from_numpy(x)
    S = np.log2(pls)
    want = torch.empty(L, B, C, dtype=torch.float16)
    wjac = torch.empty(B, L * D * C, dtype=torch.float16)
    grid_cpu.grid_encode_forward_half(x, table, offsets, want, B, D, C, L, S, 16, wjac, gridtype, align, interp)
    got = torch.empty(L, B, C, device="cuda", dtype=torch.float16)
    gjac = torch.empty(B, L * D * C, device="cuda", dtype=torch.float16)
    _backend.grid_encode_forward(dev(x), dev(table), dev(offsets), got, B, D, C, L, S, 16, gjac, gridtype, align, interp)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(gjac.cpu().view(torch.int16), wjac.view(torch.int16))
    grad = torch.from_numpy((rng.standard_normal((L, B, C)) * 0.05).astype(np.float16))
    want_g = torch.zeros(int(offsets[-1]), C, dtype=torch.float16)
    want_gi = torch.zeros(B, D, dtype=torch.float16)
    grid_cpu.grid_encode_backward_half(grad, x, offsets, want_g, B, D, C, L, S, 16, wjac, want_gi, gridtype, align, interp)
    got_g = torch.zeros(int(offsets[-1]), C, device="cuda", dtype=torch.float16)
    got_gi = torch.zeros(B, D, device="cuda", dtype=torch.float16)
    _backend.grid_encode_backward(dev(grad), dev(x), dev(table), dev(offsets), got_g, B, D, C, L, S, 16, gjac, got_gi,
                                  gridtype, align, interp)
    assert torch.equal(got_gi.cpu().view(torch.int16), want_gi.view(torch.int16))
    # half atomics: every partial sum is rounded to half, the order differs -> a few half ulps of the row sums
    scale = float(want_g.float().abs().max())
    assert scale > 0 and H.maxdiff(got_g.cpu().float(), want_g.float()) <= 8 * 2 ** -10 * scale


def test_grid_module_under_autocast_reads_half_tables():
    """grid.py:43-44: under autocast the module's fp32 parameter is cast to half per call; output dtype half."""
    from ucnerf_amd.gridencoder import GridEncoder
    enc = GridEncoder(num_levels=8, level_dim=2, desired_resolution=2048, log2_hashmap_size=11).cuda()
    enc.embeddings.data.uniform_(-1, 1)
    x = (torch.rand(500, 3, device="cuda") * 2 - 1)
    with torch.autocast("cuda", dtype=torch.float16):
        out = enc(x)
    assert out.dtype == torch.float16
    pls, offsets, _, _ = grid_cpu.table_layout(8, 2, 16, 2048, 11)
    want = torch.empty(8, 500, 2, dtype=torch.float16)
    grid_cpu.grid_encode_forward_half(((x.cpu() + 1) / 2).contiguous(), enc.embeddings.detach().cpu().half(), offsets, want,
                                      500, 3, 2, 8, np.log2(pls), 16, None, 0, False, 0)
    assert torch.equal(out.cpu().view(torch.int16), want.permute(1, 0, 2).reshape(500, 16).contiguous().view(torch.int16))
    out.float().sum().backward()
    assert enc.embeddings.grad is not None and enc.embeddings.grad.dtype == torch.float32


def test_grid_module_autograd_and_errors():
    from ucnerf_amd.gridencoder import GridEncoder, _backend
    enc = GridEncoder(num_levels=8, level_dim=2, desired_resolution=2048, log2_hashmap_size=11).cuda()
    enc.embeddings.data.uniform_(-1, 1)
    x = (torch.rand(300, 3, device="cuda") * 2 - 1)
    out = enc(x)
    out.sum().backward()
    pls, offsets, _, _ = grid_cpu.table_layout(8, 2, 16, 2048, 11)
    want = grid_cpu.encode((x.cpu() + 1) / 2, enc.embeddings.detach().cpu(), offsets, pls, 16)
    assert torch.equal(out.detach().cpu(), want)
    assert enc.embeddings.grad is not None and float(enc.embeddings.grad.abs().sum()) > 0
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _backend.grid_encode_forward(x.cpu(), enc.embeddings.data, enc.offsets, out.detach(), 300, 3, 2, 8, 1.0, 16, None, 0, False, 0)
    with pytest.raises(RuntimeError, match="C must be 1, 2, 4, or 8"):
        bad = torch.zeros(int(offsets[-1]), 3, device="cuda")
        _backend.grid_encode_forward(x.contiguous(), bad, enc.offsets, torch.empty(8, 300, 3, device="cuda"), 300, 3, 3, 8,
                                     1.0, 16, None, 0, False, 0)


# ------------------------------------------------------------------ a3 / a4: resampling
def _resample(lib, sd_prev, w_prev, dilation, anneal, S, jitter=None):
    from ucnerf_amd import _lib
    from ucnerf_amd.internal.models import _u_table
    N = sd_prev.shape[0] if sd_prev is not None else jitter.shape[0]
    u, mj = _u_table(S, jitter is not None, torch.device("cuda"))
    out = torch.empty(N, S + 1, device="cuda")
    n_prev = 0 if sd_prev is None else w_prev.shape[1]
    _lib.check(lib.ucn_resample(_lib.ptr(sd_prev), _lib.ptr(w_prev), n_prev, dilation, anneal, 0.0, u.data_ptr(),
                                _lib.ptr(jitter), 0 if jitter is None else jitter.shape[1], mj, N, S, out.data_ptr(),
                                _lib.stream()))
    return out.cpu()


def test_resample_vs_golden():
    from ucnerf_amd import _lib
    lib = _lib.load()
    fx = H.load("stepfun.npz")
    t, w, dil = dev(fx["t"]), dev(fx["w"]), float(fx["dilation"])
    knots = fx["t_dilate"][..., 1:-1]

    def close(got, want, logits):
        # Inverse-CDF sampling amplifies a 1-ulp difference in the CDF (summation order, exp/log
        # rounding) by width/weight of the bin it lands in -- unbounded for near-empty bins.  The
        # well-posed comparison is in CDF space: both sample sets must sit at the same quantiles.
        # (and, conversely, a dense bin turns a sub-ulp t difference into a visible quantile
        # difference), so every fencepost must agree EITHER in t OR in quantile to 2e-6.
        cdf = rm.cdf_of_weights(torch.softmax(logits, dim=-1))
        q_got, q_want = rm.interp_sorted(got, knots, cdf), rm.interp_sorted(want, knots, cdf)
        ok = ((got - want).abs() <= 2e-6) | ((q_got - q_want).abs() <= 2e-6)
        assert ok.all(), (float((got - want).abs()[~ok].max()), float((q_got - q_want).abs()[~ok].max()))
        assert H.maxdiff(got, want) <= 1e-4           # and still tight in t on this fixture
        assert (got[:, 1:] >= got[:, :-1]).all()

    for frac in ("1.0", "0.25"):
        f = float(frac)
        got = _resample(lib, t, w, dil, 10 * f / (9 * f + 1), 128)
        close(got, fx[f"sample_eval_{frac}"], fx[f"logits_{frac}"])
    got = _resample(lib, t, w, dil, 10 * 0.25 / (9 * 0.25 + 1), 32, jitter=dev(fx["sample_train_jitter"]))
    close(got, fx["sample_train"], fx["logits_0.25"])
    N = fx["t"].shape[0]
    from ucnerf_amd.internal.models import _u_table
    u, _ = _u_table(64, False, torch.device("cuda"))
    out = torch.empty(N, 65, device="cuda")
    _lib.check(lib.ucn_resample(None, None, 0, 0.5, 1.0, 0.0, u.data_ptr(), None, 0, 0.0, N, 64, out.data_ptr(), _lib.stream()))
    assert H.maxdiff(out.cpu(), fx["sample_level0"]) <= 2e-6


# ------------------------------------------------------------------ a10 / a11: compositing
def test_composite_vs_golden():
    from ucnerf_amd import _lib
    lib = _lib.load()
    fx = H.load("composite.npz")
    N, S = fx["density"].shape
    # the kernel takes normalised fenceposts + near/far; tdist = s*far + (1-s)*near with near=0, far=8
    sd = dev(fx["tdist"] / 8.0)
    near, far = torch.zeros(N, device="cuda"), torch.full((N,), 8.0, device="cuda")
    w = torch.empty(N, S, device="cuda"); main = torch.empty(N, 5, device="cuda"); ex = torch.empty(N, 4, device="cuda")
    dens, cols, dirs = dev(fx["density"]), dev(fx["rgbs"]), dev(fx["dirs"])     # keep alive across the launch
    for opaque, key in ((0, "weights"), (1, "weights_opaque")):
        _lib.check(lib.ucn_composite(dens.data_ptr(), cols.data_ptr(), sd.data_ptr(), near.data_ptr(),
                                     far.data_ptr(), dirs.data_ptr(), 1.0, opaque, N, S, w.data_ptr(), main.data_ptr(),
                                     ex.data_ptr(), _lib.stream()))
        torch.cuda.synchronize()
        assert H.maxdiff(w.cpu(), fx[key]) <= 5e-6
        if opaque:
            continue
        m, e = main.cpu(), ex.cpu()
        assert H.maxdiff(m[:, :3], fx["out_rgb"]) <= 1e-5
        assert H.maxdiff(m[:, 4], fx["out_acc"]) <= 1e-5
        sentinel = fx["out_depth"] == 300
        assert torch.equal(m[:, 3] == 300, sentinel) or H.maxdiff(m[:, 4], fx["out_acc"]) <= 1e-6
        assert H.maxdiff(m[:, 3][~sentinel], fx["out_depth"][~sentinel]) <= 5e-5
        assert H.maxdiff(e[:, 0], fx["out_distance_mean"]) <= 5e-5
        for i, k in enumerate(("distance_percentile_5", "distance_median", "distance_percentile_95")):
            assert H.maxdiff(e[:, 1 + i], fx["out_" + k]) <= 2e-4, k      # t up to 8.5, 1/(cdf slope) amplification


# ------------------------------------------------------------------ a5-a9: field on explicit Gaussians
def test_field_vs_golden():
    fx = H.load("field.npz")
    spec = rm.make_spec("tiny")
    sd = H.state_for(fx, spec)
    model, _ = H.hip_model(spec, sd)
    means, stds, vd = dev(fx["means"]), dev(fx["stds"]), dev(fx["viewdirs"])
    # Per-SAMPLE tolerances follow the conditioning of the function, not the kernel: a 1-ulp change of
    # a contracted coordinate (torch-CPU's vectorised sqrt is itself not correctly rounded; pow/erf
    # differ by an ulp between libraries) moves a level-15 (res 524288) lookup by ~0.03 cell, i.e.
    # O(1e-2) in that level's feature before erf damping.  The 6-level PropMLP grid (res <= 512) has
    # no such amplification and is held to 1e-6.  See DESIGN.md "Parity analysis".
    # (bracketed by the reference's own float64 error in test_bracket_gpu.py::test_field_golden_bracket: 2.2e-4 / 1.0e-4 / 1.9e-3)
    tol = dict(nerf=dict(density=1e-3, rgb=3e-4), prop=dict(density=1e-6, rgb=0.0))
    for name, mlp in (("nerf", model.nerf_mlp), ("prop", model.prop_mlp_0)):
        res = mlp(False, means, stds, viewdirs=vd)
        assert H.maxdiff(res["density"].cpu(), fx[f"{name}_density"]) <= tol[name]["density"]
        assert H.maxdiff(res["coord"].cpu(), fx[f"{name}_coord"]) <= 1e-6
        assert H.maxdiff(res["rgb"].cpu(), fx[f"{name}_rgb"]) <= tol[name]["rgb"]
        assert float((res["density"].cpu() - fx[f"{name}_density"]).abs().mean()) <= 2e-5
    raw, x, coord = model.nerf_mlp.predict_density(means, stds)
    assert H.maxdiff(raw.cpu(), fx["nerf_raw_density"]) <= 3e-3
    assert H.maxdiff(x.cpu(), fx["nerf_bottleneck"]) <= 5e-3
    assert float((x.cpu() - fx["nerf_bottleneck"]).abs().mean()) <= 5e-5
    pm, ps = dev(fx["nowarp_means"]), dev(fx["nowarp_stds"])
    raw, _, _ = model.nerf_mlp.predict_density(pm, ps, no_warp=True)
    # no contraction -> coordinates are exact IEEE arithmetic -> only erf/MLP rounding remains
    assert H.maxdiff(raw.cpu(), fx["nowarp_raw_density"]) <= 2e-5


# ------------------------------------------------------------------ a1: Model.forward end to end
@pytest.mark.parametrize("name,kind,over", [
    ("model_tiny.npz", "tiny", {}),
    ("model_tinyR.npz", "tinyR", {}),
    ("model_tiny64.npz", "tiny64", {}),                       # BASELINE configs[0] architecture: 64-wide colour MLP
    ("model_sky.npz", "tiny", dict(model_sky=True, brightness_correction=True)),
    ("model_train.npz", "tiny", {}),
    ("model_nodilate.npz", "tiny", dict(dilation_bias=0., dilation_multiplier=0.)),   # models.py:167 use_dilation False
])
def test_model_forward_vs_golden(name, kind, over):
    fx = H.load(name)
    spec = rm.make_spec(kind, **over)
    sd = H.state_for(fx, spec)
    model, cfg = H.hip_model(spec, sd)
    train = "noise0_jitter" in fx
    noise = H.noise_of(fx, spec.num_levels)
    batch = H.pin_noise(H.to_dev(H.batch_of(fx)), noise)
    cam = fx.get("eval_camidx")
    with torch.no_grad():
        rend, hist = model(train, batch, float(fx["train_frac"]), not train, zero_glo=not train,
                       eval_camidx=None if cam is None else cam.cuda())
    torch.cuda.synchronize()
    # Level 0 (proposal grid, res <= 512) is well conditioned: everything agrees to a few ulp.
    # The last level of the L=16 configs is not (per-sample noise from 1-ulp coordinate changes, see
    # test_field_vs_golden / DESIGN.md); there the per-SAMPLE bars are loose and the per-PIXEL bars
    # (what north_star specifies) carry the parity claim.  tinyR (res <= 8192) sits in between.
    fine = kind in ("tiny", "tiny64")
    for lvl in range(spec.num_levels):
        g = lambda k: fx[f"L{lvl}_{k}"]
        r = rend[lvl]
        last = lvl == spec.num_levels - 1
        samp = (1e-2 if fine else 2e-4) if last else 2e-6          # per-sample density / colour
        # (1e-2 is 1-2 decades looser than 2 x the float32 reference's own float64 error on these specs:
        # test_bracket_gpu.py::test_fine_level_features_density_colour_bracket holds that, per level and per sample)
        assert H.maxdiff(hist[lvl]["sdist"].cpu(), g("hist_sdist").reshape(hist[lvl]["sdist"].shape)) <= (5e-5 if last else 0.0), lvl
        assert H.maxdiff(hist[lvl]["density"].cpu().reshape(-1), g("hist_density").reshape(-1)) <= samp, lvl
        assert H.maxdiff(r["weights"].cpu().reshape(-1), g("weights").reshape(-1)) <= (2e-4 if last else 5e-7), lvl
        assert H.maxdiff(r["rgb"].cpu().reshape(-1), g("rgb").reshape(-1)) <= H.RGB_TOL, lvl      # the headline bar
        assert float((r["rgb"].cpu().reshape(-1) - g("rgb").reshape(-1)).abs().mean()) <= 2e-5, lvl
        assert H.maxdiff(r["acc"].cpu().reshape(-1), g("acc").reshape(-1)) <= 1e-4, lvl
        if last:
            assert H.maxdiff(hist[lvl]["rgb"].cpu().reshape(-1), g("hist_rgb").reshape(-1)) <= samp
            assert H.maxdiff(hist[lvl]["coord"].cpu().reshape(-1), g("hist_coord").reshape(-1)) <= 5e-6
        want_d = g("depth").reshape(-1)
        got_d = r["depth"].cpu().reshape(-1)
        stable = (g("acc").reshape(-1) - 0.6).abs() > 1e-3                 # away from the 0.6 sentinel switch
        assert H.maxdiff(got_d[stable], want_d[stable]) <= 1e-3, lvl
        if not train:
            for k in ("distance_mean", "distance_median", "distance_percentile_5", "distance_percentile_95"):
                assert H.maxdiff(r[k].cpu().reshape(-1), g(k).reshape(-1)) <= 2e-3, (lvl, k)
            assert H.maxdiff(r["ray_sdist"].cpu(), g("ray_sdist")) <= 5e-5
            assert H.maxdiff(r["ray_rgbs"].cpu(), g("ray_rgbs")) <= (samp if last else 1e-4)
        if "sky_rgbs" in r:
            assert H.maxdiff(r["sky_rgbs"].cpu(), g("sky_rgbs")) <= 5e-5
            assert H.maxdiff(r["affine_trans"].cpu(), g("affine_trans")) <= 1e-5
            assert H.maxdiff(r["affine_trans_sky"].cpu(), g("affine_trans_sky")) <= 1e-5


def test_model_forward_vs_oracle_larger_batch_and_chunks():
    """2000 rays through 3 internal passes (ragged last pass) against the CPU oracle."""
    spec = rm.make_spec("tiny")
    sd = rm.init_state(spec, seed=9)
    n = 2000
    rays = rm.synthetic_rays(n, seed=10)
    noise = [rm.draw_level_noise(spec, n, l, False, torch.Generator().manual_seed(11 + l)) for l in range(2)]
    with torch.no_grad():
        want, _ = rm.model_forward(spec, sd, rays, noise)
    model, _ = H.hip_model(spec, sd, max_chunk_rays=768)
    torch.set_grad_enabled(False)                          # the fused (inference) march
    got, _ = model(False, H.pin_noise(H.to_dev(rays), noise), 1.0, True)
    assert H.maxdiff(got[-1]["rgb"].cpu(), want[-1]["rgb"]) <= H.RGB_TOL
    assert float((got[-1]["rgb"].cpu() - want[-1]["rgb"]).abs().mean()) <= 1e-5
    assert H.maxdiff(got[-1]["acc"].cpu(), want[-1]["acc"]) <= 1e-4
    assert H.maxdiff(got[0]["rgb"].cpu(), want[0]["rgb"]) <= 2e-6         # proposal level: well conditioned
    for lpb in (4, 16):                                   # level grouping is a pure scheduling knob
        model.levels_per_block = lpb
        again, _ = model(False, H.pin_noise(H.to_dev(rays), noise), 1.0, True)
        assert torch.equal(again[-1]["rgb"], got[-1]["rgb"])
    model.rays_fastest = not model.rays_fastest           # thread<->sample mapping: also pure scheduling
    again, _ = model(False, H.pin_noise(H.to_dev(rays), noise), 1.0, True)
    assert torch.equal(again[-1]["rgb"], got[-1]["rgb"]) and torch.equal(again[-1]["weights"], got[-1]["weights"])
    torch.set_grad_enabled(True)


def test_mlp_modes_agree():
    """mlp_mode 0 (exact fp32 products on the fp32-input MFMA, the reference's layer-by-layer form) against
    mlp_mode 1 (split-f16 MFMA + composed colour layers, the default): same pixels to a few fp32 ulps, and both
    against the CPU oracle."""
    spec = rm.make_spec("tiny")
    sd = rm.init_state(spec, seed=31)
    n = 600
    rays = rm.synthetic_rays(n, seed=32)
    noise = [rm.draw_level_noise(spec, n, l, False, torch.Generator().manual_seed(33 + l)) for l in range(2)]
    with torch.no_grad():
        want, _ = rm.model_forward(spec, sd, rays, noise)
    model, _ = H.hip_model(spec, sd)
    torch.set_grad_enabled(False)
    out = {}
    for mode in (0, 1):
        model.nerf_mlp.mlp_mode = mode
        got, hist = model(False, H.pin_noise(H.to_dev(rays), noise), 1.0, True)
        out[mode] = (got[-1]["rgb"].cpu(), hist[-1]["density"].cpu())
        assert H.maxdiff(out[mode][0], want[-1]["rgb"]) <= H.RGB_TOL
    torch.set_grad_enabled(True)
    assert H.maxdiff(out[0][0], out[1][0]) <= 2e-6                      # pixels
    rel = (out[0][1] - out[1][1]).abs() / (out[0][1].abs() + 1e-3)
    assert float(rel.max()) <= 2e-5                                     # per-sample densities


@pytest.mark.parametrize("case", ["fresh_init", "big_table", "big_first_layer", "big_everything"])
def test_split_f16_range(case):
    """mlp_mode 1 carries every layer at a power-of-two scale chosen at pack time (field_mlp_h.hip, comment 5): f16
    operands must neither overflow (|v| > 65504 -> inf) nor lose their low halves to the subnormal range, whatever the
    magnitudes of the table and the weights.  Reference = mlp_mode 0 (exact fp32 products, itself pinned to the CPU
    oracle by the tests above) on the same points.  Without the scales `big_first_layer` overflows h0 (|h0| ~ 1e6) and
    `fresh_init` (|features| ~ 1e-4: the reference's own initialisation, grid.py:151-153) loses ~3e-4 relative."""
    spec = rm.make_spec("tiny")
    sd = rm.init_state(spec, seed=41)
    g = torch.Generator().manual_seed(42)
    if case == "fresh_init":
        sd["nerf_mlp.encoder.embeddings"] = sd["nerf_mlp.encoder.embeddings"] * 1e-4
    elif case == "big_table":
        sd["nerf_mlp.encoder.embeddings"] = sd["nerf_mlp.encoder.embeddings"] * 1e3
    elif case == "big_first_layer":
        sd["nerf_mlp.density_layer.0.weight"] = sd["nerf_mlp.density_layer.0.weight"] * 1e6
        sd["nerf_mlp.density_layer.2.weight"] = sd["nerf_mlp.density_layer.2.weight"] * 1e-6
    elif case == "big_everything":
        for k in list(sd):
            if k.startswith("nerf_mlp.") and k.endswith("weight") and "rgb_layer" not in k:
                sd[k] = sd[k] * 30.0
        sd["nerf_mlp.encoder.embeddings"] = sd["nerf_mlp.encoder.embeddings"] * 1e2
    model, _ = H.hip_model(spec, sd)
    mlp = model.nerf_mlp
    n, S = 64, 32
    means = (torch.rand(n, S, 6, 3, generator=g) * 2 - 1) * 1.5
    stds = torch.rand(n, S, 6, generator=g) * 1e-3
    vd = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    out = {}
    with torch.no_grad():
        for mode in (0, 1):
            mlp.mlp_mode = mode
            r = mlp(False, means.cuda(), stds.cuda(), viewdirs=vd.cuda()[:, None, :])
            out[mode] = (r["density"].cpu().double(), r["rgb"].cpu().double())
    d0, d1 = out[0][0], out[1][0]
    assert torch.isfinite(d1).all() and torch.isfinite(out[1][1]).all(), "f16 operand overflow"
    assert float(d0.abs().max()) > 0
    # Truth: the dense layers in float64 on the oracle's (fp32) features.  At these magnitudes fp32 itself is
    # ill-conditioned (logits of 1e5 carry 1e-2 of rounding), so "fp32-class" is stated as: the split-f16 kernel is as
    # close to the float64 evaluation as the exact-fp32-product kernel is, up to a factor and a floor of fp32 ulps.
    fs = spec.nerf
    with torch.no_grad():
        _, _, _, feat = rm.field_density_features(fs, sd, means, stds)
        W = lambda k: sd["nerf_mlp." + k].double()
        h0 = torch.relu(feat.double() @ W("density_layer.0.weight").T + W("density_layer.0.bias"))
        x = h0 @ W("density_layer.2.weight").T + W("density_layer.2.bias")
        t_d = torch.nn.functional.softplus(x[..., 0] + fs.density_bias)
        enc = rm.view_encoding(vd, fs.deg_view).double()[:, None, :].expand(n, S, 27)
        skip = torch.cat([x, enc], dim=-1)
        h1 = torch.relu(skip @ W("lin_second_stage_0.weight").T + W("lin_second_stage_0.bias"))
        h2 = torch.relu(torch.cat([h1, skip], dim=-1) @ W("lin_second_stage_1.weight").T + W("lin_second_stage_1.bias"))
        t_rgb = torch.sigmoid(h2 @ W("rgb_layer.weight").T + W("rgb_layer.bias")) * (1 + 2 * fs.rgb_padding) - fs.rgb_padding
    e0_d = float(((d0 - t_d).abs() / (t_d.abs() + 1e-3 * float(t_d.abs().max()) + 1e-9)).max())
    e1_d = float(((d1 - t_d).abs() / (t_d.abs() + 1e-3 * float(t_d.abs().max()) + 1e-9)).max())
    e0_c, e1_c = H.maxdiff(out[0][1], t_rgb), H.maxdiff(out[1][1], t_rgb)
    assert e1_d <= 3 * e0_d + 2e-6, (case, e1_d, e0_d)
    assert e1_c <= 3 * e0_c + 2e-6, (case, e1_c, e0_c)
    if case == "fresh_init":                     # well conditioned: absolute bars too
        assert e1_d <= 5e-6 and e1_c <= 5e-6, (e1_d, e1_c)


def test_config0_workload_400x400_frame():
    """BASELINE.json configs[0]: one 400 x 400 frame, random-init L16 / C2 / T = 2^19 hash grid + "2 x 64" colour MLP
    (bottleneck_width = net_width_viewdirs = 64), 64 samples per level -- the reference's CPU-runnable case, here
    through render_image.  The whole frame is rendered on the GPU; 2048 of its rays (what the CPU oracle finishes in
    seconds) are compared with the oracle given the same random cone bases, both kernel arithmetic modes."""
    from ucnerf_amd.internal import camera_utils, models
    spec = rm.make_spec("cfg1")
    sd = rm.init_state(spec, seed=91)
    model, cfg = H.hip_model(spec, sd)
    Hh = Ww = 400
    K = np.array([[500.0, 0.0, Ww / 2], [0.0, 500.0, Hh / 2], [0.0, 0.0, 1.0]])
    c2w = np.concatenate([np.eye(3), np.array([[0.05], [0.02], [0.1]])], axis=1)
    batch = camera_utils.generate_ray_batch((np.linalg.inv(K)[None], c2w[None], None, None), 0, Ww, Hh, 0.0, 8.0, device="cuda")
    batch = {k: batch[k] for k in ("origins", "directions", "viewdirs", "cam_dirs", "radii", "near", "far")}
    n = Hh * Ww
    g = torch.Generator().manual_seed(92)
    rand_vec = torch.randn(n, 6, generator=g)
    batch["rand_vec"] = rand_vec.reshape(Hh, Ww, 6).cuda()

    class One:
        num_processes, process_index, is_main_process = 1, 0, True
    pick = torch.randperm(n, generator=g)[:2048]
    flat = {k: v.reshape(n, -1)[pick.cuda()].cpu() for k, v in batch.items() if k != "rand_vec"}
    noise = [rm.LevelNoise(rand_vec=rand_vec[pick, 3 * l:3 * l + 3]) for l in range(2)]
    with torch.no_grad():
        want, _ = rm.model_forward(spec, sd, flat, noise)
    for mode in (1, 0):
        model.nerf_mlp.mlp_mode = mode
        out = models.render_image(model, One(), batch, False, 1.0, cfg, verbose=False)
        assert out["rgb"].shape == (Hh, Ww, 3) and out["weights"].shape == (Hh, Ww, 64)
        assert torch.isfinite(out["rgb"]).all()
        got = out["rgb"].reshape(n, 3)[pick.cuda()].cpu()
        assert H.maxdiff(got, want[-1]["rgb"]) <= H.RGB_TOL, mode
        assert H.maxdiff(out["acc"].reshape(n)[pick.cuda()].cpu(), want[-1]["acc"]) <= 1e-4, mode


def test_model_forward_empty_single_and_ragged_batches():
    """0 rays (empty tensors through every entry point), 1 ray, and a batch that is not a multiple of any tile
    size (partial wave, partial workgroup, ragged last pass) against the CPU oracle."""
    spec = rm.make_spec("tiny")
    sd = rm.init_state(spec, seed=21)
    model, _ = H.hip_model(spec, sd, max_chunk_rays=40)
    torch.set_grad_enabled(False)
    for n in (0, 1, 131):
        rays = rm.synthetic_rays(max(n, 1), seed=22)
        rays = {k: v[:n] for k, v in rays.items()}
        noise = [rm.draw_level_noise(spec, max(n, 1), l, False, torch.Generator().manual_seed(23 + l)) for l in range(2)]
        for nz in noise:
            nz.rand_vec = nz.rand_vec[:n]
        got, hist = model(False, H.pin_noise(H.to_dev(rays), noise), 1.0, True)
        assert got[-1]["rgb"].shape == (n, 3) and hist[-1]["sdist"].shape[0] == n
        if n:
            want, _ = rm.model_forward(spec, sd, rays, noise)
            assert H.maxdiff(got[-1]["rgb"].cpu(), want[-1]["rgb"]) <= H.RGB_TOL
            assert H.maxdiff(got[-1]["acc"].cpu(), want[-1]["acc"]) <= 1e-4
    torch.set_grad_enabled(True)


def test_features_backward_algorithms_agree():
    """Table gradient of the fused featurisation: row-block ownership (no global atomics) == atomic scatter,
    in both gradient layouts; the atomic scatter itself is pinned to the reference's training step by
    test_train_step.py."""
    from ucnerf_amd import _lib
    lib = _lib.load()
    spec = rm.make_spec("tiny")
    sd = rm.init_state(spec, seed=3)
    n = 700
    rays = rm.synthetic_rays(n, seed=4)
    noise = [rm.draw_level_noise(spec, n, l, False, torch.Generator().manual_seed(5 + l)) for l in range(2)]
    model, _ = H.hip_model(spec, sd)
    with torch.no_grad():
        _, hist = model(False, H.pin_noise(H.to_dev(rays), noise), 1.0, True)
    mlp = model.nerf_mlp
    enc = mlp.encoder
    sdist = hist[-1]["sdist"].contiguous()
    S = sdist.shape[-1] - 1
    b = H.to_dev(rays)
    flat = {k: b[k].reshape(n, -1).contiguous() for k in ("origins", "directions", "cam_dirs", "radii", "near", "far")}
    basis = torch.empty(n, 6, device="cuda")
    rvec = noise[-1].rand_vec.cuda().contiguous()
    st = _lib.stream()
    _lib.check(lib.ucn_cone_basis(flat["cam_dirs"].data_ptr(), rvec.data_ptr(), n, basis.data_ptr(), st))
    L, C = enc.num_levels, enc.level_dim
    g0 = torch.randn(L, n * S, C, device="cuda")
    g0[:, ::7] = 0                                            # samples without gradient are skipped
    g1 = g0.permute(1, 0, 2).contiguous()                     # [N*S][L*C]

    ws = torch.empty(lib.ucn_march_features_backward_ws_floats(ctypes.byref(mlp.field()), n, S), device="cuda")
    assert ws.numel() >= 24 * n * S                          # geometry planes + block-mask planes

    def run(lpb, layout, g, work=None, out=None):
        out = torch.zeros_like(enc.embeddings) if out is None else out
        _lib.check(lib.ucn_march_features_backward(
            ctypes.byref(mlp.field()), sdist.data_ptr(), flat["near"].data_ptr(), flat["far"].data_ptr(),
            flat["origins"].data_ptr(), flat["directions"].data_ptr(), basis.data_ptr(), flat["radii"].data_ptr(), None, None,
            float(model.std_scale), n, S, lpb, layout, g.data_ptr(), out.data_ptr(), _lib.ptr(work), st))
        return out

    want = run(1, 0, g0)                                      # atomic scatter
    assert float(want.abs().max()) > 0
    tol = 2e-5 * float(want.abs().max())                      # same addends, different summation order
    g3 = g0.permute(0, 2, 1).contiguous()                     # [L*C][N*S]
    assert H.maxdiff(run(0, 0, g0, ws), want) <= tol          # compacted row blocks, level-major gradient
    assert H.maxdiff(run(0, 0, g0), want) <= tol              # row blocks, geometry re-derived per workgroup
    assert H.maxdiff(run(0, 1, g1, ws), want) <= tol          # compacted row blocks, sample-major gradient (autograd's)
    assert H.maxdiff(run(0, 1, g1), want) <= tol
    assert H.maxdiff(run(0, 3, g3, ws), want) <= tol          # compacted row blocks, feature-major gradient
    assert H.maxdiff(run(0, 3, g3), want) <= tol
    with pytest.raises(RuntimeError, match="layout 3"):
        run(1, 3, g3)
    assert H.maxdiff(run(4, 1, g1), want) <= tol
    twice = run(0, 0, g0, ws, run(0, 0, g0, ws))              # accumulates into grad_embeddings
    assert H.maxdiff(twice, 2 * want) <= 2 * tol
    # fixed-point row blocks (UCN_BWD_FIXED_POINT): resolution 2^-29 of a task's summed |g|, in every gradient layout
    tol_fx = 2e-4 * float(want.abs().max())
    for lay, gg in ((0, g0), (1, g1), (3, g3)):
        assert H.maxdiff(run(0, lay | _lib.BWD_FIXED_POINT, gg, ws), want) <= tol_fx, lay
    assert H.maxdiff(run(0, 1 | _lib.BWD_FIXED_POINT, g1), want) <= tol   # no workspace: the flag is ignored (float rows)


def test_render_image_vs_golden_and_invariants():
    from ucnerf_amd.internal import models
    fx = H.load("render_image.npz")
    spec = rm.make_spec("tiny")
    sd = H.state_for(fx, spec)
    model, cfg = H.hip_model(spec, sd)
    Hh, Ww = int(fx["H"]), int(fx["W"])
    batch = {k: v.reshape(Hh, Ww, -1).cuda() for k, v in H.batch_of(fx).items()}
    batch["rand_vec"] = torch.cat([fx[f"noise{l}_rand_vec"] for l in range(2)], dim=-1).reshape(Hh, Ww, -1).cuda()

    class OneProc:
        num_processes, process_index, is_main_process = 1, 0, True
    out = models.render_image(model, OneProc(), batch, False, 1.0, cfg, verbose=False)
    assert model.training            # render_image leaves the model in train mode (models.py:1006)
    for k in [k[4:] for k in fx if k.startswith("out_")]:
        tol = dict(rgb=H.RGB_TOL, acc=1e-4, weights=2e-4).get(k, 2e-3)
        want = fx["out_" + k]
        got = out[k].cpu()
        assert got.shape == want.shape, (k, got.shape, want.shape)
        if k == "depth":
            stable = (fx["out_acc"] - 0.6).abs() > 1e-3
            assert H.maxdiff(got[stable], want[stable]) <= 1e-3
        else:
            assert H.maxdiff(got, want) <= tol, k
    assert all(len(out[k]) == 2 and out[k][0].shape[0] == 16 for k in ("ray_sdist", "ray_weights", "ray_rgbs"))
    # size-independent properties at full resolution of the frame: weights are a sub-stochastic
    # partition of each ray, acc = sum(weights), rgb inside the padded sigmoid range + white background
    w = out["weights"]
    assert (w >= 0).all() and (w.sum(-1) <= 1 + 1e-5).all()
    assert H.maxdiff(w.sum(-1).cpu(), out["acc"].cpu()) <= 1e-5
    assert (out["rgb"] >= -0.001 - 1e-5).all() and (out["rgb"] <= 1.001 + 1e-5).all()
    # the marching order of the frame's rays (config.render_ray_tile: T x T pixel blocks per wave; the 16 x 24 frame has
    # ragged blocks for T = 5) is pure scheduling: every per-pixel output is bit-identical to the row-major march
    ref = dict(out)
    for T in (1, 5, 16):
        cfg.render_ray_tile = T
        again = models.render_image(model, OneProc(), batch, False, 1.0, cfg, verbose=False)
        for k in ("rgb", "depth", "acc", "weights", "distance_mean", "distance_median"):
            assert torch.equal(again[k], ref[k]), (T, k)
    cfg.render_ray_tile = 8


def test_product_raises_without_device_tensors():
    spec = rm.make_spec("tiny")
    model, _ = H.hip_model(spec, rm.init_state(spec, seed=1))
    rays = rm.synthetic_rays(8, seed=1)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        model(False, rays, 1.0, False)


@pytest.mark.parametrize("C,log2_T", [(1, 12), (4, 12), (8, 12), (2, 16)])
def test_features_backward_every_level_dim(C, log2_T):
    """The compacted / plain row-block backward for every channel count the reference's grid supports (1, 2, 4, 8:
    gridencoder.cu:376-399) and for a table with several row blocks per level, against the atomic scatter.  The sample
    geometry comes from the tiny model; the gradient target is a bare grid of the given level_dim."""
    from ucnerf_amd import _lib
    from ucnerf_amd.gridencoder import GridEncoder
    lib = _lib.load()
    spec = rm.make_spec("tiny")
    n = 500
    rays = rm.synthetic_rays(n, seed=14)
    noise = [rm.draw_level_noise(spec, n, l, False, torch.Generator().manual_seed(15 + l)) for l in range(2)]
    model, _ = H.hip_model(spec, rm.init_state(spec, seed=13))
    with torch.no_grad():
        _, hist = model(False, H.pin_noise(H.to_dev(rays), noise), 1.0, True)
    sdist = hist[-1]["sdist"].contiguous()
    S = sdist.shape[-1] - 1
    b = H.to_dev(rays)
    flat = {k: b[k].reshape(n, -1).contiguous() for k in ("origins", "directions", "cam_dirs", "radii", "near", "far")}
    basis = torch.empty(n, 6, device="cuda")
    st = _lib.stream()
    _lib.check(lib.ucn_cone_basis(flat["cam_dirs"].data_ptr(), noise[-1].rand_vec.cuda().contiguous().data_ptr(), n,
                                  basis.data_ptr(), st))
    enc = GridEncoder(num_levels=16, level_dim=C, desired_resolution=524288, log2_hashmap_size=log2_T).cuda()
    d = _lib.UcnField()
    d.embeddings = enc.embeddings.data_ptr()
    d.offsets_host, d.grid_sizes_host = enc._offsets_np.ctypes.data, enc._sizes_np.ctypes.data
    d.num_levels, d.level_dim, d.base_resolution = 16, C, 16
    d.log2_per_level_scale = float(np.log2(enc.per_level_scale))
    L = 16
    g0 = torch.randn(L, n * S, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(C))
    g0[:, ::5] = 0
    ws = torch.empty(lib.ucn_march_features_backward_ws_floats(ctypes.byref(d), n, S), device="cuda")

    def run(lpb, g, work=None):
        out = torch.zeros_like(enc.embeddings)
        _lib.check(lib.ucn_march_features_backward(
            ctypes.byref(d), sdist.data_ptr(), flat["near"].data_ptr(), flat["far"].data_ptr(), flat["origins"].data_ptr(),
            flat["directions"].data_ptr(), basis.data_ptr(), flat["radii"].data_ptr(), None, None, float(model.std_scale),
            n, S, lpb, 0, g.data_ptr(), out.data_ptr(), _lib.ptr(work), st))
        return out

    want = run(1, g0)
    tol = 2e-5 * float(want.abs().max())
    assert float(want.abs().max()) > 0
    assert H.maxdiff(run(0, g0, ws), want) <= tol
    assert H.maxdiff(run(0, g0), want) <= tol


@pytest.mark.parametrize("n_prev,S,dil,per_sample_jitter", [(200, 300, 0.004, False), (256, 512, 0.05, True), (7, 33, 0.3, False),
                                                            (64, 128, 0.0103, True)])
def test_resample_vs_oracle_at_the_size_limits(n_prev, S, dil, per_sample_jitter):
    """k_resample (one wave per ray, dynamic LDS) against the oracle's dilate -> trim -> anneal -> sample chain
    (models.py:168-191, stepfun.py:75-105,251-294) beyond the golden's 64 -> 128: the maximum interval count, wide
    dilation windows (hundreds of intervals under one knot), zero-width and zero-weight intervals, per-sample jitter.

    On such spiky histograms the chain is ill-conditioned: its float32 evaluation (the reference) is itself up to 2e-4
    in t away from the float64 evaluation of the same formulas.  The bar is therefore: every fencepost agrees with the
    float32 oracle in t or in quantile, OR the kernel is as close to the float64 truth as the float32 oracle is."""
    from ucnerf_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(n_prev + S)
    N = 203                                                       # not a multiple of the 4 rays per workgroup
    t = torch.sort(torch.rand(N, n_prev + 1, generator=g), dim=-1).values
    t[:, 0], t[:, -1] = 0.0, 1.0
    t[::5, 3] = t[::5, 2]                                         # zero-width intervals
    w = torch.rand(N, n_prev, generator=g) ** 6
    w[::3, n_prev // 2:] = 0.0                                    # dead tails
    w = w / w.sum(-1, keepdim=True)
    anneal = 10 * 0.4 / (9 * 0.4 + 1)
    jit = torch.rand(N, S if per_sample_jitter else 1, generator=g)

    def chain(t, w, jit):
        td, wd = rm.dilate_weights(t, w, dil, 0.0, 1.0)
        td, wd = td[..., 1:-1], wd[..., 1:-1]
        logits = torch.where(td[..., 1:] > td[..., :-1], anneal * torch.log(wd), torch.full_like(wd, -torch.inf))
        return rm.sample_fenceposts(td, logits, S, 0.0, 1.0, jit), td, logits

    want, td, logits = chain(t, w, jit)
    truth = chain(t.double(), w.double(), jit.double())[0]
    got = _resample(lib, dev(t), dev(w), dil, anneal, S, jitter=dev(jit))
    assert got.shape == want.shape and bool((got[:, 1:] >= got[:, :-1]).all())
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    cdf = rm.cdf_of_weights(torch.softmax(logits, dim=-1))
    q_got, q_want = rm.interp_sorted(got, td, cdf), rm.interp_sorted(want, td, cdf)
    near = ((got - want).abs() <= 2e-6) | ((q_got - q_want).abs() <= 4e-6)
    e_ref = (want.double() - truth).abs().amax(-1, keepdim=True)
    e_hip = (got.double() - truth).abs()
    assert (near | (e_hip <= 4 * e_ref + 1e-5)).all(), (float((got - want).abs()[~near].max()), float(e_hip.max()), float(e_ref.max()))
    assert float(e_hip.max()) <= 1.5 * float(e_ref.max()) + 2e-6


# ------------------------------------------------------------------ (e) multi-rank render_image with a wrapped model
DDP_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch, torch.distributed as dist
import helpers as H
from oracle import raymarch as rm
from ucnerf_amd.internal import camera_utils, models
rank, world = int(sys.argv[3]), 2
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + sys.argv[2], rank=rank, world_size=world)
torch.cuda.set_device(0)                                  # both ranks share the box's one GPU
spec = rm.make_spec("tiny")
sd = rm.init_state(spec, seed=77)
model, cfg = H.hip_model(spec, sd)
Hh, Ww = 37, 53                                            # 1961 rays: odd -> the last shard is one row short
K = np.array([[60.0, 0.0, Ww / 2], [0.0, 60.0, Hh / 2], [0.0, 0.0, 1.0]])
c2w = np.concatenate([np.eye(3), np.array([[0.05], [0.02], [0.1]])], axis=1)
batch = camera_utils.generate_ray_batch((np.linalg.inv(K)[None], c2w[None], None, None), 0, Ww, Hh, 0.0, 8.0, device="cuda")
batch = {k: batch[k] for k in ("origins", "directions", "viewdirs", "cam_dirs", "radii", "near", "far")}
batch["rand_vec"] = torch.randn(Hh, Ww, 6, generator=torch.Generator().manual_seed(5)).cuda()
class Acc:
    def __init__(s, n, r): s.num_processes, s.process_index, s.is_main_process = n, r, r == 0
# what accelerator.prepare(model) hands to render_image at num_processes > 1 (train.py:95,330): a DDP wrapper
wrapped = torch.nn.parallel.DistributedDataParallel(model, device_ids=[0])
for rw, gw in ((False, True), (True, True), (False, False)):
    cfg.render_gather_weights = gw
    whole = models.render_image(model, Acc(1, 0), batch, False, 1.0, cfg, verbose=False, return_weights=rw)
    got = models.render_image(wrapped, Acc(world, rank), batch, False, 1.0, cfg, verbose=False, return_weights=rw)
    for k in ("rgb", "depth", "acc", "distance_mean", "distance_median") + (("weights",) if (rw or gw) else ()) + (("coord",) if rw else ()):
        assert got[k].shape == whole[k].shape, (k, got[k].shape, whole[k].shape)
        assert torch.equal(got[k], whole[k]), (rw, k, float((got[k] - whole[k]).abs().max()))
    # the returned key set never depends on the world size: the reference's keys by default (models.py:965-968 gathers
    # `weights` with everything else); config.render_gather_weights = False drops the 27x payload at EVERY world size
    assert set(got) == set(whole) and ("weights" in got) == (rw or gw)
    assert all(len(got[k]) == 2 for k in got if k.startswith("ray_"))
assert wrapped.module.training               # models.py:1006: render_image leaves the model in train mode
dist.barrier(); dist.destroy_process_group()
print("OK", rank)
'''


def test_render_image_two_ranks_with_a_ddp_wrapped_model(tmp_path):
    """SURVEY 8(e) / reference train.py:95,330, render.py:119,146: render_image receives the accelerate-prepared
    model, a DistributedDataParallel wrapper at num_processes > 1.  Two ranks (gloo, sharing this box's GPU) render
    row shards of a ragged frame and exchange them with the one packed all-gather; every gathered buffer must equal
    the single-rank frame bit for bit (a ray's result does not depend on the launch it rides in)."""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "ddp_worker.py"
    script.write_text(DDP_WORKER)
    port = str(31500 + os.getpid() % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), repo, port, str(r)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert all("OK" in o for o in outs)


# ------------------------------------------------------------------ early-termination sample compaction
def test_sample_compaction_matches_the_full_evaluation():
    """Model.compact_min_weight: colour layers only for samples with compositing weight >= threshold (the reference
    evaluates all of them, models.py:221-243).  (i) threshold below every positive weight: the frame is bit-identical
    to the uncompacted one (a sample's colour does not depend on which tile slot it rides in); (ii) threshold 4e-8:
    pixel error <= 128 * 4e-8 by construction, and most samples are skipped on a field with opaque surfaces."""
    from ucnerf_amd.internal import models
    spec = rm.make_spec("tiny")
    sd = rm.init_state(spec, seed=95)
    model, cfg = H.hip_model(spec, sd, max_chunk_rays=1000)
    model.nerf_mlp.density_bias = 8.0        # fog of density ~8 per unit length: optical depth ~60 over the ray, so the
    #                                          transmittance in front of most samples is below any float weight
    n = 2500
    rays = H.to_dev(rm.synthetic_rays(n, seed=96))
    rays["rand_vec"] = torch.randn(n, 6, generator=torch.Generator().manual_seed(97)).cuda()

    def march(thr):
        model.compact_min_weight = thr
        model._alive_stats = [] if thr > 0 else None
        with torch.no_grad():
            r, _ = model._march(False, rays, 1.0, True, None, want_history=False)
        torch.cuda.synchronize()
        return {k: r[-1][k].clone() for k in ("rgb", "depth", "acc", "weights")}, model._alive_stats

    full, _ = march(0.0)
    tiny, st0 = march(1e-45)                                   # smallest positive float: only exact zeros are skipped
    for k in full:
        assert torch.equal(full[k], tiny[k]), k
    cut, st1 = march(4e-8)
    assert H.maxdiff(cut["rgb"].cpu(), full["rgb"].cpu()) <= 128 * 4e-8 * 1.002 + 1e-7
    for k in ("depth", "acc", "weights"):
        assert torch.equal(cut[k], full[k]), k                 # geometry never depends on the colour pass
    alive = sum(a for a, _ in st1) / sum(t for _, t in st1)
    assert alive < 0.6, alive                                  # most samples sit behind an opaque medium here
    model.compact_min_weight, model._alive_stats = 0.0, None


# ------------------------------------------------------------------ sky layer only where there is background weight
def test_sky_is_skipped_for_rays_without_background_weight():
    """Model.sky_min_background: the sky NeRF runs only for rays whose background weight 1 - sum(weights) reaches the
    threshold (the reference evaluates it for every ray, models.py:326-337).  Kept rays: bit-identical sky and pixel;
    skipped rays: sky_rgbs = 0 and the pixel moves by at most background weight * |A_sky sky + b|."""
    spec = rm.make_spec("tiny", model_sky=True, brightness_correction=True)
    sd = rm.init_state(spec, seed=31)
    model, cfg = H.hip_model(spec, sd)
    n = 1500
    rays = H.to_dev(rm.synthetic_rays(n, seed=32))
    rays["rand_vec"] = torch.randn(n, 6, generator=torch.Generator().manual_seed(33)).cuda()
    cam = torch.tensor([1]).cuda()

    def march(thr):
        model.sky_min_background = thr
        with torch.no_grad():
            r, _ = model._march(False, rays, 1.0, False, cam, want_history=False)
        torch.cuda.synchronize()
        return {k: r[-1][k].clone() for k in ("rgb", "sky_rgbs", "weights")}

    full = march(0.0)
    bgw = 1 - full["weights"].reshape(n, -1).sum(-1)
    thr = float(bgw.median())
    cut = march(thr)
    kept = bgw >= thr
    assert model._sky_kept == (int(kept.sum()), n) and 0.3 * n < int(kept.sum()) < 0.7 * n
    assert torch.equal(cut["sky_rgbs"][kept], full["sky_rgbs"][kept])
    assert torch.equal(cut["rgb"].reshape(n, 3)[kept], full["rgb"].reshape(n, 3)[kept])
    assert float(cut["sky_rgbs"][~kept].abs().max()) == 0.0
    moved = (cut["rgb"].reshape(n, 3) - full["rgb"].reshape(n, 3)).abs().max(-1).values
    A_sky = model.brightness_corr.affines(cam)[1].reshape(-1, 3, 4)[0]
    bound = bgw * float(A_sky.abs().sum(-1).max()) * 1.001 + 1e-7
    assert bool((moved[~kept] <= bound[~kept]).all())
    everything = march(1e-30)                                  # threshold below every background weight: nothing skipped
    assert torch.equal(everything["rgb"], full["rgb"])
    model.sky_min_background = 0.0


# ------------------------------------------------------------------ mixed precision: render_image under autocast
def test_sky_layer_mixed_precision_against_its_rounding_model():
    """ucn_sky_render(mixed = 1): the sky NeRF with bf16 MFMA layers (what the reference's nn.Linear layers are under the
    bf16 autocast render_image runs its chunks in, models.py:957).  Pinned to a torch restatement of exactly this
    arithmetic -- bf16-rounded weights and activations at the kernel's rounding points, exact products, fp32 sums;
    layer 0 and both heads fp32; the composed matrices formed in fp64 -- over a ragged ray count; the residual is the
    order of the fp32 sums plus the rare activation that rounds the other way (stated bars: mean 2e-4, max 5e-3).
    And to the fp32-class kernel at bf16 accuracy; through Model._march the switch is the autocast state."""
    from ucnerf_amd.internal import sky as skymod
    torch.manual_seed(3)
    net = skymod.NeRF(D=8, d_in_view=3, W=256, multires_view=4, output_ch=4, skips=[4]).cuda()
    with torch.no_grad():
        net.alpha_linear.weight.mul_(6.0)                   # densities that matter over the sample spacing
        net.alpha_linear.bias.add_(0.05)
    n = 301                                                  # 36 120 samples: the last workgroup is ragged
    g = torch.Generator().manual_seed(4)
    o = (torch.randn(n, 3, generator=g) * 0.3).cuda()
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).cuda() * 1.3
    cam = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).cuda()
    far = (2.0 + 3.0 * torch.rand(n, generator=g)).cuda()
    full = net.render(o, d, cam, far)
    mixed = net.render(o, d, cam, far, mixed=True)
    torch.cuda.synchronize()
    assert torch.isfinite(mixed).all()

    def bf(t):
        return t.to(torch.bfloat16).float()

    with torch.no_grad():
        S = skymod.N_SKY_SAMPLES
        tv = torch.linspace(0., 1., steps=S).cuda()
        inv_far = 1.0 / (float(far[0]) * 1.5)
        z = far[:, None] * (1 - tv) + inv_far * tv
        pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)
        views = cam[:, None, :].expand(-1, S, -1).reshape(-1, 3)
        venc = torch.cat([views] + [fn(views * f) for f in (1., 2., 4., 8.) for fn in (torch.sin, torch.cos)], -1)
        L = net.pts_linears
        h = bf(torch.relu(pts @ L[0].weight.t() + L[0].bias))
        acc = None
        for i in range(1, 8):
            if i == 5:
                acc = h @ bf(L[5].weight[:, 3:]).t() + bf(pts) @ bf(L[5].weight[:, :3]).t() + bf(L[5].bias)
            else:
                acc = h @ bf(L[i].weight).t() + L[i].bias
            h = bf(torch.relu(acc))
        sigma = torch.relu(acc) @ net.alpha_linear.weight.t() + net.alpha_linear.bias
        Wv = net.views_linears[0].weight.double()
        Mh = bf((Wv[:, :256] @ net.feature_linear.weight.double()).float())
        bv = bf((net.views_linears[0].bias.double() + Wv[:, :256] @ net.feature_linear.bias.double()).float())
        v = torch.relu(h @ Mh.t() + bf(venc) @ bf(net.views_linears[0].weight[:, 256:]).t() + bv)
        rgb = torch.sigmoid(v @ net.rgb_linear.weight.t() + net.rgb_linear.bias).reshape(n, S, 3)
        sigma = sigma.reshape(n, S)
        dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1) * d.norm(dim=-1, keepdim=True)
        alpha = 1 - torch.exp(-torch.relu(sigma) * dists)
        trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha + 1e-10], -1), -1)[:, :-1]
        want = ((alpha * trans)[..., None] * rgb).sum(-2)
    e = (mixed - want).abs()
    assert float(e.mean()) <= 2e-4 and float(e.max()) <= 5e-3, (float(e.mean()), float(e.max()))
    e32 = (mixed - full).abs()
    assert float(e32.max()) <= 3e-2 and float(e32.mean()) <= 5e-3, (float(e32.max()), float(e32.mean()))
    assert float(e32.max()) > 0.0                            # it IS another arithmetic
    # a ray's result does not depend on the launch it rides in (1 ... 5 rays: waves without a live lane, ragged tiles)
    for k in (1, 5):
        sub = net.render(o[:k].contiguous(), d[:k].contiguous(), cam[:k].contiguous(), far[:k].contiguous(), mixed=True)
        assert torch.equal(sub, mixed[:k]), k

    # through the model: the autocast state selects it, the knob switches it off bit-exactly
    spec = rm.make_spec("tiny", model_sky=True, brightness_correction=True)
    model, cfg = H.hip_model(spec, rm.init_state(spec, seed=31))
    with torch.no_grad():
        model.skynerf.alpha_linear.bias.add_(1.0)             # a sky that is not transparent
    rays = H.to_dev(rm.synthetic_rays(700, seed=32))
    rays["rand_vec"] = torch.randn(700, 6, generator=torch.Generator().manual_seed(33)).cuda()
    camidx = torch.tensor([1]).cuda()

    def march(autocast):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            r, _ = model._march(False, rays, 1.0, False, camidx, want_history=False)
        torch.cuda.synchronize()
        return r[-1]["sky_rgbs"].float().clone(), model._sky_mixed

    s32, f0 = march(False)
    s16, f1 = march(True)
    assert (f0, f1) == (False, True)
    dm = (s16 - s32).abs()                                   # init_state's O(1) weights: bf16 through 9 layers of them
    assert 0.0 < float(dm.max()) <= 0.15 and float(dm.mean()) <= 2e-2, (float(dm.max()), float(dm.mean()))
    model.autocast_render = False
    soff, f2 = march(True)
    assert f2 is False and torch.equal(soff, s32)


def test_render_under_autocast_runs_the_mixed_precision_path():
    """The reference wraps the model call of render_image in accelerator.autocast() (models.py:957): with mixed precision
    on, its grid op gathers half tables (grid.py:41-44) and its Linear layers run in bf16.  Here the same context switches
    the inference march to the half-table gather + the bf16 MFMA kernels of the training forward (no stores), fp32
    compositing.  Checked: the path is taken for both levels, the frame agrees with the fp32-class frame to bf16 accuracy
    (stated: 8 mantissa bits through three 256-wide layers -> a few 1e-3 per pixel, 3e-2 worst case), geometry outputs
    that do not depend on the colour layers stay close, and the knob switches it off bit-exactly."""
    from ucnerf_amd.internal import models
    import bench
    model, cfg, _ = bench.build_model(torch.device("cuda", 0))           # config B: the 256-wide field the bf16 kernels cover
    n = 4096
    rays = H.to_dev(rm.synthetic_rays(n, seed=5))
    rays["rand_vec"] = torch.randn(n, 6, generator=torch.Generator().manual_seed(6)).cuda()

    def march(autocast):
        model._mixed_levels = 0
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            r, _ = model._march(False, rays, 1.0, True, None, want_history=False)
        torch.cuda.synchronize()
        return {k: r[-1][k].float().clone() for k in ("rgb", "acc", "depth", "weights")}, model._mixed_levels

    full, used0 = march(False)
    mixed, used1 = march(True)
    assert used0 == 0 and used1 == 2
    assert torch.isfinite(mixed["rgb"]).all()
    d = (mixed["rgb"] - full["rgb"]).abs()
    assert float(d.max()) <= 3e-2 and float(d.mean()) <= 3e-3, (float(d.max()), float(d.mean()))
    assert float((mixed["acc"] - full["acc"]).abs().max()) <= 3e-2
    model.autocast_bf16_features = False                     # float features between gather and MLP: the same pixels, bit for bit
    wide, used3 = march(True)
    model.autocast_bf16_features = True
    assert used3 == 2
    for k in mixed:
        assert torch.equal(wide[k], mixed[k]), k
    model.autocast_render = False
    off, used2 = march(True)
    model.autocast_render = True
    assert used2 == 0
    for k in full:
        assert torch.equal(off[k], full[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# SURVEY 8 rows a5 / a6 seen DIRECTLY: the fused featurisation's own geometry stage -- the device
# functions cast_sample / contract_to_unit that k_march_features, k_cast_cache and every backward kernel call -- written
# out by ucn_cast_probe / ucn_contract_probe and compared with the reference's cast_rays / track_linearize outputs
# (tests/golden/cast.npz, generated from the imported reference: G3 eval + train draws, G4 contraction).
def _cast_probe(fx, rand_vec, flip=None, spin=None):
    from ucnerf_amd import _lib
    lib = _lib.load()
    dev = "cuda"
    N, S1 = fx["tdist"].shape
    S = S1 - 1
    f = lambda t: t.to(dev).float().contiguous()
    # near = 0, far = 1: t = s * far + (1 - s) * near = s exactly, so the golden's metric fenceposts go in as sdist
    sdist, near, far = f(fx["tdist"]), torch.zeros(N, device=dev), torch.ones(N, device=dev)
    o, d, cam, rad = f(fx["origins"]), f(fx["directions"]), f(fx["cam_dirs"]), f(fx["radii"]).reshape(-1)
    basis = torch.empty(N, 6, device=dev)
    _lib.check(lib.ucn_cone_basis(cam.data_ptr(), f(rand_vec).data_ptr(), N, basis.data_ptr(), _lib.stream()))
    out = torch.full((N, S, 6, 10), float("nan"), device=dev)
    fl, sp = (None, None) if flip is None else (f(flip), f(spin))
    _lib.check(lib.ucn_cast_probe(sdist.data_ptr(), near.data_ptr(), far.data_ptr(), o.data_ptr(), d.data_ptr(), basis.data_ptr(),
                                  rad.data_ptr(), _lib.ptr(fl), _lib.ptr(sp), 0.5, N, S, out.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    return out.cpu()


def test_cone_cast_and_contraction_vs_reference_golden():
    fx = H.load("cast.npz")
    for tag, kw in (("eval", {}), ("train", dict(flip=fx["train_flip"], spin=fx["train_spin"]))):
        got = _cast_probe(fx, fx[f"{tag}_rand_vec"], **kw)
        means, stds, t = fx[f"{tag}_means"], fx[f"{tag}_stds"], fx[f"{tag}_t"]
        # every one of the 6 multisamples separately: a swapped / mirrored hexagon offset that keeps the mean of six fails here.
        # (test_bracket_gpu.py::test_cone_cast_and_contraction_bracket holds the same outputs to 2 x the float32 oracle's float64 error)
        # |means| up to ~8: 2 ulp of 8 = 2e-6 (the eval pattern's cos / sin are host constants, the train draws go through
        # v_sin / v_cos with ~1e-6 absolute error on an offset of size r t / sqrt(2) ~ 1e-3 t)
        assert H.maxdiff(got[..., 0:3], means) <= 4e-6, tag
        assert H.maxdiff(got[..., 4], t) <= 2e-6, tag
        # (the reference yields NaN for a zero-width interval at t = 0, render.py:116: same places, compared by maxdiff above)
        ok = torch.isfinite(stds)
        assert torch.equal(torch.isfinite(got[..., 3]), ok)
        rel = ((got[..., 3] - stds).abs() / stds.abs().clamp_min(1e-30))[ok].max()
        assert float(rel) <= 4e-7, (tag, float(rel))                 # std = std_scale * r * t / sqrt(2): a multiply for a divide
        # behind the contraction (coord.py:60-116) and the / 2 of models.py:491-493: against the oracle's restatement of
        # track_linearize on the GOLDEN's means / stds (itself pinned to the reference by G4 below and test_oracle_golden)
        okf = ok.reshape(-1)
        cm, cs = rm.contract_points(means.reshape(-1, 3)[okf], stds.reshape(-1)[okf])
        assert H.maxdiff(got[..., 5:8].reshape(-1, 3)[okf], cm / 2) <= 4e-6, tag
        relc = ((got[..., 8].reshape(-1)[okf] - cs / 2).abs() / (cs / 2).abs().clamp_min(1e-30)).max()
        assert float(relc) <= 2e-5, (tag, float(relc))               # exp2(log2(.) / 3) on the fast transcendental units
        pos = cs > 0
        rs = 1.0 / torch.sqrt(8.0 * (cs[pos].double() / 2) ** 2)
        assert float(((got[..., 9].reshape(-1)[okf][pos].double() - rs).abs() / rs).max()) <= 3e-5, tag
    # G4: the reference's track_linearize on its own inputs (origin, points inside / on / far outside the unit ball)
    from ucnerf_amd import _lib
    lib = _lib.load()
    m_in, s_in = fx["contract_in_mean"].cuda().contiguous(), fx["contract_in_std"].cuda().contiguous()
    B = m_in.shape[0]
    om, os_ = torch.empty(B, 3, device="cuda"), torch.empty(B, device="cuda")
    _lib.check(lib.ucn_contract_probe(m_in.data_ptr(), s_in.data_ptr(), B, om.data_ptr(), os_.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    assert H.maxdiff(om.cpu() * 2, fx["contract_mean"]) <= 5e-7       # |z| <= 2: 2 ulp
    rel = ((os_.cpu() * 2 - fx["contract_std"]).abs() / fx["contract_std"].abs().clamp_min(1e-30)).max()
    assert float(rel) <= 2e-5, float(rel)
    assert (om.cpu().norm(dim=-1) <= 1 + 1e-6).all()


def test_forward_routes_on_training_mode_not_on_grad_mode():
    """an eval-mode call OUTSIDE torch.no_grad() runs the fused inference march (no autograd graph,
    no training activation buffers); the training graph is built only for model.train() with autograd enabled."""
    spec = rm.make_spec("tiny")
    sd = rm.init_state(spec, seed=9)
    n = 64
    rays = rm.synthetic_rays(n, seed=10)
    noise = [rm.draw_level_noise(spec, n, l, False, torch.Generator().manual_seed(11 + l)) for l in range(2)]
    model, _ = H.hip_model(spec, sd)
    batch = H.pin_noise(H.to_dev(rays), noise)
    assert torch.is_grad_enabled() and not model.training
    a, _ = model(False, batch, 1.0, True)
    assert not a[-1]["rgb"].requires_grad and "distance_median" in a[-1]
    with torch.no_grad():
        b, _ = model(False, batch, 1.0, True)
    assert torch.equal(a[-1]["rgb"], b[-1]["rgb"])
    model.train()
    c, _ = model(False, batch, 1.0, True)
    assert c[-1]["rgb"].requires_grad and "distance_median" in c[-1]
    assert H.maxdiff(c[-1]["rgb"].detach().cpu().reshape(-1, 3), a[-1]["rgb"].cpu().reshape(-1, 3)) <= 2e-4
    with torch.no_grad():
        d, _ = model(False, batch, 1.0, True)
    assert not d[-1]["rgb"].requires_grad
    model.march_route = "inference"
    e, _ = model(False, batch, 1.0, True)
    assert not e[-1]["rgb"].requires_grad


def test_non_positive_dilation_with_dilation_on_is_refused():
    """use_dilation true (a knob > 0) but a computed dilation <= 0 (negative dilation_bias) must not silently
    take ucn_resample's undilated branch -- both routes refuse."""
    spec = rm.make_spec("tiny")
    sd = rm.init_state(spec, seed=9)
    rays = rm.synthetic_rays(8, seed=10)
    model, _ = H.hip_model(spec, sd)
    model.dilation_bias, model.dilation_multiplier = -1.0, 0.5
    for train in (False, True):
        model.train(train)
        with pytest.raises(NotImplementedError, match="dilation"):
            model(False, H.to_dev(rays), 1.0, False)


NCCL_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[2], HSA_ENABLE_IPC_MODE_LEGACY="0", UCN_DIST_INPLACE=sys.argv[3])
import torch, torch.distributed as dist
from ucnerf_amd.internal import dist as udist
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
assert dist.get_backend() == "nccl"
g = torch.Generator(device="cuda").manual_seed(1)
rp, width = 1000, 9
out = torch.full((rp, width), float("nan"), device="cuda")
mine = out[0:rp]
mine.copy_(torch.rand(rp, width, device="cuda", generator=g))
want = mine.clone()
udist._exchange(out, mine, 0, rp)                 # the collective all_gather_rows issues, on RCCL
torch.cuda.synchronize()
assert torch.equal(out, want)
dist.barrier(); dist.destroy_process_group()
print("OK")
'''


@pytest.mark.parametrize("inplace", ["0", "1"])
def test_the_frame_exchange_runs_on_rccl(tmp_path, inplace):
    """the `nccl` (= RCCL) branch of internal/dist.py had never executed anywhere.  A 1-GPU box cannot
    host two RCCL ranks, but a one-rank process group runs the real collective through RCCL on the device buffers: the
    out-of-place default and the asserted in-place form (UCN_DIST_INPLACE=1)."""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "nccl_worker.py"
    script.write_text(NCCL_WORKER)
    p = subprocess.run([sys.executable, str(script), repo, str(32500 + os.getpid() % 2000), inplace], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------------
# the per-SAMPLE bars of the fine NeRF level are loose because the function is ill-conditioned there
# (1 ulp of a contracted coordinate = 0.03 cell at resolution 524 288).  This puts a number on "loose": the same
# featurisation + density MLP evaluated in float64 on the same float32 inputs is the truth, the float32 reference
# semantics (the oracle = the golden's values) has its own distance to it, and the HIP path must be within a small factor
# of THAT distance -- per sample, not per pixel.
def _truth_density64(fs, sd, means, stds):
    """models.py:485-512 in float64 (oracle/truth64.py: contraction, / 2, hash-grid interpolation with the reference's float32
    level constants and exact integer cells, erf damping with the int32-wrapped grid_sizes ** 2, mean of 6, density MLP)."""
    from oracle import truth64 as t64
    with torch.no_grad():
        res = t64.field_forward(fs, t64.state64(sd), means, stds)
    return res["raw_density"], res["features"].flatten(-2, -1)


def test_fine_level_per_sample_error_is_bracketed_by_the_float32_reference_itself():
    fx = H.load("field.npz")
    spec = rm.make_spec("tiny")
    sd = H.state_for(fx, spec)
    model, _ = H.hip_model(spec, sd)
    means, stds = fx["means"], fx["stds"]
    truth_raw, truth_feat = _truth_density64(spec.nerf, sd, means, stds)
    want_raw = fx["nerf_raw_density"].double()                      # the reference's own float32 evaluation (golden)
    want_feat = fx["nerf_features"].double()
    got_raw, _, _ = model.nerf_mlp.predict_density(dev(means), dev(stds))
    got_raw = got_raw.cpu().double()
    e_ref, e_hip = (want_raw - truth_raw).abs(), (got_raw - truth_raw).abs()
    # the float32 reference really is that far from the truth somewhere (otherwise this test says nothing) ...
    assert float(e_ref.max()) >= 1e-4 and float((want_feat - truth_feat).abs().max()) >= 1e-4
    # ... and the HIP path is no further, worst case and on average
    assert float(e_hip.max()) <= 2.0 * float(e_ref.max()) + 1e-6, (float(e_hip.max()), float(e_ref.max()))
    assert float(e_hip.mean()) <= 2.0 * float(e_ref.mean()) + 1e-7, (float(e_hip.mean()), float(e_ref.mean()))
    print(f"fine level, raw density per sample: |reference fp32 - fp64 truth| max {float(e_ref.max()):.2e} mean {float(e_ref.mean()):.2e}; "
          f"|HIP - truth| max {float(e_hip.max()):.2e} mean {float(e_hip.mean()):.2e}")


@pytest.mark.parametrize("case", ["default", "tiny_trunk", "huge_trunk", "uneven_layers"])
def test_sky_split_f16_range(case):
    """the fp32-class sky kernel (k_sky_mlp, split-f16 operands) carried no layer scales, so the range
    guard of test_split_f16_range did not cover it.  It now carries statistical power-of-two scales chosen at pack time
    (sky.hip k_sky_scales): whatever the magnitudes of the trunk's activations -- 1e-4 (low halves would be subnormal),
    1e5 (f16 operands would overflow to inf), or alternating from layer to layer -- the rendered sky colour must stay
    fp32-class against a float64 evaluation of the same network (train_graph.sky_forward on a double copy).  In a build
    without the scales (every exponent 0) `tiny_trunk` is 1.8e-5 and `huge_trunk` 6.8e-5 off -- 100x / 400x the float32 reference's
    own 1.7e-7 -- and both cases fail this test."""
    import copy
    from ucnerf_amd.internal import train_graph as tg
    from ucnerf_amd.internal.sky import NeRF
    torch.manual_seed(21)
    net = NeRF(D=8, d_in_view=3, W=256, multires_view=4, output_ch=4, skips=[4])
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
        P = net.pts_linears
        if case == "tiny_trunk":                       # h0 ~ 1e-4 of its default size; the heads bring the outputs back
            P[0].weight.mul_(1e-4); P[0].bias.mul_(1e-4)
            for l in range(1, 8):
                P[l].bias.mul_(1e-4)
            P[5].weight[:, :3].mul_(1e-4)
            net.alpha_linear.weight.mul_(1e4); net.feature_linear.weight.mul_(1e4)
        elif case == "huge_trunk":
            P[0].weight.mul_(3e4); P[0].bias.mul_(3e4)
            for l in range(1, 8):
                P[l].bias.mul_(3e4)
            P[5].weight[:, :3].mul_(3e4)
            net.alpha_linear.weight.mul_(1 / 3e4); net.feature_linear.weight.mul_(1 / 3e4)
        elif case == "uneven_layers":
            for l, f in zip(range(1, 8), (300.0, 1 / 300.0, 300.0, 1 / 300.0, 300.0, 1 / 300.0, 300.0)):
                P[l].weight.mul_(f)
                if l == 5:
                    pass
            net.alpha_linear.weight.mul_(1 / 300.0); net.feature_linear.weight.mul_(1 / 300.0)
    n = 512
    rays = rm.synthetic_rays(n, seed=22)
    o, d, cam, far = rays["origins"], rays["directions"], rays["cam_dirs"], rays["far"]
    with torch.no_grad():
        truth = tg.sky_forward(copy.deepcopy(net).double(), o.double(), d.double(), cam.double(), far.double())
        want32 = tg.sky_forward(net, o, d, cam, far)                       # the reference's own float32 arithmetic
        got = net.cuda().render(o.cuda(), d.cuda(), cam.cuda(), far.cuda()).cpu().double()
    assert torch.isfinite(got).all(), "f16 operand overflow"
    assert float(truth.abs().max()) > 1e-3
    e_ref, e_hip = float((want32.double() - truth).abs().max()), float((got - truth).abs().max())
    assert e_hip <= 3 * e_ref + 3e-6, (case, e_hip, e_ref)
