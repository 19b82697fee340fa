"""Both marches over internal/march_level.py (-m gpu), through Model.forward only: the order of the UNPINNED random draws (every golden
pins them, so nothing else holds it) and the shape of what the two routes return."""
import pytest
import torch

import helpers as H
from oracle import raymarch as rm

pytestmark = pytest.mark.gpu

N = 64


def _same(a, b, where):
    assert type(a) is type(b), where
    if torch.is_tensor(a):
        assert a.shape == b.shape and torch.equal(a, b), where
    else:
        assert a is None and b is None, where


def _same_outputs(out_a, out_b):
    for name, la, lb in zip(("renderings", "ray_history"), out_a, out_b):
        assert len(la) == len(lb) == 2
        for i, (da, db) in enumerate(zip(la, lb)):
            assert set(da) == set(db), (name, i)
            for k in da:
                _same(da[k], db[k], (name, i, k))


@pytest.mark.parametrize("train", [False, True])
def test_unpinned_draws_follow_the_documented_order(train):
    """Nothing pinned, rand = True: the march draws, per level, rand(N, 1) (single_jitter), rand(N, S), rand(N, S), randn(N, 3) from
    torch's generator of the rays' device (stepfun.py:216, render.py:123,124,140).  The same draws made here after the same seed and
    pinned through rand_vec / march_noise give bit-identical outputs -- on the fused route (eval) and the graph route (train)."""
    spec = rm.make_spec("tiny")
    model, _ = H.hip_model(spec, rm.init_state(spec, seed=21))
    model.train(train)
    batch = H.to_dev(rm.synthetic_rays(N, seed=22))
    torch.manual_seed(1234)
    out_a = model(True, dict(batch), 0.5, True)
    if train:
        assert model.last_march_route == "train_graph"
    torch.manual_seed(1234)
    noise, vecs = [], []
    for S in (spec.num_prop_samples, spec.num_nerf_samples):
        jitter = torch.rand(N, 1, device="cuda")
        flip = torch.rand(N, S, device="cuda")
        spin = torch.rand(N, S, device="cuda")
        vecs.append(torch.randn(N, 3, device="cuda"))
        noise.append(dict(jitter=jitter, flip=flip, spin=spin))
    pinned = dict(batch, rand_vec=torch.cat(vecs, dim=-1), march_noise=noise)
    out_b = model(True, pinned, 0.5, True)
    assert model.last_march_route == ("train_graph" if train else "fused")
    _same_outputs(out_a, out_b)
    assert float(out_a[0][-1]["rgb"].abs().max()) > 0


@pytest.mark.parametrize("case", ["sky_brightness", "power_transformation"])
def test_both_routes_return_the_same_keys_and_first_fenceposts(case):
    """One pinned batch, compute_extras on: per level the two routes return the same keys (the graph route adds loss_hash_decay in
    training mode) and bit-equal level-0 fenceposts, which depend on nothing a route computes differently.  With the sky and
    brightness tails on, and with a warped raydist_fn (every kernel's tdist sibling, on both routes)."""
    if case == "sky_brightness":
        spec = rm.make_spec("tiny", model_sky=True, brightness_correction=True)
        model, _ = H.hip_model(spec, rm.init_state(spec, seed=23))
    else:
        spec = rm.make_spec("tiny")
        model, _ = H.hip_model(spec, rm.init_state(spec, seed=23), raydist_fn="power_transformation")
    noise = [rm.draw_level_noise(spec, N, lvl, True, torch.Generator().manual_seed(30 + lvl)) for lvl in range(2)]
    batch = H.pin_noise(H.to_dev(rm.synthetic_rays(N, seed=24)), noise)
    outs = {}
    for train in (False, True):
        model.train(train)
        outs[train] = model(True, dict(batch), 0.5, True)
        assert model.last_march_route == ("train_graph" if train else "fused")
    (r_f, h_f), (r_t, h_t) = outs[False], outs[True]
    assert len(r_f) == len(r_t) == len(h_f) == len(h_t) == 2
    for i in range(2):
        assert set(r_f[i]) == set(r_t[i]), i
        assert set(h_f[i]) == set(h_t[i]) - {"loss_hash_decay"}, i
    if case == "sky_brightness":
        assert {"sky_rgbs", "affine_trans", "affine_trans_sky"} <= set(r_f[0])
    assert torch.equal(h_f[0]["sdist"], h_t[0]["sdist"])
    assert torch.isfinite(r_f[-1]["rgb"]).all() and torch.isfinite(r_t[-1]["rgb"]).all()
