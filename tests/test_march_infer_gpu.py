"""The inference march's pass loop on the device (internal/march_infer.py `run_passes`): 96 rays of the `tiny` model in three passes of 32
per level -- both feature buffers and the wait on a buffer's previous reader -- on one stream and on two (`Model.overlap_streams` False,
True, 2), against the same march in ONE pass, bit for bit on every key of the renderings and of the history.  Once on the plain fields,
once on fields whose three per-sample tails all run: the NeRF field with the diffuse colour, roughness and predicted-normal heads, the
proposal field with density normals (one field cannot have predicted and density normals both)."""
import functools

import pytest
import torch

import helpers as H
from oracle import raymarch as rm
from ucnerf_amd.internal import models

pytestmark = pytest.mark.gpu

RAYS, CHUNK = 96, 32


@functools.lru_cache(maxsize=None)
def _setup(heads):
    """(model, batch with every draw pinned, the one-pass march's renderings and history)"""
    spec = rm.make_spec("tiny")
    sd = rm.init_state(spec, seed=31)
    on = {}
    if heads:
        g, nb = torch.Generator().manual_seed(32), spec.nerf.bottleneck_width
        for name, rows in (("normal_layer", 3), ("diffuse_layer", 3), ("roughness_layer", 1)):
            sd[f"nerf_mlp.{name}.weight"] = torch.randn(rows, nb, generator=g) / nb ** 0.5
            sd[f"nerf_mlp.{name}.bias"] = 0.1 * torch.randn(rows, generator=g)
        on = dict(NerfMLP=dict(use_diffuse_color=True, enable_pred_roughness=True, enable_pred_normals=True),
                  PropMLP=dict(disable_density_normals=False))
    with models.bindings(**on):
        model, _ = H.hip_model(spec, sd)
    g = torch.Generator().manual_seed(33)
    noise = [rm.draw_level_noise(spec, RAYS, lvl, True, g) for lvl in range(spec.num_levels)]
    batch = H.pin_noise(H.to_dev(rm.synthetic_rays(RAYS, seed=34)), noise)
    assert model.max_chunk_rays >= RAYS and not model.overlap_streams
    return model, batch, _marched(model, batch)


def _marched(model, batch):
    with torch.no_grad():
        out = model._march(True, batch, 1.0, True, None, want_history=True)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("overlap", [False, True, 2])
@pytest.mark.parametrize("heads", [False, True], ids=["plain", "heads"])
def test_three_passes_give_the_bits_of_one(heads, overlap):
    model, batch, (want_r, want_h) = _setup(heads)
    if heads:                                                          # all three tails ran
        assert want_h[0]["raw_grad_density"] is not None and want_h[0]["normals"].any()
        assert want_h[1]["normals_pred"].any() and want_h[1]["roughness"].any() and "roughness" in want_r[1] and "normals" in want_r[0]
    model.max_chunk_rays, model.overlap_streams, model._prof, model._prof_every = CHUNK, overlap, [], 1
    try:
        got_r, got_h = _marched(model, batch)
        prof = model._prof
    finally:
        model.max_chunk_rays, model.overlap_streams, model._prof = 10240, False, None
    assert [(lvl, n) for lvl, n, *_ in prof] == [(lvl, CHUNK) for lvl in range(model.num_levels) for _ in range(RAYS // CHUNK)]
    assert (getattr(model, "_side_stream", None) is not None) or not overlap
    differing = []
    for name, got, want in (("renderings", got_r, want_r), ("history", got_h, want_h)):
        assert len(got) == len(want) == model.num_levels
        for lvl, (g, w) in enumerate(zip(got, want)):
            assert set(g) == set(w)
            for k in sorted(w):
                if (w[k] is None) != (g[k] is None) or (w[k] is not None and not torch.equal(g[k], w[k])):
                    differing.append(f"{name}[{lvl}][{k!r}]")
    assert not differing, differing
