"""The drop-in overlay's names on a device: the body of the reference's training loop (train.py:142-224) and its
render call (train.py:330) executed through `internal.models` / `internal.train_utils` AS THE OVERLAY RESOLVES THEM
(PYTHONPATH=<repo>/ucnerf_amd/compat/dropin:<repo>, sitecustomize's meta-path finder), under `accelerate.Accelerator` like the
reference (train.py:44,95,165,221).  tools/dropin_harness.py runs the reference's own scripts up to `Model(config=...)` where a
checkout of the reference exists; this test needs none, so the caller's `internal/` package is the stand-in under
tests/stubs/upstream_internal_standin/ (three files whose presence the overlay checks; its train_utils carries a function the overlay
must replace and one it must keep)."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = textwrap.dedent('''
    import json, sys, types
    import numpy as np, torch, accelerate
    from internal import models, train_utils                     # <- the overlay's names (train.py:17-21)
    from internal import configs
    import internal
    assert internal.__file__.replace("\\\\", "/").endswith("compat/dropin/internal/__init__.py"), internal.__file__
    assert models.Model.__module__ == "ucnerf_amd.internal.models"
    assert train_utils.compute_data_loss.__module__ == "ucnerf_amd.internal.train_utils"        # replaced
    assert train_utils.tree_len.__module__ == "internal._upstream_train_utils"                   # kept from the caller's module
    sys.path.insert(0, REPO_PATH)
    import bench
    accelerator = accelerate.Accelerator()                        # train.py:44
    dev = accelerator.device
    assert dev.type == "cuda"
    config = configs.Config(model_sky=True, brightness_correction=True, training_views=210)
    for k, v in dict(lr_init=0.01, lr_final=0.001, max_steps=100, lr_delay_steps=0, lr_delay_mult=1.0, adam_beta1=0.9, adam_beta2=0.99, adam_eps=1e-8,
                     data_loss_type='charb', charb_padding=0.001, data_loss_mult=1.0, data_coarse_loss_mult=0., anti_interlevel_loss_mult=0.01,
                     pulse_width=[0.03, 0.003], distortion_loss_mult=0.005, hash_decay_mults=0.1, disable_multiscale_loss=False,
                     sky_weight=0.002, idt_weight=0.002, render_chunk_size=4096).items():
        if not hasattr(config, k):
            setattr(config, k, v)
    torch.manual_seed(0)
    kw = dict(grid_level_dim=2, grid_log2_hashmap_size=15)
    with models.bindings(NerfMLP=dict(grid_disired_resolution=8192, **kw), PropMLP=dict(**kw)):
        model = models.Model(config=config, num_levels=2, num_prop_samples=64, num_nerf_samples=32)          # train.py:69
    # (the sky NeRF keeps its default initialisation: its density head is negative on these rays, the layer renders 0 -- a LIVE sky layer
    #  composites with the reference's NEGATIVE sample spacings (SURVEY.md Appendix C.2: z runs from batch.far DOWN to 1 / far, models.py:872,
    #  so alpha = 1 - exp(+sigma |dz|) <= 0 and the transmittance grows like exp(sum sigma |dz|)) and overflows float32 once Adam has pushed
    #  sigma up: the reference's own `[Numerical Error] rgb_map contains nan or inf` (models.py:899-901); tools/nan_hunt2.py shows it at step 3
    #  of this very model with the density head lifted, on the hand-written and on the library GEMMs alike)
    optimizer, lr_fn = train_utils.create_optimizer(config, model)                                          # train.py:102
    model, optimizer = accelerator.prepare(model, optimizer)                                                # train.py:95
    module = accelerator.unwrap_model(model)
    rays = bench.frame_rays(dev)
    n_total = bench.H_IMG * bench.W_IMG
    flat = {k: v.reshape(n_total, -1) for k, v in rays.items()}
    g = torch.Generator(device=dev).manual_seed(1)
    target = torch.rand(n_total, 3, device=dev, generator=g)
    first = last = None
    n = 2048
    for step in range(1, 41):                                                                               # train.py:142-224
        idx = torch.randint(0, n_total, (n,), device=dev, generator=g)
        batch = {k: v[idx][:, None, None, :] for k, v in flat.items()}
        batch['rgb'] = target[idx][:, None, None, :]
        batch['cam_idx'] = torch.randint(0, 210, (n, 1, 1, 1), device=dev, generator=g)
        batch['sky_segs'] = (torch.rand(n, 1, 1, device=dev, generator=g) > 0.7).float()
        for pg in optimizer.param_groups:
            pg['lr'] = lr_fn(step)
        train_frac = np.clip((step - 1) / (config.max_steps - 1), 0, 1)
        optimizer.zero_grad()
        with accelerator.autocast():
            renderings, ray_history = model(True, batch, train_frac=train_frac, compute_extras=False, zero_glo=False)
        losses = {}
        losses['data'], stats = train_utils.compute_data_loss(batch, renderings, config)
        losses['sky_segments'] = config.sky_weight * train_utils.sky_loss(batch, renderings)
        losses['identity'] = config.idt_weight * train_utils.transformIdentityLoss(renderings)
        losses['anti_interlevel'] = train_utils.anti_interlevel_loss(ray_history, config)
        losses['distortion'] = train_utils.distortion_loss(ray_history, config)
        losses['hash_decay'] = train_utils.hash_decay_loss(ray_history, config)
        loss = sum(losses.values())
        accelerator.backward(loss)
        train_utils.clip_gradients(model, accelerator, config)
        optimizer.step()
        v = float(loss.detach())
        first = v if first is None else first
        last = v
    assert np.isfinite(last) and last < first, (first, last)
    assert train_utils.tree_len(losses) == 6
    # train.py:330: the test-view render through the overlay's render_image, [H, W, .] batch
    H, W = 16, 24
    vb = {k: v[:H * W].reshape(H, W, -1) for k, v in flat.items()}
    out = models.render_image(model, accelerator, vb, False, 1.0, config, verbose=False, eval_camidx=torch.tensor([7]))
    assert out['rgb'].shape == (H, W, 3) and bool(torch.isfinite(out['rgb']).all())
    assert module.training                                          # models.py:1006
    print(json.dumps(dict(first=first, last=last, mixed_precision=str(accelerator.mixed_precision))))
''')


@pytest.mark.parametrize("mixed", ["no", "bf16"])
def test_training_loop_body_and_render_through_the_overlay_names(tmp_path, mixed):
    standin = os.path.join(REPO, "tests", "stubs", "upstream_internal_standin")
    script = tmp_path / "train_like.py"
    script.write_text(SCRIPT.replace("REPO_PATH", repr(REPO)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(REPO, "ucnerf_amd", "compat", "dropin"), REPO]),
               ACCELERATE_MIXED_PRECISION=mixed, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900, env=env, cwd=standin)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert r["mixed_precision"] == mixed and r["last"] < r["first"]
