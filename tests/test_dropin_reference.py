"""The drop-in overlay's gin registration.  Running the reference's own entry scripts unchanged against the
overlay needs a checkout of the reference, which is not part of this repository: tools/dropin_harness.py does that by hand."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_models_register_with_gin_when_gin_is_importable():
    """Without the overlay: `import gin` present -> Model / NerfMLP / PropMLP are gin configurables (ref models.py:30,688,693)."""
    code = (
        "import sys; sys.path.insert(0, %r); import mini_gin; sys.modules['gin'] = mini_gin\n"
        "sys.path.insert(0, %r)\n"
        "import gin\n"
        "from ucnerf_amd.internal import models, configs\n"
        "gin.parse_config('Model.num_levels = 2\\nModel.num_nerf_samples = 48\\nNerfMLP.grid_log2_hashmap_size = 10\\n"
        "PropMLP.grid_log2_hashmap_size = 11\\nNerfMLP.bottleneck_width = 64')\n"
        "m = models.Model(config=configs.Config())\n"
        "assert (m.num_levels, m.num_nerf_samples) == (2, 48), (m.num_levels, m.num_nerf_samples)\n"
        "assert m.nerf_mlp.grid_log2_hashmap_size == 10 and m.prop_mlp_0.grid_log2_hashmap_size == 11\n"
        "assert m.nerf_mlp.bottleneck_width == 64 and m.prop_mlp_0.bottleneck_width == 256\n"
        "assert m.nerf_mlp.density_layer[2].out_features == 64 and m.prop_mlp_0.disable_rgb\n"
        "m2 = models.Model(config=configs.Config(), num_nerf_samples=16)      # explicit arguments win over bindings\n"
        "assert m2.num_nerf_samples == 16\n"
        "print('OK')\n") % (os.path.join(REPO, "tests", "stubs"), REPO)
    p = subprocess.run([sys.executable, "-B", "-c", code], capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
