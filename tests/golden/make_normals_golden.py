"""Generate tests/golden/normals_tiny.npz: the REFERENCE's `MLP.forward` with `disable_density_normals = False` (models.py:546-567), on CPU.

    python tests/golden/make_normals_golden.py          (authoring container only)

Same harness as make_golden.py (ref_import: the reference's own Python; its grid.py runs over oracle/grid_cpu.py, whose forward fills
`dy_dx` and whose backward returns `grad_inputs` -- grid.py:49-89's `calc_grad_inputs` path, taken because `means` requires grad).  So
the reference's own autograd gives raw_grad_density = mean_j d raw_density / d means_j and normals = -l2_normalize(that).

Only `no_warp=True`: with the warp on, the reference hands `means` to coord.track_linearize, which is @torch.no_grad (coord.py:75), so
its graph has no edge from the contracted means back to `means` and autograd.grad has nothing to return; the warped path therefore has no
golden (tests/normals_ref.py restates it; tests/test_normals_cpu.py holds it by finite differences).  What this fixture pins in the
restatement: the level scale in dy_dx, the damping, 1/G, the mean over j, the sign, and F.normalize's eps.

Both fields of spec `tiny` (NeRF L=16 C=2 hashed, proposal L=6 C=2), 192 samples of 6 Gaussians each, inside the grid's cube; sample 0
sits at the origin.  Weights: oracle.raymarch.init_state (seed + checksum).
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import ref_import  # noqa: E402
from oracle import raymarch as rm  # noqa: E402

SEED, N, G = 141, 192, 6


def points():
    g = torch.Generator().manual_seed(SEED + 1)
    means = (torch.rand(N, 1, 3, generator=g) * 1.9 - 0.95) + 0.003 * torch.randn(N, G, 3, generator=g)
    means[0] = 0.0
    stds = 10 ** (-4 + 3.5 * torch.rand(N, G, generator=g))      # saturated and active erf damping
    return means, stds


if __name__ == '__main__':
    ref = ref_import.load()
    torch.set_num_threads(1)              # fixed reduction order for the generating run
    spec = rm.make_spec('tiny')
    sd = rm.init_state(spec, seed=SEED)
    model, _ = ref_import.build_reference_model(ref, spec, sd)
    model.eval()
    means, stds = points()
    out = dict(seed=torch.tensor(SEED), checksum=torch.tensor(mg.state_checksum(sd), dtype=torch.float64), means=means, stds=stds)
    for name, mlp in (('nerf', model.nerf_mlp), ('prop', model.prop_mlp_0)):
        mlp.disable_density_normals = False           # the class default (models.py:391); ref_import binds True as waymo.gin does
        res = mlp(False, means.clone(), stds.clone(), viewdirs=None, no_warp=True)
        g, n = res['raw_grad_density'].detach(), res['normals'].detach()
        assert g.shape == (N, 3) and n.shape == (N, 3) and torch.isfinite(g).all() and torch.isfinite(n).all()
        assert float(g.abs().max()) > 0
        out[f'{name}_raw_grad_density'], out[f'{name}_normals'], out[f'{name}_density'] = g, n, res['density'].detach()
        out[f'{name}_coord'] = res['coord'].detach()
        print(f'{name}: |g| median {float(g.norm(dim=-1).median()):.3e} max {float(g.norm(dim=-1).max()):.3e}')
    mg.save('normals_tiny.npz', **mg.npify(out))
