"""torch-CPU restatement of `MLP.predict_density`'s graph that differentiates with respect to POSITIONS (ref models.py:485-512,
:546-567: density normals, disable_density_normals = False), on top of oracle/raymarch.py.

TEST INFRASTRUCTURE ONLY.  oracle/raymarch.py's grid (_GridEncodeCPU) has no input gradient, so the hash / tiled trilinear grid is
restated here with torch indexing on `FieldSpec.layout()` (addressing: oracle/grid_numpy.rows_of); contraction, damping and the
density layers are raymarch.py's.  It runs in float32 and in float64; the normals are autograd's:
    raw_grad_density = mean_j d raw_density / d means[..., j, :]      (stds held constant, gradient through the contraction too)
    normals          = -F.normalize(raw_grad_density, eps = float32 eps)                                   (ref_utils.l2_normalize)

The cell a point falls in is a discrete choice.  Like the reference's kernel (gridencoder.cu:141-150, "always use float"), both
runs take pos = fmaf(float32(u), scale, 0.5), its floor and its fraction from FLOAT32 arithmetic on their own u rounded to
float32; the fraction then enters the run's dtype with d frac / d u = scale.  The two runs so differ only in rounding -- and in
the cell, where the float32 rounding of u puts a point on the other side of a lattice plane (`cells`: callers leave those out).

`contract_points` below is raymarch.contract_points with the cube root evaluated on a safe argument inside the unit ball:
torch.where passes a zero gradient into the branch it does not take, and 0 * d pow(negative, 1/3) is NaN.  Forward values are
identical (tests/test_normals_cpu.py).

Note on the reference: its coord.track_linearize is decorated @torch.no_grad (coord.py:75), so with warp_fn = 'contract' the
contracted means it hands to the grid carry no graph back to `means`.  The semantics restated here are the ones the feature was
specified with: the derivative of the same forward function through the contraction.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import grid_numpy as gn
from oracle import raymarch as rm

EPS = rm.EPS


def contract_points(mean, std):
    """rm.contract_points (coord.py:60-72), safe to differentiate at every point."""
    m = (mean ** 2).sum(dim=-1, keepdim=True).clamp_min(EPS)
    inside = m <= 1
    m_out = torch.where(inside, torch.ones_like(m), m)            # the outside formulas never see an inside point
    root = torch.sqrt(m_out)
    z = torch.where(inside, mean, ((2 * root - 1) / m_out) * mean)
    shrink = (torch.pow(2 * root - 1, 1 / 3) / root) ** 2
    s = torch.where(inside[..., 0], std, shrink[..., 0] * std)
    return z, s


def locate(fs, u):
    """u [P, 3] of any dtype -> per level (cell int64 [P, 3], frac float32 [P, 3], scale, rows, res): the kernel's float32 locate."""
    pls, offsets, _, _ = fs.layout()
    scale, res, rows = gn.level_geometry(offsets.numpy(), np.log2(pls), fs.grid_base_resolution)
    u32 = u.detach().to(torch.float32).numpy()
    out = []
    for l in range(len(scale)):
        p = gn._fma(u32, np.broadcast_to(scale[l], u32.shape), np.broadcast_to(np.float32(0.5), u32.shape))
        cell = np.floor(p)
        out.append((cell.astype(np.int64), (p - cell.astype(np.float32)).astype(np.float32), float(scale[l]), rows[l], res[l]))
    return out, offsets


def grid_encode(fs, emb, u, dtype, exact_frac=False):
    """u [P, 3] in [0, 1] (dtype, may require grad) -> (features [P, L, C] like GridEncoder.forward's unflattened output, cells
    [L, P, 3]).  Trilinear weights in gridencoder.cu's product order; points outside [0, 1]^3 give zeros (gridencoder.cu:110-135).
    exact_frac: the fraction is u * scale + 0.5 - cell in `dtype` (a function finite differences can probe: gradcheck)."""
    levels, offsets = locate(fs, u)
    oob = ((u.detach() < 0) | (u.detach() > 1)).any(dim=-1)
    feats, cells = [], []
    for l, (cell, frac32, scale, rows, res) in enumerate(levels):
        us = u * scale
        if exact_frac:
            frac = us + 0.5 - torch.from_numpy(cell).to(dtype)
        else:
            frac = torch.from_numpy(frac32).to(dtype) + (us - us.detach())      # value: float32's; derivative: scale
        tab = emb[int(offsets[l]):int(offsets[l + 1])].to(dtype)
        acc = 0
        for k in range(8):
            w = 1
            corner = cell.copy()
            for d in range(3):
                if k & (1 << d):
                    w = w * frac[:, d]
                    corner[:, d] += 1
                else:
                    w = w * (1 - frac[:, d])
            with np.errstate(over='ignore'):
                r = gn.rows_of(corner.astype(np.uint32), rows, res)
            acc = acc + w[:, None] * tab[torch.from_numpy(r.astype(np.int64))]
        feats.append(torch.where(oob[:, None], torch.zeros_like(acc), acc))
        cells.append(torch.from_numpy(cell))
    return torch.stack(feats, dim=1), torch.stack(cells, dim=0)


def density_layers(fs, sd, feat, dtype):
    """feat [..., L*C] -> (raw_density [...], h [..., 64] pre-activation, bound [..., 64]: the float32 error bound of h's own sum,
    n eps (|b| + sum |W| |f|) with n = L*C + 1 terms)."""
    W0, b0 = sd[fs.prefix + '.density_layer.0.weight'].to(dtype), sd[fs.prefix + '.density_layer.0.bias'].to(dtype)
    W1, b1 = sd[fs.prefix + '.density_layer.2.weight'].to(dtype), sd[fs.prefix + '.density_layer.2.bias'].to(dtype)
    h = F.linear(feat, W0, b0)
    raw = F.linear(F.relu(h), W1[:1], b1[:1])[..., 0]
    bound = (W0.shape[1] + 1) * EPS * (b0.abs() + F.linear(feat.detach().abs(), W0.abs()))
    return raw, h, bound


def predict_density(fs, sd, means, stds, dtype=torch.float32, no_warp=False, exact_frac=False):
    """ref models.py:485-512 in `dtype`.  means [..., G, 3], stds [..., G] -> (raw_density [...], aux) with aux: feat [..., L*C],
    h / bound [..., 64], cells [L, P, 3] (P = the flattened points), coord [..., 3]."""
    _, _, grid_sizes, _ = fs.layout()
    x, s = means.to(dtype), stds.to(dtype)
    if not no_warp:
        z, s2 = contract_points(x.reshape(-1, 3), s.reshape(-1))
        x, s = z.reshape(x.shape) / 2, s2.reshape(s.shape) / 2
    u = ((x + 1) / 2).reshape(-1, 3)
    feat, cells = grid_encode(fs, sd[fs.prefix + '.encoder.embeddings'], u, dtype, exact_frac)
    feat = feat.reshape(x.shape[:-1] + feat.shape[1:])                              # [..., G, L, C]
    damp = rm.level_damping(s, grid_sizes)
    feat = (feat * damp[..., None]).mean(dim=-3).flatten(-2, -1)
    raw, h, bound = density_layers(fs, sd, feat, dtype)
    return raw, dict(feat=feat, h=h, bound=bound, cells=cells, coord=x.mean(dim=-2))


def normals(fs, sd, means, stds, dtype=torch.float32, no_warp=False):
    """ref models.py:550-567 -> dict(raw, raw_grad_density [..., 3], normals [..., 3], cells, h, bound, feat), detached."""
    m = means.detach().to(dtype).clone().requires_grad_(True)
    with torch.enable_grad():
        raw, aux = predict_density(fs, sd, m, stds.detach(), dtype, no_warp)
        (g,) = torch.autograd.grad(raw, m, torch.ones_like(raw))
    g = g.mean(dim=-2)
    n = -F.normalize(g, dim=-1, eps=EPS)
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in aux.items()}
    out.update(raw=raw.detach(), raw_grad_density=g, normals=n)
    return out


def cells_agree(c32, c64, B, G):
    """cells [L, B*G, 3] of the two runs -> bool [B]: every (j, l) of the sample fell in the same cell."""
    same = (c32 == c64).all(dim=-1).all(dim=0)
    return same.reshape(B, G).all(dim=-1)


def h_clear(h, bound):
    """bool [...]: no hidden unit of the sample is within the float32 error bound of zero (its ReLU mask is decided)."""
    return (h.abs() > bound).all(dim=-1)


def forward_choices(fs, sd, u, feat):
    """The two discrete choices as the FORWARD kernels made them, from their own outputs: u [P, 3] float32 grid coordinates
    (ucn_cast_probe / ucn_contract_probe: (c + 1) / 2) -> cells [L, P, 3] by the float32 locate; feat [B, L*C] (ucn_march_features /
    ucn_points_features) -> h [B, 64] in float64 on those features and the float32 error bound of its sum.  The gather rounds the
    contraction in another order than torch (contracted FMAs), so its u is now and then one ulp off the float32 restatement's; the
    gradient kernels take both choices from these inputs."""
    levels, _ = locate(fs, u)
    cells = torch.stack([torch.from_numpy(lv[0]) for lv in levels], dim=0)
    _, h, bound = density_layers(fs, sd, feat.double(), torch.float64)
    return cells, h, bound
