"""What the bf16 dense kernels read of a field's parameters (MFMA fragment streams, accumulator-order vectors, the view encoding): no
autograd; heads_bf16.py packs through it for training, `mixed_level` (march_infer.py) for the mixed-precision inference march."""
import torch

from .. import _lib
from . import dense_f32


def view_encoding(d, deg):
    """coord.py:214-225 pos_enc(min_deg=0, max_deg=deg, append_identity=True)."""
    scales = 2 ** torch.arange(0, deg, device=d.device)
    scaled = (d[..., None, :] * scales[:, None]).reshape(d.shape[:-1] + (-1,))
    return torch.cat([d, torch.sin(torch.cat([scaled, scaled + 0.5 * torch.pi], dim=-1))], dim=-1)


def rgb_activation(mlp, logits):
    """models.py:663-674: colours from the rgb layer's logits (sigmoid, widened by rgb_padding to both sides)."""
    return torch.sigmoid(mlp.rgb_premultiplier * logits + mlp.rgb_bias) * (1 + 2 * mlp.rgb_padding) - mlp.rgb_padding


# ------------------------------------------------------------------ fused bf16 forward of the NeRF field's dense layers
_FRAG_CACHE = {}


def _perm(r, g):
    """Feature (within a 32-wide tile) held by accumulator register r of wave half g (csrc/mfma_chain.h acc_row)."""
    return (r & 3) + 8 * (r >> 2) + 4 * g


def _fragment_index(rows, cols, natural):
    """(row, col) of every element of a [rows, cols] weight's MFMA A-fragments in consumption order
    [out tile pair][in tile][k-step][tile of the pair][lane][8] (a single output tile: [in tile][k-step][lane][8]):
    lane (row = lane & 31, g = lane >> 5) element e is W[32 ot + row][32 it + k], k = 16 s + 8 g + e for the first
    layer (features arrive in natural order) and perm(8 s + e, g) for the others (the producing layer's accumulator
    order).  Positions beyond the matrix (tile padding) come back as row = -1."""
    nto, nti = (rows + 31) // 32, (cols + 31) // 32
    p = 1 if nto == 1 else 2                                  # output tiles in pairs, the pair innermost (csrc/field_train.hip)
    assert nto % p == 0
    otp, it, s_, o2, lane, e = torch.meshgrid(torch.arange(nto // p), torch.arange(nti), torch.arange(2), torch.arange(p),
                                              torch.arange(64), torch.arange(8), indexing="ij")
    row, g = 32 * (p * otp + o2) + (lane & 31), lane >> 5
    col = 32 * it + (16 * s_ + 8 * g + e if natural else _perm(8 * s_ + e, g))
    valid = (row < rows) & (col < cols)
    return torch.where(valid, row, torch.full_like(row, -1)).reshape(-1), col.reshape(-1)


def _pack_fragments(weights, device, total=0):
    """bf16 fragment stream of [(W, natural_k_order), ...]: ONE gather from the concatenated matrices (+ a zero slot
    for the tile padding and the stream's tail); the gather index depends only on the shapes and is cached."""
    key = ("pack", tuple((tuple(W.shape), tuple(W.stride()), nat) for W, nat in weights), total, str(device))
    idx = _FRAG_CACHE.get(key)
    if idx is None:
        parts, off = [], 0
        for W, nat in weights:
            r, c = _fragment_index(W.shape[0], W.shape[1], nat)
            parts.append(torch.where(r >= 0, off + r * W.shape[1] + c, torch.full_like(r, -1)))
            off += W.numel()
        flat = torch.cat(parts)
        if total * 512 > flat.numel():
            flat = torch.cat([flat, flat.new_full((total * 512 - flat.numel(),), -1)])
        idx = torch.where(flat >= 0, flat, torch.full_like(flat, off)).to(device)      # `off` = the zero slot
        _FRAG_CACHE[key] = idx
    src = torch.cat([W.reshape(-1) for W, _ in weights] + [weights[0][0].new_zeros(1)])
    return src[idx]


def _acc_order(width, device):
    """Column permutation that puts a [.., width] vector into accumulator order [tile][wave half][16]."""
    key = ("acc", width, str(device))
    hit = _FRAG_CACHE.get(key)
    if hit is None:
        t, g, r = torch.meshgrid(torch.arange((width + 31) // 32), torch.arange(2), torch.arange(16), indexing="ij")
        hit = (32 * t + _perm(r, g)).reshape(-1).to(device)
        _FRAG_CACHE[key] = hit
    return hit


def _acc_vec(v, width, device):
    pad = torch.zeros(v.shape[:-1] + (32 * ((width + 31) // 32),), device=device, dtype=torch.float32)
    pad[..., :v.shape[-1]] = v
    return pad[..., _acc_order(width, device)].contiguous()


# Column layout of the one activation buffer ucn_train_fwd writes per sample (bf16 [M, ACT_LD]): adjacent blocks are the
# concatenated inputs of the reference's layers, so each layer's whole weight gradient -- per-sample blocks, the per-ray
# direction block AND the bias (the constant-1 column of `aux`) -- is ONE split-K GEMM on a strided view:
#   [ h2 | h1 | x | aux = (dir_enc(27), 1, 0, 0, 0, 0) | h0 | bf16 copy of the features (<= 64) | pad ]     rows of 2 KiB:
#   a row that does not start on a 128-byte line (864 columns) costs the forward kernel 15 %
#     d1^T [h1 | x | aux] = [gW1h | gW1x | gW1e | gb1]  (models.py:620-640: lin_second_stage_1 over cat([h1, x, enc]))
#     d0^T [x | aux]      = [gW0x | gW0e | gb0],      gx^T [aux | h0] -> gb_d1 (column 27), gW_d1 (columns 32..95)
_ACT_H2, _ACT_H1, _ACT_X, _ACT_AUX, _ACT_H0, _ACT_FB, ACT_LD = 0, 256, 512, 768, 800, 864, 1024


def _weave(parts, producer, consumer):
    """Fragment lists of consecutive layers -> the same lists with parts[producer] (4 output-tile PAIRS) and
    parts[consumer] (whose 8 input tiles are those output tiles) cut into quarters and alternated: pair 0 of the
    producer, the consumer's fragments for input tiles 0-1, pair 1, input tiles 2-3, ..."""
    a, b = parts[producer], parts[consumer]
    assert a.numel() % 4 == 0 and b.numel() % 4 == 0 and consumer == producer + 1
    qa, qb = a.reshape(4, -1), b.reshape(4, -1)
    woven = torch.cat([torch.cat([qa[p], qb[p]]) for p in range(4)])
    return parts[:producer] + [woven] + parts[consumer + 1:]


def _head_gather_index(F_in, NB, NW, E, total, device, dir_in_stream=False):
    """ONE gather index over the flat bf16 copy of (Wd0, Wd1, W0, W1, Wr, bd0, bd1, b0', b1', br, W0x Wd1, W1x Wd1, 0) -- the
    colour layers composed with the activation-free bottleneck and W bd1 folded into their biases -- that yields, in this
    order: the forward fragment stream, the dgrad (transposed) fragment stream, the direction blocks of W0 / W1 with
    rows in accumulator order [2 NW, E], their biases [2 NW], and bd0 / bd1 / br in accumulator order (64 + NB + 32).
    A logical matrix is a list of column blocks (base, row_stride, col_stride, ncols) of the flat source."""
    key = ("heads", F_in, NB, NW, E, total, str(device), dir_in_stream)
    hit = _FRAG_CACHE.get(key)
    if hit is not None:
        return hit
    k0, k1 = NB + E, NW + NB + E
    oWd0 = 0
    oWd1 = oWd0 + 64 * F_in
    oW0 = oWd1 + NB * 64
    oW1 = oW0 + NW * k0
    oWr = oW1 + NW * k1
    obd0 = oWr + 3 * NW
    obd1, ob0, ob1, obr = obd0 + 64, obd0 + 64 + NB, obd0 + 64 + NB + NW, obd0 + 64 + NB + 2 * NW
    oWc0 = obr + 3
    oWc1 = oWc0 + NW * 64
    zero = oWc1 + NW * 64

    def stream(mats, weave):
        parts = []
        for rows, blocks, nat in mats:
            cols = sum(b[3] for b in blocks)
            r, c = _fragment_index(rows, cols, nat)
            off = torch.full_like(r, -1)
            start = 0
            for base, rs, cs, nc in blocks:
                inside = (r >= 0) & (c >= start) & (c < start + nc)
                off = torch.where(inside, base + r * rs + (c - start) * cs, off)
                start += nc
            parts.append(off)
        parts = _weave(parts, *weave)
        flat = torch.cat(parts)
        assert flat.numel() <= total * 512
        return torch.cat([flat, flat.new_full((total * 512 - flat.numel(),), -1)])

    # forward: the rgb layer's fragments ride behind each pair of the last hidden layer's output tiles; backward: the
    # density layer's behind each pair of bottleneck-gradient tiles (field_train.hip: the consumer layer runs on every
    # finished pair, so that only one pair of accumulators is live and two workgroups fit a CU)
    # dir_in_stream (inference with rays-fastest lanes): the direction block, the layer bias (against the constant-1 column of
    # the ray's tile) and zero padding form one more 32-column input tile of the two colour layers
    aux0 = [(oW0 + NB, k0, 1, E), (ob0, 1, 0, 1), (zero, 0, 0, 31 - E)] if dir_in_stream else []
    aux1 = [(oW1 + NW + NB, k1, 1, E), (ob1, 1, 0, 1), (zero, 0, 0, 31 - E)] if dir_in_stream else []
    fwd = stream([(64, [(oWd0, F_in, 1, F_in)], True), (NB, [(oWd1, 64, 1, 64)], False), (NW, [(oWc0, 64, 1, 64)] + aux0, False),
                  (NW, [(oW1, k1, 1, NW), (oWc1, 64, 1, 64)] + aux1, False), (3, [(oWr, NW, 1, NW)], False)], weave=(3, 4))
    bwd = stream([(NW, [(oWr, 1, NW, 3)], True), (NW, [(oW1, 1, k1, NW)], False),
                  (NB, [(oW1 + NW, 1, k1, NW), (oW0, 1, k0, NW)], False), (64, [(oWd1, 1, 64, NB)], False),
                  (F_in, [(oWd0, 1, F_in, 64)], False)], weave=(2, 3))
    acc_w, acc_b, acc_64 = _acc_order(NW, "cpu"), _acc_order(NB, "cpu"), _acc_order(64, "cpu")
    e = torch.arange(E)
    we = torch.cat([(oW0 + acc_w[:, None] * k0 + NB + e[None, :]).reshape(-1),
                    (oW1 + acc_w[:, None] * k1 + NW + NB + e[None, :]).reshape(-1)])
    be = torch.cat([ob0 + acc_w, ob1 + acc_w])
    a32 = _acc_order(32, "cpu")
    bv = torch.cat([obd0 + acc_64, obd1 + acc_b, torch.where(a32 < 3, obr + a32, torch.full_like(a32, -1))])
    idx = torch.cat([fwd, bwd, we, be, bv])
    hit = (torch.where(idx >= 0, idx, torch.full_like(idx, zero)).to(device), zero + 1)
    _FRAG_CACHE[key] = hit
    return hit


def prepare_heads(Wd0, bd0, Wd1, bd1, W0, b0, W1, b1, Wr, br, dir_in_stream=False):
    """Everything ucn_train_fwd / ucn_train_bwd need from the NeRF field's dense parameters, as ONE cat + ONE cast + ONE gather:
    (forward fragment stream, dgrad fragment stream, direction blocks [2 NW, E] and their biases [2 NW] in accumulator
    order (bf16), bd0 / bd1 / br in accumulator order (fp32)).  The colour layers enter the forward stream composed with
    the activation-free bottleneck (models.py:508): (W0x Wd1), [W1h | W1x Wd1], W bd1 folded into the biases."""
    lib = _lib.load()
    dev, dt = Wd0.device, torch.bfloat16
    NB, NW, F_in = Wd1.shape[0], W0.shape[0], Wd0.shape[1]
    E = W0.shape[1] - NB
    T = lib.ucn_train_fwd_fragments()
    idx, n_src = _head_gather_index(F_in, NB, NW, E, T, dev, dir_in_stream)
    zero = _FRAG_CACHE.get(("zero1", str(dev)))
    if zero is None:
        zero = _FRAG_CACHE[("zero1", str(dev))] = torch.zeros(1, device=dev)
    W0x32, W1x32, Wd132, bd132 = W0.detach()[:, :NB].float(), W1.detach()[:, NW:NW + NB].float(), Wd1.detach().float(), bd1.detach().float()
    Wd1t = Wd132.t().contiguous()                                    # (csrc/gemm_f32.hip: no library GEMM in the autocast step, r06)
    Wc0, Wc1 = dense_f32.gemm(W0x32.contiguous(), Wd1t), dense_f32.gemm(W1x32.contiguous(), Wd1t)
    b0c, b1c = torch.addmv(b0.detach().float(), W0x32, bd132), torch.addmv(b1.detach().float(), W1x32, bd132)
    src = torch.cat([t.detach().reshape(-1).float() for t in (Wd0, Wd1, W0, W1, Wr, bd0, bd1, b0c, b1c, br, Wc0, Wc1)] + [zero]).to(dt)
    assert src.numel() == n_src
    got = src[idx]
    packed, packed_t = got[:T * 512], got[T * 512:2 * T * 512]
    o = 2 * T * 512
    We = got[o:o + 2 * NW * E].view(2 * NW, E)
    be = got[o + 2 * NW * E:o + 2 * NW * E + 2 * NW]
    bv = got[o + 2 * NW * E + 2 * NW:].float()
    return packed, packed_t, We, be, bv[:64], bv[64:64 + NB], bv[64 + NB:]
