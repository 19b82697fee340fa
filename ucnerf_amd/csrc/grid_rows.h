// One multisample point in one level of the multi-resolution table: lattice cell, fractions, the 8 corner rows, their
// trilinear weights, and one row's load (gridencoder.cu:50-84, :146-180 for D = 3, linear, align_corners = false).
// Shared by the gather (march_features.hip) and the table gradient (march_features_bwd.hip): the gradient scatters
// to exactly the rows, with exactly the weights, that the gather read.  load_row also serves march_scale.hip's row sums.
// Shape (the gather is VALU-bound, see grid_cast.h):
//   * the level's addressing mode (xor-hash vs strided, pow2 mask vs modulo) is a TEMPLATE argument
//     chosen by a wave-uniform branch, not a per-corner select between two computed indices;
//   * y*P1 and z*P2 are multiplied once per point, the +1 corners add the prime (uint32 wrap keeps
//     (y+1)*P == y*P + P).
#pragma once
#include "ucn_common.h"

namespace {

constexpr uint32_t kP1 = 2654435761u, kP2 = 805459861u;   // gridencoder.cu:54

// One multisample point in one level: lattice cell, fractions, the 8 corner rows.
// gridencoder.cu:146-159 (locate) and :66-84 (index) for D = 3, linear, align_corners = false.
template <bool HASHED, bool POW2>
__device__ __forceinline__ void corner_rows(const UcnLevel &lv, float px, float py, float pz, float &fx, float &fy,
                                            float &fz, uint32_t (&rows)[8]) {
    fx = fmaf(px, lv.scale, 0.5f); fy = fmaf(py, lv.scale, 0.5f); fz = fmaf(pz, lv.scale, 0.5f);
    const uint32_t x0 = (uint32_t)floorf(fx), y0 = (uint32_t)floorf(fy), z0 = (uint32_t)floorf(fz);
    fx -= (float)x0; fy -= (float)y0; fz -= (float)z0;
    uint32_t ya, yb, za, zb, xa, xb;
    if constexpr (HASHED) {
        xa = x0; xb = x0 + 1u;
        ya = y0 * kP1; yb = ya + kP1;
        za = z0 * kP2; zb = za + kP2;
    } else {
        xa = x0 * lv.stride[0]; xb = xa + lv.stride[0];
        ya = y0 * lv.stride[1]; yb = ya + lv.stride[1];
        za = z0 * lv.stride[2]; zb = za + lv.stride[2];
    }
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t xv = (k & 1u) ? xb : xa, yv = (k & 2u) ? yb : ya, zv = (k & 4u) ? zb : za;
        uint32_t idx;
        if constexpr (HASHED) idx = xv ^ yv ^ zv;
        else idx = xv + yv + zv;
        if constexpr (POW2) rows[k] = idx & lv.mask;
        else rows[k] = idx < lv.rows ? idx : idx % lv.rows;
    }
}

// w_k = ((1*wx)*wy)*wz in the reference's multiplication order (gridencoder.cu:168-180)
__device__ __forceinline__ void corner_weights(float fx, float fy, float fz, float (&w)[8]) {
    const float gx = 1.0f - fx, gy = 1.0f - fy, gz = 1.0f - fz;
    const float w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
    w[0] = w00 * gz; w[1] = w10 * gz; w[2] = w01 * gz; w[3] = w11 * gz;
    w[4] = w00 * fz; w[5] = w10 * fz; w[6] = w01 * fz; w[7] = w11 * fz;
}

__device__ __forceinline__ bool in_unit_cube(float px, float py, float pz) {
    return !(px < 0.0f || px > 1.0f || py < 0.0f || py > 1.0f || pz < 0.0f || pz > 1.0f);   // gridencoder.cu:110-135
}

// One table row -> C floats.  TT = float (the fp32 tables of rendering and of the fp32 training path) or _Float16: under
// autocast the reference gathers a HALF copy of the table (grid.py:41-44: `embeddings.to(torch.half)` whenever autocast is on
// and C is even) -- half the bytes per corner, and a 2 MiB level slice that fits an XCD's L2 beside the streaming traffic.
// The interpolation arithmetic stays fp32 here (the reference's is half: this side is the more exact one).
template <uint32_t C, typename TT>
__device__ __forceinline__ void load_row(const TT *__restrict__ tab, uint32_t row, float (&v)[C]) {
    const TT *r = tab + (size_t)row * C;
    if constexpr (sizeof(TT) == 4) {
        if constexpr (C == 2) {
            const float2 t = *reinterpret_cast<const float2 *>(r);
            v[0] = t.x; v[1] = t.y;
        } else if constexpr (C == 4) {
            const float4 t = *reinterpret_cast<const float4 *>(r);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
            for (uint32_t c = 0; c < C; c++) v[c] = (float)r[c];
        }
    } else {
        typedef _Float16 hx2 __attribute__((ext_vector_type(2)));
        typedef _Float16 hx4 __attribute__((ext_vector_type(4)));
        if constexpr (C == 2) {
            const hx2 t = *reinterpret_cast<const hx2 *>(r);
            v[0] = (float)t[0]; v[1] = (float)t[1];
        } else if constexpr (C == 4) {
            const hx4 t = *reinterpret_cast<const hx4 *>(r);
            v[0] = (float)t[0]; v[1] = (float)t[1]; v[2] = (float)t[2]; v[3] = (float)t[3];
        } else {
#pragma unroll
            for (uint32_t c = 0; c < C; c++) v[c] = (float)r[c];
        }
    }
}

}  // namespace
