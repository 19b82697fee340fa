// A small head on the density layer's hidden units: g = A h + c,  h = relu(W0 feat + b0) [64],  A [R, 64] a head composed with
// density_layer.2 by the host.  Shared by ucn_pred_normals (pred_normals.hip, R = 3) and ucn_ref_heads (ref_colour.hip,
// R = 7).  The hidden layer is recomputed in plain fp32 from the UNPACKED density_layer.0 weights (ucn_field_t::w_d0 / b_d0) in every
// mlp_mode -- one function for a head, the one the reference evaluates -- with the weights in LDS (every lane reads the same word: a
// broadcast), one sample per thread and the hidden units in registers, kHiddenChunk at a time; ~2 F * 64 + 2 R * 64 FLOP per sample.
#pragma once
#include "ucn_common.h"

namespace {

// density_layer.0's width (models.py:438-441).  Nothing in ucn_field_t carries it: the host builds density_layer as 64 -> 1 + bottleneck
// for every field (internal/models.py), w_d0 is read as [64][F] and row 0 of w_d1 as 64 floats; a field of another width needs
// the width in the ABI first.
constexpr uint32_t kHidden = 64;
// The hidden units in chunks of kHiddenChunk: with all 64 in one plane loop the compiler issues a whole plane's 64 x C LDS reads ahead
// of the FMAs and the kernel takes 256 VGPRs (one wave per SIMD).  A chunk holds kHiddenChunk accumulators and kHiddenChunk x C weight
// words; the sample's features are read once per chunk (the same cache lines).  Every h_k and g_j sums its terms in the order of the
// unchunked loops.
constexpr uint32_t kHiddenChunk = 16;

// the dynamic LDS of a 256-thread workgroup: [64][F] W0, then b0 [64], then the caller's own floats
struct HiddenLds { const float *w, *b; float *rest; };

// W0 and b0 into LDS.  No barrier: the caller stages its A / c behind them (`rest`) and syncs once.
__device__ __forceinline__ HiddenLds stage_hidden(const float *__restrict__ w0, const float *__restrict__ b0, uint32_t F) {
    extern __shared__ float s_w[];
    float *s_b = s_w + kHidden * F;
    for (uint32_t i = threadIdx.x; i < kHidden * F; i += 256u) s_w[i] = w0[i];
    if (threadIdx.x < kHidden) s_b[threadIdx.x] = b0[threadIdx.x];
    return {s_w, s_b, s_b + kHidden};
}

// g = c + A relu(W0 feat_b + b0) for sample b of features [P][B][C]; s_a [R][64], s_c [R] in LDS
template <uint32_t C, uint32_t R>
__device__ __forceinline__ void hidden_rows(const HiddenLds &s, const float *s_a, const float *s_c, uint32_t P,
                                            const float *__restrict__ features, size_t B, size_t b, float (&g)[R]) {
    const uint32_t F = P * C;
#pragma unroll
    for (uint32_t j = 0; j < R; j++) g[j] = s_c[j];
#pragma unroll 1
    for (uint32_t k0 = 0; k0 < kHidden; k0 += kHiddenChunk) {
        float h[kHiddenChunk];
#pragma unroll
        for (uint32_t k = 0; k < kHiddenChunk; k++) h[k] = s.b[k0 + k];
        const float *wk = s.w + k0 * F;
#pragma unroll 1
        for (uint32_t p = 0; p < P; p++) {
            float f[C];
            const float *fp = features + ((size_t)p * B + b) * C;
#pragma unroll
            for (uint32_t c = 0; c < C; c++) f[c] = fp[c];
#pragma unroll
            for (uint32_t k = 0; k < kHiddenChunk; k++)
#pragma unroll
                for (uint32_t c = 0; c < C; c++) h[k] = fmaf(wk[k * F + p * C + c], f[c], h[k]);
        }
#pragma unroll
        for (uint32_t k = 0; k < kHiddenChunk; k++) {
            const float r = fmaxf(h[k], 0.0f);
#pragma unroll
            for (uint32_t j = 0; j < R; j++) g[j] = fmaf(s_a[j * kHidden + k0 + k], r, g[j]);
        }
    }
}

// ray * S + s of sample b = ray * S + s (layout 0) or s * N + ray (layout 2)
__device__ __forceinline__ size_t ray_major_index(size_t b, uint32_t N, uint32_t S, int layout) {
    if (layout != 2) return b;
    const uint32_t s = (uint32_t)(b / N), ray = (uint32_t)(b - (size_t)s * N);
    return (size_t)ray * S + s;
}

// Host: the checks such an entry point makes (`who`: its messages' prefix); P, C, B = N * S and the LDS bytes of a workgroup that keeps
// `extra` floats of its own behind W0 and b0.  An empty call (B = 0) passes whatever its size: the entry point launches nothing.
static int hidden_rows_args(const char *who, const ucn_field_t *f, int layout, uint32_t N, uint32_t S, uint32_t extra, uint32_t *P,
                            uint32_t *C, size_t *B, size_t *lds) {
    UCN_REQUIRE(f && f->w_d0 && f->b_d0, "%s: the field's density_layer.0 pointers are missing", who);
    UCN_REQUIRE(f->num_levels >= 1 && f->num_levels <= UCN_MAX_LEVELS, "%s: num_levels must be in [1,%d], got %u", who, UCN_MAX_LEVELS,
                f->num_levels);
    *C = f->level_dim, *P = f->num_levels + f->n_scale_planes, *B = (size_t)N * S;
    *lds = ((size_t)kHidden * *P * *C + kHidden + extra) * sizeof(float);
    UCN_REQUIRE(*C == 1 || *C == 2 || *C == 4 || *C == 8, "GridEncoding: C must be 1, 2, 4, or 8.");
    UCN_REQUIRE(layout == 0 || layout == 2, "%s: layout must be 0 or 2", who);
    UCN_REQUIRE(*B <= 0xFFFFFF00ull, "%s: too many samples in one call (%zu)", who, *B);
    UCN_REQUIRE(*B == 0 || *lds <= 64u * 1024u, "%s: %u features do not fit the weight tile", who, *P * *C);
    return 0;
}

}  // namespace
