// Predicted normals (models.py:442-444, :569-578, MLP.enable_pred_normals = True): normal_layer = Linear(bottleneck, 3) over the
// density layer's output x (before the GLO modulation), grad_pred = normal_layer(x), normals_pred = -l2_normalize(grad_pred)
// (DESIGN.md 7h).
//
// The inference kernels never materialise the bottleneck x = Wd1 h + bd1 (they compose Wd1 into the colour layers); the head composes
// the same way:
//     grad_pred = Wn (Wd1 h + bd1) + bn = A h + c,   h = relu(W0 feat + b0) [64],   A = Wn Wd1 [3, 64],   c = Wn bd1 + bn [3]
// A and c are formed once per call by the host side in fp32.  One pass after the level's field MLP, on its stream, over the
// level's feature buffer (which the MLP leaves as the gather wrote it): as k_density_feature_grad (march_normals.hip) the hidden
// layer is recomputed in plain fp32 from the UNPACKED density_layer.0 weights in every mlp_mode -- one function for the head, the
// one the reference evaluates -- with the weights in LDS (every lane reads the same word: a broadcast), one sample per thread and
// the hidden units in registers, 16 at a time (see the kernel); ~2 F * 64 + 6 * 64 FLOP per sample, 24 bytes written.
#include "ucn_common.h"

namespace {

// density_layer.0's width (models.py:438-441); see march_normals.hip: nothing in ucn_field_t carries it
constexpr uint32_t kHidden = 64;

// features: [P][B][C] planes (P = num_levels + n_scale_planes), b = ray * S + s (layout 0) or s * N + ray (layout 2); outputs [ray][s][3]
template <uint32_t C>
__global__ __launch_bounds__(256) void k_pred_normals(const float *__restrict__ w0, const float *__restrict__ b0,
                                                      const float *__restrict__ A, const float *__restrict__ c3, uint32_t P,
                                                      const float *__restrict__ features, uint32_t N, uint32_t S, int layout,
                                                      float *__restrict__ grad_pred_out, float *__restrict__ normals_out) {
    extern __shared__ float s_w[];                                  // [64][F] W0, then b0 [64], A [3][64], c [3]
    const uint32_t F = P * C;
    float *s_b = s_w + kHidden * F, *s_a = s_b + kHidden, *s_c = s_a + 3u * kHidden;
    for (uint32_t i = threadIdx.x; i < kHidden * F; i += 256u) s_w[i] = w0[i];
    if (threadIdx.x < kHidden) s_b[threadIdx.x] = b0[threadIdx.x];
    if (threadIdx.x < 3u * kHidden) s_a[threadIdx.x] = A[threadIdx.x];
    if (threadIdx.x < 3u) s_c[threadIdx.x] = c3[threadIdx.x];
    __syncthreads();
    const size_t B = (size_t)N * S;
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    // The hidden units in chunks of kChunk: with all 64 in one plane loop the compiler issues a whole plane's 64 x C LDS reads ahead
    // of the FMAs and the kernel takes 256 VGPRs (one wave per SIMD).  A chunk holds kChunk accumulators and kChunk x C weight words;
    // the sample's features are read once per chunk (the same cache lines).  Every h_k and g_j sums its terms in the same order as before.
    constexpr uint32_t kChunk = 16;
    float g0 = s_c[0], g1 = s_c[1], g2 = s_c[2];
#pragma unroll 1
    for (uint32_t k0 = 0; k0 < kHidden; k0 += kChunk) {
        float h[kChunk];
#pragma unroll
        for (uint32_t k = 0; k < kChunk; k++) h[k] = s_b[k0 + k];
        const float *wk = s_w + k0 * F;
#pragma unroll 1
        for (uint32_t p = 0; p < P; p++) {
            float f[C];
            const float *fp = features + ((size_t)p * B + b) * C;
#pragma unroll
            for (uint32_t c = 0; c < C; c++) f[c] = fp[c];
#pragma unroll
            for (uint32_t k = 0; k < kChunk; k++)
#pragma unroll
                for (uint32_t c = 0; c < C; c++) h[k] = fmaf(wk[k * F + p * C + c], f[c], h[k]);
        }
#pragma unroll
        for (uint32_t k = 0; k < kChunk; k++) {
            const float r = fmaxf(h[k], 0.0f);
            g0 = fmaf(s_a[k0 + k], r, g0);
            g1 = fmaf(s_a[kHidden + k0 + k], r, g1);
            g2 = fmaf(s_a[2u * kHidden + k0 + k], r, g2);
        }
    }
    size_t o = b;
    if (layout == 2) {
        const uint32_t s = (uint32_t)(b / N), ray = (uint32_t)(b - (size_t)s * N);
        o = (size_t)ray * S + s;
    }
    // ref_utils.l2_normalize = F.normalize(eps = float32 eps): x / max(|x|, eps), negated
    const float den = fmaxf(sqrtf((g0 * g0 + g1 * g1) + g2 * g2), UCN_EPS);
    grad_pred_out[o * 3 + 0] = g0; grad_pred_out[o * 3 + 1] = g1; grad_pred_out[o * 3 + 2] = g2;
    normals_out[o * 3 + 0] = -(g0 / den); normals_out[o * 3 + 1] = -(g1 / den); normals_out[o * 3 + 2] = -(g2 / den);
}

}  // namespace

extern "C" int ucn_pred_normals(const ucn_field_t *f, const float *A, const float *c, const float *features, uint32_t N, uint32_t S,
                                int layout, float *grad_pred_out, float *normals_pred_out, ucn_stream_t stream) {
    UCN_REQUIRE(f && f->w_d0 && f->b_d0, "pred_normals: the field's density_layer.0 pointers are missing");
    UCN_REQUIRE(f->num_levels >= 1 && f->num_levels <= UCN_MAX_LEVELS, "pred_normals: num_levels must be in [1,%d], got %u",
                UCN_MAX_LEVELS, f->num_levels);
    const uint32_t C = f->level_dim, P = f->num_levels + f->n_scale_planes;
    UCN_REQUIRE(C == 1 || C == 2 || C == 4 || C == 8, "GridEncoding: C must be 1, 2, 4, or 8.");
    UCN_REQUIRE(layout == 0 || layout == 2, "pred_normals: layout must be 0 or 2");
    if (N == 0 || S == 0) return 0;
    UCN_REQUIRE(A && c && features && grad_pred_out && normals_pred_out, "pred_normals: null pointer argument");
    const size_t B = (size_t)N * S;
    UCN_REQUIRE(B <= 0xFFFFFF00ull, "pred_normals: too many samples in one call (%zu)", B);
    const size_t lds = ((size_t)kHidden * P * C + 4u * kHidden + 3u) * sizeof(float);
    UCN_REQUIRE(lds <= 64u * 1024u, "pred_normals: %u features do not fit the weight tile", P * C);
    ucn_for_level_dim(C, [&](auto cc) {
        hipLaunchKernelGGL(k_pred_normals<decltype(cc)::value>, dim3(ucn_div_up(B, 256)), dim3(256), lds, (hipStream_t)stream, f->w_d0,
                           f->b_d0, A, c, P, features, N, S, layout, grad_pred_out, normals_pred_out);
    });
    UCN_LAUNCH_CHECK("pred_normals");
    return 0;
}
