// Predicted normals (models.py:442-444, :569-578, MLP.enable_pred_normals = True): normal_layer = Linear(bottleneck, 3) over the
// density layer's output x (before the GLO modulation), grad_pred = normal_layer(x), normals_pred = -l2_normalize(grad_pred)
// (DESIGN.md 7h).
//
// The inference kernels never materialise the bottleneck x = Wd1 h + bd1 (they compose Wd1 into the colour layers); the head composes
// the same way:
//     grad_pred = Wn (Wd1 h + bd1) + bn = A h + c,   h = relu(W0 feat + b0) [64],   A = Wn Wd1 [3, 64],   c = Wn bd1 + bn [3]
// A and c are formed once per call by the host side in fp32.  One pass after the level's field MLP, on its stream, over the
// level's feature buffer (which the MLP leaves as the gather wrote it); the recompute of h and the three rows are hidden_rows.h's;
// 24 bytes written per sample.
#include "hidden_rows.h"

namespace {

// features: [P][B][C] planes (P = num_levels + n_scale_planes), b = ray * S + s (layout 0) or s * N + ray (layout 2); outputs [ray][s][3]
template <uint32_t C>
__global__ __launch_bounds__(256) void k_pred_normals(const float *__restrict__ w0, const float *__restrict__ b0,
                                                      const float *__restrict__ A, const float *__restrict__ c3, uint32_t P,
                                                      const float *__restrict__ features, uint32_t N, uint32_t S, int layout,
                                                      float *__restrict__ grad_pred_out, float *__restrict__ normals_out) {
    const HiddenLds lds = stage_hidden(w0, b0, P * C);              // then A [3][64], c [3]
    float *s_a = lds.rest, *s_c = s_a + 3u * kHidden;
    if (threadIdx.x < 3u * kHidden) s_a[threadIdx.x] = A[threadIdx.x];
    if (threadIdx.x < 3u) s_c[threadIdx.x] = c3[threadIdx.x];
    __syncthreads();
    const size_t B = (size_t)N * S;
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    float g[3];
    hidden_rows<C>(lds, s_a, s_c, P, features, B, b, g);
    const size_t o = ray_major_index(b, N, S, layout);
    // ref_utils.l2_normalize = F.normalize(eps = float32 eps): x / max(|x|, eps), negated
    const float den = fmaxf(sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]), UCN_EPS);
    grad_pred_out[o * 3 + 0] = g[0]; grad_pred_out[o * 3 + 1] = g[1]; grad_pred_out[o * 3 + 2] = g[2];
    normals_out[o * 3 + 0] = -(g[0] / den); normals_out[o * 3 + 1] = -(g[1] / den); normals_out[o * 3 + 2] = -(g[2] / den);
}

}  // namespace

extern "C" int ucn_pred_normals(const ucn_field_t *f, const float *A, const float *c, const float *features, uint32_t N, uint32_t S,
                                int layout, float *grad_pred_out, float *normals_pred_out, ucn_stream_t stream) {
    uint32_t P, C;
    size_t B, lds;
    if (int e = hidden_rows_args("pred_normals", f, layout, N, S, 3u * kHidden + 3u, &P, &C, &B, &lds)) return e;
    if (B == 0) return 0;
    UCN_REQUIRE(A && c && features && grad_pred_out && normals_pred_out, "pred_normals: null pointer argument");
    ucn_for_level_dim(C, [&](auto cc) {
        hipLaunchKernelGGL(k_pred_normals<decltype(cc)::value>, dim3(ucn_div_up(B, 256)), dim3(256), lds, (hipStream_t)stream, f->w_d0,
                           f->b_d0, A, c, P, features, N, S, layout, grad_pred_out, normals_pred_out);
    });
    UCN_LAUNCH_CHECK("pred_normals");
    return 0;
}
