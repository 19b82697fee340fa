// The Ref-NeRF colour heads (models.py:447-454, :589-597, :661-674; MLP.use_diffuse_color, use_specular_tint, enable_pred_roughness;
// DESIGN.md 7i): three Linear(bottleneck, .) heads over the density layer's output x (before the GLO modulation),
//     raw_diffuse = diffuse_layer(x) [3],   tint = sigmoid(specular_layer(x)) [3],   roughness = softplus(roughness_layer(x) + roughness_bias) [1]
// and, with the diffuse head, the colour MLP's sigmoid as a LINEAR specular colour:
//     l = (tint | 0.5) * sigmoid(premultiplier * logits + bias) + sigmoid(raw_diffuse - ln 3)
//     rgb = clip(linear_to_srgb(l), 0, 1) * (1 + 2 padding) - padding
//     linear_to_srgb(l) = 323/25 l  where l <= 0.0031308,  (211 max(l, float32 eps)^(5/12) - 11) / 200  otherwise      (image.py:31-39)
//
// ucn_ref_heads is the inference pass: the heads compose with density_layer.2 into A h + c on the hidden layer h = relu(W0 feat + b0),
// whose recompute and the seven rows are hidden_rows.h's.  ucn_ref_colour / _backward are the training graph's elementwise node.
// All arithmetic float32, powf / expf / log1pf the accurate library functions; no atomics, no workspace.
#include "hidden_rows.h"

namespace {

constexpr uint32_t kRows = 7;         // diffuse 3, tint 3, roughness 1: the rows of A in LDS (absent heads: zero rows)
constexpr float kLn3 = 1.09861228866810969f;
constexpr float kToe = 0.0031308f;
constexpr float kGamma = (float)(5.0 / 12.0), kGammaM1 = (float)(5.0 / 12.0 - 1.0);      // torch: a double scalar exponent, cast to the tensor's dtype

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
// F.softplus (beta 1, threshold 20)
__device__ __forceinline__ float softplusf_(float x) { return x > 20.0f ? x : log1pf(expf(x)); }

// clip(linear_to_srgb(l), 0, 1).  With g_l: *g_l = the gradient g of the clipped value carried to l in the order torch's autograd applies
// it (the clip passes on 0 <= srgb <= 1; where: the selected part only; / 200, * 211, the power's e x^(e-1); clamp_min passes on l >= eps)
__device__ __forceinline__ float srgb_clip(float l, float g = 0.0f, float *g_l = nullptr) {
    float srgb;
    if (l <= kToe) {
        srgb = (float)(323.0 / 25.0) * l;
        if (g_l) *g_l = (srgb >= 0.0f && srgb <= 1.0f) ? g * (float)(323.0 / 25.0) : 0.0f;
    } else {
        const float lc = fmaxf(l, UCN_EPS);
        srgb = (211.0f * powf(lc, kGamma) - 11.0f) / 200.0f;
        if (g_l) *g_l = (srgb >= 0.0f && srgb <= 1.0f && l >= UCN_EPS) ? ((g / 200.0f) * 211.0f) * (kGamma * powf(lc, kGammaM1)) : 0.0f;
    }
    return fminf(fmaxf(srgb, 0.0f), 1.0f);
}

// the final colour of one channel from the colour MLP's sigmoid s, the raw diffuse logit and the tint factor t (0.5 without the tint head)
__device__ __forceinline__ float ref_colour(float s, float raw_diffuse, float t, float padding) {
    const float l = t * s + sigmoidf_(raw_diffuse - kLn3);
    return srgb_clip(l) * (1.0f + 2.0f * padding) - padding;
}

// features: [P][B][C] planes (P = num_levels + n_scale_planes), b = ray * S + s (layout 0) or s * N + ray (layout 2); rgb [ray][s][3] in place,
// roughness_out [ray][s].  heads: bit 0 diffuse, bit 1 tint, bit 2 roughness; A holds the present heads' rows in that order.
template <uint32_t C>
__global__ __launch_bounds__(256) void k_ref_heads(const float *__restrict__ w0, const float *__restrict__ b0, const float *__restrict__ A,
                                                   const float *__restrict__ cvec, uint32_t P, uint32_t heads, float roughness_bias,
                                                   float padding, const float *__restrict__ features, uint32_t N, uint32_t S, int layout,
                                                   float *__restrict__ rgb, float *__restrict__ roughness_out) {
    const HiddenLds lds = stage_hidden(w0, b0, P * C);              // then A [7][64], c [7]
    float *s_a = lds.rest, *s_c = s_a + kRows * kHidden;
    const bool has_d = heads & 1u, has_t = (heads & 2u) && has_d, has_r = heads & 4u;      // the tint is read only beside the diffuse colour
    const uint32_t row_t = has_d ? 3u : 0u, row_r = row_t + ((heads & 2u) ? 3u : 0u);       // rows of A as the caller packed them
    for (uint32_t i = threadIdx.x; i < kRows * kHidden; i += 256u) {
        const uint32_t j = i / kHidden, k = i - j * kHidden;
        float v = 0.0f;
        if (j < 3u) { if (has_d) v = A[j * kHidden + k]; }
        else if (j < 6u) { if (has_t) v = A[(row_t + j - 3u) * kHidden + k]; }
        else if (has_r) v = A[row_r * kHidden + k];
        s_a[i] = v;
    }
    if (threadIdx.x < kRows) {
        const uint32_t j = threadIdx.x;
        float v = 0.0f;
        if (j < 3u) { if (has_d) v = cvec[j]; }
        else if (j < 6u) { if (has_t) v = cvec[row_t + j - 3u]; }
        else if (has_r) v = cvec[row_r];
        s_c[j] = v;
    }
    __syncthreads();
    const size_t B = (size_t)N * S;
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    float g[kRows];
    hidden_rows<C>(lds, s_a, s_c, P, features, B, b, g);
    const size_t o = ray_major_index(b, N, S, layout);
    if (has_d) {
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            const float t = has_t ? sigmoidf_(g[3 + k]) : 0.5f;
            rgb[o * 3 + k] = ref_colour(rgb[o * 3 + k], g[k], t, padding);
        }
    }
    if (has_r && roughness_out) roughness_out[o] = softplusf_(g[6] + roughness_bias);
}

// one thread per channel of [B, 3]
template <bool TINT>
__global__ __launch_bounds__(256) void k_ref_colour(const float *__restrict__ logits, const float *__restrict__ raw_diffuse,
                                                    const float *__restrict__ raw_tint, size_t M, float premult, float bias, float padding,
                                                    float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= M) return;
    const float s = sigmoidf_(premult * logits[i] + bias);
    const float t = TINT ? sigmoidf_(raw_tint[i]) : 0.5f;
    out[i] = ref_colour(s, raw_diffuse[i], t, padding);
}

template <bool TINT>
__global__ __launch_bounds__(256) void k_ref_colour_bwd(const float *__restrict__ logits, const float *__restrict__ raw_diffuse,
                                                        const float *__restrict__ raw_tint, const float *__restrict__ g_out, size_t M,
                                                        float premult, float bias, float padding, float *__restrict__ g_logits,
                                                        float *__restrict__ g_diffuse, float *__restrict__ g_tint) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= M) return;
    const float s = sigmoidf_(premult * logits[i] + bias);
    const float dl = sigmoidf_(raw_diffuse[i] - kLn3);
    const float t = TINT ? sigmoidf_(raw_tint[i]) : 0.5f;
    float g_l;                                                          // through the padding, the clip and the selected srgb part
    srgb_clip(t * s + dl, g_out[i] * (1.0f + 2.0f * padding), &g_l);
    // sigmoid's backward as torch forms it: (g (1 - y)) y
    g_diffuse[i] = (g_l * (1.0f - dl)) * dl;
    g_logits[i] = (((g_l * t) * (1.0f - s)) * s) * premult;
    if (TINT) g_tint[i] = ((g_l * s) * (1.0f - t)) * t;
}

}  // namespace

extern "C" int ucn_ref_heads(const ucn_field_t *f, const float *A, const float *c, uint32_t heads, float roughness_bias, float rgb_padding,
                             const float *features, uint32_t N, uint32_t S, int layout, float *rgb, float *roughness_out,
                             ucn_stream_t stream) {
    uint32_t P, C;
    size_t B, lds;
    if (int e = hidden_rows_args("ref_heads", f, layout, N, S, kRows * kHidden + 8u, &P, &C, &B, &lds)) return e;
    UCN_REQUIRE(heads >= 1 && heads <= 7, "ref_heads: heads must be a mask of 1 (diffuse), 2 (tint), 4 (roughness), got %u", heads);
    if (B == 0) return 0;
    UCN_REQUIRE(A && c && features, "ref_heads: null pointer argument");
    UCN_REQUIRE(!(heads & 1u) || rgb, "ref_heads: the diffuse head needs the rgb buffer");
    if (!(heads & 1u) && !((heads & 4u) && roughness_out)) return 0;         // a tint without the diffuse colour is never read (models.py:661-668)
    ucn_for_level_dim(C, [&](auto cc) {
        hipLaunchKernelGGL(k_ref_heads<decltype(cc)::value>, dim3(ucn_div_up(B, 256)), dim3(256), lds, (hipStream_t)stream, f->w_d0, f->b_d0,
                           A, c, P, heads, roughness_bias, rgb_padding, features, N, S, layout, rgb, roughness_out);
    });
    UCN_LAUNCH_CHECK("ref_heads");
    return 0;
}

extern "C" int ucn_ref_colour(const float *logits, const float *raw_diffuse, const float *raw_tint, uint64_t B, float rgb_premultiplier,
                              float rgb_bias, float rgb_padding, float *rgb_out, ucn_stream_t stream) {
    if (B == 0) return 0;
    UCN_REQUIRE(logits && raw_diffuse && rgb_out, "ref_colour: null pointer argument");
    UCN_REQUIRE(B <= 0x55555500ull, "ref_colour: too many samples in one call (%llu)", (unsigned long long)B);
    const size_t M = (size_t)B * 3;
    const dim3 grid(ucn_div_up(M, 256));
    if (raw_tint) hipLaunchKernelGGL(k_ref_colour<true>, grid, dim3(256), 0, (hipStream_t)stream, logits, raw_diffuse, raw_tint, M,
                                     rgb_premultiplier, rgb_bias, rgb_padding, rgb_out);
    else hipLaunchKernelGGL(k_ref_colour<false>, grid, dim3(256), 0, (hipStream_t)stream, logits, raw_diffuse, raw_tint, M,
                            rgb_premultiplier, rgb_bias, rgb_padding, rgb_out);
    UCN_LAUNCH_CHECK("ref_colour");
    return 0;
}

extern "C" int ucn_ref_colour_backward(const float *logits, const float *raw_diffuse, const float *raw_tint, const float *g_rgb, uint64_t B,
                                       float rgb_premultiplier, float rgb_bias, float rgb_padding, float *g_logits, float *g_diffuse,
                                       float *g_tint, ucn_stream_t stream) {
    if (B == 0) return 0;
    UCN_REQUIRE(logits && raw_diffuse && g_rgb && g_logits && g_diffuse, "ref_colour_backward: null pointer argument");
    UCN_REQUIRE((raw_tint == nullptr) == (g_tint == nullptr), "ref_colour_backward: raw_tint and g_tint come together");
    UCN_REQUIRE(B <= 0x55555500ull, "ref_colour_backward: too many samples in one call (%llu)", (unsigned long long)B);
    const size_t M = (size_t)B * 3;
    const dim3 grid(ucn_div_up(M, 256));
    if (raw_tint) hipLaunchKernelGGL(k_ref_colour_bwd<true>, grid, dim3(256), 0, (hipStream_t)stream, logits, raw_diffuse, raw_tint, g_rgb, M,
                                     rgb_premultiplier, rgb_bias, rgb_padding, g_logits, g_diffuse, g_tint);
    else hipLaunchKernelGGL(k_ref_colour_bwd<false>, grid, dim3(256), 0, (hipStream_t)stream, logits, raw_diffuse, raw_tint, g_rgb, M,
                            rgb_premultiplier, rgb_bias, rgb_padding, g_logits, g_diffuse, g_tint);
    UCN_LAUNCH_CHECK("ref_colour_backward");
    return 0;
}
