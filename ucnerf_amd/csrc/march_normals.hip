// Density normals (models.py:546-567, MLP.disable_density_normals = False): the gradient of the pre-activation density with
// respect to a sample's six multisample means, mean over the six, and its negated unit vector.
//
// Two passes after the level's field MLP:
//   1. k_density_feature_grad:  g[l][c] = d raw / d feat[l][c] = sum_k 1[h_k > 0] W1[0, k] W0[k, l*C + c],  h = W0 feat + b0,
//      recomputed in plain fp32 from the UNPACKED density_layer weights (ucn_field_t::w_d0 / b_d0 / w_d1) in every mlp_mode:
//      the split-f16 forward may round an h_k next to zero to the other side, and a gradient must belong to ONE function --
//      the fp32 one is the one the reference evaluates.  Weights in LDS (every lane reads the same word: a broadcast), one
//      sample per thread, h[64] in registers; ~13 kFLOP per sample beside the gather below.
//   2. k_march_density_grad / k_points_density_grad: a second gather over the tables.  The Gaussians are re-derived through
//      cast_sample / contract_to_unit (grid_cast.h), so the points are the forward's bit for bit.  Per multisample j and level l
//      the 8 corner rows are fetched once; with s_k = sum_c g[l][c] row_k[c] they give both the interpolated value
//      E = sum_k w_k s_k and its three partial derivatives (gridencoder.cu:199-243: differences of s over one axis weighted by the
//      other two axes' fractions, times the level's scale).  Accumulated per multisample over the levels, in fp32:
//          gu_j   += erf(a_jl) * scale_l * dE/dpos                     (path 1: through the interpolation)
//          gsig_j += E * (-(2/sqrt(pi)) a_jl exp(-a_jl^2))             (path 2: sigma_j * d erf(a_jl) / d sigma_j, a = 1/sqrt(8 sigma^2 gs^2))
//      and closed per multisample with the contraction's Jacobian (coord.py:43-57) and the derivative of its std factor
//      det_13(r) = ((2r - 1)^(1/3) / r)^2 (coord.py:60-72):
//          d raw / d x_j = (1/G) [ J^T gu_j / 4  +  gsig_j * (d ln det_13 / dr) * x_j / r ],     outside the unit ball,
//          d raw / d x_j = (1/G) gu_j / 4  inside it (J = 1, the std is not scaled; the clamp at the origin passes nothing).
//      One thread = one sample and ALL levels, ascending -- the order in which the gather's level groups are dispatched -- so that the
//      workgroups in flight on an XCD read one level's table slice at about the same time, and the 24 accumulators never leave
//      the thread: no atomics, one write of 6 floats per sample.
#include "ucn_common.h"
#include "grid_cast.h"
#include "grid_rows.h"
#include "hidden_rows.h"      // kHidden, density_layer.0's width; k_density_feature_grad keeps all 64 units live for its backward

namespace {

// features / gfeat: [L][B][C]; they may be the SAME buffer (a thread reads its sample's features before it writes them)
template <uint32_t C>
__global__ __launch_bounds__(256) void k_density_feature_grad(const float *__restrict__ w0, const float *__restrict__ b0,
                                                              const float *__restrict__ w1, uint32_t L, uint32_t ldw,
                                                              const float *features, size_t B, float *gfeat) {
    extern __shared__ float s_w[];                                  // [64][F] W0, then b0 [64], W1[0, :] [64]
    const uint32_t F = L * C;
    float *s_b = s_w + kHidden * F, *s_r = s_b + kHidden;
    for (uint32_t i = threadIdx.x; i < kHidden * F; i += 256u) s_w[i] = w0[(size_t)(i / F) * ldw + i % F];
    if (threadIdx.x < kHidden) { s_b[threadIdx.x] = b0[threadIdx.x]; s_r[threadIdx.x] = w1[threadIdx.x]; }
    __syncthreads();
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    float h[kHidden];
#pragma unroll
    for (uint32_t k = 0; k < kHidden; k++) h[k] = s_b[k];
    for (uint32_t l = 0; l < L; l++) {
        float f[C];
        const float *fp = features + ((size_t)l * B + b) * C;
#pragma unroll
        for (uint32_t c = 0; c < C; c++) f[c] = fp[c];
#pragma unroll
        for (uint32_t k = 0; k < kHidden; k++)
#pragma unroll
            for (uint32_t c = 0; c < C; c++) h[k] = fmaf(s_w[k * F + l * C + c], f[c], h[k]);
    }
#pragma unroll
    for (uint32_t k = 0; k < kHidden; k++) h[k] = h[k] > 0.0f ? s_r[k] : 0.0f;
    for (uint32_t l = 0; l < L; l++) {
        float g[C];
#pragma unroll
        for (uint32_t c = 0; c < C; c++) g[c] = 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < kHidden; k++)
#pragma unroll
            for (uint32_t c = 0; c < C; c++) g[c] = fmaf(h[k], s_w[k * F + l * C + c], g[c]);
        float *gp = gfeat + ((size_t)l * B + b) * C;
#pragma unroll
        for (uint32_t c = 0; c < C; c++) gp[c] = g[c];
    }
}

// one multisample point in one level: gu += erf(a) scale dE/dpos, gsig += E sigma d erf(a) / d sigma
template <uint32_t C, bool HASHED, bool POW2>
__device__ __forceinline__ void point_level_grad(const UcnLevel &lv, const float *__restrict__ tab, const float (&g)[C], float ux,
                                                 float uy, float uz, float rsj, float (&gu)[3], float &gsig) {
    float fx, fy, fz;
    uint32_t rows[8];
    corner_rows<HASHED, POW2>(lv, ux, uy, uz, fx, fy, fz, rows);
    float s[8];
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
        float v[C];
        load_row<C, float>(tab, rows[k], v);
        float t = 0.0f;
#pragma unroll
        for (uint32_t c = 0; c < C; c++) t = fmaf(g[c], v[c], t);
        s[k] = t;
    }
    float w[8];
    corner_weights(fx, fy, fz, w);
    float E = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) E = fmaf(w[k], s[k], E);
    const float gx = 1.0f - fx, gy = 1.0f - fy, gz = 1.0f - fz;
    // corner k: bit 0 = x + 1, bit 1 = y + 1, bit 2 = z + 1 (grid_rows.h)
    const float dx = (gy * gz) * (s[1] - s[0]) + (fy * gz) * (s[3] - s[2]) + (gy * fz) * (s[5] - s[4]) + (fy * fz) * (s[7] - s[6]);
    const float dy = (gx * gz) * (s[2] - s[0]) + (fx * gz) * (s[3] - s[1]) + (gx * fz) * (s[6] - s[4]) + (fx * fz) * (s[7] - s[5]);
    const float dz = (gx * gy) * (s[4] - s[0]) + (fx * gy) * (s[5] - s[1]) + (gx * fy) * (s[6] - s[2]) + (fx * fy) * (s[7] - s[3]);
    const float a = rsj * lv.inv_gs;
    // erff / expf, not the gather's erf_pos (|error| <= 1.5e-7 absolute): here the damping multiplies scale_l * dE/dpos, up to 5e5, and
    // that error was 6x the float32 restatement's own on unwarped points (tests/test_normals_gpu.py); ~60 VALU per point and level
    const float damp = erff(a) * lv.scale;
    gu[0] = fmaf(damp, dx, gu[0]); gu[1] = fmaf(damp, dy, gu[1]); gu[2] = fmaf(damp, dz, gu[2]);
    // a >= 10: exp(-a^2) < 4e-44, the term is zero in float32 (and a = inf for a zero std must not meet that zero)
    const float da = a < 10.0f ? a * expf(-(a * a)) : 0.0f;
    gsig = fmaf(E, -1.1283791670955126f * da, gsig);
}

template <uint32_t C>
__device__ __forceinline__ void density_grad_levels(const UcnLevels &lvls, const float *__restrict__ table,
                                                    const float *__restrict__ gfeat, size_t B, size_t b, const float (&u)[6][3],
                                                    const float (&rs)[6], uint32_t G, float (&gu)[6][3], float (&gsig)[6]) {
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) gu[j][0] = gu[j][1] = gu[j][2] = gsig[j] = 0.0f;
    for (uint32_t lvl = 0; lvl < lvls.L; lvl++) {
        const UcnLevel lv = lvls.lv[lvl];
        const float *tab = table + (size_t)lv.first_row * C;
        float g[C];
        const float *gp = gfeat + ((size_t)lvl * B + b) * C;
#pragma unroll
        for (uint32_t c = 0; c < C; c++) g[c] = gp[c];
        // wave-uniform dispatch on the level's addressing mode (lv lives in SGPRs), as in the gather
#pragma unroll
        for (uint32_t j = 0; j < 6; j++) {
            if (j < G && in_unit_cube(u[j][0], u[j][1], u[j][2])) {
                if (lv.hashed) {
                    if (lv.mask) point_level_grad<C, true, true>(lv, tab, g, u[j][0], u[j][1], u[j][2], rs[j], gu[j], gsig[j]);
                    else point_level_grad<C, true, false>(lv, tab, g, u[j][0], u[j][1], u[j][2], rs[j], gu[j], gsig[j]);
                } else {
                    if (lv.mask) point_level_grad<C, false, true>(lv, tab, g, u[j][0], u[j][1], u[j][2], rs[j], gu[j], gsig[j]);
                    else point_level_grad<C, false, false>(lv, tab, g, u[j][0], u[j][1], u[j][2], rs[j], gu[j], gsig[j]);
                }
            }
        }
    }
}

// acc += G * d raw / d x for one multisample at world position (x, y, z): gu through u = (contract(x) / 2 + 1) / 2 (warp) or
// u = (x + 1) / 2, gsig through the contraction's std factor
__device__ __forceinline__ void point_to_world(float x, float y, float z, bool warp, const float (&gu)[3], float gsig,
                                               float (&acc)[3]) {
    if (!warp) {
        acc[0] = fmaf(0.5f, gu[0], acc[0]); acc[1] = fmaf(0.5f, gu[1], acc[1]); acc[2] = fmaf(0.5f, gu[2], acc[2]);
        return;
    }
    const float m = fmaxf((x * x + y * y) + z * z, UCN_EPS);
    if (m <= 1.0f) {
        acc[0] = fmaf(0.25f, gu[0], acc[0]); acc[1] = fmaf(0.25f, gu[1], acc[1]); acc[2] = fmaf(0.25f, gu[2], acc[2]);
        return;
    }
    const float r = sqrtf(m);
    // coord.py:55: J = (2 x x^T (1 - r) + (2 r^3 - r^2) 1) / r^4, symmetric
    const float dot = (x * gu[0] + y * gu[1]) + z * gu[2];
    const float a1 = 2.0f * (1.0f - r) * dot, a2 = (2.0f * r - 1.0f) * m;
    const float q4 = 0.25f / (m * m);
    // d ln det_13 / dr = 4 / (3 (2r - 1)) - 2 / r;  sigma = det_13 std / 2  =>  (1 / sigma) d sigma / dx = that * x / r
    const float q = gsig * (4.0f / (3.0f * (2.0f * r - 1.0f)) - 2.0f / r) / r;
    acc[0] += fmaf(a1, x, a2 * gu[0]) * q4 + q * x;
    acc[1] += fmaf(a1, y, a2 * gu[1]) * q4 + q * y;
    acc[2] += fmaf(a1, z, a2 * gu[2]) * q4 + q * z;
}

// raw_grad = acc / G^2 (1/G of the feature mean, 1/G of models.py:562's mean over the multisamples);
// normals = -raw_grad / max(|raw_grad|, eps) (ref_utils.l2_normalize = F.normalize(eps = float32 eps))
__device__ __forceinline__ void store_normal(const float (&acc)[3], uint32_t G, float *__restrict__ raw_grad_out,
                                             float *__restrict__ normals_out, size_t o) {
    const float gg = (float)(G * G);
    const float g0 = acc[0] / gg, g1 = acc[1] / gg, g2 = acc[2] / gg;
    const float den = fmaxf(sqrtf((g0 * g0 + g1 * g1) + g2 * g2), UCN_EPS);
    raw_grad_out[o * 3 + 0] = g0; raw_grad_out[o * 3 + 1] = g1; raw_grad_out[o * 3 + 2] = g2;
    normals_out[o * 3 + 0] = -(g0 / den); normals_out[o * 3 + 1] = -(g1 / den); normals_out[o * 3 + 2] = -(g2 / den);
}

// layout: 0 = gfeat [L][N*S][C] with b = ray*S + s; 2 = [L][S*N][C] with b = s*N + ray (ucn_march_features'); outputs [ray][s]
// WARP = false (MLP.warp_fn = None): the same kernel on the uncontracted Gaussians: d raw / d x_j = (1/G) gu_j / 2, no Jacobian and
// nothing through the std (it does not depend on the mean); a sample with all six points outside the cube gets raw_grad = +0 and
// normals = -0.
template <uint32_t C, bool TD, bool WARP = true>
__global__ __launch_bounds__(256) void k_march_density_grad(UcnLevels lvls, const float *__restrict__ table, RayInputs in,
                                                            HexPattern hx, float std_scale, uint32_t N, uint32_t S, int layout,
                                                            const float *__restrict__ gfeat, float *__restrict__ raw_grad_out,
                                                            float *__restrict__ normals_out) {
    const size_t B = (size_t)N * S;
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    uint32_t ray, s;
    if (layout == 2) { s = (uint32_t)(b / N); ray = (uint32_t)(b - (size_t)s * N); }
    else { ray = (uint32_t)(b / S); s = (uint32_t)(b - (size_t)ray * S); }
    float u[6][3], rs[6], csum[3], tsum;
    float pr[6 * UCN_CAST_PROBE_FLOATS];                            // the world-space means (registers: every index is a constant)
    float *probe = pr;
    __builtin_assume(probe != nullptr);                             // folds cast_sample's `if (probe)`: pr stays in registers
    cast_sample<TD, WARP>(in, hx, std_scale, ray, s, S, u, rs, csum, tsum, probe);
    float gu[6][3], gsig[6];
    density_grad_levels<C>(lvls, table, gfeat, B, b, u, rs, 6, gu, gsig);
    float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (uint32_t j = 0; j < 6; j++)
        point_to_world(pr[j * UCN_CAST_PROBE_FLOATS], pr[j * UCN_CAST_PROBE_FLOATS + 1], pr[j * UCN_CAST_PROBE_FLOATS + 2], WARP, gu[j],
                       gsig[j], acc);
    store_normal(acc, 6, raw_grad_out, normals_out, (size_t)ray * S + s);
}

template <uint32_t C>
__global__ __launch_bounds__(256) void k_points_density_grad(UcnLevels lvls, const float *__restrict__ table,
                                                             const float *__restrict__ means, const float *__restrict__ stds,
                                                             uint32_t Bn, uint32_t G, int warp, const float *__restrict__ gfeat,
                                                             float *__restrict__ raw_grad_out, float *__restrict__ normals_out) {
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= Bn) return;
    float u[6][3], rs[6], x[6][3];
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        if (j < G) {
            const float *m = means + (b * G + j) * 3;
            x[j][0] = m[0]; x[j][1] = m[1]; x[j][2] = m[2];
            float c0, c1, c2;
            contract_to_unit(m[0], m[1], m[2], stds[b * G + j], warp != 0, u[j][0], u[j][1], u[j][2], rs[j], c0, c1, c2);
        } else {
            u[j][0] = u[j][1] = u[j][2] = 0.0f; rs[j] = 1.0f;
            x[j][0] = x[j][1] = x[j][2] = 0.0f;
        }
    }
    float gu[6][3], gsig[6];
    density_grad_levels<C>(lvls, table, gfeat, Bn, b, u, rs, G, gu, gsig);
    float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (uint32_t j = 0; j < 6; j++)
        if (j < G) point_to_world(x[j][0], x[j][1], x[j][2], warp != 0, gu[j], gsig[j], acc);
    store_normal(acc, G, raw_grad_out, normals_out, b);
}

}  // namespace

extern "C" int ucn_density_feature_grad(const ucn_field_t *f, const float *features, uint32_t B, float *gfeat_out,
                                        ucn_stream_t stream) {
    UCN_REQUIRE(f && f->w_d0 && f->b_d0 && f->w_d1, "density_feature_grad: the field's density_layer pointers are missing");
    UCN_REQUIRE(f->n_scale_planes == 0, "density_feature_grad: scale featurization is not supported (the gradient through the scale features is missing)");
    UCN_REQUIRE(f->num_levels >= 1 && f->num_levels <= UCN_MAX_LEVELS, "density_feature_grad: num_levels must be in [1,%d], got %u",
                UCN_MAX_LEVELS, f->num_levels);
    const uint32_t L = f->num_levels, C = f->level_dim;
    UCN_REQUIRE(C == 1 || C == 2 || C == 4 || C == 8, "GridEncoding: C must be 1, 2, 4, or 8.");
    if (B == 0) return 0;
    UCN_REQUIRE(features && gfeat_out, "density_feature_grad: null pointer argument");
    const size_t lds = ((size_t)kHidden * L * C + 2u * kHidden) * sizeof(float);
    UCN_REQUIRE(lds <= 64u * 1024u, "density_feature_grad: %u features do not fit the weight tile", L * C);
    ucn_for_level_dim(C, [&](auto cc) {
        hipLaunchKernelGGL(k_density_feature_grad<decltype(cc)::value>, dim3(ucn_div_up(B, 256)), dim3(256), lds, (hipStream_t)stream,
                           f->w_d0, f->b_d0, f->w_d1, L, L * C, features, (size_t)B, gfeat_out);
    });
    UCN_LAUNCH_CHECK("density_feature_grad");
    return 0;
}

extern "C" int ucn_march_density_grad(const ucn_field_t *f, const float *fenceposts, const float *near_, const float *far_,
                                      const float *origins, const float *directions, const float *basis, const float *radii,
                                      const float *flip, const float *spin, float std_scale, uint32_t N, uint32_t S, int layout,
                                      const float *gfeat, float *raw_grad_out, float *normals_out, ucn_stream_t stream) {
    return ucn_march_density_grad_warp(f, fenceposts, near_, far_, origins, directions, basis, radii, flip, spin, std_scale, 1, N, S,
                                       layout, gfeat, raw_grad_out, normals_out, stream);
}

extern "C" int ucn_march_density_grad_warp(const ucn_field_t *f, const float *fenceposts, const float *near_, const float *far_,
                                           const float *origins, const float *directions, const float *basis, const float *radii,
                                           const float *flip, const float *spin, float std_scale, int warp, uint32_t N, uint32_t S,
                                           int layout, const float *gfeat, float *raw_grad_out, float *normals_out,
                                           ucn_stream_t stream) {
    UCN_REQUIRE(warp == 0 || warp == 1, "march_density_grad: warp must be 0 (MLP.warp_fn = None) or 1 ('contract'), got %d", warp);
    UCN_REQUIRE((near_ == nullptr) == (far_ == nullptr), "march_density_grad: near and far come together (both NULL: metric fenceposts)");
    const bool td = near_ == nullptr;
    UCN_REQUIRE(N == 0 || (fenceposts && origins && directions && basis && radii && gfeat && raw_grad_out && normals_out),
                "march_density_grad: null pointer argument");
    UCN_REQUIRE((flip == nullptr) == (spin == nullptr), "march_density_grad: flip and spin come together");
    UCN_REQUIRE(layout == 0 || layout == 2, "march_density_grad: layout must be 0 or 2");
    UcnLevels lv;
    if (int rc = field_levels(f, &lv)) return rc;
    if (N == 0 || S == 0) return 0;
    const size_t B = (size_t)N * S;
    UCN_REQUIRE(B <= 0xFFFFFF00ull, "march_density_grad: too many samples in one call (%zu)", B);
    const RayInputs in{fenceposts, near_, far_, origins, directions, basis, radii, flip, spin};
    const HexPattern hx = make_hex();
    const dim3 grid(ucn_div_up(B, 256));
    ucn_for_level_dim(lv.C, [&](auto cc) {
        constexpr uint32_t CC = decltype(cc)::value;
#define UCN_DG(TDV, WARPV)                                                                                                \
    hipLaunchKernelGGL((k_march_density_grad<CC, TDV, WARPV>), grid, dim3(256), 0, (hipStream_t)stream, lv, f->embeddings, in, hx,    \
                       std_scale, N, S, layout, gfeat, raw_grad_out, normals_out)
        if (warp && td) UCN_DG(true, true);
        else if (warp) UCN_DG(false, true);
        else if (td) UCN_DG(true, false);
        else UCN_DG(false, false);
#undef UCN_DG
    });
    UCN_LAUNCH_CHECK("march_density_grad");
    return 0;
}

extern "C" int ucn_points_density_grad(const ucn_field_t *f, const float *means, const float *stds, uint32_t B, uint32_t G, int warp,
                                       const float *gfeat, float *raw_grad_out, float *normals_out, ucn_stream_t stream) {
    UCN_REQUIRE(G >= 1 && G <= 6, "points_density_grad: 1..6 Gaussians per feature, got %u", G);
    UcnLevels lv;
    if (int rc = field_levels(f, &lv)) return rc;
    if (B == 0) return 0;
    UCN_REQUIRE(means && stds && gfeat && raw_grad_out && normals_out, "points_density_grad: null pointer argument");
    ucn_for_level_dim(lv.C, [&](auto cc) {
        hipLaunchKernelGGL(k_points_density_grad<decltype(cc)::value>, dim3(ucn_div_up(B, 256)), dim3(256), 0, (hipStream_t)stream, lv,
                           f->embeddings, means, stds, B, G, warp, gfeat, raw_grad_out, normals_out);
    });
    UCN_LAUNCH_CHECK("points_density_grad");
    return 0;
}
