// Scale featurization (models.py:497-506): the per-level scale k[l] of a table (k_level_scale_*) and the scale planes of
// marched samples / caller-supplied Gaussians (k_march_scale_features, k_points_scale_features).
// One extra density-MLP input per grid level: (2 mean_j w[j, l] - 1) k[l], with w the damping factor the gather applies
// (erf_pos(rs_j * inv_gs_l), the same Gaussians through the same cast_sample / contract_to_unit: grid_cast.h) and k[l] the
// level's feature scale from k_level_scale_*.  No table access: ~800 VALU instructions of geometry and 6 L erf per sample.
// Kernels of their own names: k_march_features* (march_features.hip) stay as they are (bench.py tells launches apart by name).
#include "ucn_common.h"
#include "grid_cast.h"
#include "grid_rows.h"

namespace {

struct ScaleLevels {
    float inv_gs[UCN_MAX_LEVELS];
    uint32_t L;
};

// scale_out: sample_major ? [B][L] (b = ray*S+s always) : [ceil(L/C)][B][C] pseudo-level planes, plane p channel c = level
// p*C + c, channels past L zero -- the layout of the gather's [L][B][C] planes, behind which the caller places them.
template <uint32_t C>
__device__ __forceinline__ void scale_features_store(const ScaleLevels &sl, const float *__restrict__ level_scale,
                                                     const float (&rs)[6], uint32_t G, size_t B, size_t b,
                                                     float *__restrict__ scale_out, bool sample_major) {
    const uint32_t P = (sl.L + C - 1u) / C;
    const float g = (float)G;
    for (uint32_t p = 0; p < P; p++) {
        float v[C];
#pragma unroll
        for (uint32_t c = 0; c < C; c++) {
            const uint32_t l = p * C + c;
            v[c] = 0.0f;
            if (l < sl.L) {                                             // wave-uniform
                float sum = 0.0f;
#pragma unroll
                for (uint32_t j = 0; j < 6; j++)
                    if (j < G) sum += erf_pos(rs[j] * sl.inv_gs[l]);
                v[c] = (2.0f * (sum / g) - 1.0f) * level_scale[l];
            }
        }
        if (sample_major) {
#pragma unroll
            for (uint32_t c = 0; c < C; c++)
                if (p * C + c < sl.L) scale_out[b * sl.L + p * C + c] = v[c];
        } else {
            float *o = scale_out + ((size_t)p * B + b) * C;
            if constexpr (C == 2) *reinterpret_cast<float2 *>(o) = make_float2(v[0], v[1]);
            else if constexpr (C == 4) *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
            else {
#pragma unroll
                for (uint32_t c = 0; c < C; c++) o[c] = v[c];
            }
        }
    }
}

// WARP = false (MLP.warp_fn = None): the damping of the uncontracted std.  A point outside the unit cube adds no grid feature but
// keeps its erf weight here -- models.py:505 averages the weights over all six -- so nothing in this unit looks at u.
template <uint32_t C, bool TD, bool WARP = true>
__global__ __launch_bounds__(256) void k_march_scale_features(ScaleLevels sl, const float *__restrict__ level_scale, RayInputs in,
                                                              HexPattern hx, float std_scale, uint32_t N, uint32_t S, int layout,
                                                              float *__restrict__ scale_out) {
    const size_t B = (size_t)N * S;
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    uint32_t ray, s;                                                   // b as in march_features_body
    if (layout == 2) { s = (uint32_t)(b / N); ray = (uint32_t)(b - (size_t)s * N); }
    else { ray = (uint32_t)(b / S); s = (uint32_t)(b - (size_t)ray * S); }
    float u[6][3], rs[6], csum[3], tsum;
    cast_sample<TD, WARP>(in, hx, std_scale, ray, s, S, u, rs, csum, tsum);
    scale_features_store<C>(sl, level_scale, rs, 6, B, b, scale_out, layout == 1);
}

template <uint32_t C>
__global__ __launch_bounds__(256) void k_points_scale_features(ScaleLevels sl, const float *__restrict__ level_scale,
                                                               const float *__restrict__ means, const float *__restrict__ stds,
                                                               uint32_t Bn, uint32_t G, int warp, int sample_major,
                                                               float *__restrict__ scale_out) {
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= Bn) return;
    float rs[6];
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        rs[j] = 1.0f;
        if (j < G) {
            const float *m = means + (b * G + j) * 3;
            float u0, u1, u2, c0, c1, c2;
            contract_to_unit(m[0], m[1], m[2], stds[b * G + j], warp != 0, u0, u1, u2, rs[j], c0, c1, c2);
        }
    }
    scale_features_store<C>(sl, level_scale, rs, G, Bn, b, scale_out, sample_major != 0);
}

// k[l] = sqrt(init_std^2 + mean over the level's rows of sum_c e^2) in two passes of FIXED order (no float atomics: the
// result is bit-reproducible): kScaleBlocks partial sums per level, each a fixed slice of the level's rows summed by 256
// threads in strides and reduced by shuffles, then one thread per level adds the partials in order, in double.
constexpr uint32_t kScaleBlocks = 64;
struct LevelRows {
    uint32_t first[UCN_MAX_LEVELS + 1];
};
template <uint32_t C>
__global__ __launch_bounds__(256) void k_level_scale_partial(const float *__restrict__ table, LevelRows lr,
                                                             float *__restrict__ partial) {
    __shared__ float s_part[4];
    const uint32_t lvl = blockIdx.y;
    const uint32_t lo = lr.first[lvl], rows = lr.first[lvl + 1] - lo;
    const uint32_t per = (rows + kScaleBlocks - 1u) / kScaleBlocks;
    const uint32_t r0 = blockIdx.x * per, r1 = r0 + per < rows ? r0 + per : rows;
    float acc = 0.0f;
    for (uint32_t r = r0 + threadIdx.x; r < r1; r += 256u) {
        float v[C];
        load_row<C, float>(table + (size_t)lo * C, r, v);
        float sq = 0.0f;
#pragma unroll
        for (uint32_t c = 0; c < C; c++) sq = fmaf(v[c], v[c], sq);
        acc += sq;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63u) == 0u) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0u) partial[lvl * kScaleBlocks + blockIdx.x] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}
__global__ __launch_bounds__(64) void k_level_scale_final(const float *__restrict__ partial, LevelRows lr, uint32_t L, float init_std,
                                                          float *__restrict__ out) {
    const uint32_t lvl = threadIdx.x;
    if (lvl >= L) return;
    double sum = 0.0;
    for (uint32_t i = 0; i < kScaleBlocks; i++) sum += (double)partial[lvl * kScaleBlocks + i];
    const uint32_t rows = lr.first[lvl + 1] - lr.first[lvl];
    out[lvl] = (float)sqrt((double)init_std * (double)init_std + sum / (double)(rows ? rows : 1u));
}

ScaleLevels scale_levels(const UcnLevels &lv) {
    ScaleLevels sl;
    sl.L = lv.L;
    for (uint32_t l = 0; l < UCN_MAX_LEVELS; l++) sl.inv_gs[l] = l < lv.L ? lv.lv[l].inv_gs : 0.0f;
    return sl;
}

}  // namespace

template <bool TD, bool WARP>
static int march_scale_features_launch(const ucn_field_t *f, const RayInputs &in, float std_scale, uint32_t N, uint32_t S,
                                       const float *level_scale, int layout, float *scale_out, ucn_stream_t stream) {
    UCN_REQUIRE(N == 0 || (in.sdist && (TD || (in.near_ && in.far_)) && in.origins && in.dirs && in.basis && in.radii && level_scale &&
                           scale_out), "march_scale_features: null pointer argument");
    UCN_REQUIRE((in.flip == nullptr) == (in.spin == nullptr), "march_scale_features: flip and spin come together");
    UCN_REQUIRE(layout >= 0 && layout <= 2, "march_scale_features: layout must be 0, 1 or 2");
    UcnLevels lv;
    if (int rc = field_levels(f, &lv)) return rc;
    if (N == 0 || S == 0) return 0;
    const size_t B = (size_t)N * S;
    UCN_REQUIRE(B <= 0xFFFFFF00ull, "march_scale_features: too many samples in one call (%zu)", B);
    const ScaleLevels sl = scale_levels(lv);
    const HexPattern hx = make_hex();
    const dim3 grid(ucn_div_up(B, 256));
    ucn_for_level_dim(lv.C, [&](auto cc) {
        hipLaunchKernelGGL((k_march_scale_features<decltype(cc)::value, TD, WARP>), grid, dim3(256), 0, (hipStream_t)stream, sl,
                           level_scale, in, hx, std_scale, N, S, layout, scale_out);
    });
    UCN_LAUNCH_CHECK("march_scale_features");
    return 0;
}

extern "C" int ucn_march_scale_features_warp(const ucn_field_t *f, const float *fenceposts, const float *near_, const float *far_,
                                             const float *origins, const float *directions, const float *basis,
                                             const float *radii, const float *flip, const float *spin, float std_scale, int warp,
                                             uint32_t N, uint32_t S, const float *level_scale, int layout, float *scale_out,
                                             ucn_stream_t stream) {
    UCN_REQUIRE(warp == 0 || warp == 1, "march_scale_features: warp must be 0 (MLP.warp_fn = None) or 1 ('contract'), got %d", warp);
    UCN_REQUIRE(N == 0 || (near_ == nullptr) == (far_ == nullptr),
                "march_scale_features: near and far come together (both NULL: metric fenceposts)");
    const RayInputs in{fenceposts, near_, far_, origins, directions, basis, radii, flip, spin};
    int rc = 0;
    ucn_for_bool(near_ == nullptr, [&](auto td) {
        ucn_for_bool(warp != 0, [&](auto w) {
            rc = march_scale_features_launch<decltype(td)::value, decltype(w)::value>(f, in, std_scale, N, S, level_scale, layout, scale_out,
                                                                                      stream);
        });
    });
    return rc;
}

extern "C" int ucn_march_scale_features(const ucn_field_t *f, const float *sdist, const float *near_, const float *far_,
                                        const float *origins, const float *directions, const float *basis, const float *radii,
                                        const float *flip, const float *spin, float std_scale, uint32_t N, uint32_t S,
                                        const float *level_scale, int layout, float *scale_out, ucn_stream_t stream) {
    UCN_REQUIRE(N == 0 || (near_ && far_), "march_scale_features: null pointer argument");
    return ucn_march_scale_features_warp(f, sdist, near_, far_, origins, directions, basis, radii, flip, spin, std_scale, 1, N, S,
                                         level_scale, layout, scale_out, stream);
}

extern "C" int ucn_march_scale_features_tdist(const ucn_field_t *f, const float *tdist, const float *origins,
                                              const float *directions, const float *basis, const float *radii, const float *flip,
                                              const float *spin, float std_scale, uint32_t N, uint32_t S, const float *level_scale,
                                              int layout, float *scale_out, ucn_stream_t stream) {
    return ucn_march_scale_features_warp(f, tdist, nullptr, nullptr, origins, directions, basis, radii, flip, spin, std_scale, 1, N, S,
                                         level_scale, layout, scale_out, stream);
}

extern "C" int ucn_points_scale_features(const ucn_field_t *f, const float *means, const float *stds, uint32_t B, uint32_t G,
                                         int warp, const float *level_scale, int sample_major, float *scale_out,
                                         ucn_stream_t stream) {
    UCN_REQUIRE(means && stds && level_scale && scale_out, "points_scale_features: null pointer argument");
    UCN_REQUIRE(G >= 1 && G <= 6, "points_scale_features: 1..6 Gaussians per feature, got %u", G);
    UcnLevels lv;
    if (int rc = field_levels(f, &lv)) return rc;
    if (B == 0) return 0;
    const ScaleLevels sl = scale_levels(lv);
    const dim3 grid(ucn_div_up(B, 256));
    ucn_for_level_dim(lv.C, [&](auto cc) {
        hipLaunchKernelGGL(k_points_scale_features<decltype(cc)::value>, grid, dim3(256), 0, (hipStream_t)stream, sl, level_scale,
                           means, stds, B, G, warp, sample_major, scale_out);
    });
    UCN_LAUNCH_CHECK("points_scale_features");
    return 0;
}

extern "C" int ucn_level_scale(const float *embeddings, const int32_t *offsets_host, uint32_t L, uint32_t C, float init_std,
                               float *out, float *workspace, ucn_stream_t stream) {
    UCN_REQUIRE(embeddings && offsets_host && out && workspace, "level_scale: null pointer argument");
    UCN_REQUIRE(L >= 1 && L <= UCN_MAX_LEVELS, "level_scale: num_levels must be in [1,%d], got %u", UCN_MAX_LEVELS, L);
    UCN_REQUIRE(C == 1 || C == 2 || C == 4 || C == 8, "level_scale: C must be 1, 2, 4, or 8.");
    LevelRows lr;
    for (uint32_t l = 0; l <= UCN_MAX_LEVELS; l++) lr.first[l] = (uint32_t)offsets_host[l < L ? l : L];
    for (uint32_t l = 0; l < L; l++) UCN_REQUIRE(lr.first[l + 1] >= lr.first[l], "level_scale: offsets must not decrease");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(kScaleBlocks, L);
    static_assert(UCN_LEVEL_SCALE_WS_FLOATS >= UCN_MAX_LEVELS * kScaleBlocks, "workspace constant too small");
    ucn_for_level_dim(C, [&](auto cc) {
        hipLaunchKernelGGL(k_level_scale_partial<decltype(cc)::value>, grid, dim3(256), 0, st, embeddings, lr, workspace);
    });
    hipLaunchKernelGGL(k_level_scale_final, dim3(1), dim3(64), 0, st, workspace, lr, L, init_std, out);
    UCN_LAUNCH_CHECK("level_scale");
    return 0;
}
