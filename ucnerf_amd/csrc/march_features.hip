// Fused sample featurisation: cone cast -> contraction -> hash-grid gather -> erf damping -> mean of 6.
//
// Replaces, for one sampling level, the chain
//   render.cast_rays            (internal/render.py:94-152)
//   coord.track_linearize       (coord.py:60-116, 'contract')
//   GridEncoder.forward         (gridencoder/grid.py:158-174 -> gridencoder.cu:87-199)
//   erf down-weighting + mean   (models.py:494-496)
// The reference materialises [N*S*6,3] points, the [L,N*S*6,C] gather result, its permuted copy
// and the erf weights in HBM (~1.5 GB per 15000-ray chunk at 128 samples); here the six
// multisamples of a sample live in registers and only the [L][N*S][C] mean feature is written.
//
// This unit: the inference and training FORWARD (k_march_features / k_march_features_td, k_points_features) and the
// cast / contraction probes.  The sample geometry is grid_cast.h, the lattice addressing grid_rows.h -- both shared with the
// table gradient (march_features_bwd.hip); the scale planes are march_scale.hip.
//
// Mapping (CDNA4): one thread = one sample x one GROUP of levels (make_groups); blockIdx.y is the group, so the grid is
// level-major in dispatch order.  Auto grouping: every fine level (resolution > 2048) is a group of its own, so an XCD's L2
// (4 MiB) sees one 4 MiB hashed level slice at a time (measured: all 16 levels per thread costs 1.8x), and the coarse levels are
// dealt out over those groups -- config B: one coarse level per fine level, the coarsest with the finest -- instead of forming a
// VALU-bound group of their own that derives the sample geometry a ninth time (1.104 -> 1.042 ms per 10 240-ray pass,
// profiles/level_pairs/).  Lanes of a wave are neighbouring rays at one sample index (layout 2) or consecutive samples of a ray
// -> the [L][B][C] store is a contiguous 64*C*4-byte run per wave.
//
// What bounds it (rocprofv3, r01b): with the tables L2/MALL-resident the kernel is VALU-bound
// (SQ_ACTIVE_INST_VALU = 21 % of wave-cycles at 4 waves/SIMD = 84 % of a SIMD), ~3000 VALU
// instructions per (sample, level).  Hence the shape of the addressing (grid_rows.h) and the split between exact and
// fast arithmetic (grid_cast.h).
#include "ucn_common.h"
#include "grid_cast.h"
#include "grid_rows.h"

namespace {

// rows r and r ^ 1 (an aligned pair, C = 2) in one request: out[0..1] = row (r & ~1), out[2..3] = row (r | 1)
template <typename TT>
__device__ __forceinline__ void load_row_pair(const TT *__restrict__ tab, uint32_t row_even, float (&o)[4]) {
    if constexpr (sizeof(TT) == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(tab + (size_t)row_even * 2);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
        typedef _Float16 hx4 __attribute__((ext_vector_type(4)));
        const hx4 t = *reinterpret_cast<const hx4 *>(tab + (size_t)row_even * 2);
        o[0] = (float)t[0]; o[1] = (float)t[1]; o[2] = (float)t[2]; o[3] = (float)t[3];
    }
}

// sum_j damp_j * trilerp(point_j) for one level
template <uint32_t C, bool HASHED, bool POW2, typename TT>
__device__ __forceinline__ void level_accumulate(const UcnLevel &lv, const TT *__restrict__ tab,
                                                 const float (&u)[6][3], const float (&rs)[6], uint32_t G,
                                                 float (&acc)[C]) {
#pragma unroll
    for (uint32_t c = 0; c < C; c++) acc[c] = 0.0f;
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        if (j < G && in_unit_cube(u[j][0], u[j][1], u[j][2])) {
            float fx, fy, fz, w[8];
            uint32_t rows[8];
            corner_rows<HASHED, POW2>(lv, u[j][0], u[j][1], u[j][2], fx, fy, fz, rows);
            float v[8][C];
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) load_row<C, TT>(tab, rows[k], v[k]);
            corner_weights(fx, fy, fz, w);
            float f[C];
#pragma unroll
            for (uint32_t c = 0; c < C; c++) f[c] = 0.0f;
#pragma unroll
            for (uint32_t k = 0; k < 8; k++)
#pragma unroll
                for (uint32_t c = 0; c < C; c++) f[c] = fmaf(w[k], v[k][c], f[c]);
            // models.py:495: erf(1 / sqrt(8 std^2 gs^2)) = erf(rs_j * lv.inv_gs), gs^2 in wrapped int32
            const float damp = erf_pos(rs[j] * lv.inv_gs);
#pragma unroll
            for (uint32_t c = 0; c < C; c++) acc[c] += f[c] * damp;
        }
    }
}

// Coarse levels (cells far larger than a sample's cone section): the six multisamples of a sample usually sit in ONE
// lattice cell.  Then its 8 corner rows are derived and fetched once instead of six times; every point still forms its
// own weights and accumulates in level_accumulate's order, so the result is bit-identical.  Lanes whose points straddle a
// cell boundary take the general path (the branch diverges; the caller enables this only where straddling is rare).
template <uint32_t C, bool HASHED, bool POW2, typename TT>
__device__ __forceinline__ void level_accumulate_shared(const UcnLevel &lv, const TT *__restrict__ tab,
                                                        const float (&u)[6][3], const float (&rs)[6], float (&acc)[C]) {
    float fx[6], fy[6], fz[6];
    uint32_t x0 = 0, y0 = 0, z0 = 0;
    bool same = true, any = false;
    uint32_t inside = 0;
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        if (in_unit_cube(u[j][0], u[j][1], u[j][2])) {
            fx[j] = fmaf(u[j][0], lv.scale, 0.5f); fy[j] = fmaf(u[j][1], lv.scale, 0.5f); fz[j] = fmaf(u[j][2], lv.scale, 0.5f);
            const uint32_t xj = (uint32_t)floorf(fx[j]), yj = (uint32_t)floorf(fy[j]), zj = (uint32_t)floorf(fz[j]);
            fx[j] -= (float)xj; fy[j] -= (float)yj; fz[j] -= (float)zj;
            if (!any) { x0 = xj; y0 = yj; z0 = zj; any = true; }
            else same = same && xj == x0 && yj == y0 && zj == z0;
            inside |= 1u << j;
        }
    }
    if (!same) {
        level_accumulate<C, HASHED, POW2, TT>(lv, tab, u, rs, 6, acc);
        return;
    }
#pragma unroll
    for (uint32_t c = 0; c < C; c++) acc[c] = 0.0f;
    if (!any) return;
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
    float v[8][C];
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t xv = (k & 1u) ? xb : xa, yv = (k & 2u) ? yb : ya, zv = (k & 4u) ? zb : za;
        uint32_t idx;
        if constexpr (HASHED) idx = xv ^ yv ^ zv;
        else idx = xv + yv + zv;
        uint32_t row;
        if constexpr (POW2) row = idx & lv.mask;
        else row = idx < lv.rows ? idx : idx % lv.rows;
        load_row<C, TT>(tab, row, v[k]);
    }
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        if (inside & (1u << j)) {
            float w[8];
            corner_weights(fx[j], fy[j], fz[j], w);
            float f[C];
#pragma unroll
            for (uint32_t c = 0; c < C; c++) f[c] = 0.0f;
#pragma unroll
            for (uint32_t k = 0; k < 8; k++)
#pragma unroll
                for (uint32_t c = 0; c < C; c++) f[c] = fmaf(w[k], v[k][c], f[c]);
            const float damp = erf_pos(rs[j] * lv.inv_gs);
#pragma unroll
            for (uint32_t c = 0; c < C; c++) acc[c] += f[c] * damp;
        }
    }
}

// Fine hashed levels, C = 2, power-of-two table: the kernel is bound by the L2 request rate there (one
// request per gathered corner, ~16 per clock per XCD), so corners that are adjacent in memory are fetched
// together.  For an even lattice x the corners (x, y, z) and (x+1, y, z) hash to rows r and r^1 -- one
// aligned 16-byte pair; for an odd x they are unrelated and cost two requests.  6 requests per point on
// average instead of 8.  Same values, same fmaf order as level_accumulate.
template <typename TT>
__device__ __forceinline__ void level_accumulate_pairs(const UcnLevel &lv, const TT *__restrict__ tab,
                                                       const float (&u)[6][3], const float (&rs)[6], float (&acc)[2]) {
    acc[0] = acc[1] = 0.0f;
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        if (in_unit_cube(u[j][0], u[j][1], u[j][2])) {
            float fx, fy, fz, w[8];
            uint32_t rows[8];
            corner_rows<true, true>(lv, u[j][0], u[j][1], u[j][2], fx, fy, fz, rows);
            const bool even = ((rows[0] ^ rows[1]) == 1u);          // x0 even <=> the two rows differ in bit 0 only
            float v[8][2];
            if (even) {                                             // one divergent branch per point
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) {                  // (y, z) choice; corners 2q (x0) and 2q+1 (x0+1)
                    const uint32_t r0 = rows[2 * q];
                    float t[4];
                    load_row_pair<TT>(tab, r0 & ~1u, t);
                    const bool hi = (r0 & 1u) != 0u;
                    v[2 * q][0] = hi ? t[2] : t[0]; v[2 * q][1] = hi ? t[3] : t[1];
                    v[2 * q + 1][0] = hi ? t[0] : t[2]; v[2 * q + 1][1] = hi ? t[1] : t[3];
                }
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) load_row<2, TT>(tab, rows[k], v[k]);
            }
            corner_weights(fx, fy, fz, w);
            float f0 = 0.0f, f1 = 0.0f;
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                f0 = fmaf(w[k], v[k][0], f0);
                f1 = fmaf(w[k], v[k][1], f1);
            }
            const float damp = erf_pos(rs[j] * lv.inv_gs);
            acc[0] += f0 * damp;
            acc[1] += f1 * damp;
        }
    }
}

// LANE-PAIRED fetch (r04), C = 2, power-of-two tables.  The corners (x0, y, z) and (x0 + 1, y, z) of a point hash to rows r and
// r ^ d (hashed levels; r, r + 1 on the strided ones): in 7 cases of 8 (x0 & 7 != 7) the same aligned group of eight 8-byte rows,
// i.e. the SAME 64-byte line -- but up to 56 bytes apart, so no single load of one lane covers both, and as two load
// instructions they are two line requests (the bound of the fine levels: L1 lines per clock).  The texture-address path DOES
// merge lanes of ONE instruction that hit the same line, wherever they sit in the wave (tools/ta_merge_bench.hip: two 8-byte
// loads per point 349 G rows/s; the same rows as ONE instruction over lane pairs 532 G rows/s -- the rate of an aligned 16-byte
// load).  So a wave fetches a (y, z) combination in two instructions that each serve 32 POINTS: lane i < 32 asks for the x0 row of
// point i while lane i + 32 asks for the x0 + 1 row of the same point (second instruction: the points of lanes 32 ... 63).  One
// v_permlane32_swap of (row_x0, row_x1) forms both address registers, one per channel sorts the values back:
//   swap(a, b) -> {a.lo, b.lo}, {a.hi, b.hi}.  4.5 line requests per point instead of 6 (pair fetch) or 8, no divergent branch.
// Points outside the unit cube fetch (masked, hence valid) dummy rows and are skipped at the accumulation: same values, same
// fmaf order as level_accumulate.  Needs every lane of the wave active (the caller checks).
constexpr uint32_t kLanePairDepth = 1;                              // points whose 8 loads are in flight together (2 / 3 / 6 measured: DESIGN)
template <bool HASHED, typename TT>
__device__ __forceinline__ void level_accumulate_lanepairs(const UcnLevel &lv, const TT *__restrict__ tab,
                                                           const float (&u)[6][3], const float (&rs)[6], float (&acc)[2]) {
    acc[0] = acc[1] = 0.0f;
    constexpr uint32_t DEPTH = kLanePairDepth;
#pragma unroll
    for (uint32_t j0 = 0; j0 < 6; j0 += DEPTH) {
        float fx[DEPTH], fy[DEPTH], fz[DEPTH];
        uint32_t adr[DEPTH][4][2];
        bool valid[DEPTH];
#pragma unroll
        for (uint32_t d = 0; d < DEPTH; d++) {
            const uint32_t j = j0 + d;
            valid[d] = in_unit_cube(u[j][0], u[j][1], u[j][2]);
            uint32_t rows[8];
            corner_rows<HASHED, true>(lv, u[j][0], u[j][1], u[j][2], fx[d], fy[d], fz[d], rows);
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {                          // (y, z) choice; corners 2q (x0) and 2q + 1 (x0 + 1)
                const auto ad = __builtin_amdgcn_permlane32_swap(rows[2 * q], rows[2 * q + 1], false, false);
                adr[d][q][0] = ad[0]; adr[d][q][1] = ad[1];
            }
        }
        // every load of the group is issued before the first value is used
        uint32_t raw[DEPTH][4][2][sizeof(TT) == 4 ? 2 : 1];
#pragma unroll
        for (uint32_t d = 0; d < DEPTH; d++)
#pragma unroll
            for (uint32_t q = 0; q < 4; q++)
#pragma unroll
                for (uint32_t e = 0; e < 2; e++) {
                    if constexpr (sizeof(TT) == 4) {
                        const uint2 t = *reinterpret_cast<const uint2 *>(tab + (size_t)adr[d][q][e] * 2);
                        raw[d][q][e][0] = t.x; raw[d][q][e][1] = t.y;
                    } else {
                        raw[d][q][e][0] = *reinterpret_cast<const uint32_t *>(tab + (size_t)adr[d][q][e] * 2);   // a row = two halves = one word
                    }
                }
#pragma unroll
        for (uint32_t d = 0; d < DEPTH; d++) {
            float v[8][2], w[8];
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
                if constexpr (sizeof(TT) == 4) {
                    const auto s0 = __builtin_amdgcn_permlane32_swap(raw[d][q][0][0], raw[d][q][1][0], false, false);
                    const auto s1 = __builtin_amdgcn_permlane32_swap(raw[d][q][0][1], raw[d][q][1][1], false, false);
                    v[2 * q][0] = __builtin_bit_cast(float, (uint32_t)s0[0]); v[2 * q + 1][0] = __builtin_bit_cast(float, (uint32_t)s0[1]);
                    v[2 * q][1] = __builtin_bit_cast(float, (uint32_t)s1[0]); v[2 * q + 1][1] = __builtin_bit_cast(float, (uint32_t)s1[1]);
                } else {
                    typedef _Float16 hx2 __attribute__((ext_vector_type(2)));
                    const auto s0 = __builtin_amdgcn_permlane32_swap(raw[d][q][0][0], raw[d][q][1][0], false, false);
                    const hx2 h0 = __builtin_bit_cast(hx2, (uint32_t)s0[0]), h1 = __builtin_bit_cast(hx2, (uint32_t)s0[1]);
                    v[2 * q][0] = (float)h0[0]; v[2 * q][1] = (float)h0[1];
                    v[2 * q + 1][0] = (float)h1[0]; v[2 * q + 1][1] = (float)h1[1];
                }
            }
            corner_weights(fx[d], fy[d], fz[d], w);
            float f0 = 0.0f, f1 = 0.0f;
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                f0 = fmaf(w[k], v[k][0], f0);
                f1 = fmaf(w[k], v[k][1], f1);
            }
            const float damp = erf_pos(rs[j0 + d] * lv.inv_gs);
            if (valid[d]) {
                acc[0] += f0 * damp;
                acc[1] += f1 * damp;
            }
        }
    }
}

constexpr uint32_t kSharedCellMaxRes = 64;                          // dense levels up to this resolution use level_accumulate_shared
// levels finer than this take the lane-paired fetch when a wave's rays are neighbouring pixels (rendering: on the middle levels the
// lanes share lines anyway and the three swaps per corner pair cost more than they save -- per-level times in
// profiles/r04/level_times_*.txt); UCN_RAYS_INCOHERENT (random training rays, no sharing on any hashed level) lowers it to
// kSharedCellMaxRes
constexpr uint32_t kLanePairMinRes = 2048u;

// The thread's levels are level_of(i0) ... level_of(i1 - 1), in that order (level_of: wave-uniform index -> level).
// layout: 0 = [L][B][C] (b as given), 1 = [B][L*C]
template <uint32_t C, typename TT, typename LevelOf>
__device__ __forceinline__ void featurise(const UcnLevels &lvls, const TT *__restrict__ table, LevelOf level_of, uint32_t i0,
                                          uint32_t i1, const float (&u)[6][3], const float (&rs)[6], uint32_t G,
                                          size_t B, size_t b, float *__restrict__ out, bool sample_major, bool out_bf16 = false,
                                          bool full_wave = false, uint32_t lp_min_res = kLanePairMinRes) {
    const uint32_t F_out = lvls.L * C;
    const auto store = [&](uint32_t lvl, const float (&acc)[C]) {
        float *o = sample_major ? out + b * F_out + (size_t)lvl * C : out + ((size_t)lvl * B + b) * C;
        const float inv = (float)G;
        if constexpr (C == 2) {
            if (out_bf16) {            // [L][B] pairs of bf16 (round to nearest even): what the bf16 MLP would make of the floats
                typedef float f2v __attribute__((ext_vector_type(2)));
                typedef __bf16 bf2v __attribute__((ext_vector_type(2)));
                const f2v t = {acc[0] / inv, acc[1] / inv};
                reinterpret_cast<uint32_t *>(out)[(size_t)lvl * B + b] = __builtin_bit_cast(uint32_t, __builtin_convertvector(t, bf2v));
                return;
            }
            *reinterpret_cast<float2 *>(o) = make_float2(acc[0] / inv, acc[1] / inv);
        } else if constexpr (C == 4) {
            *reinterpret_cast<float4 *>(o) = make_float4(acc[0] / inv, acc[1] / inv, acc[2] / inv, acc[3] / inv);
        } else {
#pragma unroll
            for (uint32_t c = 0; c < C; c++) o[c] = acc[c] / inv;
        }
    };
    for (uint32_t i = i0; i < i1; i++) {
        const uint32_t lvl = level_of(i);
        const UcnLevel lv = lvls.lv[lvl];
        const TT *tab = table + (size_t)lv.first_row * C;
        float acc[C];
        // wave-uniform dispatch on the level's addressing mode (lv lives in SGPRs)
        if (lv.hashed && G == 6 && lv.resolution <= kSharedCellMaxRes) {
            if (lv.mask) level_accumulate_shared<C, true, true>(lv, tab, u, rs, acc);
            else level_accumulate_shared<C, true, false>(lv, tab, u, rs, acc);
        } else if (lv.hashed) {
            if constexpr (C == 2) {
                if (lv.mask && G == 6 && full_wave && lv.resolution > lp_min_res) level_accumulate_lanepairs<true, TT>(lv, tab, u, rs, acc);
                else if (lv.mask && lv.resolution > 2048u && G == 6) level_accumulate_pairs(lv, tab, u, rs, acc);
                else if (lv.mask) level_accumulate<C, true, true>(lv, tab, u, rs, G, acc);
                else level_accumulate<C, true, false>(lv, tab, u, rs, G, acc);
            } else {
                if (lv.mask) level_accumulate<C, true, true>(lv, tab, u, rs, G, acc);
                else level_accumulate<C, true, false>(lv, tab, u, rs, G, acc);
            }
        } else if (G == 6 && lv.resolution <= kSharedCellMaxRes) {
            if (lv.mask) level_accumulate_shared<C, false, true>(lv, tab, u, rs, acc);
            else level_accumulate_shared<C, false, false>(lv, tab, u, rs, acc);
        } else {
            if constexpr (C == 2) {
                if (lv.mask && G == 6 && full_wave && lv.stride[0] == 1u && lv.resolution > lp_min_res) {
                    level_accumulate_lanepairs<false, TT>(lv, tab, u, rs, acc);
                } else {
                    if (lv.mask) level_accumulate<C, false, true>(lv, tab, u, rs, G, acc);
                    else level_accumulate<C, false, false>(lv, tab, u, rs, G, acc);
                }
            } else {
                if (lv.mask) level_accumulate<C, false, true>(lv, tab, u, rs, G, acc);
                else level_accumulate<C, false, false>(lv, tab, u, rs, G, acc);
            }
        }
        store(lvl, acc);
    }
}

// Introspection for the parity tests: the product's own cast_sample / contract_to_unit, results
// written out instead of consumed.
// WARP = false (MLP.warp_fn = None): floats 5..8 of a point repeat its cast mean and std, 9 is 1 / sqrt(8 std^2) of the uncontracted std
template <bool TD = false, bool WARP = true>
__global__ __launch_bounds__(256) void k_cast_probe(RayInputs in, HexPattern hx, float std_scale, uint32_t N, uint32_t S,
                                                    float *__restrict__ out) {
    const size_t B = (size_t)N * S;
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    const uint32_t ray = (uint32_t)(b / S), s = (uint32_t)(b - (size_t)ray * S);
    float u[6][3], rs[6], csum[3], tsum;
    cast_sample<TD, WARP>(in, hx, std_scale, ray, s, S, u, rs, csum, tsum, out + b * 6 * UCN_CAST_PROBE_FLOATS);
}

__global__ __launch_bounds__(256) void k_contract_probe(const float *__restrict__ means, const float *__restrict__ stds,
                                                        uint32_t B, float *__restrict__ out_mean, float *__restrict__ out_std) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    float u0, u1, u2, rs, c0, c1, c2, sd;
    contract_to_unit(means[b * 3], means[b * 3 + 1], means[b * 3 + 2], stds[b], true, u0, u1, u2, rs, c0, c1, c2, &sd);
    out_mean[b * 3] = c0; out_mean[b * 3 + 1] = c1; out_mean[b * 3 + 2] = c2;
    out_std[b] = sd;
}

// Levels handled by one thread: group g = list[lo[g]] ... list[lo[g+1] - 1], in that order.  A thread re-derives the
// sample's six contracted positions (~800 VALU instructions) once per GROUP, then pays ~400-500 per level.
//
// levels_per_block = k > 0: contiguous groups of k levels.
// Auto (0): a level is COARSE up to resolution 2048 and FINE above.  Every fine level is a group of its own -- level-major dispatch
// keeps its 4 MiB slice in an XCD's L2.  Rendering (a wave's rays are neighbouring pixels): the coarse levels run at their VALU
// floor while the fine ones are bound by the texture-data return path with VALU 56 % busy, so the coarse levels are dealt out over
// the fine groups.  A thread runs its levels one after the other; what the pairing saves is the group that derived the geometry
// a ninth time, and what overlap there is comes from the other waves of the SIMD.  UCN_RAYS_INCOHERENT (random training rays: the
// coarse hashed levels share no lines and are themselves memory-bound) and grids with only one kind of level keep contiguous
// groups, the coarse levels eight together: pairing cost +25 % there (profiles/level_pairs/after.txt).
struct LevelGroups {                 // whole words: a kernel reads them from its arguments with scalar loads (bytes would go through the vector path)
    uint32_t lo[UCN_MAX_LEVELS + 1];
    uint32_t list[UCN_MAX_LEVELS];
    uint32_t n;
};
static LevelGroups make_groups(const UcnLevels &lv, uint32_t levels_per_block, bool incoherent) {
    LevelGroups g;
    g.n = 0;
    const uint32_t cres = 2048u, cgrp = 8u;   // measured: (512..8192) x (3..8) all within 3 %; this is the best
    uint32_t coarse[UCN_MAX_LEVELS], fine[UCN_MAX_LEVELS], nc = 0, nf = 0;   // each in level order = ascending resolution
    for (uint32_t l = 0; l < lv.L; l++) {
        if (lv.lv[l].resolution <= cres) coarse[nc++] = l;
        else fine[nf++] = l;
    }
    if (levels_per_block != 0 || nc == 0 || nf == 0 || incoherent) {
        for (uint32_t l = 0; l < lv.L; l++) g.list[l] = l;
        uint32_t l = 0;
        while (l < lv.L) {
            g.lo[g.n++] = l;
            const uint32_t take = levels_per_block ? levels_per_block : (lv.lv[l].resolution <= cres ? cgrp : 1u);
            uint32_t end = l + take < lv.L ? l + take : lv.L;
            if (levels_per_block == 0)                                                    // a group never mixes coarse and fine
                for (uint32_t k = l + 1; k < end; k++)
                    if (lv.lv[k].resolution > cres) { end = k; break; }
            l = end;
        }
        g.lo[g.n] = lv.L;
        return g;
    }
    // nc coarse levels over nf fine groups: nc / nf each, the remainder to the lowest-resolution (lightest) fine levels; a
    // group holds at most cgrp levels, what does not fit stays in coarse-only groups behind the fine ones
    uint32_t per = nc / nf, extra = nc % nf;
    if (per >= cgrp - 1u) { per = cgrp - 1u; extra = 0; }
    // Which coarse level with which fine level (profiles/level_pairs/assignments.txt): the fine groups ascend in resolution and take
    // the coarse levels from the top, so the coarsest levels (dense, one shared cell per sample: the least traffic) ride with the
    // finest, most return-path-bound levels.  A thread runs its coarse levels first, its fine level last.
    uint32_t c_hi = nc, n = 0;                                       // coarse[0 .. c_hi) are still to be placed
    for (uint32_t i = 0; i < nf; i++) {
        g.lo[g.n++] = n;
        const uint32_t cnt = per + (i < extra ? 1u : 0u);
        for (uint32_t k = 0; k < cnt; k++) g.list[n++] = coarse[--c_hi];
        g.list[n++] = fine[i];
    }
    for (uint32_t c_lo = 0; c_lo < c_hi;) {
        g.lo[g.n++] = n;
        for (uint32_t k = 0; k < cgrp && c_lo < c_hi; k++) g.list[n++] = coarse[c_lo++];
    }
    g.lo[g.n] = n;
    return g;
}

// layout: 0 = [L][N*S][C] with b = ray*S+s; 1 = [N*S][L*C]; 2 = [L][S*N][C] with b = s*N+ray
// FEW_LEVELS is a NAME TAG only (same code): grids of <= 8 levels (the proposal fields: L = 6) and of more (the NeRF field:
// L = 16 / 10) get distinct kernel names, so that a rocprofv3 --stats summary separates the proposal-level from the
// NeRF-level launches without subtracting one from the other.
template <uint32_t C, uint32_t TPB, typename TT, bool TD, bool WARP = true>
__device__ __forceinline__ void march_features_body(const UcnLevels &lvls, const TT *__restrict__ table, const RayInputs &in,
                                                    const HexPattern &hx, float std_scale, uint32_t N, uint32_t S,
                                                    const LevelGroups &grp, int layout,
                                                    float *__restrict__ features, float *__restrict__ coord_out,
                                                    float *__restrict__ tmean_out) {
    // co-resident shape (512 threads: launched beside an MLP workgroup on the same CU): a SIMD does not overlap VALU
    // with MFMA (tools/mfma_valu_bench.hip), so at equal priority every VALU instruction of this kernel would queue behind
    // one of the MLP wave's 32-cycle MFMAs.  With the higher priority the gather waves issue their bursts back to back and
    // the MFMAs fill the time in which all of them wait for memory.
    if constexpr (TPB == 512) __builtin_amdgcn_s_setprio(3);
    const size_t B = (size_t)N * S;
    const size_t b = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (b >= B) return;
    // layout 2 ("rays fastest"): the 64 lanes of a wave are NEIGHBOURING RAYS at one sample index.
    // On the dense coarse levels neighbouring pixels read the same few lattice cells, which the TA
    // coalesces: levels 0-7 drop to the VALU floor (-20 % on the kernel, r01b).  The model's default.
    uint32_t ray, s;
    if ((layout & 3) == 2) { s = (uint32_t)(b / N); ray = (uint32_t)(b - (size_t)s * N); }
    else { ray = (uint32_t)(b / S); s = (uint32_t)(b - (size_t)ray * S); }
    float u[6][3], rs[6], csum[3], tsum;
    cast_sample<TD, WARP>(in, hx, std_scale, ray, s, S, u, rs, csum, tsum);
    const uint32_t i0 = grp.lo[blockIdx.y], i1 = grp.lo[blockIdx.y + 1];
    const auto level_of = [&grp](uint32_t i) -> uint32_t { return grp.list[i]; };
    const bool full_wave = __ballot(true) == ~0ull;                  // the lane-paired fetch trades rows between lanes i and i + 32
    const uint32_t lp_min = (layout & 0x20) ? kSharedCellMaxRes : kLanePairMinRes;     // 0x20: UCN_RAYS_INCOHERENT (private bit)
    if constexpr (sizeof(TT) == 2) featurise<C, TT>(lvls, table, level_of, i0, i1, u, rs, 6, B, b, features, (layout & 3) == 1, (layout & 0x10) != 0, full_wave, lp_min);
    else featurise<C, TT>(lvls, table, level_of, i0, i1, u, rs, 6, B, b, features, (layout & 3) == 1, false, full_wave, lp_min);
    if (blockIdx.y == 0) {
        const size_t o = (size_t)ray * S + s;                     // per-sample side outputs stay [N,S]
        if (coord_out) {
            coord_out[o * 3 + 0] = csum[0] / 6.0f; coord_out[o * 3 + 1] = csum[1] / 6.0f; coord_out[o * 3 + 2] = csum[2] / 6.0f;
        }
        if (tmean_out) tmean_out[o] = tsum / 6.0f;
    }
}

template <uint32_t C, uint32_t TPB, typename TT = float, bool FEW_LEVELS = false>
__global__ __launch_bounds__(TPB) void k_march_features(UcnLevels lvls, const TT *__restrict__ table, RayInputs in,
                                                        HexPattern hx, float std_scale, uint32_t N, uint32_t S,
                                                        LevelGroups grp, int layout, float *__restrict__ features,
                                                        float *__restrict__ coord_out, float *__restrict__ tmean_out) {
    march_features_body<C, TPB, TT, false>(lvls, table, in, hx, std_scale, N, S, grp, layout, features, coord_out, tmean_out);
}

// The same on metric fenceposts (a warped Model.raydist_fn): a kernel of its own NAME rather than a trailing TD argument of
// k_march_features, whose last template argument (FEW_LEVELS) is how bench.py tells the NeRF-level launches from the others
template <uint32_t C, uint32_t TPB, typename TT = float, bool FEW_LEVELS = false>
__global__ __launch_bounds__(TPB) void k_march_features_td(UcnLevels lvls, const TT *__restrict__ table, RayInputs in,
                                                           HexPattern hx, float std_scale, uint32_t N, uint32_t S,
                                                           LevelGroups grp, int layout, float *__restrict__ features,
                                                           float *__restrict__ coord_out, float *__restrict__ tmean_out) {
    march_features_body<C, TPB, TT, true>(lvls, table, in, hx, std_scale, N, S, grp, layout, features, coord_out, tmean_out);
}

// MLP.warp_fn = None (a bounded scene inside [-1, 1]^3): the Gaussians go to the grid as cast, points outside the cube add
// nothing (in_unit_cube, bounds inclusive) and still count in the mean of six.  Kernels of their own name with the fencepost
// kind as a template argument, FEW_LEVELS last as above; the warped kernels keep their symbols and their code.
template <uint32_t C, uint32_t TPB, typename TT = float, bool TD = false, bool FEW_LEVELS = false>
__global__ __launch_bounds__(TPB) void k_march_features_unwarped(UcnLevels lvls, const TT *__restrict__ table, RayInputs in,
                                                                 HexPattern hx, float std_scale, uint32_t N, uint32_t S,
                                                                 LevelGroups grp, int layout, float *__restrict__ features,
                                                                 float *__restrict__ coord_out, float *__restrict__ tmean_out) {
    march_features_body<C, TPB, TT, TD, false>(lvls, table, in, hx, std_scale, N, S, grp, layout, features, coord_out, tmean_out);
}

// predict_density's featurisation for caller-supplied Gaussians (extract.py / API parity)
template <uint32_t C>
__global__ __launch_bounds__(256) void k_points_features(UcnLevels lvls, const float *__restrict__ table,
                                                         const float *__restrict__ means, const float *__restrict__ stds,
                                                         uint32_t Bn, uint32_t G, int warp, uint32_t lpb,
                                                         float *__restrict__ features, float *__restrict__ coord_out) {
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= Bn) return;
    float u[6][3], rs[6];
    float cs0 = 0.0f, cs1 = 0.0f, cs2 = 0.0f;
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        if (j < G) {
            const float *m = means + (b * G + j) * 3;
            float c0, c1, c2;
            contract_to_unit(m[0], m[1], m[2], stds[b * G + j], warp != 0, u[j][0], u[j][1], u[j][2], rs[j], c0, c1, c2);
            cs0 += c0; cs1 += c1; cs2 += c2;
        } else {
            u[j][0] = u[j][1] = u[j][2] = 0.0f; rs[j] = 1.0f;
        }
    }
    const uint32_t lvl0 = blockIdx.y * lpb;
    const uint32_t lvl1 = lvl0 + lpb < lvls.L ? lvl0 + lpb : lvls.L;
    featurise<C, float>(lvls, table, [](uint32_t i) -> uint32_t { return i; }, lvl0, lvl1, u, rs, G, Bn, b, features, false);
    if (blockIdx.y == 0 && coord_out) {
        coord_out[b * 3 + 0] = cs0 / (float)G; coord_out[b * 3 + 1] = cs1 / (float)G; coord_out[b * 3 + 2] = cs2 / (float)G;
    }
}

}  // namespace

template <bool TD, bool WARP>
static int march_features_launch(const ucn_field_t *f, const RayInputs &in, float std_scale, uint32_t N, uint32_t S,
                                 uint32_t levels_per_block, int layout, float *features_out, float *coord_out, float *tmean_out,
                                 ucn_stream_t stream) {
    UCN_REQUIRE(N == 0 || (in.sdist && (TD || (in.near_ && in.far_)) && in.origins && in.dirs && in.basis && in.radii && features_out),
                "march_features: null pointer argument");
    UCN_REQUIRE((in.flip == nullptr) == (in.spin == nullptr), "march_features: flip and spin come together");
    const bool coresident = (layout & UCN_LAUNCH_CORESIDENT) != 0;
    const bool half_table = (layout & UCN_TABLE_F16) != 0;
    const bool out_bf16 = (layout & UCN_FEATURES_BF16) != 0;
    const bool incoherent = (layout & UCN_RAYS_INCOHERENT) != 0;
    layout &= ~(UCN_LAUNCH_CORESIDENT | UCN_TABLE_F16 | UCN_FEATURES_BF16 | UCN_RAYS_INCOHERENT);
    UCN_REQUIRE(!(half_table && coresident), "march_features: the co-resident launch shape reads fp32 tables");
    UCN_REQUIRE(layout >= 0 && layout <= 2, "march_features: layout must be 0, 1 or 2");
    UCN_REQUIRE(!out_bf16 || (half_table && f->level_dim == 2 && layout != 1),
                "march_features: bf16 features come with half tables, level_dim 2 and a level-major layout");
    if (out_bf16) layout |= 0x10;                      // the kernel's private flags
    if (incoherent) layout |= 0x20;
    UcnLevels lv;
    if (int rc = field_levels(f, &lv)) return rc;
    if (N == 0) return 0;
    const size_t B = (size_t)N * S;
    UCN_REQUIRE(B <= 0xFFFFFF00ull, "march_features: too many samples in one call (%zu)", B);
    const LevelGroups grp = make_groups(lv, levels_per_block, incoherent);
    const HexPattern hx = make_hex();
    hipStream_t st = (hipStream_t)stream;
    // co-resident shape: 512 threads = two waves per SIMD, 88 KiB of LDS reserved -> ONE such workgroup per CU, and
    // room for one MLP workgroup (72 KiB, one 296-register wave per SIMD) beside it.  The kernel runs at 97 % of its
    // full-occupancy rate with two waves per SIMD (profiles/r02*/occupancy.txt): it is bound by the L2 request rate.
    const uint32_t tpb = coresident ? 512u : 256u;
    const size_t lds = coresident ? 88u * 1024u : 0u;
    const dim3 grid(ucn_div_up(B, tpb), grp.n);
// UCN_MF3(kernel, C, trailing template arguments ...): the three launch shapes of one gather kernel
#define UCN_MF3(KF, CC, ...)                                                                                              \
    do {                                                                                                                  \
        if (half_table)                                                                                                   \
            hipLaunchKernelGGL((KF<CC, 256, _Float16, __VA_ARGS__>), grid, dim3(256), lds, st, lv,                        \
                               reinterpret_cast<const _Float16 *>(f->embeddings), in, hx, std_scale, N, S, grp, layout,   \
                               features_out, coord_out, tmean_out);                                                       \
        else if (coresident)                                                                                              \
            hipLaunchKernelGGL((KF<CC, 512, float, __VA_ARGS__>), grid, dim3(512), lds, st, lv, f->embeddings, in, hx,    \
                               std_scale, N, S, grp, layout, features_out, coord_out, tmean_out);                         \
        else                                                                                                              \
            hipLaunchKernelGGL((KF<CC, 256, float, __VA_ARGS__>), grid, dim3(256), lds, st, lv, f->embeddings, in, hx,    \
                               std_scale, N, S, grp, layout, features_out, coord_out, tmean_out);                         \
    } while (0)
#define UCN_MF2(CC, FEW)                                                                                                  \
    do {                                                                                                                  \
        if constexpr (!WARP) UCN_MF3(k_march_features_unwarped, CC, TD, FEW);                                             \
        else if constexpr (TD) UCN_MF3(k_march_features_td, CC, FEW);                                                     \
        else UCN_MF3(k_march_features, CC, FEW);                                                                          \
    } while (0)
    ucn_for_level_dim(lv.C, [&](auto cc) {
        constexpr uint32_t CC = decltype(cc)::value;
        if (lv.L <= 8) UCN_MF2(CC, true);
        else UCN_MF2(CC, false);
    });
#undef UCN_MF3
#undef UCN_MF2
    UCN_LAUNCH_CHECK("march_features");
    return 0;
}

extern "C" int ucn_march_features_warp(const ucn_field_t *f, const float *fenceposts, const float *near_, const float *far_,
                                       const float *origins, const float *directions, const float *basis, const float *radii,
                                       const float *flip, const float *spin, float std_scale, int warp, uint32_t N, uint32_t S,
                                       uint32_t levels_per_block, int layout, float *features_out, float *coord_out,
                                       float *tmean_out, ucn_stream_t stream) {
    UCN_REQUIRE(warp == 0 || warp == 1, "march_features: warp must be 0 (MLP.warp_fn = None) or 1 ('contract'), got %d", warp);
    UCN_REQUIRE(N == 0 || (near_ == nullptr) == (far_ == nullptr), "march_features: near and far come together (both NULL: metric fenceposts)");
    const RayInputs in{fenceposts, near_, far_, origins, directions, basis, radii, flip, spin};
    int rc = 0;
    ucn_for_bool(near_ == nullptr, [&](auto td) {
        ucn_for_bool(warp != 0, [&](auto w) {
            rc = march_features_launch<decltype(td)::value, decltype(w)::value>(f, in, std_scale, N, S, levels_per_block, layout,
                                                                                features_out, coord_out, tmean_out, stream);
        });
    });
    return rc;
}

extern "C" int ucn_march_features(const ucn_field_t *f, const float *sdist, const float *near_, const float *far_,
                                  const float *origins, const float *directions, const float *basis,
                                  const float *radii, const float *flip, const float *spin, float std_scale,
                                  uint32_t N, uint32_t S, uint32_t levels_per_block, int layout,
                                  float *features_out, float *coord_out, float *tmean_out, ucn_stream_t stream) {
    UCN_REQUIRE(N == 0 || (near_ && far_), "march_features: null pointer argument");
    return ucn_march_features_warp(f, sdist, near_, far_, origins, directions, basis, radii, flip, spin, std_scale, 1, N, S,
                                   levels_per_block, layout, features_out, coord_out, tmean_out, stream);
}

extern "C" int ucn_march_features_tdist(const ucn_field_t *f, const float *tdist, const float *origins,
                                        const float *directions, const float *basis, const float *radii, const float *flip,
                                        const float *spin, float std_scale, uint32_t N, uint32_t S, uint32_t levels_per_block,
                                        int layout, float *features_out, float *coord_out, float *tmean_out,
                                        ucn_stream_t stream) {
    return ucn_march_features_warp(f, tdist, nullptr, nullptr, origins, directions, basis, radii, flip, spin, std_scale, 1, N, S,
                                   levels_per_block, layout, features_out, coord_out, tmean_out, stream);
}

template <bool TD, bool WARP>
static int cast_probe_launch(const RayInputs &in, float std_scale, uint32_t N, uint32_t S, float *out, ucn_stream_t stream) {
    UCN_REQUIRE(N == 0 || (in.sdist && (TD || (in.near_ && in.far_)) && in.origins && in.dirs && in.basis && in.radii && out),
                "cast_probe: null pointer argument");
    UCN_REQUIRE((in.flip == nullptr) == (in.spin == nullptr), "cast_probe: flip and spin come together");
    if (N == 0 || S == 0) return 0;
    hipLaunchKernelGGL((k_cast_probe<TD, WARP>), dim3(ucn_div_up((size_t)N * S, 256)), dim3(256), 0, (hipStream_t)stream, in, make_hex(),
                       std_scale, N, S, out);
    UCN_LAUNCH_CHECK("cast_probe");
    return 0;
}

extern "C" int ucn_cast_probe_warp(const float *fenceposts, const float *near_, const float *far_, const float *origins,
                                   const float *directions, const float *basis, const float *radii, const float *flip,
                                   const float *spin, float std_scale, int warp, uint32_t N, uint32_t S, float *out,
                                   ucn_stream_t stream) {
    UCN_REQUIRE(warp == 0 || warp == 1, "cast_probe: warp must be 0 (MLP.warp_fn = None) or 1 ('contract'), got %d", warp);
    UCN_REQUIRE(N == 0 || (near_ == nullptr) == (far_ == nullptr), "cast_probe: near and far come together (both NULL: metric fenceposts)");
    const RayInputs in{fenceposts, near_, far_, origins, directions, basis, radii, flip, spin};
    int rc = 0;
    ucn_for_bool(near_ == nullptr, [&](auto td) {
        ucn_for_bool(warp != 0, [&](auto w) { rc = cast_probe_launch<decltype(td)::value, decltype(w)::value>(in, std_scale, N, S, out, stream); });
    });
    return rc;
}

extern "C" int ucn_cast_probe(const float *sdist, const float *near_, const float *far_, const float *origins,
                              const float *directions, const float *basis, const float *radii, const float *flip,
                              const float *spin, float std_scale, uint32_t N, uint32_t S, float *out, ucn_stream_t stream) {
    UCN_REQUIRE(N == 0 || (near_ && far_), "cast_probe: null pointer argument");
    return ucn_cast_probe_warp(sdist, near_, far_, origins, directions, basis, radii, flip, spin, std_scale, 1, N, S, out, stream);
}

extern "C" int ucn_cast_probe_tdist(const float *tdist, const float *origins, const float *directions, const float *basis,
                                    const float *radii, const float *flip, const float *spin, float std_scale, uint32_t N,
                                    uint32_t S, float *out, ucn_stream_t stream) {
    return ucn_cast_probe_warp(tdist, nullptr, nullptr, origins, directions, basis, radii, flip, spin, std_scale, 1, N, S, out,
                               stream);
}

extern "C" int ucn_contract_probe(const float *means, const float *stds, uint32_t B, float *out_mean, float *out_std,
                                  ucn_stream_t stream) {
    UCN_REQUIRE(B == 0 || (means && stds && out_mean && out_std), "contract_probe: null pointer argument");
    if (B == 0) return 0;
    hipLaunchKernelGGL(k_contract_probe, dim3(ucn_div_up(B, 256)), dim3(256), 0, (hipStream_t)stream, means, stds, B, out_mean,
                       out_std);
    UCN_LAUNCH_CHECK("contract_probe");
    return 0;
}

/* The level groups of ucn_march_features for this grid (host only, no launch): group g = levels_out[first_out[g]] ...
 * levels_out[first_out[g + 1] - 1] in the thread's order; layout: only UCN_RAYS_INCOHERENT is looked at; levels_out [num_levels], first_out [num_levels + 1];
 * returns the number of groups, or -1 on a bad argument. */
extern "C" int ucn_level_groups_probe(const ucn_field_t *f, uint32_t levels_per_block, int layout, uint32_t *levels_out,
                                      uint32_t *first_out) {
    UcnLevels lv;
    if (!levels_out || !first_out || field_levels(f, &lv)) return -1;
    const LevelGroups grp = make_groups(lv, levels_per_block, (layout & UCN_RAYS_INCOHERENT) != 0);
    for (uint32_t i = 0; i < lv.L; i++) levels_out[i] = grp.list[i];
    for (uint32_t g = 0; g <= grp.n; g++) first_out[g] = grp.lo[g];
    return (int)grp.n;
}

extern "C" int ucn_points_features(const ucn_field_t *f, const float *means, const float *stds, uint32_t B, uint32_t G,
                                   int warp, uint32_t levels_per_block, float *features_out, float *coord_out,
                                   ucn_stream_t stream) {
    UCN_REQUIRE(means && stds && features_out, "points_features: null pointer argument");
    UCN_REQUIRE(G >= 1 && G <= 6, "points_features: 1..6 Gaussians per feature, got %u", G);
    UcnLevels lv;
    if (int rc = field_levels(f, &lv)) return rc;
    if (B == 0) return 0;
    if (levels_per_block == 0) levels_per_block = 1;
    const dim3 grid(ucn_div_up(B, 256), ucn_div_up(lv.L, levels_per_block));
    hipStream_t st = (hipStream_t)stream;
    ucn_for_level_dim(lv.C, [&](auto cc) {
        hipLaunchKernelGGL(k_points_features<decltype(cc)::value>, grid, dim3(256), 0, st, lv, f->embeddings, means, stds, B, G,
                           warp, levels_per_block, features_out, coord_out);
    });
    UCN_LAUNCH_CHECK("points_features");
    return 0;
}
