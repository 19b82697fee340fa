// d(loss)/d(table) of the fused sample featurisation (march_features.hip): the global-atomic scatter
// (k_march_features_bwd), the row-block kernel (k_march_features_bwd_blk) and the compacted row-block kernel
// (k_cast_cache_masks + k_march_features_bwd_cmp, float or fixed-point rows), with the one host route decision
// between them (bwd_row_block_plan).  means / stds carry no gradient, so every kernel here re-derives the forward's six
// Gaussians (grid_cast.h) and corner rows (grid_rows.h) and scatters where the gather read.
#include "ucn_common.h"
#include "wave_dpp.h"
#include "grid_cast.h"
#include "grid_rows.h"
#include <type_traits>

namespace {

// Backward of level_accumulate w.r.t. the table: grad_table[row_k] += w_k * damp_j * g
// (gridencoder.cu:304-339 composed with models.py:495-496).  When all multisamples of the sample share
// one lattice cell (coarse levels) their corner weights are summed first: 8*C atomics instead of 48*C
// -- atomics, unlike loads, do not coalesce across lanes.
template <uint32_t C, bool HASHED, bool POW2>
__device__ __forceinline__ void level_scatter(const UcnLevel &lv, float *__restrict__ gtab, const float (&u)[6][3],
                                              const float (&rs)[6], uint32_t G, const float (&gout)[C]) {
    uint32_t rows0[8];
    float wsum[8];
    bool have0 = false, shared = true;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) { wsum[k] = 0.0f; rows0[k] = 0u; }
    // pass 1: is it one cell?  (compare the corner-0 row and the integer cell through rows[0], rows[7])
    float fxs[6], fys[6], fzs[6];
    uint32_t r0s[6], r7s[6];
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        fxs[j] = fys[j] = fzs[j] = 0.0f; r0s[j] = r7s[j] = 0u;
        if (j < G) {
            if (!in_unit_cube(u[j][0], u[j][1], u[j][2])) { shared = false; continue; }
            uint32_t rows[8];
            corner_rows<HASHED, POW2>(lv, u[j][0], u[j][1], u[j][2], fxs[j], fys[j], fzs[j], rows);
            r0s[j] = rows[0]; r7s[j] = rows[7];
            if (!have0) {
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) rows0[k] = rows[k];
                have0 = true;
            } else if (rows[0] != rows0[0] || rows[7] != rows0[7] || rows[1] != rows0[1] || rows[2] != rows0[2] ||
                       rows[4] != rows0[4]) {
                shared = false;
            }
        }
    }
    if (shared && have0) {
#pragma unroll
        for (uint32_t j = 0; j < 6; j++) {
            if (j < G) {
                float w[8];
                corner_weights(fxs[j], fys[j], fzs[j], w);
                const float damp = erf_pos(rs[j] * lv.inv_gs);
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) wsum[k] += w[k] * damp;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            float *r = gtab + (size_t)rows0[k] * C;
#pragma unroll
            for (uint32_t c = 0; c < C; c++) atomicAdd(r + c, wsum[k] * gout[c]);
        }
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        if (j < G && in_unit_cube(u[j][0], u[j][1], u[j][2])) {
            float fx, fy, fz, w[8];
            uint32_t rows[8];
            corner_rows<HASHED, POW2>(lv, u[j][0], u[j][1], u[j][2], fx, fy, fz, rows);
            corner_weights(fx, fy, fz, w);
            const float damp = erf_pos(rs[j] * lv.inv_gs);
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                float *r = gtab + (size_t)rows[k] * C;
#pragma unroll
                for (uint32_t c = 0; c < C; c++) atomicAdd(r + c, (w[k] * damp) * gout[c]);
            }
        }
    }
}

// acc[r][0..C) += v in the workgroup's LDS row block.  ds_add_f32 is serialised per LANE on gfx950 (measured with
// tools/lds_atomic_bench.hip: 193 clk per wave instruction, 3 clk per active lane, whatever the addresses -- 40x
// the integer ds_add_u32).  An 8-byte compare-and-swap updates two channels per ds_cmpst_rtn_b64 in 24-37 clk per
// wave when the lanes hit different rows, and is still an exact fp32 add per addend -- but a lane whose row was
// changed in between has to retry, and on the coarser levels neighbouring lanes DO share rows.  So:
//   CAS = false (coarse levels, run-merged updates): plain ds_add_f32, contention-proof;
//   CAS = true  (fine levels): one compare-and-swap attempt, the lanes that lose fall back to ds_add_f32.
// FIXED-POINT accumulation (the autocast training step; r04).  The row block may hold, instead of C floats per row, C / 2
// 64-bit words per row, each TWO int32 fixed-point channels: word = (b << 32) + sign_extend(a).  One fire-and-forget ds_add_u64
// per channel pair replaces the read + compare-and-swap round trip (53 % of this kernel's instruction waits were LDS,
// profiles/r03/pmc_table_train.txt): integer adds are associative, so the 64-bit total is exact mod 2^64 whatever the order, and
// it splits back uniquely into (a, b) as long as each channel's FINAL sum fits int32.  That is guaranteed, not hoped for: the
// addends of a sample are (w_k damp / 6) g_c with sum_k w_k = 1, damp <= 1, six points -- their absolute values sum to at most
// |g_c|, so any row's |sum| <= L1 = sum over the task's samples of |g| (accumulated by the mask pass); the task scales its
// gradients by the power of two that puts L1 at <= 2^30.  Rounding adds <= 1/2 per addend and a task has <= 48 B addends per row at
// the very worst (6 points x 8 corners of every one of its B <= 2^22 samples landing on ONE row): 2^30 + 24 x 2^22 < 2^30.1 < 2^31
// (the host entry asserts exactly this inequality).  A non-finite gradient among the task's samples poisons the task's WHOLE row
// block on that level with NaN (the float rows poison the touched rows only; after the reference's nan_to_num, train_utils.py:342,
// both lose that step's gradient for those rows -- a superset here, never a silently dropped NaN).  The
// accumulator type selects the mode: `float` rows (exact fp32 adds, the fp32 route and every test of it) or `FxLane` rows.
struct FxLane { float raw; };                                  // same size as float: row / channel pointer arithmetic is shared
template <typename A> constexpr bool kFixed = false;
template <> constexpr bool kFixed<FxLane> = true;
__device__ __forceinline__ unsigned long long fixed_pack(float a, float b) {
    const long long ia = (long long)__float2int_rn(a), ib = (long long)__float2int_rn(b);
    return (unsigned long long)((ib << 32) + ia);
}
__device__ __forceinline__ void fixed_unpack(unsigned long long w, float inv, float &a, float &b) {
    const int lo = (int)(uint32_t)w;
    const long long hi = ((long long)w - (long long)lo) >> 32;
    a = (float)lo * inv;
    b = (float)(int)hi * inv;
}
template <uint32_t C, bool CAS, typename A>
__device__ __forceinline__ void lds_row_add(A *acc_, uint32_t r, const float (&v)[C]) {
    if constexpr (kFixed<A>) {
        static_assert(C % 2u == 0u, "fixed-point rows pack channel pairs");
#pragma unroll
        for (uint32_t c = 0; c < C; c += 2) atomicAdd(reinterpret_cast<unsigned long long *>(acc_ + r * C + c), fixed_pack(v[c], v[c + 1]));
        return;
    }
    float *acc = reinterpret_cast<float *>(acc_);
    if constexpr (CAS && (C % 2u == 0u)) {
#pragma unroll
        for (uint32_t c = 0; c < C; c += 2) {
            unsigned long long *p = reinterpret_cast<unsigned long long *>(acc + r * C + c);
            const unsigned long long seen = *p;
            float2 t = __builtin_bit_cast(float2, seen);
            t.x += v[c];
            t.y += v[c + 1];
            if (atomicCAS(p, seen, __builtin_bit_cast(unsigned long long, t)) != seen) {
                atomicAdd(acc + r * C + c, v[c]);
                atomicAdd(acc + r * C + c + 1, v[c + 1]);
            }
        }
    } else {
#pragma unroll
        for (uint32_t c = 0; c < C; c++) atomicAdd(acc + r * C + c, v[c]);
    }
}

// Run merging for coarse levels: the six multisamples of a sample mostly sit in one lattice cell, and so do the
// neighbouring samples of the ray -- the LDS updates of such a level serialise on a handful of rows (level 0 of
// the benchmark grid took 16x a fine level).  Consecutive points with the same 8 rows are summed in registers
// first: 8 row updates per RUN instead of per point.  The state is carried by the caller, so a lane that walks
// several consecutive samples (the compacted kernel) keeps merging across them.
// (A rows-only pre-pass that drops samples without a corner in this block was tried: with 64 lanes per wave
//  some lane almost always stays, so the wave pays the pre-pass AND the full path -- 25 % slower.)
// C > 2 (r05; the reference's own waymo.gin grid is C = 4): the run keeps ONE summed corner weight per row instead of C values -- 16
// registers of state instead of 8 + 8 C -- and is flushed at the end of every sample with that sample's gradient (v = weight x g), so
// it no longer merges ACROSS samples.  With v[8][4] the kernel's 128-register budget (1024 threads) did not hold a run, the next item's
// prefetched geometry and a point's corner arithmetic together: the C = 4 instantiation spilled 405 registers, 500 of its 1561 scratch
// accesses in run_flush alone, inside the item loops of every coarse level (the whole proposal grid of waymo.gin).
template <uint32_t C>
struct RowRun {
    static constexpr bool kLean = C > 2;
    uint32_t cur[8];
    float v[8][kLean ? 1 : C];
    bool have;
};

template <uint32_t C, typename A>
__device__ __forceinline__ void run_flush(A *__restrict__ acc, uint32_t row_lo, uint32_t nrows, const RowRun<C> &run, const float (&gout)[C]) {
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t r = run.cur[k] - row_lo;
        if (r < nrows) {
            if constexpr (RowRun<C>::kLean) {
                float val[C];
#pragma unroll
                for (uint32_t c = 0; c < C; c++) val[c] = run.v[k][0] * gout[c];
                lds_row_add<C, false>(acc, r, val);
            } else {
                lds_row_add<C, false>(acc, r, run.v[k]);
            }
        }
    }
}

template <uint32_t C, bool HASHED, bool POW2, typename A>
__device__ __forceinline__ void run_merge_sample(const UcnLevel &lv, A *__restrict__ acc, uint32_t row_lo, uint32_t nrows,
                                                 const float (&u)[6][3], const float (&rs)[6], const float (&gout)[C],
                                                 RowRun<C> &run) {
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        if (in_unit_cube(u[j][0], u[j][1], u[j][2])) {
            float fx, fy, fz, w[8];
            uint32_t rows[8];
            corner_rows<HASHED, POW2>(lv, u[j][0], u[j][1], u[j][2], fx, fy, fz, rows);
            corner_weights(fx, fy, fz, w);
            const float damp = erf_pos(rs[j] * lv.inv_gs);
            bool same = run.have;
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) same = same && rows[k] == run.cur[k];
            if (run.have && !same) run_flush<C>(acc, row_lo, nrows, run, gout);
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                const float wd = w[k] * damp;
                if constexpr (RowRun<C>::kLean) {
                    run.v[k][0] = same ? run.v[k][0] + wd : wd;
                } else {
#pragma unroll
                    for (uint32_t c = 0; c < C; c++) run.v[k][c] = same ? run.v[k][c] + wd * gout[c] : wd * gout[c];
                }
                run.cur[k] = rows[k];
            }
            run.have = true;
        }
    }
    if constexpr (RowRun<C>::kLean) {                                 // the run's weights belong to THIS sample's gradient
        if (run.have) run_flush<C>(acc, row_lo, nrows, run, gout);
        run.have = false;
    }
}

// Row-block variant of level_scatter: only corners whose row lies in [row_lo, row_lo + nrows) count, and
// they go to the workgroup's LDS copy of that row block (lds_row_add).
template <uint32_t C, bool HASHED, bool POW2, bool MERGE, typename A>
__device__ __forceinline__ void level_scatter_block(const UcnLevel &lv, A *__restrict__ acc, uint32_t row_lo,
                                                    uint32_t nrows, const float (&u)[6][3], const float (&rs)[6],
                                                    const float (&gout)[C]) {
    if constexpr (MERGE) {
        RowRun<C> run;
        run.have = false;
        run_merge_sample<C, HASHED, POW2>(lv, acc, row_lo, nrows, u, rs, gout, run);
        if (run.have) run_flush<C>(acc, row_lo, nrows, run, gout);
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        if (in_unit_cube(u[j][0], u[j][1], u[j][2])) {
            float fx, fy, fz;
            uint32_t rows[8];
            corner_rows<HASHED, POW2>(lv, u[j][0], u[j][1], u[j][2], fx, fy, fz, rows);
            bool any = false;
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                rows[k] -= row_lo;                      // uint32 wrap: rows below the block become huge
                any |= rows[k] < nrows;
            }
            if (any) {
                float w[8];
                corner_weights(fx, fy, fz, w);
                const float damp = erf_pos(rs[j] * lv.inv_gs);
#pragma unroll
                for (uint32_t k = 0; k < 8; k++)
                    if (rows[k] < nrows) {
                        float v[C];
#pragma unroll
                        for (uint32_t c = 0; c < C; c++) v[c] = (w[k] * damp) * gout[c];
                        lds_row_add<C, true>(acc, rows[k], v);
                    }
            }
        }
    }
}

template <uint32_t C>
__device__ __forceinline__ void featurise_bwd(const UcnLevels &lvls, float *__restrict__ grad_table, uint32_t lvl0,
                                              uint32_t lvl1, const float (&u)[6][3], const float (&rs)[6], uint32_t G,
                                              size_t B, size_t b, const float *__restrict__ grad, bool sample_major) {
    const uint32_t F = lvls.L * C;
    for (uint32_t lvl = lvl0; lvl < lvl1; lvl++) {
        const UcnLevel lv = lvls.lv[lvl];
        float *gtab = grad_table + (size_t)lv.first_row * C;
        const float *gp = sample_major ? grad + b * F + (size_t)lvl * C : grad + ((size_t)lvl * B + b) * C;
        float gout[C];
#pragma unroll
        for (uint32_t c = 0; c < C; c++) gout[c] = gp[c] / (float)G;          // d(mean over G)
        if (lv.hashed) {
            if (lv.mask) level_scatter<C, true, true>(lv, gtab, u, rs, G, gout);
            else level_scatter<C, true, false>(lv, gtab, u, rs, G, gout);
        } else {
            if (lv.mask) level_scatter<C, false, true>(lv, gtab, u, rs, G, gout);
            else level_scatter<C, false, false>(lv, gtab, u, rs, G, gout);
        }
    }
}

// d(loss)/d(table) of k_march_features.  (means/stds carry no gradient: coord.track_linearize is
// @torch.no_grad, coord.py:75, and sdist is detached, models.py:204-205.)  fp32 atomics in L2, like
// kernel_grid_backward (gridencoder.cu:336).
//
// WARP (every kernel below that re-derives the Gaussians): cast_sample<TD, WARP>, false = MLP.warp_fn = None, the Gaussians as cast.
// The kernels that read the geometry cache (k_march_features_bwd_cmp, the cached route of *_blk) need neither TD nor WARP.
template <uint32_t C, bool TD = false, bool WARP = true>
__global__ __launch_bounds__(256) void k_march_features_bwd(UcnLevels lvls, float *__restrict__ grad_table, RayInputs in,
                                                            HexPattern hx, float std_scale, uint32_t N, uint32_t S,
                                                            uint32_t lpb, int layout,
                                                            const float *__restrict__ grad_features) {
    const size_t B = (size_t)N * S;
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    const uint32_t ray = (uint32_t)(b / S), s = (uint32_t)(b - (size_t)ray * S);
    float u[6][3], rs[6], csum[3], tsum;
    cast_sample<TD, WARP>(in, hx, std_scale, ray, s, S, u, rs, csum, tsum);
    const uint32_t lvl0 = blockIdx.y * lpb;
    const uint32_t lvl1 = lvl0 + lpb < lvls.L ? lvl0 + lpb : lvls.L;
    featurise_bwd<C>(lvls, grad_table, lvl0, lvl1, u, rs, 6, B, b, grad_features, layout == 1);
}

// Same gradient without global atomics.  Scattered fp32 atomics run at ~21 G/s on MI355X whatever their
// scope (tools/atomic_bench.hip: 50 M row updates x 2 channels = 4.8 ms, against 0.14 ms for the forward's
// gathers of the same rows), and a hashed level receives ~100 updates per row per 8192-ray batch.  So:
// one workgroup OWNS a block of `rpb` rows of one level (128 KiB of LDS), walks ALL samples, recomputes
// their corners (VALU is cheap here) and accumulates the ones that fall in its block with ds_add_f32;
// the block is then added to the table gradient with plain coalesced read-modify-writes -- no other
// workgroup touches those rows.  blockIdx.x enumerates (level, block) pairs, level-major.
// The six contracted multisample positions and damping arguments of every sample, as [N*S][6] float4
// {x, y, z, std argument} (one 16-byte load per point for the compacted kernel's scattered items): written once
// per backward call, read by every (level, row block) workgroup.
template <bool TD = false, bool WARP = true>
__global__ __launch_bounds__(256) void k_cast_cache(RayInputs in, HexPattern hx, float std_scale, uint32_t N, uint32_t S,
                                                    float *__restrict__ geom) {
    const size_t B = (size_t)N * S;
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    const uint32_t ray = (uint32_t)(b / S), s = (uint32_t)(b - (size_t)ray * S);
    float u[6][3], rs[6], csum[3], tsum;
    cast_sample<TD, WARP>(in, hx, std_scale, ray, s, S, u, rs, csum, tsum);
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        reinterpret_cast<float4 *>(geom)[b * 6 + j] = make_float4(u[j][0], u[j][1], u[j][2], rs[j]);
    }
}

// ---- block masks: which row blocks of a level a sample touches.  Planes of [N*S] uint32 behind the geometry
// cache; a COARSE level (resolution <= 512: items are whole samples, run-merged; coarse = 2 up to resolution 64:
// a lane walks consecutive samples) has one plane = union over its 48 corners, bit p = some corner's row lies in
// block p (rows >> shift); a fine level one plane per GROUP of four blocks, bit 4 * j + (p & 3) of word p >> 2 =
// multisample j has a corner in block p -- either way a workgroup reads one word per sample.
// Where element (level, sample b, channel c) of the feature gradient lives: level * L + b * S + c * Cs floats.
//   layout 0 = [L][B][C]   1 = [B][L*C] (what autograd hands over)   3 = [L*C][B] (a transposed dgrad GEMM)
struct GradStrides {
    size_t level, sample, chan;
};
static GradStrides grad_strides(int layout, size_t B, uint32_t L, uint32_t C) {
    if (layout == 1) return {C, (size_t)L * C, 1};
    if (layout == 3) return {(size_t)C * B, 1, B};
    return {B * C, C, 1};
}

constexpr uint32_t kScan = 4;                                  // samples per thread and scan step (8 measured: see DESIGN)
constexpr uint32_t kMaxMaskWords = 16;                  // sample-item levels: up to 512 row blocks (16 KiB of LDS in the mask pass)
struct MaskPlan {
    uint16_t plane[UCN_MAX_LEVELS];
    uint8_t coarse[UCN_MAX_LEVELS];
    uint32_t n_planes, shift;
    uint16_t split[UCN_MAX_LEVELS];        // workgroups per row block (cut along the samples): ~128 per level, 256 for the last
    uint8_t order[UCN_MAX_LEVELS];         // levels in the order their workgroups are dispatched: longest workgroups first
    uint8_t fine_kind[UCN_MAX_LEVELS];     // point-item levels: 0 = ballot-ordered items + corner walk, 2 = lane-ordered items + (y, z) combinations, 3 = 2 on byte planes (cmp_block_bytes)
};
__host__ __device__ __forceinline__ uint32_t bwd_sample_split(uint32_t blocks_in_level, uint32_t target = 128u) {
    return blocks_in_level >= target ? 1u : target / blocks_in_level;     // ~`target` workgroups per level (default 128)
}
static bool make_mask_plan(const UcnLevels &lv, uint32_t rpb, size_t B, MaskPlan *mp, bool fixed_rows) {
    uint32_t shift = 0;
    while ((1u << shift) < rpb) shift++;
    if ((1u << shift) != rpb) return false;
    mp->shift = shift;
    mp->n_planes = 0;
    for (uint32_t l = 0; l < lv.L; l++) {
        const uint32_t nb_l = (lv.lv[l].rows + rpb - 1) / rpb;
        if (nb_l > kMaxMaskWords * 32u) return false;                     // (> 512 blocks, e.g. 2^23 rows of C = 4: the atomic fallback)
        // measured per level on the benchmark grid (tools/level_times_bwd.py): sample items + run merging win up to
        // resolution 512, walking consecutive samples in one lane up to 64
        // r06, FIXED-POINT rows (the autocast step): a row update is one fire-and-forget ds_add_u64 there, so run merging buys nothing
        // and the ~8 row blocks a SAMPLE of the hashed levels 84 ... 446 touches each redo all of its 48 corners; as point items on byte
        // planes those levels cost 44-47 instead of 45-82 ms-CU each (whole call 3.54 -> 3.20 ms; profiles/r06/bwd_coarse_res_fx.txt).
        // With float rows the same change LOSES (3.71 -> 5.3 ms: compare-and-swap collisions; bwd_coarse_res_float.txt), so the
        // threshold follows the row type.
        const uint32_t coarse_res = fixed_rows ? 64u : 512u;
        mp->coarse[l] = lv.lv[l].resolution <= coarse_res ? 1 : 0;
        // (r06: under fixed-point rows the plain sample item is cheaper than the walk on the dense levels too -- call 3.205 -> 3.164 ms --
        // but merging runs ACROSS six samples also means six times fewer ROUNDED addends on exactly the rows that collect the most
        // samples: 2.4 x the fixed-point noise there for 1 % of the step.  Not taken: 64 for both row types)
        if (mp->coarse[l] && !lv.lv[l].hashed && lv.lv[l].resolution <= 64u) mp->coarse[l] = 2;
        // More than 32 row blocks per level (the reference's own waymo.gin grid: T = 2^21 rows of C = 4 -> 256 blocks of 8192 rows):
        // the per-point masks of the point-item shapes would need 6 bits x 256 blocks per sample and level, so such a level goes by
        // SAMPLE items as well -- one bit per (sample, block) in nb / 32 mask words -- with the unmerged per-point scatter (a point's
        // corners lie in ~4.5 of the 256 blocks: the `any corner in my block` test drops most points before weights and erf).
        // Before r03 these configurations fell back to the global-atomic kernel: 83.6 of the 88.5 ms of a waymo.gin training step.
        if (nb_l > 32u && mp->coarse[l] != 2) mp->coarse[l] = 3;         // (the run-merging dense levels keep their shape, with nb / 32 mask words)
        // Point-item levels (<= 32 row blocks), three shapes (ms-CU per level of the benchmark grid):
        //   0: items appended point by point (six ballots per step), all 8 corners walked          res 1024: 75, 2048: 62, finer: 60-62, strided: 78
        //   2: items appended lane by lane (popcount + one DPP prefix sum per step), the corners taken by (y, z) combinations
        //      (point_scatter_combos)                                                                 1024: 120, 2048: 78, finer: 51-55, strided: 60
        //   3 (r06): shape 2 on BYTE PLANES -- per row block one byte per sample (bit j = multisample j has a corner in the block), so
        //      that a scanning lane reads FOUR samples of ITS block in one dword (popcount 3.4 on average) where the nibble planes
        //      give it one sample of four blocks (0.84 hits).  Same number of planes; needs B % 4 == 0 (a quad of samples per dword).
        // Lane order puts the six points of a sample next to each other in a batch: where they still share lattice cells
        // (resolution <= 2048 on these rays) their compare-and-swaps collide and fall back to ds_add_f32 -- so float rows keep shape 0
        // there; fixed-point rows (fire-and-forget adds, nothing to collide) take byte planes on every point-item level.
        // (Removed after measurement, numbers in profiles/: shape 1 = lane order + corner walk, shape 4 = byte planes + corner walk.)
        mp->fine_kind[l] = 0;
        if (!mp->coarse[l]) {
            const uint8_t kind0 = (!lv.lv[l].hashed || lv.lv[l].resolution >= 4096u) ? 2 : 0;
            mp->fine_kind[l] = (B % 4u == 0u && (fixed_rows || kind0 == 2)) ? 3 : kind0;
        }
        mp->plane[l] = (uint16_t)mp->n_planes;
        if (mp->coarse[l] == 3) {
            // bit planes: [block][ceil(B / 64)] 64-bit words (one bit per sample) = nb x 2 x ceil(B / 64) 32-bit words, in units of B
            const uint64_t words = (uint64_t)nb_l * 2u * ((B + 63u) / 64u);
            mp->n_planes += (uint32_t)((words + B - 1u) / (B ? B : 1u));
        } else {
            mp->n_planes += mp->coarse[l] ? (nb_l + 31u) / 32u : (nb_l + 3u) / 4u;
        }
    }
    // Dispatch order = longest workgroups first, so that the chip drains on short ones (workgroup clocks of the benchmark
    // grid: in level order the last 1.3 ms of a 4.26 ms kernel ran at 50-85 % occupancy -- the two finest levels started at
    // 3.1 / 3.4 ms -- where the sum of the workgroup times is 3.70 ms per CU).  Classes by what was measured per workgroup:
    // unhashed levels of more than two row blocks load their blocks unevenly (the strided fine levels of the uint32-wrap quirk:
    // 150 ... 1010 us; the dense 65^3 level: 45 ... 890 us) and go first; then the hashed sample-item levels, finest first
    // (690 / 510 / 420 us); then the hashed point-item levels, coarsest first (600 ... 460 us); the small dense levels (140 us)
    // fill the tail.
    uint32_t key[UCN_MAX_LEVELS];
    for (uint32_t l = 0; l < lv.L; l++) {
        const uint32_t nb = (lv.lv[l].rows + rpb - 1) / rpb;
        uint32_t cls, sub;
        if (mp->coarse[l] == 3) { cls = 0u; sub = l; }                         // many short workgroups: they fill the tail
        else if (!lv.lv[l].hashed && nb > 2u) { cls = 3u; sub = l; }
        else if (lv.lv[l].hashed && mp->coarse[l]) { cls = 2u; sub = l; }
        else if (lv.lv[l].hashed) { cls = 1u; sub = UCN_MAX_LEVELS - 1u - l; }
        else { cls = 0u; sub = l; }
        key[l] = cls * 256u + sub;
        mp->order[l] = (uint8_t)l;
    }
    for (uint32_t i = 1; i < lv.L; i++)                                    // insertion sort, descending key
        for (uint32_t j = i; j > 0 && key[mp->order[j]] > key[mp->order[j - 1]]; j--) {
            const uint8_t t = mp->order[j]; mp->order[j] = mp->order[j - 1]; mp->order[j - 1] = t;
        }
    // ~128 workgroups per level (flat from 128 up, measured); the LAST long level of the order is cut twice as fine: the
    // chip drains on its workgroups (the small dense levels behind it are 35 ms-CU in all), and half-length ones halve that.
    // The unevenly loaded levels are cut twice as fine as well: their hottest block sets the longest workgroup of the call
    // (waymo.gin's proposal grid, 1 M samples: one 4.7 ms workgroup of the dense 65^3 level against 2.4 ms-CU of work per CU;
    // 1 / 2 / 4 / 8 measured: 2)
    int last_long = -1;
    for (uint32_t i = 0; i < lv.L; i++)
        if (key[mp->order[i]] >= 256u) last_long = (int)mp->order[i];
    for (uint32_t l = 0; l < lv.L; l++) {
        const uint32_t nb = (lv.lv[l].rows + rpb - 1) / rpb;
        const uint32_t mult = (key[l] >= 3u * 256u || (int)l == last_long) ? 2u : 1u;
        mp->split[l] = (uint16_t)bwd_sample_split(nb, mult * 128u);
    }
    return true;
}

template <bool HASHED, bool POW2>
__device__ __forceinline__ uint32_t point_block_mask(const UcnLevel &lv, uint32_t shift, const float (&p)[3]) {
    if (!in_unit_cube(p[0], p[1], p[2])) return 0u;
    if constexpr (HASHED && POW2) {
        // row = (x ^ y P1 ^ z P2) & mask with x <= resolution + 1 < 2^shift: x only reaches the bits BELOW the block index, so the two x
        // corners of a (y, z) combination share their block and the block follows from y and z alone -- 4 hashes instead of 8 rows, no x
        if (lv.resolution + 2u <= (1u << shift)) {
            const uint32_t y0 = (uint32_t)floorf(fmaf(p[1], lv.scale, 0.5f)), z0 = (uint32_t)floorf(fmaf(p[2], lv.scale, 0.5f));
            const uint32_t ya = y0 * kP1, yb = ya + kP1, za = z0 * kP2, zb = za + kP2;
            return (1u << (((ya ^ za) & lv.mask) >> shift)) | (1u << (((yb ^ za) & lv.mask) >> shift)) |
                   (1u << (((ya ^ zb) & lv.mask) >> shift)) | (1u << (((yb ^ zb) & lv.mask) >> shift));
        }
    }
    float fx, fy, fz;
    uint32_t rows[8], m = 0u;
    corner_rows<HASHED, POW2>(lv, p[0], p[1], p[2], fx, fy, fz, rows);
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) m |= 1u << (rows[k] >> shift);
    return m;
}

// geometry planes + block masks of every sample, once per backward call
template <bool TD = false, bool WARP = true>
__global__ __launch_bounds__(256, 1) void k_cast_cache_masks(UcnLevels lvls, RayInputs in, HexPattern hx, float std_scale,
                                                          uint32_t N, uint32_t S, MaskPlan plan,
                                                          const float *__restrict__ grad_features, GradStrides gs, uint32_t C,
                                                          float *__restrict__ geom, uint32_t *__restrict__ masks,
                                                          float *__restrict__ grad_level_major /*[L][N*S][C], / 6*/,
                                                          uint32_t *__restrict__ task_counter,
                                                          float *__restrict__ l1_partial /*[L][gridDim.x] or null: sum over the block's samples of max_c |g|*/) {
    const size_t B = (size_t)N * S;
    const size_t b = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (b < 8) task_counter[b] = 0u;                      // the compacted kernel's persistent workgroups pull tasks from here
    __shared__ float s_l1[UCN_MAX_LEVELS][4];             // per level: the four waves' sums of max_c |g| (fixed-point bound)
    if ((threadIdx.x & 63u) < UCN_MAX_LEVELS) s_l1[threadIdx.x & 63u][threadIdx.x >> 6] = 0.0f;   // own column (a wave past the end leaves zeros)
    // whole waves only (the bit planes below are built by wave ballots); a wave past the end skips the body but still reaches the
    // barrier of the l1_partial reduction at the bottom (an early `return` left the barrier to part of the workgroup)
    const bool live_wave = (b & ~(size_t)63) < B;
    do {
    if (!live_wave) break;
    const bool valid = b < B;
    const size_t bb = valid ? b : B - 1;                  // lanes past the end recompute the last sample and store nothing
    const uint32_t ray = (uint32_t)(bb / S), s = (uint32_t)(bb - (size_t)ray * S);
    float u[6][3], rs[6], csum[3], tsum;
    cast_sample<TD, WARP>(in, hx, std_scale, ray, s, S, u, rs, csum, tsum);
    if (valid) {
#pragma unroll
        for (uint32_t j = 0; j < 6; j++) {
            reinterpret_cast<float4 *>(geom)[b * 6 + j] = make_float4(u[j][0], u[j][1], u[j][2], rs[j]);
        }
    }
    __shared__ uint32_t s_words[kMaxMaskWords * 256u];    // [word][thread]: a thread's own column, bank = thread
    for (uint32_t lvl = 0; lvl < lvls.L; lvl++) {
        const UcnLevel lv = lvls.lv[lvl];
        const uint32_t nb_l = (lv.rows + (1u << plan.shift) - 1u) >> plan.shift;
        bool nz = false;
        float gmax = 0.0f;
        for (uint32_t c = 0; c < C; c++) {
            const float g = grad_features[lvl * gs.level + bb * gs.sample + c * gs.chan];
            nz |= valid && g != 0.0f;
            gmax = fmaxf(gmax, valid ? fabsf(g) : 0.0f);
            if (valid && !(fabsf(g) <= 3.0e38f)) gmax = __builtin_inff();        // NaN / inf poisons the bound (fmaxf drops NaN)
            // the row-block workgroups fetch gradients per ITEM (scattered): give them 8 contiguous bytes per sample,
            // already divided by the 6 multisamples of the mean (an IEEE division is ~13 VALU instructions per channel;
            // an item stage would repeat it ~27 times per sample and level)
            if (valid && grad_level_major) grad_level_major[((size_t)lvl * B + b) * C + c] = g / 6.0f;
        }
        if (!grad_level_major) gmax *= 6.0f;                // layout 4: g arrived divided by 6 -- the bound is on the undivided gradient (6 addends of <= |g| / 6 x w)
        if (l1_partial) {                                   // (workgroup-uniform; every wave of the block gets here: no early `continue` above)
            const float wsum = wave_sum_dpp<float>(gmax);
            if ((threadIdx.x & 63u) == 0u) s_l1[lvl][threadIdx.x >> 6] = wsum;
        }
        if (nb_l > 32u || plan.coarse[lvl] == 3) {
            // one bit per (sample, block) in nb / 32 words: set through the thread's own LDS column (dynamic word index)
            const uint32_t nw = (nb_l + 31u) / 32u;
            for (uint32_t k = 0; k < nw; k++) s_words[k * 256u + threadIdx.x] = 0u;
            if (nz) {
#pragma unroll
                for (uint32_t j = 0; j < 6; j++) {
                    if (!in_unit_cube(u[j][0], u[j][1], u[j][2])) continue;
                    float fx, fy, fz;
                    uint32_t rows[8];
                    if (lv.hashed) { if (lv.mask) corner_rows<true, true>(lv, u[j][0], u[j][1], u[j][2], fx, fy, fz, rows); else corner_rows<true, false>(lv, u[j][0], u[j][1], u[j][2], fx, fy, fz, rows); }
                    else { if (lv.mask) corner_rows<false, true>(lv, u[j][0], u[j][1], u[j][2], fx, fy, fz, rows); else corner_rows<false, false>(lv, u[j][0], u[j][1], u[j][2], fx, fy, fz, rows); }
#pragma unroll
                    for (uint32_t k = 0; k < 8; k++) {
                        const uint32_t blk = rows[k] >> plan.shift;
                        atomicOr(&s_words[(blk >> 5) * 256u + threadIdx.x], 1u << (blk & 31u));     // ds_or_b32, own column
                    }
                }
            }
            if (plan.coarse[lvl] == 3) {
                // wide_block's layout: BIT PLANES [block][ceil(B / 64)] x 64 bits, one bit per sample -- the scanning workgroup of
                // a block then reads B / 8 bytes instead of 4 B (measured in place with phase clocks: the word-per-sample scan
                // was HALF of such a workgroup's time, one exposed load latency per 4096 samples).  A wave = 64 consecutive
                // samples: 32 ballots per mask word, lane i keeps the ballot of block 32 w + i.
                const uint32_t lane = threadIdx.x & 63u;
                const size_t B64 = (B + 63u) / 64u, wave_global = b >> 6;
                uint32_t *T = masks + (size_t)plan.plane[lvl] * B;
                for (uint32_t w = 0; w < nw; w++) {
                    const uint32_t word = s_words[w * 256u + threadIdx.x];
                    uint32_t keep_lo = 0u, keep_hi = 0u;
#pragma unroll
                    for (uint32_t bit = 0; bit < 32u; bit++) {
                        const uint64_t bal = __ballot((word >> bit) & 1u);
                        if (lane == bit) { keep_lo = (uint32_t)bal; keep_hi = (uint32_t)(bal >> 32); }
                    }
                    const uint32_t blk = w * 32u + lane;
                    if (lane < 32u && blk < nb_l) {
                        T[((size_t)blk * B64 + wave_global) * 2u] = keep_lo;
                        T[((size_t)blk * B64 + wave_global) * 2u + 1u] = keep_hi;
                    }
                }
                continue;
            }
            if (valid) {
                uint32_t *mpw = masks + (size_t)plan.plane[lvl] * B + b;
                for (uint32_t k = 0; k < nw; k++) mpw[(size_t)k * B] = s_words[k * 256u + threadIdx.x];
            }
            continue;
        }
        uint32_t m[6];
#pragma unroll
        for (uint32_t j = 0; j < 6; j++) {
            if (lv.hashed) m[j] = lv.mask ? point_block_mask<true, true>(lv, plan.shift, u[j]) : point_block_mask<true, false>(lv, plan.shift, u[j]);
            else m[j] = lv.mask ? point_block_mask<false, true>(lv, plan.shift, u[j]) : point_block_mask<false, false>(lv, plan.shift, u[j]);
        }
        // a sample whose feature gradient on this level is exactly zero contributes nothing: clear its masks here
        // so that the scanning workgroups never have to look at the gradient
        if (!nz) {
#pragma unroll
            for (uint32_t j = 0; j < 6; j++) m[j] = 0u;
        }
        if (plan.fine_kind[lvl] == 3) {
            // BYTE PLANES (cmp_block_bytes): plane p = B bytes, byte b = the six point bits of sample b for row block p.  A thread
            // spreads its masks into words of four block bytes (nibble x 0x00204081 puts bit i of a nibble at bit 8 i), the four
            // threads of a quad (samples 4 q ... 4 q + 3; B % 4 == 0, so a quad is in range or not as a whole) transpose 4 x 4 bytes
            // through DPP quad broadcasts + v_perm_b32, and thread i of the quad stores the dword of block 4 k + i.
            const uint32_t qi = threadIdx.x & 3u;
            const uint32_t sel01 = qi | ((4u + qi) << 8) | 0x0c0c0000u, sel23 = 0x00000c0cu | (qi << 16) | ((4u + qi) << 24);
            uint8_t *pl = reinterpret_cast<uint8_t *>(masks + (size_t)plan.plane[lvl] * B);
            const uint32_t groups = (nb_l + 3u) / 4u;
            for (uint32_t k = 0; k < groups; k++) {
                uint32_t wk = 0u;
#pragma unroll
                for (uint32_t j = 0; j < 6; j++) wk |= ((((m[j] >> (4u * k)) & 15u) * 0x00204081u) & 0x01010101u) << j;
                const uint32_t w0 = dpp_or0<0x00, 0xf>(wk), w1 = dpp_or0<0x55, 0xf>(wk), w2 = dpp_or0<0xaa, 0xf>(wk), w3 = dpp_or0<0xff, 0xf>(wk);
                const uint32_t d = __builtin_amdgcn_perm(w1, w0, sel01) | __builtin_amdgcn_perm(w3, w2, sel23);
                const uint32_t blk = 4u * k + qi;
                if (valid && blk < nb_l) *reinterpret_cast<uint32_t *>(pl + (size_t)blk * B + (b & ~(size_t)3)) = d;
            }
            continue;
        }
        if (!valid) continue;
        uint32_t *mp = masks + (size_t)plan.plane[lvl] * B + b;
        if (plan.coarse[lvl]) {
            mp[0] = m[0] | m[1] | m[2] | m[3] | m[4] | m[5];
        } else {
            // word k = blocks 4k..4k+3, bit 4 * j + (block & 3) for multisample j: a workgroup reads ONE word per sample
            const uint32_t groups = (((lv.rows + (1u << plan.shift) - 1u) >> plan.shift) + 3u) / 4u;
            for (uint32_t k = 0; k < groups; k++) {
                uint32_t wk = 0u;
#pragma unroll
                for (uint32_t j = 0; j < 6; j++) wk |= ((m[j] >> (4u * k)) & 15u) << (4u * j);
                mp[(size_t)k * B] = wk;
            }
        }
    }
    } while (false);
    if (l1_partial) {
        __syncthreads();
        if (threadIdx.x < lvls.L)                           // fixed order: deterministic
            l1_partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] =
                ((s_l1[threadIdx.x][0] + s_l1[threadIdx.x][1]) + s_l1[threadIdx.x][2]) + s_l1[threadIdx.x][3];
    }
}

// Two rows of the block at once (the x0 / x0 + 1 corners of one (y, z) combination): both reads, then both compare-and-swaps
// -- two LDS round trips where two lds_row_add calls make four.  A lane whose row is outside the block skips its half.
template <uint32_t C, typename A>
__device__ __forceinline__ void lds_row_add_pair(A *acc_, uint32_t r0, bool in0, const float (&v0)[C], uint32_t r1, bool in1,
                                                 const float (&v1)[C]) {
    if constexpr (kFixed<A>) {
#pragma unroll
        for (uint32_t c = 0; c < C; c += 2) {
            if (in0) atomicAdd(reinterpret_cast<unsigned long long *>(acc_ + r0 * C + c), fixed_pack(v0[c], v0[c + 1]));
            if (in1) atomicAdd(reinterpret_cast<unsigned long long *>(acc_ + r1 * C + c), fixed_pack(v1[c], v1[c + 1]));
        }
        return;
    }
    float *acc = reinterpret_cast<float *>(acc_);
    if constexpr (C % 2u == 0u) {
#pragma unroll
        for (uint32_t c = 0; c < C; c += 2) {
            unsigned long long *p0 = reinterpret_cast<unsigned long long *>(acc + r0 * C + c);
            unsigned long long *p1 = reinterpret_cast<unsigned long long *>(acc + r1 * C + c);
            unsigned long long s0 = 0ull, s1 = 0ull;
            if (in0) s0 = *p0;
            if (in1) s1 = *p1;
            float2 t0 = __builtin_bit_cast(float2, s0), t1 = __builtin_bit_cast(float2, s1);
            t0.x += v0[c]; t0.y += v0[c + 1];
            t1.x += v1[c]; t1.y += v1[c + 1];
            bool lost0 = false, lost1 = false;
            if (in0) lost0 = atomicCAS(p0, s0, __builtin_bit_cast(unsigned long long, t0)) != s0;
            if (in1) lost1 = atomicCAS(p1, s1, __builtin_bit_cast(unsigned long long, t1)) != s1;   // (r1 == r0: loses, correctly)
            if (lost0) { atomicAdd(acc + r0 * C + c, v0[c]); atomicAdd(acc + r0 * C + c + 1, v0[c + 1]); }
            if (lost1) { atomicAdd(acc + r1 * C + c, v1[c]); atomicAdd(acc + r1 * C + c + 1, v1[c + 1]); }
        }
    } else {
        if (in0) lds_row_add<C, true>(acc, r0, v0);
        if (in1) lds_row_add<C, true>(acc, r1, v1);
    }
}

// ONE multisample point of a fine level into the workgroup's row block, by (y, z) COMBINATIONS (r03).  A hash scatters the four
// combinations of a point over four of the 32 row blocks, the x0 / x0 + 1 pair of a combination stays together: of the 8
// corners ~2 are this block's.  Walking all 8 with 22 % of the lanes active in each costs 8 x (hash, compare, weight, products,
// two LDS round trips) per wave; here a lane lists its in-block combinations first (4 row pairs, no weights) and the wave loops
// over "my next combination" -- as many rounds as the busiest lane has combinations (2-3), each with both corners' update in
// flight together.  Same addends ((w_k damp) g_c, w_k = ((wx wy) wz)) as point_scatter_block.
template <uint32_t C, bool HASHED, bool POW2, typename A>
__device__ __forceinline__ void point_scatter_combos(const UcnLevel &lv, A *__restrict__ acc, uint32_t row_lo, uint32_t nrows,
                                                     const float (&p)[3], float rsj, const float (&gout)[C]) {
    if (!in_unit_cube(p[0], p[1], p[2])) return;
    float fx = fmaf(p[0], lv.scale, 0.5f), fy = fmaf(p[1], lv.scale, 0.5f), fz = fmaf(p[2], lv.scale, 0.5f);
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
    auto row_of = [&](uint32_t xv, uint32_t yzv) -> uint32_t {
        uint32_t idx;
        if constexpr (HASHED) idx = xv ^ yzv; else idx = xv + yzv;
        if constexpr (POW2) return idx & lv.mask;
        else return idx < lv.rows ? idx : idx % lv.rows;
    };
    uint32_t pend = 0u;
    // hashed power-of-two levels whose row block is an aligned power of two above the resolution: x only reaches the bits below
    // the block index, both x corners of a combination lie in the block of (y P1 ^ z P2) -- one test per combination (wave-uniform switch)
    bool yz_decides = false;
    if constexpr (HASHED && POW2) yz_decides = (nrows & (nrows - 1u)) == 0u && (row_lo & (nrows - 1u)) == 0u && lv.resolution + 2u <= nrows;
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) {
        const uint32_t yv = (c & 1u) ? yb : ya, zv = (c & 2u) ? zb : za;
        uint32_t yz;
        if constexpr (HASHED) yz = yv ^ zv; else yz = yv + zv;
        bool hit;
        if (yz_decides) hit = (yz & lv.mask) - row_lo < nrows;
        else hit = (row_of(xa, yz) - row_lo < nrows) || (row_of(xb, yz) - row_lo < nrows);
        pend |= hit ? 1u << c : 0u;
    }
    const float damp = erf_pos(rsj * lv.inv_gs);
    const float gx = 1.0f - fx, gy = 1.0f - fy, gz = 1.0f - fz;
    while (pend) {
        const uint32_t c = (uint32_t)__builtin_ctz(pend);
        pend &= pend - 1u;
        const uint32_t yv = (c & 1u) ? yb : ya, zv = (c & 2u) ? zb : za;
        const float wy = (c & 1u) ? fy : gy, wz = (c & 2u) ? fz : gz;
        uint32_t yz;
        if constexpr (HASHED) yz = yv ^ zv; else yz = yv + zv;
        const uint32_t r0 = row_of(xa, yz) - row_lo, r1 = row_of(xb, yz) - row_lo;
        const float w0 = ((gx * wy) * wz) * damp, w1 = ((fx * wy) * wz) * damp;
        float v0[C], v1[C];
#pragma unroll
        for (uint32_t cc = 0; cc < C; cc++) { v0[cc] = w0 * gout[cc]; v1[cc] = w1 * gout[cc]; }
        lds_row_add_pair<C>(acc, r0, r0 < nrows, v0, r1, r1 < nrows, v1);
    }
}

// Direct (no run merging) scatter of ONE multisample point into the workgroup's row block.
template <uint32_t C, bool HASHED, bool POW2, typename A>
__device__ __forceinline__ void point_scatter_block(const UcnLevel &lv, A *__restrict__ acc, uint32_t row_lo, uint32_t nrows,
                                                    const float (&p)[3], float rsj, const float (&gout)[C]) {
    if (!in_unit_cube(p[0], p[1], p[2])) return;
    float fx, fy, fz, w[8];
    uint32_t rows[8];
    corner_rows<HASHED, POW2>(lv, p[0], p[1], p[2], fx, fy, fz, rows);
    corner_weights(fx, fy, fz, w);
    const float damp = erf_pos(rsj * lv.inv_gs);
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t r = rows[k] - row_lo;
        if (r < nrows) {
            float v[C];
#pragma unroll
            for (uint32_t c = 0; c < C; c++) v[c] = (w[k] * damp) * gout[c];
            lds_row_add<C, true>(acc, r, v);
        }
    }
}

template <uint32_t C, bool TD = false, bool WARP = true>
__global__ __launch_bounds__(1024) void k_march_features_bwd_blk(UcnLevels lvls, float *__restrict__ grad_table,
                                                                 RayInputs in, HexPattern hx, float std_scale, uint32_t N,
                                                                 uint32_t S, GradStrides gs, uint32_t rpb,
                                                                 const float *__restrict__ grad_features,
                                                                 const float *__restrict__ geom) {
    extern __shared__ float s_acc[];
    uint32_t task = blockIdx.x, lvl = 0, nb = 1, split = 1;
    for (;; lvl++) {
        nb = (lvls.lv[lvl].rows + rpb - 1) / rpb;
        split = bwd_sample_split(nb);
        if (task < nb * split || lvl + 1 == lvls.L) break;
        task -= nb * split;
    }
    const UcnLevel lv = lvls.lv[lvl];
    const uint32_t row_lo = (task / split) * rpb, part = task % split;
    const uint32_t nrows = lv.rows - row_lo < rpb ? lv.rows - row_lo : rpb;
    for (uint32_t i = threadIdx.x; i < nrows * C; i += 1024u) s_acc[i] = 0.0f;
    __syncthreads();
    const size_t B = (size_t)N * S;
    // a level with few blocks (the dense coarse ones) is cut along the samples too: `split` workgroups per
    // block, interleaved in units of 1024 samples; they share the block, so their flush is atomic
    for (size_t b = (size_t)part * 1024u + threadIdx.x; b < B; b += (size_t)split * 1024u) {
        const float *gp = grad_features + lvl * gs.level + b * gs.sample;
        float gout[C];
        bool nz = false;
#pragma unroll
        for (uint32_t c = 0; c < C; c++) {
            gout[c] = gp[c * gs.chan] / 6.0f;                           // d(mean over the 6 multisamples)
            nz |= gout[c] != 0.0f;
        }
        if (!nz) continue;
        float u[6][3], rs[6];
        if (geom) {                                   // k_cast_cache's planes: every task re-reads, nobody re-derives
#pragma unroll
            for (uint32_t j = 0; j < 6; j++) {
                const float4 q = reinterpret_cast<const float4 *>(geom)[b * 6 + j];
                u[j][0] = q.x; u[j][1] = q.y; u[j][2] = q.z; rs[j] = q.w;
            }
        } else {
            const uint32_t ray = (uint32_t)(b / S), s = (uint32_t)(b - (size_t)ray * S);
            float csum[3], tsum;
            cast_sample<TD, WARP>(in, hx, std_scale, ray, s, S, u, rs, csum, tsum);
        }
        if (lv.hashed) {
            if (lv.mask && lv.resolution <= 2048u) level_scatter_block<C, true, true, true>(lv, s_acc, row_lo, nrows, u, rs, gout);
            else if (lv.mask) level_scatter_block<C, true, true, false>(lv, s_acc, row_lo, nrows, u, rs, gout);
            else level_scatter_block<C, true, false, false>(lv, s_acc, row_lo, nrows, u, rs, gout);
        } else if (lv.resolution <= 2048u) {
            if (lv.mask) level_scatter_block<C, false, true, true>(lv, s_acc, row_lo, nrows, u, rs, gout);
            else level_scatter_block<C, false, false, true>(lv, s_acc, row_lo, nrows, u, rs, gout);
        } else {                                   // the strided fine levels of the uint32-wrap quirk: nothing to merge
            if (lv.mask) level_scatter_block<C, false, true, false>(lv, s_acc, row_lo, nrows, u, rs, gout);
            else level_scatter_block<C, false, false, false>(lv, s_acc, row_lo, nrows, u, rs, gout);
        }
    }
    __syncthreads();
    float *gtab = grad_table + ((size_t)lv.first_row + row_lo) * C;
    for (uint32_t i = threadIdx.x; i < nrows * C; i += 1024u) {
        const float v = s_acc[i];
        if (v != 0.0f) {
            if (split == 1) gtab[i] += v;
            else atomicAdd(gtab + i, v);
        }
    }
}

// The same row-block ownership with COMPACTION.  A cell touches at most 8 of a level's 32 row blocks, a single
// multisample point of a fine level 7 on average: in the plain kernel 78 % of the hash/weight work of a
// workgroup is for corners that are not its own, and a per-lane "skip" does not help a 64-wide wave.  Here every
// wave reads the block masks of 64 samples at a time, appends the items that DO touch the block -- samples on
// coarse levels, (sample, multisample) pairs on fine ones -- to a ring in LDS (ballot + prefix count), and runs
// the expensive part on 64 dense items whenever the ring holds that many.
//
// Code shape matters as much as the algorithm here: the scan/process loop is ONE function template per addressing
// variant with ONE process site, everything force-inlined.  (With lambdas called from several unrolled sites the
// compiler outlined the scatter into a real function: the level descriptor then lived behind a flat pointer --
// a global load + vmcnt(0) in front of every point -- and the LDS base came from the dynamic-LDS offset table,
// an s_load per corner; that version spent 80 % of its time waiting on those.)
constexpr uint32_t kQueue = 512;                               // items per wave; 16 waves x 2 KiB beside the 128 KiB block

template <uint32_t C, bool HASHED, bool POW2, bool COARSE>
__device__ __forceinline__ void cmp_fetch(uint32_t item, bool valid, size_t B, const float *__restrict__ gl,
                                          const float *__restrict__ geom, float (&u)[6][3], float (&rs)[6], float (&gout)[C], float gscale) {
    const uint32_t b = valid ? item & 0x1FFFFFFFu : 0u, j = valid ? item >> 29 : 0u;
#pragma unroll
    for (uint32_t c = 0; c < C; c++) gout[c] = gl[(size_t)b * C + c] * gscale;             // d(mean over the 6 multisamples): / 6 done by k_cast_cache_masks; x the task's power-of-two fixed-point scale (1 for float rows)
    if constexpr (COARSE) {
#pragma unroll
        for (uint32_t jj = 0; jj < 6; jj++) {
            const float4 q = reinterpret_cast<const float4 *>(geom)[(size_t)b * 6 + jj];
            u[jj][0] = q.x; u[jj][1] = q.y; u[jj][2] = q.z; rs[jj] = q.w;
        }
    } else {
        const float4 q = reinterpret_cast<const float4 *>(geom)[(size_t)b * 6 + j];
        u[0][0] = q.x; u[0][1] = q.y; u[0][2] = q.z; rs[0] = q.w;
    }
}

template <uint32_t C, bool HASHED, bool POW2, bool COARSE, bool RUNS, bool COMBOS = false, typename A = float>
__device__ __forceinline__ void cmp_block(const UcnLevel &lv, A *__restrict__ s_acc, uint32_t *__restrict__ q, uint32_t blk,
                                          uint32_t row_lo, uint32_t nrows, uint32_t part, uint32_t split, size_t B,
                                          const uint32_t *__restrict__ mp, const float *__restrict__ gl,
                                          const float *__restrict__ geom, float gscale = 1.0f) {
    // one mask word per sample: coarse levels bit `blk`; fine levels the word of this block's group of four,
    // bit 4 * j + (blk & 3) for multisample j (k_cast_cache_masks)
    constexpr uint32_t P = COARSE ? 1u : 6u;                                  // items a sample can contribute
    const uint32_t bit0 = COARSE ? (blk & 31u) : (blk & 3u);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t head = 0, tail = 0;                                              // wave-uniform ring positions
    const size_t stride = (size_t)split * kScan * 1024u;
    size_t base = (size_t)part * kScan * 1024u;
    uint32_t cur[kScan], nxt[kScan];
#pragma unroll
    for (uint32_t u = 0; u < kScan; u++) {
        const size_t b = base + u * 1024u + threadIdx.x;
        cur[u] = b < B ? mp[b] : 0u;
    }
    // `split` workgroups share a block; they take the samples in interleaved units of kScan x 1024 (flush: atomic).
    // One workgroup per CU: the masks of the NEXT unit are requested before this unit's items are processed.
    uint32_t u = 0;
    bool more = base < B;
    while (more || tail != head) {
        if (more) {
            if (u == 0) {
                const size_t nb = base + stride;
#pragma unroll
                for (uint32_t uu = 0; uu < kScan; uu++) {
                    const size_t b = nb + uu * 1024u + threadIdx.x;
                    nxt[uu] = b < B ? mp[b] : 0u;
                }
            }
            const uint32_t b = (uint32_t)(base + u * 1024u + threadIdx.x);
            uint32_t m = cur[0];                                              // u is wave-uniform: selects, no scratch
#pragma unroll
            for (uint32_t uu = 1; uu < kScan; uu++) m = u == uu ? cur[uu] : m;
            m >>= bit0;
            if constexpr (!COMBOS) {
#pragma unroll
                for (uint32_t j = 0; j < P; j++) {
                    const bool act = (m >> (4u * j)) & 1u;
                    const uint64_t bal = __ballot(act);
                    const uint32_t pos = tail + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                    if (act) q[pos & (kQueue - 1u)] = b | (j << 29);
                    tail += (uint32_t)__popcll(bal);
                }
            } else {
                // a sample hits this block with 0.84 of its 6 points on average: count per lane, one DPP prefix sum per step,
                // then every lane writes its own items (as many rounds as the busiest lane has hits, ~3) -- six ballot /
                // mbcnt / predicated-write sections per step were a third of a fine level's time (scan alone: 166 of 490 us)
                m &= 0x111111u;
                const uint32_t cnt = (uint32_t)__popc(m);
                const uint32_t incl = wave_scan_dpp<uint32_t>(cnt);
                uint32_t pos = tail + incl - cnt;
                tail += wave_last<uint32_t>(incl);
                while (m) {
                    const uint32_t bit = (uint32_t)__builtin_ctz(m);
                    m &= m - 1u;
                    q[pos & (kQueue - 1u)] = b | (bit << 27);                    // bit = 4 j: j lands in bits 29..31
                    pos++;
                }
            }
            if (++u == kScan) {
                u = 0;
                base += stride;
                more = base < B;
#pragma unroll
                for (uint32_t uu = 0; uu < kScan; uu++) cur[uu] = nxt[uu];
            }
        }
        __builtin_amdgcn_wave_barrier();
        // Ring: <= kPer * 64 - 1 left over + <= 384 (fine) / 64 (coarse) appended per step <= kQueue.
        constexpr uint32_t kPer = RUNS ? 6u : 2u;                              // ring items per lane and round
        const uint32_t thr = more ? kPer * 64u : 1u;
        while (tail - head >= thr && tail != head) {
            const uint32_t avail = tail - head < kPer * 64u ? tail - head : kPer * 64u;
            if constexpr (RUNS) {
                // the coarsest levels (every sample of the ring is a neighbour of the previous one):
                // a lane walks kPer CONSECUTIVE ring items (neighbouring samples of a ray) and keeps merging runs
                // across them; the next item's geometry is requested before the current one is scattered
                RowRun<C> run;
                run.have = false;
                float un[6][3], rsn[6], gn[C], glast[C];               // glast: the gradient of the sample the open run belongs to (C <= 2: unused by the flush)
#pragma unroll
                for (uint32_t c = 0; c < C; c++) glast[c] = 0.0f;
                cmp_fetch<C, HASHED, POW2, true>(q[(head + kPer * lane) & (kQueue - 1u)], kPer * lane < avail, B, gl, geom, un, rsn, gn, gscale);
#pragma unroll 1
                for (uint32_t k = 0; k < kPer; k++) {
                    float uc[6][3], rsc[6], gc[C];
#pragma unroll
                    for (uint32_t j = 0; j < 6; j++) {
#pragma unroll
                        for (uint32_t d = 0; d < 3; d++) uc[j][d] = un[j][d];
                        rsc[j] = rsn[j];
                    }
#pragma unroll
                    for (uint32_t c = 0; c < C; c++) gc[c] = gn[c];
                    const uint32_t idx = kPer * lane + k;
                    if (k + 1 < kPer)
                        cmp_fetch<C, HASHED, POW2, true>(q[(head + idx + 1u) & (kQueue - 1u)], idx + 1u < avail, B, gl, geom, un, rsn, gn, gscale);
                    if (idx < avail) run_merge_sample<C, HASHED, POW2>(lv, s_acc, row_lo, nrows, uc, rsc, gc, run);
                }
                if (run.have) run_flush<C>(s_acc, row_lo, nrows, run, glast);   // (lean runs are closed by run_merge_sample: never open here)
            } else {
                // two items per lane: both items' loads are in flight before the first scatter starts
                const uint32_t i0 = q[(head + lane) & (kQueue - 1u)], i1 = q[(head + 64u + lane) & (kQueue - 1u)];
                const bool v0 = lane < avail, v1 = lane + 64u < avail;
                float u0[6][3], rs0[6], g0[C], u1[6][3], rs1[6], g1[C];
                cmp_fetch<C, HASHED, POW2, COARSE>(i0, v0, B, gl, geom, u0, rs0, g0, gscale);
                cmp_fetch<C, HASHED, POW2, COARSE>(i1, v1, B, gl, geom, u1, rs1, g1, gscale);
                if (v0) {
                    if constexpr (COARSE) level_scatter_block<C, HASHED, POW2, true>(lv, s_acc, row_lo, nrows, u0, rs0, g0);
                    else if constexpr (COMBOS) point_scatter_combos<C, HASHED, POW2>(lv, s_acc, row_lo, nrows, u0[0], rs0[0], g0);
                    else point_scatter_block<C, HASHED, POW2>(lv, s_acc, row_lo, nrows, u0[0], rs0[0], g0);
                }
                if (v1) {
                    if constexpr (COARSE) level_scatter_block<C, HASHED, POW2, true>(lv, s_acc, row_lo, nrows, u1, rs1, g1);
                    else if constexpr (COMBOS) point_scatter_combos<C, HASHED, POW2>(lv, s_acc, row_lo, nrows, u1[0], rs1[0], g1);
                    else point_scatter_block<C, HASHED, POW2>(lv, s_acc, row_lo, nrows, u1[0], rs1[0], g1);
                }
            }
            head += avail;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Point-item levels on BYTE PLANES (MaskPlan::fine_kind 3; r06, VERDICT r05 item 2 b).  `mb` = this row block's plane: one byte per
// sample, bit j = multisample j has a corner in the block (k_cast_cache_masks).  A lane reads ONE dword = four consecutive samples
// per unit of 4096 (cmp_block: four dwords, one sample each, 6 useful bits of 32), counts its hits, the wave takes one DPP prefix
// sum and every lane appends its own items; (y, z)-combination scatter as in shape 2.  A lane can hold up to 24 hits: when the
// wave's count would not fit the ring, only every lane's lowest non-empty byte (<= 6 hits, <= 384 per wave: the bound cmp_block
// lives with) is taken in this round and the rest of the word stays for the next one.
template <uint32_t C, bool HASHED, bool POW2, typename A>
__device__ __forceinline__ void cmp_block_bytes(const UcnLevel &lv, A *__restrict__ s_acc, uint32_t *__restrict__ q, uint32_t row_lo,
                                                uint32_t nrows, uint32_t part, uint32_t split, size_t B,
                                                const uint8_t *__restrict__ mb, const float *__restrict__ gl,
                                                const float *__restrict__ geom, float gscale) {
    static_assert(kScan == 4u, "a unit is 1024 dwords of four sample bytes");
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t head = 0, tail = 0;
    const size_t stride = (size_t)split * 4096u;
    size_t base = (size_t)part * 4096u;
    bool more = base < B, fresh = true;
    uint32_t cur = 0u, nxt = 0u;
    {
        const size_t b = base + 4u * threadIdx.x;
        if (b < B) cur = *reinterpret_cast<const uint32_t *>(mb + b) & 0x3f3f3f3fu;
    }
    while (more || tail != head) {
        if (more) {
            if (fresh) {                                                      // the next unit's word: in flight under this unit's items
                const size_t b = base + stride + 4u * threadIdx.x;
                nxt = b < B ? *reinterpret_cast<const uint32_t *>(mb + b) & 0x3f3f3f3fu : 0u;
                fresh = false;
            }
            uint32_t take = cur;
            uint32_t cnt = (uint32_t)__popc(take);
            uint32_t incl = wave_scan_dpp<uint32_t>(cnt);
            uint32_t tot = wave_last<uint32_t>(incl);
            if (tail - head + tot > kQueue) {                                 // (wave-uniform, rare: 64 x 3.4 hits expected)
                take = cur ? cur & (0xffu << ((uint32_t)__builtin_ctz(cur) & 24u)) : 0u;
                cnt = (uint32_t)__popc(take);
                incl = wave_scan_dpp<uint32_t>(cnt);
                tot = wave_last<uint32_t>(incl);
            }
            uint32_t pos = tail + incl - cnt;
            tail += tot;
            cur &= ~take;
            const uint32_t b4 = (uint32_t)base + 4u * threadIdx.x;
            while (take) {
                const uint32_t bit = (uint32_t)__builtin_ctz(take);
                take &= take - 1u;
                q[pos & (kQueue - 1u)] = (b4 + (bit >> 3)) | (bit << 29);       // j = bit & 7 < 6: bits 29..31 (the sample's bits fall off the top)
                pos++;
            }
            if (__ballot(cur != 0u) == 0ull) {
                base += stride;
                more = base < B;
                cur = nxt;
                fresh = true;
            }
        }
        __builtin_amdgcn_wave_barrier();
        // Ring: <= 127 left over + a fitting round (checked above) or <= 384 appended <= kQueue.
        const uint32_t thr = more ? 128u : 1u;
        while (tail - head >= thr && tail != head) {
            const uint32_t avail = tail - head < 128u ? tail - head : 128u;
            const uint32_t i0 = q[(head + lane) & (kQueue - 1u)], i1 = q[(head + 64u + lane) & (kQueue - 1u)];
            const bool v0 = lane < avail, v1 = lane + 64u < avail;
            float u0[6][3], rs0[6], g0[C], u1[6][3], rs1[6], g1[C];
            cmp_fetch<C, HASHED, POW2, false>(i0, v0, B, gl, geom, u0, rs0, g0, gscale);
            cmp_fetch<C, HASHED, POW2, false>(i1, v1, B, gl, geom, u1, rs1, g1, gscale);
            if (v0) {
                point_scatter_combos<C, HASHED, POW2>(lv, s_acc, row_lo, nrows, u0[0], rs0[0], g0);
            }
            if (v1) {
                point_scatter_combos<C, HASHED, POW2>(lv, s_acc, row_lo, nrows, u1[0], rs1[0], g1);
            }
            head += avail;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Levels of MORE THAN 32 ROW BLOCKS (the reference's own waymo.gin grid: T = 2^21 rows of C = 4 = 256 blocks of 8192 rows).
// The masks are one bit per (sample, block); a hit sample has a corner pair in this block with only ~1 of its 6 points
// (a point's four (y, z) pairs lie in ~4.5 of the 256 blocks), so walking all 48 corners of every hit sample keeps 17 % of the
// lanes busy in the expensive part (measured: 500 us per workgroup of 262 144 samples, 75 of them the scan).  Two rings per wave
// instead: ring 1 takes the hit SAMPLES from the scan; stage 1 runs 64 of them, point by point -- geometry, cell, the four
// pair rows, which of them are mine -- and appends (sample, pair, point set) items to ring 2 (popcount + one DPP prefix sum);
// stage 2 runs dense batches of ring 2: per point of the set one hash, two weights, one erf; one paired compare-and-swap update per item.
// Same addends as everywhere ((w_k damp) g_c, w_k = ((wx wy) wz)).
constexpr uint32_t kRing1 = 128, kRing2 = kQueue - kRing1;                    // 128 + 384 words of a wave's 2 KiB

template <uint32_t C, bool HASHED, bool POW2>
__device__ __forceinline__ void wide_pair_rows(const UcnLevel &lv, const float4 &g, float &fx, float &fy, float &fz,
                                               uint32_t &xa, uint32_t &xb, uint32_t (&yz)[4]) {
    fx = fmaf(g.x, lv.scale, 0.5f); fy = fmaf(g.y, lv.scale, 0.5f); fz = fmaf(g.z, lv.scale, 0.5f);
    const uint32_t x0 = (uint32_t)floorf(fx), y0 = (uint32_t)floorf(fy), z0 = (uint32_t)floorf(fz);
    fx -= (float)x0; fy -= (float)y0; fz -= (float)z0;
    uint32_t ya, yb, za, zb;
    if constexpr (HASHED) {
        xa = x0; xb = x0 + 1u;
        ya = y0 * kP1; yb = ya + kP1;
        za = z0 * kP2; zb = za + kP2;
        yz[0] = ya ^ za; yz[1] = yb ^ za; yz[2] = ya ^ zb; yz[3] = yb ^ zb;
    } else {
        xa = x0 * lv.stride[0]; xb = xa + lv.stride[0];
        ya = y0 * lv.stride[1]; yb = ya + lv.stride[1];
        za = z0 * lv.stride[2]; zb = za + lv.stride[2];
        yz[0] = ya + za; yz[1] = yb + za; yz[2] = ya + zb; yz[3] = yb + zb;
    }
}
template <bool HASHED, bool POW2>
__device__ __forceinline__ uint32_t wide_row(const UcnLevel &lv, uint32_t xv, uint32_t yzv) {
    uint32_t idx;
    if constexpr (HASHED) idx = xv ^ yzv; else idx = xv + yzv;
    if constexpr (POW2) return idx & lv.mask;
    else return idx < lv.rows ? idx : idx % lv.rows;
}

// stage 2 of wide_block: dense (sample | pair << 24 | point set << 26) items of ring 2: the points of the set share ONE lattice cell,
// so the pair's two rows are theirs in common -- their addends are summed in registers and go to the block in one paired update
// (on the coarser levels all six points of a sample share the cell: six times fewer LDS updates, and none of the same-row
// collisions that consecutive points of a sample would cause).  (A function, force-inlined at its two call sites: a lambda
// called from several sites gets outlined by hipcc -- see cmp_block.)
template <uint32_t C, bool HASHED, bool POW2, typename A>
__device__ __forceinline__ void wide_drain(const UcnLevel &lv, A *__restrict__ s_acc, const uint32_t *__restrict__ q2, uint32_t &head2,
                                           uint32_t tail2, uint32_t thr, uint32_t lane, uint32_t row_lo, uint32_t nrows,
                                           const float *__restrict__ gl, const float *__restrict__ geom, float gscale) {
    while (tail2 - head2 >= thr && tail2 != head2) {
        const uint32_t avail = tail2 - head2 < 64u ? tail2 - head2 : 64u;
        const bool v = lane < avail;
        const uint32_t it = v ? q2[(head2 + lane) % kRing2] : 0u;
        const uint32_t b = it & 0xFFFFFFu, c = (it >> 24) & 3u;
        uint32_t pts = it >> 26;
        float gout[C], v0[C], v1[C];
#pragma unroll
        for (uint32_t cc = 0; cc < C; cc++) { gout[cc] = gl[(size_t)b * C + cc] * gscale; v0[cc] = 0.0f; v1[cc] = 0.0f; }
        uint32_t r0 = 0u, r1 = 0u;
        while (pts) {
            const uint32_t j = (uint32_t)__builtin_ctz(pts);
            pts &= pts - 1u;
            const float4 g = reinterpret_cast<const float4 *>(geom)[(size_t)b * 6 + j];
            float fx, fy, fz;
            uint32_t xa, xb, yz[4];
            wide_pair_rows<C, HASHED, POW2>(lv, g, fx, fy, fz, xa, xb, yz);
            const uint32_t h = c == 0u ? yz[0] : c == 1u ? yz[1] : c == 2u ? yz[2] : yz[3];
            const float wy = (c & 1u) ? fy : 1.0f - fy, wz = (c & 2u) ? fz : 1.0f - fz;
            r0 = wide_row<HASHED, POW2>(lv, xa, h) - row_lo; r1 = wide_row<HASHED, POW2>(lv, xb, h) - row_lo;   // (the same for every point of the set)
            const float damp = erf_pos(g.w * lv.inv_gs);
            const float w0 = (((1.0f - fx) * wy) * wz) * damp, w1 = ((fx * wy) * wz) * damp;
#pragma unroll
            for (uint32_t cc = 0; cc < C; cc++) { v0[cc] += w0 * gout[cc]; v1[cc] += w1 * gout[cc]; }
        }
        if (v) lds_row_add_pair<C>(s_acc, r0, r0 < nrows, v0, r1, r1 < nrows, v1);
        head2 += avail;
    }
}

template <uint32_t K>
__device__ __forceinline__ void wide_load_group(const uint32_t *__restrict__ T, size_t first, size_t wstride, size_t B64,
                                                uint32_t (&lo)[K], uint32_t (&hi)[K]) {
#pragma unroll
    for (uint32_t i = 0; i < K; i++) {
        const size_t w = first + i * wstride;
        lo[i] = w < B64 ? T[w * 2u] : 0u;
        hi[i] = w < B64 ? T[w * 2u + 1u] : 0u;
    }
}

template <uint32_t C, bool HASHED, bool POW2, typename A>
__device__ __forceinline__ void wide_block(const UcnLevel &lv, A *__restrict__ s_acc, uint32_t *__restrict__ q, uint32_t blk,
                                           uint32_t row_lo, uint32_t nrows, uint32_t part, uint32_t split, size_t B,
                                           const uint32_t *__restrict__ mp, const float *__restrict__ gl,
                                           const float *__restrict__ geom, float gscale) {
    uint32_t *q1 = q, *q2 = q + kRing1;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t head1 = 0, tail1 = 0, head2 = 0, tail2 = 0;                      // wave-uniform ring positions
    // the block's bit plane (k_cast_cache_masks): bit i of 64-bit word w = sample 64 w + i.  A lane takes the words
    // part + split (1024 k + thread), k = 0, 1, ...: kWords of them are loaded together, the next group is requested before this
    // one is searched.  One round = every lane with bits left hands over its lowest one (<= 64 samples into ring 1).
    constexpr uint32_t kWords = 4;
    const size_t B64 = (B + 63u) / 64u;
    const uint32_t *T = mp + (size_t)blk * B64 * 2u;
    const size_t wstride = (size_t)split * 1024u, w0 = (size_t)part + (size_t)split * threadIdx.x;
    uint32_t clo[kWords], chi[kWords], nlo[kWords], nhi[kWords];
    size_t gfirst = w0;                                                        // this lane's first word of the current group
    wide_load_group<kWords>(T, gfirst, wstride, B64, clo, chi);
    bool more = (size_t)part + (size_t)split * (threadIdx.x & ~63u) < B64;     // wave-uniform: the wave's first word exists
    uint32_t wi = 0;                                                           // word of the group being searched
    uint32_t lo = 0u, hi = 0u;
    bool fresh = true;                                                         // take the next word of the group
    while (more || tail1 != head1) {
        if (more) {
            if (fresh) {
                if (wi == 0) wide_load_group<kWords>(T, gfirst + kWords * wstride, wstride, B64, nlo, nhi);
                lo = clo[0]; hi = chi[0];
#pragma unroll
                for (uint32_t i = 1; i < kWords; i++) { lo = wi == i ? clo[i] : lo; hi = wi == i ? chi[i] : hi; }
                fresh = false;
            }
            const bool act = (lo | hi) != 0u;
            uint32_t bit = lo ? (uint32_t)__builtin_ctz(lo) : 32u + (uint32_t)__builtin_ctz(hi | 0x80000000u * (hi == 0u));
            const size_t w = gfirst + wi * wstride;
            const uint32_t b = (uint32_t)(w * 64u + bit);
            if (lo) lo &= lo - 1u; else hi &= hi - 1u;
            const uint64_t bal = __ballot(act);
            const uint32_t pos = tail1 + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            if (act) q1[pos % kRing1] = b;
            tail1 += (uint32_t)__popcll(bal);
            if (__ballot((lo | hi) != 0u) == 0ull) {                           // every lane is through with its word
                fresh = true;
                if (++wi == kWords) {
                    wi = 0;
                    gfirst += kWords * wstride;
#pragma unroll
                    for (uint32_t i = 0; i < kWords; i++) { clo[i] = nlo[i]; chi[i] = nhi[i]; }
                    // the first lane's first word of the new group decides for the wave (its words come first)
                    more = (size_t)part + (size_t)split * (threadIdx.x & ~63u) + (gfirst - w0) < B64;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        // stage 1: <= 63 samples left over + <= 64 appended per round <= kRing1
        const uint32_t thr1 = more ? 64u : 1u;
        while (tail1 - head1 >= thr1 && tail1 != head1) {
            const uint32_t avail = tail1 - head1 < 64u ? tail1 - head1 : 64u;
            const bool v = lane < avail;
            const uint32_t b = v ? q1[(head1 + lane) % kRing1] : 0u;
            // the next point's geometry is requested before this one is tested (a round is otherwise one exposed load latency).
            // Consecutive points in one lattice cell form a RUN: its in-block pairs become items only when the cell changes
            // (or after the sixth point: round 6 flushes), carrying the set of its points.
            float4 gn = reinterpret_cast<const float4 *>(geom)[(size_t)b * 6];
            uint32_t run_x = 0u, run_y = 0u, run_z = 0u, run_pend = 0u, run_pts = 0u;
#pragma unroll 1
            for (uint32_t j = 0; j < 7; j++) {
                const float4 g = gn;
                if (j + 1u < 6u) gn = reinterpret_cast<const float4 *>(geom)[(size_t)b * 6 + j + 1u];
                uint32_t flush = j == 6u ? run_pend : 0u;
                if (j < 6u && v && in_unit_cube(g.x, g.y, g.z)) {
                    float fx, fy, fz;
                    uint32_t xa, xb, yz[4];
                    wide_pair_rows<C, HASHED, POW2>(lv, g, fx, fy, fz, xa, xb, yz);
                    const uint32_t cx = (uint32_t)floorf(fmaf(g.x, lv.scale, 0.5f)), cy = (uint32_t)floorf(fmaf(g.y, lv.scale, 0.5f)),
                                   cz = (uint32_t)floorf(fmaf(g.z, lv.scale, 0.5f));
                    if (run_pts != 0u && cx == run_x && cy == run_y && cz == run_z) {
                        run_pts |= 1u << j;
                    } else {
                        flush = run_pend;                                       // (0 for the first point)
                        uint32_t pend = 0u;
#pragma unroll
                        for (uint32_t c = 0; c < 4; c++) {
                            const bool hit = (wide_row<HASHED, POW2>(lv, xa, yz[c]) - row_lo < nrows) || (wide_row<HASHED, POW2>(lv, xb, yz[c]) - row_lo < nrows);
                            pend |= hit ? 1u << c : 0u;
                        }
                        // the items of the run that ends here carry ITS point set: emit below, then start the new run
                        const uint32_t old_pts = run_pts;
                        run_x = cx; run_y = cy; run_z = cz; run_pend = pend;
                        run_pts = (1u << j) | (old_pts << 8);                   // bits 8..13: the ended run's points, until the emit
                    }
                }
                const uint32_t emit_pts = j == 6u ? run_pts & 63u : run_pts >> 8;
                run_pts &= 63u;
                const uint32_t cnt = (uint32_t)__popc(flush);
                const uint32_t incl = wave_scan_dpp<uint32_t>(cnt);
                uint32_t pos = tail2 + incl - cnt;
                tail2 += wave_last<uint32_t>(incl);
                while (flush) {
                    const uint32_t c = (uint32_t)__builtin_ctz(flush);
                    flush &= flush - 1u;
                    q2[pos % kRing2] = b | (c << 24) | (emit_pts << 26);
                    pos++;
                }
                __builtin_amdgcn_wave_barrier();
                // ring 2: <= 63 left over + <= 256 appended per round <= kRing2
                wide_drain<C, HASHED, POW2>(lv, s_acc, q2, head2, tail2, 64u, lane, row_lo, nrows, gl, geom, gscale);
            }
            head1 += avail;
        }
        __builtin_amdgcn_wave_barrier();
    }
    wide_drain<C, HASHED, POW2>(lv, s_acc, q2, head2, tail2, 1u, lane, row_lo, nrows, gl, geom, gscale);
}

// PERSISTENT workgroups (r03): one per CU, tasks (level, row block, sample part) pulled from a counter in the plan's
// longest-first order.  With one workgroup per task the hardware dispatcher hands workgroup k to XCD k mod 8 IN ORDER: where
// task times differ (45 ... 1010 us inside the uneven levels) a full XCD blocks the dispatch for all eight -- the workgroup
// clocks of the benchmark grid showed 164-208 of 256 CUs busy behind the uneven levels and a 1.3 ms drain at the end
// (4.26 ms where the workgroup times sum to 3.70 ms per CU).
template <uint32_t C, bool FX = false>
__global__ __launch_bounds__(1024) void k_march_features_bwd_cmp(UcnLevels lvls, float *__restrict__ grad_table, uint32_t N,
                                                                 uint32_t S, uint32_t rpb, MaskPlan plan,
                                                                 const float *__restrict__ grad_features /*[L][N*S][C]*/,
                                                                 const float *__restrict__ geom,
                                                                 const uint32_t *__restrict__ masks,
                                                                 uint32_t *__restrict__ counter, uint32_t total,
                                                                 const float *__restrict__ l1_partial /*FX: [L][ceil(B / 256)]*/) {
    extern __shared__ float s_acc[];                      // 128 KiB row block + 16 rings of 2 KiB: all of the CU's 160 KiB
    using Acc = typename std::conditional<FX, FxLane, float>::type;
    Acc *acc_rows = reinterpret_cast<Acc *>(s_acc);       // FX: the same bytes as int32 fixed-point channel pairs (0.0f == 0)
    for (uint32_t i = threadIdx.x; i < rpb * C; i += 1024u) s_acc[i] = 0.0f;          // a flush leaves zeros behind
    uint32_t *q = reinterpret_cast<uint32_t *>(s_acc + (size_t)rpb * C) + (threadIdx.x >> 6) * kQueue;
    volatile uint32_t *s_task = reinterpret_cast<uint32_t *>(s_acc + (size_t)rpb * C);   // = wave 0's ring, idle between tasks
    const size_t B = (size_t)N * S;
    // Eight queues, one per XCD: queue y holds the tasks k = y (mod 8), i.e. exactly the workgroups the in-order dispatcher
    // would have placed on XCD y.  That keeps what the static launch had for free: the `split` parts of all row blocks of a
    // level that scan the SAME samples (same mask words, geometry, gradients) run on the same XCD and share its L2 -- with one
    // global queue the point-item levels' workgroups took 650 us instead of 480.  An XCD whose queue is dry steals.
    const uint32_t home = __builtin_amdgcn_s_getreg(20 /*HW_REG_XCC_ID*/ | (3u << 11)) & 7u;
    for (;;) {
        if (threadIdx.x == 0) {
            uint32_t t = total;
            for (uint32_t a = 0; a < 8u; a++) {
                const uint32_t y = (home + a) & 7u;
                const uint32_t k = atomicAdd(counter + y, 1u) * 8u + y;
                if (k < total) { t = k; break; }
            }
            *s_task = t;
        }
        __syncthreads();                                                              // (also: zeros / flush of s_acc are done)
        const uint32_t task0 = __builtin_amdgcn_readfirstlane(*s_task);               // wave-uniform: everything derived stays scalar
        __syncthreads();                                                              // before wave 0 refills its ring
        if (task0 >= total) break;
        uint32_t task = task0, lvl = 0, nb = 1, split = 1;
        for (uint32_t i = 0;; i++) {
            lvl = plan.order[i];
            nb = (lvls.lv[lvl].rows + rpb - 1) / rpb;
            split = plan.split[lvl];
            if (task < nb * split || i + 1 == lvls.L) break;                        // (`total` is the sum of nb * split)
            task -= nb * split;
        }
        const UcnLevel lv = lvls.lv[lvl];
        const uint32_t blk = task / split, part = task % split;
        const uint32_t row_lo = blk * rpb;
        const uint32_t nrows = lv.rows - row_lo < rpb ? lv.rows - row_lo : rpb;
        const uint32_t *mp = masks + (size_t)(plan.plane[lvl] + (plan.coarse[lvl] ? blk >> 5 : blk >> 2)) * B;
        const float *gl = grad_features + (size_t)lvl * B * C;
        float gscale = 1.0f, ginv = 1.0f;
        if constexpr (FX) {
            // the task's bound: L1 = sum over ITS samples of max_c |g| (256-sample partials of the mask pass; the sample-item
            // and point-item shapes take the units of kScan x 1024 samples with unit % split == part, the wide shape interleaves
            // 64-sample words and is given the whole level's sum), then the power of two that puts L1 at <= 2^30
            const uint32_t nblk = (uint32_t)((B + 255u) / 256u);
            const float *lp = l1_partial + (size_t)lvl * nblk;
            const bool every = plan.coarse[lvl] == 3 || split == 1u;
            float mine = 0.0f;
            for (uint32_t i = threadIdx.x; i < nblk; i += 1024u)
                if (every || (i / (kScan * 4u)) % split == part) mine += lp[i];
            mine = wave_sum_dpp<float>(mine);
            volatile float *s_red = reinterpret_cast<volatile float *>(s_acc + (size_t)rpb * C) + 16;      // wave 0's ring, idle here
            if ((threadIdx.x & 63u) == 0u) s_red[threadIdx.x >> 6] = mine;
            __syncthreads();
            float l1 = 0.0f;
#pragma unroll
            for (uint32_t w = 0; w < 16u; w++) l1 += s_red[w];                     // fixed order, every thread the same value
            __syncthreads();                                                       // before the rings are used again
            l1 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, l1)));
            // (a level whose resolution^2 wrapped negative in int32 has a NaN damping factor, models.py:495: NaN rows in the reference and on
            // the float route -- a NaN addend would pack as 0 here, so the task is poisoned like one with a non-finite gradient)
            const bool nan_level = lv.inv_gs != lv.inv_gs;
            if (!nan_level && l1 > 0.0f && l1 <= 3.0e38f) {
                int x;
                (void)frexpf(l1, &x);                                              // l1 = m 2^x, m in [0.5, 1): l1 <= 2^x
                int e = 30 - x;
                e = e > 120 ? 120 : (e < -100 ? -100 : e);                          // x <= 128 (l1 <= 3e38): e >= -98, never clamped from below
                gscale = ldexpf(1.0f, e);
                ginv = ldexpf(1.0f, -e);
            } else if (nan_level || !(l1 <= 3.0e38f)) {
                ginv = __builtin_nanf("");                                         // a non-finite gradient on this level: every row of the task's block becomes NaN (flush below)
            }
        }
#define UCN_CMP(H, P2, CO, RU) cmp_block<C, H, P2, CO, RU>(lv, acc_rows, q, blk, row_lo, nrows, part, split, B, mp, gl, geom, gscale)
#define UCN_CMPF(H, P2)                                                                                                      \
    do {                                                                                                                     \
        if (plan.fine_kind[lvl] == 3) cmp_block_bytes<C, H, P2>(lv, acc_rows, q, row_lo, nrows, part, split, B, reinterpret_cast<const uint8_t *>(masks + (size_t)plan.plane[lvl] * B) + (size_t)blk * B, gl, geom, gscale); \
        else if (plan.fine_kind[lvl] == 2) cmp_block<C, H, P2, false, false, true>(lv, acc_rows, q, blk, row_lo, nrows, part, split, B, mp, gl, geom, gscale);    \
        else cmp_block<C, H, P2, false, false, false>(lv, acc_rows, q, blk, row_lo, nrows, part, split, B, mp, gl, geom, gscale);         \
    } while (0)
        if (plan.coarse[lvl] == 2) {                                          // all workgroup-uniform; the coarsest
            if (lv.mask) UCN_CMP(false, true, true, true);                    // levels are never hashed
            else UCN_CMP(false, false, true, true);
        } else if (plan.coarse[lvl] == 3) {                                   // > 32 row blocks: sample items, unmerged scatter
#define UCN_CMPW(H, P2) wide_block<C, H, P2>(lv, acc_rows, q, blk, row_lo, nrows, part, split, B, masks + (size_t)plan.plane[lvl] * B, gl, geom, gscale)
            if (lv.hashed) { if (lv.mask) UCN_CMPW(true, true); else UCN_CMPW(true, false); }
            else { if (lv.mask) UCN_CMPW(false, true); else UCN_CMPW(false, false); }
#undef UCN_CMPW
        } else if (plan.coarse[lvl]) {
            if (lv.hashed) { if (lv.mask) UCN_CMP(true, true, true, false); else UCN_CMP(true, false, true, false); }
            else { if (lv.mask) UCN_CMP(false, true, true, false); else UCN_CMP(false, false, true, false); }
        } else {
            if (lv.hashed) { if (lv.mask) UCN_CMPF(true, true); else UCN_CMPF(true, false); }
            else { if (lv.mask) UCN_CMPF(false, true); else UCN_CMPF(false, false); }
        }
#undef UCN_CMP
#undef UCN_CMPF
        __syncthreads();
        float *gtab = grad_table + ((size_t)lv.first_row + row_lo) * C;
        if constexpr (FX) {
            unsigned long long *words = reinterpret_cast<unsigned long long *>(s_acc);
            for (uint32_t i = threadIdx.x; i < nrows * C / 2u; i += 1024u) {
                const unsigned long long w = words[i];
                if (w != 0ull || ginv != ginv) {                 // poisoned task: a NaN addend packs as 0, so untouched-looking rows are flushed too
                    words[i] = 0ull;
                    float a, b;
                    fixed_unpack(w, ginv, a, b);
                    if (split == 1) { gtab[2u * i] += a; gtab[2u * i + 1u] += b; }
                    else { atomicAdd(gtab + 2u * i, a); atomicAdd(gtab + 2u * i + 1u, b); }
                }
            }
        } else {
        for (uint32_t i = threadIdx.x; i < nrows * C; i += 1024u) {
            const float v = s_acc[i];
            if (v != 0.0f) {
                s_acc[i] = 0.0f;
                if (split == 1) gtab[i] += v;
                else atomicAdd(gtab + i, v);
            }
        }
        }
    }
}

}  // namespace

// The one route decision of the table gradient: true (and `plan` filled in) where ucn_march_features_backward(levels_per_block = 0)
// takes the compacted row-block kernel, given a workspace.  Item words hold the sample in 29 bits (cmp_block), wide_block's in 24.
static bool bwd_row_block_plan(const UcnLevels &lv, size_t B, bool fixed, MaskPlan *plan) {
    const uint32_t rpb = 128u * 1024u / (lv.C * 4u);
    if (B >= (1ull << 29) || !make_mask_plan(lv, rpb, B, plan, fixed)) return false;
    if (B >= (1ull << 24))
        for (uint32_t l = 0; l < lv.L; l++)
            if (plan->coarse[l] == 3) return false;
    return true;
}

// CUs of the current device (the persistent backward launches one workgroup per CU)
static uint32_t device_cu_count() {
    static thread_local int cached_dev = -1;
    static thread_local uint32_t cached = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256u;
    if (dev != cached_dev) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached = (uint32_t)n;
        cached_dev = dev;
    }
    return cached;
}

// Workspace of ucn_march_features_backward: the geometry planes (24 B floats; the fallbacks use these alone), and where the call takes
// the compacted row-block kernel the block-mask planes (room for the float-row and the fixed-point plan, whichever has more), a
// level-major copy of the gradient, the task counter and the 256-sample L1 partials of the fixed-point mode.
extern "C" uint64_t ucn_march_features_backward_ws_floats(const ucn_field_t *f, uint32_t N, uint32_t S) {
    UcnLevels lv;
    if (field_levels(f, &lv)) return 0;
    const size_t B = (size_t)N * S;
    MaskPlan plan, plan_fx;
    const bool masks = bwd_row_block_plan(lv, B, false, &plan);
    if (masks && bwd_row_block_plan(lv, B, true, &plan_fx) && plan_fx.n_planes > plan.n_planes) plan.n_planes = plan_fx.n_planes;
    uint64_t n = (24ull + (masks ? plan.n_planes + lv.L * lv.C : 0u)) * B + 64u;             // + the task counter
    n += (((uint64_t)lv.L * ucn_div_up(B, 256) + 63u) & ~63ull);                                 // + the 256-sample L1 partials of the fixed-point mode
    return n;
}

// 1 if ucn_march_features_backward(levels_per_block = 0, with a workspace) takes the compacted row-block kernel for this field and call
// size under float AND under fixed-point rows -- the route that reads a layout-4 gradient (bwd_row_block_plan, as in the launcher)
extern "C" int ucn_march_features_backward_row_blocks(const ucn_field_t *f, uint32_t N, uint32_t S) {
    UcnLevels lv;
    if (field_levels(f, &lv)) return 0;
    const size_t B = (size_t)N * S;
    MaskPlan plan;
    return (B > 0 && bwd_row_block_plan(lv, B, false, &plan) && bwd_row_block_plan(lv, B, true, &plan)) ? 1 : 0;
}

template <bool TD, bool WARP>
static int march_features_backward_launch(const ucn_field_t *f, const RayInputs &in, float std_scale, uint32_t N, uint32_t S,
                                          uint32_t levels_per_block, int layout, const float *grad_features,
                                          float *grad_embeddings, float *workspace, ucn_stream_t stream) {
    UCN_REQUIRE(in.sdist && (TD || (in.near_ && in.far_)) && in.origins && in.dirs && in.basis && in.radii && grad_features &&
                grad_embeddings, "march_features_backward: null pointer argument");
    UCN_REQUIRE((in.flip == nullptr) == (in.spin == nullptr), "march_features_backward: flip and spin come together");
    const bool want_fixed = (layout & UCN_BWD_FIXED_POINT) != 0;
    layout &= ~UCN_BWD_FIXED_POINT;
    const bool prediv = layout == 4;                     // level-major and already / 6: read in place
    if (prediv) layout = 0;
    UCN_REQUIRE(layout == 0 || layout == 1 || layout == 3, "march_features_backward: layout must be 0, 1, 3 or 4");
    UcnLevels lv;
    if (int rc = field_levels(f, &lv)) return rc;
    if (N == 0) return 0;
    const size_t B = (size_t)N * S;
    UCN_REQUIRE(B <= 0xFFFFFF00ull, "march_features_backward: too many samples in one call (%zu)", B);
    // fixed-point row blocks pack channel PAIRS and bound a row's rounding slack by 24 B (48 B addends x 1/2) on top of the 2^30
    // target: C = 1 and calls with 2^30 + 24 B >= 2^31 keep float rows
    const bool fixed = want_fixed && lv.C % 2u == 0u && B <= (1ull << 22);
    static_assert((1ull << 30) + 24ull * (1ull << 22) < (1ull << 31), "fixed-point row blocks: int32 headroom");
    const HexPattern hx = make_hex();
    const GradStrides gs = grad_strides(layout, B, lv.L, lv.C);
    hipStream_t st = (hipStream_t)stream;
    if (levels_per_block == 0) {
        // row-block ownership (no global atomics) while the recomputation stays cheap: every block walks
        // all samples, so the cost grows with the number of blocks; above 64 blocks per level the atomic
        // scatter below wins again
        const uint32_t rpb = 128u * 1024u / (lv.C * 4u);
        uint32_t tasks = 0, blocks = 0;
        for (uint32_t l = 0; l < lv.L; l++) {
            const uint32_t nb = ucn_div_up(lv.lv[l].rows, rpb);
            blocks += nb;
            tasks += nb * bwd_sample_split(nb);
        }
        MaskPlan plan;
        if (workspace && bwd_row_block_plan(lv, B, fixed, &plan)) {
            tasks = 0;
            for (uint32_t l = 0; l < lv.L; l++) {
                const uint32_t nb = ucn_div_up(lv.lv[l].rows, rpb);
                tasks += nb * plan.split[l];
            }
            // compacting variant: block masks next to the geometry planes, dense items from a per-wave ring in LDS
            uint32_t *masks = reinterpret_cast<uint32_t *>(workspace + 24ull * B);
            float *glm = workspace + (24ull + plan.n_planes) * B;                               // level-major copy, / 6
            uint32_t *task_counter = reinterpret_cast<uint32_t *>(workspace + (24ull + plan.n_planes + (size_t)lv.L * lv.C) * B);
            float *l1_partial = reinterpret_cast<float *>(task_counter + 64);                   // [L][ceil(B / 256)] (fixed-point mode)
            hipLaunchKernelGGL((k_cast_cache_masks<TD, WARP>), dim3(ucn_div_up(B, 256)), dim3(256), 0, st, lv, in, hx, std_scale, N, S, plan,
                               grad_features, gs, lv.C, workspace, masks, prediv ? nullptr : glm, task_counter, fixed ? l1_partial : nullptr);
            const float *glv = prediv ? grad_features : glm;                                    // [L][B][C], / 6
            const uint32_t cus = device_cu_count();
            ucn_for_level_dim(lv.C, [&](auto cc) {
                constexpr uint32_t CC = decltype(cc)::value;
                const dim3 grid(tasks < cus ? tasks : cus);
                const size_t lds = (size_t)rpb * CC * 4 + 16 * kQueue * 4;
                if (!tasks) return;
                if constexpr (CC % 2 == 0) {                   // fixed-point rows pack channel pairs (`fixed` implies an even C)
                    if (fixed) {
                        hipLaunchKernelGGL((k_march_features_bwd_cmp<CC, true>), grid, dim3(1024), lds, st, lv, grad_embeddings, N, S, rpb,
                                           plan, glv, workspace, masks, task_counter, tasks, l1_partial);
                        return;
                    }
                }
                hipLaunchKernelGGL((k_march_features_bwd_cmp<CC, false>), grid, dim3(1024), lds, st, lv, grad_embeddings, N, S, rpb, plan,
                                   glv, workspace, masks, task_counter, tasks, nullptr);
            });
            UCN_LAUNCH_CHECK("march_features_backward (row blocks, compacted)");
            return 0;
        }
        UCN_REQUIRE(!prediv, "march_features_backward: layout 4 (pre-divided level-major gradient) is the compacted row-block kernel's input; this call would take a fallback");
        if (blocks <= 64u * lv.L) {
            if (workspace)
                hipLaunchKernelGGL((k_cast_cache<TD, WARP>), dim3(ucn_div_up(B, 256)), dim3(256), 0, st, in, hx, std_scale, N, S, workspace);
            ucn_for_level_dim(lv.C, [&](auto cc) {
                constexpr uint32_t CC = decltype(cc)::value;
                hipLaunchKernelGGL((k_march_features_bwd_blk<CC, TD, WARP>), dim3(tasks), dim3(1024), (size_t)rpb * CC * 4, st, lv,
                                   grad_embeddings, in, hx, std_scale, N, S, gs, rpb, grad_features, workspace);
            });
            UCN_LAUNCH_CHECK("march_features_backward (row blocks)");
            return 0;
        }
        levels_per_block = 1;
    }
    UCN_REQUIRE(layout != 3, "march_features_backward: layout 3 is a row-block layout (levels_per_block = 0, <= 64 blocks per level)");
    UCN_REQUIRE(!prediv, "march_features_backward: layout 4 is a row-block layout (levels_per_block = 0 with a workspace)");
    const dim3 grid(ucn_div_up(B, 256), ucn_div_up(lv.L, levels_per_block));
    ucn_for_level_dim(lv.C, [&](auto cc) {
        hipLaunchKernelGGL((k_march_features_bwd<decltype(cc)::value, TD, WARP>), grid, dim3(256), 0, st, lv, grad_embeddings, in, hx,
                           std_scale, N, S, levels_per_block, layout, grad_features);
    });
    UCN_LAUNCH_CHECK("march_features_backward");
    return 0;
}

extern "C" int ucn_march_features_backward_warp(const ucn_field_t *f, const float *fenceposts, const float *near_,
                                                const float *far_, const float *origins, const float *directions,
                                                const float *basis, const float *radii, const float *flip, const float *spin,
                                                float std_scale, int warp, uint32_t N, uint32_t S, uint32_t levels_per_block,
                                                int layout, const float *grad_features, float *grad_embeddings, float *workspace,
                                                ucn_stream_t stream) {
    UCN_REQUIRE(warp == 0 || warp == 1, "march_features_backward: warp must be 0 (MLP.warp_fn = None) or 1 ('contract'), got %d", warp);
    UCN_REQUIRE((near_ == nullptr) == (far_ == nullptr),
                "march_features_backward: near and far come together (both NULL: metric fenceposts)");
    const RayInputs in{fenceposts, near_, far_, origins, directions, basis, radii, flip, spin};
    int rc = 0;
    ucn_for_bool(near_ == nullptr, [&](auto td) {
        ucn_for_bool(warp != 0, [&](auto w) {
            rc = march_features_backward_launch<decltype(td)::value, decltype(w)::value>(f, in, std_scale, N, S, levels_per_block, layout,
                                                                                         grad_features, grad_embeddings, workspace, stream);
        });
    });
    return rc;
}

extern "C" int ucn_march_features_backward(const ucn_field_t *f, const float *sdist, const float *near_, const float *far_,
                                           const float *origins, const float *directions, const float *basis,
                                           const float *radii, const float *flip, const float *spin, float std_scale,
                                           uint32_t N, uint32_t S, uint32_t levels_per_block, int layout,
                                           const float *grad_features, float *grad_embeddings, float *workspace,
                                           ucn_stream_t stream) {
    UCN_REQUIRE(near_ && far_, "march_features_backward: null pointer argument");
    return ucn_march_features_backward_warp(f, sdist, near_, far_, origins, directions, basis, radii, flip, spin, std_scale, 1, N, S,
                                            levels_per_block, layout, grad_features, grad_embeddings, workspace, stream);
}

extern "C" int ucn_march_features_backward_tdist(const ucn_field_t *f, const float *tdist, const float *origins,
                                                 const float *directions, const float *basis, const float *radii,
                                                 const float *flip, const float *spin, float std_scale, uint32_t N, uint32_t S,
                                                 uint32_t levels_per_block, int layout, const float *grad_features,
                                                 float *grad_embeddings, float *workspace, ucn_stream_t stream) {
    return ucn_march_features_backward_warp(f, tdist, nullptr, nullptr, origins, directions, basis, radii, flip, spin, std_scale, 1, N,
                                            S, levels_per_block, layout, grad_features, grad_embeddings, workspace, stream);
}
