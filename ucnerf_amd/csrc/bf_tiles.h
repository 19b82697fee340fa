// bf16 MFMA tile helpers shared by the training kernels (field_train.hip) and the mixed-precision sky layer (sky.hip):
// a wave owns 32 samples (the N of v_mfma_f32_32x32x16_bf16); activations live in registers as B operands (two k-steps of
// 8 bf16 per 32-wide tile), weights arrive as 1 KiB A-fragments through the LDS-DMA ring of mlp_ring.h.
#pragma once
#include <utility>

#include "mlp_ring.h"
#include "wave_dpp.h"

namespace {

typedef __bf16 bf8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x16 mfma_bf(bf8 a, bf8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }

// fp32 -> bf16, round to nearest even: the C cast is v_cvt_pk_bf16_f32 on gfx950 (two values per instruction)
// (written as two-element vector conversions: element by element -- these files are built without the SLP vectoriser --
// the compiler emitted one conversion per VALUE plus a v_perm_b32 per pair, twice the instructions)
__device__ __forceinline__ bf8 pack8(const float (&v)[8]) {
    typedef float f2v __attribute__((ext_vector_type(2)));
    typedef __bf16 bf2v __attribute__((ext_vector_type(2)));
    bf8 o;
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        const f2v t = {v[e], v[e + 1]};
        const bf2v r = __builtin_convertvector(t, bf2v);
        o[e] = r[0];
        o[e + 1] = r[1];
    }
    return o;
}
// 8 accumulator registers (k-step s of a tile) -> the B operand of the next layer
__device__ __forceinline__ bf8 to_b(const f32x16 &a, int s, bool relu) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = a[8 * s + e];
    const bf8 o = pack8(v);
    if (!relu) return o;
    // ReLU on the packed result: a negative bf16 is a negative int16 (v_pk_max_i16, two values per instruction; -0 -> +0)
    typedef short s8v __attribute__((ext_vector_type(8)));
    const s8v z = {0, 0, 0, 0, 0, 0, 0, 0};
    return __builtin_bit_cast(bf8, __builtin_elementwise_max(__builtin_bit_cast(s8v, o), z));
}
__device__ __forceinline__ void zero_acc(f32x16 &a) {
#pragma unroll
    for (int r = 0; r < 16; r++) a[r] = 0.0f;
}
__device__ __forceinline__ void load_acc(const float *__restrict__ p, f32x16 &acc) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float4 v = reinterpret_cast<const float4 *>(p)[q];
        acc[4 * q + 0] = v.x; acc[4 * q + 1] = v.y; acc[4 * q + 2] = v.z; acc[4 * q + 3] = v.w;
    }
}

constexpr int kTChunk = 16;                          // fragments (KiB) per chunk of the training kernels' rings

template <int... Is, class F>
__device__ __forceinline__ void sfor_impl(std::integer_sequence<int, Is...>, F &&f) { (f(std::integral_constant<int, Is>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void sfor(F &&f) { sfor_impl(std::make_integer_sequence<int, N>{}, f); }

// P output tiles (a PAIR, or one) from NT_IN input tiles: acc[o2] += A(frag) . in[it][s], fragments [it][s][o2] from
// stream position G0.  The two tiles of a pair alternate (two MFMAs into the same accumulator do not issue back to
// back); only the pair's 32 accumulator registers are live, the caller converts / stores it before the next pair.
template <int P, int NT_IN, int G0, class RING>
__device__ __forceinline__ void tile_pair(RING &ring, f32x16 (&acc)[P], const bf8 (&in)[NT_IN][2]) {
    sfor<NT_IN * 2 * P>([&](auto i) {
        constexpr int I = i.value, G = G0 + I;
        constexpr int o2 = I % P, s = (I / P) % 2, it = I / (2 * P);
        constexpr int CH = RING::kChunk, NW = RING::kWaves;     // a wave issues one DMA piece per NW fragments
        if constexpr (G % CH == 0 && G / CH >= 1) ring.template boundary<G / CH>();
        if constexpr (G % NW == 0) ring.template piece<G / CH + RING::kLeadChunks, (G % CH) / NW>();
        acc[o2] = mfma_bf(__builtin_bit_cast(bf8, ring.template group<G>()), in[it][s], acc[o2]);
        // one operand read per MFMA: left alone, the scheduler hoists a chunk's sixteen reads (64 registers) to its start
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    });
}
constexpr int kWAhead = 3, kWSlots = kWAhead + 1;   // weight fragments requested ahead of their MFMAs; register slots of the pipe
// request fragment GF: the ring's housekeeping rides on the requests (as pipe_fetch of mlp_ring.h)
template <int GF, int NG, class RING>
__device__ __forceinline__ void frag_fetch(RING &ring, bf8 (&wp)[kWSlots]) {
    if constexpr (GF < NG) {
        constexpr int CH = RING::kChunk, NW = RING::kWaves;
        if constexpr (GF % CH == 0 && GF / CH >= 1) ring.template boundary<GF / CH>();
        if constexpr (GF % NW == 0) ring.template piece<GF / CH + RING::kLeadChunks, (GF % CH) / NW>();
        wp[GF % kWSlots] = __builtin_bit_cast(bf8, ring.template group<GF>());
    }
}
// tile_pair with the fragment pipe: the plain form above issues "one operand read, one MFMA" and the register allocator gives every
// read the SAME four registers -- read, wait for it, MFMA: with one wave per SIMD the LDS latency stands in front of every MFMA (a pair's
// 32 MFMAs took ~1900 cycles instead of 1024).  Here fragment G + kWAhead is requested in front of the MFMA of G (program order pinned
// by a scheduling barrier per step), the pipe lives across pairs and layers.
template <int P, int NT_IN, int G0, int NG, class RING>
__device__ __forceinline__ void tile_pair_pf(RING &ring, bf8 (&wp)[kWSlots], f32x16 (&acc)[P], const bf8 (&in)[NT_IN][2]) {
    sfor<NT_IN * 2 * P>([&](auto i) {
        constexpr int I = i.value, G = G0 + I;
        constexpr int o2 = I % P, s = (I / P) % 2, it = I / (2 * P);
        frag_fetch<G + kWAhead, NG>(ring, wp);
        acc[o2] = mfma_bf(wp[G % kWSlots], in[it][s], acc[o2]);
        __builtin_amdgcn_sched_barrier(0);
    });
}
// bit r = accumulator register r is positive (the ReLU mask of the lane's 16 features of a tile).  One v_alignbit_b32 per
// register shifts its SIGN bit into the word ((m << 1) | sign), registers taken from 15 down to 0, then one inversion: 17 VALU
// instructions per tile where compare + select + or took 48 (the training kernels' masks were 2700 of the sky forward's 5600
// VALU instructions per wave).  A pre-activation of exactly +0 counts as positive: relu'(0) = 1 here, a valid subgradient
// where torch picks 0.  MFMA accumulation from a +0 / bias start cannot produce -0; a bias that cancels a dot product exactly
// is rare but real with bf16 operands and few terms (F = 1: feat w = -bias, tests/test_heads_layerwise_cpu.py) -- the stored
// activation is 0 there and the bit is set, which the layer-wise tests allow only inside the fp32 error band around 0.
__device__ __forceinline__ uint32_t mask16(const f32x16 &a) {
    uint32_t m = 0;
#pragma unroll
    for (int r = 15; r >= 0; r--) m = __builtin_amdgcn_alignbit(m, __float_as_uint(a[r]), 31);
    return ~m & 0xFFFFu;
}
// the masked (ReLU') half tile as a B operand: v_bfe_i32 spreads the register's mask bit over a word, one v_and_b32 applies it
__device__ __forceinline__ bf8 to_b_masked(const f32x16 &a, int s, uint32_t bits) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e++)
        v[e] = __uint_as_float(__float_as_uint(a[8 * s + e]) & (uint32_t)__builtin_amdgcn_sbfe((int)bits, 8 * s + e, 1));
    return pack8(v);
}
// store a tile of activations: lane (j, h) holds features 32t + (r&3) + 8(r>>2) + 4h of sample j -- four 8-byte pieces
// {0-3, 8-11, 16-19, 24-27} + 4h.  The two lanes of a sample first trade pieces (v_permlane32_swap: lane j's pieces 2, 3
// against lane j + 32's pieces 0, 1), after which lane (j, 0) holds features 0-15 and lane (j, 1) features 16-31 of the
// tile contiguously: two 16-byte stores per lane instead of four 8-byte ones -- the kernels' 1.8 GB of activations leave
// in half as many write transactions.  (Transposing whole rows through LDS: 1.13 -> 1.06 ms, not worth 66 KiB of LDS.)
__device__ __forceinline__ void store_tile(uint16_t *__restrict__ dst, uint32_t width, uint32_t sample, int t, int h, const bf8 (&b)[2],
                                           bool live) {
    const uint4 lo = __builtin_bit_cast(uint4, b[0]), hi = __builtin_bit_cast(uint4, b[1]);
    // (a, b) -> a keeps lanes 0-31 and takes b's lanes 0-31 into its lanes 32-63; b takes a's lanes 32-63 into its lanes 0-31
    const auto s0 = __builtin_amdgcn_permlane32_swap(lo.x, hi.x, false, false);
    const auto s1 = __builtin_amdgcn_permlane32_swap(lo.y, hi.y, false, false);
    const auto s2 = __builtin_amdgcn_permlane32_swap(lo.z, hi.z, false, false);
    const auto s3 = __builtin_amdgcn_permlane32_swap(lo.w, hi.w, false, false);
    if (!live) return;
    uint4 *p = reinterpret_cast<uint4 *>(dst + (size_t)sample * width + 32 * t + 16 * h);
    p[0] = make_uint4(s0[0], s1[0], s0[1], s1[1]);      // h = 0: features 0-3 (own), 4-7 (partner);  h = 1: 16-19, 20-23
    p[1] = make_uint4(s2[0], s3[0], s2[1], s3[1]);      // h = 0: features 8-11, 12-15;                h = 1: 24-27, 28-31
}
// A PAIR of tiles (64 adjacent features = 128 bytes of the row) through the wave's own LDS tile (kernels that run ONE workgroup per CU have
// the room): stored per lane, a pair is 4 store instructions of 64 separate 16-byte requests each (a lane = a row), 256 texture-address cycles per pair and wave --
// with four waves per CU as long as the pair's 32 MFMAs take, i.e. the training kernels were bound by the address unit, not by bytes
// (without the stores the sky forward kernel runs 1.29 ms instead of 1.89).  Here a lane writes its eight 8-byte pieces to row j of a
// [32][128 B + 16] tile (no lane swaps), the wave reads the tile back row-contiguous and stores 8 rows x one whole 128-byte line per
// instruction: 8 requests instead of 64.  `sample0` = the wave's first sample, `n_rows` = how many of its 32 rows exist.
constexpr int kStageRow = 144;                                       // bytes
constexpr int kStageTile = 32 * kStageRow;                           // 4.5 KiB per wave
__device__ __forceinline__ void store_pair_staged(uint8_t *__restrict__ tile, uint16_t *__restrict__ dst, uint32_t width, uint32_t sample0,
                                                  uint32_t n_rows, int tp, int lane, const bf8 (&t0)[2], const bf8 (&t1)[2]) {
    const int j = lane & 31, h = lane >> 5;
    wave_lds_handoff();                                               // the previous pair's reads are done
    // ds_write_b64 is served 16 consecutive lanes at a time on 32 banks; with a 36-dword row stride rows j and j + 8 start on the same
    // bank (2-way conflicts on every write: 5.0e7 conflict cycles per launch, SQ_LDS_BANK_CONFLICT, where the kernels had none before
    // the staging).  Rows with bit 3 set keep the two 8-byte halves of each 16-byte unit swapped; the read below (row >> 3 == i) undoes
    // it for free by naming the dwords in the other order.
    uint8_t *row = tile + j * kStageRow + 8 * (h ^ ((j >> 3) & 1));
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const uint4 lo = __builtin_bit_cast(uint4, t == 0 ? t0[0] : t1[0]), hi = __builtin_bit_cast(uint4, t == 0 ? t0[1] : t1[1]);
        // bf8 [0] = features {0-3, 8-11} + 4h, [1] = {16-19, 24-27} + 4h of the tile: 8-byte pieces at byte 2 x feature
        *reinterpret_cast<uint2 *>(row + 64 * t + 0) = make_uint2(lo.x, lo.y);
        *reinterpret_cast<uint2 *>(row + 64 * t + 16) = make_uint2(lo.z, lo.w);
        *reinterpret_cast<uint2 *>(row + 64 * t + 32) = make_uint2(hi.x, hi.y);
        *reinterpret_cast<uint2 *>(row + 64 * t + 48) = make_uint2(hi.z, hi.w);
    }
    wave_lds_handoff();
    // a full tile (wave-uniform; all but a launch's last tiles) stores without per-row predicates: each predicate is an exec save, a
    // branch and a restore around ONE store -- 700 of the sky forward kernel's 10 k instructions per wave, at one wave per SIMD
    const bool full = __builtin_amdgcn_readfirstlane(n_rows) == 32u;
    const uint32_t r0 = (uint32_t)lane >> 3, c = (uint32_t)lane & 7u;
    const uint8_t *src = tile + r0 * kStageRow + 16u * c;
    uint16_t *out = dst + (size_t)(sample0 + r0) * width + 32 * tp + 8u * c;
    const size_t step = (size_t)8 * width;                            // 8 rows further per instruction
    if (full) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint4 u = *reinterpret_cast<const uint4 *>(src + i * 8 * kStageRow);
            *reinterpret_cast<uint4 *>(out + i * step) = (i & 1) ? make_uint4(u.z, u.w, u.x, u.y) : u;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint4 u = *reinterpret_cast<const uint4 *>(src + i * 8 * kStageRow);
            if (8u * i + r0 < n_rows) *reinterpret_cast<uint4 *>(out + i * step) = (i & 1) ? make_uint4(u.z, u.w, u.x, u.y) : u;
        }
    }
}
template <class RING>
__device__ __forceinline__ void ring_start(RING &ring) {
    rstatic_for<RING::kLeadChunks>([&](auto c) { ring.template issue_chunk<c.value>(); });
}

}  // namespace
