// Colour correction of an evaluation frame on the device.
//
// ref: internal/image.py:71-111 color_correct, three channels.  Per iteration the reference builds the [n, 10] quadratic design
// matrix of the current image, masks its rows per channel and calls lstsq three times.  A pixel's row is never needed in memory here,
// only its contribution to the 10 x 10 Gram matrix A^T A and to A^T b of each channel, so an iteration is one streaming pass over the
// pixels and one small solve:
//   row(p)   = [r r, r g, r b, g g, g b, b b, r, g, b, 1] of the current image's pixel p = (r, g, b)
//   mask_c   = unclipped(img0[c]) & unclipped(cur[c]) & unclipped(ref[c]),   unclipped(z) = eps <= z <= 1 - eps
//   warp_c   = argmin |mask_c (A w - ref[c])|^2                               (normal equations in double, LDL^T)
//   cur     <- clip(row . warp, 0, 1)
// k_cc_pass<UPDATE, ACCUM>: with UPDATE, cur = clip(row(prev) . warp, 0, 1) is formed from the previous iterate and the previous solve's
// warp (in double, rounded once to float32) and written; with ACCUM, blockIdx.y = channel accumulates the upper triangle of A^T A (55) and
// A^T b (10) in double per thread, sums them over the wave on the DPP path and over the workgroup's four waves in a fixed order, and writes
// one partial per workgroup.  No atomics anywhere: the result is bit-reproducible.  k_cc_solve (one workgroup) adds the partials in a
// fixed order, factors the three systems and writes the float32 warp; a pivot that is not positive beyond rounding, or a non-finite
// result, sets the channel's bit of *status (the bits of the first iteration in which any channel failed are kept).  num_iters iterations are num_iters + 1 passes and num_iters solves on one stream with no
// host round trip: pass 0 only accumulates (cur = img), pass num_iters only updates (into `out`).
#include "ucn_common.h"
#include "wave_dpp.h"

namespace {

constexpr uint32_t CC_THREADS = 256, CC_MAX_BLOCKS = 512, CC_TERMS = 65, CC_SEGMENTS = 5, CC_SOLVE_THREADS = 1024;
// a pivot d_j <= 2^-40 A_jj is zero to rounding: forming it lost 40 of double's 53 bits, cond(A^T A) >= 1e12, so cond(A) >= 1e6 -- the
// float32 pixels do not determine such a system
constexpr double CC_PIVOT_FLOOR = 9.094947017729282e-13;

__device__ __forceinline__ bool cc_unclipped(float z, float lo, float hi) { return z >= lo && z <= hi; }
__host__ __device__ constexpr uint32_t cc_tri(uint32_t i, uint32_t j) { return i * 10u - i * (i - 1u) / 2u + (j - i); }   // i <= j

template <bool UPDATE, bool ACCUM>
__global__ __launch_bounds__(CC_THREADS) void k_cc_pass(const float *__restrict__ prev, const float *__restrict__ img0, const float *__restrict__ ref,
                                                        const float *__restrict__ warp, uint32_t n, float lo, float hi,
                                                        float *__restrict__ cur_out, double *__restrict__ partials) {
    __shared__ double s_part[CC_THREADS / 64][CC_TERMS];
    const uint32_t c = blockIdx.y;
    double w[UPDATE ? 30 : 1];
    if (UPDATE) {
#pragma unroll
        for (int i = 0; i < 30; i++) w[i] = (double)warp[i];
    }
    double acc[ACCUM ? CC_TERMS : 1];
    if (ACCUM) {
#pragma unroll
        for (uint32_t k = 0; k < CC_TERMS; k++) acc[k] = 0.0;
    }
    const uint64_t stride = (uint64_t)gridDim.x * CC_THREADS;
    for (uint64_t p = (uint64_t)blockIdx.x * CC_THREADS + threadIdx.x; p < n; p += stride) {
        float r = prev[p * 3 + 0], g = prev[p * 3 + 1], b = prev[p * 3 + 2];
        if (UPDATE) {
            const double dr = r, dg = g, db = b;
            const double row[10] = {dr * dr, dr * dg, dr * db, dg * dg, dg * db, db * db, dr, dg, db, 1.0};
            double o[3];
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < 10; i++) s = fma(row[i], w[i * 3 + ch], s);
                o[ch] = fmin(fmax(s, 0.0), 1.0);
            }
            r = (float)o[0]; g = (float)o[1]; b = (float)o[2];
            if (c == 0) { cur_out[p * 3 + 0] = r; cur_out[p * 3 + 1] = g; cur_out[p * 3 + 2] = b; }
        }
        if (ACCUM) {
            const float cur_c = c == 0 ? r : (c == 1 ? g : b);
            const float in_c = UPDATE ? img0[p * 3 + c] : cur_c;             // pass 0: the current image is the input image
            const float ref_c = ref[p * 3 + c];
            if (cc_unclipped(in_c, lo, hi) && cc_unclipped(cur_c, lo, hi) && cc_unclipped(ref_c, lo, hi)) {
                const double dr = r, dg = g, db = b;
                const double a[10] = {dr * dr, dr * dg, dr * db, dg * dg, dg * db, db * db, dr, dg, db, 1.0};
                const double rhs = ref_c;
#pragma unroll
                for (uint32_t i = 0; i < 10; i++) {
#pragma unroll
                    for (uint32_t j = i; j < 10; j++) acc[cc_tri(i, j)] = fma(a[i], a[j], acc[cc_tri(i, j)]);
                    acc[55 + i] = fma(a[i], rhs, acc[55 + i]);
                }
            }
        }
    }
    if (ACCUM) {
#pragma unroll
        for (uint32_t k = 0; k < CC_TERMS; k++) {
            const double v = wave_sum_dpp<double>(acc[k]);
            if ((threadIdx.x & 63u) == 0u) s_part[threadIdx.x >> 6][k] = v;
        }
        __syncthreads();
        if (threadIdx.x < CC_TERMS)
            partials[((size_t)c * gridDim.x + blockIdx.x) * CC_TERMS + threadIdx.x] =
                (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
    }
}

// One workgroup.  Threads (segment, channel, term) add their segment of the partials in block order, the segments are added in order,
// then thread c < 3 factors channel c's system in place in the LDS (upper triangle: L_ij, i > j, at tri(j, i); d_j at tri(j, j)); its loops stay
// rolled, so the system lives in the LDS and not in 130 registers of a 1024-thread workgroup.
__global__ __launch_bounds__(CC_SOLVE_THREADS) void k_cc_solve(const double *__restrict__ partials, uint32_t nb, int first, float *__restrict__ warp,
                                                              float *__restrict__ warp_copy, int32_t *__restrict__ status) {
    __shared__ double s_seg[CC_SEGMENTS][3 * CC_TERMS];
    __shared__ double s_m[3][CC_TERMS];
    __shared__ double s_x[3][10];
    __shared__ int s_bad[3];
    const uint32_t t = threadIdx.x;
    if (t < CC_SEGMENTS * 3 * CC_TERMS) {
        const uint32_t seg = t / (3 * CC_TERMS), v = t - seg * (3 * CC_TERMS), c = v / CC_TERMS, k = v - c * CC_TERMS;
        const uint32_t b0 = (uint32_t)((uint64_t)nb * seg / CC_SEGMENTS), b1 = (uint32_t)((uint64_t)nb * (seg + 1) / CC_SEGMENTS);
        double s = 0.0;
        for (uint32_t b = b0; b < b1; b++) s += partials[((size_t)c * nb + b) * CC_TERMS + k];
        s_seg[seg][v] = s;
    }
    __syncthreads();
    if (t < 3 * CC_TERMS) {
        double s = s_seg[0][t];
#pragma unroll
        for (uint32_t seg = 1; seg < CC_SEGMENTS; seg++) s += s_seg[seg][t];
        s_m[t / CC_TERMS][t % CC_TERMS] = s;
    }
    __syncthreads();
    if (t < 3) {
        double *m = s_m[t], *x = s_x[t];
        int bad = 0;
#pragma unroll 1
        for (uint32_t j = 0; j < 10; j++) {
            const double diag = m[cc_tri(j, j)];
            double d = diag;
    #pragma unroll 1
        for (uint32_t k = 0; k < j; k++) { const double l = m[cc_tri(k, j)]; d -= l * l * m[cc_tri(k, k)]; }
            if (!(d > diag * CC_PIVOT_FLOOR)) bad = 1;           // also a NaN, and an empty system (diag = 0)
            m[cc_tri(j, j)] = d;
    #pragma unroll 1
        for (uint32_t i = j + 1; i < 10; i++) {
                double s = m[cc_tri(j, i)];
        #pragma unroll 1
        for (uint32_t k = 0; k < j; k++) s -= m[cc_tri(k, i)] * m[cc_tri(k, j)] * m[cc_tri(k, k)];
                m[cc_tri(j, i)] = s / d;
            }
        }
#pragma unroll 1
        for (uint32_t i = 0; i < 10; i++) {                       // L y = A^T b
            double s = m[55 + i];
    #pragma unroll 1
        for (uint32_t k = 0; k < i; k++) s -= m[cc_tri(k, i)] * x[k];
            x[i] = s;
        }
#pragma unroll 1
        for (uint32_t i = 0; i < 10; i++) x[i] /= m[cc_tri(i, i)];
#pragma unroll 1
        for (uint32_t ii = 0; ii < 10; ii++) {                    // L^T w = D^-1 y
            const uint32_t i = 9u - ii;
            double s = x[i];
    #pragma unroll 1
        for (uint32_t k = i + 1; k < 10; k++) s -= m[cc_tri(i, k)] * x[k];
            x[i] = s;
        }
#pragma unroll 1
        for (uint32_t i = 0; i < 10; i++) {
            const float wf = (float)x[i];
            if (!isfinite(wf)) bad = 1;
            warp[i * 3 + t] = wf;
            if (warp_copy) warp_copy[i * 3 + t] = wf;
        }
        s_bad[t] = bad;
    }
    __syncthreads();
    if (t == 0) {
        const int32_t bits = s_bad[0] | (s_bad[1] << 1) | (s_bad[2] << 2);
        // a deficient channel's warp is garbage or NaN, its estimate collapses to clipped values (a NaN clips to 0) and every channel's later
        // systems, which share the row, fail after it: keep the first failure's bits
        if (first || (*status == 0 && bits != 0)) *status = bits;
    }
}

inline uint32_t cc_blocks(uint32_t n) {
    const uint32_t nb = ucn_div_up(n, CC_THREADS);
    return nb < CC_MAX_BLOCKS ? (nb ? nb : 1u) : CC_MAX_BLOCKS;
}
inline size_t cc_cur_bytes(uint32_t n) { return ((size_t)n * 3 * sizeof(float) + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t ucn_colour_correct_ws_bytes(uint32_t n_pixels) {
    return 2 * cc_cur_bytes(n_pixels) + (size_t)3 * cc_blocks(n_pixels) * CC_TERMS * sizeof(double) + 256 /*the warp [10][3]*/ + 256 /*alignment*/;
}

extern "C" int ucn_colour_correct(const float *img, const float *ref, uint32_t n_pixels, uint32_t num_iters, float eps, void *workspace,
                                  float *out, float *warps, int32_t *status, ucn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    UCN_REQUIRE(status, "colour_correct: null status pointer");
    UCN_REQUIRE(n_pixels == 0 || (img && ref && out), "colour_correct: null image pointer");
    UCN_REQUIRE(n_pixels == 0 || num_iters == 0 || workspace, "colour_correct: null workspace");
    if (n_pixels == 0 || num_iters == 0) {
        if (hipMemsetAsync(status, 0, sizeof(int32_t), stream) != hipSuccess) return ucn_fail("colour_correct: clearing the status word failed");
        if (n_pixels && out != img &&
            hipMemcpyAsync(out, img, (size_t)n_pixels * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess)
            return ucn_fail("colour_correct: copying the image failed");
        return 0;
    }
    UCN_REQUIRE(out != img && out != ref, "colour_correct: out must not alias an input");
    const uint32_t nb = cc_blocks(n_pixels);
    uint8_t *base = reinterpret_cast<uint8_t *>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    float *cur[2] = {reinterpret_cast<float *>(base), reinterpret_cast<float *>(base + cc_cur_bytes(n_pixels))};
    double *partials = reinterpret_cast<double *>(base + 2 * cc_cur_bytes(n_pixels));
    float *warp = reinterpret_cast<float *>(partials + (size_t)3 * nb * CC_TERMS);
    const float lo = eps, hi = (float)(1.0 - (double)eps);
    const float *prev = img;
    for (uint32_t it = 0; it <= num_iters; it++) {
        if (it == 0) {
            hipLaunchKernelGGL((k_cc_pass<false, true>), dim3(nb, 3), dim3(CC_THREADS), 0, stream, prev, img, ref, warp, n_pixels, lo, hi,
                               (float *)nullptr, partials);
        } else if (it < num_iters) {
            float *next = cur[it & 1u];
            hipLaunchKernelGGL((k_cc_pass<true, true>), dim3(nb, 3), dim3(CC_THREADS), 0, stream, prev, img, ref, warp, n_pixels, lo, hi, next,
                               partials);
            prev = next;
        } else {
            hipLaunchKernelGGL((k_cc_pass<true, false>), dim3(nb, 1), dim3(CC_THREADS), 0, stream, prev, img, ref, warp, n_pixels, lo, hi, out,
                               (double *)nullptr);
            break;
        }
        hipLaunchKernelGGL(k_cc_solve, dim3(1), dim3(CC_SOLVE_THREADS), 0, stream, partials, nb, it == 0 ? 1 : 0, warp,
                           warps ? warps + (size_t)it * 30 : (float *)nullptr, status);
    }
    UCN_LAUNCH_CHECK("colour_correct");
    return 0;
}
