// The geometry of one sample, as every grid-featurisation unit derives it: cone cast -> contraction -> the [0,1] grid
// coordinates and damping arguments of the sample's six multisample Gaussians.
//   render.cast_rays            (internal/render.py:94-152)
//   coord.track_linearize       (coord.py:60-116, 'contract')
//   the /2 and the erf argument (models.py:491-496)
// The contract between the units: the table gradient (march_features_bwd.hip) and the scale planes (march_scale.hip)
// RE-DERIVE the Gaussians the gather (march_features.hip) used instead of reading them back, so all three go through
// cast_sample / contract_to_unit / erf_pos below and nothing else -- a change here changes all of them together.
// Everything is force-inlined into its callers; the host helpers (make_hex, field_levels) are per-unit copies.
//
// UCN_SAME_IN_EVERY_UNIT on cast_sample / contract_to_unit.  Their `probe`, `sd_out` and `warp` arguments are only varied by the
// probe and points kernels, which live in march_features.hip.  Both functions have internal linkage (their argument types sit
// in the anonymous namespace, which the kernels' mangled names need), so in a unit where every call passes nullptr / true the
// compiler's interprocedural constant propagation folds those branches BEFORE inlining, and the same arithmetic comes out in
// another schedule and register assignment than in the unit that holds the probes (28 kernels of the gradient and scale units
// differed from the single-file build that way: profiles/featurise_split/isa_identity.txt).  `used` keeps the compiler from
// treating a unit's calls as all there are; the kernels then inline one and the same body wherever they are compiled, the one
// the probes exercise.  Cost: an uncalled device copy of each function per unit (~3,000 instructions beside kernels of 14-49 k).
#define UCN_SAME_IN_EVERY_UNIT __attribute__((used))
//
// Which arithmetic is exact and which is fast (the gather is VALU-bound with its tables L2/MALL-resident, ~3000 VALU
// instructions per (sample, level): rocprofv3, r01b):
//   * quantities that only feed the erf damping (std) use fast reciprocals / exp2-log2 instead of
//     IEEE division and powf, and erf itself is the Abramowitz-Stegun 7.1.26 form (|err| <= 1.5e-7);
//     everything that feeds a COORDINATE uses correctly-rounded div/sqrt and no contraction.  Measured
//     (tests/test_bracket_gpu.py, profiles/bracket/bracket_report.txt): 3806 of 3828 eval-pattern and
//     3785 of 3828 training-pattern multisample positions of the cast fixture are bit-identical to the
//     reference's, the others differ by <= 4.8e-7 (1 ulp of 8: the 3-term basis sum is associated
//     differently, the training angles go through v_sin / v_cos); against a float64 evaluation the
//     kernel's positions are as far off as the reference's own float32 ones (ratio 0.87 - 1.00).  The
//     interpolation for GIVEN float32 positions is bit-identical to the reference's (fixed fmaf chain, grid_rows.h);
//     the fast-math contracted std is up to 2.4x the reference's own float32 error (9e-7 relative).
#pragma once
#include "ucn_common.h"

namespace {

struct HexPattern {
    float cs[2][6];   // cos of the deterministic angles for even / odd samples (render.py:126-131)
    float sn[2][6];
    float ang[6];     // pi/3 * [0,2,4,3,5,1]   (render.py:119)
    float cj[6];      // 3/sqrt(7) * (2j/5 - 1)  (render.py:116)
};

// sdist: normalised fenceposts [N,S+1] of the identity curve, read with near_ / far_; in the kernels' TD = true variants
// it holds metric fenceposts (ucn_s_to_t's tdist of a warped Model.raydist_fn) and near_ / far_ are unused.
struct RayInputs {
    const float *sdist, *near_, *far_, *origins, *dirs, *basis, *radii, *flip, *spin;
};

// erf(x), x >= 0: Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7 (the damping multiplies O(1) features)
__device__ __forceinline__ float erf_pos(float x) {
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, x, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    return fmaf(-(p * t), __builtin_amdgcn_exp2f(-1.4426950408889634f * x * x), 1.0f);
}

// coord.py:60-72 followed by the /2 of models.py:491-493; returns the [0,1] grid coordinate (exact op
// sequence of the reference) and rs = 1/sqrt(8 std^2) of the contracted, halved std (fast math: it only
// feeds the erf damping).
// sd_out (ucn_cast_probe / ucn_contract_probe only): the contracted, halved std as the damping sees it.
UCN_SAME_IN_EVERY_UNIT __device__ __forceinline__ void contract_to_unit(float x, float y, float z, float sd, bool warp, float &u0, float &u1,
                                                 float &u2, float &rs, float &c0, float &c1, float &c2,
                                                 float *sd_out = nullptr) {
    if (warp) {
        const float m = fmaxf((x * x + y * y) + z * z, UCN_EPS);
        if (!(m <= 1.0f)) {
            const float root = sqrtf(m);
            const float k = (2.0f * root - 1.0f) / m;
            x = k * x; y = k * y; z = k * z;
            // ((2 root - 1)^(1/3) / root)^2 ; coord.py:69
            const float cb = __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(2.0f * root - 1.0f) * 0.3333333432674408f);
            const float sh = cb * __builtin_amdgcn_rcpf(root);
            sd = (sh * sh) * sd;
        }
        x = x / 2.0f; y = y / 2.0f; z = z / 2.0f;
        sd = sd / 2.0f;
    }
    c0 = x; c1 = y; c2 = z;
    u0 = (x + 1.0f) / 2.0f; u1 = (y + 1.0f) / 2.0f; u2 = (z + 1.0f) / 2.0f;    // grid.py:162, bound = 1
    rs = __builtin_amdgcn_rsqf(8.0f * (sd * sd));
    if (sd_out) *sd_out = sd;
}

// The six multisample Gaussians of sample (ray, s): render.py:108-152 then contract_to_unit.
// Shared by the forward and the backward kernel (the backward recomputes it instead of reading back
// 6x4 floats per sample).  TD: in.sdist holds metric fenceposts (see RayInputs).
// WARP = false (MLP.warp_fn = None, a bounded scene): the Gaussians reach the grid as cast, u = (x + 1) / 2 and std unscaled.
// A template argument, not a run-time one: with WARP = true the body is the one every kernel inlined before the argument
// existed, so those kernels keep their machine code (profiles/unwarped/isa_identity.txt).  A kernel that calls this hands on a
// trailing `bool WARP = true` of its own: one __global__ text per kernel, no *_body twin and no k_*_unwarped sibling.
template <bool TD = false, bool WARP = true>
UCN_SAME_IN_EVERY_UNIT __device__ __forceinline__ void cast_sample(const RayInputs &in, const HexPattern &hx, float std_scale, uint32_t ray,
                                            uint32_t s, uint32_t S, float (&u)[6][3], float (&rs)[6],
                                            float (&csum)[3], float &tsum, float *probe = nullptr) {
    const float nr = TD ? 0.0f : in.near_[ray], fr = TD ? 0.0f : in.far_[ray];
    const float s0 = in.sdist[(size_t)ray * (S + 1) + s], s1 = in.sdist[(size_t)ray * (S + 1) + s + 1];
    const float t0 = TD ? s0 : s0 * fr + (1.0f - s0) * nr, t1 = TD ? s1 : s1 * fr + (1.0f - s1) * nr;
    const float rad = in.radii[ray];
    const float *bp = in.basis + (size_t)ray * 6;
    const float e1x = bp[0], e1y = bp[1], e1z = bp[2], e2x = bp[3], e2y = bp[4], e2z = bp[5];
    const float dx = in.dirs[ray * 3 + 0], dy = in.dirs[ray * 3 + 1], dz = in.dirs[ray * 3 + 2];
    const float ox = in.origins[ray * 3 + 0], oy = in.origins[ray * 3 + 1], oz = in.origins[ray * 3 + 2];
    // render.py:112-117
    const float t_m = (t0 + t1) / 2.0f, t_d = (t1 - t0) / 2.0f;
    const float td2 = t_d * t_d, tm2 = t_m * t_m;
    const float a_ = t_d / (td2 + 3.0f * tm2);
    const float inner = td2 - tm2;
    const float root = sqrtf(inner * inner + 4.0f * (tm2 * tm2));
    const float base = t1 * t1 + 2.0f * tm2;
    // angles: deterministic hexagon (rotated 30 deg + mirrored on odd samples) or random spin/flip
    const bool rnd = in.flip != nullptr;
    float spin2pi = 0.0f;
    bool keep = true;
    if (rnd) {
        keep = in.flip[(size_t)ray * S + s] > 0.5f;
        spin2pi = 6.2831854820251465f * in.spin[(size_t)ray * S + s];
    }
    const float sd_unit = (std_scale * rad) * 0.70710678118654752f;   // std only: multiply instead of IEEE divide
    const uint32_t odd = s & 1u;
    csum[0] = csum[1] = csum[2] = 0.0f;
    tsum = 0.0f;
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        const float t = t0 + a_ * (base + hx.cj[j] * root);
        float cs, sn;
        if (rnd) {
            float ang = hx.ang[j] + spin2pi;
            if (!keep) ang = 5.235987663269043f - ang;
            // v_sin_f32 / v_cos_f32 (argument in revolutions, |error| ~1e-6 absolute): the angle only places a multisample
            // on its circle of radius ~r t / sqrt(2) (render.py:126-136), so the position moves by < 1e-9.  The precise
            // cosf / sinf were ~100 VALU instructions per point and level group; removing them did not change the training
            // forward's time (2.02 ms before and after: random rays leave it bound by the gather, not by VALU).
            const float rev = ang * 0.15915494309189535f;
            cs = __builtin_amdgcn_cosf(rev); sn = __builtin_amdgcn_sinf(rev);
        } else {
            cs = odd ? hx.cs[1][j] : hx.cs[0][j];
            sn = odd ? hx.sn[1][j] : hx.sn[0][j];
        }
        const float rt = rad * t;
        const float l0 = (rt * cs) / 1.4142135381698608f, l1 = (rt * sn) / 1.4142135381698608f;
        // math.matmul with basis^T (render.py:146-148): sum_k local_k * axis_k, then + origin
        const float wx = ((l0 * e1x + l1 * e2x) + t * dx) + ox;
        const float wy = ((l0 * e1y + l1 * e2y) + t * dy) + oy;
        const float wz = ((l0 * e1z + l1 * e2z) + t * dz) + oz;
        float c0, c1, c2;
        if (probe) {
            // ucn_cast_probe: what render.cast_rays returns (means, stds, t) and what the grid sees behind the contraction
            float *pr = probe + j * UCN_CAST_PROBE_FLOATS;
            float sdc;
            contract_to_unit(wx, wy, wz, sd_unit * t, WARP, u[j][0], u[j][1], u[j][2], rs[j], c0, c1, c2, &sdc);
            pr[0] = wx; pr[1] = wy; pr[2] = wz; pr[3] = sd_unit * t; pr[4] = t;
            pr[5] = c0; pr[6] = c1; pr[7] = c2; pr[8] = sdc; pr[9] = rs[j];
        } else {
            contract_to_unit(wx, wy, wz, sd_unit * t, WARP, u[j][0], u[j][1], u[j][2], rs[j], c0, c1, c2);
        }
        csum[0] += c0; csum[1] += c1; csum[2] += c2; tsum += t;
    }
}

static inline HexPattern make_hex() {
    HexPattern hx;
    const int order[6] = {0, 2, 4, 3, 5, 1};
    const float third = (float)(M_PI / 3.0), sixth = (float)(M_PI / 6.0), fivethirds = (float)(M_PI * 5.0 / 3.0);
    for (int j = 0; j < 6; j++) {
        const float a = third * (float)order[j];
        hx.ang[j] = a;
        hx.cs[0][j] = cosf(a);
        hx.sn[0][j] = sinf(a);
        const float o = fivethirds - (a + sixth);
        hx.cs[1][j] = cosf(o);
        hx.sn[1][j] = sinf(o);
        hx.cj[j] = (float)(3.0 / sqrt(7.0)) * ((float)(2 * j) / 5.0f - 1.0f);
    }
    return hx;
}

static inline int field_levels(const ucn_field_t *f, UcnLevels *lv) {
    UCN_REQUIRE(f && f->embeddings && f->offsets_host && f->grid_sizes_host, "field: grid pointers missing");
    UCN_REQUIRE(f->level_dim == 1 || f->level_dim == 2 || f->level_dim == 4 || f->level_dim == 8,
                "GridEncoding: C must be 1, 2, 4, or 8.");
    return ucn_build_levels(lv, f->offsets_host, f->grid_sizes_host, f->num_levels, f->level_dim, 3,
                            f->log2_per_level_scale, f->base_resolution, 0, 0);
}

}  // namespace
