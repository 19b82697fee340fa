// Model.raydist_fn: the curve of coord.construct_ray_warps (coord.py:137-177) that maps a metric ray distance t to the
// normalised s in [0, 1] and back.  The one place where the six formulas live: ucn_s_to_t (march_ray.hip) evaluates
//     t = fn_inv(s * fn(far) + (1 - s) * fn(near))                                        (coord.py:175-176)
// per fencepost, and the geometry and compositing kernels read the resulting tdist.  fp32 in the reference's operation
// order, with the precise powf / logf / expf / IEEE division: near s_far the power inverse cancels (1 - 0.6 y + eps ~ 0),
// and the few ulp of an approximate instruction there become large errors in t.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/ucnerf_march.h"

// The curve and its constants.  The reference forms lam_1 = |lam - 1|, lam_1 / lam and 1 / lam as Python floats
// (coord.py:120-134) and each enters a float32 tensor op as one rounded scalar: derived here in double, then rounded.
struct UcnRaydist {
    int curve;
    float lam, lam_1, lam_ratio, inv_lam;
};

__host__ __device__ inline UcnRaydist ucn_raydist_make(int curve, double lam) {
    const double lam_1 = fabs(lam - 1.0);
    return UcnRaydist{curve, (float)lam, (float)lam_1, (float)(lam_1 / lam), (float)(1.0 / lam)};
}

// fn: the forward map of a metric distance before normalisation.
__device__ __forceinline__ float ucn_raydist_fwd(const UcnRaydist &r, float x) {
    switch (r.curve) {
        case UCN_RAYDIST_PIECEWISE:                    // coord.py:158: where(x < 1, .5 x, 1 - .5 / x)
            return x < 1.0f ? 0.5f * x : 1.0f - 0.5f / x;
        case UCN_RAYDIST_POWER:                        // coord.py:161 -> :120-124 power_transformation(2 x, lam)
            return r.lam_ratio * (powf((x * 2.0f) / r.lam_1 + 1.0f, r.lam) - 1.0f);
        case UCN_RAYDIST_RECIPROCAL: return 1.0f / x;
        case UCN_RAYDIST_LOG: return logf(x);
        case UCN_RAYDIST_EXP: return expf(x);
        case UCN_RAYDIST_SQRT: return sqrtf(x);
        case UCN_RAYDIST_SQUARE: return x * x;
        default: return x;                             // identity (raydist_fn = None)
    }
}

// fn_inv (coord.py:159, :162 -> :127-134, :165-172).  The power inverse keeps the reference's `+ eps`,
// eps = torch.finfo(float32).eps = FLT_EPSILON.
__device__ __forceinline__ float ucn_raydist_inv(const UcnRaydist &r, float y) {
    switch (r.curve) {
        case UCN_RAYDIST_PIECEWISE:                    // where(y < .5, 2 y, .5 / (1 - y))
            return y < 0.5f ? 2.0f * y : 0.5f / (1.0f - y);
        case UCN_RAYDIST_POWER:                        // inv_power_transformation(y, lam) / 2
            return ((powf((y * r.lam) / r.lam_1 + 1.0f + 1.1920928955078125e-07f, r.inv_lam) - 1.0f) * r.lam_1) / 2.0f;
        case UCN_RAYDIST_RECIPROCAL: return 1.0f / y;  // inv_mapping (coord.py:165-171): reciprocal <-> reciprocal,
        case UCN_RAYDIST_LOG: return expf(y);          // log <-> exp, sqrt <-> square
        case UCN_RAYDIST_EXP: return logf(y);
        case UCN_RAYDIST_SQRT: return y * y;
        case UCN_RAYDIST_SQUARE: return sqrtf(y);
        default: return y;
    }
}

// s_to_t of one fencepost of a ray with metric near / far and sn = fn(near), sf = fn(far) (coord.py:175, derived once per ray by
// the caller).  The identity curve is the expression the march kernels inline where they read normalised fenceposts (their
// TD = false variants), bit for bit.
__device__ __forceinline__ float ucn_raydist_s_to_t(const UcnRaydist &r, float s, float nr, float fr, float sn, float sf) {
    if (r.curve == UCN_RAYDIST_IDENTITY) return s * fr + (1.0f - s) * nr;
    return ucn_raydist_inv(r, s * sf + (1.0f - s) * sn);
}
