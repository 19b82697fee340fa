// One ray from one pixel of one camera: the body shared by k_generate_rays (rays.hip) and k_train_batch (batch.hip).
//
//   ray_from_pixel <- camera_utils.py:448-557 (pixels_to_rays: perspective pinhole, no distortion, no NDC) + datasets.py:446
//                     (cam_dirs) and the broadcast near / far columns of datasets.py:413-419; <1> = camtype == 'panoroma'
//                     (:507-510)
//
// Float64 with the reference's operation order (explicit mul / add, -ffp-contract=off; IEEE double division and sqrt) and one
// rounding at the store: both kernels run this one text, so their float32 rays are the same bits.
#pragma once
#include "ucn_common.h"

namespace {

struct RayOut {
    float *origins, *directions, *viewdirs, *radii, *imageplane, *cam_dirs, *near_, *far_, *lossmult, *cam_idx;
};

__device__ __forceinline__ void matvec3(const double *__restrict__ A, uint32_t ld, double x, double y, double z, double (&o)[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = (A[i * ld + 0] * x + A[i * ld + 1] * y) + A[i * ld + 2] * z;
}
__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// Ray i through pixel (x, y) of camera `cam`: origins, directions, viewdirs, radii, imageplane, cam_dirs and the near / far
// columns.  lossmult and cam_idx are the caller's.  MODEL 0 = perspective, 1 = panorama (camera_utils.py:507-510).
template <int MODEL>
__device__ __forceinline__ void ray_from_pixel(uint32_t i, int32_t cam, double x, double y, const double *__restrict__ pixtocams,
                                               const double *__restrict__ camtoworlds, float near_v, float far_v,
                                               const RayOut &out) {
    const double *P = pixtocams + (size_t)cam * 9, *M = camtoworlds + (size_t)cam * 12;
    // pixel centre and its +1 neighbours in x and y (:487-495), inverse intrinsics (:501), OpenCV -> OpenGL (:531)
    double c[3][3], d[3][3];
    matvec3(P, 3, x + 0.5, y + 0.5, 1.0, c[0]);
    matvec3(P, 3, (x + 1.0) + 0.5, y + 0.5, 1.0, c[1]);
    matvec3(P, 3, x + 0.5, (y + 1.0) + 0.5, 1.0, c[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if constexpr (MODEL == 1) {                                              // the image plane bent onto a cylinder (:507-510)
            sincos(c[k][0], &c[k][0], &c[k][2]);                                 // one argument reduction for both
        }
        c[k][1] = -c[k][1];
        c[k][2] = -c[k][2];
        matvec3(M, 4, c[k][0], c[k][1], c[k][2], d[k]);                          // camera rotation (:538)
    }
    const double nd = norm3(d[0][0], d[0][1], d[0][2]);
    const double dxn = norm3(d[1][0] - d[0][0], d[1][1] - d[0][1], d[1][2] - d[0][2]);      // :548-549
    const double dyn = norm3(d[2][0] - d[0][0], d[2][1] - d[0][1], d[2][2] - d[0][2]);
    const double radius = (0.5 * (dxn + dyn)) * 2.0 / 3.4641016151377544;        // :562, np.sqrt(12)
#pragma unroll
    for (int k = 0; k < 3; k++) {
        out.origins[(size_t)i * 3 + k] = (float)M[k * 4 + 3];
        out.directions[(size_t)i * 3 + k] = (float)d[0][k];
        out.viewdirs[(size_t)i * 3 + k] = (float)(d[0][k] / nd);                 // :544
        out.cam_dirs[(size_t)i * 3 + k] = (float)(-M[k * 4 + 2]);               // datasets.py:446
    }
    out.radii[i] = (float)radius;
    if (out.imageplane) {
        out.imageplane[(size_t)i * 2 + 0] = (float)c[0][0];
        out.imageplane[(size_t)i * 2 + 1] = (float)c[0][1];
    }
    if (out.near_) out.near_[i] = near_v;
    if (out.far_) out.far_[i] = far_v;
}

}  // namespace
