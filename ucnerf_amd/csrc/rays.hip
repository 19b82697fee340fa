// On-GPU ray generation for full frames and pixel batches.
//
//   k_generate_rays <- camera_utils.py:448-557 (pixels_to_rays: perspective pinhole, no distortion, no NDC -- the
//                      Waymo / UC-NeRF configuration, datasets.py:855) + datasets.py:421-447 (_make_ray_batch:
//                      cam_dirs and the broadcast near / far / lossmult / cam_idx columns); <1> = the same with
//                      camtype == 'panoroma' (:507-510, the nuScenes render path, datasets.py:872-878)
//   k_spherical_rays <- camera_utils.py:635-678 (cast_spherical_rays, render_camtype == 'pano', datasets.py:574-578)
//
// The two later models call the device's double sin / cos, which are not libm's to the last bit: their float32 batch is the
// reference's to within one float32 unit of the ray's vector norm (tests/golden/rays_pano.npz); what follows about
// bit-identity is the perspective kernel's, whose code they leave untouched.
//
// The reference does this with numpy on DataLoader workers, in FLOAT64 (integer pixel + .5 promotes everything), and
// casts the batch to float32 at the very end (datasets.py:476); 64 bytes per ray then cross PCIe (157 MB per
// 1920x1280 frame).  Here one thread derives one ray from two small per-camera matrices, in float64 with the
// reference's operation order (explicit mul / add, -ffp-contract=off; IEEE double division and sqrt), and rounds once
// at the store -- the float32 batch is bit-identical to the reference's (tests/golden/rays.npz).  The kernel is a pure
// streaming write: 68 B per ray (76 with the image plane) out, 8 B in when pixel coordinates are given.
#include "rays_core.h"

namespace {

// MODEL 0 = perspective, 1 = panorama (camera_utils.py:507-510, camtype == 'panoroma')
template <int MODEL>
__global__ __launch_bounds__(256) void k_generate_rays(const int32_t *__restrict__ pix_x, const int32_t *__restrict__ pix_y,
                                                       const int32_t *__restrict__ cam_idx, int32_t cam_scalar,
                                                       const double *__restrict__ pixtocams, const double *__restrict__ camtoworlds,
                                                       uint32_t width, uint32_t n, float near_v, float far_v, RayOut out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int32_t cam = cam_idx ? cam_idx[i] : cam_scalar;
    const double x = (double)(pix_x ? pix_x[i] : (int32_t)(i % width));          // camera_utils.py:368-370 'xy' meshgrid
    const double y = (double)(pix_y ? pix_y[i] : (int32_t)(i / width));
    ray_from_pixel<MODEL>(i, cam, x, y, pixtocams, camtoworlds, near_v, far_v, out);   // rays_core.h, shared with batch.hip
    if (out.lossmult) out.lossmult[i] = 1.0f;
    if (out.cam_idx) out.cam_idx[i] = (float)cam;
}

// R (-sin phi sin theta, cos phi, sin phi cos theta), camera_utils.py:643-650 (y is up)
__device__ __forceinline__ void sphere_dir(const double *__restrict__ M, double sp, double cp, double st, double ct, double (&o)[3]) {
    matvec3(M, 4, -sp * st, cp, sp * ct, o);
}

// One thread per pixel (i, j) of a height x width frame.  np.linspace(0, stop, n + 1) is arange * (stop / n) with the last
// value overwritten by stop, so grid line n is exactly 2 pi / pi.
__global__ __launch_bounds__(256) void k_spherical_rays(const double *__restrict__ M, uint32_t width, uint32_t height, uint32_t n,
                                                        float near_v, float far_v, RayOut out) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= n) return;
    const uint32_t i = idx / width, j = idx % width;
    const double two_pi = 6.283185307179586, pi = 3.141592653589793;            // 2 * np.pi, np.pi
    const double dth = two_pi / (double)width, dph = pi / (double)height;
    const double th0 = (double)j * dth, th1 = j + 1 == width ? two_pi : (double)(j + 1) * dth;
    const double ph0 = (double)i * dph, ph1 = i + 1 == height ? pi : (double)(i + 1) * dph;
    double st0, ct0, st1, ct1, sp0, cp0, sp1, cp1;
    sincos(th0, &st0, &ct0);
    sincos(th1, &st1, &ct1);
    sincos(ph0, &sp0, &cp0);
    sincos(ph1, &sp1, &cp1);
    double d[3][3];                                                              // (i, j), (i, j + 1), (i + 1, j)
    sphere_dir(M, sp0, cp0, st0, ct0, d[0]);
    sphere_dir(M, sp0, cp0, st1, ct1, d[1]);
    sphere_dir(M, sp1, cp1, st0, ct0, d[2]);
    const double dxn = norm3(d[1][0] - d[0][0], d[1][1] - d[0][1], d[1][2] - d[0][2]);      // :652-660
    const double dyn = norm3(d[2][0] - d[0][0], d[2][1] - d[0][1], d[2][2] - d[0][2]);
    const double radius = (0.5 * (dxn + dyn)) * 2.0 / 3.4641016151377544;        // :661, np.sqrt(12)
#pragma unroll
    for (int k = 0; k < 3; k++) {
        out.origins[(size_t)idx * 3 + k] = (float)M[k * 4 + 3];
        out.directions[(size_t)idx * 3 + k] = (float)d[0][k];
        out.viewdirs[(size_t)idx * 3 + k] = (float)d[0][k];                      // :655, not renormalised
        out.cam_dirs[(size_t)idx * 3 + k] = (float)(-M[k * 4 + 2]);              // datasets.py:446
    }
    out.radii[idx] = (float)radius;
    if (out.imageplane) {
        out.imageplane[(size_t)idx * 2 + 0] = 0.0f;                              // :663
        out.imageplane[(size_t)idx * 2 + 1] = 0.0f;
    }
    if (out.near_) out.near_[idx] = near_v;
    if (out.far_) out.far_[idx] = far_v;
    if (out.lossmult) out.lossmult[idx] = 1.0f;
    if (out.cam_idx) out.cam_idx[idx] = 0.0f;
}

}  // namespace

extern "C" int ucn_generate_rays_model(const int32_t *pix_x, const int32_t *pix_y, const int32_t *cam_idx, int32_t cam_idx_scalar,
                                       const double *pixtocams, const double *camtoworlds, uint32_t n_cams, uint32_t width,
                                       uint32_t height, uint32_t n_rays, float near_, float far_, float *origins,
                                       float *directions, float *viewdirs, float *radii, float *imageplane, float *cam_dirs,
                                       float *near_out, float *far_out, float *lossmult_out, float *cam_idx_out, int camera_model,
                                       ucn_stream_t stream) {
    UCN_REQUIRE(camera_model == 0 || camera_model == 1, "generate_rays: camera model %d (0 = perspective, 1 = panorama)", camera_model);
    if (n_rays == 0) return 0;                            // an empty batch has null data pointers
    UCN_REQUIRE(pixtocams && camtoworlds && origins && directions && viewdirs && radii && cam_dirs,
                "generate_rays: null pointer argument");
    UCN_REQUIRE((pix_x == nullptr) == (pix_y == nullptr), "generate_rays: pix_x and pix_y come together");
    UCN_REQUIRE(pix_x || (width > 0 && (uint64_t)width * height == n_rays),
                "generate_rays: without pixel coordinates n_rays must be width * height (%u x %u != %u)", width, height, n_rays);
    UCN_REQUIRE(n_cams > 0 && (cam_idx || (cam_idx_scalar >= 0 && (uint32_t)cam_idx_scalar < n_cams)),
                "generate_rays: camera index %d out of range [0, %u)", cam_idx_scalar, n_cams);
    const RayOut out{origins, directions, viewdirs, radii, imageplane, cam_dirs, near_out, far_out, lossmult_out, cam_idx_out};
    const auto kernel = camera_model == 1 ? k_generate_rays<1> : k_generate_rays<0>;
    hipLaunchKernelGGL(kernel, dim3(ucn_div_up(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, pix_x, pix_y, cam_idx,
                       cam_idx_scalar, pixtocams, camtoworlds, width ? width : 1u, n_rays, near_, far_, out);
    UCN_LAUNCH_CHECK("generate_rays");
    return 0;
}

extern "C" int ucn_generate_rays(const int32_t *pix_x, const int32_t *pix_y, const int32_t *cam_idx, int32_t cam_idx_scalar,
                                 const double *pixtocams, const double *camtoworlds, uint32_t n_cams, uint32_t width,
                                 uint32_t height, uint32_t n_rays, float near_, float far_, float *origins, float *directions,
                                 float *viewdirs, float *radii, float *imageplane, float *cam_dirs, float *near_out,
                                 float *far_out, float *lossmult_out, float *cam_idx_out, ucn_stream_t stream) {
    return ucn_generate_rays_model(pix_x, pix_y, cam_idx, cam_idx_scalar, pixtocams, camtoworlds, n_cams, width, height, n_rays,
                                   near_, far_, origins, directions, viewdirs, radii, imageplane, cam_dirs, near_out, far_out,
                                   lossmult_out, cam_idx_out, 0, stream);
}

extern "C" int ucn_spherical_rays(const double *camtoworld, uint32_t width, uint32_t height, float near_, float far_,
                                  float *origins, float *directions, float *viewdirs, float *radii, float *imageplane,
                                  float *cam_dirs, float *near_out, float *far_out, float *lossmult_out, float *cam_idx_out,
                                  ucn_stream_t stream) {
    const uint64_t n = (uint64_t)width * height;
    if (n == 0) return 0;                                 // an empty frame has null data pointers
    UCN_REQUIRE(n <= 0xffffffffull, "spherical_rays: %u x %u rays do not fit a 32-bit ray index", width, height);
    UCN_REQUIRE(camtoworld && origins && directions && viewdirs && radii && cam_dirs, "spherical_rays: null pointer argument");
    const RayOut out{origins, directions, viewdirs, radii, imageplane, cam_dirs, near_out, far_out, lossmult_out, cam_idx_out};
    hipLaunchKernelGGL(k_spherical_rays, dim3(ucn_div_up((uint32_t)n, 256)), dim3(256), 0, (hipStream_t)stream, camtoworld, width,
                       height, (uint32_t)n, near_, far_, out);
    UCN_LAUNCH_CHECK("spherical_rays");
    return 0;
}
