// Training and test batches assembled on the device from a resident dataset: rays, gathered image planes and the broadcast
// columns in one launch, one thread per ray.
//
//   k_train_batch <- datasets.py:386-476 (_make_ray_batch, both branches): camera_utils.cast_ray_batch through the cast triple
//                    (cam_cast, x_cast, y_cast), `images[cam, y, x]` and its siblings (disp_images, sky_segments,
//                    normal_images, alphas) through the look-up triple (cam_look, x_look, y_look), the near / far / lossmult /
//                    cam_idx columns; raw_utils.py:38-46 (pixels_to_bayer_mask) for the lossmult of apply_bayer_mask
//
// The two triples differ only in the virtual-pose branch (:457-473), which casts a ray through a virtual camera and takes its
// supervision from the real pixel that warps onto it.  The ray is rays_core.h's ray_from_pixel, the text k_generate_rays runs,
// so the rays of both kernels are the same bits; the planes are float32 in the dataset and copied bit for bit.
//
// Traffic per ray: 12 B of indices in (24 with a look-up triple), 60 B of rays + 16 B of columns out, and per plane one
// C-float read at a random address plus C floats out.  A streaming write and a 4..16 B random gather: nothing is reused
// between threads, so there is nothing to tile or to stage in LDS.
//
// An index that would read outside its array never does: the thread writes NaN instead and stores 1 into a status word
// (plain vector store; every writer stores the same value, so the race is benign).  status[0] = a look-up index outside
// [0, n_images) x [0, H) x [0, W) (NaN planes), status[1] = a cast camera outside [0, n_cams) (NaN rays).
#include "rays_core.h"

namespace {

struct BatchPlanes {
    const float *src[UCN_BATCH_MAX_PLANES];
    float *dst[UCN_BATCH_MAX_PLANES];
    uint32_t channels[UCN_BATCH_MAX_PLANES];
    uint32_t count;
};

struct BatchIndex {
    const int32_t *cam_cast, *x_cast, *y_cast, *cam_look, *x_look, *y_look;
    int32_t cam_scalar;
};

template <int MODEL>
__global__ __launch_bounds__(256) void k_train_batch(BatchIndex ix, const double *__restrict__ pixtocams,
                                                     const double *__restrict__ camtoworlds, uint32_t n_cams, uint32_t n_images,
                                                     uint32_t height, uint32_t width, uint32_t n, float near_v, float far_v,
                                                     const float *__restrict__ lossmult_in, uint32_t lossmult_channels, int flags,
                                                     BatchPlanes planes, RayOut out, uint32_t *__restrict__ status) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float nan = __builtin_nanf("");
    const int32_t cam = ix.cam_cast ? ix.cam_cast[i] : ix.cam_scalar;
    const int32_t x = ix.x_cast ? ix.x_cast[i] : (int32_t)(i % width);           // camera_utils.py:368-370 'xy' meshgrid
    const int32_t y = ix.y_cast ? ix.y_cast[i] : (int32_t)(i / width);
    if (cam >= 0 && (uint32_t)cam < n_cams) {
        ray_from_pixel<MODEL>(i, cam, (double)x, (double)y, pixtocams, camtoworlds, near_v, far_v, out);
    } else {                                                                     // the camera tables end before this row
#pragma unroll
        for (int k = 0; k < 3; k++) {
            out.origins[(size_t)i * 3 + k] = nan;
            out.directions[(size_t)i * 3 + k] = nan;
            out.viewdirs[(size_t)i * 3 + k] = nan;
            out.cam_dirs[(size_t)i * 3 + k] = nan;
        }
        out.radii[i] = nan;
        if (out.imageplane) out.imageplane[(size_t)i * 2 + 0] = out.imageplane[(size_t)i * 2 + 1] = nan;
        if (out.near_) out.near_[i] = near_v;
        if (out.far_) out.far_[i] = far_v;
        if (status) status[1] = 1u;
    }
    if (out.cam_idx) out.cam_idx[i] = (float)cam;                                // datasets.py:418 / :426, the cast camera

    const int32_t lc = ix.cam_look ? ix.cam_look[i] : cam, lx = ix.x_look ? ix.x_look[i] : x, ly = ix.y_look ? ix.y_look[i] : y;
    if (out.lossmult) {
        if (flags & UCN_BATCH_BAYER_MASK) {                                      // raw_utils.py:38-46, red at (0, 0)
            const bool ex = (lx & 1) == 0, ey = (ly & 1) == 0;
            out.lossmult[(size_t)i * 3 + 0] = ex && ey ? 1.0f : 0.0f;
            out.lossmult[(size_t)i * 3 + 1] = ex != ey ? 1.0f : 0.0f;
            out.lossmult[(size_t)i * 3 + 2] = !ex && !ey ? 1.0f : 0.0f;
        } else if (lossmult_in) {
            for (uint32_t k = 0; k < lossmult_channels; k++)
                out.lossmult[(size_t)i * lossmult_channels + k] = lossmult_in[(size_t)i * lossmult_channels + k];
        } else {
            out.lossmult[i] = 1.0f;                                              // datasets.py:415
        }
    }
    if (planes.count == 0) return;
    const bool inside = lc >= 0 && (uint32_t)lc < n_images && ly >= 0 && (uint32_t)ly < height && lx >= 0 && (uint32_t)lx < width;
    const size_t pixel = ((size_t)(inside ? lc : 0) * height + (size_t)(inside ? ly : 0)) * width + (size_t)(inside ? lx : 0);
#pragma unroll
    for (uint32_t p = 0; p < UCN_BATCH_MAX_PLANES; p++) {
        if (p >= planes.count) break;
        const uint32_t C = planes.channels[p];
        const float *__restrict__ src = planes.src[p] + pixel * C;
        float *__restrict__ dst = planes.dst[p] + (size_t)i * C;
        for (uint32_t k = 0; k < C; k++) dst[k] = inside ? src[k] : nan;
    }
    if (!inside && status) status[0] = 1u;
}

}  // namespace

extern "C" int ucn_train_batch(const int32_t *cam_cast, int32_t cam_cast_scalar, const int32_t *x_cast, const int32_t *y_cast,
                               const int32_t *cam_look, const int32_t *x_look, const int32_t *y_look, const double *pixtocams,
                               const double *camtoworlds, uint32_t n_cams, uint32_t n_images, uint32_t height, uint32_t width,
                               uint32_t n_rays, const float *const *plane_src_host, float *const *plane_dst_host,
                               const uint32_t *plane_channels_host, uint32_t n_planes, float near_, float far_,
                               const float *lossmult_in, uint32_t lossmult_channels, int flags, float *origins, float *directions,
                               float *viewdirs, float *radii, float *imageplane, float *cam_dirs, float *near_out, float *far_out,
                               float *lossmult_out, float *cam_idx_out, uint32_t *status, int camera_model, ucn_stream_t stream) {
    UCN_REQUIRE(camera_model == 0 || camera_model == 1, "train_batch: camera model %d (0 = perspective, 1 = panorama)", camera_model);
    UCN_REQUIRE((flags & ~UCN_BATCH_BAYER_MASK) == 0, "train_batch: unknown flags 0x%x", flags);
    UCN_REQUIRE(n_planes <= UCN_BATCH_MAX_PLANES, "train_batch: %u planes, at most %d", n_planes, UCN_BATCH_MAX_PLANES);
    if (n_rays == 0) return 0;                            // an empty batch has null data pointers
    UCN_REQUIRE(pixtocams && camtoworlds && origins && directions && viewdirs && radii && cam_dirs,
                "train_batch: null pointer argument");
    UCN_REQUIRE((x_cast == nullptr) == (y_cast == nullptr), "train_batch: x_cast and y_cast come together");
    UCN_REQUIRE(x_cast || (width > 0 && (uint64_t)width * height == n_rays),
                "train_batch: without pixel coordinates n_rays must be width * height (%u x %u != %u)", width, height, n_rays);
    UCN_REQUIRE(n_cams > 0 && (cam_cast || (cam_cast_scalar >= 0 && (uint32_t)cam_cast_scalar < n_cams)),
                "train_batch: camera index %d out of range [0, %u)", cam_cast_scalar, n_cams);
    UCN_REQUIRE((cam_look == nullptr) == (x_look == nullptr) && (x_look == nullptr) == (y_look == nullptr),
                "train_batch: cam_look, x_look and y_look come together");
    UCN_REQUIRE(!lossmult_in || (lossmult_out && lossmult_channels >= 1 && lossmult_channels <= 4),
                "train_batch: a per-ray lossmult needs its output and 1..4 channels (%u)", lossmult_channels);
    BatchPlanes planes{};
    planes.count = n_planes;
    if (n_planes) {
        UCN_REQUIRE(plane_src_host && plane_dst_host && plane_channels_host, "train_batch: null plane table");
        UCN_REQUIRE(n_images > 0 && height > 0 && width > 0, "train_batch: planes of %u x %u x %u pixels", n_images, height, width);
        for (uint32_t p = 0; p < n_planes; p++) {
            UCN_REQUIRE(plane_src_host[p] && plane_dst_host[p], "train_batch: plane %u has a null pointer", p);
            UCN_REQUIRE(plane_channels_host[p] >= 1 && plane_channels_host[p] <= 4, "train_batch: plane %u has %u channels (1..4)", p,
                        plane_channels_host[p]);
            planes.src[p] = plane_src_host[p];
            planes.dst[p] = plane_dst_host[p];
            planes.channels[p] = plane_channels_host[p];
        }
    }
    const BatchIndex ix{cam_cast, x_cast, y_cast, cam_look, x_look, y_look, cam_cast_scalar};
    const RayOut out{origins, directions, viewdirs, radii, imageplane, cam_dirs, near_out, far_out, lossmult_out, cam_idx_out};
    const auto kernel = camera_model == 1 ? k_train_batch<1> : k_train_batch<0>;
    hipLaunchKernelGGL(kernel, dim3(ucn_div_up(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, ix, pixtocams, camtoworlds, n_cams,
                       n_images, height, width ? width : 1u, n_rays, near_, far_, lossmult_in, lossmult_channels, flags, planes, out,
                       status);
    UCN_LAUNCH_CHECK("train_batch");
    return 0;
}
