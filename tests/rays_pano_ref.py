"""Float64 numpy restatement of the two render-path camera models beyond the perspective pinhole -- a test helper, the CPU
reference the GPU tests use where the reference project itself is not present.

  panorama_rays    camera_utils.py:448-557 `pixels_to_rays` with camtype == 'panoroma' (:507-510), no distortion, no NDC:
                   (x, y, 1) -> (sin x, y, cos x) between the inverse intrinsics and the OpenCV -> OpenGL flip
  spherical_rays   camera_utils.py:635-678 `cast_spherical_rays`
  cam_dirs         datasets.py:446

Same numpy calls in the same order as the reference, so on one machine (same numpy, same libm) the results are bit-identical
to it: tests/test_rays_pano_cpu.py holds both functions to tests/golden/rays_pano.npz bit for bit.  Unlike the reference's
panorama branch (`[:, :, :, 0]`, 2-D pixel arrays only) this takes pixels of any shape.
"""
import numpy as np

PANORAMA = 'panoroma'
VECTOR_KEYS = ('origins', 'directions', 'viewdirs', 'imageplane', 'cam_dirs')
EPS = 2.0 ** -23


def _mat_vec_mul(A, b):
    return np.matmul(A, b[..., None])[..., 0]


def panorama_rays(pix_x_int, pix_y_int, pixtocams, camtoworlds):
    """pixtocams / camtoworlds broadcastable to the pixel shape + [3, 3] / [3, 4].  Float64 origins, directions, viewdirs,
    radii, imageplane."""
    def pix_to_dir(x, y):
        return np.stack([x + .5, y + .5, np.ones_like(x)], axis=-1)
    stacked = np.stack([pix_to_dir(pix_x_int, pix_y_int), pix_to_dir(pix_x_int + 1, pix_y_int),
                        pix_to_dir(pix_x_int, pix_y_int + 1)], axis=0)
    cam = _mat_vec_mul(pixtocams, stacked)
    cam = np.stack([np.sin(cam[..., 0]), cam[..., 1], np.cos(cam[..., 0])], axis=-1)
    cam = np.matmul(cam, np.diag(np.array([1., -1., -1.])))
    imageplane = cam[0, ..., :2]
    directions, dx, dy = _mat_vec_mul(camtoworlds[..., :3, :3], cam)
    origins = np.broadcast_to(camtoworlds[..., :3, -1], directions.shape)
    viewdirs = directions / np.linalg.norm(directions, axis=-1, keepdims=True)
    dx_norm = np.linalg.norm(dx - directions, axis=-1)
    dy_norm = np.linalg.norm(dy - directions, axis=-1)
    radii = (0.5 * (dx_norm + dy_norm))[..., None] * 2 / np.sqrt(12)
    return dict(origins=origins, directions=directions, viewdirs=viewdirs, radii=radii, imageplane=imageplane)


def panorama_batch(pix_x_int, pix_y_int, cam_idx, pixtocams, camtoworlds):
    """cast_ray_batch (:560-608) for stacked [N, 3, 3] / [N, 3, 4] cameras and an integer cam_idx of the pixels' shape, plus
    cam_dirs."""
    cam_idx = np.broadcast_to(cam_idx, pix_x_int.shape)
    out = panorama_rays(pix_x_int, pix_y_int, pixtocams[cam_idx], camtoworlds[cam_idx])
    out['cam_dirs'] = -camtoworlds[cam_idx][..., :3, 2]
    return out


def spherical_rays(camtoworld, height, width, near, far):
    """The reference's nine keys, float64, [height, width, k], plus cam_dirs (which the reference's spherical batch lacks)."""
    theta_vals = np.linspace(0, 2 * np.pi, width + 1)
    phi_vals = np.linspace(0, np.pi, height + 1)
    theta, phi = np.meshgrid(theta_vals, phi_vals, indexing='xy')
    directions = np.stack([-np.sin(phi) * np.sin(theta), np.cos(phi), np.sin(phi) * np.cos(theta)], axis=-1)
    directions = np.matmul(camtoworld[:3, :3], directions[..., None])[..., 0]
    dy = np.diff(directions[:, :-1], axis=0)
    dx = np.diff(directions[:-1, :], axis=1)
    directions = directions[:-1, :-1]
    origins = np.broadcast_to(camtoworld[:3, -1], directions.shape)
    dx_norm = np.linalg.norm(dx, axis=-1)
    dy_norm = np.linalg.norm(dy, axis=-1)
    radii = (0.5 * (dx_norm + dy_norm))[..., None] * 2 / np.sqrt(12)
    col = lambda v: np.broadcast_to(v, radii.shape[:-1])[..., None]
    return dict(origins=origins, directions=directions, viewdirs=directions, radii=radii,
                imageplane=np.zeros_like(directions[..., :2]), lossmult=col(1.), near=col(near), far=col(far), cam_idx=col(0),
                cam_dirs=np.broadcast_to(-camtoworld[:3, 2], directions.shape))


def within_bar(key, got, want):
    """The bar of the GPU tests: both sides compute in float64 and round once to float32, and the device's double sin / cos
    may differ from libm's in the last bits (OpenCL allows 4 ulp), so two results a few float64 ulps apart round to the same
    float32 or to neighbours.  Vector outputs: |got - want| <= 2^-23 * ||want|| per component, ||want|| the ray's vector norm
    (a component near zero carries the absolute error of the large ones); radii: |got - want| <= 2^-23 * want.  The
    neighbour differences behind the radii cancel, but even in the second row of a 900 x 8000 sphere the difference is
    ~2.7e-6 against ~1e-15 of error: 1e-9 relative, far below 2^-23, so no margin on top.  No element is excluded.
    Returns (all within, number of elements that differ at all, largest |got - want| / bar)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (key, got.shape, want.shape)
    bar = EPS * (np.abs(want) if key == 'radii' else np.broadcast_to(np.linalg.norm(want, axis=-1, keepdims=True), want.shape))
    diff = np.abs(got - want)
    ratio = float(np.max(diff / np.maximum(bar, 1e-300))) if diff.size else 0.0
    return bool(np.all(diff <= bar)), int(np.count_nonzero(got != want)), ratio
