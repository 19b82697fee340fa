"""Float64 numpy restatement of both branches of the reference's `Dataset._make_ray_batch` (datasets.py:386-476) and of
`generate_ray_batch` (:572-583) -- a test helper, the CPU reference the GPU tests use where the reference project itself is not
present, and the stand-in for the reference's worker-side cost in tools/time_train_batch.py.

`data` is a mapping with the attributes `_make_ray_batch` reads off the dataset:
  images [N,H,W,3], camtoworlds [M,3,4], pixtocams [M,3,3] (M >= N: the virtual cameras are appended, :867-870), near, far,
  optional disp_images / sky_segments / normal_images / alphas, and the switches virtual_poses, test_split, render_path,
  load_disps, load_normals, load_segs, camtype ('perspective' or 'panoroma').

Rays come from oracle/rays.py (perspective; bit-exact against the reference on tests/golden/rays.npz) and tests/rays_pano_ref.py
(panorama), the gathers and columns are the reference's numpy expressions, and the whole batch gets the `.float()` of :476.
tests/test_train_batch_cpu.py holds this to tests/golden/train_batch.npz bit for bit, key set and shapes included.
"""
import numpy as np

import rays_pano_ref
from oracle import rays as oracle_rays

RAY_KEYS = ('origins', 'directions', 'viewdirs', 'radii', 'imageplane', 'cam_dirs')
COLUMN_KEYS = ('lossmult', 'near', 'far')
PLANE_KEYS = ('rgb', 'disps', 'normals', 'alphas', 'sky_segs')
NONE_KEYS = ('exposure_idx', 'exposure_values')          # camera_utils.py:606-607: present in the dict, always None here


def bayer_mask(pix_x, pix_y):
    """raw_utils.py:38-46 pixels_to_bayer_mask."""
    r = (pix_x % 2 == 0) * (pix_y % 2 == 0)
    g = (pix_x % 2 == 1) * (pix_y % 2 == 0) + (pix_x % 2 == 0) * (pix_y % 2 == 1)
    b = (pix_x % 2 == 1) * (pix_y % 2 == 1)
    return np.stack([r, g, b], -1).astype(np.float32)


def _cast(data, pix_x, pix_y, cam_idx):
    """camera_utils.py:560-608 cast_ray_batch for stacked cameras; cam_idx has the pixels' shape."""
    p2c, c2w = np.asarray(data['pixtocams'], np.float64)[cam_idx], np.asarray(data['camtoworlds'], np.float64)[cam_idx]
    if data.get('camtype', 'perspective') == rays_pano_ref.PANORAMA:
        return rays_pano_ref.panorama_rays(pix_x, pix_y, p2c, c2w)
    rays = dict(zip(RAY_KEYS[:5], oracle_rays.pixels_to_rays(pix_x, pix_y, p2c, c2w)))
    # The sign of a zero: the reference flips OpenCV -> OpenGL by `matmul(dirs, diag(1, -1, -1))` (camera_utils.py:524), whose
    # last term is 1 * 0.0, so a pixel whose image-plane y is exactly 0 gets +0.0; the oracle (and the kernels) negate and get
    # -0.0.  Equal as numbers (np.array_equal, torch.equal); adding 0.0 restates the reference's bits and changes nothing else.
    rays['imageplane'] = rays['imageplane'] + 0.0
    return rays


def make_ray_batch(data, pix_x_int, pix_y_int, cam_idx, lossmult=None, cam_idx_with_src=None, cam_idx_with_ref=None,
                   pixel_x_int_with_src=None, pixel_y_int_with_src=None, pixel_x_int_with_ref=None, pixel_y_int_with_ref=None):
    """datasets.py:386-476.  Returns {key: float32 array | None}."""
    plain = not data.get('virtual_poses', False) or data.get('test_split', False)
    if plain:
        cast_x, cast_y, cast_cam = pix_x_int, pix_y_int, cam_idx
        look_x, look_y, look_cam = pix_x_int, pix_y_int, cam_idx
    else:
        cast_x, cast_y, cast_cam = pixel_x_int_with_src, pixel_y_int_with_src, cam_idx_with_src
        look_x, look_y, look_cam = pixel_x_int_with_ref, pixel_y_int_with_ref, cam_idx_with_ref
    cast_x, cast_y = np.asarray(cast_x), np.asarray(cast_y)
    broadcast_scalar = lambda x: np.broadcast_to(x, cast_x.shape)[..., None]          # :413 / :421
    ray_kwargs = dict(lossmult=broadcast_scalar(1.) if lossmult is None else lossmult, near=broadcast_scalar(data['near']),
                      far=broadcast_scalar(data['far']), cam_idx=broadcast_scalar(cast_cam))
    batch = _cast(data, cast_x, cast_y, ray_kwargs['cam_idx'][..., 0])
    batch.update(ray_kwargs)
    batch.update({k: None for k in NONE_KEYS})
    batch['cam_dirs'] = -np.asarray(data['camtoworlds'], np.float64)[ray_kwargs['cam_idx'][..., 0]][..., :3, 2]      # :446
    if not data.get('render_path', False):
        batch['rgb'] = data['images'][look_cam, look_y, look_x]
    if data.get('load_disps', False):
        batch['disps'] = data['disp_images'][look_cam, look_y, look_x]
    if data.get('load_normals', False):
        batch['normals'] = data['normal_images'][look_cam, look_y, look_x]
        batch['alphas'] = data['alphas'][look_cam, look_y, look_x]
    if data.get('load_segs', False):
        batch['sky_segs'] = data['sky_segments'][look_cam, look_y, look_x]
    if plain:
        batch['camera_id'] = ray_kwargs['cam_idx'][..., 0]                             # :456
    else:
        batch['camera_id'] = broadcast_scalar(look_cam)[..., 0]                        # :472
        batch['cam_idx'] = broadcast_scalar(look_cam)[..., 0]                          # :473, without the trailing axis
    return {k: np.ascontiguousarray(v).astype(np.float32) if v is not None else None for k, v in batch.items()}      # :476


def generate_ray_batch(data, cam_idx, width, height):
    """datasets.py:579-583: every pixel of frame `cam_idx` (the plain branch; pixel_coordinates is the 'xy' meshgrid)."""
    pix_x_int, pix_y_int = np.meshgrid(np.arange(width), np.arange(height), indexing='xy')
    return make_ray_batch(data, pix_x_int, pix_y_int, cam_idx)


def sampler_shapes(batch_size, world_size, patch_size, border, width, height, virtual_poses):
    """The host-side arithmetic of `_next_train` (:277-279, :483-494): patches per batch, how many of them the virtual branch
    adds, and the half-open ranges the patch origins are drawn from."""
    patch = max(patch_size, 1)
    per_process = batch_size // world_size
    num_patches = per_process // patch ** 2
    lower, upper = border, border + patch - 1
    return dict(patch_size=patch, num_patches=num_patches, num_patches_for_virtual=int(0.2 * num_patches) if virtual_poses else 0,
                x_range=(lower, width - upper), y_range=(lower, height - upper))
