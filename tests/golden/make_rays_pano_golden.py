"""Golden vectors for the panorama and spherical camera models from the reference's own camera_utils.py.

Runs ONLY in the authoring container (imports the reference read-only through ref_import's stubs):
    python tests/golden/make_rays_pano_golden.py          -> tests/golden/rays_pano.npz
Outputs are what the model would see: the float64 results of camera_utils.cast_ray_batch(..., 'panoroma') (+ the cam_dirs of
datasets.py:446) and of camera_utils.cast_spherical_rays, cast with `.float()` (datasets.py:476), plus the inputs.

  pano_frame.*   every pixel of a 64 x 12 frame for two cameras [2, 12, 64, k]: focal lengths 16 / 14.5 with the principal point
                 off centre, so x / f runs from about -1.8 to 2.2 (2.4): past +-pi/2 on both sides, cos changes sign and the rays
                 behind the image plane are covered
  pano_batch.*   a [B, 1] pixel batch with per-ray cam_idx from the 8000 x 900 frame of the nuScenes render path
                 (datasets.py:872-878), f = 1266.417; contains columns 0, 1, 3999, 4000, 7999 and rows 0, 899
  sph_6x16.*, sph_5x7.*   whole spherical frames
  sph_big.*      the 900 x 8000 spherical frame computed in full, stored at rows {0, 1, 449, 450, 898, 899} x 64 spread
                 columns (0 and 7999 among them): [6, 64, k]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
from make_rays_golden import rotation  # noqa: E402

RAY_KEYS = ('origins', 'directions', 'viewdirs', 'radii', 'imageplane')
BIG_ROWS = (0, 1, 449, 450, 898, 899)


def main():
    ref_import.load()
    cwd = os.getcwd()
    os.chdir(ref_import.REF)
    try:
        from internal import camera_utils
    finally:
        os.chdir(cwd)
    rng = np.random.default_rng(23)
    out = {}
    f32 = lambda a: np.ascontiguousarray(np.asarray(a).astype(np.float32))        # datasets.py:476 `.float()`

    def pose(n):
        return np.concatenate([np.stack([rotation(rng) for _ in range(n)]), rng.standard_normal((n, 3, 1)) * 0.5], axis=-1)

    def cast(tag, px, py, ci, pixtocams, camtoworlds):
        b = lambda v: np.broadcast_to(v, px.shape)[..., None]
        pixels = dict(pix_x_int=px, pix_y_int=py, lossmult=b(1.), near=b(0.), far=b(8.), cam_idx=b(ci))
        batch = camera_utils.cast_ray_batch((pixtocams, camtoworlds, None, None), pixels, 'panoroma')
        batch['cam_dirs'] = -camtoworlds[pixels['cam_idx'][..., 0]][..., :3, 2]   # datasets.py:446
        return {k: f32(batch[k]) for k in RAY_KEYS + ('cam_dirs',)}

    # (a) two small full frames
    W, H = 64, 12
    intr = np.stack([np.array([[f, 0.0, 29.3], [0.0, f, 5.1], [0.0, 0.0, 1.0]]) for f in (16.0, 14.5)])
    p2c, c2w = np.array([np.linalg.inv(k) for k in intr]), pose(2)
    px, py = camera_utils.pixel_coordinates(W, H)
    frames = [cast('pano_frame', px, py, c, p2c, c2w) for c in range(2)]
    out.update({'pano_frame.pixtocams': p2c, 'pano_frame.camtoworlds': c2w, 'pano_frame.width': W, 'pano_frame.height': H})
    out.update({f'pano_frame.{k}': np.stack([fr[k] for fr in frames]) for k in frames[0]})

    # (b) a pixel batch of the nuScenes render frame
    W, H, n_cam, B = 8000, 900, 3, 512
    intr = np.stack([np.array([[1266.417203, 0.0, 4000.2 + 1.5 * i], [0.0, 1266.417203, 449.7 - i], [0.0, 0.0, 1.0]])
                     for i in range(n_cam)])
    p2c, c2w = np.array([np.linalg.inv(k) for k in intr]), pose(n_cam)
    px, py = rng.integers(0, W, size=(B, 1)), rng.integers(0, H, size=(B, 1))
    px[:5, 0], py[:5, 0] = [0, 1, 3999, 4000, 7999], [0, 899, 450, 0, 899]
    ci = rng.integers(0, n_cam, size=(B, 1))
    out.update({'pano_batch.pixtocams': p2c, 'pano_batch.camtoworlds': c2w, 'pano_batch.width': W, 'pano_batch.height': H,
                'pano_batch.pix_x': px.astype(np.int32), 'pano_batch.pix_y': py.astype(np.int32),
                'pano_batch.cam_idx': ci.astype(np.int32)})
    out.update({f'pano_batch.{k}': v for k, v in cast('pano_batch', px, py, ci, p2c, c2w).items()})

    # (c) spherical frames
    def sphere(tag, H, W, near, far, rows=None, cols=None):
        c2w = pose(1)[0]
        b = camera_utils.cast_spherical_rays(c2w, H, W, near, far)
        out.update({f'{tag}.camtoworld': c2w, f'{tag}.height': H, f'{tag}.width': W, f'{tag}.near': near, f'{tag}.far': far,
                    f'{tag}.cam_dirs': f32(-c2w[:3, 2])})                         # datasets.py:446
        for k in RAY_KEYS + ('lossmult', 'near', 'far', 'cam_idx'):
            v = np.asarray(b[k])
            assert v.shape[:2] == (H, W), (k, v.shape)
            out[f'{tag}.{k}' if k not in ('near', 'far') else f'{tag}.{k}_col'] = f32(v if rows is None else v[np.ix_(rows, cols)])
    sphere('sph_6x16', 6, 16, 0.25, 8.0)
    sphere('sph_5x7', 5, 7, 0.5, 100.0)
    rows, cols = np.array(BIG_ROWS), np.round(np.linspace(0, 7999, 64)).astype(np.int64)
    assert cols[0] == 0 and cols[-1] == 7999 and len(set(cols)) == 64
    out['sph_big.rows'], out['sph_big.cols'] = rows.astype(np.int32), cols.astype(np.int32)
    sphere('sph_big', 900, 8000, 0.1, 1e6, rows, cols)

    path = os.path.join(HERE, 'rays_pano.npz')
    np.savez_compressed(path, **out)
    print(f'rays_pano.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays')


if __name__ == '__main__':
    main()
