"""Golden vectors for the device batch assembler (ucnerf_amd/internal/datasets.py) from the reference's own datasets.py.

Runs ONLY in the authoring container (imports the reference read-only through ref_import's stubs, plus `internal.datasets`,
which ref_import itself does not load):
    python tests/golden/make_train_batch_golden.py          -> tests/golden/train_batch.npz
A subclass of the reference's `Dataset` whose `_load_renderings` fills synthetic arrays stands in for the loaders (which read
nuScenes / Waymo from disk): 3 real + 2 virtual cameras, 12 x 16 float32 images with non-integer values, a depth plane and a
sky-segment plane.  The outputs are what `Dataset._make_ray_batch` / `generate_ray_batch` return (datasets.py:386-476, :572-583),
i.e. after the `.float()` of :476; the inputs are recorded beside them.

  a.*   the plain branch, 37 rays in shape [37, 1, 1] with per-ray cameras
  b.*   the plain branch with patch_size = 2: [9, 2, 2] pixels, [9, 1, 1] cameras
  c.*   the virtual branch (config.virtual_poses, train split): 37 + 7 rays, distinct cast (`*_with_src`) and look-up
        (`*_with_ref`) triples; the 7 virtual rays are cast through cameras 3 and 4
  d.*   generate_ray_batch(1): the whole 12 x 16 frame of camera 1
  e.*   case a at 257 rays (more than one 256-thread block)
`X.keys` is the JSON list of the returned dict's keys in order, `X.none` of those whose value is None (camera_utils.py:606-607).
`meta` says how the file was made.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
from make_rays_golden import rotation  # noqa: E402

N_REAL, N_VIRTUAL, H, W = 3, 2, 12, 16
NEAR, FAR = 0.25, 8.0
INDEX_ARGS = ('pix_x_int', 'pix_y_int', 'cam_idx', 'cam_idx_with_src', 'cam_idx_with_ref', 'pixel_x_int_with_src',
              'pixel_y_int_with_src', 'pixel_x_int_with_ref', 'pixel_y_int_with_ref')


def synthetic_scene(rng):
    n = N_REAL + N_VIRTUAL
    intr = np.stack([np.array([[17.0 + 0.75 * i, 0.0, 7.6 + 0.1 * i], [0.0, 16.5 + 0.5 * i, 5.7 - 0.1 * i], [0.0, 0.0, 1.0]])
                     for i in range(n)])
    return dict(
        images=rng.random((N_REAL, H, W, 3)).astype(np.float32),
        disp_images=(rng.random((N_REAL, H, W)) * 3.0 + 0.5).astype(np.float32),
        sky_segments=(rng.random((N_REAL, H, W)) < 0.3).astype(np.float32),
        pixtocams=np.array([np.linalg.inv(k) for k in intr]),                      # datasets.py:855
        camtoworlds=np.concatenate([np.stack([rotation(rng) for _ in range(n)]), rng.standard_normal((n, 3, 1)) * 0.5], axis=-1))


def main():
    ref_import.load()
    cwd = os.getcwd()
    os.chdir(ref_import.REF)
    try:
        from internal import datasets, utils                   # beyond ref_import.load(): the module under restatement
    finally:
        os.chdir(cwd)
    ref = ref_import.load()
    rng = np.random.default_rng(41)
    scene = synthetic_scene(rng)

    class Synthetic(datasets.Dataset):
        def _load_renderings(self, config):
            self.images, self.disp_images, self.sky_segments = scene['images'], scene['disp_images'], scene['sky_segments']
            self.n_examples = len(self.images)
            self.height, self.width = H, W
            self.cam_num = 1
            if config.virtual_poses and self.split == utils.DataSplit.TRAIN:          # :867-870
                self.camtoworlds, self.pixtocams = scene['camtoworlds'], scene['pixtocams']
                self.virtual_poses = scene['camtoworlds'][N_REAL:]
            else:
                self.camtoworlds, self.pixtocams = scene['camtoworlds'][:N_REAL], scene['pixtocams'][:N_REAL]

    def dataset(split='train', **kw):
        cfg = ref.configs.Config()
        cfg.world_size, cfg.global_rank = 1, 0                                        # datasets.py:1148-1149
        cfg.near, cfg.far, cfg.batch_size = NEAR, FAR, 64
        cfg.compute_disp_metrics, cfg.load_sky_segments, cfg.compute_normal_metrics = True, True, False
        for k, v in kw.items():
            setattr(cfg, k, v)
        return Synthetic(split, '', cfg)

    out = {f'scene.{k}': v for k, v in scene.items()}
    out.update({'scene.near': NEAR, 'scene.far': FAR, 'scene.n_real': N_REAL, 'scene.height': H, 'scene.width': W})

    def record(tag, batch, **inputs):
        for k, v in inputs.items():
            out[f'{tag}.in.{k}'] = np.asarray(v).astype(np.int32)
        out[f'{tag}.keys'] = np.array(json.dumps(list(batch)))
        out[f'{tag}.none'] = np.array(json.dumps([k for k, v in batch.items() if v is None]))
        for k, v in batch.items():
            if v is not None:
                assert v.dtype.is_floating_point and str(v.dtype) == 'torch.float32', (tag, k, v.dtype)
                out[f'{tag}.out.{k}'] = v.numpy()

    def plain(tag, ds, n, patch=1):
        px = rng.integers(0, W - patch + 1, size=(n, 1, 1))
        py = rng.integers(0, H - patch + 1, size=(n, 1, 1))
        px[:4, 0, 0], py[:4, 0, 0] = [0, W - patch, 0, W - patch], [0, 0, H - patch, H - patch]      # the frame's corners
        dx, dy = ref_camera_utils.pixel_coordinates(patch, patch)                     # datasets.py:497-500
        px, py = px + dx, py + dy
        ci = rng.integers(0, N_REAL, size=(n, 1, 1))
        record(tag, ds._make_ray_batch(px, py, ci), pix_x_int=px, pix_y_int=py, cam_idx=ci)

    from internal import camera_utils as ref_camera_utils
    real = dataset()
    plain('a', real, 37)
    plain('b', dataset(patch_size=2), 9, patch=2)
    plain('e', real, 257)
    record('d', real.generate_ray_batch(1), cam_idx=1)

    # (c) the virtual branch with the argument layout of _next_train (:550-555), incl. its (x, x) cast pixels of the real rays
    n, v = 37, 7
    px, py = rng.integers(0, W, size=(n, 1, 1)), rng.integers(0, H, size=(n, 1, 1))
    ci = rng.integers(0, N_REAL, size=(n, 1, 1))
    src_cam = rng.integers(N_REAL, N_REAL + N_VIRTUAL, size=(v, 1, 1))
    ref_cam = rng.integers(0, N_REAL, size=(v, 1, 1))
    src_x, src_y = rng.integers(0, W, size=(v, 1, 1)), rng.integers(0, H, size=(v, 1, 1))
    ref_x, ref_y = rng.integers(0, W, size=(v, 1, 1)), rng.integers(0, H, size=(v, 1, 1))
    cat = lambda a, b: np.concatenate((a, b), axis=0)
    args = dict(cam_idx_with_src=cat(ci, src_cam), cam_idx_with_ref=cat(ci, ref_cam),
                pixel_x_int_with_src=cat(px, src_x), pixel_y_int_with_src=cat(px, src_y),                # :553 concatenates pix_x_int
                pixel_x_int_with_ref=cat(px, ref_x), pixel_y_int_with_ref=cat(py, ref_y))
    virtual = dataset(virtual_poses=True)
    assert virtual.size == N_REAL and virtual.camtoworlds.shape[0] == N_REAL + N_VIRTUAL
    record('c', virtual._make_ray_batch(px, py, ci, **args), pix_x_int=px, pix_y_int=py, cam_idx=ci, **args)

    out['meta'] = np.array(json.dumps(dict(
        source='the reference Dataset._make_ray_batch / generate_ray_batch, imported with stubs (datasets.py:386-476, 572-583)',
        generator='tests/golden/make_train_batch_golden.py', numpy=np.__version__, seed=41)))
    path = os.path.join(HERE, 'train_batch.npz')
    np.savez_compressed(path, **out)
    print(f'train_batch.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays')


if __name__ == '__main__':
    main()
