"""Training and test batches assembled on the device from a resident dataset (SURVEY.md 8 f1 + f3).

ref internal/datasets.py:213-593 (`Dataset`): `_make_ray_batch` (:386-476), `_next_train` (:478-570),
`generate_ray_batch` (:572-583) and the DataLoader surface (`size`, `__len__`, `__getitem__`, `collate_fn`, :357-365, :585-593).
The reference runs these in numpy on DataLoader workers: it draws pixels, casts rays in float64, fancy-indexes the image arrays,
warps a whole depth map on the CPU when `config.virtual_poses` is on, converts every key to float32 and ships the batch across
PCIe.  `DeviceDataset` uploads the arrays once and produces the same batch with one launch of `ucn_train_batch`
(csrc/batch.hip): rays, gathered planes and the broadcast columns, one thread per ray.  Same key set and shapes in both
branches of `_make_ray_batch`; every tensor is float32 on the device.  The perspective batch is bit-identical to the
reference's on the same indices; the panorama model's rays are within one float32 unit of the ray's vector norm (device
sin / cos, see camera_utils.py), its gathered planes bit-identical.

What differs from upstream, on purpose:
  * the random stream: the draws are torch's, on the device, not `np.random`'s, so a batch equals the reference's on the same
    indices (`make_ray_batch`), never draw for draw;
  * `num_workers` must be 0: a forked DataLoader worker must not touch the GPU, and `__getitem__` / `collate_fn` refuse to run
    in one;
  * `next_train(max_virtual_tries=64)` raises RuntimeError after that many warps where the reference's virtual-pose selection loop (:509-529) spins
    forever on a dataset whose warps never keep enough pixels;
  * `next_train(fix_src_rows=True)` repairs datasets.py:553, see there.
No CPU path: host tensors for pixel indices raise like every other entry point.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from . import camera_utils, train_utils

ALL_IMAGES, SINGLE_IMAGE = 'all_images', 'single_image'          # utils.py:65-68 BatchingMethod
VIRTUAL_CASE = 9                                                 # datasets.py:508: virtual poses per real image
MAX_PLANES = _lib.BATCH_MAX_PLANES


def _require_main_process(what):
    """A DataLoader worker is a forked process: the HIP runtime of the parent is not usable there."""
    if torch.utils.data.get_worker_info() is not None:
        raise RuntimeError(f"DeviceDataset.{what} called in a DataLoader worker process: the batches are made on the GPU, "
                           "build the DataLoader with num_workers=0")


def camtype_value(camtype):
    """An enum member's value, anything else as it is.  The reference's `Dataset.camtype` is a member of ITS `ProjectionType`
    (datasets.py:306), which equals neither this package's member nor the string; its value 'perspective' is what
    `camera_utils._check_supported` knows.  'panoroma' is a plain string upstream (datasets.py:878)."""
    return getattr(camtype, 'value', camtype)


def _device_index(t, what, device):
    """An index argument as a device tensor: tensors must already be there, Python / numpy scalars are uploaded."""
    if torch.is_tensor(t):
        _lib.require_device(t, what)
        return t
    if np.ndim(t) != 0:
        raise RuntimeError(f"{what} must be a CUDA tensor")     # an array of indices on the host: no CPU path
    return torch.tensor(int(t), device=device, dtype=torch.int32)


def _flat_i32(t, shape):
    return t.expand(shape).to(torch.int32).reshape(-1).contiguous()


def sampler_shapes(batch_size, world_size, patch_size, border, width, height, virtual_poses):
    """The host-side arithmetic of `_next_train` (:277-279, :483-494): patches per batch, how many of them the virtual branch
    appends, and the half-open ranges the patch origins are drawn from."""
    patch = max(int(patch_size), 1)
    per_process = int(batch_size) // int(world_size)
    if patch ** 2 > per_process:
        raise ValueError(f'Patch size {patch}^2 too large for per-process batch size {per_process}')      # :279-281
    num_patches = per_process // patch ** 2
    lower, upper = int(border), int(border) + patch - 1
    return dict(patch_size=patch, num_patches=num_patches, num_patches_for_virtual=int(0.2 * num_patches) if virtual_poses else 0,
                x_range=(lower, int(width) - upper), y_range=(lower, int(height) - upper))


class DeviceDataset(torch.utils.data.Dataset):
    """The reference's `Dataset` with its arrays resident on the device.

    images [N, H, W, 3]; camtoworlds [M, 3|4, 4] and pixtocams [M, 3, 3] (or one [3, 3]), M >= N because the reference appends
    the virtual cameras (:867-870); optional disp_images [N, H, W] or [N, H, W, 1], sky_segments, normal_images + alphas;
    virtual_poses [N * 9, 4, 4] and cam_num for the virtual branch.  Planes are uploaded as float32 (what the reference's final
    `.float()` makes of them), the camera tables as float64.  The keywords after `camtype` are the config fields `_next_train`
    and `_make_ray_batch` read, with the reference's names and defaults.  `width` / `height` default to the images'."""

    def __init__(self, images, camtoworlds, pixtocams, near, far, disp_images=None, sky_segments=None, normal_images=None,
                 alphas=None, virtual_poses=None, cam_num=None, camtype=camera_utils.ProjectionType.PERSPECTIVE, split='train',
                 width=None, height=None, batch_size=2 ** 16, world_size=1, patch_size=1, batching=ALL_IMAGES,
                 num_border_pixels_to_mask=0, apply_bayer_mask=False, virtual_poses_enabled=None, compute_disp_metrics=False,
                 compute_normal_metrics=False, load_sky_segments=True, render_path=False, render_spherical=False,
                 compute_visibility=False, device='cuda', seed=None):
        super().__init__()
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError("DeviceDataset: device must be a CUDA device (there is no CPU path)")
        self.camtype = camtype_value(camtype)
        self._model = camera_utils._check_supported(None, None, self.camtype)
        self.split = getattr(split, 'value', split)
        if self.split not in ('train', 'test'):
            raise ValueError(f"split {split!r}: 'train' or 'test'")
        self.virtual_poses_enabled = bool(virtual_poses is not None if virtual_poses_enabled is None else virtual_poses_enabled)
        self.near, self.far = float(near), float(far)
        self.render_path, self._render_spherical = bool(render_path), bool(render_spherical)
        self.compute_visibility = bool(compute_visibility)
        self._load_disps, self._load_normals = bool(compute_disp_metrics), bool(compute_normal_metrics)
        self._load_segs = bool(load_sky_segments)
        self._apply_bayer_mask = bool(apply_bayer_mask)
        self._batching = getattr(batching, 'value', batching)
        if self._batching not in (ALL_IMAGES, SINGLE_IMAGE):
            raise ValueError(f"batching {batching!r}: {ALL_IMAGES!r} or {SINGLE_IMAGE!r}")

        def plane(a, what):
            if a is None:
                return None
            t = torch.as_tensor(a)
            if t.dim() not in (3, 4) or (t.dim() == 4 and not 1 <= t.shape[3] <= 4):
                raise RuntimeError(f"{what} must be [N, H, W] or [N, H, W, 1..4], got {tuple(t.shape)}")
            return t.to(device=self.device, dtype=torch.float32).contiguous()
        self.images = plane(images, "images")
        self.disp_images, self.sky_segments = plane(disp_images, "disp_images"), plane(sky_segments, "sky_segments")
        self.normal_images, self.alphas = plane(normal_images, "normal_images"), plane(alphas, "alphas")
        if self.images is None or self.images.dim() != 4:
            raise RuntimeError("images must be [N, H, W, C]")
        for name, need in (("disp_images", self._load_disps), ("sky_segments", self._load_segs),
                           ("normal_images", self._load_normals), ("alphas", self._load_normals)):
            t = getattr(self, name)
            if need and t is None:
                raise RuntimeError(f"{name} is None but the configuration loads it")
            if t is not None and t.shape[:3] != self.images.shape[:3]:
                raise RuntimeError(f"{name} {tuple(t.shape)} does not match images {tuple(self.images.shape)}")
        self._plane_hw = (int(self.images.shape[1]), int(self.images.shape[2]))
        self.height = int(self._plane_hw[0] if height is None else height)
        self.width = int(self._plane_hw[1] if width is None else width)

        p2c = camera_utils._cam_table(pixtocams, 3, self.device, "pixtocams")
        c2w = camera_utils._cam_table(camtoworlds, 4, self.device, "camtoworlds")
        m = max(p2c.shape[0], c2w.shape[0])
        if 1 not in (p2c.shape[0], c2w.shape[0]) and p2c.shape[0] != c2w.shape[0]:
            raise RuntimeError("pixtocams and camtoworlds must hold one camera or as many as each other")
        self.pixtocams, self.camtoworlds = p2c.expand(m, 3, 3).contiguous(), c2w.expand(m, 3, 4).contiguous()
        # host copies of the camera tables for the scalar work of the virtual-pose loop (a pose and an intrinsic per attempt)
        self._c2w_host, self._p2c_host = self.camtoworlds.cpu().numpy(), self.pixtocams.cpu().numpy()
        self.cam_num = None if cam_num is None else int(cam_num)
        self._virtual_host = None
        if virtual_poses is not None:
            self._virtual_host = np.asarray(torch.as_tensor(virtual_poses).cpu().numpy(), np.float64)[..., :3, :]
        if self.virtual_poses_enabled and self.split == 'train':
            self._n_examples = int(self.images.shape[0])                                  # :341-342
        else:
            self._n_examples = m                                                          # :344
        self._shapes = sampler_shapes(batch_size, world_size, patch_size, num_border_pixels_to_mask, self.width, self.height,
                                      self.virtual_poses_enabled)
        self._patch_size = self._shapes['patch_size']
        self._status = torch.zeros(2, dtype=torch.int32, device=self.device)
        # seed=None: torch's global seed, i.e. what torch.manual_seed / accelerate's set_seed(seed, device_specific=True)
        # (train.py:67) gave this process, so the ranks of a world_size > 1 run draw different batches.  A fresh
        # torch.Generator() would start from the same fixed default seed in every process and every run.
        self._host_generator = torch.Generator()
        self._host_generator.manual_seed(torch.initial_seed() if seed is None else int(seed))
        self._device_generator = torch.Generator(device=self.device)
        self._train_route = self.split == 'train' and not self.compute_visibility        # :352-355, which `_next_fn`

    @classmethod
    def from_dataset(cls, ds, device='cuda', seed=None):
        """The one-line binding: the same attributes off an instance of the reference's `Dataset` (after its `__init__`).
        seed=None takes torch's global seed of this process (see `__init__`)."""
        if getattr(ds, 'distortion_params', None) is not None or getattr(ds, 'pixtocam_ndc', None) is not None:
            camera_utils._check_supported(ds.distortion_params, ds.pixtocam_ndc, camtype_value(ds.camtype))
        cfg = ds.config
        return cls(ds.images, ds.camtoworlds, ds.pixtocams, ds.near, ds.far, disp_images=getattr(ds, 'disp_images', None),
                   sky_segments=getattr(ds, 'sky_segments', None), normal_images=getattr(ds, 'normal_images', None),
                   alphas=getattr(ds, 'alphas', None), virtual_poses=getattr(ds, 'virtual_poses', None),
                   cam_num=getattr(ds, 'cam_num', None), camtype=ds.camtype, split=ds.split, width=ds.width, height=ds.height,
                   batch_size=cfg.batch_size, world_size=cfg.world_size, patch_size=cfg.patch_size, batching=cfg.batching,
                   num_border_pixels_to_mask=cfg.num_border_pixels_to_mask, apply_bayer_mask=cfg.apply_bayer_mask,
                   virtual_poses_enabled=cfg.virtual_poses, compute_disp_metrics=cfg.compute_disp_metrics,
                   compute_normal_metrics=cfg.compute_normal_metrics, load_sky_segments=cfg.load_sky_segments,
                   render_path=ds.render_path, render_spherical=getattr(ds, '_render_spherical', False),
                   compute_visibility=getattr(cfg, 'compute_visibility', False), device=device, seed=seed)

    # ------------------------------------------------------------------ the DataLoader surface (:357-365, :585-593)
    @property
    def size(self):
        return self._n_examples

    def __len__(self):
        return 1000 if self.split == 'train' and not self.compute_visibility else self._n_examples

    def _next_test(self, item):
        """:585-587: one full frame and its index."""
        return self.generate_ray_batch(int(item)), torch.tensor(int(item))

    def _next(self, item):
        return self.next_train() if self._train_route else self._next_test(item)

    def collate_fn(self, item):
        """`DataLoader(np.arange(len(ds)), num_workers=0, batch_size=1, collate_fn=ds.collate_fn)` as train.py:75-87 writes it;
        num_workers must be 0."""
        _require_main_process("collate_fn")
        return self._next(item[0])

    def __getitem__(self, item):
        _require_main_process("__getitem__")
        return self._next(item)

    # ------------------------------------------------------------------ _make_ray_batch (:386-476)
    def _planes(self):
        """(key, array) of what `_make_ray_batch` gathers, in its order (:447-455 / :463-471)."""
        out = []
        if not self.render_path:
            out.append(('rgb', self.images))
        if self._load_disps:
            out.append(('disps', self.disp_images))
        if self._load_normals:
            out += [('normals', self.normal_images), ('alphas', self.alphas)]
        if self._load_segs:
            out.append(('sky_segs', self.sky_segments))
        if len(out) > MAX_PLANES:
            raise NotImplementedError(f"{len(out)} image planes in one batch; ucn_train_batch gathers at most {MAX_PLANES} (no "
                                      "UC-NeRF loader fills normal_images)")
        return out

    def _assemble(self, shape, cast, look, cam_scalar, lossmult, bayer, validate):
        """One launch of ucn_train_batch.  cast / look = (cam, x, y) flat int32 device tensors or None; returns the reference's
        dict in the reference's key order, every ray key shaped `shape + [k]`."""
        lib = _lib.load()
        dev = self.device
        n = 1
        for s in shape:
            n *= int(s)
        if n >= 1 << 32:
            raise RuntimeError(f"{n} rays do not fit a 32-bit ray index")
        f32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        rays = dict(origins=f32(n, 3), directions=f32(n, 3), viewdirs=f32(n, 3), radii=f32(n, 1), imageplane=f32(n, 2))
        lm_in, lm_ch = None, 1
        if lossmult is not None:
            lm_ch = int(lossmult.shape[-1])
            lm_in = lossmult.to(torch.float32).expand(tuple(shape) + (lm_ch,)).reshape(n, lm_ch).contiguous()
        cols = dict(lossmult=f32(n, 3 if bayer else lm_ch), near=f32(n, 1), far=f32(n, 1), cam_idx=f32(n, 1))
        cam_dirs = f32(n, 3)
        planes = self._planes()
        gathered = [f32(n, 1 if a.dim() == 3 else a.shape[3]) for _, a in planes]
        count = len(planes)
        src = (ctypes.c_void_p * max(count, 1))(*[a.data_ptr() for _, a in planes])
        dst = (ctypes.c_void_p * max(count, 1))(*[g.data_ptr() for g in gathered])
        channels = (ctypes.c_uint32 * max(count, 1))(*[g.shape[1] for g in gathered])
        if validate:
            self._status.zero_()
        cast = cast or (None, None, None)
        look = look or (None, None, None)
        H, W = self._plane_hw if cast[1] is not None else (self.height, self.width)
        _lib.check(lib.ucn_train_batch(
            _lib.ptr(cast[0]), int(cam_scalar), _lib.ptr(cast[1]), _lib.ptr(cast[2]), _lib.ptr(look[0]), _lib.ptr(look[1]),
            _lib.ptr(look[2]), self.pixtocams.data_ptr(), self.camtoworlds.data_ptr(), self.pixtocams.shape[0],
            self.images.shape[0], H, W, n, ctypes.addressof(src), ctypes.addressof(dst), ctypes.addressof(channels), count,
            self.near, self.far, _lib.ptr(lm_in), lm_ch, _lib.BATCH_BAYER_MASK if bayer else 0, rays['origins'].data_ptr(),
            rays['directions'].data_ptr(), rays['viewdirs'].data_ptr(), rays['radii'].data_ptr(), rays['imageplane'].data_ptr(),
            cam_dirs.data_ptr(), cols['near'].data_ptr(), cols['far'].data_ptr(), cols['lossmult'].data_ptr(),
            cols['cam_idx'].data_ptr(), self._status.data_ptr() if validate else None, self._model, _lib.stream()))
        if validate:
            bad_look, bad_cam = self._status.tolist()                  # the one sync of validate=True
            if bad_cam:
                raise IndexError(f"make_ray_batch: a camera index is outside [0, {self.pixtocams.shape[0]})")
            if bad_look:
                raise IndexError(f"make_ray_batch: an image look-up is outside [0, {self.images.shape[0]}) x [0, "
                                 f"{self._plane_hw[0]}) x [0, {self._plane_hw[1]})")
        shape = tuple(shape)
        batch = {k: v.reshape(shape + (v.shape[1],)) for k, v in rays.items()}
        batch.update({k: v.reshape(shape + (v.shape[1],)) for k, v in cols.items()})
        batch.update(exposure_idx=None, exposure_values=None)          # camera_utils.py:606-607
        batch['cam_dirs'] = cam_dirs.reshape(shape + (3,))
        for (key, a), g in zip(planes, gathered):
            batch[key] = g.reshape(shape + tuple(a.shape[3:]))
        return batch

    def make_ray_batch(self, pix_x_int, pix_y_int, cam_idx, lossmult=None, cam_idx_with_src=None, cam_idx_with_ref=None,
                       pixel_x_int_with_src=None, pixel_y_int_with_src=None, pixel_x_int_with_ref=None,
                       pixel_y_int_with_ref=None, validate=True):
        """datasets.py:386-476 with its arguments, key set and shapes.  Integer device tensors of broadcastable shapes (`cam_idx`
        may be a Python int); the result's ray keys are shaped `pixels' shape + [k]`, float32, on the device.

        Without `virtual_poses`, or on the test split, rays are cast through and planes gathered at (cam_idx, pix_y, pix_x).
        With it (train split) the `*_with_src` triple casts the rays and the `*_with_ref` triple gathers the planes (:457-473),
        and, as there, `cam_idx` is overwritten by the reference camera WITHOUT the trailing axis and `camera_id` is the
        reference camera too.  `rgb` is absent under `render_path`; `exposure_idx` / `exposure_values` are None.

        validate=True reads the kernel's status word (one device sync) and raises IndexError if a look-up left the arrays or
        a camera index left the tables; with validate=False those rays' planes (rays) are NaN and nothing syncs."""
        plain = not self.virtual_poses_enabled or self.split == 'test'
        if plain:
            xs, ys, cams = (pix_x_int, "pix_x_int"), (pix_y_int, "pix_y_int"), (cam_idx, "cam_idx")
        else:
            xs, ys = (pixel_x_int_with_src, "pixel_x_int_with_src"), (pixel_y_int_with_src, "pixel_y_int_with_src")
            cams = (cam_idx_with_src, "cam_idx_with_src")
        for t, what in (xs, ys):
            if not torch.is_tensor(t):
                raise RuntimeError(f"{what} must be a CUDA tensor")
            _lib.require_device(t, what)
        x, y, cam = xs[0], ys[0], _device_index(cams[0], cams[1], xs[0].device)
        shape = torch.broadcast_shapes(x.shape, y.shape)
        if torch.broadcast_shapes(shape, cam.shape) != shape:
            raise RuntimeError(f"{cams[1]} {tuple(cam.shape)} does not broadcast to the pixels' shape {tuple(shape)}")
        if lossmult is not None:
            _lib.require_device(lossmult, "lossmult")
            if lossmult.dim() != len(shape) + 1 or not 1 <= lossmult.shape[-1] <= 4:
                raise RuntimeError(f"lossmult must be the pixels' shape + [1..4], got {tuple(lossmult.shape)}")
        cast = (_flat_i32(cam, shape), _flat_i32(x, shape), _flat_i32(y, shape))
        if plain:
            batch = self._assemble(shape, cast, None, 0, lossmult, False, validate)
            batch['camera_id'] = batch['cam_idx'][..., 0]                                  # :456
            return batch
        look = []
        for t, what in ((cam_idx_with_ref, "cam_idx_with_ref"), (pixel_x_int_with_ref, "pixel_x_int_with_ref"),
                        (pixel_y_int_with_ref, "pixel_y_int_with_ref")):
            t = _device_index(t, what, x.device)
            if torch.broadcast_shapes(shape, t.shape) != shape:
                raise RuntimeError(f"{what} {tuple(t.shape)} does not broadcast to the cast pixels' shape {tuple(shape)}")
            look.append(_flat_i32(t, shape))
        batch = self._assemble(shape, cast, tuple(look), 0, lossmult, False, validate)
        ref_cam = look[0].to(torch.float32).reshape(tuple(shape))
        batch['camera_id'] = ref_cam                                                       # :472
        batch['cam_idx'] = ref_cam                                                         # :473
        return batch

    # ------------------------------------------------------------------ generate_ray_batch (:572-583)
    def generate_ray_batch(self, cam_idx):
        """Every pixel of frame `cam_idx` with `rgb` and the optional planes, [height, width, k]; a spherical frame
        (`render_camtype == 'pano'`) is `camera_utils.cast_spherical_rays`, as in the reference.  The pixel grid is not
        materialised: the kernel derives (x, y) from the ray index."""
        cam_idx = int(cam_idx)
        if self._render_spherical:
            return camera_utils.cast_spherical_rays(self.camtoworlds[cam_idx], self.height, self.width, self.near, self.far,
                                                    device=self.device)
        if self.virtual_poses_enabled and self.split == 'train':
            raise RuntimeError("generate_ray_batch on a virtual-pose training set: the reference's _make_ray_batch takes its "
                               "virtual branch there and fails on the missing *_with_src arguments (datasets.py:421)")
        if not 0 <= cam_idx < self.pixtocams.shape[0]:
            raise IndexError(f"generate_ray_batch: camera {cam_idx} outside [0, {self.pixtocams.shape[0]})")
        shape = (self.height, self.width)
        planes = self._planes()
        if planes and (shape != self._plane_hw or cam_idx >= self.images.shape[0]):
            raise IndexError(f"generate_ray_batch: frame {cam_idx} of {shape[0]} x {shape[1]} pixels has no image planes "
                             f"({self.images.shape[0]} images of {self._plane_hw[0]} x {self._plane_hw[1]})")
        batch = self._assemble(shape, None, None, cam_idx, None, False, False)
        batch['camera_id'] = batch['cam_idx'][..., 0]
        return batch

    # ------------------------------------------------------------------ _next_train (:478-570)
    def _randint(self, low, high, shape):
        if high <= low:
            raise ValueError(f"next_train: empty range [{low}, {high}) (border and patch leave no pixel)")
        return torch.randint(low, high, shape, device=self.device, dtype=torch.int32, generator=self._device_generator)

    def sample_train_indices(self, generator=None, max_virtual_tries=64, fix_src_rows=False):
        """The draws of `_next_train`: the keyword arguments `make_ray_batch` is called with.  See `next_train`."""
        gen = self._host_generator if generator is None else generator
        if gen.device.type != 'cpu':
            raise RuntimeError("next_train: `generator` is a CPU torch.Generator; the device draws are seeded from it")
        scalar = lambda low, high: int(torch.randint(low, high, (1,), generator=gen))
        self._device_generator.manual_seed(scalar(0, 2 ** 62))
        sh = self._shapes
        num_patches, patch = sh['num_patches'], sh['patch_size']
        pix_x_int = self._randint(*sh['x_range'], (num_patches, 1, 1))                      # :490-494
        pix_y_int = self._randint(*sh['y_range'], (num_patches, 1, 1))
        dx, dy = camera_utils.pixel_coordinates(patch, patch, device=self.device)          # :497-500
        pix_x_int, pix_y_int = pix_x_int + dx, pix_y_int + dy
        if self._batching == ALL_IMAGES:                                                    # :502-505
            cam_idx = self._randint(0, self._n_examples, (num_patches, 1, 1))
        else:
            cam_idx = self._randint(0, self._n_examples, (1,))
        args = dict(pix_x_int=pix_x_int, pix_y_int=pix_y_int, cam_idx=cam_idx)
        if not self.virtual_poses_enabled:
            return args
        if patch != 1 or self._batching != ALL_IMAGES:
            raise ValueError("virtual_poses needs patch_size = 1 and batching = 'all_images': the reference concatenates "
                             "[num_patches, 1, 1] arrays (datasets.py:550-555)")
        if self._virtual_host is None or self.cam_num is None or self.disp_images is None:
            raise RuntimeError("virtual_poses needs virtual_poses, cam_num and disp_images")
        num_virtual = sh['num_patches_for_virtual']
        flip = np.diag([1., -1., -1., 1.])
        to44 = lambda p: np.concatenate([p, [[0., 0., 0., 1.]]], axis=0)
        if self._n_examples <= 3 * self.cam_num:
            raise RuntimeError(f"next_train: {self._n_examples} images and cam_num = {self.cam_num}: no reference camera is "
                               ">= 3 * cam_num (datasets.py:519 would never be true)")
        interval = [-2 * self.cam_num, -self.cam_num, 0, self.cam_num, 2 * self.cam_num]   # :512
        warps = 0
        while warps < int(max_virtual_tries):                                               # :509 `while True`
            src = scalar(0, self._n_examples * VIRTUAL_CASE)
            src_true = src // VIRTUAL_CASE
            step = interval[scalar(0, len(interval))]
            ref = src_true + step if 0 <= src_true + step < self._n_examples else src_true
            if ref < 3 * self.cam_num:                                                      # :519
                continue                                                                    # a host-side redraw, not a try
            warps += 1
            depth = self.disp_images[ref].reshape(self._plane_hw)
            ref_pose, src_pose = to44(self._c2w_host[ref]) @ flip, to44(self._virtual_host[src]) @ flip      # :524-525
            pts_in_src, mask = train_utils.img_warping(ref_pose, src_pose, depth, np.linalg.inv(self._p2c_host[ref]))
            if int(mask.sum()) >= num_virtual:                                              # :528, the one sync per attempt
                break
        else:
            raise RuntimeError(f"next_train: no virtual pose kept {num_virtual} valid pixels in {max_virtual_tries} warps "
                               "(the reference loops forever here, datasets.py:509-529)")
        if num_virtual:
            ref_x, ref_y, src_x, src_y = train_utils.sample_virtual_pixels(pts_in_src, mask, num_virtual,
                                                                          generator=self._device_generator)
        else:
            ref_x = ref_y = src_x = src_y = torch.empty(0, dtype=torch.int32, device=self.device)
        col = lambda t: t.reshape(-1, 1, 1)
        full = lambda v: torch.full((num_virtual, 1, 1), v, dtype=torch.int32, device=self.device)
        cat = lambda a, b: torch.cat((a, b), dim=0)
        src_rows = pix_y_int if fix_src_rows else pix_x_int                                 # :553 concatenates pix_x_int
        args.update(cam_idx_with_src=cat(cam_idx, full(src + self._n_examples)), cam_idx_with_ref=cat(cam_idx, full(ref)),
                    pixel_x_int_with_src=cat(pix_x_int, col(src_x)), pixel_y_int_with_src=cat(src_rows, col(src_y)),
                    pixel_x_int_with_ref=cat(pix_x_int, col(ref_x)), pixel_y_int_with_ref=cat(pix_y_int, col(ref_y)))
        return args

    def next_train(self, generator=None, max_virtual_tries=64, fix_src_rows=False):
        """datasets.py:478-570: one random training batch.  Patch origins inside the border, patch offsets, and the camera
        draw (`all_images`: one per patch, `single_image`: one for the batch) are `torch.randint` on the device.

        `generator` is a CPU `torch.Generator` (default: the dataset's own): the scalar draws of the virtual-pose loop come
        from it directly, and the device generator behind the tensor draws is re-seeded from it at each call, so two calls
        with equally seeded generators return equal batches.  The stream is not `np.random`'s.

        With `virtual_poses` the reference's selection loop runs as written: a source among `n_examples * 9` virtual poses,
        one of the five `cam_num` intervals for the reference camera, the `>= 3 * cam_num` condition, then
        `train_utils.img_warping` of that camera's depth plane (on the device) until `mask.sum() >= int(0.2 * num_patches)`.
        Reading that sum is one `.item()` per warp, the only syncs of a batch.  `max_virtual_tries` counts warps: a draw the
        `>= 3 * cam_num` condition rejects is redrawn on the host and does not count (a dataset where no camera can meet it
        is refused up front).  After that many warps without enough pixels it raises RuntimeError; the reference loops
        unbounded.  `sample_virtual_pixels` then draws the virtual rays.

        datasets.py:553 reads `pixel_y_int_with_src = np.concatenate((pix_x_int, src_valid_pixel_y))`: the REAL rays of a
        virtual-pose batch are cast through pixel (x, x), while their colours come from (x, y).  This is reproduced by
        default, because parity with the reference is the contract; `fix_src_rows=True` concatenates `pix_y_int` instead.

        `apply_bayer_mask`: lossmult is `raw_utils.pixels_to_bayer_mask` of each ray's pixel, computed in the kernel; with
        `virtual_poses` it is refused (the reference hands the real rays' mask to the longer batch)."""
        args = self.sample_train_indices(generator, max_virtual_tries, fix_src_rows)
        if not self._apply_bayer_mask:
            return self.make_ray_batch(**args, validate=False)              # in range by construction
        if self.virtual_poses_enabled:
            raise NotImplementedError("apply_bayer_mask with virtual_poses: the reference's lossmult has the real rays' shape, "
                                      "the batch is longer (datasets.py:559-567)")
        x, y, cam = args['pix_x_int'], args['pix_y_int'], args['cam_idx']
        shape = torch.broadcast_shapes(x.shape, y.shape)
        batch = self._assemble(shape, (_flat_i32(cam, shape), _flat_i32(x, shape), _flat_i32(y, shape)), None, 0, None, True, False)
        batch['camera_id'] = batch['cam_idx'][..., 0]
        return batch
