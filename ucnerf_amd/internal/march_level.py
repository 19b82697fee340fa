"""What a sampling level needs around its kernels, once for both marches (ref models.py:97-324): `march` (march_infer.py, the
fused inference march) and `march_train` (train_graph.py, the autograd march; its nodes: march_nodes.py) walk the same level schedule.  Here: the batch's
rays, the level plan and anneal value, the random draws in the reference's order, a level's fenceposts with the choice between
an entry point and its `_tdist` sibling, the inference march's pass plan, and a level's outputs with the result dictionaries made of them.
What runs in between -- featurisation, dense layers, compositing, the sky and brightness tails -- stays with each march (kernels in one,
autograd nodes in the other)."""
import ctypes
import functools

import numpy as np
import torch

from .. import _lib


def _f32(t, n, c):
    t = t.reshape(n, c)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


class Rays:
    """The batch as float32 [N, c] tensors, its leading shape `prefix`, and the optional keys that pin the random draws: `rand_vec`
    [N, 3 * num_levels] and `noise` (batch['march_noise']: per level a dict of 'jitter', 'flip', 'spin', 'bg'; {} where nothing is pinned)."""
    __slots__ = ("o", "d", "vd", "cam", "rad", "near", "far", "prefix", "N", "dev", "rand_vec", "noise")

    def __init__(self, batch, num_levels, on_device=True):
        origins = batch['origins']
        if on_device:
            _lib.require_device(origins, "batch['origins']")
        self.dev, self.prefix = origins.device, tuple(origins.shape[:-1])
        self.N = N = int(np.prod(self.prefix))
        self.o, self.d, self.vd, self.cam = (_f32(batch[k], N, 3) for k in ('origins', 'directions', 'viewdirs', 'cam_dirs'))
        self.rad, self.near, self.far = (_f32(batch[k], N, 1) for k in ('radii', 'near', 'far'))
        rand_vec, noise = batch.get('rand_vec'), batch.get('march_noise')
        self.rand_vec = None if rand_vec is None else _f32(rand_vec, N, 3 * num_levels)
        self.noise = [{}] * num_levels if noise is None else noise


def anneal_of(anneal_slope, train_frac):
    """models.py:179-184: Schlick's bias of the training fraction; 1 with the slope off."""
    return (anneal_slope * train_frac) / ((anneal_slope - 1) * train_frac + 1) if anneal_slope > 0 else 1.


def s_near_of(model, train_frac):
    """models.py:137-141: where the rays' normalised interval starts -- 0 without Model.near_anneal_rate, else
    clip(1 - train_frac / near_anneal_rate, 0, near_anneal_init).  The ONE place that computes it: the level plan's dilation, the
    first level's interval and the resampling domain (`fenceposts`) read it from here."""
    rate = getattr(model, 'near_anneal_rate', None)
    if rate is None:
        return 0.
    if train_frac is None:
        raise ValueError("Model.near_anneal_rate is set: the level plan depends on train_frac")
    return float(np.clip(1 - train_frac / rate, 0, model.near_anneal_init))


def level_plan(model, train_frac=None):
    """[(i_level, is_prop, S, mlp, dilation)] of models.py:152-168.  dilation = bias + multiplier * (1 - s_near) / (the product of the
    earlier levels' sample counts), s_near = `s_near_of(model, train_frac)` (0 without near_anneal_rate: train_frac is not read);
    0.0 with use_dilation off (both knobs <= 0), which ucn_resample reads as "resample undilated"."""
    use_dilation = model.dilation_bias > 0 or model.dilation_multiplier > 0
    span = 1.0 - s_near_of(model, train_frac)                # init_s_far - init_s_near
    plan, prod_num_samples = [], 1
    for i_level in range(model.num_levels):
        is_prop = i_level < model.num_levels - 1
        S = model.num_prop_samples if is_prop else model.num_nerf_samples
        mlp = model.get_submodule(f'prop_mlp_{i_level}') if is_prop else model.nerf_mlp
        dilation = model.dilation_bias + model.dilation_multiplier * span / prod_num_samples if use_dilation else 0.0
        if use_dilation and not dilation > 0:
            # (a negative dilation_bias) the reference would dilate by it; ucn_resample takes dilation <= 0 as the UNdilated branch
            raise NotImplementedError(f"dilation {dilation} <= 0 at level {i_level} with use_dilation on: not the shipped configuration")
        prod_num_samples *= S
        plan.append((i_level, is_prop, S, mlp, dilation))
    return plan


def pass_plan(N, nerf_chunk, level_row, nerf_row, is_prop):
    """(chunk, [(i_pass, r0, n)]): the inference march's passes over a level's N rays, `chunk` rays each and the rest in the last.
    nerf_chunk = Model.max_chunk_rays is quoted for the NeRF level (nerf_row feature floats per ray); a proposal level with a shorter row
    (level_row: fewer samples, narrower features) takes proportionally more rays per pass -- the same workspace bytes, fewer and longer
    launches -- in multiples of 256, at most 65536."""
    chunk = nerf_chunk
    if is_prop and level_row < nerf_row:
        chunk = max(nerf_chunk, min(nerf_chunk * nerf_row // level_row // 256 * 256, 1 << 16))
    return chunk, [(i_pass, r0, min(chunk, N - r0)) for i_pass, r0 in enumerate(range(0, N, chunk))]


def timed_pass(i_pass, prof_every):
    """whether pass i_pass gets timing events (Model._prof): one of every prof_every passes, from the middle of each group"""
    return i_pass % prof_every == prof_every // 2


def draws(rays, i_level, S, rand, single_jitter):
    """(jitter, flip, spin, rvec) of one level, in the reference's order: stepfun.py:216 rand(N, 1 | S), render.py:123 and :124
    rand(N, S) each -- these three only with `rand`, else None -- then render.py:140 randn(N, 3) always.  A value the batch pins
    is taken instead of drawn (and consumes nothing of the generator); the others are still drawn, in that order."""
    N, dev = rays.N, rays.dev
    jitter = flip = spin = None
    if rand:
        pn = rays.noise[i_level]
        jcols = 1 if single_jitter else S
        jitter = _f32(pn['jitter'], N, jcols) if 'jitter' in pn else torch.rand(N, jcols, device=dev)
        flip = _f32(pn['flip'], N, S) if 'flip' in pn else torch.rand(N, S, device=dev)
        spin = _f32(pn['spin'], N, S) if 'spin' in pn else torch.rand(N, S, device=dev)
    rvec = torch.randn(N, 3, device=dev) if rays.rand_vec is None else rays.rand_vec[:, 3 * i_level:3 * i_level + 3].contiguous()
    return jitter, flip, spin, rvec


def background(model, rays, i_level, rand):
    """(bg, ray_bg) of one level (models.py:245-256): the scalar background intensity, and float32 [N, 3] per-ray colours or None.
    A one-valued Model.bg_intensity_range is that value; a two-valued one is its midpoint for `rand is None` ALONE (models.py:249),
    else -- `rand = False` included, which is what every evaluation caller of the reference passes: there the reference draws too --
    one rand(N, 3) * (max - min) + min, drawn AFTER the level's `draws` and its MLP (models.py:256; nothing between them consumes the
    generator here), so both marches call this behind their dense layers.  With rand = False that is right behind the level's
    randn(N, 3): jitter, flip and spin are not drawn.  batch['march_noise'][i_level]['bg'] pins the colours (and then consumes
    nothing of the generator)."""
    lo, hi = float(model.bg_intensity_range[0]), float(model.bg_intensity_range[1])
    if lo == hi:
        return lo, None
    if rand is None:
        return (lo + hi) / 2, None
    pn = rays.noise[i_level]
    if 'bg' in pn:
        return lo, _f32(pn['bg'], rays.N, 3)
    return lo, torch.rand(rays.N, 3, device=rays.dev) * (hi - lo) + lo


def ray_gain(model, batch, rays):
    """models.py:258-269, the RawNeRF exposure: float32 [N, 3] colour gain of every ray, or None without batch['exposure_idx'].
    gain = exposure_values, times 1 + (exposure_idx > 0) * exposure_scaling_offsets(exposure_idx) with learned_exposure_scaling --
    plain torch, so autograd carries the compositing node's gradient on it to the embedding."""
    idx = batch.get('exposure_idx')
    if idx is None:
        return None
    values = batch.get('exposure_values')
    if values is None:
        raise TypeError("batch['exposure_idx'] is set but batch['exposure_values'] is None (the reference indexes None here, models.py:261)")
    N = rays.N
    gain = values.to(rays.dev).float().reshape(N, -1).expand(N, 3)
    if model.learned_exposure_scaling:
        idx = idx.to(rays.dev).reshape(N, -1)[:, 0]
        scaling = 1 + (idx > 0)[:, None] * model.exposure_scaling_offsets(idx.long())
        gain = gain * scaling.float()
    return gain.contiguous()


def composite(posts, density, rgbs, dirs, gain, ray_bg, bg, opaque, weights, main, extras, stream):
    """One compositing launch of a level's N rays: ucn_composite, or ucn_composite_rays with a per-ray gain (the scaled colours are
    written over `rgbs`, as the reference scales ray_results['rgb'] in place) and / or per-ray background colours."""
    lib = _lib.load()
    N, S = density.shape
    if rgbs is None:
        gain = None                                            # models.py:584-585: a proposal level's colours are zeros, gain * 0 = 0
    if gain is None and ray_bg is None:
        _lib.check(posts.entry(lib, 'ucn_composite')(density.data_ptr(), _lib.ptr(rgbs), *posts.compositing(), dirs.data_ptr(),
                                                     float(bg), int(bool(opaque)), N, S, weights.data_ptr(), main.data_ptr(),
                                                     _lib.ptr(extras), stream))
        return
    _lib.check(posts.entry(lib, 'ucn_composite_rays')(density.data_ptr(), _lib.ptr(rgbs), *posts.compositing(), dirs.data_ptr(),
                                                      _lib.ptr(gain), _lib.ptr(ray_bg), float(bg), int(bool(opaque)), N, S,
                                                      weights.data_ptr(), main.data_ptr(), _lib.ptr(extras),
                                                      _lib.ptr(rgbs) if gain is not None else None, stream))


@functools.lru_cache(maxsize=None)
def _u_table(num_samples, train, device):
    """stepfun.py:203-216: (the u grid of the inverse-CDF lookup on `device`, max_jitter); constant per S, so cached."""
    eps = float(torch.finfo(torch.float32).eps)
    if train:
        u_max = eps + (1 - eps) / num_samples
        max_jitter = (1 - u_max) / (num_samples - 1) - eps
        u = torch.linspace(0, 1 - u_max, num_samples)
    else:
        pad = 1 / (2 * num_samples)
        max_jitter = 0.0
        u = torch.linspace(pad, 1. - pad - eps, num_samples)
    return u.to(device), max_jitter


def s_to_t(model, sdist, near, far, stream):
    """models.py:208 `tdist = s_to_t(sdist)` on the device (ucn_s_to_t) for a model with a warped ray-distance curve; None for
    the identity curve, whose kernels derive t from sdist, near and far themselves (nothing extra is launched)."""
    if not model._raydist_curve:
        return None
    N, S1 = sdist.shape
    tdist = torch.empty(N, S1, device=sdist.device)
    _lib.check(_lib.load().ucn_s_to_t(sdist.data_ptr(), near.data_ptr(), far.data_ptr(), N, S1, model._raydist_curve,
                                      float(model.power_lambda), tdist.data_ptr(), stream))
    return tdist


class Fenceposts:
    """A level's fenceposts: sdist [N, S+1] with the batch's near / far, their metric form tdist for a warped Model.raydist_fn, and the
    cone basis [N, 6].  The one place that knows which sibling of an entry point reads them, with which pointer arguments."""
    __slots__ = ("sdist", "near", "far", "tdist", "basis")

    def __init__(self, sdist, near, far, tdist, basis):
        self.sdist, self.near, self.far, self.tdist, self.basis = sdist, near, far, tdist, basis

    def entry(self, lib, name):
        """lib.<name> (ucn_march_features[_backward], ucn_composite[_rays][_backward]), or its `_tdist` sibling on metric fenceposts."""
        return getattr(lib, name if self.tdist is None else name + '_tdist')

    def geometry(self, rays, flip, spin, sl=slice(None)):
        """The featurisation's geometry arguments for the rays `sl`: what the kernels derive t from, then the cones."""
        fence = (self.sdist, self.near, self.far) if self.tdist is None else (self.tdist,)
        return [t[sl].data_ptr() for t in fence + (rays.o, rays.d, self.basis, rays.rad)] + [
            None if flip is None else flip[sl].data_ptr(), None if spin is None else spin[sl].data_ptr()]

    def normals_geometry(self, rays, flip, spin, sl=slice(None)):
        """`geometry` for the entry points without a `_tdist` sibling (`ray_call`): metric fenceposts go with near = far = NULL."""
        g = self.geometry(rays, flip, spin, sl)
        return g if self.tdist is None else [g[0], None, None] + g[1:]

    def ray_call(self, lib, name, field, rays, flip, spin, sl, std_scale, warp, *tail):
        """One of the ray-path entry points -- ucn_march_features[_backward], ucn_march_scale_features, ucn_march_density_grad -- for a
        field of the given warp (MLP.warp: 1 = 'contract', 0 = warp_fn None): lib.<name>[_tdist](field, geometry, std_scale, *tail) or
        lib.<name>_warp(field, fenceposts, near, far, cones, std_scale, 0, *tail)."""
        if not warp:
            return getattr(lib, name + '_warp')(field, *self.normals_geometry(rays, flip, spin, sl), float(std_scale), 0, *tail)
        # 'contract': the entry points the warped field always called (themselves calls of the above with warp = 1)
        if name == 'ucn_march_density_grad':
            return lib.ucn_march_density_grad(field, *self.normals_geometry(rays, flip, spin, sl), float(std_scale), *tail)
        return self.entry(lib, name)(field, *self.geometry(rays, flip, spin, sl), float(std_scale), *tail)

    def compositing(self, sl=slice(None), backward=False):
        """The compositing arguments for the rays `sl`; the forward `_tdist` sibling also reads the batch's metric far."""
        fence = (self.sdist, self.near, self.far) if self.tdist is None else (self.tdist,) if backward else (self.tdist, self.far)
        return [t[sl].data_ptr() for t in fence]


def fenceposts(model, rays, i_level, S, dilation, train_frac, rand, prev, weights_prev, stream, pinned_sdist=None):
    """The level's draws, then ucn_resample from the previous level's fenceposts `prev` and weights (None at level 0), ucn_cone_basis
    and s_to_t: (Fenceposts, flip, spin).  pinned_sdist: the training route's test hook -- fenceposts handed in instead of the
    resampling kernel's (no gradient flows through them in the reference either, stepfun.py:251-294)."""
    lib, N, dev = _lib.load(), rays.N, rays.dev
    jitter, flip, spin, rvec = draws(rays, i_level, S, rand, model.single_jitter)
    u_tab, max_jitter = _u_table(S, bool(rand), dev)
    sdist = torch.empty(N, S + 1, device=dev)
    basis = torch.empty(N, 6, device=dev)
    sdist_prev, n_prev = (None, 0) if prev is None else (prev.sdist, prev.sdist.shape[1] - 1)
    wp = None if weights_prev is None else weights_prev.detach().contiguous()
    s_near = s_near_of(model, train_frac)
    tail = (u_tab.data_ptr(), _lib.ptr(jitter), 0 if jitter is None else jitter.shape[1], max_jitter, N, S, sdist.data_ptr(), stream)
    head = (_lib.ptr(sdist_prev), _lib.ptr(wp), n_prev, dilation, anneal_of(model.anneal_slope, train_frac), float(model.resample_padding))
    if s_near == 0:
        _lib.check(lib.ucn_resample(*head, *tail))
    else:                                                      # near_anneal_rate: the domain [s_near, 1] (models.py:143-146,173,200)
        _lib.check(lib.ucn_resample_domain(*head, s_near, *tail))
    if pinned_sdist is not None:
        sdist = _f32(pinned_sdist, N, S + 1).clone()
    _lib.check(lib.ucn_cone_basis(rays.cam.data_ptr(), rvec.data_ptr(), N, basis.data_ptr(), stream))
    return Fenceposts(sdist, rays.near, rays.far, s_to_t(model, sdist, rays.near, rays.far, stream), basis), flip, spin


def density_normals(mlp, posts, rays, flip, spin, sl, n, S, std_scale, layout, feat, raw_grad, normals, stream, field=None):
    """models.py:550-567 for the n rays `sl` of a level, after its dense layers, on `stream`: the feature buffer `feat` ([L][n*S][C],
    layout 0 or 2 as ucn_march_features wrote it) becomes d raw_density / d features IN PLACE (ucn_density_feature_grad), then the second
    gather fills raw_grad[sl] and normals[sl] ([N, S, 3]).  Nothing here carries an autograd graph.  field: the level's
    mlp.normals_field(), for a caller that runs many passes of one level."""
    lib = _lib.load()
    d = mlp.normals_field() if field is None else field
    _lib.check(lib.ucn_density_feature_grad(ctypes.byref(d), feat.data_ptr(), n * S, feat.data_ptr(), stream))
    _lib.check(posts.ray_call(lib, 'ucn_march_density_grad', ctypes.byref(d), rays, flip, spin, sl, std_scale, mlp.warp, n, S, layout,
                              feat.data_ptr(), raw_grad[sl].data_ptr(), normals[sl].data_ptr(), stream))


def pred_normals(desc, head, feat, sl, n, S, layout, grad_pred, normals_pred, stream):
    """models.py:569-578 for the n rays `sl` of a level, after its dense layers, on `stream`: ucn_pred_normals reads the pass's feature
    buffer `feat` ([L + scale planes][n*S][C], layout 0 or 2 as the gather wrote it) and fills grad_pred[sl] and normals_pred[sl]
    ([N, S, 3]).  desc: the level's mlp.field() (its unpacked density_layer.0); head: mlp.pred_head().  No autograd graph."""
    A, c = head
    _lib.check(_lib.load().ucn_pred_normals(ctypes.byref(desc), A.data_ptr(), c.data_ptr(), feat.data_ptr(), n, S, layout,
                                            grad_pred[sl].data_ptr(), normals_pred[sl].data_ptr(), stream))


def ref_heads(mlp, desc, head, feat, sl, n, S, layout, rgbs, roughness, stream):
    """models.py:589-597 and :661-674 for the n rays `sl` of a level, after its dense layers, on `stream`: ucn_ref_heads reads the pass's
    feature buffer `feat` (as `pred_normals`), turns rgbs[sl] ([N, S, 3], the colour MLP's sigmoid WITHOUT padding) into the final colour in
    place when the field has the diffuse head, and fills roughness[sl] ([N, S], or None: not wanted).  desc: the level's mlp.field();
    head: mlp.ref_head().  No autograd graph."""
    A, c = head
    _lib.check(_lib.load().ucn_ref_heads(ctypes.byref(desc), A.data_ptr(), c.data_ptr(), mlp.ref_heads_mask(), float(mlp.roughness_bias),
                                         float(mlp.rgb_padding), feat.data_ptr(), n, S, layout, None if rgbs is None else rgbs[sl].data_ptr(),
                                         None if roughness is None else roughness[sl].data_ptr(), stream))


# ---- result dictionaries (the keys of ref models.py:262-324) -------------------------------------------------------------
def rendering_entry(rgb, depth, acc, weights, extras, prefix, sdist=None, rgbs=None, n_vis=16, normals=None, normals_pred=None,
                    roughness=None):
    """rgb [N, 3], depth [N], acc [N], weights [N, S]; with extras [N, 4] (compute_extras: distance mean, 5 %, median, 95 %) also the
    'ray_*' keys: the first n_vis rays' fenceposts, weights and colours (rgbs None, a proposal level: zeros until `broadcast_final`)."""
    N, S = weights.shape
    r = dict(rgb=rgb.reshape(prefix + (3,)), depth=depth.reshape(prefix), acc=acc.reshape(prefix))
    if extras is not None and normals is not None:          # render.py:218-222: alpha-composited like the colours, no background term
        r['normals'] = (weights.detach()[..., None] * normals).sum(dim=-2).reshape(prefix + (3,))
    # the same for the predicted normals (a key that starts with 'normals', models.py:279-283).  The rendered key carries NO gradient, in the
    # training graph too (the reference composites it with the graph attached; no loss reads the rendering: train_utils reads the history)
    if extras is not None and normals_pred is not None:
        r['normals_pred'] = (weights.detach()[..., None] * normals_pred.detach()).sum(dim=-2).reshape(prefix + (3,))
    # and the roughness [N, S] (models.py:279-283 `k in ['roughness']`), no gradient either: nothing on the path consumes it
    if extras is not None and roughness is not None:
        r['roughness'] = (weights.detach() * roughness.detach().reshape(N, S)).sum(dim=-1).reshape(prefix + (1,))
    if extras is not None:
        for j, k in enumerate(('distance_mean', 'distance_percentile_5', 'distance_median', 'distance_percentile_95')):
            r[k] = extras[:, j].reshape(prefix)
    r['weights'] = weights.reshape(prefix + (S,))
    if extras is not None:
        r['ray_sdist'], r['ray_weights'] = sdist[:n_vis], weights[:n_vis]
        r['ray_rgbs'] = rgbs[:n_vis] if rgbs is not None else torch.zeros(min(n_vis, N), S, 3, device=weights.device)
    return r


def broadcast_final(renderings):
    """ref models.py:313-324: the last level's composited ray colours stand in for the proposal levels' ray_rgbs."""
    final = (renderings[-1]['ray_rgbs'] * renderings[-1]['ray_weights'][..., None]).sum(dim=-2)
    for r in renderings[:-1]:
        r['ray_rgbs'] = final[:, None, :].expand(r['ray_rgbs'].shape)


def history_entry(coord, density, rgbs, sdist, weights, prefix, raw_grad=None, normals=None, grad_pred=None, normals_pred=None,
                  roughness=None):
    """coord [N, S, 3], density [N, S], rgbs [N, S, 3] or None (zeros), sdist [N, S+1], weights [N, S], roughness [N, S] or None."""
    N, S = weights.shape
    rgb = torch.zeros(N, S, 3, device=weights.device) if rgbs is None else rgbs
    return dict(coord=coord.reshape(prefix + (S, 3)), density=density.reshape(prefix + (S,)), rgb=rgb.reshape(prefix + (S, 3)),
                raw_grad_density=None if raw_grad is None else raw_grad.reshape(prefix + (S, 3)),
                grad_pred=None if grad_pred is None else grad_pred.reshape(prefix + (S, 3)),
                normals=None if normals is None else normals.reshape(prefix + (S, 3)),
                normals_pred=None if normals_pred is None else normals_pred.reshape(prefix + (S, 3)),
                roughness=None if roughness is None else roughness.reshape(prefix + (S, 1)),
                sdist=sdist.reshape(prefix + (S + 1,)).clone(), weights=weights.reshape(prefix + (S,)).clone())


class LevelOutputs:
    """What one level of either march produces: per sample density [N, S], rgbs [N, S, 3] (None: a field without colour layers), weights
    [N, S], coord, raw_grad, normals, grad_pred, normals_pred [N, S, 3], roughness [N, S] or [N, S, 1]; per ray main = the composited
    (rgb, depth, acc) -- the compositing kernel's [N, 5] buffer, or the three tensors of the autograd nodes -- and extras [N, 4].  None =
    not produced.  The one place that turns them into the result dictionaries."""
    __slots__ = ("density", "rgbs", "weights", "main", "extras", "coord", "raw_grad", "normals", "grad_pred", "normals_pred", "roughness")

    def __init__(self, **outputs):
        for k in self.__slots__:
            setattr(self, k, outputs.pop(k, None))
        assert not outputs, sorted(outputs)

    @classmethod
    def allocate(cls, mlp, N, S, dev, want_history, compute_extras):
        """The buffers the inference march's kernels fill for `mlp`'s level: colours with the field's colour layers (the NeRF level's, and
        those of a proposal field built with PropMLP.disable_rgb = False, which the reference composites like the last level's,
        models.py:221-283); extras with compute_extras; coord with want_history; density normals, predicted normals (7h)
        and roughness (7i) where the field has them and something returns them (the history, or the renderings' extras)."""
        buf = lambda want, *shape: torch.empty(N, *shape, device=dev) if want else None
        returned = want_history or compute_extras
        normals = (not mlp.disable_density_normals) and returned
        pred = mlp.enable_pred_normals and returned
        rough = bool(mlp.ref_heads_mask() & mlp.HEAD_ROUGHNESS) and returned
        return cls(density=buf(True, S), rgbs=buf(not mlp.disable_rgb, S, 3), weights=buf(True, S), main=buf(True, 5),
                   extras=buf(compute_extras, 4), coord=buf(want_history, S, 3), raw_grad=buf(normals, S, 3), normals=buf(normals, S, 3),
                   grad_pred=buf(pred, S, 3), normals_pred=buf(pred, S, 3), roughness=buf(rough, S))

    def rendering(self, prefix, sdist, n_vis):
        rgb, depth, acc = self.main if isinstance(self.main, tuple) else (self.main[:, 0:3], self.main[:, 3], self.main[:, 4])
        return rendering_entry(rgb, depth, acc, self.weights, self.extras, prefix, sdist, self.rgbs, n_vis, normals=self.normals,
                               normals_pred=self.normals_pred, roughness=self.roughness)

    def history(self, prefix, sdist):
        return history_entry(self.coord, self.density, self.rgbs, sdist, self.weights, prefix, self.raw_grad, self.normals,
                             grad_pred=self.grad_pred, normals_pred=self.normals_pred, roughness=self.roughness)
