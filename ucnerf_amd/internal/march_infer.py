"""The fused inference march (ref models.py:97-365 without a graph), beside train_graph.py: `march` walks march_level.py's level schedule;
a level is its outputs (`march_level.LevelOutputs`), four closures chosen once -- `_gather`, `mlp_route`'s dense layers, `_tails`' per-sample
passes behind them -- and `run_passes`, which alone knows streams and events.  `mixed_level` decides the mixed-precision route of a level;
`_sky_tail` and `_brightness_tail` finish the renderings.  `Model._march` (models.py) delegates here."""
import ctypes
from types import SimpleNamespace

import torch

from .. import _lib
from . import march_level as ml
from .head_pack import prepare_heads, view_encoding
from .models import _cached


def _dir_tiles(enc):
    """[N, E <= 31] direction encodings -> [N, 32] bf16 tiles [enc, 1, 0...]: the input tile whose column E meets the bias column
    of the colour layers' weight streams (head_pack._head_gather_index(dir_in_stream=True))."""
    n, e = enc.shape
    t = torch.zeros(n, 32, device=enc.device, dtype=torch.bfloat16)
    t[:, :e] = enc
    t[:, e] = 1.0
    return t


def mixed_level(model, mlp, is_prop, F_in):
    """Mixed-precision inference of one level (see `Model.autocast_render`): None = the fp32-class path, else what the bf16
    kernels need -- the half table behind a copy of the grid descriptor and the packed / rounded dense parameters."""
    if not (model.autocast_render and torch.is_autocast_enabled() and torch.get_autocast_dtype('cuda') == torch.bfloat16):
        return None
    # fp32-class path for what reads fp32 features of the fp32 table: scale planes, the density normals' pass (7d), the
    # predicted-normal head (7h) and the Ref-NeRF colour heads (7i)
    if mlp.scale_featurization or not mlp.disable_density_normals or mlp.enable_pred_normals or mlp.ref_heads_mask():
        return None
    from .train_graph import heads_route
    emb = mlp.encoder.embeddings
    # the level's bf16 kernels are the training step's: the same route decision (no GLO here: every inference march is zero_glo)
    if heads_route(mlp, F_in, emb.is_cuda, torch.bfloat16, None) != ("prop_fused" if is_prop else "fused_bf16"):      # (the features are fp32)
        return None

    def build():
        out = {}
        half = mlp.encoder.level_dim % 2 == 0                      # grid.py:41-44: half tables when C is even
        if half:
            out['table'] = emb.detach().to(torch.half)
        out['desc'], out['table_flag'] = mlp.grid_field_with(out['table'] if half else emb), (_lib.TABLE_F16 if half else 0)
        # the NeRF level's features leave the gather as the bf16 pairs its MLP consumes (half the workspace traffic)
        out['feat_flag'] = _lib.FEATURES_BF16 if (half and mlp.encoder.level_dim == 2 and not is_prop and model.autocast_bf16_features) else 0
        with torch.autocast('cuda', enabled=False):
            if is_prop:
                l0, l1 = mlp.density_layer[0], mlp.density_layer[2]
                out['prop'] = tuple(t.detach().float().contiguous() for t in (l0.weight, l0.bias, l1.weight, l1.bias))
            else:
                d0, d1, c0, c1, lr = mlp.density_layer[0], mlp.density_layer[2], mlp.lin_second_stage_0, mlp.lin_second_stage_1, mlp.rgb_layer
                # a GLO field: the zero code's modulation folded into the colour layers (every inference march here is zero_glo)
                W0, b0, W1, b1 = mlp._glo_folded() if mlp.uses_glo() else (c0.weight, c0.bias, c1.weight, c1.bias)
                packed, _, We, be, bias0, bias1, biasr = prepare_heads(d0.weight, d0.bias, d1.weight, d1.bias, W0, b0,
                                                                      W1, b1, lr.weight, lr.bias, dir_in_stream=True)
                out.update(packed=packed, We=We, be=be, bias0=bias0, bias1=bias1, biasr=biasr, NW=c0.weight.shape[0],
                           head=(ctypes.c_float * 4)(float(mlp.density_bias), float(mlp.rgb_premultiplier), float(mlp.rgb_bias),
                                                     float(mlp.rgb_padding)),
                           enc=lambda v: _dir_tiles(view_encoding(v.float(), mlp.deg_view)))
        return out
    # the half table and the packed weights are rebuilt only when a parameter changed (a frame is tens of chunks); one slot per field
    slot = model.__dict__.setdefault('_mixed_cache', {}).setdefault(id(mlp), SimpleNamespace())
    return _cached(slot, 'level', mlp.parameters(), build, extra=(bool(model.autocast_bf16_features),))


def mlp_route(model, mlp, is_prop, desc, mixed, out, rays, posts, dirb, co, nc):
    """The level's dense layers as one callable run(fb, sl, r0, n): density (and colours) of the n rays `sl` = [r0, r0 + n) from the feature
    buffer `fb` into `out`.  Chosen once per level: mixed-precision proposal / NeRF level, compacted colour pass, plain ucn_field_mlp.
    dirb: the level's direction terms; co: its launch-shape flag; nc: the rays of its largest pass."""
    lib, st, dev = _lib.load(), _lib.stream(), rays.dev
    density, rgbs, weights, main = out.density, out.rgbs, out.weights, out.main
    S, L, C = density.shape[1], mlp.encoder.num_levels, mlp.encoder.level_dim
    dir_row = dirb.numel() // max(rays.N, 1)            # (an empty batch runs no pass)
    rf = int(bool(model.rays_fastest))
    if mlp.ref_heads_mask() & mlp.HEAD_DIFFUSE:         # the diffuse head finishes the colours: the dense layers leave the plain sigmoid
        desc = mlp.unpadded_field(desc)
    if mixed is not None and is_prop:
        w0, b0_, w1, b1_ = mixed['prop']
        def run(fb, sl, r0, n):
            _lib.check(lib.ucn_prop_train_fwd(fb.data_ptr(), L * C, w0.shape[0], w0.data_ptr(), b0_.data_ptr(), w1.data_ptr(),
                                              b1_.data_ptr(), float(mlp.density_bias), 1, n * S, density[sl].data_ptr(), n, C, st))
    elif mixed is not None:
        # the ray's direction tile rides in the weight stream's last input tile (no per-ray terms to pre-multiply)
        vd_enc = mixed['enc'](rays.vd)
        feat_flags = C | (_lib.FEAT_BF16 if mixed['feat_flag'] else 0)
        def run(fb, sl, r0, n):
            _lib.check(lib.ucn_train_fwd(fb.data_ptr(), L * C, mixed['packed'].data_ptr(), mixed['bias0'].data_ptr(),
                                         mixed['bias1'].data_ptr(), mixed['biasr'].data_ptr(), None, None, n, S,
                                         None, None, None, None, 0, vd_enc[sl].data_ptr(), None, None, mixed['head'],
                                         density[sl].data_ptr(), rgbs[sl].data_ptr(), None, None, None, feat_flags, st))
    # early-termination compaction (`Model.compact_min_weight`): the last level of a march that returns no per-sample history (no `coord`)
    elif not is_prop and out.coord is None and model.compact_min_weight > 0 and mlp.mlp_mode == 1:
        composite = posts.entry(lib, 'ucn_composite')
        bg, opaque = float(model.bg_intensity_range[0]), int(bool(model.opaque_background))
        def run(fb, sl, r0, n):
            # density head -> weights of this pass's rays -> alive list -> colour layers of the alive samples
            _lib.check(lib.ucn_field_mlp(ctypes.byref(desc), fb.data_ptr(), n * S, S, rf, None, density[sl].data_ptr(),
                                         None, None, st))
            _lib.check(composite(density[sl].data_ptr(), None, *posts.compositing(sl), rays.d[sl].data_ptr(), bg, opaque,
                                 n, S, weights[sl].data_ptr(), main[sl].data_ptr(), None, st))
            if getattr(model, '_alive_idx', None) is None or model._alive_idx.numel() < n * S or model._alive_idx.device != dev:
                model._alive_idx = torch.empty(max(n, nc) * S, dtype=torch.int32, device=dev)
                model._alive_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(lib.ucn_compact_alive(weights[sl].data_ptr(), n, S, rf, float(model.compact_min_weight),
                                             model._alive_idx.data_ptr(), model._alive_cnt.data_ptr(), st))
            rgbs[sl].zero_()
            _lib.check(lib.ucn_field_rgb_compacted(ctypes.byref(desc), fb.data_ptr(), n * S, S, rf,
                                                   dirb[r0 * dir_row:].data_ptr(), model._alive_idx.data_ptr(),
                                                   model._alive_cnt.data_ptr(), rgbs[sl].data_ptr(), st))
            stats = getattr(model, '_alive_stats', None)
            if stats is not None:                              # diagnostics (tools/alive_fraction.py): forces a sync
                stats.append((int(model._alive_cnt.item()), n * S))
    else:
        def run(fb, sl, r0, n):
            _lib.check(lib.ucn_field_mlp(
                ctypes.byref(desc), fb.data_ptr(), n * S, S, rf | co,
                None if rgbs is None else dirb[r0 * dir_row:].data_ptr(),
                density[sl].data_ptr(), None if rgbs is None else rgbs[sl].data_ptr(), None, st))
    return run


def _gather(model, mlp, desc, posts, rays, flip, spin, S, layout, coord):
    """The level's featurisation as gather(fb, sl, n, stream): ucn_march_features of the n rays `sl` into `fb` (and their `coord`), then,
    with scale_featurization, the scale planes of these n * S samples behind its L grid planes."""
    lib, field = _lib.load(), ctypes.byref(desc)
    L, C, std, lpb = mlp.encoder.num_levels, mlp.encoder.level_dim, model.std_scale, int(model.levels_per_block)
    level_scale = mlp.level_scale() if mlp.scale_featurization else None           # once per level, not per pass

    def gather(fb, sl, n, stream):
        _lib.check(posts.ray_call(lib, 'ucn_march_features', field, rays, flip, spin, sl, std, mlp.warp, n, S, lpb, layout, fb.data_ptr(),
                                  None if coord is None else coord[sl].data_ptr(), None, stream.cuda_stream))
        if level_scale is not None:
            _lib.check(posts.ray_call(lib, 'ucn_march_scale_features', field, rays, flip, spin, sl, std, mlp.warp, n, S,
                                      level_scale.data_ptr(), layout & 3, fb[L * n * S * C:].data_ptr(), stream.cuda_stream))
    return gather


def _tails(model, mlp, desc, out, posts, rays, flip, spin, S, layout):
    """The per-sample passes behind a level's dense layers, on their stream, as callables tail(fb, sl, n) in the order they run; each
    closes over its head or descriptor, composed once per level, not per pass.  For every sample (compacted or not), when something returns
    their outputs -- and always for the diffuse head, which changes the colours."""
    # The ORDER is load-bearing.  ucn_ref_heads and ucn_pred_normals read all of the pass's feature planes (grid and scale) as the gather
    # wrote them -- the dense layers leave them intact; density_normals overwrites the grid planes in place (they become d raw_density /
    # d features), so it comes behind every reader.  pred_normals stands behind it only because the two never meet: MLP.__init__ refuses
    # enable_pred_normals with disable_density_normals = False.  A new reader goes in front of density_normals.
    st, tails = _lib.stream(), []
    if mlp.ref_heads_mask() & mlp.HEAD_DIFFUSE or out.roughness is not None:
        ref_head, rgbs, roughness = mlp.ref_head(), out.rgbs, out.roughness
        tails.append(lambda fb, sl, n: ml.ref_heads(mlp, desc, ref_head, fb, sl, n, S, layout, rgbs, roughness, st))
    if out.raw_grad is not None:
        # (with _prof set the pass's "MLP" time includes the tails)
        field, std, raw_grad, normals = mlp.normals_field(), model.std_scale, out.raw_grad, out.normals
        tails.append(lambda fb, sl, n: ml.density_normals(mlp, posts, rays, flip, spin, sl, n, S, std, layout, fb, raw_grad, normals, st, field=field))
    if out.grad_pred is not None:
        pred_head, grad_pred, normals_pred = mlp.pred_head(), out.grad_pred, out.normals_pred
        tails.append(lambda fb, sl, n: ml.pred_normals(desc, pred_head, fb, sl, n, S, layout, grad_pred, normals_pred, st))
    return tails


def run_passes(model, i_level, passes, feat_floats, dev, overlap, gather, run_mlp, tails):
    """A level's passes [(i_pass, r0, n)] (`march_level.pass_plan`) through gather -> run_mlp -> tails.  Owns the feature buffer(s) of
    feat_floats floats, the side stream, the events between the two streams and the timing events of `model._prof`.

    overlap (`Model.overlap_streams`): two HIP streams and two buffers -- the gather of pass i+1 (L2-request / VALU bound) runs on `side`
    beside the MLP of pass i (MFMA bound) on the caller's stream `cur`; the hardware splits the CUs between the two kernels.  Per pass:
       1. side.wait_event(mlp_done of pass i-2)        the buffer's previous reader (from the third pass on)
       2. e0.record(side)                              [timed]
       3. gather(fb, sl, n, side)
       4. e1.record(side)                              [timed]
       5. ready.record(side); cur.wait_event(ready)
       6. m0.record(cur)                               [timed]
       7. run_mlp(fb, sl, r0, n)
       8. the tails
       9. mlp_done.record(cur)
      10. e2.record(cur)                               [timed]
    and behind the last pass cur.wait_stream(side).  Without overlap everything runs on `cur`, one buffer: steps 1, 5, 6 and 9 and the
    final wait do not exist, and m0 is e1 (the MLP starts where the gather ends).
    Timed = every `_prof_every`-th pass while `model._prof` is a list (bench.py's live per-kernel times): it gets (i_level, n, e0, e1, m0,
    e2) -- features e0..e1 on their stream, MLP and tails m0..e2.  An event record costs the queue ~10 us of idle time at a kernel boundary
    (around every pass that was 9 ms of a 470 ms frame, tools/frame_gaps.py): none is created or recorded beyond the above."""
    cur = side = torch.cuda.current_stream()
    feats = [torch.empty(feat_floats, device=dev)]
    if overlap:
        feats.append(torch.empty_like(feats[0]))
        if getattr(model, '_side_stream', None) is None:
            model._side_stream = torch.cuda.Stream()
        side = model._side_stream
        side.wait_stream(cur)
    prof = getattr(model, '_prof', None)
    prof_every = max(1, int(getattr(model, '_prof_every', 1)))
    mlp_done = [None, None]
    for i_pass, r0, n in passes:
        sl, fb = slice(r0, r0 + n), feats[i_pass % len(feats)]
        timed = prof is not None and ml.timed_pass(i_pass, prof_every)
        if timed:
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            m0 = torch.cuda.Event(enable_timing=True) if overlap else e1
        if overlap and mlp_done[i_pass % 2] is not None:
            side.wait_event(mlp_done[i_pass % 2])
        if timed:
            e0.record(side)
        gather(fb, sl, n, side)
        if timed:
            e1.record(side)
        if overlap:
            ready = torch.cuda.Event()
            ready.record(side)
            cur.wait_event(ready)
            if timed:
                m0.record(cur)
        run_mlp(fb, sl, r0, n)
        for tail in tails:
            tail(fb, sl, n)
        if overlap:
            mlp_done[i_pass % 2] = torch.cuda.Event()
            mlp_done[i_pass % 2].record(cur)
        if timed:
            e2.record(cur)
            prof.append((i_level, n, e0, e1, m0, e2))
    if overlap:
        cur.wait_stream(side)


def _dir_bias(desc, rays, st):
    """the per-ray direction terms of the field `desc`'s colour layers (ucn_field_dir_bias)"""
    lib = _lib.load()
    dirb = torch.empty(lib.ucn_field_dir_floats(ctypes.byref(desc), rays.N), device=rays.dev)
    _lib.check(lib.ucn_field_dir_bias(ctypes.byref(desc), rays.vd.data_ptr(), rays.N, dirb.data_ptr(), st))
    return dirb


def march(model, rand, batch, train_frac, compute_extras, eval_camidx, want_history):
    st = _lib.stream()
    rays = ml.Rays(batch, model.num_levels)
    N, dev, prefix = rays.N, rays.dev, rays.prefix
    model.last_march_route = 'fused'      # diagnostics / tests: the route of the last forward (train_graph: 'train_graph')
    dirb = _dir_bias(model.nerf_mlp.field(glo_fold=True), rays, st)          # a GLO field: zero codes folded into the colour layers
    renderings, ray_history = [], []
    posts = out = None
    gain = ml.ray_gain(model, batch, rays)                  # the RawNeRF exposure (None without batch['exposure_idx'])
    nerf_chunk = max(1, int(model.max_chunk_rays))
    row = lambda m, S: S * (m.encoder.num_levels + m.scale_planes()) * m.encoder.level_dim          # feature floats per ray
    nerf_row, n_vis = row(model.nerf_mlp, model.num_nerf_samples), getattr(model.config, 'vis_num_rays', 16)
    for i_level, is_prop, S, mlp, dilation in ml.level_plan(model, train_frac):
        desc = mlp.field(glo_fold=not is_prop)
        chunk, passes = ml.pass_plan(N, nerf_chunk, row(mlp, S), nerf_row, is_prop)
        # ---- random draws and fenceposts (resample -> cone basis -> metric fenceposts of a warped raydist_fn)
        posts, flip, spin = ml.fenceposts(model, rays, i_level, S, dilation, train_frac, rand, posts, None if out is None else out.weights, st)
        out = ml.LevelOutputs.allocate(mlp, N, S, dev, want_history, compute_extras)
        # a proposal field built with its colour layers (PropMLP.disable_rgb = False) has direction terms of its own
        level_dirb = _dir_bias(desc, rays, st) if is_prop and out.rgbs is not None else dirb
        mixed = mixed_level(model, mlp, is_prop, mlp.encoder.num_levels * mlp.encoder.level_dim)
        model._mixed_levels = getattr(model, '_mixed_levels', 0) + (mixed is not None)      # diagnostics / tests
        overlap = bool(model.overlap_streams) and N > chunk
        co = _lib.LAUNCH_CORESIDENT if (overlap and not is_prop and model.overlap_streams != 2) else 0     # launch shapes that share a CU (2: plain shapes, tails only)
        layout = ((2 if model.rays_fastest else 0) | co) if mixed is None else (2 | mixed['table_flag'] | (mixed['feat_flag'] if not is_prop else 0))
        run_mlp = mlp_route(model, mlp, is_prop, desc, mixed, out, rays, posts, level_dirb, co, min(chunk, N))
        gather = _gather(model, mlp, desc if mixed is None else mixed['desc'], posts, rays, flip, spin, S, layout, out.coord)
        tails = _tails(model, mlp, desc, out, posts, rays, flip, spin, S, layout & 3)
        run_passes(model, i_level, passes, min(chunk, N) * row(mlp, S), dev, overlap, gather, run_mlp, tails)
        # the level's background colours (drawn behind its MLP, models.py:256), then one launch: `rgbs` leaves it scaled by the gain
        bg, ray_bg = ml.background(model, rays, i_level, rand)
        ml.composite(posts, out.density, out.rgbs, rays.d, gain, ray_bg, bg, model.opaque_background, out.weights, out.main, out.extras, st)
        renderings.append(out.rendering(prefix, posts.sdist, n_vis))
        if want_history:
            ray_history.append(out.history(prefix, posts.sdist))
    if compute_extras:                                             # ref models.py:313-324
        ml.broadcast_final(renderings)
    if getattr(model.config, 'model_sky', False):                  # ref models.py:326-337
        _sky_tail(model, rays, renderings, rand)
    if getattr(model.config, 'brightness_correction', False):      # ref models.py:339-363
        _brightness_tail(model, batch, rays, renderings, eval_camidx)
    return renderings, ray_history


def _sky_tail(model, rays, renderings, rand):
    """every rendering's 'sky_rgbs': the sky NeRF on the rays, or with `Model.sky_min_background` on those whose background weight reaches it"""
    N, o, d, cam, far = rays.N, rays.o, rays.d, rays.cam, rays.far
    # inference under an active bf16 autocast: the sky NeRF's nn.Linear layers are bf16 in the reference
    model._sky_mixed = sky_mixed = bool(model.autocast_render and torch.is_autocast_enabled() and torch.get_autocast_dtype('cuda') == torch.bfloat16)
    if model.sky_min_background > 0 and not rand:
        bgw = 1 - renderings[-1]['weights'].reshape(N, -1).sum(dim=-1)
        keep = torch.nonzero(bgw >= model.sky_min_background).reshape(-1)      # host sync, like far[0] in render()
        sky = torch.zeros(N, 3, device=rays.dev)
        if keep.numel() == N:
            sky = model.skynerf.render(o, d, cam, far, mixed=sky_mixed)
        elif keep.numel():
            # far0 = 1.5 * far[0] of the FULL batch (models.py:329), not of the kept rays
            sky[keep] = model.skynerf.render(o[keep], d[keep], cam[keep], far[keep], far0=far.reshape(-1)[:1], mixed=sky_mixed)
        model._sky_kept = (int(keep.numel()), N)
    else:
        sky = model.skynerf.render(o, d, cam, far, mixed=sky_mixed)
    for r in renderings:
        r['sky_rgbs'] = sky


def _brightness_tail(model, batch, rays, renderings, eval_camidx):
    """every rendering's 'rgb' through its camera's colour-correction affine (ucn_apply_affine), the sky's blended in behind the last level's weights"""
    lib, st, N, dev = _lib.load(), _lib.stream(), rays.N, rays.dev
    with_sky = getattr(model.config, 'model_sky', False)
    if eval_camidx is None:
        cam_idx = batch['cam_idx'].reshape(N, -1)[:, 0]
    else:
        cam_idx = torch.as_tensor(eval_camidx).to(dev).reshape(-1)[:1]
    A, A_sky, row_of = model.brightness_corr.affines(cam_idx)
    last_w = renderings[-1]['weights'].reshape(N, -1)          # loop-leaked `rendering` (Appendix C.3)
    for r in renderings:
        rgb_in = r['rgb'].reshape(N, 3).contiguous()
        rgb_out = torch.empty(N, 3, device=dev)
        _lib.check(lib.ucn_apply_affine(rgb_in.data_ptr(), A.data_ptr(), _lib.ptr(row_of),
                                        last_w.data_ptr() if with_sky else None, last_w.shape[1],
                                        r['sky_rgbs'].data_ptr() if with_sky else None,
                                        _lib.ptr(A_sky), N, rgb_out.data_ptr(), st))
        # ref :356-359: [N,1,1,3] for training batches, [N,3] with eval_camidx
        r['rgb'] = rgb_out.reshape(N, 1, 1, 3) if eval_camidx is None else rgb_out
        full = A if row_of is None else A[row_of]
        r['affine_trans'] = full.reshape(-1, 3, 4).expand(N, 3, 4)
        if with_sky:
            full_s = A_sky if row_of is None else A_sky[row_of]
            r['affine_trans_sky'] = full_s.reshape(-1, 3, 4).expand(N, 3, 4)
