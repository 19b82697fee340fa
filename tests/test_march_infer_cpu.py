"""The host side of the inference march without a GPU or the library: march_level.pass_plan against the chunk rule written out here,
the timed-pass rule, LevelOutputs.allocate against a table of the conditions under which the march has each buffer, and
march_infer.run_passes' sequence of stream operations, recorded by fakes of torch.cuda's streams and events."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from ucnerf_amd.internal import march_infer as mi
from ucnerf_amd.internal import march_level as ml


def _check_plan(N, nerf_chunk, level_row, nerf_row, is_prop, want_chunk):
    chunk, passes = ml.pass_plan(N, nerf_chunk, level_row, nerf_row, is_prop)
    assert chunk == want_chunk
    assert [p[0] for p in passes] == list(range(len(passes)))
    covered = [r for _, r0, n in passes for r in range(r0, r0 + n)]
    assert covered == list(range(N))                                   # [0, N) exactly once and in order
    assert all(0 < n <= chunk for _, _, n in passes) and all(n == chunk for _, _, n in passes[:-1])


@pytest.mark.parametrize("N", [0, 1, 31, 32, 33, 96])
@pytest.mark.parametrize("is_prop", [False, True])
def test_pass_plan_small(N, is_prop):
    level_row, nerf_row = 64 * 5 * 2, 32 * 10 * 4                      # a proposal level's shorter row: the ratio is 2
    assert 32 * nerf_row // level_row // 256 * 256 == 0                # the multiple-of-256 term vanishes: the chunk stays nerf_chunk
    _check_plan(N, 32, level_row, nerf_row, is_prop, 32)
    assert len(ml.pass_plan(N, 32, level_row, nerf_row, is_prop)[1]) == -(-N // 32)
    assert ml.pass_plan(0, 32, level_row, nerf_row, is_prop)[1] == []


def test_pass_plan_proposal_chunks():
    _check_plan(10000, 1024, 100, 400, True, 4096)                     # nerf_row = 4 * level_row
    _check_plan(10000, 1024, 100, 400, False, 1024)                    # the NeRF level never widens
    _check_plan(10000, 1024, 400, 400, True, 1024)                     # nor does a proposal level whose row is as long
    _check_plan(10000, 1024, 401, 400, True, 1024)
    _check_plan(200000, 10240, 100, 1700, True, 1 << 16)               # 174080 capped
    _check_plan(5000, 1000, 100, 330, True, 3072)                      # 3300 rounded down to a multiple of 256
    for nerf_chunk, level_row, nerf_row in itertools.product((1, 32, 1000, 10240, 100000), (7, 640, 1280), (640, 1280, 40960)):
        want = nerf_chunk
        if level_row < nerf_row:
            want = max(nerf_chunk, min(nerf_chunk * nerf_row // level_row // 256 * 256, 1 << 16))
        _check_plan(3 * want + 5, nerf_chunk, level_row, nerf_row, True, want)


@pytest.mark.parametrize("p", [1, 2, 30])
def test_timed_passes(p):
    assert {i for i in range(7) if ml.timed_pass(i, p)} == {i for i in range(7) if i % p == p // 2}


# ------------------------------------------------------------------ LevelOutputs
ROUGH = 4
FIELDS = dict(plain=dict(), density_normals=dict(disable_density_normals=False), pred_normals=dict(enable_pred_normals=True),
              rough_diffuse=dict(mask=1 | ROUGH))


def _field(disable_rgb=False, disable_density_normals=True, enable_pred_normals=False, mask=0):
    return SimpleNamespace(disable_rgb=disable_rgb, disable_density_normals=disable_density_normals, enable_pred_normals=enable_pred_normals,
                           HEAD_ROUGHNESS=ROUGH, ref_heads_mask=lambda: mask)


@pytest.mark.parametrize("field", sorted(FIELDS))
@pytest.mark.parametrize("compute_extras", [False, True])
@pytest.mark.parametrize("want_history", [False, True])
def test_level_outputs_allocate(want_history, compute_extras, field):
    N, S = 5, 3
    out = ml.LevelOutputs.allocate(_field(**FIELDS[field]), N, S, "cpu", want_history, compute_extras)
    returned = want_history or compute_extras
    want = dict(density=(N, S), rgbs=(N, S, 3), weights=(N, S), main=(N, 5))
    if compute_extras:
        want["extras"] = (N, 4)
    if want_history:
        want["coord"] = (N, S, 3)
    if field == "density_normals" and returned:
        want.update(raw_grad=(N, S, 3), normals=(N, S, 3))
    if field == "pred_normals" and returned:
        want.update(grad_pred=(N, S, 3), normals_pred=(N, S, 3))
    if field == "rough_diffuse" and returned:
        want["roughness"] = (N, S)
    got = {k: tuple(getattr(out, k).shape) for k in ml.LevelOutputs.__slots__ if getattr(out, k) is not None}
    assert got == want
    assert all(getattr(out, k).dtype == torch.float32 for k in got)


def test_level_outputs_of_a_proposal_level_without_colour_layers():
    out = ml.LevelOutputs.allocate(_field(disable_rgb=True), 5, 3, "cpu", True, True)
    assert out.rgbs is None and out.roughness is None and out.density.shape == (5, 3)
    with pytest.raises(AssertionError):
        ml.LevelOutputs(densities=None)


def test_level_outputs_dictionaries_equal_the_entry_functions():
    N, S, g = 6, 4, torch.Generator().manual_seed(5)
    r = lambda *s: torch.rand(*s, generator=g)
    kw = dict(density=r(N, S), rgbs=r(N, S, 3), weights=r(N, S), main=r(N, 5), extras=r(N, 4), coord=r(N, S, 3), raw_grad=r(N, S, 3),
              normals=r(N, S, 3), grad_pred=r(N, S, 3), normals_pred=r(N, S, 3), roughness=r(N, S))
    sdist, main = r(N, S + 1), kw["main"]
    same = lambda a, b: set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    for out in (ml.LevelOutputs(**kw), ml.LevelOutputs(**dict(kw, main=(main[:, :3], main[:, 3], main[:, 4])))):      # the kernel's buffer; the nodes' three
        assert same(out.rendering((2, 3), sdist, 4), ml.rendering_entry(main[:, :3], main[:, 3], main[:, 4], kw["weights"], kw["extras"], (2, 3), sdist,
                                                                       kw["rgbs"], 4, normals=kw["normals"], normals_pred=kw["normals_pred"],
                                                                       roughness=kw["roughness"]))
        assert same(out.history((2, 3), sdist), ml.history_entry(kw["coord"], kw["density"], kw["rgbs"], sdist, kw["weights"], (2, 3), kw["raw_grad"],
                                                                 kw["normals"], grad_pred=kw["grad_pred"], normals_pred=kw["normals_pred"],
                                                                 roughness=kw["roughness"]))
    bare = ml.LevelOutputs(density=kw["density"], weights=kw["weights"], main=main, coord=kw["coord"])
    assert set(bare.rendering((N,), sdist, 4)) == {"rgb", "depth", "acc", "weights"}
    h = bare.history((N,), sdist)
    assert not h["rgb"].any() and all(h[k] is None for k in ("raw_grad_density", "grad_pred", "normals", "normals_pred", "roughness"))


# ------------------------------------------------------------------ the pass loop's stream sequence
class _Stream:
    def __init__(self, log, name):
        self.log, self.name, self.cuda_stream = log, name, name

    def wait_event(self, event):
        self.log.append(("wait_event", self.name, event.name))

    def wait_stream(self, other):
        self.log.append(("wait_stream", self.name, other.name))


def _fake_cuda(monkeypatch):
    """torch.cuda's Stream, Event and current_stream replaced by recorders: the log of (op, stream, event) and the events made"""
    log, events = [], []

    class Event:
        def __init__(self, enable_timing=False):
            self.name, self.timing = f"ev{len(events)}", enable_timing
            events.append(self)

        def record(self, stream):
            log.append(("record", stream.name, self.name))
    cur = _Stream(log, "cur")
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: cur)
    monkeypatch.setattr(torch.cuda, "Stream", lambda: _Stream(log, "side"))
    monkeypatch.setattr(torch.cuda, "Event", Event)
    return log, events


def _run(log, model, overlap, n_tails=2, passes=((0, 0, 32), (1, 32, 32), (2, 64, 32))):
    buffers = []

    def gather(fb, sl, n, stream):
        buffers.append(fb.data_ptr())
        log.append(("gather", stream.cuda_stream, sl.start))
    run_mlp = lambda fb, sl, r0, n: log.append(("mlp", fb.data_ptr(), r0))
    tails = [lambda fb, sl, n, k=k: log.append((f"tail{k}", fb.data_ptr(), sl.start)) for k in range(n_tails)]
    mi.run_passes(model, 1, list(passes), 8, "cpu", overlap, gather, run_mlp, tails)
    return buffers


def test_stream_sequence_with_overlap(monkeypatch):
    log, events = _fake_cuda(monkeypatch)
    model = SimpleNamespace()
    b = _run(log, model, True)
    assert b[0] != b[1] and b[2] == b[0]                               # two feature buffers, alternating
    assert model._side_stream.name == "side"
    assert log == [
        ("wait_stream", "side", "cur"),
        # pass 0: nobody has read its buffer yet
        ("gather", "side", 0), ("record", "side", "ev0"), ("wait_event", "cur", "ev0"),
        ("mlp", b[0], 0), ("tail0", b[0], 0), ("tail1", b[0], 0), ("record", "cur", "ev1"),
        # pass 1: the other buffer
        ("gather", "side", 32), ("record", "side", "ev2"), ("wait_event", "cur", "ev2"),
        ("mlp", b[1], 32), ("tail0", b[1], 32), ("tail1", b[1], 32), ("record", "cur", "ev3"),
        # pass 2: the first buffer again, behind pass 0's MLP and tails (mlp_done = ev1)
        ("wait_event", "side", "ev1"),
        ("gather", "side", 64), ("record", "side", "ev4"), ("wait_event", "cur", "ev4"),
        ("mlp", b[0], 64), ("tail0", b[0], 64), ("tail1", b[0], 64), ("record", "cur", "ev5"),
        ("wait_stream", "cur", "side")]
    assert len(events) == 6 and not any(e.timing for e in events)
    side = model._side_stream
    _run(log, model, True)
    assert model._side_stream is side                                  # made once, kept on the model


def test_stream_sequence_with_overlap_and_timing(monkeypatch):
    log, events = _fake_cuda(monkeypatch)
    model = SimpleNamespace(_prof=[], _prof_every=1)
    b = _run(log, model, True, n_tails=1)
    want = [("wait_stream", "side", "cur")]
    for i, r0 in enumerate((0, 32, 64)):
        e0, e1, e2, m0, ready, done = (f"ev{6 * i + k}" for k in range(6))           # the order in which a pass makes them
        if i == 2:
            want.append(("wait_event", "side", "ev5"))                               # 1. pass 0's mlp_done
        want += [("record", "side", e0), ("gather", "side", r0), ("record", "side", e1),                 # 2. 3. 4.
                 ("record", "side", ready), ("wait_event", "cur", ready), ("record", "cur", m0),         # 5. 6.
                 ("mlp", b[i % 2], r0), ("tail0", b[i % 2], r0),                                         # 7. 8.
                 ("record", "cur", done), ("record", "cur", e2)]                                         # 9. 10.
    assert log == want + [("wait_stream", "cur", "side")]
    assert [(lvl, n) + tuple(e.name for e in ev) for lvl, n, *ev in model._prof] == [
        (1, 32, "ev0", "ev1", "ev3", "ev2"), (1, 32, "ev6", "ev7", "ev9", "ev8"), (1, 32, "ev12", "ev13", "ev15", "ev14")]
    assert [e.timing for e in events] == [True, True, True, True, False, False] * 3


def test_stream_sequence_without_overlap(monkeypatch):
    log, events = _fake_cuda(monkeypatch)
    model = SimpleNamespace()
    b = _run(log, model, False)
    assert len(set(b)) == 1 and not events and not hasattr(model, "_side_stream")
    assert log == [step for r0 in (0, 32, 64) for step in (("gather", "cur", r0), ("mlp", b[0], r0), ("tail0", b[0], r0), ("tail1", b[0], r0))]
    # timed: three events per timed pass, on the one stream; the MLP's interval starts where the gather's ends
    del log[:]
    model._prof, model._prof_every = [], 2
    b = _run(log, model, False, n_tails=0)
    assert log == [("gather", "cur", 0), ("mlp", b[0], 0),
                   ("record", "cur", "ev0"), ("gather", "cur", 32), ("record", "cur", "ev1"), ("mlp", b[0], 32), ("record", "cur", "ev2"),
                   ("gather", "cur", 64), ("mlp", b[0], 64)]
    assert len(events) == 3 and all(e.timing for e in events)
    (lvl, n, e0, e1, m0, e2), = model._prof
    assert (lvl, n) == (1, 32) and m0 is e1 and [e.name for e in (e0, e1, e2)] == ["ev0", "ev1", "ev2"]
    model._prof_every = 1
    _run(log, model, False)
    assert len(model._prof) == 4 and all(len(t) == 6 and t[4] is t[3] for t in model._prof)
    model._prof = None                                                 # bench.py's state after its timed frames: no events again
    n_events = len(events)
    _run(log, model, False)
    assert len(events) == n_events
