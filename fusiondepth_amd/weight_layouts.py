"""Host-side cache of kernel-side weight layouts: when a convolution may read a cached layout and when it must be re-derived, the
one-launch refresh behind the fused Adam kernel with its "late" side-stream half, and when an idle or dead layout is retired.

Parameters whose owner opted in (``enable_weight_cache``; the Trainer does) keep their layouts here.  A layout is re-derived when the
parameter was modified through torch (``_version``) or by the fused Adam kernel (the weights epoch, bumped by adam_step*), i.e. once
per optimiser step instead of once per launch (the six ResNet passes of the two micro-batches reuse the same weights).  Tensors that
did not opt in are re-laid-out on every call."""
import collections
import ctypes
import weakref

import torch

from . import _lib
from . import tuning
from ._lib import call, ptr, query, stream


class _Entry:
    __slots__ = ("stamp",        # _layout_stamp of the weights the buffer was derived from (or is being derived from by this call)
                 "buf",          # the layout buffer
                 "desc",         # conv descriptor (None: not refreshable by the plan)
                 "param",        # weakref(parameter)
                 "late",         # refreshed on the side stream
                 "last_use",     # weights epoch of the last use
                 "unplanned")    # left out of the plan while idle

    def __init__(self, stamp, buf, desc, w):
        self.stamp, self.buf, self.desc, self.param = stamp, buf, desc, weakref.ref(w)
        self.late, self.last_use, self.unplanned = False, _weights_epoch, False


# one half (early / late) of the plan: the device job table of one fd_relayout_batch launch and the cache keys it refreshes
_PlanPart = collections.namedtuple("_PlanPart", "table n_jobs blocks keys")

_weights_epoch = 0
_frozen_epoch = 0
_next_cache_id = 1
_entries = {}             # (cache id, kind, layout floats) -> _Entry
_retired = []             # replaced layout buffers / job tables: a captured hipGraph may still hold their raw pointers
_plan = None              # (early _PlanPart or None, late _PlanPart or None)
_plan_stale = False

# The re-layout launch that follows the Adam kernel is pure HBM traffic (~0.5 GB: every 3x3 weight in its forward and its
# data-gradient layout, the F(2x2, 3x3) ones at 16 floats per tap) with nothing to overlap it on the stream that just finished the
# step.  Only the small forward layouts of the first layers are needed at once; everything else ("late": data-gradient layouts,
# forward layouts from 1 MB up = ResNet layer3 / layer4 and the decoder's deep blocks) is refreshed on a side stream while the next
# step's stems and first blocks run, and a stream that is about to USE a late layout waits for that launch first
# (``weight_layout``), as does the next optimiser step before it changes the weights again.  tuning.host.late_relayout = False: one launch.
_LATE_MIN_FLOATS = 1 << 18
_late_event = None        # recorded behind the pending side-stream re-layout
_late_waited = set()      # the streams that already wait for it
_late_stream = None

# A trained weight keeps one layout per input shape it was used at (the stacked training batch AND the validation batch: the format
# depends on the kernel family).  A layout that no convolution has used for _PLAN_IDLE_STEPS optimiser steps stays OUT of the per-step
# refresh - it is re-derived lazily by its next user through the stamp mismatch, which also drops the plan so that the layout is
# refreshed with the others again while it stays in use (a validation pass of several batches: one rebuild, then one launch per step) -
# and after _RETIRE_IDLE_STEPS its buffer is released (a rare shape no longer costs traffic and memory on every step).
_PLAN_IDLE_STEPS = 8
_RETIRE_IDLE_STEPS = 512


def has_plan():
    return _plan is not None


def layout_buffers():
    """Every cached layout buffer (memory a recorded call sequence may point into)."""
    return [e.buf for e in _entries.values()]


def layout_buffer(key):
    e = _entries.get(key)
    return e.buf if e is not None else None


def late_stream():
    return _late_stream


def late_event():
    """The event behind the pending side-stream re-layout, or None."""
    return _late_event


def frozen_epoch():
    return _frozen_epoch


def epoch_fingerprint(frozen_only):
    """What a recorded call sequence that reads cached layouts was valid for (``frozen_only``: it reads no trained weight)."""
    return (_frozen_epoch, 0 if frozen_only else _weights_epoch)


def is_frozen(p):
    return getattr(p, "_fd_frozen", False)


def unfreeze(p):
    """A formerly frozen parameter that something will change now: back under the optimiser epoch."""
    if is_frozen(p):
        p._fd_frozen = False
        _drop_plan()


def _drop_plan():
    global _plan
    if _plan is not None:
        _retired.extend(part.table for part in _plan if part is not None)
        _plan = None
    sync_late_layouts(host=True)


def _late_relayout_on():
    return tuning.host.late_relayout and not torch.cuda.is_current_stream_capturing()


def wait_late_layouts():
    """Order the current stream behind the pending side-stream re-layout (once per stream and optimiser step)."""
    if _late_event is None:
        return
    sid = stream()
    if sid not in _late_waited:
        torch.cuda.current_stream().wait_event(_late_event)
        _late_waited.add(sid)


def sync_late_layouts(host=False):
    """Order the current stream behind a pending side-stream re-layout and forget it (call before capturing a hipGraph, before
    touching the cached layouts from outside).  ``host``: wait on the host as well - for callers in the middle of a step (a new
    layout shape dropped the plan), where other streams may be about to use a late layout without passing through the current
    stream first."""
    global _late_event, _late_waited
    if _late_event is not None:
        if host and not torch.cuda.is_current_stream_capturing():
            _late_event.synchronize()
        torch.cuda.current_stream().wait_event(_late_event)
        _late_event = None
        _late_waited = set()


def evict_dead_weight_layouts():
    """Forget the layouts of parameters that no longer exist (a Trainer that was deleted): their buffers move to the retired
    list instead of being freed at once, because a hipGraph captured by that Trainer may still reference them; returns the
    number of entries dropped.  ``release_retired_layouts()`` frees the list once no such graph can be replayed any more."""
    dead = [k for k, e in _entries.items() if e.param() is None]
    for k in dead:
        _retired.append(_entries.pop(k).buf)
    if dead:
        _drop_plan()
    return len(dead)


def release_retired_layouts():
    n = len(_retired)
    _retired.clear()
    return n


def bump_weights_epoch():
    global _weights_epoch
    _weights_epoch += 1


def invalidate_frozen_layouts():
    """Frozen weights' layouts ignore the per-optimiser-step epoch; their stamp is (``_version``, this epoch, ``data_ptr``).  A write that
    torch's version counter does not see - ``p.data.copy_``, a broadcast into ``p.data``, a raw kernel - must be followed by this call
    (``weights_replaced`` does it): every frozen layout is re-derived at its next use."""
    global _frozen_epoch
    _frozen_epoch += 1


def weights_replaced():
    """Weights were written behind torch's back (a checkpoint copied into ``p.data``, a broadcast): no cached layout, trained or
    frozen, is current any more."""
    bump_weights_epoch()
    invalidate_frozen_layouts()


def enable_weight_cache(params, frozen=False):
    """``frozen``: weights that no optimiser touches (the Refiner's stage-1 networks).  Their layouts are derived once and stay valid
    across optimiser steps (the epoch stamp that invalidates trained weights' layouts after every Adam launch is ignored; an in-place
    change through torch - ``load_state_dict`` - still bumps ``_version``), and they stay out of the post-Adam refresh launch.
    Round 4 re-laid them out on EVERY call: 100 launches per Refiner step."""
    global _next_cache_id
    for p in params:
        if p.dim() == 4 and not hasattr(p, "_fd_cache_id"):
            p._fd_cache_id = _next_cache_id
            _next_cache_id += 1
        if p.dim() == 4:
            if frozen:
                p._fd_frozen = True
            else:
                unfreeze(p)


def _layout_stamp(w):
    if is_frozen(w):
        return (w._version, -1 - _frozen_epoch, w.data_ptr())
    return (w._version, _weights_epoch, w.data_ptr())


def weight_layout(w, cache_id, kind, nfloats, desc=None):
    """-> (buffer, ready flag) for weight ``w`` and layout ``kind`` ('f' forward, 'd' data-gradient)."""
    if cache_id is None:
        return torch.empty((nfloats,), device=w.device, dtype=torch.float32), 0
    # nfloats is part of the key: the layout FORMAT of a weight depends on the kernel family its input shape is routed to (12 or 16
    # floats per tap: conv_wino_route.hip::wino_fwd_mode looks at N*H*W), so a weight used at two batch sizes (the stacked training batch and
    # a smaller validation batch) keeps both layouts resident instead of rebuilding one over the other on every switch
    key = (cache_id, kind, nfloats)
    stamp = _layout_stamp(w)
    ent = _entries.get(key)
    if _lib.RECORDER[0] is not None:
        _lib.RECORDER[0].side("layout", (w, key))
    if ent is not None:
        if _late_event is not None and ent.late:
            wait_late_layouts()
        if ent.unplanned and not is_frozen(w) and _weights_epoch - ent.last_use > _PLAN_IDLE_STEPS:
            _drop_plan()                # it left the per-step refresh while idle and is in use again: let the next plan include it
        ent.last_use = _weights_epoch
        if ent.stamp == stamp:
            return ent.buf, 1
        ent.stamp = stamp
        return ent.buf, 0
    buf = torch.empty((nfloats,), device=w.device, dtype=torch.float32)
    _entries[key] = _Entry(stamp, buf, desc, w)
    if not is_frozen(w):
        _drop_plan()                    # a layout the plan does not know: fall back to per-call re-layout until rebuilt
    return buf, 0


def use_if_current(key, w, data_ptr):
    """For a recorded call sequence that read the layout ``key`` of ``w`` at ``data_ptr``: None if it has to be re-derived (the
    sequence cannot be replayed), otherwise the layout is marked used and the result says whether it is refreshed late."""
    ent = _entries.get(key)
    if ent is None or ent.stamp != _layout_stamp(w) or ent.buf.data_ptr() != data_ptr:
        return None
    ent.last_use = _weights_epoch
    return ent.late


# One-launch refresh of every cached layout (fd_relayout_batch): built once the cache is populated (after the first full
# forward + backward), run by adam_step* right after the weights change.
def build_weight_plan():
    """Collect the re-layout jobs of every cached weight layout into a device table; returns the number of jobs."""
    global _plan, _plan_stale
    evict_dead_weight_layouts()
    _plan_stale = False
    now = _weights_epoch
    for k in [k for k, e in _entries.items() if now - e.last_use > _RETIRE_IDLE_STEPS and not is_frozen(e.param())]:
        _retired.append(_entries.pop(k).buf)
    ents = []
    for k, e in _entries.items():
        if e.desc is None or is_frozen(e.param()):
            continue
        e.unplanned = now - e.last_use > _PLAN_IDLE_STEPS
        if not e.unplanned:
            ents.append((k, e))
    if not ents:
        _drop_plan()
        return 0
    def table(part):
        if not part:
            return None
        jobs = (_lib.RelayoutJob * (4 * len(part)))()
        n = 0
        for (cid, kind, _nf), e in part:
            n += query("fd_conv2d_relayout_jobs", ctypes.addressof(e.desc), 0 if kind == "f" else 1, ptr(e.param()), ptr(e.buf),
                       ctypes.addressof(jobs) + n * ctypes.sizeof(_lib.RelayoutJob))
        if n == 0:
            return None
        blocks = query("fd_relayout_plan", ctypes.addressof(jobs), n)
        raw = bytes(memoryview(jobs))[: n * ctypes.sizeof(_lib.RelayoutJob)]
        dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(part[0][1].buf.device)
        return _PlanPart(dev, n, blocks, [k for k, _ in part])
    for k, e in ents:
        e.late = k[1] != "f" or e.buf.numel() >= _LATE_MIN_FLOATS
    early = table([(k, e) for k, e in ents if not e.late])
    late = table([(k, e) for k, e in ents if e.late])
    _drop_plan()
    n_jobs = sum(part.n_jobs for part in (early, late) if part is not None)
    if n_jobs:
        _plan = (early, late)
    return n_jobs


def refresh_weight_layouts():
    """Re-derive every planned layout from the current weights (one launch) and mark them valid for this epoch."""
    global _plan_stale, _late_event, _late_waited, _late_stream
    if _plan is None:
        return False
    early, late = _plan
    sync_late_layouts()                        # (a refresh without an optimiser step in between: never two in flight)
    for part in (early, late):
        if part is None:
            continue
        if part is late and _late_relayout_on():
            cur = torch.cuda.current_stream()
            if _late_stream is None:
                _late_stream = torch.cuda.Stream()
            side = _late_stream
            side.wait_stream(cur)              # behind the Adam kernel (and everything that read the old layouts)
            with torch.cuda.stream(side):
                call("fd_relayout_batch", ptr(part.table), part.n_jobs, part.blocks, stream())
                ev = torch.cuda.Event()
                ev.record(side)
            _late_event, _late_waited = ev, set()
        else:
            call("fd_relayout_batch", ptr(part.table), part.n_jobs, part.blocks, stream())
        for k in part.keys:
            e = _entries[k]
            w = e.param()
            if w is not None:
                e.stamp = _layout_stamp(w)
            if _weights_epoch - e.last_use > _PLAN_IDLE_STEPS:
                _plan_stale = True             # refreshed, but nobody has read it for a while: the owner rebuilds the plan without it
    return True


def weight_plan_needs_rebuild():
    """No plan yet, or the plan carries layouts that have gone idle (``_PLAN_IDLE_STEPS``): ``build_weight_plan`` leaves those out."""
    return _plan is None or _plan_stale


def rebuild_weight_plan():
    """Build the plan; a FIRST plan is followed by one refresh, so that every layout it covers is valid from now on."""
    had_plan = _plan is not None
    if build_weight_plan() > 0 and not had_plan:
        refresh_weight_layouts()
