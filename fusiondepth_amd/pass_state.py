"""Host-side state of one forward / backward pass: which parameters accumulate their gradients in place and who is told when such a
gradient is complete, how often a parameter was used since the pass began, the decoder's side-stream weight gradients and the
tensors they keep alive, and the BatchNorm group count with its deferred ``num_batches_tracked`` updates.

functional.py's wrappers and replay.py's replayed nodes report to it; the Trainer and dp.py configure and read it.  Nothing here
launches a kernel."""
import weakref

import torch

from . import _lib
from .weight_layouts import unfreeze

_grad_ready_subs = []     # weak references to the bound callbacks of live subscribers (one per GradientSynchronizer with world > 1)
_param_uses = {}          # id(param) -> number of forward uses since begin_forward_pass() (a network may run twice per pass)
_wgrad_streams = {}       # issuing stream -> its side stream
_wgrad_keepalive = []     # what the side-stream kernels read, until join_wgrad_streams()
_bn_groups = 1
_bn_counters = None       # the pending (counter, groups) updates inside defer_bn_counters, else None


def enable_direct_grad(params):
    """Opt-in: weight / bias / BatchNorm-affine gradients are accumulated by the backward kernels straight into the
    pre-allocated ``param.grad`` (a view of the trainer's flat gradient buffer) instead of being returned to autograd,
    which would launch one ATen add per parameter per micro-batch (~600 tiny kernels per optimiser step)."""
    for p in params:
        p._fd_direct_grad = True
        unfreeze(p)                                        # it gets gradients, so something will change it


def direct_grad_target(p):
    if p is not None and getattr(p, "_fd_direct_grad", False) and p.grad is not None and p.grad.is_contiguous():
        return p.grad
    return None


def has_direct_grad(p):
    """The backward kernels accumulate this parameter's gradient in place (``enable_direct_grad`` and a contiguous ``p.grad``)."""
    return direct_grad_target(p) is not None


# ---- "this parameter's gradient is complete" notifications ------------------------------------------------------------------
# With in-place accumulation autograd never sees a parameter gradient, so post-accumulate hooks do not fire.  The backward
# wrappers call this right after LAUNCHING the kernel that finishes a parameter's gradient; dp.GradientSynchronizer uses it to
# issue a bucket's all-reduce behind that kernel on the same stream while the rest of the backward pass is still being issued.
def add_grad_ready_callback(bound_method):
    """Subscribe ``bound_method(param)``.  Held weakly: a deleted trainer's synchroniser (and its flat buffers) is not kept
    alive by this module, and several trainers in one process (a Trainer and a Refiner, two Trainers) each keep their overlap -
    every subscriber is told about every parameter and ignores the ones it does not own."""
    _grad_ready_subs.append(weakref.WeakMethod(bound_method))


def _live_grad_ready():
    live = [(r, r()) for r in _grad_ready_subs]
    if any(cb is None for _, cb in live):
        _grad_ready_subs[:] = [r for r, cb in live if cb is not None]
    return [cb for _, cb in live if cb is not None]


def begin_forward_pass():
    """Start counting parameter uses afresh: the backward pass of this forward runs one gradient kernel per use.  Side-stream
    weight gradients of a previous backward pass that nobody joined (a caller driving process_batch + backward itself, without
    Trainer._join_side_streams) are joined here, so that the tensors they keep alive are released at the latest one pass later."""
    _param_uses.clear()
    if _wgrad_keepalive:
        join_wgrad_streams()


def param_uses(p):
    return _param_uses.get(id(p), 1)


def note_use(*params):
    if _lib.RECORDER[0] is not None:
        _lib.RECORDER[0].side("note_use", params)
    if _grad_ready_subs:
        for p in params:
            if p is not None:
                _param_uses[id(p)] = _param_uses.get(id(p), 0) + 1


def grad_ready(*params):
    rec = _lib.RECORDER[0]
    if rec is not None:
        rec.side("grad_ready", params)
        if rec.mute_grad_ready:
            return                      # an isolated recording pass: its gradients are thrown away, nobody may be told
    if _grad_ready_subs:
        for cb in _live_grad_ready():
            for p in params:
                if p is not None:
                    cb(p)


# ---- weight gradients of the decoder on a side stream -----------------------------------------------------------------------
# Decoder -> loss -> decoder is the serial section of the step: one kernel at a time on the main stream, at batch 12 and 16-128
# channels, while the encoder streams have little or nothing to run.  In a conv's backward only the data gradient feeds the next
# layer; the weight gradient (+ its slab reduction + the bias sums) is a leaf, so for parameters marked by ``enable_side_wgrad`` it
# is issued on ONE side stream per issuing stream.  The tensors those kernels read are kept alive until ``join_wgrad_streams``
# (the caching allocator would otherwise hand their memory to later kernels of the issuing stream).  Round 2's FD_ASYNC_WGRAD did
# this for EVERY convolution - slower (the encoders' streams already fill the chip) and its notifications were given on the wrong
# stream; this is the decoder only, opt-in per parameter.
def enable_side_wgrad(params, on=True):
    for p in params:
        if p.dim() == 4:
            p._fd_side_wgrad = bool(on)


def has_side_wgrad(p):
    return getattr(p, "_fd_side_wgrad", False)


def wgrad_stream():
    """The side stream of the current stream, ordered behind everything queued on it so far."""
    cur = torch.cuda.current_stream()
    st = _wgrad_streams.get(cur.cuda_stream)
    if st is None:
        st = _wgrad_streams[cur.cuda_stream] = torch.cuda.Stream()
    st.wait_stream(cur)
    return st


def keep_until_wgrad_join(*tensors):
    """What a side-stream weight gradient reads: held until ``join_wgrad_streams``."""
    _wgrad_keepalive.append(tensors)


def pending_side_wgrads():
    """Number of side-stream weight gradients issued since the last join (0: nothing to join)."""
    return len(_wgrad_keepalive)


def join_wgrad_streams():
    """Order every side-stream weight gradient before what follows on the current stream (optimiser / all-reduce)."""
    if not _wgrad_streams:
        return
    cur = torch.cuda.current_stream()
    for st in _wgrad_streams.values():
        cur.wait_stream(st)
    _wgrad_keepalive.clear()


# ---- BatchNorm groups and step counters -------------------------------------------------------------------------------------
def current_bn_groups():
    return _bn_groups


def bump_bn_counter(counter, groups):
    """``num_batches_tracked += groups`` - deferred to one multi-tensor launch inside ``defer_bn_counters``; reported to an active call
    recorder (replay.py replays the bump with the network's recorded calls)."""
    rec = _lib.RECORDER[0]
    if rec is not None:
        rec.side("bn_counter", (counter, groups))
    if _bn_counters is not None:
        _bn_counters.append((counter, groups))
    else:
        counter.add_(groups)


class defer_bn_counters:
    """Collect the ``num_batches_tracked += groups`` updates of every BatchNorm called inside the block and apply them
    with ONE multi-tensor launch on exit (80 one-element ATen kernels per optimiser step otherwise)."""

    def __enter__(self):
        global _bn_counters
        self.prev = _bn_counters
        _bn_counters = []
        return self

    def __exit__(self, *exc):
        global _bn_counters
        pending, _bn_counters = _bn_counters, self.prev
        if pending and exc[0] is None:
            torch._foreach_add_([t for t, _ in pending], [int(g) for _, g in pending])
        return False


class bn_groups:
    """``with bn_groups(G):`` every training-mode BatchNorm inside treats its batch as G consecutive sub-batches that are
    normalised (and tracked in the running statistics) independently, i.e. exactly like G separate forward passes."""

    def __init__(self, groups):
        self.groups = int(groups)

    def __enter__(self):
        global _bn_groups
        self.prev = _bn_groups
        _bn_groups = self.groups

    def __exit__(self, *a):
        global _bn_groups
        _bn_groups = self.prev
