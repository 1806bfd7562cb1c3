"""fusiondepth_amd.pass_state on the CPU: the BatchNorm group count and deferred counters, the use counts, the weakly held
gradient-ready subscribers and the direct-gradient predicate.  No kernel is launched."""
import gc

import pytest
import torch

from fusiondepth_amd import pass_state as PS


class _Owner:
    def __init__(self):
        self.seen = []

    def on_grad(self, p):
        self.seen.append(p)


@pytest.fixture(autouse=True)
def own_subscribers():
    """Each test starts without subscribers and use counts and leaves the module as it found it."""
    subs, uses = list(PS._grad_ready_subs), dict(PS._param_uses)
    PS._grad_ready_subs.clear()
    PS._param_uses.clear()
    yield
    PS._grad_ready_subs[:] = subs
    PS._param_uses.clear()
    PS._param_uses.update(uses)


def test_bn_groups_nest_and_restore():
    assert PS.current_bn_groups() == 1
    with PS.bn_groups(3):
        assert PS.current_bn_groups() == 3
        with PS.bn_groups(2):
            assert PS.current_bn_groups() == 2
        assert PS.current_bn_groups() == 3
        with pytest.raises(ValueError):
            with PS.bn_groups(2):
                assert PS.current_bn_groups() == 2
                raise ValueError("inner")
        assert PS.current_bn_groups() == 3
    assert PS.current_bn_groups() == 1


def test_defer_bn_counters_applies_on_exit():
    c = torch.zeros((), dtype=torch.int64)
    with PS.defer_bn_counters():
        PS.bump_bn_counter(c, 2)
        assert int(c) == 0
    assert int(c) == 2
    PS.bump_bn_counter(c, 3)                    # outside a block: at once
    assert int(c) == 5


def test_defer_bn_counters_drops_the_bumps_of_a_block_that_raises():
    c, d = torch.zeros((), dtype=torch.int64), torch.zeros((), dtype=torch.int64)
    with PS.defer_bn_counters():
        PS.bump_bn_counter(d, 1)
        with pytest.raises(ValueError):
            with PS.defer_bn_counters():
                PS.bump_bn_counter(c, 2)
                raise ValueError("inner")
        assert int(c) == 0
        PS.bump_bn_counter(d, 1)                # the outer collector is back: still deferred
        assert int(d) == 0
    assert int(c) == 0 and int(d) == 2
    PS.bump_bn_counter(c, 1)                    # and no collector is left behind
    assert int(c) == 1


def test_defer_bn_counters_nested_blocks_apply_their_own_bumps():
    c, d = torch.zeros((), dtype=torch.int64), torch.zeros((), dtype=torch.int64)
    with PS.defer_bn_counters():
        PS.bump_bn_counter(c, 2)
        with PS.defer_bn_counters():
            PS.bump_bn_counter(d, 3)
            assert int(c) == 0 and int(d) == 0
        assert int(c) == 0 and int(d) == 3
    assert int(c) == 2 and int(d) == 3


def test_use_counts():
    owner = _Owner()
    PS.add_grad_ready_callback(owner.on_grad)
    p = torch.nn.Parameter(torch.zeros(2))
    PS.begin_forward_pass()
    PS.note_use(p, None)
    PS.note_use(p)
    assert PS.param_uses(p) == 2
    PS.begin_forward_pass()
    assert PS.param_uses(p) == 1


def test_nothing_is_counted_without_a_subscriber():
    p = torch.nn.Parameter(torch.zeros(2))
    PS.begin_forward_pass()
    PS.note_use(p, None)
    PS.note_use(p)
    assert PS.param_uses(p) == 1 and not PS._param_uses
    PS.grad_ready(p, None)                      # nobody to tell: no error


def test_subscribers_are_held_weakly():
    p = torch.nn.Parameter(torch.zeros(2))
    owner = _Owner()
    seen = owner.seen
    PS.add_grad_ready_callback(owner.on_grad)
    PS.grad_ready(p, None)
    assert len(seen) == 1 and seen[0] is p
    del owner
    gc.collect()
    PS.grad_ready(p, None)
    assert len(seen) == 1
    assert PS._live_grad_ready() == [] and not PS._grad_ready_subs


def test_direct_gradient_predicate():
    p = torch.nn.Parameter(torch.zeros(3, 2))
    assert not PS.has_direct_grad(p)
    p.grad = torch.zeros(3, 2)
    assert not PS.has_direct_grad(p)            # not opted in
    PS.enable_direct_grad([p])
    assert PS.has_direct_grad(p) and PS.direct_grad_target(p) is p.grad
    p.grad = None
    assert not PS.has_direct_grad(p) and PS.direct_grad_target(p) is None
    assert not PS.has_direct_grad(None)
