"""The host-side cache of kernel-side weight layouts (fusiondepth_amd/weight_layouts.py) on CPU tensors: when a cached layout is
reported ready, what invalidates it, and how the layouts of a dead parameter are retired.  No library call is made."""
import gc

import torch

from fusiondepth_amd import weight_layouts as WL


def test_ready_flag_invalidation_and_retirement():
    WL.evict_dead_weight_layouts(); WL.release_retired_layouts()
    w = torch.nn.Parameter(torch.randn(8, 16, 3, 3))
    wf = torch.nn.Parameter(torch.randn(8, 16, 3, 3))
    WL.enable_weight_cache([w])
    WL.enable_weight_cache([wf], frozen=True)
    assert w._fd_cache_id != wf._fd_cache_id and WL.is_frozen(wf) and not WL.is_frozen(w)
    ask = lambda p, kind="f", n=1152: WL.weight_layout(p, p._fd_cache_id, kind, n)

    buf, ready = ask(w)
    assert ready == 0 and buf.shape == (1152,) and buf.dtype == torch.float32
    assert ask(w)[1] == 1 and ask(w)[0] is buf
    WL.bump_weights_epoch()                      # the fused Adam kernel changed the weights
    assert (ask(w)[1], ask(w)[1]) == (0, 1) and ask(w)[0] is buf
    with torch.no_grad():
        w.mul_(2.0)                              # torch changed them
    assert (ask(w)[1], ask(w)[1]) == (0, 1) and ask(w)[0] is buf
    other_n, other_kind = ask(w, n=1536), ask(w, kind="d")
    assert other_n[1] == 0 and other_kind[1] == 0
    assert len({buf.data_ptr(), other_n[0].data_ptr(), other_kind[0].data_ptr()}) == 3

    fbuf, ready = ask(wf)
    assert ready == 0 and ask(wf)[1] == 1
    WL.bump_weights_epoch()                      # a frozen weight ignores the optimiser epoch ...
    assert ask(wf)[1] == 1 and ask(wf)[0] is fbuf
    WL.invalidate_frozen_layouts()               # ... but not a write behind torch's back
    assert (ask(wf)[1], ask(wf)[1]) == (0, 1) and ask(wf)[0] is fbuf

    a, b = WL.weight_layout(w, None, "f", 1152), WL.weight_layout(w, None, "f", 1152)
    assert a[1] == 0 and b[1] == 0 and a[0] is not b[0] and a[0] is not buf

    assert not WL.has_plan() and WL.weight_plan_needs_rebuild()

    n_mine = len([k for k in WL._entries if k[0] == w._fd_cache_id])
    assert n_mine == 3
    n_retired = len(WL._retired)
    del w
    gc.collect()
    assert WL.evict_dead_weight_layouts() == n_mine
    assert len(WL._retired) == n_retired + n_mine
    assert WL.release_retired_layouts() == n_retired + n_mine
    del wf
    gc.collect()
    assert WL.evict_dead_weight_layouts() == 1
    WL.release_retired_layouts()
