"""fusiondepth_amd.optim.FlatAdam on the CPU: the ``adam.pth`` layout against the installed torch's own Adam, the round-1 flat
layout, the error cases and the StepLR schedule.  ``step()`` launches a kernel and is not called here."""
import pytest
import torch

from fusiondepth_amd import dp
from fusiondepth_amd.optim import FlatAdam

SHAPES = [(4, 3, 3, 3), (4,), (2, 5)]
LR = 1.5e-4


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]


def _adam(step_size=6):
    return FlatAdam(dp.FlatParameters(_params()), LR, step_size)


def _stepped(n=3):
    """A FlatAdam as ``n`` kernel launches would leave it (host side: moments filled, counts advanced)."""
    ad = _adam()
    g = torch.Generator().manual_seed(7)
    ad.exp_avg.copy_(torch.randn(ad.exp_avg.shape, generator=g))
    ad.exp_avg_sq.copy_(torch.rand(ad.exp_avg_sq.shape, generator=g))
    ad.step_count = n
    ad.state[0] = float(n)
    return ad


def _types(x):
    """The structure of a state dict: keys and value types, tensors with their shapes."""
    if isinstance(x, dict):
        return {k: _types(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return (type(x), [_types(v) for v in x])
    if torch.is_tensor(x):
        return (torch.Tensor, tuple(x.shape))
    return type(x)


def test_state_dict_has_torch_adams_keys_and_types():
    ref_params = _params()
    ref = torch.optim.Adam(ref_params, LR)
    torch.optim.lr_scheduler.StepLR(ref, 6, 0.1)              # the reference's Adam sits under one (trainer.py:129-131): "initial_lr"
    for p in ref_params:
        p.grad = torch.ones_like(p)
    ref.step()
    want, got = ref.state_dict(), _stepped(1).state_dict()
    # keys of torch's parameter group that ``state_dict()`` - moved verbatim, written against an older torch - does not write; each
    # with the reason why ``adam.pth`` still interchanges.  Everything else must be there with torch's own value types.
    not_written = {"decoupled_weight_decay": "Adam's own default (False = plain Adam); torch's load_state_dict keeps the loading "
                                             "optimiser's value for a key the file lacks (checked below)"}
    group = want["param_groups"][0]
    assert set(group) - set(got["param_groups"][0]) <= set(not_written)
    for k in not_written:
        group.pop(k, None)
    assert _types(got) == _types(want)
    assert got["param_groups"][0]["betas"] == group["betas"] and got["param_groups"][0]["eps"] == group["eps"]
    loader = torch.optim.Adam(_params(), LR)
    defaults = {k: loader.param_groups[0][k] for k in not_written if k in loader.param_groups[0]}
    loader.load_state_dict(got)                                 # torch reads what FlatAdam writes ...
    assert {k: loader.param_groups[0][k] for k in defaults} == defaults      # ... and keeps its defaults for the keys left out
    assert torch.equal(loader.state_dict()["state"][2]["exp_avg"], got["state"][2]["exp_avg"])
    assert got["param_groups"][0]["params"] == want["param_groups"][0]["params"]
    assert float(got["state"][0]["step"]) == float(want["state"][0]["step"]) == 1.0
    assert _adam().state_dict()["state"] == {} == torch.optim.Adam(_params(), LR).state_dict()["state"]      # before any step


def test_load_state_dict_restores_everything():
    src = _stepped(3)
    src.lr = LR * 0.1
    st = src.state_dict()
    dst = _adam()
    dst.load_state_dict(st)
    assert torch.equal(dst.exp_avg, src.exp_avg) and torch.equal(dst.exp_avg_sq, src.exp_avg_sq)
    assert dst.step_count == 3 and dst.lr == LR * 0.1
    assert dst.state.tolist() == [3.0, float(torch.tensor(LR * 0.1))]
    for i, p in enumerate(dst.flat.params):            # per-parameter moments sit at the parameter's flat offset
        o = dst.flat.offsets[i]
        assert torch.equal(dst.exp_avg[o:o + p.numel()].view(p.shape), st["state"][i]["exp_avg"])


def test_round1_flat_layout_loads():
    src, dst = _stepped(5), _adam()
    dst.load_state_dict({"exp_avg": src.exp_avg.clone(), "exp_avg_sq": src.exp_avg_sq.clone(), "step": 5, "lr": 2e-5})
    assert torch.equal(dst.exp_avg, src.exp_avg) and torch.equal(dst.exp_avg_sq, src.exp_avg_sq)
    assert dst.step_count == 5 and dst.lr == 2e-5 and float(dst.state[0]) == 5.0
    dst.load_state_dict({"exp_avg": src.exp_avg, "exp_avg_sq": src.exp_avg_sq, "step": 6})      # no lr: the current one stays
    assert dst.step_count == 6 and dst.lr == 2e-5


def test_load_state_dict_errors():
    st = _stepped(2).state_dict()
    few = {"state": st["state"], "param_groups": [dict(st["param_groups"][0], params=[0, 1])]}
    with pytest.raises(RuntimeError, match=r"adam.pth holds 2 parameters, this trainer has 3 \(different network set\?\)"):
        _adam().load_state_dict(few)
    bad = _stepped(2).state_dict()
    bad["state"][2]["exp_avg"] = torch.zeros(5, 2)
    with pytest.raises(RuntimeError, match=r"adam.pth: moment 2 has shape \(5, 2\), parameter has \(2, 5\)"):
        _adam().load_state_dict(bad)
    uneven = _stepped(2).state_dict()
    uneven["state"][1]["step"] = torch.tensor(4.0)
    with pytest.raises(RuntimeError, match=r"adam.pth: per-parameter step counts differ \(2..4\); the flat Adam kernel keeps one"):
        _adam().load_state_dict(uneven)
    with pytest.raises(RuntimeError, match=r"adam.pth: unknown layout \(keys \['moments'\]\)"):
        _adam().load_state_dict({"moments": 1})
    with pytest.raises(RuntimeError, match=r"adam.pth: 3 moments for %d parameters" % _adam().exp_avg.numel()):
        _adam().load_state_dict({"exp_avg": torch.zeros(3), "exp_avg_sq": torch.zeros(3), "step": 1})


def test_scheduler_step_drops_lr_every_step_size_calls():
    ad = _adam(step_size=3)
    lrs = []
    for _ in range(7):
        ad.scheduler_step()
        lrs.append(ad.lr)
        assert float(ad.state[1]) == float(torch.tensor(ad.lr))
    a, b = LR * 0.1, LR * 0.1 * 0.1
    assert lrs == [LR, LR, a, a, a, b, b]
    assert ad.initial_lr == LR and ad.state_dict()["param_groups"][0]["initial_lr"] == LR
    never = _adam(step_size=0)
    for _ in range(5):
        never.scheduler_step()
    assert never.lr == LR and float(never.state[1]) == float(torch.tensor(LR))
