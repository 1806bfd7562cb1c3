"""fusiondepth_amd.checkpoint.load_state_by_key on the CPU: filtered by key, strict or tolerant by argument, copied in place."""
import pytest
import torch

from fusiondepth_amd import dp
from fusiondepth_amd.checkpoint import load_state_by_key


def _net(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4), torch.nn.Linear(4, 2))


def test_extra_keys_are_skipped_and_tensors_are_copied_in_place(tmp_path):
    src, net = _net(1), _net(2)
    sd = dict(src.state_dict(), height=192, width=640, use_stereo=False)          # what save_model adds to encoder.pth
    torch.save(sd, tmp_path / "encoder.pth")
    flat = dp.FlatParameters(list(net.parameters()))                              # parameters become views of one buffer
    ptrs = {k: v.data_ptr() for k, v in net.state_dict().items()}
    load_state_by_key(net, str(tmp_path / "encoder.pth"))
    for k, v in net.state_dict().items():
        assert torch.equal(v, src.state_dict()[k]) and v.data_ptr() == ptrs[k], k
    for p, o in zip(flat.params, flat.offsets):                                   # the views survived: the flat buffer holds the file
        assert p.data_ptr() == flat.flat_param.data_ptr() + 4 * o
        assert torch.equal(flat.flat_param[o:o + p.numel()].view(p.shape), p.detach())


def test_missing_keys_raise_unless_allowed(tmp_path):
    src, net = _net(3), _net(4)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    sd = {k: v for k, v in src.state_dict().items() if not k.startswith("2.")}
    path = str(tmp_path / "depth.pth")
    torch.save(sd, path)
    with pytest.raises(RuntimeError) as e:
        load_state_by_key(net, path)
    assert str(e.value) == "%s: missing keys %s" % (path, ["2.weight", "2.bias"])
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), "a refused file must leave the network as it was (%s)" % k
    load_state_by_key(net, path, allow_missing=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k] if k.startswith("2.") else src.state_dict()[k]), k
