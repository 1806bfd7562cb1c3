"""A stand-in for torchvision's ``resnet{18,50}-*.pth``: the keys and shapes of ``torchvision.models.resnet{n}().state_dict()``, written
out here from the architecture (torchvision is not installed), filled with seeded random values.  No real ImageNet file is on the test
machines; what the tests check is where the values land, not what they are."""
import os

import torch

_BLOCKS = {18: ("basic", [2, 2, 2, 2]), 50: ("bottleneck", [3, 4, 6, 3])}


def _bn(prefix, c):
    return [(prefix + ".weight", (c,)), (prefix + ".bias", (c,)), (prefix + ".running_mean", (c,)), (prefix + ".running_var", (c,)),
            (prefix + ".num_batches_tracked", ())]


def layout(num_layers):
    """[(key, shape)] in torchvision's order."""
    kind, counts = _BLOCKS[num_layers]
    exp = 1 if kind == "basic" else 4
    keys = [("conv1.weight", (64, 3, 7, 7))] + _bn("bn1", 64)
    inplanes = 64
    for li, (planes, n) in enumerate(zip((64, 128, 256, 512), counts)):
        for bi in range(n):
            p = "layer%d.%d" % (li + 1, bi)
            stride = (1 if li == 0 else 2) if bi == 0 else 1
            if kind == "basic":
                keys += [(p + ".conv1.weight", (planes, inplanes, 3, 3))] + _bn(p + ".bn1", planes)
                keys += [(p + ".conv2.weight", (planes, planes, 3, 3))] + _bn(p + ".bn2", planes)
            else:
                keys += [(p + ".conv1.weight", (planes, inplanes, 1, 1))] + _bn(p + ".bn1", planes)
                keys += [(p + ".conv2.weight", (planes, planes, 3, 3))] + _bn(p + ".bn2", planes)
                keys += [(p + ".conv3.weight", (planes * 4, planes, 1, 1))] + _bn(p + ".bn3", planes * 4)
            if stride != 1 or inplanes != planes * exp:
                keys += [(p + ".downsample.0.weight", (planes * exp, inplanes, 1, 1))] + _bn(p + ".downsample.1", planes * exp)
            inplanes = planes * exp
    return keys + [("fc.weight", (1000, inplanes)), ("fc.bias", (1000,))]


def state_dict(num_layers, seed=0):
    gen = torch.Generator().manual_seed(1000 * num_layers + seed)
    sd = {}
    for key, shape in layout(num_layers):
        if key.endswith("num_batches_tracked"):
            sd[key] = torch.tensor(int(torch.randint(1, 1000, (1,), generator=gen)))       # int64, as torchvision stores it
        elif key.endswith("running_var"):
            sd[key] = torch.rand(shape, generator=gen) + 0.5
        else:
            sd[key] = torch.randn(shape, generator=gen) * 0.05
    return sd


def write(folder, num_layers, name=None, seed=0):
    """``<folder>/resnet{n}-<8 hex digits>.pth`` as torch hub names its downloads -> (path, the state dict)."""
    os.makedirs(folder, exist_ok=True)
    sd = state_dict(num_layers, seed)
    path = os.path.join(folder, name or "resnet%d-%08x.pth" % (num_layers, 0xf37072fd + num_layers))
    torch.save(sd, path)
    return path, sd
