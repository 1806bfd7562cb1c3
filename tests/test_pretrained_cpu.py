"""``ResnetEncoder(num_layers, pretrained)`` from a torchvision file on disk (reference networks/resnet_encoder.py:33-50, 71-87), on
the CPU: which values land where, where the file is looked for, and what is refused.  The file is tests/imagenet_file.py's stand-in:
seeded random values in torchvision's layout."""
import os

import pytest
import torch

import imagenet_file as IF


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def hub(tmp_path_factory):
    """One directory with both stand-in files -> (directory, {num_layers: (path, state dict)})."""
    folder = str(tmp_path_factory.mktemp("hub"))
    return folder, {n: IF.write(folder, n) for n in (18, 50)}


@pytest.mark.parametrize("n", [18, 50])
def test_every_tensor_is_the_files(hub, n):
    from fusiondepth_amd.networks import ResnetEncoder
    folder, files = hub
    path, sd = files[n]
    for where in (path, folder):                                 # a file, or the directory that holds it
        enc = ResnetEncoder(n, where)
        assert enc.pretrained_file == path
        own = enc.encoder.state_dict()
        assert list(own) == list(sd)                             # the trunk declares torchvision's keys, fc and the counters included
        for k, v in sd.items():
            assert _same(own[k], v), k
    assert ResnetEncoder(n, False).pretrained_file is None


@pytest.mark.parametrize("n", [18, 50])
def test_two_input_images_share_the_stem(hub, n):
    from fusiondepth_amd.networks import ResnetEncoder
    folder, files = hub
    sd = files[n][1]
    enc = ResnetEncoder(n, folder, num_input_images=2)
    own = enc.encoder.state_dict()
    want = torch.cat([sd["conv1.weight"]] * 2, 1) / 2            # resnet_encoder.py:47-48
    assert _same(own["conv1.weight"], want) and own["conv1.weight"].shape == (64, 6, 7, 7)
    for k, v in sd.items():
        if k != "conv1.weight":
            assert _same(own[k], v), k


@pytest.mark.parametrize("n", [18, 50])
def test_replaced_stems_keep_the_scratch_initialisation(hub, n):
    """resnet_encoder.py:76-87 replaces conv1 AFTER the file was loaded: a fresh ``nn.Conv2d``, never the file's values."""
    from fusiondepth_amd.networks import ResnetEncoder
    folder, files = hub
    sd = files[n][1]
    stems = [(dict(cat4beam_to_color=True), 4), (dict(cat2channel=True), 5), (dict(beam_encoder=True), 2),
             (dict(beam_encoder=True, num_input_images=2), 4), (dict(refine_encoder=True), 6)]
    for kw, channels in stems:
        torch.manual_seed(31)
        enc = ResnetEncoder(n, folder, **kw)
        torch.manual_seed(31)
        scratch = ResnetEncoder(n, False, **kw)
        own = enc.encoder.state_dict()
        w = own["conv1.weight"]
        assert w.shape == (64, channels, 7, 7), kw
        assert _same(w, scratch.encoder.conv1.weight.detach()), kw          # what the scratch path gives the stem
        k = min(channels, 3)
        assert not torch.equal(w[:, :k], sd["conv1.weight"][:, :k]) and float(w.std()) > 0      # ... and not the file's
        for key, v in sd.items():
            if key != "conv1.weight":
                assert _same(own[key], v), (kw, key)


def test_search_order(hub, tmp_path, monkeypatch):
    from fusiondepth_amd.networks import ResnetEncoder
    from fusiondepth_amd.networks import resnet_encoder as RE
    home, torch_home, given = tmp_path / "home", tmp_path / "torch_home", tmp_path / "given"
    monkeypatch.setenv("HOME", str(home))
    monkeypatch.setenv("TORCH_HOME", str(torch_home))
    in_home, in_torch_home = str(home / ".cache" / "torch" / "hub" / "checkpoints"), str(torch_home / "hub" / "checkpoints")
    assert RE.imagenet_search_path() == [in_torch_home, in_home]
    with pytest.raises(RuntimeError) as e:                       # nothing anywhere: today's error, and where it looked
        ResnetEncoder(18, True)
    assert "cannot be downloaded" in str(e.value) and in_torch_home in str(e.value) and in_home in str(e.value)
    p_home, sd_home = IF.write(in_home, 18, seed=1)
    assert RE.find_imagenet_file(18, True) == p_home
    with pytest.raises(RuntimeError, match="cannot be downloaded"):
        RE.find_imagenet_file(50, True)                          # the ResNet-18 file does not serve ResNet-50
    p_torch, sd_torch = IF.write(in_torch_home, 18, name="resnet18.pth", seed=2)
    assert RE.find_imagenet_file(18, True) == p_torch            # $TORCH_HOME before ~/.cache
    enc = ResnetEncoder(18, True)
    assert enc.pretrained_file == p_torch and _same(enc.encoder.state_dict()["layer4.1.conv2.weight"], sd_torch["layer4.1.conv2.weight"])
    monkeypatch.delenv("TORCH_HOME")
    assert RE.imagenet_search_path() == [in_home] and RE.find_imagenet_file(18, True) == p_home
    # --pretrained_path comes first: Trainer._build_networks hands opt.pretrained_path to the constructor in place of True
    p_given, _ = IF.write(str(given), 18, seed=3)
    assert RE.find_imagenet_file(18, str(given)) == p_given and RE.find_imagenet_file(18, p_given) == p_given
    with pytest.raises(RuntimeError) as e:                       # a path that was given is not backed up by the caches
        RE.find_imagenet_file(50, str(given))
    assert str(given) in str(e.value) and in_home not in str(e.value)


def test_refusals(hub, tmp_path):
    from fusiondepth_amd.networks import ResnetEncoder
    folder, files = hub
    path18, sd18 = files[18]
    path50, _ = files[50]
    with pytest.raises(RuntimeError) as e:                       # a ResNet-50 file for --num_layers 18
        ResnetEncoder(18, path50)
    assert path50 in str(e.value) and "unexpected key layer1.0.conv3.weight" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        ResnetEncoder(50, path18)
    assert path18 in str(e.value) and "missing key layer1.0.conv3.weight" in str(e.value)
    two = tmp_path / "two"
    a, _ = IF.write(str(two), 18, name="resnet18-aaaaaaaa.pth")
    b, _ = IF.write(str(two), 18, name="resnet18.pth")
    with pytest.raises(RuntimeError) as e:                       # two candidates: both are listed
        ResnetEncoder(18, str(two))
    assert a in str(e.value) and b in str(e.value) and "more than one" in str(e.value)

    def broken(name, change):
        sd = dict(sd18)
        change(sd)
        p = str(tmp_path / name)
        torch.save(sd, p)
        return p

    p = broken("short.pth", lambda sd: sd.pop("layer3.1.bn2.running_var"))
    with pytest.raises(RuntimeError, match="missing key layer3.1.bn2.running_var") as e:
        ResnetEncoder(18, p)
    assert p in str(e.value)
    p = broken("long.pth", lambda sd: sd.update({"layer9.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="unexpected key layer9.weight") as e:
        ResnetEncoder(18, p, beam_encoder=True)                  # strict for the replaced stems too
    assert p in str(e.value)
    p = broken("shape.pth", lambda sd: sd.update({"layer2.0.conv1.weight": torch.zeros(128, 64, 1, 1)}))
    with pytest.raises(RuntimeError, match=r"layer2.0.conv1.weight has shape \(128, 64, 1, 1\)") as e:
        ResnetEncoder(18, p)
    assert p in str(e.value)
    p = broken("stem.pth", lambda sd: sd.update({"conv1.weight": torch.zeros(64, 6, 7, 7)}))
    with pytest.raises(RuntimeError, match="conv1.weight has shape") as e:
        ResnetEncoder(18, p, num_input_images=2)                 # the file's stem is torchvision's, whatever this encoder's is
    assert p in str(e.value)
    with pytest.raises(RuntimeError, match="cannot be downloaded"):
        ResnetEncoder(18, str(tmp_path / "nowhere"))
    with pytest.raises(ValueError, match="not a valid number of resnet layers"):
        ResnetEncoder(19, path18)
