"""A network's ``<name>.pth`` read as the reference's drivers do (trainer.py:717-746, refiner.py:84-152): by key, in place."""
import torch


def load_state_by_key(net, path, allow_missing=False):
    """Copy the tensors of the state dict at ``path`` into ``net`` IN PLACE, by key: parameters stay views of a flat buffer.  Keys
    that ``net`` does not have are skipped (``encoder.pth`` also carries height / width / use_stereo); keys that the file lacks raise
    unless ``allow_missing``.  The caller calls ``weight_layouts.weights_replaced()`` once after its last file."""
    own = net.state_dict()
    loaded = torch.load(path, map_location="cpu")
    missing = [k for k in own if k not in loaded]
    if missing and not allow_missing:
        raise RuntimeError("%s: missing keys %s" % (path, missing[:4]))
    with torch.no_grad():
        for k, v in loaded.items():
            if k in own:
                own[k].copy_(v)
