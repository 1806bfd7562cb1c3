"""Stage-1 inference: the frozen ``encoder`` / ``beam_encoder`` / ``depth`` networks of a ``Trainer.save_model`` folder, run the way
the reference's ``inf_depth_map.py`` runs them (:53-84 model set, :159-172 ``process_batch``).

    p = Predictor(folder, num_layers=18)
    disp = p.predict(batch)[("disp", 0)]            # batch: "color_aug", 0, 0 and "2channel", as KITTIRAWBatches builds them

The forward passes go through ``FrozenRunner``, which the Refiner's frozen block uses too: eval-mode networks under
``torch.no_grad``, kernel-side weight layouts derived once (the frozen weight cache), recorded call sequences.
"""
import os

import torch

from . import functional as FD
from . import networks
from . import weight_layouts
from .checkpoint import load_state_by_key

PREDICTOR_MODELS = ("encoder", "beam_encoder", "depth")


class FrozenRunner:
    """Runs the networks of ``models`` that nothing trains.  Under no_grad and in eval mode a network's libfdhip calls are recorded
    once per input signature and replayed by ONE ``fd_replay`` call afterwards (replay.py; ~45 launches per ResNet-18 encoder, ~40
    per depth decoder), through ``replays[name]``.  With gradients enabled, in training mode, or for a network in ``trained``: eagerly."""

    def __init__(self, models, owner, trained=()):
        self.models, self.owner, self.trained = models, owner, trained
        self.replays = {}

    def run(self, name, *tensors):
        net = self.models[name]      # ``depth`` takes the encoder features (+ the LiDAR encoder's) as a flat argument list
        if name == "depth":
            n = len(net.num_ch_enc)
            call = lambda *f: net(list(f[:n]), beam_features=list(f[n:])) if len(f) > n else net(list(f))
        else:
            call = lambda x: list(net(x))
        if name in self.trained or torch.is_grad_enabled() or net.training:
            return call(*tensors)
        rp = self.replays.get(name)
        if rp is None:
            from .replay import Replayable
            rp = self.replays[name] = Replayable(call, lambda: list(net.parameters()) + list(net.buffers()), name="%s.%s" % (self.owner, name))
        return rp(*tensors)


class Predictor:
    """``load_weights_folder``: ``encoder.pth`` / ``beam_encoder.pth`` / ``depth.pth`` (the encoder file also carries height / width /
    use_stereo; filtered by key like the reference does).  The remaining arguments are the options the three constructors read."""

    def __init__(self, load_weights_folder, num_layers=50, scales=(0, 1, 2, 3), cat_4beam_to_color=False, cat2start=False,
                 cat2end=False, device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("fusiondepth_amd.Predictor needs an MI355X: there is no CPU path (use oracle/ for CPU checks)")
        self.device = torch.device(device)
        if self.device.index is not None:
            torch.cuda.set_device(self.device)
        m = {}
        m["encoder"] = networks.ResnetEncoder(num_layers, False, cat4beam_to_color=cat_4beam_to_color, cat2channel=cat2start)
        m["beam_encoder"] = networks.ResnetEncoder(num_layers, False, beam_encoder=True)
        m["depth"] = networks.DepthDecoder(m["encoder"].num_ch_enc, list(scales), cat2end=cat2end)
        self.models = {k: m[k].to(self.device).eval() for k in PREDICTOR_MODELS}
        self._load(load_weights_folder)
        params = [p for net in self.models.values() for p in net.parameters()]
        for p in params:
            p.requires_grad_(False)
        FD.enable_weight_cache(params, frozen=True)
        self.frozen = FrozenRunner(self.models, "Predictor")

    def _load(self, folder):
        """Every key of every network must be in its file; extra keys of the encoder file are skipped."""
        folder = os.path.expanduser(folder)
        if not os.path.isdir(folder):
            raise FileNotFoundError("Cannot find a folder at {}".format(folder))
        for name, net in self.models.items():
            path = os.path.join(folder, "{}.pth".format(name))
            if not os.path.isfile(path):
                raise FileNotFoundError("load_weights_folder: %s is missing" % path)
            load_state_by_key(net, path)
        weight_layouts.weights_replaced()

    def predict(self, batch):
        """inf_depth_map.py:159-172 -> {("disp", s)} for the decoder's scales."""
        color, two = batch["color_aug", 0, 0], batch["2channel"]
        if color.device != self.device:
            color, two = color.to(self.device), two.to(self.device)
        with torch.no_grad():
            features = self.frozen.run("encoder", color.contiguous())
            beam_features = self.frozen.run("beam_encoder", two.contiguous())
            return dict(self.frozen.run("depth", *features, *beam_features))
