"""Stage-1 inference: the frozen ``encoder`` / ``beam_encoder`` / ``depth`` networks of a ``Trainer.save_model`` folder, run the way
the reference's ``inf_depth_map.py`` runs them (:53-84 model set, :159-172 ``process_batch``).

    p = Predictor(folder, num_layers=18)
    disp = p.predict(batch)[("disp", 0)]            # batch: "color_aug", 0, 0 and "2channel", as KITTIRAWBatches builds them

The forward passes go through the same machinery as the Refiner's frozen block (``Refiner._run_module``): eval-mode networks
under ``torch.no_grad``, kernel-side weight layouts derived once (the frozen weight cache), each network's libfdhip calls recorded
once per input signature and replayed by one ``fd_replay`` call afterwards.
"""
import os

import torch

from . import functional as FD
from . import networks
from . import weight_layouts

PREDICTOR_MODELS = ("encoder", "beam_encoder", "depth")


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
        self._replays = {}

    def _load(self, folder):
        """The three networks' tensors copied in place by key, as ``Refiner._load_pretrained`` does - but stricter: a key missing
        from a file raises for the encoder too (the Refiner tolerates that one); extra keys of the encoder file are skipped."""
        folder = os.path.expanduser(folder)
        if not os.path.isdir(folder):
            raise FileNotFoundError("Cannot find a folder at {}".format(folder))
        for name, net in self.models.items():
            path = os.path.join(folder, "{}.pth".format(name))
            if not os.path.isfile(path):
                raise FileNotFoundError("load_weights_folder: %s is missing" % path)
            own = net.state_dict()
            loaded = torch.load(path, map_location="cpu")
            missing = [k for k in own if k not in loaded]
            if missing:
                raise RuntimeError("%s: missing keys %s" % (path, missing[:4]))
            with torch.no_grad():
                for k, v in loaded.items():
                    if k in own:
                        own[k].copy_(v)
        weight_layouts.weights_replaced()

    def _run_module(self, name, *tensors):
        """``Refiner._run_module``: recorded once per input signature, replayed afterwards.  ``depth`` takes the encoder features
        followed by the LiDAR encoder's as a flat argument list."""
        net = self.models[name]
        if name == "depth":
            n = len(net.num_ch_enc)
            call = lambda *f: net(list(f[:n]), beam_features=list(f[n:]))
        else:
            call = lambda x: list(net(x))
        rp = self._replays.get(name)
        if rp is None:
            from .replay import Replayable
            rp = self._replays[name] = Replayable(call, lambda: list(net.parameters()) + list(net.buffers()), name="Predictor." + name)
        return rp(*tensors)

    def predict(self, batch):
        """inf_depth_map.py:159-172 -> {("disp", s)} for the decoder's scales."""
        color, two = batch["color_aug", 0, 0], batch["2channel"]
        if color.device != self.device:
            color, two = color.to(self.device), two.to(self.device)
        with torch.no_grad():
            features = self._run_module("encoder", color.contiguous())
            beam_features = self._run_module("beam_encoder", two.contiguous())
            return dict(self._run_module("depth", *features, *beam_features))
