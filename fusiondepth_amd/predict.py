"""Inference with saved networks.  Stage 1: the frozen ``encoder`` / ``beam_encoder`` / ``depth`` networks of a ``Trainer.save_model``
folder, run the way the reference's ``inf_depth_map.py`` runs them (:53-84 model set, :159-172 ``process_batch``).

    p = Predictor(folder, num_layers=18)
    disp = p.predict(batch)[("disp", 0)]            # batch: "color_aug", 0, 0 and "2channel", as KITTIRAWBatches builds them

Stage 2 (``refine_2d=True``, a ``Refiner.save_model`` folder): the ``refine2d_decoder`` on top, the way the reference's
``evaluate_depth.py`` runs it (:132-139 model set, :183-233); the batch then also needs "4beam" and ("inv_K", s).

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
                 cat2end=False, device="cuda", refine_2d=False, catxy=True, refine2d_deep=True, refine_a0=True, refine_iter=1,
                 refine_offset=False, refine_depthnet_with_beam=True, height=192, width=640, min_depth=0.1, max_depth=100.0):
        """The arguments from ``refine_2d`` on are read with ``refine_2d`` only: the refine decoder's variant (``catxy``,
        ``refine2d_deep``), how its input maps are built (``refine_a0``, ``height`` / ``width`` of the network input, ``min_depth`` /
        ``max_depth``), how often it runs (``refine_iter``), its output activation (``refine_offset``: tanh) and whether the coarse
        decoder sees the LiDAR features (``refine_depthnet_with_beam``)."""
        if not torch.cuda.is_available():
            raise RuntimeError("fusiondepth_amd.Predictor needs an MI355X: there is no CPU path (use oracle/ for CPU checks)")
        self.device = torch.device(device)
        if self.device.index is not None:
            torch.cuda.set_device(self.device)
        m = {}
        m["encoder"] = networks.ResnetEncoder(num_layers, False, cat4beam_to_color=cat_4beam_to_color, cat2channel=cat2start)
        m["beam_encoder"] = networks.ResnetEncoder(num_layers, False, beam_encoder=True)
        m["depth"] = networks.DepthDecoder(m["encoder"].num_ch_enc, list(scales), cat2end=cat2end)
        self.scales, self.refine_2d = list(scales), bool(refine_2d)
        if self.refine_2d:
            if cat2end:
                raise NotImplementedError("Predictor: cat2end with refine_2d is not covered (the reference's refine branch reads beam_features, "
                                          "which its cat2end branch never computes)")
            m["refine2d_decoder"] = networks.DepthDecoder(m["encoder"].num_ch_enc, list(scales), road=True, catxy=bool(catxy),
                                                          deep=bool(refine2d_deep))
            self.refine = dict(catxy=bool(catxy), pool_disp0=bool(refine_a0), iters=int(refine_iter), tanh=bool(refine_offset),
                               with_beam=bool(refine_depthnet_with_beam), height=int(height), width=int(width),
                               min_depth=float(min_depth), max_depth=float(max_depth))
        self.models = {k: m[k].to(self.device).eval() for k in PREDICTOR_MODELS + (("refine2d_decoder",) if self.refine_2d else ())}
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
        """inf_depth_map.py:159-172 -> {("disp", s)} for the decoder's scales.  With ``refine_2d``, evaluate_depth.py:183-233: the coarse
        decoder (with the LiDAR features only if ``refine_depthnet_with_beam``), then ``refine_iter`` times the refine decoder's input
        maps from the current disparities (``FD.refine_inputs``: "4beam", "2channel", ("inv_K", s)) and the refine decoder, whose
        outputs replace ("disp", s).  The three stage-1 networks replay recorded call sequences (``FrozenRunner``); the refine decoder
        runs eagerly under ``no_grad``: a recording is keyed by a flat list of tensors, which its ``depth_maps`` dict is not."""
        color, two = batch["color_aug", 0, 0], batch["2channel"]
        if color.device != self.device:
            color, two = color.to(self.device), two.to(self.device)
        with torch.no_grad():
            features = self.frozen.run("encoder", color.contiguous())
            beam_features = self.frozen.run("beam_encoder", two.contiguous())
            if not self.refine_2d:
                return dict(self.frozen.run("depth", *features, *beam_features))
            r = self.refine
            out = dict(self.frozen.run("depth", *features, *beam_features) if r["with_beam"] else self.frozen.run("depth", *features))
            beam = batch["4beam"].to(self.device)
            inv_Ks = [batch[("inv_K", s)].to(self.device) for s in self.scales]
            for _ in range(r["iters"]):
                maps = FD.refine_inputs([out[("disp", s)] for s in self.scales], beam, two, inv_Ks, r["height"], r["width"], r["min_depth"],
                                        r["max_depth"], catxy=r["catxy"], pool_disp0=r["pool_disp0"])
                refined = self.models["refine2d_decoder"](features, beam_features=beam_features,
                                                          depth_maps={("disp", s): m for s, m in zip(self.scales, maps)}, tanh=r["tanh"])
                for s in self.scales:
                    out[("disp", s)] = refined[("disp", s)]
            return out
