"""``FlatAdam``: torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-8) + StepLR(gamma 0.1) over a ``dp.FlatParameters`` buffer
(trainer.py:129-131 of the reference).  It owns the moments, the step count and the learning rate - on the host and in the
device-side ``[step, lr]`` pair the kernel reads - and the ``adam.pth`` layout; it knows nothing of training."""
import math

import torch

from . import functional as FD
from . import tuning


def check_guard(mode, max_norm):
    """(mode, max_norm) validated: ``mode`` "off" or "skip", ``max_norm`` a finite float >= 0 that needs "skip" when positive."""
    if mode not in FlatAdam.GUARD_MODES:
        raise ValueError("grad_guard must be one of %s, got %r" % (" | ".join(FlatAdam.GUARD_MODES), mode))
    max_norm = float(max_norm)
    if not math.isfinite(max_norm) or max_norm < 0:
        raise ValueError("clip_grad_norm must be a finite number >= 0, got %r" % (max_norm,))
    if max_norm > 0 and mode == "off":
        raise ValueError("clip_grad_norm %g needs grad_guard 'skip': a gradient that is not finite has no norm to clip to" % max_norm)
    return mode, max_norm


def _segment_table(flat, segments):
    """``segments`` (parameter counts or (name, count) pairs, None: one) -> (names, element offsets: 0 first, numel last)."""
    if not segments:
        return ["all"], [0, flat.numel()]
    names, offsets, at = [], [0], 0
    for i, seg in enumerate(segments):
        name, count = seg if isinstance(seg, (tuple, list)) else ("segment%d" % i, seg)
        at += int(count)
        names.append(str(name))
        offsets.append(flat.offsets[at])
    if at != len(flat.params):
        raise ValueError("segments cover %d parameters, the flat buffer holds %d" % (at, len(flat.params)))
    if len(names) > FD.GUARD_MAX_SEGMENTS:
        raise ValueError("%d segments, the guard covers %d" % (len(names), FD.GUARD_MAX_SEGMENTS))
    return names, offsets


class FlatAdam:
    GUARD_MODES = ("off", "skip")

    def __init__(self, flat, lr, scheduler_step_size, segments=None):
        """``segments``: the cut of the parameter list into networks, as ``dp.GradientSynchronizer`` gets it - parameter counts,
        or ``(name, count)`` pairs; the guard reports one gradient norm per segment.  None: one segment."""
        self.flat = flat
        self.segment_names, self._segment_offsets = _segment_table(flat, segments)
        self.guard_mode, self.max_norm = "off", 0.0
        self.guard_stats = self.guard_counters = self._guard_ws = self._guard_seg = None
        self.exp_avg = torch.zeros_like(flat.flat_param)
        self.exp_avg_sq = torch.zeros_like(flat.flat_param)
        self.step_count = 0
        self.lr = self.initial_lr = lr
        self.state = torch.tensor([0.0, lr], device=flat.flat_param.device)      # [step, lr] on the device (graph-safe)
        self.scheduler_epochs = 0
        self.scheduler_step_size = scheduler_step_size

    def step(self, grad_scale=1.0):
        """One fused launch.  Step counter and lr are read from device memory, so the launch can live inside a captured hipGraph -
        whose replays advance the device counter but not ``step_count``.  Returns True if the launch also left
        ``flat_grad`` all zeros (``tuning.host.adam_zero``, the default); otherwise the gradient is the caller's to zero."""
        self.step_count += 1
        zero = bool(tuning.host.adam_zero)
        if self.guard_mode != "off":
            # with the guard on ``step_count`` counts the calls; the steps taken are ``state[0]`` (``applied_steps``)
            FD.grad_stats(self.flat.flat_grad, self._guard_seg, self._guard_ws, self.guard_stats, self.guard_counters, self.state,
                          grad_scale=grad_scale, max_norm=self.max_norm, skip_nonfinite=True)
            FD.adam_step_guarded(self.flat.flat_param, self.flat.flat_grad, self.exp_avg, self.exp_avg_sq, self.state, self.guard_stats,
                                 grad_scale=grad_scale, zero_grad=zero)
            return zero
        FD.adam_step_dev(self.flat.flat_param, self.flat.flat_grad, self.exp_avg, self.exp_avg_sq, self.state, grad_scale=grad_scale,
                         zero_grad=zero)
        return zero

    # ---- the guard: skip a step whose gradient is not finite, clip by the global norm ----
    def configure_guard(self, mode="off", max_norm=0.0):
        """``mode`` "skip": every ``step`` is ``fd_grad_stats`` + ``fd_adam_step_guarded`` - a gradient with a NaN or an inf changes
        neither parameters, moments nor the step count and is cleared; ``max_norm`` > 0 also scales the gradient by
        ``min(1, max_norm / (norm + 1e-6))`` (``torch.nn.utils.clip_grad_norm_``) and needs "skip".  The device tables are allocated
        here, once; a second call keeps the counters.  "off": ``step`` issues the unguarded call, as without this method."""
        mode, max_norm = check_guard(mode, max_norm)
        self.guard_mode, self.max_norm = mode, max_norm
        if mode != "off" and self.guard_stats is None:
            dev, n_seg = self.flat.flat_param.device, len(self.segment_names)
            self._guard_seg = torch.tensor(self._segment_offsets, dtype=torch.int64, device=dev)
            self._guard_ws = torch.empty(FD.grad_stats_ws_bytes(self.flat.numel(), n_seg) // 8, dtype=torch.float64, device=dev)
            self.guard_stats = torch.zeros(4 + n_seg, dtype=torch.float64, device=dev)
            self.guard_stats[2] = 1.0
            self.guard_counters = torch.tensor([0, -1, -1], dtype=torch.int64, device=dev)

    def guard_report(self):
        """What the latest ``step`` measured and decided, and the skip counters -> dict of ``grad_norm``, ``grad_norm/<network>``,
        ``clip_coef``, ``nonfinite``, ``skipped_steps``, ``first_skipped_step``, ``last_skipped_step`` ({} with the guard off).  Reads
        the two small device arrays: it synchronises, and ``step`` never calls it."""
        if self.guard_stats is None or self.guard_mode == "off":
            return {}
        stats, counters = self.guard_stats.tolist(), self.guard_counters.tolist()
        rep = {"grad_norm": stats[0]}
        for name, v in zip(self.segment_names, stats[4:]):
            rep["grad_norm/%s" % name] = v
        rep.update(clip_coef=stats[2], nonfinite=int(stats[1]), skipped_steps=int(counters[0]), first_skipped_step=int(counters[1]),
                   last_skipped_step=int(counters[2]))
        return rep

    def guard_counters_host(self):
        """[skipped steps, first skipped optimiser step, last] as ints ([0, -1, -1] with the guard never configured)."""
        return [0, -1, -1] if self.guard_counters is None else [int(c) for c in self.guard_counters.tolist()]

    def load_guard_counters(self, counters):
        if self.guard_counters is not None:
            self.guard_counters.copy_(torch.tensor([int(c) for c in counters], dtype=torch.int64))

    def applied_steps(self):
        """The Adam steps taken: ``state[0]`` with the guard on (a skipped step is not one; synchronises), ``step_count`` otherwise."""
        return int(float(self.state[0])) if self.guard_mode != "off" else self.step_count

    def scheduler_step(self):
        """StepLR(step_size, 0.1).step()  (trainer.py:266): the learning rate drops by 10x every ``scheduler_step_size`` calls."""
        self.scheduler_epochs += 1
        if self.scheduler_step_size > 0 and self.scheduler_epochs % self.scheduler_step_size == 0:
            self.lr *= 0.1
            self.state[1] = self.lr

    def state_dict(self):
        """``torch.optim.Adam.state_dict()`` layout (what trainer.py:714-715 writes), so that ``adam.pth`` interchanges with the
        reference: per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq`` in ``parameters_to_train`` order (the reference builds
        that list in the same network order, trainer.py:66-129), one parameter group carrying the current learning rate."""
        state = {}
        steps = self.applied_steps()           # with the guard on a skipped step is not an Adam step (torch's GradScaler.step)
        step = torch.tensor(float(steps))
        if steps > 0:
            avg, sq = self.exp_avg.detach().cpu(), self.exp_avg_sq.detach().cpu()
            for i, p in enumerate(self.flat.params):
                o, n = self.flat.offsets[i], p.numel()
                state[i] = {"step": step.clone(), "exp_avg": avg[o:o + n].view(p.shape).clone(),
                            "exp_avg_sq": sq[o:o + n].view(p.shape).clone()}
        group = {"lr": self.lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "maximize": False,
                 "foreach": None, "capturable": False, "differentiable": False, "fused": None, "initial_lr": self.initial_lr,
                 "params": list(range(len(self.flat.params)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, st):
        """Inverse of ``state_dict``; also reads the flat layout round 1 of this package wrote.  Restores the moments, the step
        count (bias correction) and the learning rate (StepLR decays already taken) on the host AND in the device-side ``state``
        the Adam kernel reads."""
        if "state" in st and "param_groups" in st:
            n_params = len(self.flat.params)
            groups = st["param_groups"]
            listed = sum(len(g["params"]) for g in groups)
            if listed != n_params:
                raise RuntimeError("adam.pth holds %d parameters, this trainer has %d (different network set?)" % (listed, n_params))
            steps = []
            self.exp_avg.zero_(); self.exp_avg_sq.zero_()
            for i, entry in st["state"].items():
                i = int(i)
                p, o = self.flat.params[i], self.flat.offsets[i]
                if tuple(entry["exp_avg"].shape) != tuple(p.shape):
                    raise RuntimeError("adam.pth: moment %d has shape %s, parameter has %s" % (i, tuple(entry["exp_avg"].shape), tuple(p.shape)))
                self.exp_avg[o:o + p.numel()].copy_(entry["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + p.numel()].copy_(entry["exp_avg_sq"].reshape(-1))
                steps.append(int(float(entry["step"])))
            if steps and min(steps) != max(steps):
                raise RuntimeError("adam.pth: per-parameter step counts differ (%d..%d); the flat Adam kernel keeps one" % (min(steps), max(steps)))
            self.step_count = steps[0] if steps else 0
            self.lr = float(groups[0]["lr"])
        elif "exp_avg" in st:
            if st["exp_avg"].numel() != self.exp_avg.numel():
                raise RuntimeError("adam.pth: %d moments for %d parameters" % (st["exp_avg"].numel(), self.exp_avg.numel()))
            self.exp_avg.copy_(st["exp_avg"]); self.exp_avg_sq.copy_(st["exp_avg_sq"])
            self.step_count = int(st["step"])
            self.lr = float(st.get("lr", self.lr))
        else:
            raise RuntimeError("adam.pth: unknown layout (keys %s)" % sorted(st))
        self.state[0] = float(self.step_count)
        self.state[1] = self.lr
