"""``FlatAdam``: torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-8) + StepLR(gamma 0.1) over a ``dp.FlatParameters`` buffer
(trainer.py:129-131 of the reference).  It owns the moments, the step count and the learning rate - on the host and in the
device-side ``[step, lr]`` pair the kernel reads - and the ``adam.pth`` layout; it knows nothing of training."""
import torch

from . import functional as FD
from . import tuning


class FlatAdam:
    def __init__(self, flat, lr, scheduler_step_size):
        self.flat = flat
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
        FD.adam_step_dev(self.flat.flat_param, self.flat.flat_grad, self.exp_avg, self.exp_avg_sq, self.state, grad_scale=grad_scale,
                         zero_grad=zero)
        return zero

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
        step = torch.tensor(float(self.step_count))
        if self.step_count > 0:
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
