"""``Trainer.train_step`` replayed from a captured hipGraph (HIP graphs instead of a tracing compiler): the ~4500 kernel launches
of one optimiser step cost one graph launch on the host.  The first call runs eagerly (allocator warm-up), the second captures,
later calls copy the new batch into the captured input buffers and replay.  With several ranks the forward/backward micro-steps
are replayed and the gradient all-reduce + Adam run after the graph."""
import torch

from . import functional as FD
from . import weight_layouts


class GraphedStep:
    """The captured step of one trainer ``tr``, which every method takes (no reference is kept: a deleted trainer frees its memory)."""

    def __init__(self):
        self.graph = None          # None -> "warm" (one eager step has run) -> the captured torch.cuda.CUDAGraph
        self.active = False        # True only inside step(): the captured step keeps every fork on the capture stream
        self.static_in = self.static_losses = self.last_mbs = self.side = None

    def step(self, tr, micro_batches):
        self.active = True             # the captured step keeps the pose decoder on the capture stream (see Trainer.predict_poses)
        try:
            losses = self._step(tr, micro_batches)
        finally:
            self.active = False        # direct process_batch / train_step calls afterwards fork their side streams again
        tr.step += tr.accumulate_step
        tr.batch_idx += tr.accumulate_step
        return losses

    def _step(self, tr, micro_batches):
        if self.graph is None:
            if tr.stack_microbatches:
                self.static_in = tr.stack_micro_batches(micro_batches)
                if len(micro_batches) == 1:
                    self.static_in = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.static_in.items()}
            else:
                self.static_in = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in mb.items()} for mb in micro_batches]
            self.last_mbs = micro_batches
            self.graph = "warm"
            # warm up on the stream the capture will use, so that autograd's AccumulateGrad nodes are bound to it
            self.side = torch.cuda.Stream()
            self.side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.side):
                losses = self._body(tr)
                if tr.world_size > 1:
                    self._sync_and_step(tr)
            torch.cuda.current_stream().wait_stream(self.side)
            return losses
        if micro_batches is not self.last_mbs:
            self._copy_into_static(micro_batches, tr.stack_microbatches)
            self.last_mbs = micro_batches
        if self.graph == "warm":
            with torch.cuda.stream(self.side):
                tr._ensure_weight_plan()       # layouts valid now; inside the graph Adam is followed by the batched refresh
            if not weight_layouts.has_plan():
                FD.bump_weights_epoch()        # no plan: the captured step must re-derive every weight layout at first use
            FD.sync_late_layouts()             # no event from outside the capture may be waited on inside it
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self.side):
                self.static_losses = self._body(tr)
            self.graph = g
        # A refresh of the cached weight layouts issued eagerly since the last replay - the optimiser step that follows the graph when
        # world_size > 1, load_model() - puts the large layouts on a side stream behind an event (weight_layouts.refresh_weight_layouts).
        # The captured kernels were recorded with "layout ready" and never look at that event: the replay stream waits for it here.
        FD.sync_late_layouts()
        self.graph.replay()
        if tr.world_size > 1:
            self._sync_and_step(tr)
        return self.static_losses

    def _copy_into_static(self, micro_batches, stacked):
        if not stacked:
            for dst, src in zip(self.static_in, micro_batches):
                for k, v in src.items():
                    if torch.is_tensor(v):
                        dst[k].copy_(v)
            return
        for i, mb in enumerate(micro_batches):
            for k, v in mb.items():
                if torch.is_tensor(v):
                    n = v.shape[0]
                    self.static_in[k][i * n:(i + 1) * n].copy_(v)
                elif k == "_noise":
                    for s_, t in enumerate(v):
                        self.static_in[k][s_][i * t.shape[0]:(i + 1) * t.shape[0]].copy_(t)

    def _body(self, tr):
        _, _, losses = tr._forward_backward(self.static_in, eager=False)
        if tr.world_size == 1:
            if not tr.optim.step():
                tr.flat.flat_grad.zero_()
        return {k: v.detach() for k, v in losses.items()}

    def _sync_and_step(self, tr):
        import torch.distributed as dist
        dist.all_reduce(tr.flat.flat_grad, op=dist.ReduceOp.SUM)
        tr.optimizer_step(1.0 / tr.world_size)
