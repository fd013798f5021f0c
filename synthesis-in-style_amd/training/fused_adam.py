"""``GradientClipAdam`` (reference: training_builder/doc_ufcn_train_builder.py:18-33, imported there from the third-party
``pytorch_training.optimizer``) on two HIP launches per step (``sis_adam_clip_step``).

ASSUMED clip rule -- the package is not available to check: ``torch.nn.utils.clip_grad_norm_(all parameters of the optimizer,
max_norm)`` (total L2 norm over every gradient, factor ``min(1, max_norm / (norm + 1e-6))``), then ``torch.optim.Adam`` (L2 weight
decay added to the gradient, not AdamW).  The rule lives in ``clip_coefficient`` (host path) and ``adam_step_kernel``
(csrc/doc_ufcn.hip): change both there if the package says otherwise.  Unlike ``clip_grad_norm_``, the fused step leaves
``p.grad`` unclipped (the clip factor only enters the update).

Device path: a table of (param, grad, exp_avg, exp_avg_sq) chunks as ``FusedSGD`` keeps (training/fused_sgd.py); the first launch
writes one partial squared norm per chunk and advances a device-side step counter, the second sums the partials in a fixed order
in every workgroup (deterministic) and updates its chunk with the bias correction of that counter.  lr / betas / eps / weight decay
per group and max_norm are read from a device tensor that ``push_hyper()`` refreshes through a ring of pinned buffers, so a
captured hipGraph of the step follows the LR schedule on replay.  CPU parameters (the gloo rehearsals) take a plain torch path.

Differences from ``torch.optim.Adam`` on the device path: ONE step counter for the whole optimizer (torch counts per
parameter), so a parameter that has no gradient on some step gets the bias correction of the optimizer's count, not of its
own (DocUFCN gives every parameter a gradient on every step); the state holds ``exp_avg`` / ``exp_avg_sq`` per parameter but no
``state['step']``, so its ``state_dict`` cannot be loaded into ``torch.optim.Adam`` or the other way round.
"""
import math

import numpy as np
import torch
from torch.optim.optimizer import Optimizer

import sis_hip


def clip_coefficient(total_norm, max_norm):
    """The factor every gradient is multiplied by (torch.nn.utils.clip_grad_norm_)."""
    return min(1.0, max_norm / (total_norm + 1e-6))


class GradientClipAdam(Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=1.0):
        if lr < 0 or eps < 0 or weight_decay < 0 or max_norm <= 0 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError("GradientClipAdam: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) > 4:
            raise ValueError("GradientClipAdam supports at most 4 parameter groups")
        self.max_norm = float(max_norm)
        self._table_key = None
        self._grad_key = None
        self._hyper = None
        self._hyper_hosts = None
        self._capture_host = None
        self._step_dev = None

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none=set_to_none)

    # ---- host path ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _step_torch(self, entries):
        grads = [p.grad for _, p in entries]
        total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g, 2.0) for g in grads]), 2.0).item()
        coef = clip_coefficient(total, self.max_norm)
        for gi, p in entries:
            group = self.param_groups[gi]
            b1, b2 = group['betas']
            state = self.state[p]
            if not state:
                state['step'] = 0
                state['exp_avg'] = torch.zeros_like(p)
                state['exp_avg_sq'] = torch.zeros_like(p)
            state['step'] += 1
            t = state['step']
            g = p.grad * coef
            if group['weight_decay'] != 0:
                g = g.add(p, alpha=group['weight_decay'])
            state['exp_avg'].lerp_(g, 1 - b1)
            state['exp_avg_sq'].mul_(b2).addcmul_(g, g, value=1 - b2)
            step_size = group['lr'] / (1 - b1 ** t)
            denom = (state['exp_avg_sq'].sqrt() / math.sqrt(1 - b2 ** t)).add_(group['eps'])
            p.addcdiv_(state['exp_avg'], denom, value=-step_size)

    # ---- device path --------------------------------------------------------------------------------------------------------
    def _layout(self, entries):
        chunk = sis_hip.adam_chunk_elems()
        owner, offset, count = [], [], []
        for ti, (gi, p) in enumerate(entries):
            n = p.numel()
            for off in range(0, n, chunk):
                owner.append(ti)
                offset.append(4 * off)
                count.append(min(chunk, n - off) | (gi << 48))
        self._owner = np.asarray(owner, dtype=np.int64)
        self._offset = np.asarray(offset, dtype=np.int64)
        self._count = np.asarray(count, dtype=np.int64)
        self._n_chunks = len(owner)
        device = entries[0][1].device
        self._hosts = [[torch.empty((self._n_chunks, 5), dtype=torch.int64).pin_memory(), None] for _ in range(4)]
        self._flip = 0
        self._table = torch.empty((self._n_chunks, 5), dtype=torch.int64, device=device)
        self._partial = torch.empty(self._n_chunks, dtype=torch.float32, device=device)

    def push_hyper(self):
        """Copies lr / betas / eps / weight decay of ``param_groups`` and max_norm into the device tensor the step reads."""
        device = self.param_groups[0]['params'][0].device
        if self._hyper is None:
            self._hyper = torch.zeros(21, dtype=torch.float32, device=device)
            self._hyper_hosts = [[torch.zeros(21, dtype=torch.float32).pin_memory(), None] for _ in range(4)]
            self._hyper_slot = 0
        if self._table_key is not None and (self._capture_host is None or self._capture_host.shape[0] != self._n_chunks):
            self._capture_host = torch.empty((self._n_chunks, 5), dtype=torch.int64).pin_memory()
        self._hyper_slot = (self._hyper_slot + 1) % len(self._hyper_hosts)
        slot = self._hyper_hosts[self._hyper_slot]
        if slot[1] is not None:
            slot[1].synchronize()
        host = slot[0].numpy()
        host[:] = 0.0
        for gi, group in enumerate(self.param_groups):
            host[5 * gi:5 * gi + 5] = (group['lr'], group['betas'][0], group['betas'][1], group['eps'], group['weight_decay'])
        host[20] = self.max_norm
        self._hyper.copy_(slot[0], non_blocking=True)
        slot[1] = torch.cuda.current_stream(device).record_event()

    def _upload(self, entries, capturing):
        ptrs = np.asarray([(p.data_ptr(), p.grad.data_ptr(), self.state[p]['exp_avg'].data_ptr(),
                            self.state[p]['exp_avg_sq'].data_ptr()) for _, p in entries], dtype=np.int64)
        if capturing:
            pinned, slot = self._capture_host, None
        else:
            self._flip = (self._flip + 1) % len(self._hosts)
            slot = self._hosts[self._flip]
            if slot[1] is not None:
                slot[1].synchronize()
            pinned = slot[0]
        host = pinned.numpy()
        host[:, :4] = ptrs[self._owner] + self._offset[:, None]
        host[:, 4] = self._count
        self._table.copy_(pinned, non_blocking=True)
        if slot is not None:
            slot[1] = torch.cuda.current_stream(self._table.device).record_event()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        entries = [(gi, p) for gi, group in enumerate(self.param_groups) for p in group['params'] if p.grad is not None]
        if not entries:
            return loss
        if not entries[0][1].is_cuda:
            self._step_torch(entries)
            return loss
        sis_hip.flush_deferred()
        fresh = False
        for _, p in entries:
            if p.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous():
                raise RuntimeError("GradientClipAdam needs contiguous float32 parameters and gradients")
            state = self.state[p]
            if 'exp_avg' not in state:
                state['exp_avg'] = torch.zeros_like(p)
                state['exp_avg_sq'] = torch.zeros_like(p)
                fresh = True
        capturing = torch.cuda.is_current_stream_capturing()
        static_key = tuple(id(p) for _, p in entries)
        if static_key != self._table_key:
            if capturing:
                raise RuntimeError("GradientClipAdam: capture needs one eager step() and a push_hyper() call first")
            self._layout(entries)
            self._table_key = static_key
            self._grad_key = None
        if self._step_dev is None:
            self._step_dev = torch.zeros(1, dtype=torch.int32, device=entries[0][1].device)
        if capturing and (fresh or self._hyper is None or self._capture_host is None):
            raise RuntimeError("GradientClipAdam: capture needs one eager step() and a push_hyper() call first")
        if not capturing:
            self.push_hyper()
        # the update below bypasses torch's version counter: modules that keep state derived from a parameter (packed weight
        # images, folded BatchNorms, bf16 copies) watch this mark next to ``_version`` (sis_hip.weight_stamp)
        sis_hip.mark_written(p for _, p in entries)
        grad_key = tuple(p.grad.data_ptr() for _, p in entries)
        if grad_key != self._grad_key or capturing:
            self._upload(entries, capturing)
            self._grad_key = None if capturing else grad_key
        sis_hip.adam_clip_step(self._table, self._n_chunks, self._partial, self._hyper, self._step_dev)
        return loss
