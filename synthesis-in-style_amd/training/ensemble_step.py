"""One training step of every member of a ``PixelEnsembleClassifier`` on the kernels of csrc/pixel_ensemble_train.h
(DESIGN.md §8): the members are batched inside the launches, so the number of launches per step -- apart from the members'
optimizers -- does not depend on how many members there are.

``FusedEnsembleStep(ensemble)`` stacks each kind of parameter of the members into one ``[N, ...]`` tensor.  Every member's
``nn.Parameter`` keeps its identity (optimizers created before or after see the same objects), its name and its ``state_dict``
key; only its storage moves: ``p.data`` and ``p.grad`` become contiguous views of the stacks, and so do the BatchNorm buffers.
Moving a member to another device afterwards (``.to``) would detach it from the stacks: build the step last.

Construction launches nothing and works on CPU tensors; ``step`` needs a HIP device and raises on anything the kernels do not
cover (``FusedEnsembleStep.unsupported`` says why) -- there is no quiet fallback here; choosing the ATen loop instead is the
updater's explicit decision (updater/dataset_gan_updater.py).
"""
from typing import Dict, Optional

import torch

import sis_hip

# kind -> (index into PixelClassifier.layers, attribute); the order of sis_hip.PE_TRAIN_PARAMS after the first layer
_KINDS = {"w1": (0, "weight"), "b1": (0, "bias"), "g1": (2, "weight"), "be1": (2, "bias"), "w2": (3, "weight"), "b2": (3, "bias"),
          "g2": (5, "weight"), "be2": (5, "bias"), "w3": (6, "weight"), "b3": (6, "bias")}
_BUFFERS = {"mean1": (2, "running_mean"), "var1": (2, "running_var"), "tracked1": (2, "num_batches_tracked"),
            "mean2": (5, "running_mean"), "var2": (5, "running_var"), "tracked2": (5, "num_batches_tracked")}


class FusedEnsembleStep:
    def __init__(self, ensemble, optimizers: Optional[Dict] = None):
        self.members = list(ensemble.get_networks().values())
        self.optimizers = optimizers
        reason = self.unsupported(ensemble)
        if reason:
            raise ValueError(f"FusedEnsembleStep: {reason}")
        first = self.members[0].layers
        self.n, self.features, self.classes = len(self.members), first[0].in_features, first[6].out_features
        self.stacks, self.grads, self.buffers = {}, {}, {}
        with torch.no_grad():
            for kind, (li, attr) in _KINDS.items():
                params = [getattr(m.layers[li], attr) for m in self.members]
                stack = torch.stack([p.detach() for p in params]).contiguous()
                grad = torch.zeros_like(stack)
                for i, p in enumerate(params):
                    p.data = stack[i]
                    p.grad = grad[i]
                self.stacks[kind], self.grads[kind] = stack, grad
            for name, (li, attr) in _BUFFERS.items():
                stack = torch.stack([getattr(m.layers[li], attr).detach() for m in self.members]).contiguous()
                for i, m in enumerate(self.members):
                    getattr(m.layers[li], attr).data = stack[i]
                self.buffers[name] = stack
        self._scratch = {}
        self._table_key, self._table = None, None

    @staticmethod
    def unsupported(ensemble) -> Optional[str]:
        """None when the fused path covers the ensemble, else the reason it does not."""
        members = list(ensemble.get_networks().values())
        if not 1 <= len(members) <= sis_hip.PE_TRAIN_MAX_MEMBERS:
            return f"{len(members)} members (1..{sis_hip.PE_TRAIN_MAX_MEMBERS})"
        first = members[0].layers
        shape = (first[0].in_features, first[0].out_features, first[3].out_features, first[6].out_features)
        if shape[1:3] != sis_hip.PE_TRAIN_HIDDEN:
            return (f"hidden widths {shape[1:3]}: the wide variant (32 or more classes) is not on the fused path -- its second "
                    f"layer (256 x 128 per member) does not fit the tail kernels' one-member-per-workgroup tiles")
        if not 2 <= shape[3] < 32:
            return f"{shape[3]} classes (2..31)"
        if shape[0] % 32:
            return f"{shape[0]} features (a multiple of 32)"
        for m in members:
            l = m.layers
            if (l[0].in_features, l[0].out_features, l[3].out_features, l[6].out_features) != shape:
                return "the members differ in shape"
            if not m.training:
                return "a member is in eval mode"
            if l[2].momentum != 0.1 or l[5].momentum != 0.1 or l[2].eps != 1e-5 or l[5].eps != 1e-5:
                return "BatchNorm momentum / eps differ from (0.1, 1e-5)"
            if any(p.dtype != torch.float32 for p in m.parameters()):
                return "parameters are not float32"
        if len({str(p.device) for m in members for p in m.parameters()}) != 1:
            return "the members live on different devices"
        return None

    @property
    def device(self):
        return self.stacks["w1"].device

    def _buffers_for(self, npix):
        if npix not in self._scratch:
            self._scratch.clear()   # one batch size at a time: the scratch of a 65536-pixel batch is not kept beside another
            dev, m = self.device, self.n * sis_hip.PE_TRAIN_HIDDEN[0]
            self._scratch[npix] = {
                "x": torch.empty((npix, self.features), dtype=torch.float32, device=dev),
                "a1": torch.empty((npix, m), dtype=torch.float32, device=dev),
                "dz1": torch.empty((npix, m), dtype=torch.float32, device=dev),
                "loss": torch.empty((2, self.n), dtype=torch.float32, device=dev),   # two slots: the caller may still read the last
                "tail_ws": torch.empty(sis_hip.pe_train_workspace_bytes(0, npix, self.features, self.n), dtype=torch.uint8, device=dev),
                "wgrad_ws": torch.empty(sis_hip.pe_train_workspace_bytes(1, npix, self.features, self.n), dtype=torch.uint8,
                                        device=dev),
                "flip": 0,
            }
        return self._scratch[npix]

    def _restore_grads(self):
        """``zero_grad(set_to_none=True)`` of an optimizer drops the views: put them back (the kernels overwrite every element)."""
        for kind, (li, attr) in _KINDS.items():
            for i, m in enumerate(self.members):
                p = getattr(m.layers[li], attr)
                if p.grad is None or p.grad.data_ptr() != self.grads[kind][i].data_ptr():
                    p.grad = self.grads[kind][i]

    @torch.no_grad()
    def forward_backward(self, x: torch.Tensor, labels: torch.Tensor, want_logits: bool = False):
        """Gradients of every member's mean cross-entropy on features x [P, F] into the stacked ``.grad``s, BatchNorm running
        statistics advanced -> (losses [N], logits [N, P, C] or None)."""
        if self.device.type != "cuda":
            raise RuntimeError("FusedEnsembleStep.step needs the ensemble on a HIP device")
        npix = x.shape[0]
        if npix < 2:
            raise ValueError("Expected more than 1 value per channel when training (BatchNorm1d), got a batch of one pixel")
        if x.shape[1] != self.features:
            raise ValueError(f"the ensemble classifies {self.features} features per pixel, the batch has {x.shape[1]}")
        s = self._buffers_for(npix)
        self._restore_grads()
        st, gr = self.stacks, self.grads
        a1 = sis_hip.pe_train_l1_forward(x, st["w1"].view(-1, self.features), st["b1"].view(-1), out=s["a1"])
        s["flip"] ^= 1
        tail = sis_hip.pe_train_tail(
            a1, labels, {k: st[k] for k in sis_hip.PE_TRAIN_PARAMS}, self.classes, running=self.buffers,
            grads={"d" + k: gr[k] for k in sis_hip.PE_TRAIN_PARAMS}, dz1=s["dz1"], loss=s["loss"][s["flip"]],
            want_logits=want_logits, workspace=s["tail_ws"])
        sis_hip.pe_train_l1_wgrad(tail["dz1"], x, dw1=gr["w1"].view(-1, self.features), db1=gr["b1"].view(-1), workspace=s["wgrad_ws"])
        return tail["loss"], tail["logits"]

    def step_features(self, x: torch.Tensor, labels: torch.Tensor, optimizers: Optional[Dict] = None) -> torch.Tensor:
        """forward_backward, then ``optimizer_{i}.step()`` of every member -> losses [N] on the device (no host sync)."""
        optimizers = optimizers if optimizers is not None else self.optimizers
        if optimizers is None:
            raise ValueError("FusedEnsembleStep: no optimizers given")
        loss, _ = self.forward_backward(x, labels)
        for i in range(self.n):
            optimizers[f"optimizer_{i}"].step()
        return loss

    def gather(self, pixels: torch.Tensor, dataset) -> torch.Tensor:
        layers = dataset.layers
        key = tuple(t.data_ptr() for t in layers)
        if key != self._table_key:
            self._table, self._table_key = sis_hip.pe_train_layer_table(layers), key
        return sis_hip.pe_train_gather(layers, pixels, dataset.image_size, table=self._table,
                                       out=self._buffers_for(pixels.shape[0])["x"])

    def step(self, pixels: torch.Tensor, labels: torch.Tensor, dataset, optimizers: Optional[Dict] = None) -> torch.Tensor:
        """pixels int32 [P, 3] = (image, y, x) and labels int64 [P] on the device, ``dataset`` holding the resident activation
        ``layers`` and ``image_size`` (data/dataset_gan_dataset.py) -> losses [N]."""
        if pixels.shape[0] < 2:
            raise ValueError("Expected more than 1 value per channel when training (BatchNorm1d), got a batch of one pixel")
        return self.step_features(self.gather(pixels, dataset), labels, optimizers)
