"""DatasetGAN's per-pixel MLP ensemble (reference: networks/pixel_classifier/model.py:13-121).

Same constructor arguments, member naming and state_dict schema as the reference.  ``forward`` is the plain ATen
``nn.Sequential`` (the A/B leg of tools/bench_dataset_gan.py, and training on CPU tensors; on a HIP device the ensemble is
trained by training/ensemble_step.py, all members per launch).  Labelling a generator's activations on a HIP
device goes through ``PixelEnsembleClassifier.fused_weights`` and ``sis_hip.pixel_ensemble_label``
(segmentation/dataset_gan_segmenter.py): eval mode only, BatchNorm folded into the following ``Linear``.
"""
from contextlib import contextmanager
from typing import Any, Dict, List, Sequence, Tuple

import torch
from torch import nn

from networks.base_segmenter import BaseSegmenter


class PixelEnsembleClassifier(BaseSegmenter):
    def __init__(self, numpy_class: int, dim: int, number_of_models: int):
        super().__init__()
        self.number_of_models = number_of_models
        self.networks = {}   # a plain dict, as in the reference: the members are not submodules of the ensemble
        self.last_net_id = 0
        for i in range(self.number_of_models):
            self.networks["network_{}".format(i)] = PixelClassifier(numpy_class, dim)
            self.networks["network_{}".format(i)].init_weights()
            self.last_net_id += 1
        self._fused = {}

    def get_networks(self) -> Dict[str, BaseSegmenter]:
        return self.networks

    def set_network(self, network_name: str, network: BaseSegmenter):
        self.networks[network_name] = network
        self._fused.clear()

    def add_network(self, network: BaseSegmenter):
        self.last_net_id += 1
        self.networks["network_{}".format(self.last_net_id)] = network
        self._fused.clear()

    def forward(self, x: Any):
        raise NotImplementedError

    def predict(self, x: Any):
        raise NotImplementedError

    def predict_classes(self, x: torch.Tensor) -> torch.Tensor:
        """[P, F] -> float [P]: the members' labels stacked as float [P, N], then ``torch.mode`` (the reference allocates the
        stack on 'cuda', model.py:41; here on the input's device)."""
        predictions = torch.zeros((x.shape[0], len(self.networks)), device=x.device)
        for i, model in enumerate(self.networks.values()):
            predictions[:, i] = model.predict_classes(x).squeeze()
        return torch.mode(predictions).values

    def fused_weights(self, layout: Sequence[Tuple[int, int]], size: int, device) -> Dict:
        """Device weights of the fused label pass for activation layers ``layout`` = [(channels, resolution)] in feature
        order, output size ``size`` (cached per layout; the members must be in eval mode and are not changed afterwards).

        {"full": [layer indices at full resolution], "w1f": [Kf][N*H1] k-major, "groups": [([layer indices], wt [K][N*H1])],
         "b1": [N*H1], "w2t": [N][H1][H2], "b2": [N][H2], "w3t": [N][H2][CP], "b3": [N][CP], "hidden1", "classes"}.
        BatchNorm y = s * relu(x) + t is folded into the following Linear in float64: W' = W diag(s), b' = W t + b."""
        device = torch.device(device)
        key = (tuple(layout), size, str(device))
        if key in self._fused:
            return self._fused[key]
        members = list(self.networks.values())
        if not members:
            raise ValueError("the ensemble has no members")
        h1, h2 = members[0].layers[0].out_features, members[0].layers[3].out_features
        classes, dim = members[0].layers[6].out_features, members[0].layers[0].in_features
        for m in members:
            if m.training:
                raise RuntimeError("the fused label pass runs the members in eval mode (ensemble_eval_mode / .eval())")
            if (m.layers[0].in_features, m.layers[0].out_features, m.layers[6].out_features) != (dim, h1, classes):
                raise ValueError("the ensemble's members differ in shape")
        if sum(c for c, _ in layout) != dim:
            raise ValueError(f"the ensemble classifies {dim} features per pixel, the activations have "
                             f"{sum(c for c, _ in layout)} channels")
        cp = 32 if h1 == 128 else 64
        offsets = [0]
        for c, _ in layout:
            offsets.append(offsets[-1] + c)
        w1 = torch.cat([m.layers[0].weight.detach().double().cpu() for m in members], 0)   # [N*H1, F]

        def k_major(idx: List[int]) -> torch.Tensor:
            return torch.cat([w1[:, offsets[i]:offsets[i + 1]] for i in idx], 1).t().contiguous()

        full = [i for i, (_, r) in enumerate(layout) if r == size]
        by_res: Dict[int, List[int]] = {}
        for i, (_, r) in enumerate(layout):
            if r != size:
                by_res.setdefault(r, []).append(i)
        groups = []
        for r in sorted(by_res, reverse=True):
            idx = by_res[r]
            groups += [idx[j:j + 2] for j in range(0, len(idx), 2)]
        w2t, b2, w3t, b3 = [], [], [], []
        for m in members:
            lin2, bn1, lin3, bn2 = m.layers[3], m.layers[2], m.layers[6], m.layers[5]
            s1, t1 = _bn_affine(bn1)
            s2, t2 = _bn_affine(bn2)
            w2, w3 = lin2.weight.detach().double().cpu(), lin3.weight.detach().double().cpu()
            w2t.append((w2 * s1[None]).t())
            b2.append(w2 @ t1 + lin2.bias.detach().double().cpu())
            pad = torch.zeros(h2, cp, dtype=torch.float64)
            pad[:, :classes] = (w3 * s2[None]).t()
            w3t.append(pad)
            pb = torch.zeros(cp, dtype=torch.float64)
            pb[:classes] = w3 @ t2 + lin3.bias.detach().double().cpu()
            b3.append(pb)

        def dev32(t):
            return t.to(device=device, dtype=torch.float32).contiguous()

        out = {
            "full": full, "w1f": dev32(k_major(full)) if full else None,
            "groups": [(idx, dev32(k_major(idx))) for idx in groups],
            "b1": dev32(torch.cat([m.layers[0].bias.detach().double().cpu() for m in members])),
            "w2t": dev32(torch.stack(w2t)), "b2": dev32(torch.stack(b2)),
            "w3t": dev32(torch.stack(w3t)), "b3": dev32(torch.stack(b3)),
            "hidden1": h1, "classes": classes,
        }
        self._fused[key] = out
        return out


def _bn_affine(bn: nn.BatchNorm1d) -> Tuple[torch.Tensor, torch.Tensor]:
    """Eval-mode BatchNorm1d as y = s * x + t (float64)."""
    s = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
    return s, bn.bias.detach().double().cpu() - bn.running_mean.detach().double().cpu() * s


@contextmanager
def ensemble_eval_mode(ensemble: PixelEnsembleClassifier):
    for network in ensemble.networks.values():
        network.eval()
    yield
    for network in ensemble.networks.values():
        network.train()


class PixelClassifier(BaseSegmenter):
    def __init__(self, numpy_class: int, dim: int):
        super().__init__()
        if numpy_class < 32:
            self.layers = nn.Sequential(
                nn.Linear(dim, 128),
                nn.ReLU(),
                nn.BatchNorm1d(num_features=128),
                nn.Linear(128, 32),
                nn.ReLU(),
                nn.BatchNorm1d(num_features=32),
                nn.Linear(32, numpy_class),
            )
        else:
            self.layers = nn.Sequential(
                nn.Linear(dim, 256),
                nn.ReLU(),
                nn.BatchNorm1d(num_features=256),
                nn.Linear(256, 128),
                nn.ReLU(),
                nn.BatchNorm1d(num_features=128),
                nn.Linear(128, numpy_class),
            )

    def init_weights(self, init_type: str = 'normal', gain: float = 0.02):
        """The reference's initialiser (pytorch-CycleGAN-and-pix2pix networks.py:39): Linear weights from the chosen
        distribution, biases zero.  Its BatchNorm2d branch never fires for these BatchNorm1d layers, as in the reference."""

        def init_func(m):
            classname = m.__class__.__name__
            if hasattr(m, 'weight') and (classname.find('Conv') != -1 or classname.find('Linear') != -1):
                if init_type == 'normal':
                    nn.init.normal_(m.weight.data, 0.0, gain)
                elif init_type == 'xavier':
                    nn.init.xavier_normal_(m.weight.data, gain=gain)
                elif init_type == 'kaiming':
                    nn.init.kaiming_normal_(m.weight.data, a=0, mode='fan_in')
                elif init_type == 'orthogonal':
                    nn.init.orthogonal_(m.weight.data, gain=gain)
                if hasattr(m, 'bias') and m.bias is not None:
                    nn.init.constant_(m.bias.data, 0.0)
            elif classname.find('BatchNorm2d') != -1:
                nn.init.normal_(m.weight.data, 1.0, gain)
                nn.init.constant_(m.bias.data, 0.0)

        self.apply(init_func)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.layers(x)

    def predict(self, x: torch.Tensor) -> torch.Tensor:
        return torch.log_softmax(self.forward(x), dim=1)

    def predict_classes(self, x: torch.Tensor) -> torch.Tensor:
        """The reference's BaseSegmenter.predict_classes (networks/base_segmenter.py:59-62): max over the classes of
        ``predict``, index kept as [P, 1]."""
        return torch.unsqueeze(torch.max(self.predict(x), dim=1)[1], dim=1)
