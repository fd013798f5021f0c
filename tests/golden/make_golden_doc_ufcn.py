"""Maker of tests/golden/doc_ufcn_step.npz: the UNMODIFIED reference DocUFCN (networks/doc_ufcn/doc_ufcn.py of the reference
tree) on the CPU, imported by file path with the bare packages and the cv2 stub of oracle/load_reference.py.

Config: B = 2, 64^2, dropout p = 0, class weights (1, 2, 0.5); weights from ``seeded_state_dict`` (a numpy stream defined here);
two iterations of forward -> weighted CE -> backward -> clip_grad_norm_(1.0) + Adam(lr 5e-3, betas (0.5, 0.999), weight decay
1e-4).  Recorded: logits, losses, per-parameter gradient norms, a gradient sample, running statistics after each iteration, and
the reference state_dict key / shape list of the three variants.  The test imports this module for ``seeded_state_dict`` /
``seeded_batch`` / ``CONFIG``; only the outputs are stored.

    python tests/golden/make_golden_doc_ufcn.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIG = dict(batch=2, size=64, class_weights=(1.0, 2.0, 0.5), lr=5e-3, betas=(0.5, 0.999), weight_decay=1e-4, max_norm=1.0,
              iterations=2)
VARIANTS = ('base', 'no_dropout', 'pixelshuffle')


def seeded_state_dict(schema, seed=7):
    """{key: tensor} for a state_dict schema [(key, shape)]: weights ~ N(0, 1/fan_in), BN scales ~ U(0.5, 1.5), biases small,
    running stats (0, 1), num_batches_tracked 0."""
    rng = np.random.RandomState(seed)
    sd = {}
    for key, shape in schema:
        if key.endswith('num_batches_tracked'):
            sd[key] = torch.tensor(0, dtype=torch.int64)
        elif key.endswith('running_mean'):
            sd[key] = torch.zeros(shape)
        elif key.endswith('running_var'):
            sd[key] = torch.ones(shape)
        elif key.endswith('bn.weight'):
            sd[key] = torch.from_numpy(rng.uniform(0.5, 1.5, shape).astype(np.float32))
        elif key.endswith('bias'):
            sd[key] = torch.from_numpy((0.1 * rng.randn(*shape)).astype(np.float32))
        else:
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
            sd[key] = torch.from_numpy((rng.randn(*shape) / np.sqrt(fan_in)).astype(np.float32))
    return sd


def seeded_batch(seed=8):
    rng = np.random.RandomState(seed)
    b, s = CONFIG['batch'], CONFIG['size']
    x = torch.from_numpy(rng.randn(b, 3, s, s).astype(np.float32))
    y = torch.from_numpy(rng.randint(0, 3, (b, s, s)).astype(np.int64))
    return x, y


def run_step(net, iterations=None):
    """Two iterations of the reference training step on ``net`` (train mode) -> dict of recorded arrays."""
    x, y = seeded_batch()
    w = torch.tensor(CONFIG['class_weights'])
    opt = torch.optim.Adam(net.parameters(), lr=CONFIG['lr'], betas=CONFIG['betas'], weight_decay=CONFIG['weight_decay'])
    out = {}
    names = [n for n, _ in net.named_parameters()]
    for it in range(iterations or CONFIG['iterations']):
        opt.zero_grad()
        logits = net(x)
        loss = F.cross_entropy(logits, y, weight=w)
        loss.backward()
        out[f'logits{it}'] = logits.detach().numpy()
        out[f'loss{it}'] = np.float64(loss.item())
        out[f'grad_norms{it}'] = np.array([p.grad.norm().item() for p in net.parameters()])
        out[f'grad_sample{it}'] = np.concatenate([p.grad.reshape(-1)[:4].numpy() for p in net.parameters()])
        torch.nn.utils.clip_grad_norm_(list(net.parameters()), CONFIG['max_norm'])
        opt.step()
        out[f'running{it}'] = np.concatenate([b.reshape(-1).numpy() for n, b in net.named_buffers() if 'running' in n])
    out['param_names'] = np.array(names)
    return out


def _load_reference_doc_ufcn():
    """The reference module, with the bare ``networks`` / ``utils`` packages of oracle/load_reference.py (a fresh process)."""
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle.load_reference import load_reference_segmenters
    load_reference_segmenters()
    return importlib.import_module('networks.doc_ufcn.doc_ufcn')


def main():
    torch.manual_seed(0)
    R = _load_reference_doc_ufcn()
    classes = {'base': R.DocUFCN, 'no_dropout': R.DocUFCNNoDropout, 'pixelshuffle': R.PixelShuffleDocUFCN}
    out = {}
    for v in VARIANTS:
        sd = classes[v](3, 3).state_dict()
        out[f'keys_{v}'] = np.array(list(sd))
        out[f'shapes_{v}'] = np.array([','.join(map(str, t.shape)) for t in sd.values()])
    net = R.DocUFCN(3, 3, encoder_dropout_prob=0.0, decoder_dropout_prob=0.0)
    schema = [(k, tuple(t.shape)) for k, t in net.state_dict().items()]
    net.load_state_dict(seeded_state_dict(schema), strict=True)
    net.train()
    out.update(run_step(net))
    np.savez_compressed(os.path.join(HERE, 'doc_ufcn_step.npz'), **out)


if __name__ == '__main__':
    main()
