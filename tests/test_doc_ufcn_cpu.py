"""DocUFCN without a GPU: builder lookup, the reference's state_dict schema, the plain-torch path against the reference fixture
(tests/golden/doc_ufcn_step.npz, made by tests/golden/make_golden_doc_ufcn.py from the unmodified reference), and the host
path of GradientClipAdam against clip_grad_norm_ + torch.optim.Adam."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_golden_doc_ufcn as G  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "doc_ufcn_step.npz"))


def test_builder_selection_returns_doc_ufcn_builder():
    from training_builder.doc_ufcn_train_builder import DocUFCNTrainBuilder
    from training_builder.train_builder_selection import get_train_builder_class
    assert get_train_builder_class({'network': 'DocUFCN'}) is DocUFCNTrainBuilder
    with pytest.raises(NotImplementedError):
        get_train_builder_class({'network': 'PixelEnsemble'})


def test_builder_builds_reference_network_and_optimizer():
    from networks.doc_ufcn import DocUFCN
    from training.fused_adam import GradientClipAdam
    from training_builder.doc_ufcn_train_builder import DocUFCNTrainBuilder
    cfg = {'network': 'DocUFCN', 'lr': 1e-3, 'beta1': 0.5, 'beta2': 0.99, 'weight_decay': 1e-4, 'class_weights': [1, 2, 0.5]}
    builder = DocUFCNTrainBuilder(cfg)
    net = builder.get_network()
    assert type(net) is DocUFCN and net.num_classes == 3 and net.num_input_channels == 3 and net.min_contour_area == 55
    opt = builder.get_optimizers()['main']
    assert isinstance(opt, GradientClipAdam) and opt is builder.get_optimizers()['main']
    assert opt.param_groups[0]['betas'] == (0.5, 0.99) and opt.param_groups[0]['weight_decay'] == 1e-4


@pytest.mark.parametrize("variant", G.VARIANTS)
def test_state_dict_schema_matches_reference(fixture, variant):
    from networks.doc_ufcn import get_doc_ufcn
    sd = get_doc_ufcn(variant)(3, 3).state_dict()
    assert list(sd) == list(fixture[f'keys_{variant}'])
    assert [','.join(map(str, t.shape)) for t in sd.values()] == list(fixture[f'shapes_{variant}'])
    get_doc_ufcn(variant)(3, 3).load_state_dict(sd, strict=True)


def test_cpu_step_matches_reference_fixture(fixture):
    from networks.doc_ufcn import DocUFCN
    net = DocUFCN(3, 3, encoder_dropout_prob=0.0, decoder_dropout_prob=0.0)
    schema = [(k, tuple(t.shape)) for k, t in net.state_dict().items()]
    net.load_state_dict(G.seeded_state_dict(schema), strict=True)
    net.train()
    out = G.run_step(net)
    assert list(out['param_names']) == list(fixture['param_names'])
    for it in range(G.CONFIG['iterations']):
        ref = fixture[f'logits{it}']
        assert np.abs(out[f'logits{it}'] - ref).max() <= 1e-5 * np.abs(ref).max()
        assert abs(out[f'loss{it}'] - fixture[f'loss{it}']) <= 1e-5 * abs(fixture[f'loss{it}'])
        np.testing.assert_allclose(out[f'grad_norms{it}'], fixture[f'grad_norms{it}'], rtol=1e-3, atol=1e-6)
        np.testing.assert_allclose(out[f'running{it}'], fixture[f'running{it}'], rtol=1e-5, atol=1e-6)


def test_input_size_must_be_multiple_of_eight():
    from networks.doc_ufcn import DocUFCN
    with pytest.raises(ValueError, match="multiples of 8"):
        DocUFCN(3, 3)(torch.randn(1, 3, 60, 64))


@pytest.mark.parametrize("scale", [0.01, 10.0])   # clipping inactive / active
def test_gradient_clip_adam_host_path(scale):
    from training.fused_adam import GradientClipAdam
    g = torch.Generator().manual_seed(2)
    shapes = [(8, 4, 3, 3), (8,), (5, 7)]
    init = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    grads = [[torch.randn(s, generator=g, dtype=torch.float64) * scale for s in shapes] for _ in range(3)]
    hp = dict(lr=5e-3, betas=(0.5, 0.999), weight_decay=1e-4, eps=1e-8)
    mine = [p.clone().requires_grad_() for p in init]
    ref = [p.clone().requires_grad_() for p in init]
    opt = GradientClipAdam(mine, max_norm=1.0, **hp)
    ref_opt = torch.optim.Adam(ref, **hp)
    clipped = []
    for step in grads:
        for p, q, gr in zip(mine, ref, step):
            p.grad, q.grad = gr.clone(), gr.clone()
        opt.step()
        clipped.append(torch.nn.utils.clip_grad_norm_(ref, 1.0).item() > 1.0)
        ref_opt.step()
    assert all(clipped) == (scale > 1) and any(clipped) == (scale > 1)
    for a, b in zip(mine, ref):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-14)
