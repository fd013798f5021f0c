"""CPU suite: ``sis_hip.backward_scope`` (what belongs to one autograd backward) and ``sis_hip.may_complete_late`` (the one rule
for a gradient that is written after autograd has taken its tensor).  Everything here runs on CPU tensors inside the backward
of a small custom ``Function``: the rule is about autograd, not about kernels."""
import pytest
import torch
from torch import nn
from torch.autograd import Function


class _Inside(Function):
    """y = w; the backward calls ``fn(grad)`` -- code under test that has to run INSIDE a backward."""

    @staticmethod
    def forward(ctx, w, fn):
        ctx.fn = fn
        return w.clone()

    @staticmethod
    def backward(ctx, grad):
        ctx.fn(grad)
        return grad, None


class _Boom(Exception):
    pass


def _backward(w, fn, **kw):
    _Inside.apply(w, fn).sum().backward(**kw)


def test_may_complete_late_is_true_only_where_autograd_keeps_the_tensor_unread(monkeypatch):
    import sis_hip
    w, bias = nn.Parameter(torch.randn(3)), nn.Parameter(torch.randn(3))
    seen = []

    def ask(params, **kw):
        seen.clear()
        _backward(w, lambda g: seen.append(sis_hip.may_complete_late(params(), **kw)))
        w.grad = None
        return seen[0]

    both = lambda: (w, bias)
    assert ask(both) is True and ask(both, wgrad=False) is True and ask(tuple) is True
    assert sis_hip.may_complete_late((w, bias)) is False                    # outside a backward
    bias.grad = torch.zeros(3)                                               # a gradient in place: autograd ADDS the new one
    assert ask(both) is False and ask(lambda: (w,)) is True
    bias.grad = None
    for register in (bias.register_hook, bias.register_post_accumulate_grad_hook):   # both read the tensor the moment it arrives
        handle = register(lambda t: None)
        assert ask(both) is False and ask(both, wgrad=False) is False
        handle.remove()
        assert ask(both) is True
    vouching = lambda t: None
    vouching.completes_late_gradients = True                                 # (the data-parallel wrap's hook: it flushes before it reads)
    handle = bias.register_post_accumulate_grad_hook(vouching)
    assert ask(both) is True
    handle.remove()
    scaled = bias * 2
    assert ask(lambda: (w, scaled)) is False                                 # not a leaf: no AccumulateGrad takes its gradient
    seen.clear()
    _backward(w, lambda g: seen.append(sis_hip.may_complete_late((bias,))), create_graph=True)   # grad mode on: .grad is a COPY
    w.grad = None
    assert seen == [False]

    class Owner:
        pass

    owner = Owner()
    sis_hip.block_deferral(owner)                                            # a consumer that reads .grad inside the backward
    assert ask(both) is False and ask(both, wgrad=False) is False
    sis_hip.block_deferral(owner, False)
    assert ask(both) is True
    sis_hip.block_wgrad_deferral(owner)                                      # buckets leave during the backward: reductions only
    assert ask(both) is False and ask(both, wgrad=False) is True
    sis_hip.block_wgrad_deferral(owner, False)
    monkeypatch.setattr(sis_hip, "_DEFER_WGRAD", False)
    assert ask(both) is False and ask(both, wgrad=False) is True
    monkeypatch.setattr(sis_hip, "_DEFER", False)
    assert ask(both, wgrad=False) is False
    monkeypatch.undo()
    sis_hip.block_deferral(owner)                                            # ... and is released when its owner goes
    assert ask(both) is False
    del owner
    assert ask(both) is True and not sis_hip._defer_blockers


def test_at_end_runs_once_per_backward_and_key():
    from sis_hip import backward_scope as B
    w = nn.Parameter(torch.randn(3))
    calls, inside = [], []

    def request(g):
        for _ in range(3):
            inside.append(B.at_end("a", lambda: calls.append("a"), first=lambda: calls.append("first a")))
        inside.append(B.at_end("b", lambda: calls.append("b")))
        inside.append(B.at_end("a", lambda: calls.append("a again")))
        assert calls == ["first a"]                                          # nothing has run yet: the backward is still going

    assert B.at_end("a", lambda: calls.append("outside")) is False and not B.in_backward()
    scopes = []
    for _ in range(3):
        calls.clear()
        _backward(w, lambda g: (request(g), scopes.append(B._scope())))
        assert calls == ["first a", "a", "b"]
    assert inside == [True] * 15 and len({id(s) for s in scopes}) == 3       # one scope per backward
    del scopes
    assert len(B._scopes) == 0


def test_a_backward_that_raises_leaves_nothing_behind():
    from sis_hip import backward_scope as B
    w = nn.Parameter(torch.randn(3))
    calls = []
    big = torch.zeros(1000)

    def failing(g):
        B.at_end("a", lambda: calls.append("a of the failed backward"))
        B.hand_over("x", g, big.view(1000))
        assert B.pending_values() == 1
        raise _Boom()

    with pytest.raises(_Boom):
        _backward(w, failing)
    assert calls == [] and B.pending_values() == 0 and len(B._scopes) == 0   # the engine dropped the graph task and the scope with it
    assert big._use_count() == 1                                             # (the handed-over view is gone, not merely unreachable)
    got = []
    _backward(w, lambda g: (got.append(B.take("x", g)), B.at_end("a", lambda: calls.append("a"))))
    assert got == [None] and calls == ["a"] and len(B._scopes) == 0


def test_a_nested_backward_has_a_scope_of_its_own():
    from sis_hip import backward_scope as B
    w, v = nn.Parameter(torch.randn(3)), nn.Parameter(torch.randn(3))
    calls = []

    def outer(g):
        B.at_end("k", lambda: calls.append("outer"))
        B.hand_over("x", g, "of the outer backward")
        with torch.enable_grad():
            _backward(v, lambda h: (B.at_end("k", lambda: calls.append("inner")), calls.append(B.take("x", g))))
        calls.append(B.take("x", g))

    _backward(w, outer)
    assert calls == [None, "inner", "of the outer backward", "outer"]


def test_handed_over_value_is_for_the_same_address_and_version_only():
    from sis_hip import backward_scope as B
    w = nn.Parameter(torch.randn(4))
    got = []

    def handoff(g):
        g = g.clone()
        B.hand_over(("cast", 2), g, "cast")
        got.append(B.take(("cast", 2), g.view(2, 2)))                        # a view: same address, same version counter
        got.append(B.take(("cast", 2), g))                                   # taken once
        B.hand_over(("cast", 2), g, "cast")
        g.add_(1.0)                                                          # what autograd does for a second consumer
        got.append(B.take(("cast", 2), g))
        B.hand_over(("cast", 2), g, "cast")
        got.append(B.take(("cast", 2), g.clone()))                           # another tensor
        B.hand_over(("cast", 6), g, "left over")

    _backward(w, handoff)
    assert got == ["cast", None, None, None] and B.pending_values() == 0
    g = torch.zeros(4)
    B.hand_over("k", g, "outside a backward")
    assert B.take("k", g) is None and B.pending_values() == 0
