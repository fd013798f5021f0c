"""What belongs to ONE autograd backward: work that runs once at its end, values that live until then, and the rule for a
gradient that is completed only after autograd has taken its tensor.

Every running backward (a graph task of the engine; their ids are drawn from a process-wide counter and never repeat) gets one
``_Scope`` on first use.  The scope is OWNED by the engine: the only strong reference to it is the final callback queued on its
graph task, this module finds it through a weak one.  A backward that ends runs the callback and releases it; a backward that
RAISES runs no callback, but the engine drops the graph task, and the scope, its queued functions and its values go with it
before ``backward()`` has returned to the caller.  So nothing of a failed backward is left to suppress, misdirect or keep
alive anything in a later one, and a nested backward has a scope of its own beside the enclosing one's.

Pure Python on torch alone: importable without the native library.
"""
import weakref

import torch

_scopes = weakref.WeakValueDictionary()   # graph task id -> _Scope (kept alive by that graph task's final callback)


class _Scope:
    def __init__(self):
        self.at_end = {}   # key -> function, in the order of their first request
        self.values = {}

    def close(self):
        self.values.clear()
        while self.at_end:   # (a function may request another one)
            self.at_end.pop(next(iter(self.at_end)))()


def _scope():
    task = torch._C._current_graph_task_id()
    if task < 0:
        return None
    scope = _scopes.get(task)
    if scope is None:
        scope = _scopes[task] = _Scope()
        torch.autograd.Variable._execution_engine.queue_callback(scope.close)
    return scope


def in_backward():
    return torch._C._current_graph_task_id() >= 0


def at_end(key, fn, first=None):
    """``fn()`` runs once when the running backward has finished, however often it is requested under ``key``; different keys
    run in the order of their first request.  ``first()`` runs now if this is the first request of ``key`` in this backward
    (state that a backward which raised left half-way is put right there).  False outside a backward: nothing is queued."""
    scope = _scope()
    if scope is None:
        return False
    if key not in scope.at_end:
        scope.at_end[key] = fn
        if first is not None:
            first()
    return True


def hand_over(key, tensor, value):
    """Keeps ``value``, computed from ``tensor`` as it is now, for whoever receives that tensor later in this backward."""
    scope = _scope()
    if scope is not None:
        scope.values[key] = (tensor.data_ptr(), tensor._version, value)


def take(key, tensor):
    """The value handed over under ``key`` if ``tensor`` is the one it was computed from, unchanged: same address AND same
    version (autograd adds the gradient of a second consumer in place -- same address, other contents).  None otherwise."""
    scope = _scope()
    address, version, value = scope.values.pop(key, (None, None, None)) if scope is not None else (None, None, None)
    return value if (address, version) == (tensor.data_ptr(), tensor._version) else None


def pending_values():
    """Number of handed-over values of all live backwards (tests: none outside a backward)."""
    return sum(len(s.values) for s in _scopes.values())


def taken_as_is(params):
    """True when autograd's AccumulateGrad KEEPS the tensor it is handed as the gradient of each of ``params`` and nothing reads
    that tensor before the backward ends -- the condition under which a kernel may write it late.  Inside a backward only; with
    grad mode on (``create_graph=True``) the gradient is copied; a parameter that already has a gradient gets the new one ADDED
    on the spot; a tensor hook or a post-accumulate-grad hook reads it the moment it arrives -- unless the hook vouches, by an
    attribute ``completes_late_gradients = True``, that it has them completed before it reads one (the data-parallel wrap)."""
    return (in_backward() and not torch.is_grad_enabled()
            and all(p.is_leaf and p.grad is None and not p._backward_hooks
                    and all(getattr(hook, "completes_late_gradients", False) for hook in (p._post_accumulate_grad_hooks or {}).values())
                    for p in params))
