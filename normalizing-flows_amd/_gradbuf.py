"""Where a parameter's gradient is WRITTEN by the backward kernels.

The one-call layer backward (ops.coupling_train_bwd / nf_coupling_train_bwd) takes a destination address per gradient.  By
default that is a fresh tensor per parameter; dp.FlatParameters registers, for each of its parameters, a view of ONE flat gradient
buffer here, so the kernels write the whole model's gradient contiguously: the optimizer steps one flat tensor in one launch
(torch.optim.Adam(fused=True) on 608 parameter tensors: 17 launches, 0.72 ms per step of the benchmark model; on one flat
tensor: one launch, ~0.05 ms) and data-parallel all-reduces run on slices of that buffer in place (no torch.cat, no copy back).

A registered destination is handed out AT MOST ONCE per reset() (dp.FlatParameters.zero_grad / sync) and only while the parameter's
`.grad` is None.  Every later request gets a fresh tensor and autograd accumulates it the ordinary way.  Handing the slice out twice
would let the second backward overwrite the first one's gradient before autograd adds the two: a second micro-batch without zero_grad
(2 g2 instead of g1 + g2), two losses in one graph, or a torch.autograd.grad next to backward() writing into a `.grad` it must not touch.

The training Functions also count their forward uses of each registered parameter since zero_grad (use()): a count of 1 means no
second contribution can meet the first in the same graph, which autograd._pair_side_ok needs before it moves gradient writes to the
side stream (_sidestream.py).

Keyed by id() with a weak reference to the parameter (tensors cannot be dictionary keys by value); an entry dies with its
parameter or when its owner calls release().
"""
import weakref

import torch

_targets = {}      # id(param) -> [weakref to param, flat view, claimed since reset, training-Function forward uses since zero_grad]


def register(param, view):
    pid = id(param)

    def _gone(_, pid=pid):
        _targets.pop(pid, None)
    _targets[pid] = [weakref.ref(param, _gone), view, False, 0]


def release(param):
    _targets.pop(id(param), None)


def _entry(param):
    ent = _targets.get(id(param))
    if ent is None or ent[0]() is not param:
        return None
    return ent


def target(param):
    """The registered destination view of `param` (the registered object itself), or None."""
    ent = _entry(param)
    return None if ent is None else ent[1]


def reset(param, uses=True):
    """The registered slice may be handed out again (its content is no longer a gradient anybody relies on); uses=True also
    forgets the forward uses (a new step)."""
    ent = _entry(param)
    if ent is not None:
        ent[2] = False
        if uses:
            ent[3] = 0


def use(params):
    """A training Function's forward: one more use of every registered parameter in `params` (see sole_use)."""
    for p in params:
        ent = _targets.get(id(p))
        if ent is not None and ent[0]() is p:
            ent[3] += 1


def sole_use(param):
    """True when `param` is registered and exactly one training-Function forward has used it since zero_grad."""
    ent = _entry(param)
    return ent is not None and ent[3] == 1


def is_slice(param, t):
    """True when `t` (a tensor out() returned for `param`) is the registered destination itself."""
    v = target(param)
    return v is not None and t.data_ptr() == v.data_ptr()


def out(param):
    """A tensor the backward kernels write `param`'s gradient into: a FRESH view of the registered destination when it is unclaimed
    and `param.grad` is None (autograd's AccumulateGrad adopts a returned gradient without copying only when nobody else holds that
    tensor object), otherwise a new tensor."""
    ent = _entry(param)
    if ent is not None and not ent[2] and param.grad is None:
        v = ent[1]
        if v.dtype == param.dtype and v.device == param.device:
            ent[2] = True
            return v.view(v.shape)
    return torch.empty_like(param, memory_format=torch.contiguous_format)
