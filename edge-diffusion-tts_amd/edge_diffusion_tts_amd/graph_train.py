"""GraphedTrainStep -- a whole training step as one graph launch.

The reference's trainer runs its decoder under ``torch.compile(mode="reduce-overhead")`` (train_v2.py:253-254), which is graph
replay.  Here the step itself -- key advance, forwards with dropout, objective, backward, clip, AdamW, EMA, blob mirror, learning
rate -- is captured once and replayed: the dropout keys and the noise seeds come from a ``KeyStream`` that the graph advances, the
learning rate from the optimiser's device-resident schedule or lr tensor, and blobs that no optimiser mirrors are packed inside the
graph.  Every replay is bitwise the eager step it stands for.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import torch

from . import native
from ._cache import capture_scope

__all__ = ["KeyStream", "GraphedTrainStep"]


class KeyStream(native.KeyStream):
    """``KeyStream(seed, n_slots, n_rows=0, device="cuda")``: ``n_slots`` dropout keys and ``n_rows`` noise seeds in device memory.

    ``advance()`` -- one capturable launch -- writes the keys of the next call counter; ``slot(k)`` is a 1-element view of dropout
    key k and ``rows()`` the int64 [n_rows] view that ``DiffusionObjective.prepare(seeds=...)`` takes.  Set
    ``decoder.dropout_keys = (keys, first_slot)`` (and on a ``SemanticEncoder``, with slots of its own): the module's n-th
    differentiable forward of a step then reads slot first_slot + n.  ``keys_at(counter)`` recomputes on the host what the advance
    with that counter wrote; ``counter()`` reads the device counter (synchronises)."""


class GraphedTrainStep:
    """``step = GraphedTrainStep(fn, optimizer, example_inputs, keys=None, warmup=1, accumulate=False)``;
    ``loss, *aux = step(*inputs, optimizer_step=True)``.

    ``fn(*static_inputs)`` returns a 0-dim loss, or a tuple that begins with it and continues with auxiliary tensors.  Construction
    runs ``warmup`` (>= 1) real eager steps on the example inputs -- they count as training steps -- and then captures one chain on
    one stream: ``keys.advance()`` -> ``fn`` -> ``loss.backward()`` -> ``optimizer.step()``; with ``accumulate=True`` also a second
    graph without the optimiser step, in the same memory pool.  A call copies the inputs into the static buffers, replays, and
    returns the static outputs (valid until the next call): the loss, the auxiliaries and, when the optimiser clips, the gradient
    norm as the last element (stepping replays only).

    Needs ``FusedAdamW(capturable=True, zero_grads=True)``.  With dropout the modules need ``dropout_keys`` from ``keys`` and device
    length tensors.  A replay bumps no tensor version, so by default each call does the step's host bookkeeping afterwards
    (``increment_version`` on the stepped parameters and EMA teachers, ``_mirror_commit`` on the mirrored decoders): any eager call
    after a replay sees the current parameters.  ``bookkeeping=False`` defers that to an explicit ``finish()``.
    ``SemanticEncoder(train_vq=True)`` and the compiled kernel families stay outside."""

    def __init__(self, fn: Callable, optimizer, example_inputs: Sequence[torch.Tensor], keys: Optional[KeyStream] = None, warmup: int = 1,
                 accumulate: bool = False, bookkeeping: bool = True):
        if not getattr(optimizer, "capturable", False) or not getattr(optimizer, "zero_grads", False):
            raise ValueError("GraphedTrainStep needs FusedAdamW(capturable=True, zero_grads=True): the captured step keeps its "
                             "pointers, and the gradients must stay allocated")
        if int(warmup) < 1:
            raise ValueError("GraphedTrainStep: warmup must be at least 1 (the optimiser's first step allocates and uploads: it is eager)")
        for i, x in enumerate(example_inputs):
            if not isinstance(x, torch.Tensor) or not x.is_cuda:
                raise ValueError(f"GraphedTrainStep: example input {i} must be a tensor on the HIP device")
        self.fn, self.optimizer, self.keys, self.bookkeeping = fn, optimizer, keys, bool(bookkeeping)
        self._static = [x.clone() for x in example_inputs]
        self._pending = 0
        for _ in range(int(warmup)):
            self._chain(True)
        torch.cuda.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        with capture_scope(), torch.cuda.graph(self._graph):
            self._out = self._chain(True)
        self._graph_acc, self._out_acc = None, None
        if accumulate:
            self._graph_acc = torch.cuda.CUDAGraph()
            with capture_scope(), torch.cuda.graph(self._graph_acc, pool=self._graph.pool()):
                self._out_acc = self._chain(False)
        # (the captures ran the optimiser's host bookkeeping without running a kernel: harmless, parameters and blobs did not move)

    def _chain(self, optimizer_step: bool) -> List[torch.Tensor]:
        if self.keys is not None:
            self.keys.advance()
        out = self.fn(*self._static)
        loss, aux = (out[0], list(out[1:])) if isinstance(out, (tuple, list)) else (out, [])
        if loss.dim() != 0:
            raise ValueError(f"GraphedTrainStep: fn must return a 0-dim loss (first), got shape {list(loss.shape)}")
        loss.backward()
        res = [loss.detach(), *[a.detach() for a in aux]]
        if optimizer_step:
            norm = self.optimizer.step()
            if norm is not None:
                res.append(norm)
        return res

    def __call__(self, *inputs: torch.Tensor, optimizer_step: bool = True):
        if len(inputs) != len(self._static):
            raise ValueError(f"GraphedTrainStep: expected {len(self._static)} inputs, got {len(inputs)}")
        if not optimizer_step and self._graph_acc is None:
            raise ValueError("GraphedTrainStep: optimizer_step=False needs accumulate=True at construction")
        for i, (dst, src) in enumerate(zip(self._static, inputs)):
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError(f"GraphedTrainStep: input {i}: expected {dst.dtype} {list(dst.shape)}, got {src.dtype} {list(src.shape)}")
            dst.copy_(src, non_blocking=True)
        if optimizer_step:
            self._graph.replay()
            self._pending += 1
            if self.bookkeeping:
                self.finish()
            return tuple(self._out)
        self._graph_acc.replay()
        return tuple(self._out_acc)

    def finish(self) -> None:
        """The host bookkeeping of the stepping replays since the last call: version bumps and mirror commits, so that every cache
        keyed on the parameters' versions sees the update.  Cheap when nothing is pending."""
        if not self._pending:
            return
        self._pending = 0
        self.optimizer.replay_bookkeeping()
