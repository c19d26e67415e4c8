"""FusedAdamW -- the tail of a training step on the library's kernels.

The reference's trainers run, after ``loss.backward()``: ``clip_grad_norm_(params, cfg.grad_clip)`` and ``AdamW.step()``
(train_v2.py:299-309; edge_diffusion_tts/train.py:160-170,245-249,279-281) and, in the consistency stage,
``ConsistencyTrainer.update_teacher()`` (training/consistency.py:45-50: ``lerp_`` over every parameter).  Here that is one call of
``edtts_optim_step`` -- two or three launches, no host synchronisation -- which also writes the new values into the packed blob of
an attached ``EdgeDiffusionDecoder(kernels="generic")``, so the next forward packs nothing.  There is no CPU path.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from . import native

__all__ = ["FusedAdamW", "CHUNK", "build_chunks", "cosine_lr"]


def __getattr__(name):  # CHUNK comes from the library (edtts_optim_chunk_size): read on first use, so importing needs no build
    if name == "CHUNK":
        return native.optim_chunk_size()
    raise AttributeError(name)


def build_chunks(numels) -> List[Tuple[int, int, int]]:
    """[(tensor index, first element, count)]: how a step cuts tensors of these sizes (the library's own table builder)."""
    return native.optim_chunk_table(list(numels))


def cosine_lr(step: int, total_steps: int, warmup_steps: int, base_lr: float, min_lr: float = 1e-6) -> float:
    """The learning rate ``train_v2.cosine_lr_schedule`` sets at ``step``: linear warm-up, then a cosine from base_lr to min_lr (the
    formula continues past total_steps).  ``FusedAdamW.device_lr_schedule("cosine", ...)`` evaluates it on the device."""
    if step < warmup_steps:
        return base_lr * step / max(warmup_steps, 1)
    progress = (step - warmup_steps) / max(total_steps - warmup_steps, 1)
    return min_lr + 0.5 * (base_lr - min_lr) * (1 + math.cos(math.pi * progress))


def _n_chunks(numel: int, chunk: int) -> int:
    return (numel + chunk - 1) // chunk


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (decoupled weight decay, no amsgrad) with the gradient clipping in front of it and, optionally, an EMA
    teacher and the decoder's packed blob behind it, as one pass of HIP kernels.

    ``max_norm``: None, or ``clip_grad_norm_``'s bound over every parameter of the optimiser that has a gradient; ``step()`` then
    returns the total norm (before clipping) as a 0-dim device tensor, otherwise None.  The gradients themselves are read, not
    rescaled in place (``clip_grad_norm_`` stores the scaled gradients; here they only enter the update).
    ``skip_nonfinite``: a step whose total norm is inf or NaN changes nothing at all and is counted in ``skipped_steps()``.
    ``zero_grads``: the step leaves every gradient it used zero-filled (the tensors stay; ``zero_grad(set_to_none=False)`` for free).

    Param groups carry ``lr`` / ``betas`` / ``eps`` / ``weight_decay`` as in torch (``cosine_lr_schedule`` and any LRScheduler work
    unchanged).  A parameter whose ``.grad`` is None is skipped as torch skips it: no state, no bit changed; so is a parameter
    without elements.  ONE device-resident step counter serves all parameters (it feeds the bias corrections): torch's per-parameter
    ``step`` is that counter for every parameter in ``state_dict()``, and ``load_state_dict()`` raises on unequal steps.
    Parameters must be contiguous fp32 tensors on one HIP device when ``step()`` runs; anything else raises.
    ``step()`` never synchronises; ``state_dict()`` reads the counter and may.

    ``capturable=True``: the step runs on a table that stays in device memory (``edtts_optim_upload`` once, then
    ``edtts_optim_step_resident``: no copy, no event, no host allocation), so it can be captured in a graph.
    The first step must be eager: it allocates the state and uploads the table.  Every later step compares the live pointers and
    hyper-parameters with the uploaded ones on the host; on a change it uploads again when the stream is not capturing and raises
    ``RuntimeError`` when it is.  ``group["lr"]`` may be a float (baked in at upload) or a 0-dim fp64 device tensor, read by the
    kernels at run time (``fill_`` it between replays, torch's capturable convention); ``device_lr_schedule`` makes the step
    compute its own learning rate from its device-resident counters.  Results are bitwise those of ``capturable=False``."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 *, max_norm: Optional[float] = None, skip_nonfinite: bool = False, zero_grads: bool = False, capturable: bool = False):
        if isinstance(lr, torch.Tensor):
            if not capturable:
                raise ValueError("FusedAdamW: a tensor lr needs capturable=True")
        elif not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_norm is not None and not float(max_norm) >= 0.0:
            raise ValueError(f"Invalid max_norm: {max_norm}")
        # (the keys torch.optim.AdamW keeps in a group, so that a state_dict loads there and back)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite, self.zero_grads = bool(skip_nonfinite), bool(zero_grads)
        self._scratch: Optional[torch.Tensor] = None
        self._host_step = 0          # the counter while there is no scratch yet (a loaded state_dict)
        self._decoders: List = []    # attach_decoder
        self._mirror: Dict = {}      # parameter -> (decoder index, offset floats, rows, cols, transposed)
        self._ema: Dict = {}         # student parameter -> (teacher tensor, decay)
        self._ema_pairs: List = []   # every (student, teacher, decay) of attach_ema, for update_ema
        self._ema_scratch: Optional[torch.Tensor] = None
        self.capturable = bool(capturable)
        self._uploaded = None        # capturable: what the table in the scratch was built from
        self._n_chunks = 0           # ... its number of chunks, and where its groups lie in the scratch
        self._groups_offset = 0
        self._lr_dev: Optional[torch.Tensor] = None   # fp64 [n_groups]: the run-time learning rates (tensor lrs are copied in each step)
        self._sched = None           # device_lr_schedule
        self._stepped = ([], [])     # the parameters and the mirrored decoders of the last step (replay_bookkeeping)

    # ------------------------------------------------------------------------------------------ attachments
    def attach_decoder(self, decoder) -> bool:
        """Mirror every step into ``decoder``'s packed blob: after a step whose blob was current -- packed, and packed from the
        parameters as they stood -- the blob holds the new values and the next forward packs nothing.  A stale blob is left alone
        and the next forward re-packs, as without this call.  Applies to ``kernels="generic"`` fp32 decoders (with or without
        AdaLN); for any other decoder this is a no-op -- its fragment-order blob re-packs as today -- and returns False."""
        table = decoder._mirror_map()
        if table is None:
            return False
        idx = len(self._decoders)
        self._decoders.append(decoder)
        decoder._blob.mirrored = True  # (under graph capture: a blob that a step keeps current is not packed inside the graph)
        for name, p in decoder.named_parameters():
            if name in table:
                self._mirror[p] = (idx, *table[name])
        return True

    def attach_ema(self, student_module, teacher_module, decay: float = 0.999) -> None:
        """``ConsistencyTrainer.update_teacher`` inside the step: teacher = lerp(teacher, student, 1 - decay) for every parameter of
        ``student_module`` THAT THE STEP UPDATES (a parameter without a gradient leaves its teacher alone -- torch's loop would
        still pull it toward the unchanged student; ``update_ema()`` is that loop).  Parameters pair by name.  A teacher that is a
        generic fp32 ``EdgeDiffusionDecoder`` has its blob mirrored like an attached decoder's."""
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"Invalid EMA decay: {decay}")
        teacher = dict(teacher_module.named_parameters())
        for name, p in student_module.named_parameters():
            if name not in teacher:
                raise KeyError(f"attach_ema: the teacher has no parameter {name!r}")
            if teacher[name].shape != p.shape:
                raise ValueError(f"attach_ema: {name}: student {tuple(p.shape)} and teacher {tuple(teacher[name].shape)} differ")
            self._ema[p] = (teacher[name], float(decay))
            self._ema_pairs.append((p, teacher[name], float(decay)))
        if hasattr(teacher_module, "_mirror_map"):
            self.attach_decoder(teacher_module)

    # ------------------------------------------------------------------------------------------ the step
    @staticmethod
    def _check(t: torch.Tensor, what: str, dev=None) -> int:
        if not t.is_cuda:
            raise native.EdttsError(f"FusedAdamW: {what}: expected a tensor on the HIP device, got {t.device} -- there is no CPU fallback")
        if t.dtype != torch.float32:
            raise native.EdttsError(f"FusedAdamW: {what}: expected dtype torch.float32, got {t.dtype}")
        if not t.is_contiguous():
            raise native.EdttsError(f"FusedAdamW: {what}: tensor must be contiguous")
        if dev is not None and t.device != dev:
            raise native.EdttsError(f"FusedAdamW: {what}: on {t.device}, the step runs on {dev}")
        return t.data_ptr()

    def device_lr_schedule(self, kind: str, base_lr: float, min_lr: float = 1e-6, warmup_steps: int = 0, total_steps: int = 1) -> None:
        """``capturable=True`` only: every step sets every group's lr itself, on the device, from the schedule evaluated at
        n = steps taken + steps skipped before it.  ``"cosine"`` is ``train_v2.cosine_lr_schedule`` in fp64 (``cosine_lr`` is the
        same formula on the host).  ``group["lr"]`` is then not read; ``current_lr()`` shows the values in force."""
        if not self.capturable:
            raise ValueError("FusedAdamW.device_lr_schedule needs capturable=True")
        self._sched = native.optim_schedule(kind, base_lr, min_lr, warmup_steps, total_steps)

    def current_lr(self) -> List[float]:
        """``capturable=True``: each group's learning rate as the last step left it on the device (synchronises); before the first
        step, the groups' own values."""
        if not self.capturable or self._uploaded is None:
            return [float(g["lr"]) for g in self.param_groups]
        n, size, at = len(self.param_groups), native.OPTIM_GROUP_BYTES, native.OPTIM_GROUP_LR_OFFSET
        raw = self._scratch[self._groups_offset:self._groups_offset + size * n].cpu().reshape(n, size)
        return [float(v) for v in raw[:, at:at + 8].contiguous().view(torch.float64).reshape(n)]

    def _resident_step(self, tab, n: int, groups, flags: int, scratch: torch.Tensor) -> None:
        capturing = torch.cuda.is_current_stream_capturing()
        n_groups = len(self.param_groups)
        lrs = [g["lr"] for g in self.param_groups]
        for lr in lrs:
            if isinstance(lr, torch.Tensor) and (lr.dtype != torch.float64 or lr.dim() != 0 or lr.device != scratch.device):
                raise native.EdttsError(f"FusedAdamW: a tensor lr must be a 0-dim fp64 tensor on {scratch.device}, got {lr.dtype} "
                                        f"{list(lr.shape)} on {lr.device}")
        # (the table as bytes: ctypes zero-fills its padding, so equal tables are equal bytes)
        key = (bytes(tab), bytes(groups), tuple(isinstance(lr, torch.Tensor) for lr in lrs), flags)
        if key != self._uploaded:
            if capturing:
                raise RuntimeError(f"FusedAdamW(capturable=True): the step's table changed under graph capture ({self._table_diff(key)}); "
                                   "a captured step needs the pointers and hyper-parameters of the last eager step (keep the "
                                   "gradients allocated: zero_grads=True, no zero_grad(set_to_none=True))")
            self._n_chunks, self._groups_offset = native.optim_upload(tab, n, groups, n_groups, flags, scratch)
            if self._lr_dev is None or self._lr_dev.device != scratch.device or self._lr_dev.numel() != n_groups:
                self._lr_dev = torch.zeros(n_groups, dtype=torch.float64, device=scratch.device)
            floats = torch.tensor([0.0 if isinstance(lr, torch.Tensor) else float(lr) for lr in lrs], dtype=torch.float64)
            self._lr_dev.copy_(native.host_to_device(floats, scratch.device))
            self._uploaded = key
        lr_dev = None
        if self._sched is None and any(isinstance(lr, torch.Tensor) for lr in lrs):
            for g, lr in enumerate(lrs):
                if isinstance(lr, torch.Tensor):
                    self._lr_dev[g].copy_(lr)  # (device to device on the current stream: capturable)
            lr_dev = self._lr_dev
        native.optim_step_resident(self._n_chunks, n_groups, self.max_norm, flags, scratch, lr_dev, self._sched)

    def _table_diff(self, key) -> str:
        """What differs between the table of this step and the uploaded one, for an error message."""
        old_t, old_g, old_kind, old_flags = self._uploaded
        if len(key[0]) != len(old_t):
            return "the number of tensors with a gradient"
        size = native.OPTIM_TENSOR_BYTES
        for i in range(0, len(key[0]), size):
            if key[0][i:i + size] != old_t[i:i + size]:
                field = next((f for f, at, n in native.OPTIM_TENSOR_FIELDS if key[0][i + at:i + at + n] != old_t[i + at:i + at + n]), "padding")
                return f"tensor {i // size}: {field}"
        if key[1] != old_g or key[2] != old_kind:
            return "a group's lr, betas, eps or weight_decay"
        return "the flags"

    def _ensure_scratch(self, dev) -> torch.Tensor:
        if self._scratch is None or self._scratch.device != dev:
            chunk = native.optim_chunk_size()
            n = sum(_n_chunks(p.numel(), chunk) for g in self.param_groups for p in g["params"])
            step = self._read_step()
            self._scratch = torch.zeros(native.optim_scratch_bytes(n, len(self.param_groups)), dtype=torch.uint8, device=dev)
            self._scratch_chunks = n
            self._uploaded = None  # (a new scratch holds no table)
            if step:
                self._write_step(step)
        return self._scratch

    def _read_step(self) -> int:
        if self._scratch is None:
            return self._host_step
        return int(self._scratch[:8].cpu().view(torch.int64)[0])

    def _write_step(self, step: int) -> None:
        self._host_step = int(step)
        if self._scratch is not None:
            self._scratch[:8].copy_(torch.tensor([int(step)], dtype=torch.int64).view(torch.uint8))

    def skipped_steps(self) -> int:
        """Steps that ``skip_nonfinite`` has dropped (reads the device counter: synchronises)."""
        return 0 if self._scratch is None else int(self._scratch[8:16].cpu().view(torch.int64)[0])

    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        if getattr(self, "_scratch", None) is not None:  # more chunks, another group: a larger scratch, the counters carried over
            step, skipped = self._read_step(), self._scratch[8:16].clone()
            self._host_step, self._scratch = step, None
            dev = skipped.device
            self._ensure_scratch(dev)[8:16].copy_(skipped)

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("FusedAdamW.step: a closure is not supported (compute the loss and call backward() first)")
        if self.capturable and self._uploaded is None and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            # (before anything is allocated: memory made under capture would never be zero-filled)
            raise RuntimeError("FusedAdamW(capturable=True): the first step() ran under graph capture; run one eager step first (it "
                               "allocates the optimiser state and uploads the table of pointers)")
        live, dev = [], None
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("FusedAdamW: amsgrad / maximize are not built")
            for p in group["params"]:
                g = p.grad
                if g is None or p.numel() == 0:
                    continue
                if dev is None:
                    self._check(p, "parameter")
                    dev = p.device
                live.append((gi, p, g))
        if not live:
            return None
        blobs = [d._mirror_target() for d in self._decoders]
        n = len(live)
        tab = (native.EdttsOptimTensor * n)()
        for i, (gi, p, g) in enumerate(live):
            e = tab[i]
            e.p = self._check(p, "parameter", dev)
            if g.is_sparse:
                raise native.EdttsError("FusedAdamW: sparse gradients are not supported")
            if g.shape != p.shape:
                raise native.EdttsError(f"FusedAdamW: gradient of shape {tuple(g.shape)} for a parameter of shape {tuple(p.shape)}")
            e.g = self._check(g, "gradient", dev)
            st = self.state[p]
            if "exp_avg" not in st:
                if self.capturable and torch.cuda.is_current_stream_capturing():
                    # (before its state is allocated: memory made under capture would never be zero-filled)
                    raise RuntimeError(f"FusedAdamW(capturable=True): the step's table changed under graph capture (parameter {i} of the "
                                       "step has a gradient for the first time); a captured step needs the tensors of the last eager step")
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            e.m = self._check(st["exp_avg"], "exp_avg", dev)
            e.v = self._check(st["exp_avg_sq"], "exp_avg_sq", dev)
            e.numel, e.group = p.numel(), gi
            mir = self._mirror.get(p)
            if mir is not None and blobs[mir[0]] is not None:
                e.mirror = blobs[mir[0]].data_ptr() + 4 * mir[1]
                if mir[4]:
                    e.rows, e.cols = mir[2], mir[3]
            ema = self._ema.get(p)
            if ema is not None:
                e.ema = self._check(ema[0], "EMA target", dev)
                e.ema_decay = ema[1]
                tm = self._mirror.get(ema[0])
                if tm is not None and blobs[tm[0]] is not None:
                    e.ema_mirror = blobs[tm[0]].data_ptr() + 4 * tm[1]
                    if tm[4]:
                        e.rows, e.cols = tm[2], tm[3]
        groups = (native.EdttsOptimGroup * len(self.param_groups))()
        for gi, group in enumerate(self.param_groups):
            q = groups[gi]
            lr = group["lr"]
            q.lr = 0.0 if self.capturable and isinstance(lr, torch.Tensor) else float(lr)
            q.eps, q.weight_decay = float(group["eps"]), float(group["weight_decay"])
            q.beta1, q.beta2 = float(group["betas"][0]), float(group["betas"][1])
        scratch = self._ensure_scratch(dev)
        flags = (native.OPT_SKIP_NONFINITE if self.skip_nonfinite else 0) | (native.OPT_ZERO_GRADS if self.zero_grads else 0)
        if self.capturable:
            self._resident_step(tab, n, groups, flags, scratch)
        else:
            native.optim_step(tab, n, groups, len(self.param_groups), self.max_norm, flags, scratch)
        self._stepped = ([p for _, p, _ in live], [d for d, blob in zip(self._decoders, blobs) if blob is not None])
        self.replay_bookkeeping()
        if self.max_norm is None:
            return None
        return scratch[16:20].view(torch.float32).reshape(()).clone()

    def replay_bookkeeping(self) -> None:
        """The host side of the last ``step()`` once more: what a replay of a graph that captured that step leaves undone.  Every
        cache keyed on the parameters' versions (the decoder blob, the semantic-head blobs) sees an in-place update, and the
        decoders whose blob the step mirrored are current again."""
        params, decoders = self._stepped
        bump = torch.autograd.graph.increment_version
        for p in params:
            bump(p)
            ema = self._ema.get(p)
            if ema is not None:
                bump(ema[0])
        for d in decoders:
            d._mirror_commit()

    @torch.no_grad()
    def update_ema(self) -> None:
        """``ConsistencyTrainer.update_teacher`` as torch runs it: every pair of ``attach_ema``, stepped or not."""
        pairs = [(s, t, d) for s, t, d in self._ema_pairs if s.numel()]
        if not pairs:
            return
        dev = pairs[0][0].device
        blobs = [d._mirror_target() for d in self._decoders]
        tab = (native.EdttsOptimTensor * len(pairs))()
        for e, (s, t, decay) in zip(tab, pairs):
            e.p, e.ema = self._check(s, "parameter", dev), self._check(t, "EMA target", dev)
            e.numel, e.ema_decay = s.numel(), decay
            tm = self._mirror.get(t)
            if tm is not None and blobs[tm[0]] is not None:
                e.ema_mirror = blobs[tm[0]].data_ptr() + 4 * tm[1]
                if tm[4]:
                    e.rows, e.cols = tm[2], tm[3]
        if self._ema_scratch is None or self._ema_scratch.device != dev:
            chunk = native.optim_chunk_size()
            self._ema_scratch = torch.zeros(native.optim_scratch_bytes(sum(_n_chunks(s.numel(), chunk) for s, _, _ in pairs), 1),
                                            dtype=torch.uint8, device=dev)
        groups = (native.EdttsOptimGroup * 1)()
        native.optim_step(tab, len(pairs), groups, 1, None, native.OPT_EMA_ONLY, self._ema_scratch)
        for _, t, _ in pairs:
            torch.autograd.graph.increment_version(t)
        teachers = {id(t) for _, t, _ in pairs}
        for d, blob in zip(self._decoders, blobs):
            if blob is not None and any(id(p) in teachers for p in d.parameters()):
                d._mirror_commit()

    # ------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """torch.optim.AdamW's format: per parameter ``step`` (a float32 0-dim CPU tensor: the shared counter), ``exp_avg``,
        ``exp_avg_sq``.  Reads the device counter (synchronises)."""
        step = float(self._read_step())
        sd = super().state_dict()
        sd["state"] = {k: dict(v, step=torch.tensor(step, dtype=torch.float32)) for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict) -> None:
        steps = {float(v["step"]) for v in state_dict["state"].values() if "step" in v}
        if len(steps) > 1:
            raise ValueError(f"FusedAdamW keeps one step counter for all parameters; the state holds steps {sorted(steps)}")
        for g in state_dict["param_groups"]:
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError("FusedAdamW: amsgrad / maximize are not built")
        super().load_state_dict(state_dict)
        for st in self.state.values():
            st.pop("step", None)
            st.pop("max_exp_avg_sq", None)
        self._write_step(int(steps.pop()) if steps else 0)
