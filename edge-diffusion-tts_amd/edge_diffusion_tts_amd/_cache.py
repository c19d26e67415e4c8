"""The host state every module keeps in front of the kernels: one packed weight blob, re-packed when a
parameter changes and ordered across streams, and a bounded cache of per-stream workspaces.  Both guard their bookkeeping with a
lock of their own that is never held across a GPU wait, and a copy or a pickle of either starts empty with a new lock."""
from __future__ import annotations

import contextlib
import threading
import warnings

import torch

from .native import EdttsError


# Graph capture.  A replay bumps no tensor version, so a blob packed from trainable tensors that no optimiser
# mirrors would be stale on the second replay: while a stream is capturing, such a blob is packed INSIDE the capture, so every
# replay packs from the parameters as they then stand.  Whether a call trains is the caller's to say (get(trainable=True): the
# differentiable forwards and their backwards -- torch runs both with grad mode off, so it cannot be read there); an inference
# call's capture is as before.  Once per capture is enough, and who captures says where a capture begins: capture_scope()
# (GraphedTrainStep opens one per graph).  Outside any scope every trainable get() under capture packs.
_capture_epoch = 0
_in_scope = False


@contextlib.contextmanager
def capture_scope():
    """One graph capture: a trainable, unmirrored PackedBlob is packed once inside it, at its first get()."""
    global _capture_epoch, _in_scope
    _capture_epoch += 1
    prev, _in_scope = _in_scope, True
    try:
        yield
    finally:
        _in_scope = prev


class PackedBlob:
    """One packed blob, the signature of the tensors it was packed from and the event that orders other streams behind the pack.
    ``nbytes_of(key)`` and ``pack(key, tensors, blob)`` are the library's byte-count query and pack call, and ``key`` is what they
    take first: the module's dims, which compare by value (HuBERT binds its compute dtype into the two calls).  Changing parameters
    while calls that read the old blob are still in flight on other streams is the caller's to order, as for any module."""

    def __init__(self, nbytes_of, pack, what: str = "weight"):
        self.__setstate__((nbytes_of, pack, what))

    # copies (copy.deepcopy, pickling) keep the callables only: a copied blob could never match the copy's tensors
    def __getstate__(self):
        return self._nbytes_of, self._pack, self._what

    def __setstate__(self, state):
        self._nbytes_of, self._pack, self._what = state
        self._lock = threading.Lock()
        self.blob = None
        self.sig = None         # signature of the last pack
        self._event = None      # recorded on the packing stream right behind the last pack (GPU blobs only)
        self._waited = set()    # streams that have waited for it
        self.mirrored = False   # an optimiser writes every update into the blob as well (FusedAdamW.attach_decoder)
        self._cap_epoch = None  # the capture scope that has packed it

    @staticmethod
    def signature(key, tensors):
        """``key``, the device and each tensor's (storage pointer, version).  The device is read once: a pack checks that all tensors
        are on one device, a tensor that moves gets new storage, and a device read per tensor costs a decoder call (93 tensors, B = 1:
        the host-limited case of DESIGN.md section 10) a third more than the rest of the signature."""
        return (key, tensors[0].device) + tuple((t.data_ptr(), t._version) for t in tensors)

    def _record(self) -> None:
        self._event, self._waited = None, set()
        # (not while capturing: an event recorded inside a capture cannot order an eager stream, and the pack has not run)
        if self.blob.is_cuda and not torch.cuda.is_current_stream_capturing():
            stream = torch.cuda.current_stream(self.blob.device)
            self._event = torch.cuda.Event()
            self._event.record(stream)
            self._waited.add(stream.cuda_stream)

    def _wait_once(self, while_capturing: bool) -> None:
        if self._event is not None:
            stream = torch.cuda.current_stream(self.blob.device)
            if stream.cuda_stream not in self._waited and (while_capturing or not torch.cuda.is_current_stream_capturing()):
                stream.wait_event(self._event)  # (enqueues a wait; the host does not block)
                self._waited.add(stream.cuda_stream)

    def get(self, key, tensors, packs=None, names=None, trainable: bool = False) -> torch.Tensor:
        """The blob, (re-)packed on the current stream when ``key`` or a tensor's storage, version or device changed.  A call on
        another stream waits once per pack for the event recorded behind it, so its first use is ordered after the pack (not while
        capturing: a capture follows an eager warm-up, and torch.cuda.graph synchronises the device before it starts).
        ``packs``: a callable that returns the tensors to pack where they are not ``tensors`` themselves, called on a miss only;
        ``names``: what to call each of them in an error, by default its index.  ``trainable``: the call belongs to a training
        step (a differentiable forward or its backward): under graph capture the blob is then packed inside the capture unless an
        optimiser mirrors it or no tensor requires grad (see capture_scope)."""
        with self._lock:
            sig = self.signature(key, tensors)
            if self.blob is None or sig != self.sig or (trainable and self._pack_in_capture(tensors)):
                src = tensors if packs is None else packs()
                dev = src[0].device
                for i, t in enumerate(src):
                    if t.device != dev or t.dtype != torch.float32:
                        raise EdttsError(f"{self._what} {i if names is None else names[i]}: expected fp32 on {dev}, got {t.dtype} on {t.device}")
                nbytes = self._nbytes_of(key)
                if self.blob is None or self.blob.numel() != nbytes or self.blob.device != dev:
                    self.blob = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                self._pack(key, [t.detach().contiguous() for t in src], self.blob)
                self.sig = sig
                self._record()
            else:
                self._wait_once(False)
            return self.blob

    def _pack_in_capture(self, tensors) -> bool:
        """A trainable get(): True when the stream is capturing and the blob must be packed inside the capture (see capture_scope)."""
        if self.mirrored or not self.blob.is_cuda or not torch.cuda.is_current_stream_capturing():
            return False
        if _in_scope and self._cap_epoch == _capture_epoch:
            return False
        if not any(t.requires_grad for t in tensors):
            return False
        self._cap_epoch = _capture_epoch
        return True

    def invalidate(self) -> None:
        """The next get() packs again although no tensor's version moved (a kernel wrote into a packed tensor's storage)."""
        with self._lock:
            self.sig = None

    def current(self, key, tensors):
        """The blob if it is packed from the tensors as they stand, else None.  The current stream is ordered behind the pack, so work
        enqueued on it may write new values into the blob."""
        with self._lock:
            if self.blob is None or self.sig != self.signature(key, tensors):
                return None
            self._wait_once(True)
            return self.blob

    def commit(self, key, tensors) -> None:
        """After work on the current stream that wrote the tensors' new values into the blob as well: the blob is current again."""
        with self._lock:
            self.sig = self.signature(key, tensors)
            self._record()


class WorkspaceCache:
    """Scratch tensors per (head..., stream), least recently used first in ``entries``.  A workspace belongs to the stream it was
    made for, so calls on several streams (from one thread or several) never share one.  At most ``owner.WORKSPACE_CACHE`` are kept;
    the least recently USED one is dropped to make room -- never one that a captured hipGraph points at: a workspace handed out while
    the stream was capturing is pinned until ``release_pinned`` (a replay writes into it)."""

    def __init__(self):
        self.__setstate__({})

    def __getstate__(self):  # copies (copy.deepcopy, pickling) start empty
        return {}

    def __setstate__(self, state):
        self._lock = threading.Lock()
        self.entries = {}
        self.pinned = set()  # keys handed out during graph capture (never evicted)

    def get(self, owner, head: tuple, device, stream, alloc) -> torch.Tensor:
        """The workspace of ``head`` on ``stream`` (None: the device's current stream; a CPU device has none), made by ``alloc()`` on
        a miss.  While capturing, the capturing stream's own workspace is taken if it has one, otherwise the one of the eager warm-up
        (the most recently used with this head on any stream), so graphs captured on one stream share a workspace and graphs captured
        on streams that were each warmed up have one each."""
        on_gpu = (device if isinstance(device, torch.device) else torch.device(device)).type == "cuda"
        if on_gpu and stream is None:
            stream = torch.cuda.current_stream(device)
        key = head + (None if stream is None else stream.cuda_stream,)
        with self._lock:
            ws = self.entries.pop(key, None)
            if ws is None and on_gpu and torch.cuda.is_current_stream_capturing():
                same = [k for k in self.entries if k[:-1] == head]
                if same:
                    key = same[-1]
                    ws = self.entries.pop(key)
            if ws is None:
                evictable = [k for k in self.entries if k not in self.pinned]
                while len(self.entries) >= owner.WORKSPACE_CACHE and evictable:
                    # (an evicted workspace goes back to the caching allocator's pool of the stream it was made on: the next block
                    # handed out there is ordered behind the calls still reading it)
                    del self.entries[evictable.pop(0)]
                ws = alloc()
            self.entries[key] = ws  # (re-)inserted last = most recently used
            n_pinned = 0
            if ws.is_cuda and torch.cuda.is_current_stream_capturing():
                self.pinned.add(key)
                n_pinned = len(self.pinned)
        if n_pinned and n_pinned > owner.WORKSPACE_CACHE:
            warnings.warn(f"{type(owner).__name__}: {n_pinned} workspaces are pinned by captured graphs (more than "
                          f"WORKSPACE_CACHE = {owner.WORKSPACE_CACHE}); call release_pinned() for shapes whose graphs are gone",
                          RuntimeWarning, stacklevel=4)
        return ws

    def release_pinned(self, match) -> int:
        """Un-pin and drop the pinned workspaces whose key ``match`` accepts; returns how many.  A pin is keyed by shape, not by
        graph, and nobody here can see a hipGraph die: call this once the graphs that replay into those workspaces have been destroyed
        (replaying one afterwards would write into freed memory)."""
        with self._lock:
            keys = [k for k in self.pinned if match(k)]
            for k in keys:
                self.pinned.discard(k)
                self.entries.pop(k, None)
        return len(keys)
