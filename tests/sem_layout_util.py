"""Shared by tests/test_sem_layout_host.py and tests/golden/make_sem_train_layout.py: what the library answers, without a GPU, about
the training of the semantic head -- the six byte-count queries over the training cases and the slab edges,
and code and text of every refusal of the training entry points, each called with every pointer it does not need NULL, so that no
call reaches HIP.  Where two refusals apply to one call the record is the one that wins."""
import ctypes as C
import os
import re

import sem_train_util as SU
import vq_train_util as VU
from edge_diffusion_tts_amd import native

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sem_train_layout.json")
# beside each case's own (B, T): no frames, one frame, M = 256 / 257 (one slab / two slabs of edtts_train_dw_slab_rows) and 32 slabs
EXTRA_SHAPES = ((0, 5), (1, 1), (1, 256), (1, 257), (16, 1500))
FAKE = 0x1000  # a non-NULL pointer for an argument whose refusal comes before anything looks at it


def heads():
    """{case name: (dims, B, T, vq)} of H1-H5 and V1-V5."""
    out = {}
    for name, (in_dim, S, levels, _, B, T) in SU.CASES.items():
        out[name] = (native.sem_dims(in_dim, S, levels), B, T, False)
    for name, (in_dim, S, K, _, B, T) in VU.CASES.items():
        out[name] = (native.sem_dims(in_dim, S, None, K), B, T, True)
    return out


def layout_records():
    """{"<case> B x T": {"blob", "tape", "scratch"}} through the six byte-count queries."""
    rec = {}
    for name, (dims, B, T, vq) in sorted(heads().items()):
        blob, tape, scratch = ((native.sem_vq_train_packed_bytes, native.sem_vq_tape_bytes, native.sem_vq_scratch_bytes) if vq else
                               (native.sem_train_packed_bytes, native.sem_train_tape_bytes, native.sem_train_scratch_bytes))
        for b, t in ((B, T),) + EXTRA_SHAPES:
            rec[f"{name} {b}x{t}"] = {"blob": blob(dims), "tape": tape(dims, b, t), "scratch": scratch(dims, b, t)}
    return rec


def outcome(fn, *args, **kw):
    """[code, text] of one call of an export: [0, ""] when it returns EDTTS_OK."""
    try:
        fn(*args, **kw)
    except native.EdttsError as e:
        m = re.match(r"^\w+ failed \(code (-?\d+)\): (.*)$", str(e), flags=re.S)
        return [int(m.group(1)), m.group(2)]
    return [0, ""]


def refusal_records():
    """{label: [code, text]} of the refusals of the training entry points of both quantizers."""
    L = native.lib()
    d = {"fsq": native.sem_dims(64, 32, [3, 3]), "fsq0": native.sem_dims(0, 32, [3, 3]), "vq": native.sem_dims(64, 32, None, 128),
         "vq0": native.sem_dims(0, 32, None, 128)}
    out_bytes = C.c_size_t(0)
    ob = C.byref(out_bytes)

    def drop(p, dev=False):  # (a _dev twin: the key lies in device memory; no refusal reads it)
        return None if p is None else C.byref(native.EdttsDropoutDev(p, FAKE) if dev else native.EdttsDropout(p, 1))

    # every entry point as f(dims, **what the refusals vary), all other arguments NULL
    def q(name, shaped):
        fn = getattr(L, name)
        return (lambda dims, B=1, T=1, out=ob: fn(C.byref(dims), B, T, out)) if shaped else (lambda dims, out=ob, **_: fn(C.byref(dims), out))

    def pack(name):
        fn = getattr(L, name)
        return lambda dims, slots=None, n=0, dst=None, **_: fn(C.byref(dims), slots, n, dst, None)

    def enc(name):
        fn = getattr(L, name)
        return lambda dims, B=1, T=1, p=None, ptr=None, **_: fn(C.byref(dims), ptr, ptr, B, T, None, ptr, ptr, None, ptr, drop(p, name.endswith("_dev")), None)

    def bwd(name):
        fn = getattr(L, name)
        return lambda dims, B=1, T=1, n=10, d_z=None, p=None, **_: fn(C.byref(dims), None, None, None, None, B, T, None, None, None, n, d_z, None,
                                                                   drop(p, name.endswith("_dev")), None)

    def mask(name):
        fn = getattr(L, name)
        return lambda dims, B=1, T=1, p=0.5, **_: fn(C.byref(dims), B, T, drop(p, name.endswith("_dev")), None, None)

    def vq_enc(dims, B=1, T=1, p=None, commit=0.25, **_):
        return L.edtts_sem_vq_encode_train(C.byref(dims), None, None, B, T, None, None, None, None, None, None, 1, commit, drop(p), None)

    def vq_ema(dims, B=1, T=1, decay=0.99, eps=1e-5, **_):
        return L.edtts_sem_vq_ema_update(C.byref(dims), None, None, B, T, None, None, decay, eps, None, None, None, None, None)

    def vq_bwd(dims, B=1, T=1, n=7, d_z=None, p=None, commit=0.25, **_):
        return L.edtts_sem_vq_backward(C.byref(dims), None, None, None, None, None, B, T, None, None, None, commit, None, n, d_z, None, drop(p), None)

    fsq_calls = {"edtts_sem_train_packed_bytes": q("edtts_sem_train_packed_bytes", False), "edtts_sem_train_pack": pack("edtts_sem_train_pack"),
                 "edtts_sem_train_tape_bytes": q("edtts_sem_train_tape_bytes", True),
                 "edtts_sem_train_scratch_bytes": q("edtts_sem_train_scratch_bytes", True),
                 "edtts_sem_encode_train": enc("edtts_sem_encode_train"), "edtts_sem_encode_train_dev": enc("edtts_sem_encode_train_dev"),
                 "edtts_sem_backward": bwd("edtts_sem_backward"), "edtts_sem_backward_dev": bwd("edtts_sem_backward_dev"),
                 "edtts_sem_dropout_mask": mask("edtts_sem_dropout_mask"), "edtts_sem_dropout_mask_dev": mask("edtts_sem_dropout_mask_dev")}
    vq_calls = {"edtts_sem_vq_train_packed_bytes": q("edtts_sem_vq_train_packed_bytes", False),
                "edtts_sem_vq_train_pack": pack("edtts_sem_vq_train_pack"), "edtts_sem_vq_tape_bytes": q("edtts_sem_vq_tape_bytes", True),
                "edtts_sem_vq_scratch_bytes": q("edtts_sem_vq_scratch_bytes", True), "edtts_sem_vq_encode_train": vq_enc,
                "edtts_sem_vq_ema_update": vq_ema, "edtts_sem_vq_backward": vq_bwd}
    dropping = {n for n in list(fsq_calls) + list(vq_calls) if "encode_train" in n or "backward" in n or "dropout_mask" in n}
    rec = {}

    def note(label, fn, dims, **kw):
        assert label not in rec, label
        rec[label] = outcome(fn, d[dims], **kw)

    for family, calls, proj, alone, other in (("fsq", fsq_calls, "fsq", "fsq0", "vq"), ("vq", vq_calls, "vq", "vq0", "fsq")):
        slots_of = lambda n: (C.c_void_p * n)(*([FAKE] * n))  # noqa: E731
        want = {proj: 10 if family == "fsq" else 7, alone: 4 if family == "fsq" else 1}
        for name, fn in calls.items():
            note(f"{name}: the other quantizer's dims", fn, other)
            if name.endswith("_bytes"):
                note(f"{name}: NULL out_bytes", fn, proj, out=None)
                note(f"{name}: the other quantizer's dims and NULL out_bytes", fn, other, out=None)
                if "packed" not in name:
                    note(f"{name}: NULL out_bytes and B < 0", fn, proj, out=None, B=-1)
            if name.endswith("_pack"):
                for dims in (proj, alone):
                    n = want[dims]
                    note(f"{name} {dims}: wrong n_slots", fn, dims, slots=slots_of(n + 1), n=n + 1, dst=FAKE)
                    note(f"{name} {dims}: wrong n_slots and NULL slots", fn, dims, n=n + 1)
                    note(f"{name} {dims}: NULL slots", fn, dims, n=n, dst=FAKE)
                    note(f"{name} {dims}: NULL packed_train", fn, dims, slots=slots_of(n), n=n)
                    for i in sorted({0, n - 1}):
                        s = slots_of(n)
                        s[i] = None
                        note(f"{name} {dims}: NULL slot {i}", fn, dims, slots=s, n=n, dst=FAKE)
            if "bytes" in name and "packed" in name or name.endswith("_pack"):
                continue
            for B, T in ((-1, 1), (1, -1), (1 << 16, 1 << 16)):
                note(f"{name}: B={B} T={T}", fn, proj, B=B, T=T)
            if name.endswith("_bytes"):
                continue
            note(f"{name}: NULL pointers", fn, proj)
            note(f"{name} {alone}: NULL pointers", fn, alone, n=want[alone])
            if name in dropping:
                for p in (1.0, -0.1, 0.999995):
                    note(f"{name}: dropout p={p}", fn, proj, p=p)
                note(f"{name}: dropout on a head without proj", fn, alone, p=0.5, n=want[alone])
                note(f"{name}: dropout p=1.0 and B < 0", fn, proj, p=1.0, B=-1)
            if "dropout_mask" in name:
                note(f"{name}: NULL drop", fn, proj, p=None)
                note(f"{name}: p = 0 and NULL keep", fn, proj, p=0.0)
            if "backward" in name:
                note(f"{name}: wrong n_slots", fn, proj, n=want[proj] - 1)
                note(f"{name} {alone}: wrong n_slots", fn, alone, n=want[proj])
                note(f"{name}: d_z with a proj", fn, proj, n=want[proj], d_z=FAKE)
                note(f"{name}: wrong n_slots and d_z with a proj", fn, proj, n=1, d_z=FAKE)
                note(f"{name}: B < 0 and wrong n_slots", fn, proj, B=-1, n=1)
            if name in ("edtts_sem_vq_encode_train", "edtts_sem_vq_backward"):
                for commit in (-1.0, float("nan"), 2e6):
                    note(f"{name}: commit={commit}", fn, proj, commit=commit)
                note(f"{name}: commit=-1.0 and dropout p=1.0", fn, proj, commit=-1.0, p=1.0)
            if name == "edtts_sem_vq_ema_update":
                for decay in (0.0, 1.5, float("nan")):
                    note(f"{name}: decay={decay}", fn, proj, decay=decay)
                for eps in (-1.0, float("nan")):
                    note(f"{name}: epsilon={eps}", fn, proj, eps=eps)
                note(f"{name}: decay=0.0 and B < 0", fn, proj, decay=0.0, B=-1)
    return rec


def records():
    return {"layouts": layout_records(), "refusals": refusal_records()}
