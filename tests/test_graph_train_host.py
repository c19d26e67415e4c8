"""The host side of the captured training step, without a GPU: the key function against the numpy Philox of
tests/dropout_util.py, the cosine schedule against train_v2.cosine_lr_schedule's text, the new structs, and argument errors of the new
exports (reported before any pointer is looked at)."""
import ctypes
import math

import pytest
import torch

import dropout_util as U
from edge_diffusion_tts_amd import FusedAdamW, GraphedTrainStep, KeyStream, native, optim

BASES = (0, 7, 0x0123456789ABCDEF, 0xFFFFFFFFFFFFFFFF)
COUNTERS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63)
SLOTS = (0, 70000)


def numpy_key(base, c, i):
    """K(base, c, i) from the contract's text: words 0 and 1 of philox4x32_10(key = base, counter = (i, c lo, 0x50000, c hi)), bit 63
    cleared."""
    w = U.philox4x32_10((base & 0xFFFFFFFF, base >> 32), (i, c & 0xFFFFFFFF, 0x50000, c >> 32))
    return (int(w[0]) | (int(w[1]) << 32)) & (2 ** 63 - 1)


@pytest.mark.parametrize("base", BASES)
def test_keys_host_is_the_numpy_philox_composition(base):
    for c in COUNTERS:
        for first in SLOTS:
            got = native.keys_host(base, c, first, 3)
            assert got == [numpy_key(base, c, first + j) for j in range(3)], (base, c, first)
            assert all(k < 2 ** 63 for k in got)  # bit 63 is clear: a legal int64 seed
    assert native.keys_host(base, 5, 0, 0) == []
    # a key depends on the counter and on the slot
    assert len({native.keys_host(base, c, 0, 1)[0] for c in COUNTERS}) == len(COUNTERS)
    assert len(set(native.keys_host(base, 0, 0, 300))) == 300


def test_the_key_stream_word_is_its_own():
    """0x50000 lies outside every other generator's range (include/edtts.h, "Philox stream ids")."""
    assert native.KEY_STREAM == 0x50000
    assert native.KEY_STREAM not in (native.OBJ_NOISE_STREAM, native.SEM_DROP_STREAM)
    assert native.KEY_STREAM >= 0x30000 + 4 * 33 and native.KEY_STREAM > native.SEM_DROP_STREAM


def reference_cosine(step, total_steps, warmup_steps, base_lr, min_lr=1e-6):
    """train_v2.cosine_lr_schedule, lines 86-90, as the reference writes them."""
    if step < warmup_steps:
        lr = base_lr * step / max(warmup_steps, 1)
    else:
        progress = (step - warmup_steps) / max(total_steps - warmup_steps, 1)
        lr = min_lr + 0.5 * (base_lr - min_lr) * (1 + math.cos(math.pi * progress))
    return lr


@pytest.mark.parametrize("total,warmup,base,low", [(100, 10, 3e-4, 1e-6), (7, 0, 1e-3, 0.0), (5, 5, 2e-4, 1e-5), (1000, 1, 1.0, 0.5)])
def test_cosine_lr_is_the_reference_formula(total, warmup, base, low):
    for n in (0, 1, warmup - 1, warmup, (warmup + total) // 2, total, total + 5):
        if n < 0:
            continue
        assert optim.cosine_lr(n, total, warmup, base, low) == reference_cosine(n, total, warmup, base, low), n
    assert optim.cosine_lr(0, total, warmup, base, low) == (0.0 if warmup else base)
    if total > warmup:
        assert abs(optim.cosine_lr(total, total, warmup, base, low) - low) <= 1e-15 * max(base, 1e-30) + 1e-18


def test_new_structs_have_the_layout_of_the_header():
    assert ctypes.sizeof(native.EdttsDropoutDev) == 16 and native.EdttsDropoutDev.key.offset == 8
    assert ctypes.sizeof(native.EdttsOptimSchedule) == 40
    assert [native.EdttsOptimSchedule.base_lr.offset, native.EdttsOptimSchedule.min_lr.offset, native.EdttsOptimSchedule.warmup_steps.offset,
            native.EdttsOptimSchedule.total_steps.offset] == [8, 16, 24, 32]
    assert native.lib().edtts_version() == 400  # additive: the ABI version stays


def test_argument_errors_are_reported_as_errors():
    L = native.lib()
    out = (ctypes.c_uint64 * 4)()
    with pytest.raises(native.EdttsError, match="edtts_keys_host"):
        L.edtts_keys_host(1, 0, -1, 1, out)
    with pytest.raises(native.EdttsError, match="edtts_keys_host"):
        L.edtts_keys_host(1, 0, 2 ** 32 - 1, 2, out)
    with pytest.raises(native.EdttsError, match="edtts_keys_host"):
        L.edtts_keys_host(1, 0, 0, 2, None)
    with pytest.raises(native.EdttsError, match="edtts_keys_advance"):
        L.edtts_keys_advance(None, 3, None, None)
    with pytest.raises(native.EdttsError, match="edtts_keys_advance.*aligned"):
        L.edtts_keys_advance(4, 1, 8, None)
    with pytest.raises(native.EdttsError, match="EDTTS_OPT_EMA_ONLY has no resident form"):
        L.edtts_optim_step_resident(1, 1, 0.0, native.OPT_EMA_ONLY, 16, 4096, None, None, None)
    with pytest.raises(native.EdttsError, match="n_groups=0"):
        L.edtts_optim_step_resident(1, 0, 0.0, 0, 16, 4096, None, None, None)
    with pytest.raises(native.EdttsError, match="max_norm"):
        L.edtts_optim_step_resident(1, 1, -1.0, native.OPT_CLIP, 16, 4096, None, None, None)
    bad = native.EdttsOptimSchedule(7, 0, 1e-3, 0.0, 0, 10)
    with pytest.raises(native.EdttsError, match="schedule kind 7"):
        L.edtts_optim_step_resident(1, 1, 0.0, 0, 16, 4096, None, ctypes.byref(bad), None)
    neg = native.EdttsOptimSchedule(native.EDTTS_SCHED_COSINE, 0, -1.0, 0.0, 0, 10)
    with pytest.raises(native.EdttsError, match="cosine schedule"):
        L.edtts_optim_step_resident(1, 1, 0.0, 0, 16, 4096, None, ctypes.byref(neg), None)
    with pytest.raises(native.EdttsError, match="need 384 bytes of scratch, got 8"):
        L.edtts_optim_step_resident(3, 1, 0.0, 0, 16, 8, None, None, None)
    with pytest.raises(native.EdttsError, match="edtts_optim_upload"):
        L.edtts_optim_upload(None, 1, None, 1, 0, None, 0, None, None, None)
    # the *_dev twins: a NULL or misaligned key is an argument error before anything else is looked at
    dims = native.EdttsDims(64, 2, 2, 16, 2, 16, 8, -1, 64, 64, 16, native.KERNELS["generic"])
    for key, what in ((None, "key is NULL"), (12, "8-byte aligned")):
        drop = native.EdttsDropoutDev(0.2, key)
        with pytest.raises(native.EdttsError, match=what):
            L.edtts_dropout_mask_dev(ctypes.byref(dims), 0, 0, 1, 4, 4, ctypes.byref(drop), None, None)
        with pytest.raises(native.EdttsError, match=what):
            L.edtts_decoder_forward_train_dev(ctypes.byref(dims), None, None, None, 1, 4, 4, None, None, None, None, None, None,
                                              ctypes.byref(drop), None, None, None)
    sd = native.sem_dims(48, 16, [8, 6, 5, 5, 5])
    drop = native.EdttsDropoutDev(0.2, None)
    with pytest.raises(native.EdttsError, match="key is NULL"):
        L.edtts_sem_dropout_mask_dev(ctypes.byref(sd), 1, 5, ctypes.byref(drop), None, None)


def test_python_argument_errors():
    with pytest.raises(ValueError, match="schedule kind"):
        native.optim_schedule("linear", 1e-3, 0.0, 0, 10)
    with pytest.raises(ValueError, match="schedule:"):
        native.optim_schedule("cosine", -1e-3, 0.0, 0, 10)
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="capturable=True"):
        FusedAdamW([p]).device_lr_schedule("cosine", 1e-3)
    with pytest.raises(ValueError, match="tensor lr needs capturable=True"):
        FusedAdamW([p], lr=torch.tensor(1e-3, dtype=torch.float64))
    with pytest.raises(ValueError, match="capturable=True, zero_grads=True"):
        GraphedTrainStep(lambda: None, FusedAdamW([p]), [])
    with pytest.raises(ValueError, match="capturable=True, zero_grads=True"):
        GraphedTrainStep(lambda: None, FusedAdamW([p], capturable=True), [])
    with pytest.raises(native.EdttsError, match="no CPU fallback"):
        KeyStream(1, 2, device="cpu")
    with pytest.raises(native.EdttsError, match="DropKey"):
        native.DropKey(0.2, torch.zeros(1, dtype=torch.int64))
