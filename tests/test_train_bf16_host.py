"""bf16-matmul training, host side: the ``matmul_dtype`` keyword and its validation, the EDTTS_MATMUL_BF16 bit
of EdttsDims.compute_dtype and what the library answers with it, and the CPU yardsticks of tests/train_bf16_util.py -- the model of
the feature's arithmetic must itself meet every bar the GPU tests hold the kernels to, so that a drift of the yardstick code which
made the bars unreachable or vacuous shows on the CPU.  No GPU needed."""
import os
import re

import pytest
import torch

import train_bf16_util as U
from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, native
from train_util import CASES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIT = native.EDTTS_MATMUL_BF16


def dec(matmul_dtype="bf16", kernels="generic", name=None, **kw):
    cfg = CFG(device="cpu", **(CASES[name][0] if name else {}))
    return EdgeDiffusionDecoder(cfg, kernels=kernels, matmul_dtype=matmul_dtype, **kw)


# ---------------------------------------------------------------------------------------------- the keyword
def test_matmul_dtype_is_validated():
    assert EdgeDiffusionDecoder(CFG(device="cpu")).matmul_dtype == "f32"
    assert native.MATMUL_DTYPES["f32"] == 0 and native.MATMUL_DTYPES["bf16"] == BIT
    for good in native.MATMUL_DTYPES:
        assert dec(good).matmul_dtype == good
    with pytest.raises(ValueError, match="matmul_dtype must be one of"):
        dec("fp16")
    with pytest.raises(ValueError, match="matmul_dtype must be one of"):
        dec(None)


@pytest.mark.parametrize("kernels", ["compiled", "auto"])
def test_bf16_matmuls_need_the_generic_kernels(kernels):
    with pytest.raises(ValueError, match="matmul_dtype='bf16' needs kernels='generic'"):
        dec("bf16", kernels)
    assert dec("f32", kernels).dims().compute_dtype == native.KERNELS[kernels]


def test_storage_spelling_keeps_raising():
    """compute_dtype describes storage, and storage stays fp32: the spelling tests/test_generic_host.py pins is not the new option."""
    with pytest.raises(ValueError, match="fp32 only"):
        EdgeDiffusionDecoder(CFG(device="cpu", hidden=256, heads=8), compute_dtype="bf16", kernels="generic", matmul_dtype="bf16")


def test_dims_carry_the_bit():
    assert BIT == 0x400 and BIT > max(native.KERNELS.values()) and not BIT & (0x300 | 1)
    assert dec().dims().compute_dtype == 0x100 | BIT
    assert dec(autograd=True, train_dropout=True, train_lengths=True).dims().compute_dtype == 0x100 | BIT
    assert dec("f32").dims().compute_dtype == 0x100
    assert EdgeDiffusionDecoder(CFG(device="cpu")).dims().compute_dtype == 0  # the default decoder's dims are unchanged
    assert native.COMPUTE_DTYPES == {"f32": 0, "fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1}
    assert native.KERNELS == {"compiled": 0, "generic": 0x100, "auto": 0x200}


def test_header_constant_is_the_python_one():
    with open(os.path.join(REPO, "include", "edtts.h")) as f:
        m = re.search(r"\benum\s*\{\s*EDTTS_MATMUL_BF16\s*=\s*(\w+)\s*\}", f.read())
    assert m and int(m.group(1), 0) == BIT


# ---------------------------------------------------------------------------------------------- the library
@pytest.mark.parametrize("name", list(CASES))
def test_sizes_and_slots_are_the_fp32_generic_decoders(name):
    _, B, T, S, _, _ = CASES[name]
    a, b = dec("bf16", name=name, autograd=True).dims(), dec("f32", name=name, autograd=True).dims()
    assert a.compute_dtype == b.compute_dtype | BIT
    for q in (native.packed_bytes, lambda d: native.workspace_bytes(d, B, T, S, B), lambda d: native.workspace_bytes(d, B, T, S, 3),
              lambda d: native.train_tape_bytes(d, B, T, S), lambda d: native.train_scratch_bytes(d, B, T, S)):
        assert q(a) == q(b) > 0
    n_slots = len(native.slot_names(a.layers))
    assert [native.generic_slot_dest(a, i) for i in range(n_slots)] == [native.generic_slot_dest(b, i) for i in range(n_slots)]
    assert native.substreams_for(a, B, T) == 1


def test_blob_mirror_is_the_fp32_generic_decoders():
    assert dec("bf16", autograd=True)._mirror_map() == dec("f32", autograd=True)._mirror_map() != None  # noqa: E711


@pytest.mark.parametrize("bits, why", [
    (0, "EDTTS_F32 alone"),
    (1, "EDTTS_BF16"),
    (1 | 0x100, "EDTTS_BF16 | EDTTS_KERNELS_GENERIC"),
    (0x200, "EDTTS_KERNELS_AUTO at a compiled shape"),
    (0x300, "both kernel bits"),
])
def test_library_refuses_the_bit_elsewhere(bits, why):
    d = EdgeDiffusionDecoder(CFG(device="cpu")).dims()  # 160/4/80: a compiled instance
    d.compute_dtype = bits | BIT
    for query in (native.packed_bytes, lambda x: native.workspace_bytes(x, 2, 32, 16, 2), lambda x: native.train_tape_bytes(x, 2, 32, 16),
                  lambda x: native.train_scratch_bytes(x, 2, 32, 16), lambda x: native.generic_slot_dest(x, 0)):
        with pytest.raises(native.EdttsError, match=r"code -1\).*EDTTS_MATMUL_BF16"):  # EDTTS_ERR_UNSUPPORTED, naming the bit
            query(d)
    d.compute_dtype = 0x200 | BIT
    d.hidden, d.heads = 224, 7  # AUTO would resolve to the generic kernels here: still not the legal spelling
    with pytest.raises(native.EdttsError, match=r"code -1\).*EDTTS_MATMUL_BF16"):
        native.packed_bytes(d)


def test_without_the_bit_the_old_refusals_stand():
    d = EdgeDiffusionDecoder(CFG(device="cpu")).dims()
    d.compute_dtype = 1 | 0x100
    with pytest.raises(native.EdttsError, match="fp32 only"):
        native.packed_bytes(d)
    d.compute_dtype = 0x200
    with pytest.raises(native.EdttsError, match="generic kernels only"):
        native.train_tape_bytes(d, 2, 32, 16)


# ---------------------------------------------------------------------------------------------- the model meets its own bars
def test_model_linear_rounds_operands_only():
    g = torch.Generator().manual_seed(0)
    x, w, b = (torch.randn(s, generator=g, requires_grad=True) for s in ((3, 5, 7), (4, 7), (4,)))
    y = U.model_linear(x, w, b)
    rb = lambda v: v.detach().bfloat16().float()
    assert torch.equal(y.detach(), rb(x) @ rb(w).T + b.detach()) and y.dtype == torch.float32
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    assert torch.equal(x.grad, rb(dy) @ rb(w))
    assert torch.equal(w.grad, rb(dy).reshape(-1, 4).T @ rb(x).reshape(-1, 7))
    assert torch.equal(b.grad, dy.reshape(-1, 4).sum(0))  # the bias gradient sums the unrounded dY
    assert not torch.equal(y.detach(), x.detach() @ w.detach().T + b.detach())


@pytest.mark.parametrize("name, two", [(n, False) for n in CASES] + [("G4", True)])
def test_model_meets_the_gradient_bars(name, two):
    y = U.grad_yardsticks(name, two)
    assert 1e-4 < y["med_a"] < 5e-2  # autocast's own level: fp32's is about 3e-7
    U.check_grads(y["g_m"], y, f"model {name}{' two forwards' if two else ''}")


def test_model_meets_the_gradient_bars_ragged_and_with_dropout():
    U.check_grads(U.ragged_yardsticks()["g_m"], U.ragged_yardsticks(), f"model {U.RAGGED_CASE}")
    U.check_grads(U.dropout_yardsticks()["g_m"], U.dropout_yardsticks(), f"model {U.DROP_CASE} dropout")


@pytest.mark.parametrize("name", list(CASES))
def test_model_meets_the_forward_bars(name):
    y = U.forward_yardsticks(name)
    U.check_output(y["out_m"], y, f"model {name} eps")


@pytest.mark.parametrize("name", ["G2", "G4"])
def test_model_meets_the_sampler_bars(name):
    y = U.sampler_yardsticks(name)
    U.check_output(y["out_m"], y, f"model {name} DPM-Solver++ order 2, {U.SAMPLER_STEPS} steps")
