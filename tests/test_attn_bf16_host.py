"""bf16 attention, host side: the ``attn_dtype`` keyword and its validation, the EDTTS_ATTN_BF16 bit of
EdttsDims.compute_dtype and what the library answers with it, and the CPU yardsticks of tests/attn_bf16_util.py -- the model of the
rounding contract must itself meet every bar the GPU tests hold the kernels to, alone and stacked with the bf16 linears.  No GPU needed."""
import os
import re

import pytest
import torch

import attn_bf16_util as AU
import train_bf16_util as U
from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, native
from train_util import CASES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIT, MM = native.EDTTS_ATTN_BF16, native.EDTTS_MATMUL_BF16
GRAD_CASES = [(n, False) for n in CASES] + [("G4", True), ("A1", False), ("A2", False)]


def dec(attn_dtype="bf16", kernels="generic", name=None, **kw):
    cfg = CFG(device="cpu", **(CASES[name][0] if name else {}))
    return EdgeDiffusionDecoder(cfg, kernels=kernels, attn_dtype=attn_dtype, **kw)


# ---------------------------------------------------------------------------------------------- the keyword
def test_attn_dtype_is_validated():
    assert EdgeDiffusionDecoder(CFG(device="cpu")).attn_dtype == "f32"
    assert native.ATTN_DTYPES["f32"] == 0 and native.ATTN_DTYPES["bf16"] == BIT
    assert set(native.ATTN_DTYPES) == set(native.MATMUL_DTYPES)  # spelled alike
    for good in native.ATTN_DTYPES:
        assert dec(good).attn_dtype == good
    with pytest.raises(ValueError, match="attn_dtype must be one of"):
        dec("fp16")
    with pytest.raises(ValueError, match="attn_dtype must be one of"):
        dec(None)


@pytest.mark.parametrize("kernels", ["compiled", "auto"])
def test_bf16_attention_needs_the_generic_kernels(kernels):
    with pytest.raises(ValueError, match="attn_dtype='bf16' needs kernels='generic'"):
        dec("bf16", kernels)
    assert dec("f32", kernels).dims().compute_dtype == native.KERNELS[kernels]


def test_dims_carry_the_bit_in_all_four_combinations():
    assert BIT == 0x800 and BIT > max(native.KERNELS.values()) and not BIT & (0x300 | 1 | MM)
    for md, ad, want in (("f32", "f32", 0x100), ("bf16", "f32", 0x100 | MM), ("f32", "bf16", 0x100 | BIT), ("bf16", "bf16", 0x100 | MM | BIT)):
        assert dec(ad, matmul_dtype=md).dims().compute_dtype == want
    assert dec(autograd=True, train_dropout=True, train_lengths=True).dims().compute_dtype == 0x100 | BIT
    assert EdgeDiffusionDecoder(CFG(device="cpu")).dims().compute_dtype == 0  # the default decoder's dims are unchanged


def test_header_constant_is_the_python_one():
    with open(os.path.join(REPO, "include", "edtts.h")) as f:
        m = re.search(r"\benum\s*\{\s*EDTTS_ATTN_BF16\s*=\s*(\w+)\s*\}", f.read())
    assert m and int(m.group(1), 0) == BIT


# ---------------------------------------------------------------------------------------------- the library
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("matmul_dtype", ["f32", "bf16"])
def test_sizes_and_slots_are_the_fp32_generic_decoders(name, matmul_dtype):
    _, B, T, S, _, _ = CASES[name]
    a = dec("bf16", name=name, autograd=True, matmul_dtype=matmul_dtype).dims()
    b = dec("f32", name=name, autograd=True).dims()
    assert a.compute_dtype == b.compute_dtype | BIT | native.MATMUL_DTYPES[matmul_dtype]
    for q in (native.packed_bytes, lambda d: native.workspace_bytes(d, B, T, S, B), lambda d: native.workspace_bytes(d, B, T, S, 3),
              lambda d: native.train_tape_bytes(d, B, T, S), lambda d: native.train_scratch_bytes(d, B, T, S)):
        assert q(a) == q(b) > 0
    n_slots = len(native.slot_names(a.layers))
    assert [native.generic_slot_dest(a, i) for i in range(n_slots)] == [native.generic_slot_dest(b, i) for i in range(n_slots)]
    assert native.substreams_for(a, B, T) == 1


def test_blob_mirror_is_the_fp32_generic_decoders():
    assert dec("bf16", autograd=True)._mirror_map() == dec("f32", autograd=True)._mirror_map() != None  # noqa: E711
    assert dec("bf16", autograd=True, matmul_dtype="bf16")._mirror_map() == dec("f32", autograd=True)._mirror_map()


@pytest.mark.parametrize("extra", [0, MM], ids=["alone", "with EDTTS_MATMUL_BF16"])
@pytest.mark.parametrize("bits, why", [
    (0, "EDTTS_F32 alone"),
    (1, "EDTTS_BF16"),
    (1 | 0x100, "EDTTS_BF16 | EDTTS_KERNELS_GENERIC"),
    (0x200, "EDTTS_KERNELS_AUTO at a compiled shape"),
    (0x300, "both kernel bits"),
])
def test_library_refuses_the_bit_elsewhere(bits, why, extra):
    d = EdgeDiffusionDecoder(CFG(device="cpu")).dims()  # 160/4/80: a compiled instance
    d.compute_dtype = bits | BIT | extra
    for query in (native.packed_bytes, lambda x: native.workspace_bytes(x, 2, 32, 16, 2), lambda x: native.train_tape_bytes(x, 2, 32, 16),
                  lambda x: native.train_scratch_bytes(x, 2, 32, 16), lambda x: native.generic_slot_dest(x, 0)):
        with pytest.raises(native.EdttsError, match=r"code -1\).*EDTTS_ATTN_BF16"):  # EDTTS_ERR_UNSUPPORTED, naming the bit
            query(d)
    d.compute_dtype = 0x200 | BIT | extra
    d.hidden, d.heads = 224, 7  # AUTO would resolve to the generic kernels here: still not the legal spelling
    with pytest.raises(native.EdttsError, match=r"code -1\).*EDTTS_ATTN_BF16"):
        native.packed_bytes(d)


def test_the_legal_spellings_are_accepted():
    d = EdgeDiffusionDecoder(CFG(device="cpu")).dims()
    for bits in (0x100 | BIT, 0x100 | BIT | MM):
        d.compute_dtype = bits
        assert native.packed_bytes(d) > 0 and native.train_tape_bytes(d, 2, 32, 16) > 0


# ---------------------------------------------------------------------------------------------- the model is the contract
def _hand(with_mult):
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(s, generator=g, requires_grad=True) for s in ((2, 3, 5, 8), (2, 3, 7, 8), (2, 3, 7, 8)))
    mask = torch.rand(5, 7, generator=g) > 0.3
    mask[:, 0] = True  # no empty row
    mult = ((torch.rand(2, 3, 5, 7, generator=g) > 0.2).float() * 1.25) if with_mult else None
    return q, k, v, mask, mult, torch.randn(2, 3, 5, 8, generator=g)


@pytest.mark.parametrize("with_mult", [False, True], ids=["plain", "dropout"])
def test_model_attention_rounds_what_the_contract_names(with_mult):
    q, k, v, mask, mult, do = _hand(with_mult)
    o = AU.model_attention(q, k, v, mask, mult)
    rb = lambda t: t.detach().bfloat16().float()
    D = 1.0 if mult is None else mult
    s = ((rb(q) @ rb(k).transpose(-1, -2)) * 8 ** -0.5).masked_fill(~mask, float("-inf"))
    pt = torch.exp(s - s.amax(-1, keepdim=True))
    l = pt.sum(-1, keepdim=True)
    want = (rb(pt * D) @ rb(v)) / l
    assert o.dtype == torch.float32 and torch.equal(o.detach(), want)
    o.backward(do)
    p = pt / l
    delta = (do * want).sum(-1, keepdim=True)
    dp = rb(do) @ rb(v).transpose(-1, -2)
    ds = p * (dp * D - delta)
    assert torch.equal(v.grad, rb(p * D).transpose(-1, -2) @ rb(do))
    assert torch.equal(q.grad, (rb(ds) @ rb(k)) * 8 ** -0.5)
    assert torch.equal(k.grad, (rb(ds).transpose(-1, -2) @ rb(q)) * 8 ** -0.5)
    # ... and nothing else: it is not the unrounded attention, and the softmax statistics are not those of rounded probabilities
    plain = (torch.softmax(((q.detach() @ k.detach().transpose(-1, -2)) * 8 ** -0.5).masked_fill(~mask, float("-inf")), -1) * D) @ v.detach()
    assert not torch.equal(o.detach(), plain)
    assert not torch.equal(o.detach(), (rb(pt * D) @ rb(v)) / rb(pt).sum(-1, keepdim=True))
    torch.testing.assert_close(o.detach(), plain, rtol=0, atol=0.05)


def test_model_patches_both_oracles_and_stacks():
    from oracle import edtts_oracle as O
    import dropout_util
    before = (O.attention, dropout_util._attention, O.linear)
    with AU.model("attn"):
        assert O.attention is AU.model_attention and dropout_util._attention is AU.model_attention and O.linear is before[2]
    with AU.model("both"):
        assert O.attention is AU.model_attention and O.linear is U.model_linear
    assert (O.attention, dropout_util._attention, O.linear) == before


# ---------------------------------------------------------------------------------------------- the model meets its own bars
@pytest.mark.parametrize("variant", AU.VARIANTS)
@pytest.mark.parametrize("name, two", GRAD_CASES)
def test_model_meets_the_gradient_bars(name, two, variant):
    y = AU.grad_yardsticks(name, two, variant)
    assert 1e-4 < y["med_a"] < 5e-2  # autocast's own level: fp32's is about 3e-7
    U.check_grads(y["g_m"], y, f"model[{variant}] {name}{' two forwards' if two else ''}")


@pytest.mark.parametrize("variant", AU.VARIANTS)
def test_model_meets_the_gradient_bars_ragged_and_with_dropout(variant):
    U.check_grads(AU.ragged_yardsticks(variant)["g_m"], AU.ragged_yardsticks(variant), f"model[{variant}] {U.RAGGED_CASE}")
    U.check_grads(AU.dropout_yardsticks(variant)["g_m"], AU.dropout_yardsticks(variant), f"model[{variant}] {U.DROP_CASE} dropout")


@pytest.mark.parametrize("variant", AU.VARIANTS)
@pytest.mark.parametrize("name", list(CASES) + ["A1", "A2"])
def test_model_meets_the_forward_bars(name, variant):
    y = AU.forward_yardsticks(name, variant)
    U.check_output(y["out_m"], y, f"model[{variant}] {name} eps")


@pytest.mark.parametrize("variant", AU.VARIANTS)
@pytest.mark.parametrize("name", ["G2", "G4"])
def test_model_meets_the_sampler_bars(name, variant):
    y = AU.sampler_yardsticks(name, variant)
    U.check_output(y["out_m"], y, f"model[{variant}] {name} DPM-Solver++ order 2, {U.SAMPLER_STEPS} steps")
