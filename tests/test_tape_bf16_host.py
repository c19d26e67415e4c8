"""bf16 activation storage, host side: the ``tape_dtype`` keyword and its validation, the EDTTS_TAPE_BF16 bit of
EdttsDims.compute_dtype and what the library answers with it (refusals, the tape's size and its regions), and the argument for the
option's bar restated on the CPU: storing bf16(x) where every consumer rounds x to bf16 changes no bit.  No GPU needed."""
import os
import re

import pytest
import torch

import attn_bf16_util as AU
import tape_bf16_util as TU
import train_util
from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, native
from train_util import CASES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIT, MM, ATT, BOTH = native.EDTTS_TAPE_BF16, native.EDTTS_MATMUL_BF16, native.EDTTS_ATTN_BF16, TU.BOTH
GEN = native.KERNELS["generic"]


def dec(tape_dtype="bf16", kernels="generic", matmul_dtype="bf16", attn_dtype="bf16", name=None, **kw):
    cfg = CFG(device="cpu", **((CASES.get(name) or AU.ACASES[name])[0] if name else {}))
    return EdgeDiffusionDecoder(cfg, kernels=kernels, matmul_dtype=matmul_dtype, attn_dtype=attn_dtype, tape_dtype=tape_dtype, **kw)


# ---------------------------------------------------------------------------------------------- the keyword
def test_tape_dtype_is_validated():
    assert EdgeDiffusionDecoder(CFG(device="cpu")).tape_dtype == "f32"
    assert native.TAPE_DTYPES["f32"] == 0 and native.TAPE_DTYPES["bf16"] == BIT
    assert set(native.TAPE_DTYPES) == set(native.MATMUL_DTYPES) == set(native.ATTN_DTYPES)  # spelled alike
    for good in native.TAPE_DTYPES:
        assert dec(good).tape_dtype == good
    with pytest.raises(ValueError, match="tape_dtype must be one of"):
        dec("fp16")
    with pytest.raises(ValueError, match="tape_dtype must be one of"):
        dec(None)


@pytest.mark.parametrize("kw, missing", [
    (dict(kernels="compiled", matmul_dtype="f32", attn_dtype="f32"), ["kernels='generic'", "matmul_dtype='bf16'", "attn_dtype='bf16'"]),
    (dict(kernels="auto", matmul_dtype="f32", attn_dtype="f32"), ["kernels='generic'", "matmul_dtype='bf16'", "attn_dtype='bf16'"]),
    (dict(matmul_dtype="f32"), ["matmul_dtype='bf16'"]),
    (dict(attn_dtype="f32"), ["attn_dtype='bf16'"]),
    (dict(matmul_dtype="f32", attn_dtype="f32"), ["matmul_dtype='bf16'", "attn_dtype='bf16'"]),
])
def test_bf16_storage_needs_both_bf16_options_on_the_generic_kernels(kw, missing):
    with pytest.raises(ValueError, match="tape_dtype='bf16' needs") as e:
        dec("bf16", **kw)
    for m in missing:
        assert m in str(e.value)
    for present in {"kernels='generic'", "matmul_dtype='bf16'", "attn_dtype='bf16'"} - set(missing):
        assert present not in str(e.value)  # what is satisfied is not named
    assert dec("f32", **kw).tape_dtype == "f32"  # the default asks for nothing


def test_dims_carry_the_bit_only_when_asked():
    assert BIT == 0x1000 and not BIT & (0x300 | 1 | BOTH)
    assert dec("bf16").dims().compute_dtype == GEN | BOTH | BIT
    assert dec("bf16", autograd=True, train_dropout=True, train_lengths=True).dims().compute_dtype == GEN | BOTH | BIT
    # the default: exactly today's bits, in every combination of the other two options and for the default decoder
    for md, ad, want in (("f32", "f32", GEN), ("bf16", "f32", GEN | MM), ("f32", "bf16", GEN | ATT), ("bf16", "bf16", GEN | BOTH)):
        assert dec("f32", matmul_dtype=md, attn_dtype=ad).dims().compute_dtype == want
        assert EdgeDiffusionDecoder(CFG(device="cpu"), kernels="generic", matmul_dtype=md, attn_dtype=ad).dims().compute_dtype == want
    assert EdgeDiffusionDecoder(CFG(device="cpu")).dims().compute_dtype == 0


def test_header_constants_are_the_python_ones():
    with open(os.path.join(REPO, "include", "edtts.h")) as f:
        text = f.read()
    m = re.search(r"\benum\s*\{\s*EDTTS_TAPE_BF16\s*=\s*(\w+)\s*\}", text)
    assert m and int(m.group(1), 0) == BIT
    for i, name in enumerate(native.TAPE_REGIONS):
        m = re.search(r"\bEDTTS_TAPE_%s\s*=\s*(\d+)" % name.upper(), text)
        assert m and int(m.group(1)) == i == getattr(native, "EDTTS_TAPE_" + name.upper())
    assert set(native.TAPE_NARROWED) == set(TU.NARROWED) <= set(native.TAPE_REGIONS)


# ---------------------------------------------------------------------------------------------- the library: refusals
QUERIES = (native.packed_bytes, lambda x: native.workspace_bytes(x, 2, 32, 16, 2), lambda x: native.train_tape_bytes(x, 2, 32, 16),
           lambda x: native.train_scratch_bytes(x, 2, 32, 16), lambda x: native.generic_slot_dest(x, 0),
           lambda x: native.train_tape_region(x, 2, 32, 16, 0, "qkv"))


@pytest.mark.parametrize("bits, why", [
    (GEN, "neither bf16 option"),
    (GEN | MM, "without EDTTS_ATTN_BF16"),
    (GEN | ATT, "without EDTTS_MATMUL_BF16"),
    (BOTH, "without EDTTS_KERNELS_GENERIC"),
    (0, "EDTTS_F32 alone"),
    (1 | GEN | BOTH, "EDTTS_BF16"),
    (1, "EDTTS_BF16 alone"),
    (0x200 | BOTH, "EDTTS_KERNELS_AUTO at a compiled shape"),
    (0x300 | BOTH, "both kernel bits"),
    (GEN | BOTH | 0x2000, "an unknown bit on top"),
])
def test_library_refuses_the_bit_elsewhere(bits, why):
    d = EdgeDiffusionDecoder(CFG(device="cpu")).dims()  # 160/4/80: a compiled instance
    d.compute_dtype = bits | BIT
    for query in QUERIES:
        with pytest.raises(native.EdttsError, match=r"code -1\).*EDTTS_TAPE_BF16"):  # EDTTS_ERR_UNSUPPORTED, naming the bit
            query(d)
    d.compute_dtype = 0x200 | BOTH | BIT
    d.hidden, d.heads = 224, 7  # AUTO would resolve to the generic kernels here: still not the legal spelling
    with pytest.raises(native.EdttsError, match=r"code -1\).*EDTTS_TAPE_BF16"):
        native.packed_bytes(d)


def test_the_legal_spelling_is_accepted():
    d = EdgeDiffusionDecoder(CFG(device="cpu")).dims()
    d.compute_dtype = GEN | BOTH | BIT
    assert native.packed_bytes(d) > 0 and native.train_tape_bytes(d, 2, 32, 16) > 0


def _message(bits):
    d = EdgeDiffusionDecoder(CFG(device="cpu")).dims()
    d.compute_dtype = bits
    with pytest.raises(native.EdttsError) as e:
        native.packed_bytes(d)
    return str(e.value)


def test_refusals_without_the_bit_keep_their_words():
    att = ("EDTTS_ATTN_BF16 is legal only as EDTTS_F32 | EDTTS_KERNELS_GENERIC | EDTTS_ATTN_BF16, with or without "
           "EDTTS_MATMUL_BF16")
    mm = "EDTTS_MATMUL_BF16 is legal only as EDTTS_F32 | EDTTS_KERNELS_GENERIC | EDTTS_MATMUL_BF16"
    for bits in (ATT, 1 | ATT, 0x200 | ATT, BOTH, 0x300 | BOTH):
        msg = _message(bits)
        assert f"compute_dtype=0x{bits:x}: {att}" in msg and "EDTTS_TAPE_BF16" not in msg and "code -1" in msg
    for bits in (MM, 1 | MM, 0x200 | MM, 1 | GEN | MM):
        msg = _message(bits)
        assert f"compute_dtype=0x{bits:x}: {mm}" in msg and "code -1" in msg
        assert "EDTTS_TAPE_BF16" not in msg and "EDTTS_ATTN_BF16" not in msg
    assert "EDTTS_KERNELS_GENERIC and EDTTS_KERNELS_AUTO are exclusive" in _message(0x300)
    assert "the generic kernels are fp32 only" in _message(1 | GEN)


def test_region_query_checks_its_arguments():
    d = dec("bf16", name="G2").dims()
    # (the numbers behind the per-layer members name the whole-model ones, native.TAPE_GLOBALS; the first number past those is refused)
    for layer, which in ((-1, 0), (2, 0), (0, -1), (0, len(native.TAPE_REGIONS) + len(native.TAPE_GLOBALS)), (2, len(native.TAPE_REGIONS))):
        with pytest.raises((native.EdttsError, ValueError)):
            native.train_tape_region(d, 2, 19, 9, layer, which)


# ---------------------------------------------------------------------------------------------- the library: sizes
@pytest.mark.parametrize("name", TU.NAMES)
def test_tape_shrinks_by_the_four_regions_and_nothing_else_moves(name):
    B, T, S = AU.shape(name)
    on, off = dec("bf16", name=name, autograd=True), dec("f32", name=name, autograd=True)
    a, b, cfg = on.dims(), off.dims(), on.cfg
    assert a.compute_dtype == b.compute_dtype | BIT
    L = cfg.layers
    saved = native.train_tape_bytes(b, B, T, S) - native.train_tape_bytes(a, B, T, S)
    want = 2 * L * TU.narrowed_elements(cfg, B, T, S)  # 2 bytes per element of M 3H + M H + M FM H + B S 2H, per layer
    assert abs(saved - want) <= 256 * 4 * L and saved > 0  # (each of the 4 L narrowed regions is padded to 256 bytes)
    for q in (native.packed_bytes, lambda d: native.workspace_bytes(d, B, T, S, B), lambda d: native.workspace_bytes(d, B, T, S, 3),
              lambda d: native.train_scratch_bytes(d, B, T, S)):
        assert q(a) == q(b) > 0
    n_slots = len(native.slot_names(a.layers))
    assert [native.generic_slot_dest(a, i) for i in range(n_slots)] == [native.generic_slot_dest(b, i) for i in range(n_slots)]
    assert on._mirror_map() == off._mirror_map() != None  # noqa: E711
    assert native.substreams_for(a, B, T) == 1


@pytest.mark.parametrize("name", TU.NAMES)
def test_regions_are_disjoint_aligned_and_inside_the_tape(name):
    B, T, S = AU.shape(name)
    for tape_dtype in ("bf16", "f32"):
        d16 = dec(tape_dtype, name=name, autograd=True)
        d, cfg = d16.dims(), d16.cfg
        total = native.train_tape_bytes(d, B, T, S)
        spans = []
        for layer in range(cfg.layers):
            for which in native.TAPE_REGIONS:
                off, n, eb = native.train_tape_region(d, B, T, S, layer, which)
                assert (off, n, eb) == native.train_tape_region(d, B, T, S, layer, native.TAPE_REGIONS.index(which))
                assert eb == (2 if tape_dtype == "bf16" and which in TU.NARROWED else 4), (layer, which)
                rows, cols = TU.region_shape(cfg, B, T, S, which)
                assert n == rows * cols * eb and off % 256 == 0 and 0 <= off and off + n <= total
                spans.append((off, off + n))
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        assert spans[0][0] > 0  # the AdaLN and context rows lie in front of the first layer


def test_default_model_tape_goes_from_11_to_8_hidden_widths_per_frame_and_layer():
    """The figure of DESIGN.md section 28, as arithmetic on the library's answers: at the default model (H 160, FM 2) a frame's share
    of a layer's decoder-row regions is h0 + h1 + h2 + qkv (3) + att1 + qc + att2 + act (2) = 11 H floats, of which qkv, qc and act
    (6 H) halve: 8 H."""
    on, off = dec("bf16", autograd=True), dec("f32", autograd=True)
    cfg, B, T, S = on.cfg, 8, 512, 256
    per = {}
    for key, d in (("on", on.dims()), ("off", off.dims())):
        per[key] = sum(native.train_tape_region(d, B, T, S, 0, w)[1] for w in native.TAPE_REGIONS if w not in ("crp", "kv", "lse1", "lse2"))
    assert per["off"] == 11 * cfg.hidden * 4 * B * T and per["on"] == 8 * cfg.hidden * 4 * B * T


# ---------------------------------------------------------------------------------------------- why "bitwise" is the right bar
@pytest.mark.parametrize("name", ["G2", "A2"])
def test_storing_the_rounded_value_changes_no_gradient_bit(name):
    """Under the model of both bf16 options every consumer of q, k, v (both attentions) and of the SwiGLU output rounds it to bf16.
    Rounding those values once more BEFORE the consumers see them -- which is what a bf16 buffer does -- changes no bit of eps or of
    any gradient: round-to-nearest-even is idempotent.  This runs no new code; it is the argument for comparing with torch.equal."""
    cfg, sd, inp = AU.case(name)
    with AU.model("both"):
        loss_a, g_a = train_util.oracle_grads(cfg, sd, inp, torch.float32)
    counts = {}
    with TU.stored_model(cfg, counts):
        loss_b, g_b = train_util.oracle_grads(cfg, sd, inp, torch.float32)
    assert counts == {"attn": 2 * cfg.layers, "act": cfg.layers}  # every hook fired: both attentions and the down projection of each layer
    assert torch.equal(loss_a, loss_b)
    assert set(g_a) == set(g_b)
    seen = 0
    for k, v in g_a.items():
        if v is None:
            assert g_b[k] is None, k
            continue
        assert torch.equal(v, g_b[k]), f"{name} {k}: {int((v != g_b[k]).sum())} elements differ"
        seen += 1
    assert seen > 10 and float(g_a["d_x"].abs().max()) > 0
    # ... and the hook is not a no-op on the values themselves: the stored q differs from the fp32 one
    x = torch.randn(64, generator=torch.Generator().manual_seed(0))
    assert not torch.equal(TU._Stored.apply(x), x) and torch.equal(TU._Stored.apply(TU._Stored.apply(x)), TU._Stored.apply(x))
