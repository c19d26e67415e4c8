"""The stage audit of the generic training forward, host side (tests/tape_audit_util.py): the stage references
chained are the fp64 oracle, an fp32 emulation of the rounding contract meets every bar under every option set, and each mutant of
that emulation -- a fault of the kind a kernel can have -- fails the bar of its stage.  The GPU file audits the kernels with the same
references and bars.  Pure CPU."""
import functools
import os
import re

import pytest

import dropout_util as DU
import tape_audit_util as TA
import tape_bf16_util as TU
import train_bf16_util as U
import train_ragged_util as R
from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, native
from oracle import edtts_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALL = TA.PLAIN + TA.RAGGED
SMALL = ("G2", "A2", "D4")  # what the mutants run on (R4 for the ragged one, G2 for the dropout one)


def drop_of(name):
    return TA.drop_mults(TA.case(name), U.DROP_P, U.drop_seeds()[0])


@functools.lru_cache(maxsize=None)
def emulated(name, opts, dropped=False, mutant=None):
    cs = TA.case(name)
    drop = drop_of(name) if dropped else None
    return TA.audit(cs, opts, TA.emulate(cs, opts, drop, mutant), drop)


# ------------------------------------------------------------------------------------------------------------ 1. the host query
def test_header_and_binding_name_the_whole_model_members():
    with open(os.path.join(REPO, "include", "edtts.h")) as f:
        text = f.read()
    for i, name in enumerate(native.TAPE_GLOBALS, start=len(native.TAPE_REGIONS)):
        m = re.search(r"\bEDTTS_TAPE_%s\s*=\s*(\d+)" % name.upper(), text)
        assert m and int(m.group(1)) == i == getattr(native, "EDTTS_TAPE_" + name.upper())
    assert native.TAPE_GLOBALS == ("cond", "tcond", "ctx", "hl") and len(native.TAPE_REGIONS) == 12


@pytest.mark.parametrize("bits", [0, TU.BOTH | TU.BIT])
def test_whole_model_regions_lie_where_the_layout_puts_them(bits):
    cfg = CFG(device="cpu", hidden=50, heads=5, n_mels=45, semantic_dim=7, attn_window_size=3, layers=2)
    kw = dict(matmul_dtype="bf16", attn_dtype="bf16", tape_dtype="bf16") if bits else {}
    d = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, **kw).dims()
    B, T, S, H, L = 3, 19, 9, 50, 2
    total = native.train_tape_bytes(d, B, T, S)
    got = {}
    for which in native.TAPE_GLOBALS:
        per_layer = {native.train_tape_region(d, B, T, S, layer, which) for layer in range(L)}
        assert len(per_layer) == 1  # the answer does not depend on the layer
        got[which] = per_layer.pop()
        assert got[which] == native.train_tape_region(d, B, T, S, 0, len(native.TAPE_REGIONS) + native.TAPE_GLOBALS.index(which))
        rows, cols = TU.region_shape(cfg, B, T, S, which)
        assert got[which][1:] == (rows * cols * 4, 4)  # always fp32
    assert got["cond"][0] == 0 and got["tcond"][0] == B * L * 4 * H * 4  # t_cond right behind the AdaLN rows
    first = min(native.train_tape_region(d, B, T, S, 0, w)[0] for w in native.TAPE_REGIONS)
    assert got["tcond"][0] + got["tcond"][1] <= got["ctx"][0] and got["ctx"][0] % 256 == 0
    assert got["ctx"][0] + got["ctx"][1] <= first  # the context rows lie between the conditioning rows and layer 0
    last = max(sum(native.train_tape_region(d, B, T, S, L - 1, w)[:2]) for w in native.TAPE_REGIONS)
    assert last <= got["hl"][0] and got["hl"][0] % 256 == 0 and got["hl"][0] + got["hl"][1] <= total < got["hl"][0] + got["hl"][1] + 256
    for layer, which in ((-1, "ctx"), (L, "hl"), (0, 16)):
        with pytest.raises(native.EdttsError, match="edtts_train_tape_region"):
            native.train_tape_region(d, B, T, S, layer, which)


# ------------------------------------------------------------------------------------------------------------ 2. the references
@pytest.mark.parametrize("name", TA.PLAIN)
def test_chained_references_are_the_fp64_oracle(name):
    cs = TA.case(name)
    inp, cfg = cs.inp, cs.cfg
    want = O.decoder_forward(TA.weights(cs), inp["x"].double(), inp["t"], inp["sem"], inp["si"], None if inp["f"] is None else inp["f"].double(),
                             heads=cfg.heads, window=cfg.attn_window_size)
    got = TA.chain(cs)["eps"].reshape(want.shape)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("name", TA.DROPPED)
def test_chained_references_under_dropout_are_the_masked_oracle(name):
    cs = TA.case(name)
    inp, cfg, seed = cs.inp, cs.cfg, U.drop_seeds()[0]
    want = DU.decoder_forward(TA.weights(cs), inp["x"].double(), inp["t"], inp["sem"], inp["si"], None if inp["f"] is None else inp["f"].double(),
                              heads=cfg.heads, window=cfg.attn_window_size, p=U.DROP_P, seed=seed)
    got = TA.chain(cs, drop=drop_of(name))["eps"].reshape(want.shape)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert float((got - TA.chain(cs)["eps"].reshape(want.shape)).abs().max()) > 1e-3  # the masks act


@pytest.mark.parametrize("name", TA.RAGGED)
def test_chained_references_of_a_ragged_batch_are_the_per_utterance_oracle(name):
    cs = TA.case(name)
    inp = cs.inp
    solo = R.ragged_eps(cs.cfg, TA.weights(cs), inp["x"].double(), None if inp["f"] is None else inp["f"].double(), inp, cs.t_len, cs.s_len)
    got = TA.chain(cs)["eps"].reshape(cs.B, cs.T, -1)
    for b, e in enumerate(solo):
        Tb = int(cs.t_len[b])
        assert float((got[b, :Tb] - e[0]).abs().max()) <= 1e-12 * max(1.0, float(e.abs().max())), b
        assert not bool(got[b, Tb:].any())  # exactly 0 past T_b


# ------------------------------------------------------------------------------------------------------------ 3. the bars can be met
@pytest.mark.parametrize("opts", TA.OPTION_SETS, ids=lambda o: "mm%d-att%d-tape%d" % o)
@pytest.mark.parametrize("name", ALL)
def test_emulation_meets_every_bar(name, opts):
    by = TA.check(emulated(name, opts), f"{name} {tuple(opts)}")
    assert set(by) == {"exact", "norm", "attention", "norm+function"}


@pytest.mark.parametrize("opts", TA.OPTION_SETS, ids=lambda o: "mm%d-att%d-tape%d" % o)
@pytest.mark.parametrize("name", TA.DROPPED)
def test_emulation_with_dropout_meets_every_bar(name, opts):
    TA.check(emulated(name, opts, True), f"{name} p={U.DROP_P} {tuple(opts)}")


# ------------------------------------------------------------------------------------------------------------ 4. ... and are not vacuous
def _mutant_runs():
    f32, mm, att, all3 = TA.OPTION_SETS[0], TA.OPTION_SETS[1], TA.OPTION_SETS[2], TA.OPTION_SETS[4]
    runs = []
    for m in ("last_key", "window", "k_term_exact", "k_term_norm", "swap", "bias", "snapshot"):
        runs += [(m, n, o, False) for n in SMALL for o in (f32, all3)]
    runs += [("key_at_len", "R4", o, False) for o in (f32, all3)] + [("key_at_len", "R2", all3, False)]
    runs += [("unrounded_mm", n, o, False) for n in SMALL for o in (mm, all3)]
    # (with bf16 storage q, k and v arrive rounded: leaving them "unrounded" is then no fault, so the option sets without it)
    runs += [("unrounded_att", n, o, False) for n in SMALL for o in (att, TA.OPTION_SETS[3])]
    runs += [("drop_l", "G2", o, True) for o in (f32, all3)]
    return runs


@pytest.mark.parametrize("mutant, name, opts, dropped", _mutant_runs(), ids=lambda v: v if isinstance(v, str) else ("mm%d-att%d-tape%d" % v if isinstance(v, tuple) else str(int(v))))
def test_every_mutant_fails_the_bar_of_its_stage(mutant, name, opts, dropped):
    res = emulated(name, opts, dropped, mutant)
    stage = TA.MUTANTS[mutant]
    clean = emulated(name, opts, dropped)
    print(f"{mutant} on {name} {tuple(opts)}: {stage} error / bar {res[stage].ratio:.3g} (unmutated {clean[stage].ratio:.3g})")
    assert res[stage].ratio > 1.0 and clean[stage].ratio <= 1.0
    # every stage before it is untouched (each stage is judged on its own operands)
    for k in res:
        if k in (stage, stage.replace("lse", "att")):  # (an attention's output and log-sum-exp are one launch)
            break
        assert res[k].ratio == clean[k].ratio, k


# ------------------------------------------------------------------------------------------------------------ 5. the premises
@pytest.mark.parametrize("name", ALL)
def test_ambiguous_operands_are_under_one_percent_of_every_stage(name):
    cs = TA.case(name)
    amb = []
    TA.audit(cs, TA.OPTION_SETS[3], TA.emulate(cs, TA.OPTION_SETS[3]), amb=amb)
    assert len(amb) == 4 * cs.cfg.layers + 1  # kv, qkv, qc, act per layer, eps
    print(f"{name}: ambiguous fraction per norm-class stage, worst {max(amb):.3%}")
    assert max(amb) <= TA.AMBIGUOUS_MAX


def test_measured_allowances_are_the_ones_in_use():
    eta, c_lse, c_fn = TA.measure_allowances(ALL)
    print(f"fp32 oracle against fp64 on the audit cases: eta {eta:.3e} (x{TA.MARGIN:g} = {TA.MARGIN * eta:.3e}, in use {TA.ETA:.3e}); "
          f"c {c_lse:.2f} u (x{TA.MARGIN:g} = {TA.MARGIN * c_lse:.2f}, in use {TA.C_LSE}); "
          f"function {c_fn:.2f} u (x{TA.MARGIN:g} = {TA.MARGIN * c_fn:.2f}, in use {TA.C_FN})")
    for measured, used in ((eta, TA.ETA), (c_lse, TA.C_LSE), (c_fn, TA.C_FN)):
        assert used / 2 < TA.MARGIN * measured <= used  # the constant is the margin times the measurement, rounded up to a power of two
