"""The stage audit of the generic training backward, host side (tests/bwd_audit_util.py): the site references
chained are torch.autograd through the fp64 oracle, an fp32 emulation of the rounding contract meets every bar under every option
set, each mutant of that emulation -- a fault of the kind a kernel can have -- fails the bar of its site, and the measured allowances
are the ones in use.  The GPU file audits the kernels with the same references and bars.  Pure CPU."""
import functools
import os
import re

import pytest
import torch

import bwd_audit_util as BA
import dropout_util as DU
import tape_audit_util as TA
import train_bf16_util as U
import train_ragged_util as R
from edge_diffusion_tts_amd import EdgeDiffusionDecoder, native
from oracle import edtts_oracle as O
from train_util import BUFFERS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = TA.PLAIN + TA.RAGGED
IDS = {o: "mm%d-att%d-tape%d" % o for o in TA.OPTION_SETS}
opt_sets = pytest.mark.parametrize("opts", TA.OPTION_SETS, ids=lambda o: IDS[o])


def drop_of(name):
    return TA.drop_mults(TA.case(name), U.DROP_P, U.drop_seeds()[0])


# ------------------------------------------------------------------------------------------------------------ 1. the host queries
def test_header_and_binding_name_the_same_sites_and_regions():
    with open(os.path.join(REPO, "include", "edtts.h")) as f:
        text = f.read()
    for i, name in enumerate(native.BWD_SITES):
        m = re.search(r"\bEDTTS_BWD_%s\s*=\s*(\d+)" % name.upper(), text)
        assert m and int(m.group(1)) == i, name
    assert int(re.search(r"\bEDTTS_BWD_COUNT\s*=\s*(\d+)", text).group(1)) == len(native.BWD_SITES)
    for i, name in enumerate(native.SCRATCH_REGIONS):
        m = re.search(r"\bEDTTS_SCRATCH_%s\s*=\s*(\d+)" % name.upper(), text)
        assert m and int(m.group(1)) == i, name
    assert native.BWD_LAYER_SITES == native.BWD_SITES[2:19] and native.BWD_LAYER_SITES[0] == "dropdown" and native.BWD_LAYER_SITES[-1] == "n1"


@pytest.mark.parametrize("name", ALL)
def test_scratch_regions_tile_the_scratch_and_its_size_is_unchanged(name):
    """The members lie in SCRATCH_REGIONS order, each on a multiple of 256 bytes right behind the one before it, and the last one ends
    where edtts_train_scratch_bytes says -- which is the figure the layout gave before the members had names (restated here)."""
    cs = TA.case(name)
    cfg, B, T, S = cs.cfg, cs.B, cs.T, cs.S
    for kw in ({}, dict(matmul_dtype="bf16", attn_dtype="bf16", tape_dtype="bf16")):
        d = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, **kw).dims()
        at = 0
        sizes = {}
        for which in native.SCRATCH_REGIONS:
            off, n = native.train_scratch_region(d, B, T, S, which)
            assert off == at and off % 256 == 0 and n % 4 == 0, which
            assert (off, n) == native.train_scratch_region(d, B, T, S, native.SCRATCH_REGIONS.index(which))
            at = (off + n + 255) // 256 * 256
            sizes[which] = n // 4
        assert at == native.train_scratch_bytes(d, B, T, S)
        H, M, CS, FH, Rk, L = cfg.hidden, B * T, B * S, cfg.ffn_mult * cfg.hidden, cfg.hidden // 2, cfg.layers
        want = dict(dh=M * H, xn=M * H, ga=M * H, gq=M * H, big=M * max(2 * FH, 3 * H), da=M * FH, stat=2 * max(M, CS), delta=M * cfg.heads,
                    dkv=CS * 2 * H, crn=CS * Rk, dcr=CS * Rk, dcp=CS * Rk, dctx=CS * H, dmod=B * L * 4 * H, dtc=B * H, e=B * H, a1=B * H,
                    u1=B * H, du1=B * H)
        assert {k: sizes[k] for k in want} == want

        def dwp(rows, n, k):
            r = native.train_dw_slab_rows(rows)
            ns = (rows + r - 1) // r
            return ns * n * k if ns > 1 else 0

        mel, sdim = cfg.n_mels, cfg.semantic_dim
        part = max(dwp(M, mel, H), dwp(M, H, FH), dwp(M, 2 * FH, H), dwp(M, H, H), dwp(M, 3 * H, H), dwp(M, H, mel), dwp(CS, 2 * H, Rk),
                   dwp(CS, Rk, H), dwp(CS, H, sdim), dwp(B, 2 * H, H), dwp(B, H, H), (M + 255) // 256 * max(2 * FH, mel), (CS + 255) // 256 * H,
                   B * ((max(T, S) + 63) // 64) * 3 * H)
        assert sizes["part"] == part
    for which in (-1, len(native.SCRATCH_REGIONS)):
        with pytest.raises(native.EdttsError, match="edtts_train_scratch_region"):
            native.train_scratch_region(d, B, T, S, which)


# ------------------------------------------------------------------------------------------------------------ 2. the references
def _leaves(cs):
    sd = TA.weights(cs)
    p = {k: (v.clone().requires_grad_(k not in BUFFERS) if v.is_floating_point() else v) for k, v in sd.items()}
    x = cs.inp["x"].double().clone().requires_grad_(True)
    f = None if cs.inp["f"] is None else cs.inp["f"].double().clone().requires_grad_(True)
    return p, x, f


def _check_chain(cs, st, p, x, f):
    checked = 0
    for k, v in list(p.items()) + [("d_x", x), ("d_sem", f)]:
        if v is None or not v.is_floating_point() or k in BUFFERS or v.grad is None:
            continue
        got = st[k if k in ("d_x", "d_sem") else "g:" + k].reshape(v.grad.shape)
        assert float(v.grad.abs().max()) > 0 or cs.S == 1, k  # (one key: the cross scores have no gradient, D7)
        assert float((got - v.grad).abs().max()) <= 1e-12 * max(1.0, float(v.grad.abs().max())), k
        checked += 1
    assert checked == sum(1 for k in st if k.startswith("g:") or k in ("d_x", "d_sem"))


@pytest.mark.parametrize("name", TA.PLAIN)
def test_chained_references_are_autograd_through_the_fp64_oracle(name):
    cs = TA.case(name)
    inp, cfg = cs.inp, cs.cfg
    p, x, f = _leaves(cs)
    eps = O.decoder_forward(p, x, inp["t"], inp["sem"], inp["si"], f, heads=cfg.heads, window=cfg.attn_window_size)
    (eps * BA.d_eps_of(cs).double()).sum().backward()
    _check_chain(cs, BA.chain(BA.Ctx(cs, TA.OPTION_SETS[0], TA.chain(cs))), p, x, f)


@pytest.mark.parametrize("name", TA.DROPPED)
def test_chained_references_under_dropout_are_autograd_through_the_masked_oracle(name):
    cs = TA.case(name)
    inp, cfg, seed = cs.inp, cs.cfg, U.drop_seeds()[0]
    p, x, f = _leaves(cs)
    eps = DU.decoder_forward(p, x, inp["t"], inp["sem"], inp["si"], f, heads=cfg.heads, window=cfg.attn_window_size, p=U.DROP_P, seed=seed)
    (eps * BA.d_eps_of(cs).double()).sum().backward()
    drop = drop_of(name)
    _check_chain(cs, BA.chain(BA.Ctx(cs, TA.OPTION_SETS[0], TA.chain(cs, drop=drop), drop)), p, x, f)


@pytest.mark.parametrize("name", TA.RAGGED)
def test_chained_references_of_a_ragged_batch_are_autograd_through_the_per_utterance_oracle(name):
    cs = TA.case(name)
    p, x, f = _leaves(cs)
    d_eps = BA.d_eps_of(cs).double()
    eps = R.ragged_eps(cs.cfg, p, x, f, cs.inp, cs.t_len, cs.s_len)
    sum((e * d_eps[b:b + 1, :e.shape[1]]).sum() for b, e in enumerate(eps)).backward()
    # NaN in all padding of x, sem_features and d_eps: no reference reads it
    inp = dict(cs.inp)
    inp["x"] = inp["x"].masked_fill(~R.frame_mask(cs.t_len, cs.T), float("nan"))
    inp["f"] = inp["f"].masked_fill(~R.frame_mask(cs.s_len, cs.S), float("nan"))
    nan_cs = cs._replace(inp=inp)
    cx = BA.Ctx(nan_cs, TA.OPTION_SETS[0], TA.chain(cs), d_eps=d_eps.masked_fill(~R.frame_mask(cs.t_len, cs.T), float("nan")))
    st = BA.chain(cx)
    _check_chain(cs, st, p, x, f)
    assert not bool(st["d_x"].reshape(cs.B, cs.T, -1)[~R.frame_mask(cs.t_len, cs.T).expand(-1, -1, cs.cfg.n_mels)].any())
    assert not bool(st["d_sem"].reshape(cs.B, cs.S, -1)[~R.frame_mask(cs.s_len, cs.S).expand(-1, -1, cs.cfg.semantic_dim)].any())


# ------------------------------------------------------------------------------------------------------------ 3. the bars can be met
@functools.lru_cache(maxsize=None)
def context(name, opts, dropped=False):
    cs = TA.case(name)
    drop = drop_of(name) if dropped else None
    return BA.Ctx(cs, opts, TA.emulate(cs, opts, drop), drop)


@functools.lru_cache(maxsize=None)
def emulated(name, opts, dropped=False, mutant=None):
    cx = context(name, opts, dropped)
    return BA.audit(cx, BA.emulated(cx, mutant))


@opt_sets
@pytest.mark.parametrize("name", ALL)
def test_emulation_meets_every_bar(name, opts):
    by = BA.check(emulated(name, opts), f"{name} {IDS[opts]}")
    assert set(native.BWD_SITES) - {"dropdown", "ada", "step", "time"} <= set(by)


@opt_sets
@pytest.mark.parametrize("name", TA.DROPPED)
def test_emulation_with_dropout_meets_every_bar(name, opts):
    by = BA.check(emulated(name, opts, True), f"{name} p={U.DROP_P} {IDS[opts]}")
    assert "dropdown" in by


# ------------------------------------------------------------------------------------------------------------ 4. ... and are not vacuous
SMALL = ("G2", "A2", "D4", "G4")
ROUNDING = {"bias_rounded": lambda o: o.mm, "unrounded": lambda o: o.mm, "delta_rounded": lambda o: o.att}  # faults only where something is rounded


def _mutant_runs():
    runs = []
    for m in BA.MUTANTS:
        names, dropped = SMALL, False
        if m in ("row_at_len", "dw_dead_row"):
            names = TA.RAGGED
        if m == "drop_delta":
            names, dropped = TA.DROPPED, True
        runs += [(m, o, names, dropped) for o in TA.OPTION_SETS if ROUNDING.get(m, lambda o: True)(o)]
    return runs


@pytest.mark.parametrize("mutant, opts, names, dropped", _mutant_runs(),
                         ids=lambda v: v if isinstance(v, str) else (IDS[v] if isinstance(v, TA.Opts) else ""))
def test_every_mutant_fails_the_bar_of_its_site(mutant, opts, names, dropped):
    """On at least one case under every option set (under which the mutant is a fault at all); the sites before it are untouched."""
    worst = 0.0
    for name in names:
        cx = context(name, opts, dropped)
        target = BA.mutant_target(cx, mutant)
        res, clean = emulated(name, opts, dropped, mutant), emulated(name, opts, dropped)
        if target not in res:
            continue
        assert clean[target].ratio <= 1.0
        for k in res:
            if k[0] == target[0]:
                break
            assert res[k].ratio == clean[k].ratio, k
        print(f"{mutant} on {name} {IDS[opts]}: {target} error / bar {res[target].ratio:.3g} (unmutated {clean[target].ratio:.3g})")
        worst = max(worst, res[target].ratio)
    print(f"{mutant} {IDS[opts]}: worst error / bar {worst:.3g}")
    assert worst > 1.0


# ------------------------------------------------------------------------------------------------------------ 5. the premises
def test_the_ambiguous_share_decides_between_the_bracket_and_the_relative_term():
    """Under bf16 attention rnd(dS) and rnd(P D) could be bracketed as section 29 brackets norm rows if all but 1 % of each stage's
    operand were decided for the reference alone on every case; otherwise the bars carry 2^-8 per summand.  BA.ATT_BRACKET must say
    which of the two the measured shares allow."""
    worst = {}
    for name in ALL + tuple(n + "+drop" for n in TA.DROPPED):
        cx = context(name.split("+")[0], TA.OPTION_SETS[3], name.endswith("+drop"))
        amb = []
        BA.audit(cx, BA.emulated(cx), amb=amb)
        assert len(amb) == 6 * cx.L  # dq, dk, dv of both attentions of every layer
        worst[name] = max(amb, key=lambda a: a[1])
        print(f"{name}: ambiguous fraction per attention-backward operand, worst {worst[name][1]:.3%} at {worst[name][0]}")
    assert (max(w[1] for w in worst.values()) <= TA.AMBIGUOUS_MAX) == BA.ATT_BRACKET


def test_measured_allowances_are_the_ones_in_use():
    m = BA.measure_allowances(ALL)
    for k in BA.ALLOWANCES:
        used = getattr(BA, k)
        print(f"{k}: fp32 CPU against fp64 on the audit cases {m[k]:.3e} (x{BA.MARGIN:g} = {BA.MARGIN * m[k]:.3e}, in use {used:.3e})")
    for k in BA.ALLOWANCES:
        used = getattr(BA, k)
        assert used / 2 < BA.MARGIN * m[k] <= used, k  # the constant is the margin times the measurement, rounded up to a power of two
