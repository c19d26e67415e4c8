"""CPU side of the HuBERT backbone's site-by-site audit (tests/hubert_audit_util.py): the chained fp64 references
are the model (the fixture's stored fp64 outputs; transformers in fp64 where it is installed), an fp32 emulation of either compute
dtype meets every bar on every case, each seeded mutant of it misses the bar of its own site, and the measured allowances are what
the constants say.  No GPU."""
import json
import os
import re

import pytest
import torch

import hubert_audit_util as HU
from edge_diffusion_tts_amd import native

CASES = ("F",) + HU.ECASES + ("A1",)
RUNS = [(c, bf) for c in CASES for bf in (False, True) if not bf or c in HU.BF16_LEGAL]


def shape(name, tag):
    return [s for s in HU.shapes(name) if s.tag == tag][0]


def test_site_names_mirror_the_header():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "edtts.h")) as f:
        text = f.read()
    for i, name in enumerate(native.HUB_SITES):
        assert int(re.search(r"\bEDTTS_HUB_%s\s*=\s*(\d+)" % name.upper(), text).group(1)) == i, name
    assert int(re.search(r"\bEDTTS_HUB_COUNT\s*=\s*(\d+)", text).group(1)) == len(native.HUB_SITES)
    for i, name in enumerate(native.HUB_WS_REGIONS):
        assert int(re.search(r"\bEDTTS_HUB_WS_%s\s*=\s*(\d+)" % name.upper(), text).group(1)) == i, name
    assert int(re.search(r"\bEDTTS_HUB_WS_COUNT\s*=\s*(\d+)", text).group(1)) == len(native.HUB_WS_REGIONS)
    assert native.HUB_LAYER_SITES == ("qkv", "vt", "attn", "oproj", "ln1", "ff1", "ff2", "ln2")
    assert "kGnChunk = %d;" % native.HUB_GN_CHUNK in open(os.path.join(os.path.dirname(native.__file__), "..", "csrc", "edtts_hubert.h")).read()


def test_the_cases_are_the_shapes_they_are_meant_to_be():
    for name in HU.ECASES:
        cs = HU.case(name)
        t1, ragged, t130 = HU.shapes(name)[:3]
        assert HU.stage_frames(cs, t1.wav.shape[1])[-1] == 1 and HU.stage_frames(cs, t1.wav.shape[1] - 1)[-1] < 1
        assert HU.stage_frames(cs, t130.wav.shape[1])[-1] == 130 and t130.wav.shape[0] == 2
        T_audio = ragged.wav.shape[1]
        n = ragged.lengths.clamp(HU.samples_for(cs, 1), T_audio)
        assert HU.stage_frames(cs, n)[-1].tolist() == [65, 65, 33, 1] and HU.stage_frames(cs, T_audio)[-1] == 65
        assert int(ragged.lengths[1]) > T_audio and int(ragged.lengths[3]) < HU.samples_for(cs, 1)  # both clamps
        assert bool(torch.isnan(ragged.wav[3]).any()) and float(ragged.wav[2].max()) == 1e4
        per_utt = [(int(t) + 255) // 256 for t in HU.stage_frames(cs, n)[0]]
        assert len(set(per_utt)) > 1 or name == "E2"  # GroupNorm chunk counts that differ from the padded one
    e1 = HU.case("E1")
    assert [HU.stage_frames(e1, s.wav.shape[1])[0] for s in HU.shapes("E1")[3:]] == list(HU.GN_T0)
    assert HU.stage_frames(e1, 3 * e1.S[0] + e1.K[0])[-1] < 1  # T0 = 4 leaves no output frame: 5 is the smallest
    a1, (sh,) = HU.case("A1"), HU.shapes("A1")
    T0, T1 = HU.stage_frames(a1, sh.wav.shape[1])
    assert T1 == 8100 and (T1 + 127) // 128 * ((a1.C[1] + 127) // 128) * sh.wav.shape[0] == 512 and (T0 + 255) // 256 == 64
    assert HU.case("E2").C[1] < 16 and HU.case("E3").DH == 96 and HU.case("E4").DH == 128 and HU.case("E3").Cg > 64


def test_the_chain_is_the_fixtures_fp64_model():
    cs = HU.case("F")
    z, _, _ = HU.fixture()
    w64 = HU.fold_pos(cs, torch.float64)  # (the stored outputs are transformers' in fp64: its fold is fp64 too)
    pad, ragged = HU.shapes("F")
    snap = HU.chain(cs, pad, False, w64)
    for n in range(4):
        got = snap[("ln2", n - 1) if n else ("encnorm", 0)]
        ref = torch.from_numpy(z[f"pad64_{n}"])
        assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12, n
    out = HU.chain(cs, ragged, False, w64)["zero", 0]
    for b, n in enumerate(ragged.lengths.tolist()):
        ref = torch.from_numpy(z[f"solo64_3_{b}"])
        F = ref.shape[0]
        assert F == HU.stage_frames(cs, n)[-1] and float((out[b, :F] - ref).abs().max()) <= 1e-12, b
        assert float(out[b, F:].abs().sum()) == 0.0


@pytest.mark.parametrize("name", ["F", "E1", "E2"])
def test_the_chain_is_transformers_in_fp64(name):
    transformers = pytest.importorskip("transformers")
    cs = HU.case(name)
    model = transformers.HubertModel(transformers.HubertConfig(**cs.cfg)).eval()
    model.load_state_dict(cs.sd, strict=False)
    got = {k: v for k, v in model.state_dict().items() if k != "masked_spec_embed"}
    assert set(got) == set(cs.sd) and all(torch.equal(got[k], cs.sd[k]) for k in got)
    model = model.double()
    w64 = HU.fold_pos(cs, torch.float64)
    for sh in HU.shapes(name):
        if sh.lengths is not None or sh.until is not None:
            continue  # (transformers' padded batch normalises over the padded time axis: only the calls without lengths compare)
        with torch.no_grad():
            hs = model(sh.wav.double(), output_hidden_states=True).hidden_states
        snap = HU.chain(cs, sh, False, w64)
        for n in range(cs.layers + 1):
            got = snap[("ln2", n - 1) if n else ("encnorm", 0)]
            assert got.shape == hs[n].shape and float((got - hs[n]).abs().max()) <= 1e-12, (sh.tag, n)


@pytest.mark.parametrize("name,bf", RUNS)
def test_the_emulation_meets_every_bar(name, bf):
    cs = HU.case(name)
    for sh in HU.shapes(name):
        res = HU.audit(cs, sh, bf, HU.emulate(cs, sh, bf))
        assert list(res) == HU.site_list(cs, bf, sh.lengths is not None, sh.until)
        HU.check(res, f"hubert emulation {name} {sh.tag} {'bf16' if bf else 'fp32'}")


@pytest.mark.parametrize("mutant", sorted(HU.MUTANTS))
def test_every_mutant_misses_the_bar_of_its_own_site(mutant):
    name, tag, bf, site = HU.MUTANTS[mutant]
    cs, sh = HU.case(name), shape(name, tag)._replace(until=HU.MUTANTS[mutant][3])
    res = HU.audit(cs, sh, bf, HU.emulate(cs, sh, bf, mutant))
    ok = HU.audit(cs, sh, bf, HU.emulate(cs, sh, bf))
    print(f"hubert mutant {mutant}: {site[0]} {site[1]} error / bar {res[site].ratio:.3g} (unmutated {ok[site].ratio:.3f})")
    assert res[site].ratio > 1.0 and ok[site].ratio <= 1.0
    assert all(r.ratio <= 1.0 for k, r in res.items() if k != site), "the sites before it are untouched"


def test_measured_allowances():
    eta, c_gelu = HU.measure_allowances(("F",) + HU.ECASES)
    print(f"hubert allowances: eta {eta:.3e} (x MARGIN = {HU.MARGIN * eta / HU.ETA:.3f} ETA), c_gelu {c_gelu:.3f} (x MARGIN = {HU.MARGIN * c_gelu:.3f})")
    assert HU.ETA / 2 < HU.MARGIN * eta <= HU.ETA
    assert HU.C_GELU / 2 < HU.MARGIN * c_gelu <= HU.C_GELU
    # section 29's form, (|x| + |mean|) rstd |w| + |b| with its ETA = 2^-19, does NOT hold the fp32 CPU evaluation on these operands
    # (rows after a LayerNorm'd residual: mean ~ 0 and elements near 0, while the mean's rounding error scales with mean |x|)
    worst = 0.0
    for name in HU.ECASES:
        cs = HU.case(name)
        for sh in HU.shapes(name)[:3]:
            snap, prev = {}, None
            for key, cls, ref, _, live in HU.sites(cs, sh, False, snap):
                snap[key] = ref
                if cls == "norm":
                    x32 = HU.clean(snap[prev]).float()
                    w, b = (cs.sd[HU.NORM_PARAMS[key[0]].format(key[1]) + n] for n in ("weight", "bias"))
                    y32 = torch.nn.functional.layer_norm(x32, (x32.shape[-1],), w, b, cs.eps)
                    y64, d = HU.AT.layer_rows(x32.double().reshape(-1, x32.shape[-1]), w.double(), b.double(), cs.eps)
                    r = (y32.double().reshape(y64.shape) - y64).abs() / d
                    worst = max(worst, float(r[live.expand_as(x32).reshape(y64.shape)].max()))
                prev = key
    print(f"hubert allowances: section 29's norm bar on these operands, CPU fp32 error / bar {worst:.3f}")
    assert HU.MARGIN * worst > 1.0


def test_the_fold_bar_holds_the_cpu_fold():
    for name in ("F",) + HU.ECASES:
        cs = HU.case(name)
        err = (HU.fold_pos(cs).double() - HU.fold_pos(cs, torch.float64)).abs()
        assert float((err / HU.fold_bar(cs)).max()) <= 1.0


def test_layouts_are_the_recorded_ones():
    """The blob and workspace layouts of both compute dtypes are those of the library before the host side described them once
    (tests/golden/hubert_layout.json, recorded from that library): every size and every member's offset and extent, exactly."""
    with open(HU.LAYOUT_GOLDEN) as f:
        want = json.load(f)
    got = HU.layout_records()
    assert sorted(got) == sorted(want) and len(want) == (1 + 15 + 1) + (1 + 12) + 2  # fp32: F (one B x T_audio), E1-E5, A1; bf16: F, E1 E3 E4 E5; base
    for key in want:
        assert got[key] == want[key], key


def test_workspace_regions():
    """edtts_hubert_workspace_region answers from the layout: the members tile the workspace in order, the views have their shapes,
    and what does not exist is refused by name."""
    for name, dtype in (("F", "fp32"), ("F", "bf16"), ("E1", "bf16"), ("E2", "fp32"), ("A1", "fp32")):
        cs, dt = HU.case(name), native.HUBERT_DTYPES[dtype]
        d = HU.module(cs, dtype).dims
        for sh in HU.shapes(name)[:3]:
            B, T_audio = sh.wav.shape
            total = native.hubert_workspace_bytes(d, B, T_audio, dt)
            names = native.HUB_WS_REGIONS[:8 + dt]
            regs = [native.hubert_workspace_region(d, B, T_audio, dt, n) for n in names]
            assert regs[0][0] == 0 and all(o % 256 == 0 and n % 256 == 0 and n > 0 for o, n in regs)
            assert all(regs[i][0] + regs[i][1] == regs[i + 1][0] for i in range(len(regs) - 1)) and regs[-1][0] + regs[-1][1] == total
            v = native.hubert_workspace_views(d, B, T_audio, dt, torch.zeros(total, dtype=torch.uint8))
            Ts = HU.stage_frames(cs, T_audio)
            T, bf = Ts[-1], bool(dt)
            assert [tuple(c.shape) for c in v["conv"]] == [(B, Ts[i], cs.C[i]) for i in range(len(cs.C))]
            assert [c.dtype for c in v["conv"]] == [torch.bfloat16 if bf and i + 1 < len(cs.C) else torch.float32 for i in range(len(cs.C))]
            assert v["conv"][0].data_ptr() == v["fpnorm"].data_ptr() if len(cs.C) % 2 == 0 else v["conv"][1].data_ptr() == v["fpnorm"].data_ptr()
            assert tuple(v["h"].shape) == tuple(v["att"].shape) == (B, T, cs.H) and tuple(v["qkv"].shape) == (B, T, 3 * cs.H)
            assert v["qkv"].dtype == (torch.bfloat16 if bf else torch.float32) and tuple(v["ff"].shape) == (B, T, cs.I)
            assert tuple(v["lens"].shape) == (2, B) and tuple(v["stats"].shape) == (B, 2, cs.C[0])
            assert ("vt" in v) == bf and (not bf or tuple(v["vt"].shape) == (B, cs.heads, cs.DH, (T + 31) // 32 * 32))
    d = HU.module(HU.case("E1")).dims
    with pytest.raises(native.EdttsError, match="EDTTS_HUB_WS_VT exists only under EDTTS_HUBERT_BF16"):
        native.hubert_workspace_region(d, 1, 4000, 0, "vt")
    for which in (-1, 9):
        with pytest.raises(native.EdttsError, match="edtts_hubert_workspace_region: which="):
            native.hubert_workspace_region(d, 1, 4000, 1, which)
    with pytest.raises(native.EdttsError, match="compute_dtype=2"):
        native.hubert_workspace_region(d, 1, 4000, 2, "h")
    with pytest.raises(native.EdttsError, match="gives no output frame"):
        native.hubert_workspace_region(d, 1, 25, 0, "h")
    assert native.lib().edtts_version() == 400
