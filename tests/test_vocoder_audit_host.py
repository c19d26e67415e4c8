"""Host tests of the vocoder audit (tests/vocoder_audit_util.py): the scratch layout the audit reads through,
the stage references against the oracle composed end to end, the fp32 restatement of every stage within every bar, seeded faults in
the CPU reference each caught by the bar of their own stage and by no other, and the skip cap of stage 5 from the fp64 reference
alone.  No GPU."""
import pytest
import torch

import vocoder_audit_util as VA
from edge_diffusion_tts_amd import GriffinLim, native
from oracle import edtts_oracle as O
from vocoder_audit_util import F32, F64

WINDOW = torch.hann_window(1024)
CASES = VA.gl_cases()
SMALL = VA.gl_cases(hops=(160, 300, 512))  # the fault runs: an even hop that divides 1024, one that does not, and hop = n_fft / 2


@pytest.fixture(scope="module")
def restated():
    """{case: [R0, R1, R2]} of the fp32 restatement, built once."""
    return {repr(cs): [VA.emulate(cs, n, WINDOW) for n in range(3)] for cs in CASES}


def test_window_is_the_modules():
    assert torch.equal(GriffinLim(n_fft=1024, hop_length=160).window, WINDOW)


@pytest.mark.parametrize("B,T,hop", [(1, 2, 1024), (1, 5, 160), (3, 5, 160), (4, 40, 160), (2, 3, 300), (4, 9, 512), (7, 11, 200)])
def test_scratch_members_tile_the_scratch(B, T, hop):
    need = native.griffin_lim_scratch_floats(B, T, 1024, hop)
    lay = native.griffin_lim_scratch_layout(B, T, 1024, hop)
    assert [m for m, _, _ in lay] == ["mag", "ang", "tprev", "frames", "wave"]
    end = 0
    for name, off, shape in lay:
        assert off == end, name
        end = off + int(torch.Size(shape).numel())
    assert end == need
    scratch = torch.arange(need + 3, dtype=F32)
    v = native.griffin_lim_scratch_views(scratch, B, T, 1024, hop)
    assert v["mag"].shape == (B, T, 513) and v["ang"].shape == v["tprev"].shape == (B, T, 513, 2)
    assert v["frames"].shape == (B, T, 1024) and v["wave"].shape == (B, 1024 + hop * (T - 1))
    assert torch.equal(torch.cat([x.reshape(-1) for x in v.values()]), scratch[:need])
    assert all(x.data_ptr() == scratch.data_ptr() + 4 * off for x, (_, off, _) in zip(v.values(), lay))


def test_scratch_too_small_raises():
    spec = torch.zeros(1, 513, 5)
    need = native.griffin_lim_scratch_floats(1, 5, 1024, 160)
    with pytest.raises(native.EdttsError, match=f"at least {need} floats"):
        native.griffin_lim(spec, 1024, 160, WINDOW, WINDOW, 0, 0.99, 2.0, None, scratch=torch.zeros(need - 1))


def test_cases_are_the_issues():
    assert len(CASES) == 30 and max(cs.B for cs in CASES) == 4 and max(cs.T for cs in CASES) == 40
    for cs in CASES:
        t_min = min(cs.rows())
        assert cs.hop * (t_min - 1) > 512 >= cs.hop * (t_min - 2), cs  # the smallest legal row is in every case
        zeros = float((cs.spec == 0).float().mean())
        assert 0.1 < zeros < 0.5, (cs, zeros)


def test_reflect_padding_is_torch_stft():
    cs = CASES[1]
    wave = torch.randn(cs.B, cs.Lp, dtype=F64)
    got = VA.stage_stft(wave, WINDOW, cs.hop, cs.rows(), cs.T)
    for b, Tb in enumerate(cs.rows()):
        ref = torch.stft(wave[b, 512:512 + cs.hop * (Tb - 1)], 1024, cs.hop, 1024, window=WINDOW.double(), center=True, pad_mode="reflect",
                         return_complex=True)
        assert torch.equal(VA.cplx(got[b, :Tb]), ref.transpose(0, 1))


@pytest.mark.parametrize("cs", CASES, ids=repr)
def test_stage_references_compose_to_the_oracle(cs):
    """The stages chained in fp64 are oracle.griffin_lim in fp64 (torch.istft / torch.stft), row by row."""
    for n in range(3):
        st = VA.emulate(cs, n, WINDOW, F64)
        for b, Tb in enumerate(cs.rows()):
            ref = O.griffin_lim(cs.spec[b:b + 1, :, :Tb].double(), 1024, cs.hop, 1024, n, cs.power, cs.momentum,
                                angles0=cs.a0[b:b + 1, :, :Tb].to(torch.complex128))[0]
            got = st["out"][b, :cs.hop * (Tb - 1)]
            # the emulation stores every stage as fp32: agreement to fp32 rounding of the chain, far below any seeded fault
            assert float((got.double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), (n, b)


@pytest.mark.parametrize("cs", CASES, ids=repr)
def test_fp32_restatement_meets_every_bar(cs, restated):
    """(End to end the fp32 restatement is the yardstick itself, oracle.griffin_lim in fp32: there is nothing to restate.)"""
    rep = VA.audit(cs, restated[repr(cs)], WINDOW)
    print(rep.line())
    assert not rep.fails, rep.fails
    assert set(rep.ratios) == {"1", "2", "3", "4", "5", "6", "7"}


def test_end_to_end_bar_on_the_host():
    cs = CASES[0]
    for n in range(3):
        yardstick = O.griffin_lim(cs.spec, 1024, cs.hop, 1024, n, cs.power, cs.momentum, angles0=cs.a0)
        rep = VA.end_to_end(cs, n, yardstick)
        assert not rep.fails and rep.ratios[f"e2e{n}"] <= 0.25
    assert VA.end_to_end(cs, 2, VA.emulate(cs, 2, WINDOW, F32, "momentum")["out"]).fails


@pytest.mark.parametrize("cs", CASES, ids=repr)
def test_skip_cap_from_the_fp64_reference(cs):
    st = [VA.emulate(cs, n, WINDOW, F64) for n in (1, 2)]
    live = cs.live()
    zero = torch.zeros_like(st[0]["tprev"])
    for rb, tp in ((st[0]["tprev"], zero), (st[1]["tprev"], st[0]["tprev"])):
        rb, tp = torch.where(live[:, :, None, None], rb, zero), torch.where(live[:, :, None, None], tp, zero)
        mod = VA.stage_phase(rb, tp, cs.mom)[1]
        share = int((VA.skip_mask(mod, live) & live[:, :, None]).sum()) / (int(live.sum()) * 513)
        assert share <= VA.SKIP_CAP, share


def fault_cases(fault):
    if fault == "sqrt":
        return [cs for cs in SMALL if cs.power != 2.0]
    if fault == "momentum":
        return [cs for cs in SMALL if cs.momentum > 0]
    return [cs for cs in SMALL if cs.power == 2.0]


@pytest.mark.parametrize("fault", [f for f, s in VA.GL_FAULTS.items() if s is not None])
def test_seeded_fault_is_caught_by_its_stage(fault):
    for cs in fault_cases(fault):
        rep = VA.audit(cs, [VA.emulate(cs, n, WINDOW, F32, fault) for n in range(3)], WINDOW)
        # (the skip cap is a property of the case's data, not a bar: a broken overlap-add at hop 512 blows up the signal it judges)
        bars = {s for s, what in rep.fails if "skipped" not in what}
        assert bars == {VA.GL_FAULTS[fault]}, (fault, cs, rep.fails)


@pytest.mark.parametrize("fault", ["dc_imag", "nyquist_imag"])
def test_dc_and_nyquist_imaginary_parts_cannot_reach_the_frames(fault):
    """The imaginary parts of the DC and Nyquist bins, kept in the Hermitian extension, add only to the imaginary part of the complex
    inverse transform: the real frames k_gl_istft writes do not depend on whether the kernel drops them.  No bar can catch that
    fault, and none has to."""
    cs = CASES[0]
    mag = VA.stage_mag(cs.spec, cs.power) + 1.0
    ang = torch.view_as_real(cs.a0.transpose(1, 2).contiguous())
    assert float(ang[..., 0, 1].abs().max()) > 0 and float(ang[..., 512, 1].abs().max()) > 0
    ref, kept = VA.stage_istft(mag, ang, WINDOW), VA.stage_istft(mag, ang, WINDOW, fault=fault)
    assert float((ref - kept).abs().max()) <= 1e-13 * float(ref.abs().max())  # two fp64 transforms: 2^-29 of an fp32 ulp


# ------------------------------------------------------------------------------------------------ inverse mel scale
@pytest.mark.parametrize("M,NF", VA.MEL_SHAPES)
@pytest.mark.parametrize("mode", VA.MEL_MODES, ids=str)
def test_inverse_mel_fp32_restatement_meets_the_contract(M, NF, mode):
    inv = VA.inv_module(M, NF)
    lin, mel_n, mean, std = VA.mel_inputs(M, 4, 33, 100 * M + NF)
    rep = VA.Report(f"{M}x{NF} {mode}")
    for b, Tb in enumerate(VA.MEL_RAGGED):
        row = (lin[b, :, :Tb], mel_n[b, :Tb], mean[b], std[b])
        op32, _ = VA.mel_operand(mode, *row, dtype=F32)
        got = torch.relu(inv.pinv @ op32)
        op64, e_lin = VA.mel_operand(mode, *row)
        ref, bar = VA.mel_contract(inv.pinv, op64, e_lin)
        rep.bound("contract", (got.double() - ref).abs(), bar, f"row {b}")
    print(rep.line())
    assert not rep.fails, rep.fails


@pytest.mark.parametrize("kh,kw", VA.SMOOTHS)
def test_box_filter_count_fault_is_caught(kh, kw):
    """A box filter that divides by the in-range count instead of kh kw, through the contract bar of every shape's edge rows."""
    for M in (3, 80):
        inv = VA.inv_module(M, 513)
        lin, mel_n, mean, std = VA.mel_inputs(M, 4, 33, 7)
        for b, Tb in enumerate(VA.MEL_RAGGED):
            row = (lin[b, :, :Tb], mel_n[b, :Tb], mean[b], std[b])
            bad = torch.relu(inv.pinv @ VA.box(row[0], kh, kw, fault="count"))
            rep = VA.Report("count")
            op64, e_lin = VA.mel_operand((kh, kw), *row)
            ref, bar = VA.mel_contract(inv.pinv, op64, e_lin)
            rep.bound("contract", (bad.double() - ref).abs(), bar, "count")
            assert rep.fails, (M, Tb)


def test_box_is_avg_pool_of_the_rows_own_slice():
    lin = VA.mel_inputs(3, 1, 5, 1)[0][0].double()
    got = VA.box(lin[:, :2], 9, 9)
    want = torch.stack([torch.stack([lin[:, :2].sum() / 81 for _ in range(2)]) for _ in range(3)])
    assert torch.allclose(got, want, rtol=1e-14, atol=0)
