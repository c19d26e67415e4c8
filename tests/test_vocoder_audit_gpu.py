"""The vocoder (csrc/edtts_melpost.h) on the GPU, stage by stage against fp64 (tests/vocoder_audit_util.py):
the seven Griffin-Lim stages through the scratch of three calls with n_iter = 0, 1, 2, the returned waveform end to end, and both
inverse-mel kernels against their contract and against least squares.  hop in {160, 200, 256, 300, 512} x (power, momentum) in
{(2, 0.99), (1, 0), (3, 0.5)}, the entry point without lengths (B = 2, the smallest legal row) and the ragged one (B = 4, large
finite garbage behind every row's end).  Each test prints its worst error / bar per stage.
Run on the GPU box: python -m pytest tests/test_vocoder_audit_gpu.py -m gpu -s."""
import pytest
import torch

import vocoder_audit_util as VA
from edge_diffusion_tts_amd import GriffinLim, InverseMelScale, native

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = VA.gl_cases()


def gl_module(cs):
    return GriffinLim(n_fft=1024, n_iter=0, win_length=1024, hop_length=cs.hop, power=cs.power, momentum=cs.momentum).to(DEV)


def run(gl, spec, B, T, hop, n_iter, a0=None, seed=0, lens=None, seeds=None):
    """One native.griffin_lim call on a scratch of 0xFF bytes -> the scratch members and the returned waveform, on the CPU."""
    need = native.griffin_lim_scratch_floats(B, T, 1024, hop)
    scratch = torch.full((need + 16,), -1, dtype=torch.int32, device=DEV).view(torch.float32)
    t_len = None if lens is None else torch.tensor(lens, dtype=torch.int64).to(DEV)
    sd = None if seeds is None else torch.tensor(seeds, dtype=torch.int64).to(DEV)
    out = native.griffin_lim(spec, 1024, hop, gl.window, gl.twiddle, n_iter, gl.momentum, gl.power, a0, seed, t_len=t_len, seeds=sd,
                             idx_err=None if lens is None else gl.idx_err, scratch=scratch)
    torch.cuda.synchronize()
    assert lens is None or native.index_errors(gl.idx_err) == 0
    assert bool((scratch[need:].view(torch.int32) == -1).all()), "written past edtts_griffin_lim_scratch_floats"
    st = {k: v.cpu().clone() for k, v in native.griffin_lim_scratch_views(scratch, B, T, 1024, hop).items()}
    st["out"] = out.cpu()
    return st


def device_inputs(cs):
    spec, a0 = (cs.spec, cs.a0) if cs.lens is None else (VA.pad_garbage(cs.spec, cs.lens), VA.pad_garbage(cs.a0, cs.lens))
    return spec.to(DEV), torch.view_as_real(a0).contiguous().to(DEV)


@pytest.mark.parametrize("cs", CASES, ids=repr)
def test_griffin_lim_stage_by_stage(cs):
    gl = gl_module(cs)
    spec, a0 = device_inputs(cs)
    R = [run(gl, spec, cs.B, cs.T, cs.hop, n, a0, lens=cs.lens) for n in range(3)]
    window = gl.window.cpu()
    rep = VA.audit(cs, R, window)
    print("\n" + rep.line())
    # the module's own call is the call the audit looked into
    gl.n_iter = 2
    a0c = torch.view_as_complex(a0)
    got = gl(spec, angles0=a0c) if cs.lens is None else gl(spec, angles0=a0c, lengths=torch.tensor(cs.lens, dtype=torch.int64))[0]
    assert torch.equal(got.cpu(), R[2]["out"])
    assert not rep.fails, rep.fails


@pytest.mark.parametrize("cs", CASES, ids=repr)
def test_griffin_lim_end_to_end(cs):
    """The returned waveform for n_iter = 0, 1, 2 under the 4x rule against oracle.griffin_lim in fp64, the fp32 oracle the yardstick.
    The phase update divides by |a|: a bin of the rebuilt spectrum far below its row's level turns the transforms' absolute error into
    a phase error 1 / |a| times as large, which no stage bar sees.  With fp32 transforms two of these cases missed this bar (1.56 and
    2.37 of it, one bin each); k_gl_istft and k_gl_stft transform in fp64 since (worst figure now 0.56)."""
    gl = gl_module(cs)
    spec, a0 = device_inputs(cs)
    rep = VA.Report(repr(cs))
    for n in range(3):
        VA.end_to_end(cs, n, run(gl, spec, cs.B, cs.T, cs.hop, n, a0, lens=cs.lens)["out"], rep)
    print("\n" + rep.line())
    assert not rep.fails, rep.fails


@pytest.mark.parametrize("hop", list(VA.HOPS))
def test_library_drawn_phases(hop):
    """angles0 = None: both components of every draw lie in [0, 1), a ragged row's draws are its solo call's, tprev is 0 and the
    frames t >= T_b keep the fill."""
    cs = [c for c in CASES if c.hop == hop and c.lens is not None][0]
    gl = gl_module(cs)
    spec, _ = device_inputs(cs)
    seeds = [5, 6, 7, 8]
    st = run(gl, spec, cs.B, cs.T, hop, 0, lens=cs.lens, seeds=seeds)
    live = cs.live()
    ang = st["ang"]
    assert bool((ang[live] >= 0).all()) and bool((ang[live] < 1).all())
    assert bool(VA.is_fill(ang)[~live].all()) and not bool(st["tprev"][live].any())
    for b, Tb in enumerate(cs.lens):
        solo = run(gl, cs.spec[b:b + 1, :, :Tb].contiguous().to(DEV), 1, Tb, hop, 0, seed=seeds[b])
        assert torch.equal(solo["ang"][0], ang[b, :Tb]), b
        assert torch.equal(solo["out"][0], st["out"][b, :hop * (Tb - 1)]), b
    assert float(ang[live].std()) > 0.25  # uniform on [0, 1): 0.289


# ------------------------------------------------------------------------------------------------ inverse mel scale
_GPU_INV = {}


def gpu_inv(M, NF):
    if (M, NF) not in _GPU_INV:
        _GPU_INV[M, NF] = InverseMelScale(n_stft=NF, n_mels=M, sample_rate=16000, f_min=0.0, f_max=8000.0).to(DEV)
    return _GPU_INV[M, NF]


def call_inv(inv, mode, lin, mel_n, mean, std, lens=None):
    ln = None if lens is None else torch.tensor(lens, dtype=torch.int64)
    if lens is not None:
        lin = VA.pad_garbage(lin, lens)
        mel_n = VA.pad_garbage(mel_n.transpose(1, 2), lens).transpose(1, 2)
    if mode == "normalized":
        return inv.from_normalized(mel_n.contiguous().to(DEV), mean.to(DEV), std.to(DEV), lengths=ln).cpu()
    return inv(lin.to(DEV), lengths=ln, smooth=None if mode == "linear" else mode).cpu()


@pytest.mark.parametrize("M,NF", VA.MEL_SHAPES)
@pytest.mark.parametrize("mode", VA.MEL_MODES, ids=str)
def test_inverse_mel_contract_and_parity(M, NF, mode):
    cpu, inv = VA.inv_module(M, NF), gpu_inv(M, NF)
    assert torch.equal(inv.pinv.cpu(), cpu.pinv) and torch.equal(inv.fb.cpu(), cpu.fb)
    rep = VA.Report(f"inverse mel {M}x{NF} {mode}")
    for T in VA.MEL_T:  # the rectangular entry point
        inp = VA.mel_inputs(M, 2, T, 100 * M + NF + T)
        got = call_inv(inv, mode, *inp)
        assert got.shape == (2, NF, T)
        for b in range(2):
            VA.audit_mel(rep, got[b], mode, cpu.pinv, cpu.fb, (inp[0][b], inp[1][b], inp[2][b], inp[3][b]), f"T {T} row {b}")
    inp = VA.mel_inputs(M, 4, 33, 100 * M + NF)  # the ragged one
    got = call_inv(inv, mode, *inp, lens=VA.MEL_RAGGED)
    for b, Tb in enumerate(VA.MEL_RAGGED):
        VA.audit_mel(rep, got[b, :, :Tb], mode, cpu.pinv, cpu.fb, (inp[0][b, :, :Tb], inp[1][b, :Tb], inp[2][b], inp[3][b]),
                     f"ragged row {b} ({Tb} frames)")
        assert not bool(got[b, :, Tb:].any()), f"row {b}: frames past its length are not zero"
    print("\n" + rep.line())
    assert not rep.fails, rep.fails
