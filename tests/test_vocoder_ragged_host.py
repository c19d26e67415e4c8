"""Host tests of the ragged vocoder (edge_diffusion_tts_amd/melpost.py): the new C symbols, the argument errors
raised before any launch, and the padding / unpadding of MelVocoder.from_linear with the two launches stubbed out.  No GPU."""
import os
import re

import pytest
import torch

from edge_diffusion_tts_amd import CFG, GriffinLim, InverseMelScale, MelVocoder, native
from edge_diffusion_tts_amd import melpost

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP, NFFT, BINS, MELS = 160, 1024, 513, 80


def make_inv():
    return InverseMelScale(n_stft=BINS, n_mels=MELS, sample_rate=16000, f_min=0.0, f_max=8000.0)


def make_gl(n_iter=2):
    return GriffinLim(n_fft=NFFT, n_iter=n_iter, win_length=NFFT, hop_length=HOP, power=2.0)


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "edtts.h")).read()
    sig = re.search(r"int edtts_griffin_lim_len\(([^;]*)\);", header).group(1)
    assert "const int64_t* t_len" in sig and "const uint64_t* seeds" in sig
    sig = re.search(r"int edtts_mel_to_spec_len\(([^;]*)\);", header).group(1)
    assert "const int64_t* t_len" in sig and "int smooth_h" in sig and "int smooth_w" in sig
    assert melpost.SMOOTH_MAX == 9
    kernels = open(os.path.join(REPO, "edge-diffusion-tts_amd", "csrc", "edtts_melpost.h")).read()
    assert re.search(r"kSmoothMax\s*=\s*9\b", kernels) and re.search(r"kSmoothMaxMels\s*=\s*256\b", kernels)


def test_library_rejects_bad_arguments():
    L = native.lib()
    p = 16  # any non-NULL pointer: the checks run before anything is launched
    with pytest.raises(native.EdttsError, match="odd"):
        L.edtts_mel_to_spec_len(p, None, None, p, 1, 8, 80, 513, None, 4, 3, None, p, None)
    with pytest.raises(native.EdttsError, match="odd"):
        L.edtts_mel_to_spec_len(p, None, None, p, 1, 8, 80, 513, None, 5, 0, None, p, None)
    with pytest.raises(native.EdttsError, match="odd"):
        L.edtts_mel_to_spec_len(p, None, None, p, 1, 8, 80, 513, None, 5, 11, None, p, None)
    with pytest.raises(native.EdttsError, match="linear"):
        L.edtts_mel_to_spec_len(p, p, p, p, 1, 8, 80, 513, None, 5, 3, None, p, None)
    with pytest.raises(native.EdttsError, match="n_mels <= 256"):
        L.edtts_mel_to_spec_len(p, None, None, p, 1, 8, 300, 513, None, 5, 3, None, p, None)
    with pytest.raises(native.EdttsError, match="NULL"):
        L.edtts_mel_to_spec_len(p, None, None, None, 1, 8, 80, 513, None, 0, 0, None, p, None)
    gl = (1, 40, 1024, 160, p, p, 2, 0.99, 2.0)
    with pytest.raises(native.EdttsError, match="t_len is NULL"):
        L.edtts_griffin_lim_len(p, *gl, p, None, None, None, p, p, None)
    with pytest.raises(native.EdttsError, match="seeds"):
        L.edtts_griffin_lim_len(p, *gl, None, p, None, None, p, p, None)
    with pytest.raises(native.EdttsError, match="reflect padding"):
        L.edtts_griffin_lim_len(p, 1, 4, 1024, 160, p, p, 2, 0.99, 2.0, p, p, None, None, p, p, None)
    with pytest.raises(native.EdttsError, match="n_fft=512"):
        L.edtts_griffin_lim_len(p, 1, 40, 512, 160, p, p, 2, 0.99, 2.0, p, p, None, None, p, p, None)


def test_inverse_mel_argument_errors():
    inv = make_inv()
    lin = torch.rand(3, MELS, 20)
    for bad in (torch.tensor([20, 5, 7], dtype=torch.int32), torch.tensor([20, 5], dtype=torch.int64), [20, 5, 7],
                torch.tensor([20, 0, 7], dtype=torch.int64), torch.tensor([21, 5, 7], dtype=torch.int64)):
        with pytest.raises(ValueError, match="lengths"):
            inv(lin, lengths=bad)
    for bad in ((4, 3), (5, 2), (5, 11), (0, 3), (5,), 5, (5.0, 3), (-1, 3)):
        with pytest.raises(ValueError, match="smooth"):
            inv(lin, smooth=bad)
    mel_n, stat = torch.zeros(3, 20, MELS), torch.zeros(3, 1, MELS)
    with pytest.raises(ValueError, match="smooth"):
        inv.from_normalized(mel_n, stat, stat + 1, smooth=(5, 3))
    with pytest.raises(ValueError, match="smooth"):
        inv._spec(mel_n, stat.reshape(3, MELS), stat.reshape(3, MELS), None, (5, 3))
    wide = InverseMelScale(n_stft=BINS, n_mels=300, sample_rate=16000)
    with pytest.raises(ValueError, match="n_mels <= 256"):
        wide(torch.rand(1, 300, 20), smooth=(5, 3))
    # valid arguments get as far as the launch, which has no CPU path
    with pytest.raises(native.EdttsError, match="HIP device"):
        inv(lin, lengths=torch.tensor([20, 5, 7], dtype=torch.int64), smooth=(5, 3))
    assert "idx_err" not in inv.state_dict() and "idx_err" not in make_gl().state_dict()


def test_griffin_lim_argument_errors():
    gl = make_gl()
    spec = torch.rand(3, BINS, 20)
    for bad in (torch.tensor([20, 5, 7], dtype=torch.int32), torch.tensor([20, 5], dtype=torch.int64), (20, 5, 7),
                torch.tensor([20, 0, 7], dtype=torch.int64), torch.tensor([21, 5, 7], dtype=torch.int64)):
        with pytest.raises(ValueError, match="lengths"):
            gl(spec, lengths=bad)
    # 4 frames = 480 samples, not longer than the reflect padding 512; 5 frames = 640 are
    with pytest.raises(ValueError, match="reflect padding"):
        gl(spec, lengths=torch.tensor([20, 4, 7], dtype=torch.int64))
    ok = torch.tensor([20, 5, 7], dtype=torch.int64)
    for bad in ([1, 2], [1, 2, 3, 4], torch.tensor([1, 2], dtype=torch.int64), torch.tensor([1, 2, 3], dtype=torch.int32)):
        with pytest.raises(ValueError, match="seeds"):
            gl(spec, lengths=ok, seeds=bad)
        with pytest.raises(ValueError, match="seeds"):
            gl(spec, lengths=ok, seeds=bad, angles0=torch.zeros(3, BINS, 20, dtype=torch.complex64))
    with pytest.raises(ValueError, match="seeds"):
        gl(spec, seeds=[1, 2, 3])  # per-row seeds come with lengths
    with pytest.raises(native.EdttsError, match="HIP device"):
        gl(spec, lengths=ok, seeds=[1, 2, 3])


class StubInverse(torch.nn.Module):
    """Stands in for InverseMelScale: records the call, returns a spectrogram that encodes (entry, frame)."""

    def __init__(self):
        super().__init__()
        self.n_mels, self.calls = MELS, []

    def forward(self, batch, *, lengths=None, smooth=None):
        self.calls.append((batch.clone(), lengths.clone(), smooth))
        N, _, T = batch.shape
        return batch[:, :1, :].expand(N, BINS, T).contiguous()


class StubGriffinLim(torch.nn.Module):
    """Stands in for GriffinLim: sample i of row n = 1000 n + i / hop inside the row's length, -1 behind it."""

    def __init__(self, n_iter):
        super().__init__()
        self.n_fft, self.hop, self.n_iter, self.calls = NFFT, HOP, n_iter, []

    def forward(self, spec, *, angles0=None, seed=0, lengths=None, seeds=None):
        self.calls.append({"n_iter": self.n_iter, "angles0": angles0, "lengths": lengths.clone(), "seeds": seeds, "spec": spec})
        N, _, T = spec.shape
        wave = torch.full((N, HOP * (T - 1)), -1.0)
        for n in range(N):
            k = HOP * (int(lengths[n]) - 1)
            wave[n, :k] = 1000.0 * float(spec[n, 0, 0]) + torch.arange(k) // HOP
        return wave, (lengths - 1) * HOP


def stub_vocoder(n_iter=32):
    voc = MelVocoder(CFG(), n_iter=n_iter)
    voc.inverse_mel, voc.griffin_lim = StubInverse(), StubGriffinLim(n_iter)
    return voc


def test_from_linear_pads_and_unpads_in_order():
    voc = stub_vocoder()
    frames = [12, 40, 5, 33]
    mels = [torch.full((MELS, t), float(n + 1)) for n, t in enumerate(frames)]
    waves = voc.from_linear(mels, n_iter=100, seeds=[3, 1, 4, 1])
    batch, lens, smooth = voc.inverse_mel.calls[0]
    assert len(voc.inverse_mel.calls) == len(voc.griffin_lim.calls) == 1  # one call each, whatever the list's length
    assert batch.shape == (4, MELS, 40) and lens.tolist() == frames and lens.dtype == torch.int64 and smooth == (5, 3)
    for n, t in enumerate(frames):
        assert torch.equal(batch[n, :, :t], mels[n]) and not bool(batch[n, :, t:].any())  # zero padding
    call = voc.griffin_lim.calls[0]
    assert call["n_iter"] == 100 and voc.griffin_lim.n_iter == 32  # the override holds for the call only
    assert call["lengths"].tolist() == frames and call["seeds"] == [3, 1, 4, 1] and call["angles0"] is None
    assert [tuple(w.shape) for w in waves] == [(HOP * (t - 1),) for t in frames]
    for n, (w, t) in enumerate(zip(waves, frames)):
        assert float(w[0]) == 1000.0 * (n + 1) and float(w[-1]) == 1000.0 * (n + 1) + t - 2 and float(w.min()) >= 0  # row n, unpadded
    # defaults: the constructor's n_iter, no seeds given, smooth=None passed through
    voc = stub_vocoder(n_iter=7)
    voc.from_linear(mels[:2], smooth=None)
    assert voc.griffin_lim.calls[0]["n_iter"] == 7 and voc.griffin_lim.calls[0]["seeds"] is None and voc.inverse_mel.calls[0][2] is None
    # injected phases are padded like the mels
    voc = stub_vocoder()
    a0 = [torch.full((BINS, t), complex(n + 1, -1.0), dtype=torch.complex64) for n, t in enumerate(frames)]
    voc.from_linear(mels, angles0=a0)
    got = voc.griffin_lim.calls[0]["angles0"]
    assert got.shape == (4, BINS, 40) and got.dtype == torch.complex64
    for n, t in enumerate(frames):
        assert torch.equal(got[n, :, :t], a0[n]) and not bool(got[n, :, t:].abs().any())
    # the override is undone when the launch raises
    voc = stub_vocoder()
    voc.griffin_lim = make_gl(32)
    with pytest.raises(native.EdttsError, match="HIP device"):
        voc.from_linear(mels, n_iter=100)
    assert voc.griffin_lim.n_iter == 32


def test_from_linear_argument_errors():
    voc = stub_vocoder()
    good = torch.rand(MELS, 20)
    with pytest.raises(ValueError, match="empty"):
        voc.from_linear([])
    for bad in (torch.rand(MELS + 1, 20), torch.rand(1, MELS, 20), torch.rand(20)):
        with pytest.raises(ValueError, match="entry 1"):
            voc.from_linear([good, bad])
    with pytest.raises(ValueError, match="entry 1.*reflect padding"):
        voc.from_linear([good, torch.rand(MELS, 4)])
    with pytest.raises(ValueError, match="seeds"):
        voc.from_linear([good, good], seeds=[1])
    with pytest.raises(ValueError, match="angles0"):
        voc.from_linear([good, good], angles0=[torch.zeros(BINS, 20, dtype=torch.complex64)])
    with pytest.raises(ValueError, match="angles0"):
        voc.from_linear([good], angles0=[torch.zeros(BINS, 19, dtype=torch.complex64)])
    assert not voc.inverse_mel.calls and not voc.griffin_lim.calls  # nothing was launched
    voc = MelVocoder(CFG())
    with pytest.raises(ValueError, match="smooth"):
        voc.from_linear([good], smooth=(4, 3))


def test_generate_long_docstring_points_at_from_linear():
    from edge_diffusion_tts_amd import InpaintSampler
    assert "MelVocoder.from_linear" in InpaintSampler.generate_long.__doc__
