"""The ragged vocoder on the GPU: InverseMelScale / GriffinLim with per-utterance frame counts, the box filter
fused into the inverse mel scale, and MelVocoder.from_linear.  Row b of a ragged call is bitwise the call on that row alone, nothing
past a row's length is read (the padding holds 1e6), and the outputs past it are exact zeros.

Geometry: CFG() (n_fft 1024, hop 160, 80 mels, 513 bins); B = 4 rows padded to 40 frames with 40 (full), 17 (off the 16-frame tile of
k_mel_to_spec), 5 (the shortest legal row: 160 * 4 = 640 > 512, reflect padding and overlap-add edges touch) and 33 (one past a tile
boundary) frames.  Run on the GPU box: python -m pytest tests -m gpu."""
import pytest
import torch
import torch.nn.functional as F

from conftest import max_abs
from edge_diffusion_tts_amd import CFG, GriffinLim, InverseMelScale, MelVocoder, native
from oracle import edtts_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, TMAX, LENS, SEEDS = 4, 40, [40, 17, 5, 33], [5, 6, 7, 8]
HOP, NFFT, BINS, MELS = 160, 1024, 513, 80
GARBAGE = 1e6


def pad_garbage(x, lens):
    """x [B, ., T] (real or complex) with everything at or past lens[b] replaced by large finite garbage."""
    x = x.clone()
    for b, n in enumerate(lens):
        x[b, :, n:] = GARBAGE
    return x


@pytest.fixture(scope="module")
def data():
    """Seeded inputs, built once on the CPU and never modified: linear mels, their least-squares spectrogram, initial phases."""
    g = torch.Generator().manual_seed(17)
    lin = torch.exp(1.5 * torch.randn(B, MELS, TMAX, generator=g).clamp(-3, 3) - 5.0)
    fb = O.melscale_fbanks(BINS, 0.0, 8000.0, MELS, 16000)
    spec = O.inverse_mel_scale(lin, fb)
    a0 = torch.complex(torch.rand(B, BINS, TMAX, generator=g), torch.rand(B, BINS, TMAX, generator=g))
    return {"lin": lin, "fb": fb, "spec": spec, "a0": a0, "lens": torch.tensor(LENS, dtype=torch.int64)}


def make_gl(n_iter):
    cfg = CFG(device=DEV)
    return GriffinLim(n_fft=cfg.n_fft, n_iter=n_iter, win_length=cfg.win_length, hop_length=cfg.hop_length, power=2.0).to(DEV)


def make_inv():
    return InverseMelScale(n_stft=BINS, n_mels=MELS, sample_rate=16000, f_min=0.0, f_max=8000.0).to(DEV)


def check_rows(wave, wave_lengths, lens, solo):
    """Row b: bitwise solo(b) in its first hop (T_b - 1) samples, exact zeros behind; the returned lengths."""
    assert wave.shape == (len(lens), HOP * (TMAX - 1))
    assert wave_lengths.tolist() == [HOP * (n - 1) for n in lens]
    for b, n in enumerate(lens):
        want = solo(b, n)
        assert want.shape == (1, HOP * (n - 1))
        assert torch.equal(wave[b, :HOP * (n - 1)], want[0]), f"row {b} ({n} frames) differs from its solo call"
        assert not bool(wave[b, HOP * (n - 1):].any()), f"row {b}: samples past its length are not zero"


@pytest.mark.parametrize("n_iter", [0, 2, 32])
def test_griffin_lim_ragged_injected_phases(data, n_iter):
    gl = make_gl(n_iter)
    spec, a0 = data["spec"].to(DEV), data["a0"].to(DEV)
    wave, wl = gl(pad_garbage(spec, LENS), angles0=pad_garbage(a0, LENS), lengths=data["lens"])
    assert bool(torch.isfinite(wave).all())
    check_rows(wave, wl, LENS, lambda b, n: gl(spec[b:b + 1, :, :n].contiguous(), angles0=a0[b:b + 1, :, :n].contiguous()))


def test_griffin_lim_ragged_library_phases(data):
    gl = make_gl(32)
    spec = data["spec"].to(DEV)
    padded = pad_garbage(spec, LENS)
    wave, wl = gl(padded, lengths=data["lens"], seeds=SEEDS)
    check_rows(wave, wl, LENS, lambda b, n: gl(spec[b:b + 1, :, :n].contiguous(), seed=SEEDS[b]))
    again, _ = gl(padded, lengths=data["lens"], seeds=torch.tensor(SEEDS, dtype=torch.int64))
    assert torch.equal(wave, again)
    other, _ = gl(padded, lengths=data["lens"], seeds=[9, 6, 7, 8])
    assert not torch.equal(other[0], wave[0]) and torch.equal(other[1:], wave[1:])


def test_griffin_lim_ragged_order_independence(data):
    gl = make_gl(2)
    spec = pad_garbage(data["spec"].to(DEV), LENS)
    wave, wl = gl(spec, lengths=data["lens"], seeds=SEEDS)
    perm = [2, 0, 3, 1]
    wave_p, wl_p = gl(spec[perm].contiguous(), lengths=data["lens"][perm], seeds=[SEEDS[i] for i in perm])
    assert torch.equal(wave_p, wave[perm]) and torch.equal(wl_p, wl[perm])


def test_griffin_lim_full_lengths_shared_seed(data):
    """lengths = [Tmax] * B with one shared seed: each row equals its solo call with that seed.  Not compared against the batch call
    without lengths: that one hashes the element index of the whole batch ((b * 513 + f) * T + t), this one the row's own (f * T + t),
    so their draws differ by design for b > 0."""
    gl = make_gl(2)
    spec = data["spec"].to(DEV)
    full = [TMAX] * B
    wave, wl = gl(spec, lengths=torch.tensor(full, dtype=torch.int64), seed=11)
    check_rows(wave, wl, full, lambda b, n: gl(spec[b:b + 1].contiguous(), seed=11))


def test_inverse_mel_ragged_unsmoothed(data):
    inv = make_inv()
    lin = data["lin"].to(DEV)
    got = inv(pad_garbage(lin, LENS), lengths=data["lens"])
    assert got.shape == (B, BINS, TMAX)
    for b, n in enumerate(LENS):
        assert torch.equal(got[b, :, :n], inv(lin[b:b + 1, :, :n].contiguous())[0])
        assert not bool(got[b, :, n:].any())
    # the normalised entry takes lengths too
    mel_n = torch.log(lin).transpose(1, 2).contiguous()
    mean, std = torch.zeros(B, 1, MELS, device=DEV), torch.ones(B, 1, MELS, device=DEV)
    fused = inv.from_normalized(pad_garbage(mel_n.transpose(1, 2), LENS).transpose(1, 2).contiguous(), mean, std, lengths=data["lens"])
    for b, n in enumerate(LENS):
        assert torch.equal(fused[b, :, :n], inv.from_normalized(mel_n[b:b + 1, :n].contiguous(), mean[b:b + 1], std[b:b + 1])[0])
        assert not bool(fused[b, :, n:].any())


def test_inverse_mel_smoothed_vs_reference(data):
    """Against the reference's own function on the CPU, per row: inverse_mel_scale(avg_pool2d(lin[b, :, :T_b], (5, 3), stride 1,
    padding (2, 1))).  Bound: the project's for this product (test_gpu_parity.py:test_inverse_mel_scale_vs_oracle), max-abs <
    2e-5 * scale + 1e-9; the box filter's 15 non-negative fp32 terms in another order add at most about 2 * 15 * 2^-24 = 2e-6 relative."""
    inv = make_inv()
    lin, fb = data["lin"], data["fb"]
    got = inv(pad_garbage(lin.to(DEV), LENS), lengths=data["lens"], smooth=(5, 3))
    for b, n in enumerate(LENS):
        pooled = F.avg_pool2d(lin[b:b + 1, None, :, :n], (5, 3), stride=1, padding=(2, 1))[:, 0]
        ref = O.inverse_mel_scale(pooled, fb)
        scale = float(ref.abs().max())
        err = max_abs(got[b:b + 1, :, :n].cpu(), ref)
        print(f"smoothed inverse mel row {b} ({n} frames): max-abs {err:.3e}, bound {2e-5 * scale + 1e-9:.3e}")
        assert err < 2e-5 * scale + 1e-9
        assert not bool(got[b, :, n:].any())
        # the edge is the row's own end: bitwise the solo smoothed call
        assert torch.equal(got[b, :, :n], inv(lin[b:b + 1, :, :n].contiguous().to(DEV), smooth=(5, 3))[0])
    # smooth without lengths is the rectangular batch; (1, 1) is the unsmoothed call
    rect = inv(lin.to(DEV), smooth=(5, 3)).cpu()
    ref = O.inverse_mel_scale(F.avg_pool2d(lin[:, None], (5, 3), stride=1, padding=(2, 1))[:, 0], fb)
    assert max_abs(rect, ref) < 2e-5 * float(ref.abs().max()) + 1e-9
    plain = inv(lin.to(DEV))
    one = inv(lin.to(DEV), smooth=(1, 1))
    assert max_abs(one, plain) < 2e-5 * float(plain.abs().max()) + 1e-9
    ref1 = O.inverse_mel_scale(lin, fb)
    assert max_abs(one.cpu(), ref1) < 2e-5 * float(ref1.abs().max()) + 1e-9


def test_mel_vocoder_from_linear(data):
    cfg = CFG(device=DEV)
    voc = MelVocoder(cfg, n_iter=32).to(DEV)
    lin, fb, a0 = data["lin"], data["fb"], data["a0"]
    mels = [lin[b, :, :n].contiguous().to(DEV) for b, n in enumerate(LENS)]
    waves = voc.from_linear(mels, n_iter=4, seeds=SEEDS)
    assert [tuple(w.shape) for w in waves] == [(HOP * (n - 1),) for n in LENS]
    assert voc.griffin_lim.n_iter == 32  # the override is per call
    for b in range(B):
        solo = voc.from_linear([mels[b]], n_iter=4, seeds=[SEEDS[b]])
        assert len(solo) == 1 and torch.equal(solo[0], waves[b])
    # end to end against the oracle pipeline with the same initial phases (the bar of test_mel_vocoder_end_to_end)
    angles = [a0[b, :, :n].contiguous().to(DEV) for b, n in enumerate(LENS)]
    got = voc.from_linear(mels, n_iter=4, angles0=angles)
    for b, n in enumerate(LENS):
        pooled = F.avg_pool2d(lin[b:b + 1, None, :, :n], (5, 3), stride=1, padding=(2, 1))[:, 0]
        ref = O.griffin_lim(O.inverse_mel_scale(pooled, fb), cfg.n_fft, cfg.hop_length, cfg.win_length, 4, angles0=a0[b:b + 1, :, :n])
        rel = float((got[b].cpu() - ref[0]).norm() / ref.norm())
        print(f"from_linear entry {b} ({n} frames) vs the oracle pipeline: relative L2 error {rel:.2e}")
        assert got[b].shape == ref[0].shape and rel < 1e-3, (b, rel)


def test_out_of_range_device_lengths_are_clamped_and_flagged(data):
    """Device-side lengths are not range-checked on the host: the kernels clamp them into [1, Tmax] and set EDTTS_IDX_LEN (nothing out
    of bounds is read: the spectrogram here has no padding at all past Tmax)."""
    gl, inv = make_gl(2), make_inv()
    spec, lin, a0 = data["spec"].to(DEV), data["lin"].to(DEV), data["a0"].to(DEV)
    assert native.index_errors(gl.idx_err) == 0 and native.index_errors(inv.idx_err) == 0
    bad = torch.tensor([TMAX + 7, 17, 0, 33], dtype=torch.int64, device=DEV)
    wave, wl = gl(spec, angles0=a0, lengths=bad)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(wave).all())
    assert native.index_errors(gl.idx_err) & native.EDTTS_IDX_LEN
    assert native.index_errors(gl.idx_err) == 0  # read and cleared
    ok, wl_ok = gl(spec, angles0=a0, lengths=torch.tensor([TMAX, 17, 33, 33], dtype=torch.int64))
    assert native.index_errors(gl.idx_err) == 0
    assert wl.tolist() == [HOP * (TMAX - 1), HOP * 16, 0, HOP * 32]
    assert torch.equal(wave[0], ok[0]) and torch.equal(wave[1], ok[1]) and torch.equal(wave[3], ok[3])
    assert not bool(wave[2].any())  # clamped to one frame: no samples
    # a row shorter than the reflect padding is in range for the clamp but flagged: its solo call would refuse it
    gl(spec, angles0=a0, lengths=torch.tensor([TMAX, 17, 4, 33], dtype=torch.int64, device=DEV))
    assert native.index_errors(gl.idx_err) & native.EDTTS_IDX_LEN
    out = inv(lin, lengths=bad)
    assert native.index_errors(inv.idx_err) & native.EDTTS_IDX_LEN
    want = inv(lin, lengths=torch.tensor([TMAX, 17, 1, 33], dtype=torch.int64))
    assert torch.equal(out, want) and native.index_errors(inv.idx_err) == 0
    old = native.CHECK_INDICES
    native.CHECK_INDICES = True
    try:
        with pytest.raises(IndexError, match="length"):
            inv(lin, lengths=bad)
    finally:
        native.CHECK_INDICES = old
