"""GPU tests of the audio front end (csrc/edtts_audio.h): MelSpectrogram (power mel, log-mel, statistics, segment statistics) and
resample, against the fp64 restatements of tests/test_audio_host.py.

Parity bar (the HuBERT rule): max-abs error against the fp64 restatement is at most 4x the error of the same
restatement run in fp32 on the CPU (what torchaudio itself computes) against that fp64 run.  Invariances (batch rows, lengths,
segments, graphs, streams) are bitwise."""
import threading

import pytest
import torch

from edge_diffusion_tts_amd import (CFG, DiffusionSchedule, EdgeDiffusionDecoder, EdgeInference, InpaintSampler, MelSpectrogram,
                                    MelVocoder, Resample, SemanticEncoder, resample, synth_state_dict)
from edge_diffusion_tts_amd.melpost import normalize_mel
from edge_diffusion_tts_amd.synth import HubertStandIn, synth_semantic_head
from test_audio_host import GEOMETRY, ref_fb, ref_log_mel, ref_mel, ref_resample, ref_stats, signals

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 4.0
SR, HOP = 16000, 160


def mel_module():
    return MelSpectrogram(SR, n_fft=1024, win_length=1024, hop_length=HOP, f_min=0, f_max=8000, n_mels=80, power=2.0,
                          normalized=False).to(DEV)


def within_bar(got, ref64, ref32, what):
    """max|got - ref64| <= 4 max|ref32 - ref64| (plus one fp32 ulp of the scale, for cases where fp32 happens to be exact)."""
    got, ref64, ref32 = got.double().cpu(), ref64.double(), ref32.double()
    fin = torch.isfinite(ref64)
    assert torch.equal(fin, torch.isfinite(got)), what
    e = float((got - ref64)[fin].abs().max())
    e32 = float((ref32 - ref64)[fin].abs().max())
    floor = 1.2e-7 * float(ref64[fin].abs().max())
    assert e <= BAR * e32 + floor, f"{what}: max-abs {e:.3e} vs fp32 restatement {e32:.3e}"
    return e, e32


CASES = [(1, 8000), (3, 16000 + 77), (64, 2 * 16000 + 5)]


@pytest.mark.parametrize("B,L", CASES)
def test_mel_logmel_stats_parity(B, L):
    mel = mel_module()
    wav = signals(B, L, B)
    within_bar(mel(wav.to(DEV)), ref_mel(wav), ref_mel(wav, dtype=torch.float32), "power mel")
    lm64, lm32 = ref_log_mel(wav), ref_log_mel(wav, dtype=torch.float32)
    within_bar(mel.log_mel(wav.to(DEV)), lm64, lm32, "log-mel")
    mean, std = mel.stats(wav.to(DEV))
    (m64, s64), (m32, s32) = ref_stats(lm64), ref_stats(lm32)
    within_bar(mean, m64, m32, "mean")
    within_bar(std, s64, s32, "std")


def test_long_rows_and_near_silence():
    mel = mel_module()
    wav = torch.cat([signals(1, 160000, 5, "chirp"), signals(1, 160000, 6, "quiet"), signals(1, 160000, 7, "noise")])
    lm64 = ref_log_mel(wav)
    assert float((lm64[1] <= torch.log(torch.tensor(1e-5, dtype=torch.float64)) + 1e-12).double().mean()) > 0.5  # the clamp is active
    within_bar(mel.log_mel(wav.to(DEV)), lm64, ref_log_mel(wav, dtype=torch.float32), "log-mel 10 s")
    mean, std = mel.stats(wav.to(DEV))
    (m64, s64), (m32, s32) = ref_stats(lm64), ref_stats(ref_log_mel(wav, dtype=torch.float32))
    within_bar(mean, m64, m32, "mean 10 s")
    within_bar(std, s64, s32, "std 10 s")


def test_ragged_lengths_equal_solo_calls_bitwise():
    mel = mel_module()
    lens = [513, 8000, 16000 + 77, 1601, 24000]
    L = max(lens)
    wav = signals(len(lens), L, 9)
    dirty = wav.clone()
    for b, n in enumerate(lens):
        dirty[b, n:] = float("nan")
    ln = torch.tensor(lens, dtype=torch.int64)
    lm = mel.log_mel(dirty.to(DEV), ln)
    pw = mel(dirty.to(DEV), ln)
    mean, std = mel.stats(dirty.to(DEV), ln.to(DEV))
    for b, n in enumerate(lens):
        T = n // HOP + 1
        solo = wav[b:b + 1, :n].to(DEV)
        assert torch.equal(lm[b, :T], mel.log_mel(solo)[0]) and not lm[b, T:].any()
        assert torch.equal(pw[b, :, :T], mel(solo)[0]) and not pw[b, :, T:].any()
        sm, ss = mel.stats(solo)
        assert torch.equal(mean[b], sm[0]) and torch.equal(std[b], ss[0])
        # and the parity bar on the trimmed row
        within_bar(lm[b, :T], ref_log_mel(wav[b:b + 1, :n])[0], ref_log_mel(wav[b:b + 1, :n], dtype=torch.float32)[0], f"len {n}")


def test_batch_rows_equal_single_calls_bitwise():
    mel = mel_module()
    wav = signals(5, 12345, 2).to(DEV)
    lm, pw = mel.log_mel(wav), mel(wav)
    mean, std = mel.stats(wav)
    for b in range(5):
        assert torch.equal(lm[b], mel.log_mel(wav[b:b + 1])[0])
        assert torch.equal(pw[b], mel(wav[b:b + 1])[0])
        sm, ss = mel.stats(wav[b:b + 1])
        assert torch.equal(mean[b], sm[0]) and torch.equal(std[b], ss[0])
    y = resample(wav, 22050, 16000)
    for b in range(5):
        assert torch.equal(y[b], resample(wav[b:b + 1], 22050, 16000)[0])


def test_segment_stats_equal_stats_of_the_slice_bitwise():
    mel = mel_module()
    wav = signals(3, 60000, 4).to(DEV)
    segs = [(0, 0, 60000), (1, 24000, 56000), (2, 48000, 80000), (0, 100, 613), (1, 5000, 5600), (2, 333, 20000)]
    mean, std = mel.segment_stats(wav, [s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs])
    for i, (r, s, e) in enumerate(segs):
        piece = wav[r:r + 1, s:min(e, 60000)]
        sm, ss = mel.stats(piece)
        assert torch.equal(mean[i], sm[0]) and torch.equal(std[i], ss[0]), i
        m64, s64 = ref_stats(ref_log_mel(piece.cpu()))
        m32, s32 = ref_stats(ref_log_mel(piece.cpu(), dtype=torch.float32))
        within_bar(mean[i], m64[0], m32[0], f"segment {i} mean")
        within_bar(std[i], s64[0], s32[0], f"segment {i} std")
    # a one-frame segment (hop > its length) has NaN std, as torch.std of one value
    coarse = MelSpectrogram(SR, n_fft=1024, win_length=1024, hop_length=1024, f_min=0, f_max=8000, n_mels=80).to(DEV)
    m1, s1 = coarse.segment_stats(wav, [0], [1000], [1900])
    ref = ref_log_mel(wav[0:1, 1000:1900].cpu(), hop=1024)
    assert ref.shape[1] == 1 and torch.isnan(s1).all() and torch.isnan(ref.std(dim=1)).all()
    assert torch.equal(m1, coarse.stats(wav[0:1, 1000:1900])[0])


@pytest.mark.parametrize("orig", [22050, 24000, 44100, 48000, 8000])
def test_resample_parity(orig):
    B = 3
    x = signals(B, orig // 2 + 101, orig % 7, "mix")
    got = resample(x.to(DEV), orig, 16000)
    within_bar(got, ref_resample(x, orig, 16000), ref_resample(x, orig, 16000, dtype=torch.float32), f"resample {orig}")
    got_t = Resample(orig, 16000)(x.to(DEV))
    within_bar(got_t, ref_resample(x, orig, 16000), ref_resample(x, orig, 16000, dtype=torch.float32), f"Resample {orig}")


def test_resample_large_and_lengths_bitwise():
    lens = [1, 441, 22050 * 3 + 17, 100000, 22050 * 10]
    L = max(lens)
    x = signals(len(lens), L, 8)
    dirty = x.clone()
    for b, n in enumerate(lens):
        dirty[b, n:] = float("nan")
    y, yl = resample(dirty.to(DEV), 22050, 16000, lengths=torch.tensor(lens, dtype=torch.int64).to(DEV))
    assert y.shape == (len(lens), -(-16000 * L // 22050))
    for b, n in enumerate(lens):
        m = -(-16000 * n // 22050)
        assert int(yl[b]) == m
        solo = resample(x[b:b + 1, :n].to(DEV), 22050, 16000)
        assert torch.equal(y[b, :m], solo[0]) and not y[b, m:].any()
    within_bar(y[-1:], ref_resample(x[-1:], 22050, 16000), ref_resample(x[-1:], 22050, 16000, dtype=torch.float32), "resample 10 s")
    big = signals(64, 22050 * 2, 3).to(DEV)
    yb = resample(big, 22050, 16000)
    assert torch.equal(yb[17], resample(big[17:18], 22050, 16000)[0])


# ------------------------------------------------------------------------------------------------ paths no other test reaches
def test_magnitude_mel_parity():
    """power = 1.0: the sqrtf branch of mel_frame."""
    mel = MelSpectrogram(SR, n_fft=1024, win_length=1024, hop_length=HOP, f_min=0, f_max=8000, n_mels=80, power=1.0).to(DEV)
    wav = signals(2, 8000, 3)
    got = mel(wav.to(DEV))
    assert got.shape == (2, 80, 8000 // HOP + 1)
    within_bar(got, ref_mel(wav, power=1.0), ref_mel(wav, dtype=torch.float32, power=1.0), "magnitude mel")
    for call in (lambda: mel.log_mel(wav.to(DEV)), lambda: mel.stats(wav.to(DEV)), lambda: mel.segment_stats(wav.to(DEV), [0], [0], [8000])):
        with pytest.raises(NotImplementedError, match="power=2.0"):
            call()


@pytest.mark.parametrize("n_mels,sr,f_min,f_max", [(1, SR, 0.0, 8000.0), (64, SR, 0.0, 8000.0), (65, SR, 0.0, 8000.0), (128, SR, 0.0, 8000.0),
                                                  (100, 22050, 50.0, 7600.0)])
def test_mel_bin_counts(n_mels, sr, f_min, f_max):
    """The lane-ownership edges of mel_frame and k_mel_segstats: the second half-wave idle (1, 64), with one lane (65), full (128)."""
    mel = MelSpectrogram(sr, n_fft=1024, win_length=1024, hop_length=HOP, f_min=f_min, f_max=f_max, n_mels=n_mels).to(DEV)
    fb = ref_fb(n_mels, sr, f_min, f_max)
    assert torch.equal(mel.fb.cpu(), fb)
    wav = signals(2, 4000, n_mels)
    dev = wav.to(DEV)
    within_bar(mel(dev), ref_mel(wav, fb=fb), ref_mel(wav, dtype=torch.float32, fb=fb), "power mel")
    lm64, lm32 = ref_log_mel(wav, fb=fb), ref_log_mel(wav, dtype=torch.float32, fb=fb)
    within_bar(mel.log_mel(dev), lm64, lm32, "log-mel")
    mean, std = mel.stats(dev)
    (m64, s64), (m32, s32) = ref_stats(lm64), ref_stats(lm32)
    within_bar(mean, m64, m32, "mean")
    within_bar(std, s64, s32, "std")
    segs = [(0, 0, 4000), (1, 0, 4000), (1, 700, 3001), (0, 3000, 3513)]
    sm, ss = mel.segment_stats(dev, [s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs])
    assert sm.shape == ss.shape == (len(segs), 1, n_mels)
    # the fused kernel on a whole row is the two-kernel path bitwise (k_mel_segstats<1> == <0>); a slice is its own waveform
    assert torch.equal(sm[:2], mean) and torch.equal(ss[:2], std)
    refs = {torch.float64: [], torch.float32: []}
    for i, (r, s, e) in enumerate(segs):
        pm, ps = mel.stats(dev[r:r + 1, s:e])
        assert torch.equal(sm[i], pm[0]) and torch.equal(ss[i], ps[0]), i
        for dt in refs:
            refs[dt].append(ref_stats(ref_log_mel(wav[r:r + 1, s:e], dtype=dt, fb=fb)))
    # one bar per output of the call, as for every other output here: with n_mels = 1 a segment's statistics are ONE number each, and
    # the fp32 restatement's error on one number is anywhere between 0 and its typical size (a 4-frame segment of a steady tone has a
    # std of 1e-4 on log-mels of 7.5, whose fp32 storage alone moves it by 2e-7: the restatement gave 2e-7 on one CPU, 6e-9 on another)
    for k, what in enumerate(("segment means", "segment stds")):
        within_bar(sm if k == 0 else ss, torch.cat([m[k] for m in refs[torch.float64]]), torch.cat([m[k] for m in refs[torch.float32]]), what)


@pytest.mark.parametrize("hop,L", [(1, 513), (100, 513), (256, 513), (441, 513), (512, 513), (1024, 513),
                                   (100, 2049), (256, 2049), (441, 2049), (512, 2049), (1024, 2049)])
def test_hops(hop, L):
    mel = MelSpectrogram(SR, n_fft=1024, win_length=1024, hop_length=hop, f_min=0, f_max=8000, n_mels=80).to(DEV)
    wav = signals(3, L, hop % 5)
    T = L // hop + 1
    lm64, lm32 = ref_log_mel(wav, hop), ref_log_mel(wav, hop, torch.float32)
    lm = mel.log_mel(wav.to(DEV))
    assert lm.shape == lm64.shape == (3, T, 80)
    within_bar(lm, lm64, lm32, "log-mel")
    mean, std = mel.stats(wav.to(DEV))
    (m64, s64), (m32, s32) = ref_stats(lm64), ref_stats(lm32)
    within_bar(mean, m64, m32, "mean")
    if T > 1:
        within_bar(std, s64, s32, "std")
    else:  # one frame: torch.std of one value
        assert torch.isnan(std).all() and torch.isnan(s64).all()
    # a ragged batch with NaN behind each row's length against the solo calls
    lens = [L, 513, (L + 513) // 2]
    dirty = wav.clone()
    for b, n in enumerate(lens):
        dirty[b, n:] = float("nan")
    ln = torch.tensor(lens, dtype=torch.int64)
    rl, (rm, rs) = mel.log_mel(dirty.to(DEV), ln), mel.stats(dirty.to(DEV), ln)
    for b, n in enumerate(lens):
        Tb = n // hop + 1
        solo = wav[b:b + 1, :n].to(DEV)
        assert torch.equal(rl[b, :Tb], mel.log_mel(solo)[0]) and not rl[b, Tb:].any()
        sm, ss = mel.stats(solo)
        assert torch.equal(rm[b], sm[0])
        assert torch.equal(rs[b], ss[0]) if Tb > 1 else bool(torch.isnan(rs[b]).all() and torch.isnan(ss).all())


@pytest.mark.parametrize("orig,new", [r for r in GEOMETRY if r[1] != 16000 or r[0] == 11025])
def test_resample_launch_geometries(orig, new):
    """The grids test_audio_host.py's GEOMETRY lists: upsampling with 7 grid rows of one-tile groups, five-tile groups with a second
    grid row, the K padding with and without a remainder.  Parity for both entry points; ragged rows against their solo calls."""
    L = 3001
    x = signals(2, L, orig % 11)
    r64, r32 = ref_resample(x, orig, new), ref_resample(x, orig, new, dtype=torch.float32)
    within_bar(resample(x.to(DEV), orig, new), r64, r32, f"resample {orig}->{new}")
    within_bar(Resample(orig, new)(x.to(DEV)), r64, r32, f"Resample {orig}->{new}")
    for lens in ([1, 2500], [L, 2]):
        dirty = x.clone()
        for b, n in enumerate(lens):
            dirty[b, n:] = float("nan")
        y, yl = resample(dirty.to(DEV), orig, new, lengths=torch.tensor(lens, dtype=torch.int64).to(DEV))
        assert y.shape == (2, -(-new * L // orig))
        for b, n in enumerate(lens):
            m = -(-new * n // orig)
            assert int(yl[b]) == m
            solo = resample(x[b:b + 1, :n].to(DEV), orig, new)
            assert torch.equal(y[b, :m], solo[0]) and not y[b, m:].any(), (lens, b)
            within_bar(y[b:b + 1, :m], ref_resample(x[b:b + 1, :n], orig, new), ref_resample(x[b:b + 1, :n], orig, new, dtype=torch.float32),
                       f"{orig}->{new} len {n}")


def test_graph_capture_replays_the_eager_result():
    mel = mel_module()
    wav = signals(4, 30000, 1).to(DEV)
    ln = torch.tensor([30000, 20000, 513, 12345], dtype=torch.int64, device=DEV)
    rows = torch.tensor([0, 1, 3], dtype=torch.int64, device=DEV)
    st = torch.tensor([0, 5000, 100], dtype=torch.int64, device=DEV)
    en = torch.tensor([30000, 15000, 9000], dtype=torch.int64, device=DEV)
    eager = (mel.log_mel(wav, ln), *mel.stats(wav, ln), *mel.segment_stats(wav, rows, st, en, lengths=ln),
             resample(wav, 22050, 16000, lengths=ln)[0], mel(wav))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up (tables to the device) off the capture
        resample(wav, 22050, 16000, lengths=ln)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = (mel.log_mel(wav, ln), *mel.stats(wav, ln), *mel.segment_stats(wav, rows, st, en, lengths=ln),
               resample(wav, 22050, 16000, lengths=ln)[0], mel(wav))
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)
    del g


def test_two_streams_equal_sequential_calls():
    mel = mel_module()
    wavs = [signals(8, 40000, k).to(DEV) for k in (1, 2)]
    seq = [(mel.log_mel(w), *mel.stats(w), resample(w, 22050, 16000)) for w in wavs]
    torch.cuda.synchronize()
    res = [None, None]

    def run(i):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            for _ in range(3):
                res[i] = (mel.log_mel(wavs[i]), *mel.stats(wavs[i]), resample(wavs[i], 22050, 16000))
        s.synchronize()

    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for a, b in zip(seq, res):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ end to end, no torchaudio
def semantic_encoder(cfg):
    proj_sd, q_sd = synth_semantic_head(768, cfg.semantic_dim, None, cfg.codebook_size, 0, False)
    return SemanticEncoder.from_checkpoint({"encoder_proj": proj_sd, "encoder_vq": q_sd}, hubert=HubertStandIn(768, 0), device=DEV)


def decoder(cfg):
    dec = EdgeDiffusionDecoder(cfg)
    dec.load_state_dict(synth_state_dict(cfg, 0, max_pos=dec.max_len, max_ctx_pos=dec.max_context_len))
    return dec.to(DEV).eval()


def test_short_form_end_to_end():
    """generate_sample.py:75-145 on this package: 22.05 kHz ragged batch -> resample -> semantic tokens -> generate -> stats -> vocoder."""
    cfg = CFG(device=DEV)
    lens22 = torch.tensor([22050 * 2, 30000, 22050], dtype=torch.int64)
    wav22 = signals(3, int(lens22.max()), 12).to(DEV)
    wav16, lens16 = resample(wav22, 22050, cfg.sample_rate, lengths=lens22.to(DEV))
    assert wav16.shape[1] == -(-16000 * int(lens22.max()) // 22050)
    assert lens16.tolist() == [-(-16000 * int(n) // 22050) for n in lens22]
    infer = EdgeInference(cfg, DiffusionSchedule(cfg.diff_steps).to(DEV), semantic_encoder(cfg), decoder(cfg))
    mel_n = infer.generate_from_audio(wav16, num_steps=4)
    mel = MelSpectrogram(cfg.sample_rate, n_fft=cfg.n_fft, win_length=cfg.win_length, hop_length=cfg.hop_length, f_min=cfg.f_min,
                         f_max=cfg.f_max, n_mels=cfg.n_mels).to(DEV)
    mean, std = mel.stats(wav16, lens16)
    lm = mel.log_mel(wav16, lens16)
    for b in range(3):
        T = int(lens16[b]) // cfg.hop_length + 1
        _, m_ref, s_ref = normalize_mel(lm[b:b + 1, :T])
        assert float(((mean[b] - m_ref[0]).abs() / m_ref[0].abs().clamp_min(1e-3)).max()) <= 1e-5
        assert float(((std[b] - s_ref[0]).abs() / s_ref[0]).max()) <= 1e-5
    wave = MelVocoder(cfg, n_iter=4).to(DEV)(mel_n, mean, std)
    assert wave.shape == (3, cfg.hop_length * (mel_n.shape[1] - 1))
    assert torch.isfinite(wave).all()


def test_long_form_end_to_end():
    """inference_pipeline.py:206-367: per-chunk statistics from the audio feed generate_long_batch, three utterances."""
    cfg = CFG(device=DEV)
    smp = InpaintSampler(cfg, DiffusionSchedule(cfg.diff_steps).to(DEV), decoder(cfg))
    mel = MelSpectrogram(cfg.sample_rate, n_fft=1024, win_length=1024, hop_length=HOP, f_min=0, f_max=8000, n_mels=cfg.n_mels).to(DEV)
    totals = [20000, 41000, 9000]
    wavs = [resample(signals(1, -(-22050 * t // 16000), 20 + i).to(DEV), 22050, 16000)[0, :t] for i, t in enumerate(totals)]
    chunk, ov = 8000, 2000
    stats = smp.chunk_stats_from_audio(wavs, chunk, ov, mel)
    for w, st in zip(wavs, stats):
        n = max(1, -(-(w.numel() - ov) // (chunk - ov)))
        assert len(st) == n
        for i, (m, s) in enumerate(st):
            piece = w[i * (chunk - ov):i * (chunk - ov) + chunk][None]
            sm, ss = mel.stats(piece)
            assert torch.equal(m, sm) and torch.equal(s, ss)
    cf, of = chunk // HOP, ov // HOP
    g = torch.Generator().manual_seed(3)
    feats = [torch.randn(1, t // 320 + 1, cfg.semantic_dim, generator=g).to(DEV) for t in totals]
    frames = [t // HOP + 1 for t in totals]
    out = smp.generate_long_batch(feats, frames, cf, of, stats, seeds=[1, 2, 3], strength=0.6, steps=2, hop_length=HOP,
                                  sample_rate=cfg.sample_rate, chunk_samples=chunk, overlap_samples=ov, total_samples=totals)
    assert len(out) == 3
    for o, f in zip(out, frames):
        assert o.shape == (cfg.n_mels, f) and torch.isfinite(o).all()
