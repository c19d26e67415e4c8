"""Audio front-end timing: MelSpectrogram.stats and resample 22050 -> 16000 against the torch-on-GPU path
(what torchaudio does on the device: torch.stft -> abs()**2 -> matmul(fb) -> log(clamp) -> mean / std; F.conv1d with the same sinc
table at stride orig), at B = 64 x 10 s and B = 1 x 5 s.  Medians of N alternated calls, each timed with device events.
Writes profiles/r05_audio_time.json (or the path given as the first argument)."""
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "edge-diffusion-tts_amd"), REPO]
from edge_diffusion_tts_amd import MelSpectrogram, resample  # noqa: E402
from edge_diffusion_tts_amd.audio import sinc_resample_kernel  # noqa: E402

N = 25
DEV = "cuda"


def timed(fns):
    """Alternate the callables N times (after 3 warm-ups), event-timing each call; medians in microseconds."""
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(N):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) * 1000.0)
    return [sorted(t)[len(t) // 2] for t in ts]


def main(out_path):
    torch.manual_seed(0)
    mel = MelSpectrogram(16000, n_fft=1024, win_length=1024, hop_length=160, f_min=0, f_max=8000, n_mels=80).to(DEV)
    win = torch.hann_window(1024, device=DEV)
    fb = mel.fb

    def torch_stats(w):
        spec = torch.stft(w, 1024, 160, 1024, window=win, center=True, pad_mode="reflect", return_complex=True)
        m = torch.matmul((spec.abs() ** 2).transpose(-1, -2), fb)
        lm = torch.log(torch.clamp(m, min=1e-5))
        return lm.mean(dim=1, keepdim=True), lm.std(dim=1, keepdim=True).clamp_min(1e-5)

    h, width = sinc_resample_kernel(441, 320, 6, 0.99, torch.float32)
    h = h.to(DEV)[:, None, :]

    def torch_resample(x):
        L = x.shape[1]
        xp = torch.nn.functional.pad(x, (width, width + 441))
        y = torch.nn.functional.conv1d(xp[:, None], h, stride=441).transpose(1, 2).reshape(x.shape[0], -1)
        return y[:, :-(-320 * L // 441)]

    res = {"calls": N, "unit": "us (median of alternated, event-timed calls)"}
    for name, B, secs in (("large", 64, 10), ("small", 1, 5)):
        w16 = (0.1 * torch.randn(B, 16000 * secs, device=DEV))
        ours, ref = timed([lambda: mel.stats(w16), lambda: torch_stats(w16)])
        m0, s0 = mel.stats(w16)
        m1, s1 = torch_stats(w16)
        frames = B * (16000 * secs // 160 + 1)
        res[f"mel_stats_{name}"] = {"B": B, "seconds": secs, "frames": frames, "ours_us": ours, "torch_us": ref, "speedup": ref / ours,
                                    "max_abs_mean_vs_torch": float((m0 - m1).abs().max()), "max_abs_std_vs_torch": float((s0 - s1).abs().max())}
        lm_us, = timed([lambda: mel.log_mel(w16)])
        res[f"log_mel_{name}_us"] = lm_us
        w22 = (0.1 * torch.randn(B, 22050 * secs, device=DEV))
        ours, ref = timed([lambda: resample(w22, 22050, 16000), lambda: torch_resample(w22)])
        n_out = B * (-(-320 * 22050 * secs // 441))
        flop = n_out * 2 * 459  # one 459-tap dot product per output sample
        bound_us = flop / 157.3e12 * 1e6
        err = float((resample(w22, 22050, 16000) - torch_resample(w22)).abs().max())
        res[f"resample_{name}"] = {"B": B, "seconds": secs, "outputs": n_out, "ours_us": ours, "torch_us": ref, "speedup": ref / ours,
                                   "gflop": flop / 1e9, "fp32_mfma_bound_us": bound_us, "fraction_of_bound": bound_us / ours,
                                   "max_abs_vs_torch_conv1d": err}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "r05_audio_time.json"))
