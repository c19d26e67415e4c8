"""Semantic head encode at B = 64, T = 500 HuBERT frames (10 s utterances), FSQ and VQ at the defaults: the HIP kernel
(edtts_sem_encode) against the torch eager composition of the reference's head on the same GPU, alternated, median of N calls.
Kernel-only times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.  DESIGN.md section 13."""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "edge-diffusion-tts_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from edge_diffusion_tts_amd import SemanticEncoder  # noqa: E402
from edge_diffusion_tts_amd.synth import synth_hubert_features, synth_semantic_head  # noqa: E402

B, T, N, WARM = 64, 500, int(os.environ.get("SEM_CALLS", "30")), 5


def torch_head(enc, h):
    """The reference's head as torch ops (models/encoder.py proj + FSQEncoder.forward / VectorQuantizer.forward, eval)."""
    p = enc.proj
    z = F.linear(F.layer_norm(F.gelu(F.linear(h, p[0].weight, p[0].bias)), (z_dim := p[0].out_features,), p[2].weight, p[2].bias),
                 p.final.weight, p.final.bias)
    q = enc.vq
    if hasattr(q, "fsq"):
        zb = torch.tanh(F.linear(z, q.proj_down.weight, q.proj_down.bias))
        half = (q.fsq._levels.float() - 1) / 2
        zq = torch.minimum(torch.clamp(torch.round((zb + 1) * half), min=0), q.fsq._levels.float() - 1) / half - 1
        zq = zb + (zq - zb)
        idx = (torch.round((zq + 1) * half).long() * q.fsq._basis).sum(-1)
        out = F.linear(zq, q.proj_up.weight, q.proj_up.bias)
        n = q.fsq.codebook_size
    else:
        flat = z.reshape(-1, z_dim)
        w = q.codebook.weight
        idx = (flat.pow(2).sum(1, keepdim=True) - 2 * flat @ w.t() + w.pow(2).sum(1, keepdim=True).t()).argmin(1)
        out = z + (w[idx].view_as(z) - z)
        idx = idx.view(z.shape[:-1])
        n = q.codebook_size
    counts = torch.bincount(idx.flatten(), minlength=n).float()
    probs = counts / counts.sum().clamp_min(1.0)
    return out, idx, torch.exp(-(probs * torch.log(probs.clamp_min(1e-12))).sum()), (counts > 0).sum()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


@torch.no_grad()
def main():
    h = synth_hubert_features(B, T, 768, 11).cuda()
    for kind, levels, K in (("fsq", [4, 4, 3, 3, 2, 2, 2, 2], 0), ("vq", None, 512)):
        proj_sd, q_sd = synth_semantic_head(768, 128, levels, K, seed=1)
        enc = SemanticEncoder.from_checkpoint({"encoder_proj": proj_sd, ("encoder_fsq" if levels else "encoder_vq"): q_sd}, device="cuda")
        hip = lambda: enc.quantize_features(h)  # noqa: E731
        ref = lambda: torch_head(enc, h)  # noqa: E731
        agree = float((hip()[1] == ref()[1]).float().mean())
        for _ in range(WARM):
            hip(), ref()
        th, tr = [], []
        for _ in range(N):
            th.append(timed(hip))
            tr.append(timed(ref))
        mh, mr = statistics.median(th), statistics.median(tr)
        flop = B * T * (2 * 768 * 128 + 2 * 128 * 128 + (4 * 128 * len(levels) if levels else 2 * 128 * K))
        print(f"{kind}: HIP encode + stats median {mh:.1f} us ({flop / mh / 1e6:.1f} TFLOP/s; fp32 MFMA bound {flop / 157.3e6:.1f} us), "
              f"torch eager {mr:.1f} us, speed-up {mr / mh:.2f}x; idx agreement with torch {agree:.5f}")


if __name__ == "__main__":
    main()
