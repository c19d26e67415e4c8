#!/usr/bin/env python3
"""One training step's decoder part on a ragged batch: padded without lengths against the same batch with per-utterance lengths
(EdgeDiffusionDecoder(kernels="generic", autograd=True, train_lengths=True)).

    python scratch/train_ragged_time.py [--out profiles/train_ragged_time.json] [--reps 20] [--shapes 64x512x256,8x173x100]
                                        [--one-step ragged|padded] [--kernel-stats FILE.csv --stat-steps N]

Protocol of scratch/train_time.py: default model (hidden 160, 4 heads, 80 mels, 4 layers, window 64), fp32, dropout off; per shape
5 warm-up steps, then the median of `reps` steps between hipEvents, each variant timed first once and second once.  Lengths: S_b
uniform in [S / 4, S] from a fixed seed, T_b = T S_b / S (B = 64, T = 512, S = 256: S_b in [64, 256], T_b = 2 S_b).  Both variants
compute the masked loss ((eps - target) mask)^2 .sum() / live elements; (a) "padded" passes no lengths, (b) "ragged" passes them.
--one-step runs warmed steps of one variant at the first shape and nothing else (the process to put under
`rocprofv3 --kernel-trace --stats`); --kernel-stats adds that run's per-kernel table (times divided by --stat-steps) to the output."""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "edge-diffusion-tts_amd"))
from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, synth_state_dict  # noqa: E402

DEV = "cuda"


def lengths_of(B, T, S):
    g = torch.Generator().manual_seed(1000 * B + S)
    s_len = torch.randint(max(1, S // 4), S + 1, (B,), generator=g)
    t_len = (s_len * T // S).clamp(min=1)
    return t_len, s_len


def make_step(dec, sch, cfg, B, T, S, t_len, s_len, ragged):
    g = torch.Generator().manual_seed(B + T)
    x0 = torch.randn(B, T, cfg.n_mels, generator=g).to(DEV)
    noise = torch.randn(B, T, cfg.n_mels, generator=g).to(DEV)
    feats = torch.randn(B, S, cfg.semantic_dim, generator=g).to(DEV)
    t = torch.randint(1, 1000, (B,), generator=g).to(DEV)
    si = torch.zeros(B, dtype=torch.long, device=DEV)
    tl, sl = t_len.to(DEV), s_len.to(DEV)  # device lengths: no host-to-device copy inside the step
    mask = (torch.arange(T, device=DEV)[None, :] < tl[:, None])[..., None].float()
    live = float(t_len.sum() * cfg.n_mels)

    def step():
        dec.zero_grad(set_to_none=True)
        x_t, _ = sch.q_sample(x0, t, noise)
        if ragged:
            v = dec(x_t, t, sem_features=feats, step_idx=si, x_lengths=tl, sem_lengths=sl)
        else:
            v = dec(x_t, t, sem_features=feats, step_idx=si)
        loss = (((v - sch.get_v_target(x0, noise, t)) * mask) ** 2).sum() / live
        loss.backward()
        return loss

    return step


def timed(step, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def kernel_stats(path, steps):
    """rocprofv3's *_kernel_stats.csv -> [{name, calls_per_step, ms_per_step, percent}], largest first."""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append(dict(name=r["Name"], calls_per_step=int(r["Calls"]) / steps, ms_per_step=float(r["TotalDurationNs"]) / steps / 1e6,
                             percent=float(r["Percentage"])))
    return sorted(rows, key=lambda r: -r["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="64x512x256,8x173x100")
    ap.add_argument("--one-step", default=None, choices=("ragged", "padded"))
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--stat-steps", type=int, default=1)
    a = ap.parse_args()
    cfg = CFG(device=DEV, dropout=0.0)
    sch = DiffusionSchedule(cfg.diff_steps).to(DEV)
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, train_lengths=True)
    dec.load_state_dict(synth_state_dict(cfg, 0))
    dec = dec.to(DEV).train()
    results = []
    for shape in a.shapes.split(","):
        B, T, S = (int(v) for v in shape.split("x"))
        t_len, s_len = lengths_of(B, T, S)
        steps = {k: make_step(dec, sch, cfg, B, T, S, t_len, s_len, k == "ragged") for k in ("padded", "ragged")}
        if a.one_step:
            for _ in range(a.warmup):
                steps[a.one_step]()
            torch.cuda.synchronize()
            print(f"one {a.one_step} step at {shape}: loss {float(steps[a.one_step]()):.4f}")
            torch.cuda.synchronize()
            return
        for s in steps.values():
            for _ in range(a.warmup):
                s()
        torch.cuda.synchronize()
        ms = {"padded": [], "ragged": []}
        for order in (("padded", "ragged"), ("ragged", "padded")):
            for k in order:
                ms[k].append(statistics.median(timed(steps[k], a.reps)))
        r = dict(B=B, T=T, S=S, live_frames=float(t_len.sum()) / (B * T), live_tokens=float(s_len.sum()) / (B * S),
                 padded_ms_by_order=ms["padded"], ragged_ms_by_order=ms["ragged"], padded_ms=statistics.median(ms["padded"]),
                 ragged_ms=statistics.median(ms["ragged"]))
        r["ragged_over_padded"] = r["ragged_ms"] / r["padded_ms"]
        print(json.dumps(r))
        results.append(r)
    if a.out and results:
        doc = dict(model="hidden 160, heads 4, n_mels 80, layers 4, window 64, fp32", device=torch.cuda.get_device_name(0), reps=a.reps,
                   warmup=a.warmup, lengths="S_b uniform in [S/4, S] (fixed seed), T_b = T S_b / S", results=results)
        if a.kernel_stats:
            doc["ragged_step_kernels"] = dict(shape=a.shapes.split(",")[0], steps_traced=a.stat_steps, kernels=kernel_stats(a.kernel_stats, a.stat_steps))
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
