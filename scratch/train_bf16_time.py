#!/usr/bin/env python3
"""One training step's decoder part on EdgeDiffusionDecoder(kernels="generic", autograd=True) with matmul_dtype="bf16" against the
same decoder with matmul_dtype="f32", same GPU, same build: scratch/train_time.py's protocol (its step, warm-up, medians of hipEvent
times, each variant timed first once and second once).  DESIGN.md section 26.

    python scratch/train_bf16_time.py [--out profiles/train_bf16_time.json] [--reps 20] [--shapes 8x173x100,64x512x256] [--one-step bf16|f32]
                                      [--variants f32,bf16]

--one-step runs warmed steps of one variant and nothing else (the process to put under a kernel trace).
--variants f32 times the fp32 step alone, twice (what a library without the option can run: EDTTS_LIB=<the parent commit's build>)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_time import DEV, make_step, timed  # noqa: E402  (it puts the package on sys.path)
from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, synth_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="8x173x100,64x512x256")
    ap.add_argument("--one-step", default=None, choices=("bf16", "f32"))
    ap.add_argument("--variants", default="f32,bf16")
    a = ap.parse_args()
    cfg = CFG(device=DEV, dropout=0.0)
    sch = DiffusionSchedule(cfg.diff_steps).to(DEV)
    decs = {}
    variants = a.variants.split(",")
    for md in variants:
        d = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, matmul_dtype=md)
        d.load_state_dict(synth_state_dict(cfg, 0))
        decs[md] = d.to(DEV).train()
    results = []
    for shape in a.shapes.split(","):
        B, T, S = (int(v) for v in shape.split("x"))
        steps = {md: make_step(d, sch, cfg, B, T, S, True) for md, d in decs.items()}
        if a.one_step:
            for _ in range(a.warmup):
                steps[a.one_step]()
            torch.cuda.synchronize()
            print(f"one {a.one_step} step at {shape}: loss {float(steps[a.one_step]()):.4f}")
            torch.cuda.synchronize()
            continue
        for s in steps.values():
            for _ in range(a.warmup):
                s()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for order in (variants[::-1], variants):
            for k in order:
                ms[k].append(statistics.median(timed(steps[k], a.reps)))
        r = dict(B=B, T=T, S=S, context="features")
        for k in variants:
            r[k + "_ms_by_order"], r[k + "_ms"] = ms[k], statistics.median(ms[k])
        if len(variants) == 2:
            r["bf16_over_f32"] = r["bf16_ms"] / r["f32_ms"]
        print(json.dumps(r))
        results.append(r)
    if a.out and results:
        with open(a.out, "w") as f:
            json.dump(dict(model="hidden 160, heads 4, n_mels 80, layers 4, window 64; storage fp32, matmul_dtype f32 / bf16",
                           device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
