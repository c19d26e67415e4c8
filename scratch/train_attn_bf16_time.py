#!/usr/bin/env python3
"""One training step's decoder part on EdgeDiffusionDecoder(kernels="generic", autograd=True) for the four (matmul_dtype, attn_dtype)
combinations, same GPU, same build: scratch/train_time.py's protocol (its step, 5 warm-up steps, medians of 20 hipEvent times, each
variant timed once in ascending and once in descending order).  DESIGN.md section 27.

    python scratch/train_attn_bf16_time.py [--out profiles/train_attn_bf16_time.json] [--reps 20] [--shapes 8x173x100,64x512x256]
                                           [--variants f32/f32,bf16/f32,f32/bf16,bf16/bf16] [--one-step bf16/bf16]

A variant is matmul_dtype/attn_dtype.  --one-step runs warmed steps of one variant and nothing else (the process to put under a kernel
trace).  --variants f32/f32,bf16/f32 is what a library without the option can run (EDTTS_LIB=<the parent commit's build>)."""
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
    ap.add_argument("--one-step", default=None)
    ap.add_argument("--variants", default="f32/f32,bf16/f32,f32/bf16,bf16/bf16")
    ap.add_argument("--label", default="this build", help="which library the numbers belong to (written into --out)")
    a = ap.parse_args()
    cfg = CFG(device=DEV, dropout=0.0)
    sch = DiffusionSchedule(cfg.diff_steps).to(DEV)
    variants = [a.one_step] if a.one_step else a.variants.split(",")
    decs = {}
    for v in variants:
        md, ad = v.split("/")
        d = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, matmul_dtype=md, attn_dtype=ad)
        d.load_state_dict(synth_state_dict(cfg, 0))
        decs[v] = d.to(DEV).train()
    results = []
    for shape in a.shapes.split(","):
        B, T, S = (int(v) for v in shape.split("x"))
        steps = {v: make_step(d, sch, cfg, B, T, S, True) for v, d in decs.items()}
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
        for order in (variants, variants[::-1]):
            for k in order:
                ms[k].append(statistics.median(timed(steps[k], a.reps)))
        r = dict(B=B, T=T, S=S, context="features")
        for k in variants:
            r[k + "_ms_by_order"], r[k + "_ms"] = ms[k], statistics.median(ms[k])
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.out and results:
        with open(a.out, "w") as f:
            json.dump(dict(model="hidden 160, heads 4, n_mels 80, layers 4, window 64; storage fp32; variants are matmul_dtype/attn_dtype",
                           library=a.label,
                           device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
