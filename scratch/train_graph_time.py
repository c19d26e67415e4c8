#!/usr/bin/env python3
"""The training step eager and as one graph launch: decoder forward with dropout, DiffusionObjective, backward,
clip + AdamW + blob mirror, cosine learning rate.

    python scratch/train_graph_time.py [--out profiles/train_graph_time.json] [--reps 10] [--contenders parent,eager,graph,graph_deferred]
    python scratch/train_graph_time.py --contenders parent       # runs on a checkout of the parent commit too: the baseline
    python scratch/train_graph_time.py --trace graph --shape 8x173x100 --precision fp32   # the process to put under a kernel trace
    python scratch/train_graph_time.py --merge parent=DIR,eager=DIR,graph=DIR --out profiles/train_graph_time.json

Contenders: "parent" -- the eager step through the API of the commit before GraphedTrainStep (host dropout seed, host noise seeds,
FusedAdamW with the learning rate set in the groups by the host's cosine formula); "eager" -- the same step on the capturable path
(KeyStream, FusedAdamW(capturable=True) with the device schedule); "graph" / "graph_deferred" -- GraphedTrainStep replays with the
host bookkeeping after every replay / left to finish().  Shapes B x T x S = 8 x 173 x 100 and 64 x 512 x 256 on the default model
(hidden 160, 4 heads, 80 mels, 4 layers, window 64), fp32 and bf16 matmul + attention + tape, dropout 0.2, device lengths (full).
Protocol: a settle phase, then passes over the contenders, alternately in the given and in the reversed order, `rounds` of each
(2 x rounds passes); a pass times `reps` one-step windows between hipEvents per contender and keeps their median; a contender's
figure is the median over its passes and its spread their max - min; the host time of a step is the wall time of its call without a
synchronisation.  --trace runs warmed steps with one k_randn launch in front of each as a marker; --merge counts the launches
between the last two markers of each kernel trace."""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "edge-diffusion-tts_amd"))
import edge_diffusion_tts_amd as E  # noqa: E402
from edge_diffusion_tts_amd import CFG, DiffusionObjective, DiffusionSchedule, EdgeDiffusionDecoder, FusedAdamW, native, synth_state_dict  # noqa: E402

DEV = "cuda"
SHAPES = ((8, 173, 100), (64, 512, 256))
PRECISIONS = {"fp32": {}, "bf16": dict(matmul_dtype="bf16", attn_dtype="bf16", tape_dtype="bf16")}
HYPER = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
SCHED = dict(base_lr=2e-4, min_lr=1e-6, warmup_steps=100, total_steps=100000)


def host_cosine(step):
    if step < SCHED["warmup_steps"]:
        return SCHED["base_lr"] * step / max(SCHED["warmup_steps"], 1)
    progress = (step - SCHED["warmup_steps"]) / max(SCHED["total_steps"] - SCHED["warmup_steps"], 1)
    return SCHED["min_lr"] + 0.5 * (SCHED["base_lr"] - SCHED["min_lr"]) * (1 + math.cos(math.pi * progress))


def build(contender, B, T, S, precision):
    """A callable that runs one training step of `contender`, and one that finishes deferred work."""
    cfg = CFG(device=DEV, dropout=0.2)
    g = torch.Generator().manual_seed(B + T)
    mel = (torch.randn(B, T, cfg.n_mels, generator=g) * 1.5 - 4.0).to(DEV)
    t = torch.randint(1, 1000, (B,), generator=g).to(DEV)
    feats = torch.randn(B, S, cfg.semantic_dim, generator=g).to(DEV)
    si = torch.zeros(B, dtype=torch.long, device=DEV)
    xl, sl = torch.full((B,), T, device=DEV), torch.full((B,), S, device=DEV)
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, train_dropout=True, train_lengths=True, **PRECISIONS[precision])
    dec.load_state_dict(synth_state_dict(cfg, 0))
    dec = dec.to(DEV).train()
    obj = DiffusionObjective(DiffusionSchedule(cfg.diff_steps).to(DEV), "v")
    if contender == "parent":
        opt = FusedAdamW(dec.parameters(), max_norm=cfg.grad_clip, zero_grads=True, **HYPER)
        opt.attach_decoder(dec)
        count = [0]

        def step():
            lr = host_cosine(count[0])
            for group in opt.param_groups:
                group["lr"] = lr
            count[0] += 1
            prep = obj.prepare(mel, t, lengths=xl)
            loss = obj.loss(dec(prep.x_t, t, sem_features=feats, step_idx=si, x_lengths=xl, sem_lengths=sl), prep)
            loss.backward()
            opt.step()

        return step, lambda: None
    keys = E.KeyStream(1234, n_slots=1, n_rows=B, device=DEV)
    dec.dropout_keys = (keys, 0)
    opt = FusedAdamW(dec.parameters(), max_norm=cfg.grad_clip, zero_grads=True, capturable=True, **HYPER)
    opt.attach_decoder(dec)
    opt.device_lr_schedule("cosine", **SCHED)

    def fn(mel, t, feats, si, xl, sl):
        prep = obj.prepare(mel, t, lengths=xl, seeds=keys.rows())
        return obj.loss(dec(prep.x_t, t, sem_features=feats, step_idx=si, x_lengths=xl, sem_lengths=sl), prep)

    inputs = (mel, t, feats, si, xl, sl)
    if contender == "eager":
        def step():
            keys.advance()
            fn(*inputs).backward()
            opt.step()

        return step, lambda: None
    graphed = E.GraphedTrainStep(fn, opt, inputs, keys=keys, warmup=2, bookkeeping=contender == "graph")
    return (lambda: graphed(*inputs)), graphed.finish


def timed(call, reps):
    """(ms per step between hipEvents, host ms per call) over `reps` one-step windows."""
    dev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        h0 = time.perf_counter()
        call()
        host.append((time.perf_counter() - h0) * 1e3)
        b.record()
        b.synchronize()
        dev.append(a.elapsed_time(b))
    return statistics.median(dev), statistics.median(host)


def contest(calls, reps, warmup, rounds):
    for step, finish in calls.values():
        for _ in range(warmup):
            step()
        finish()
    torch.cuda.synchronize()
    names = list(calls)
    ms, host = {k: [] for k in names}, {k: [] for k in names}
    for order in (names, names[::-1]) * rounds:
        for k in order:
            d, h = timed(calls[k][0], reps)
            calls[k][1]()
            ms[k].append(d)
            host[k].append(h)
    out = {}
    for k in names:
        out[k] = dict(ms_by_pass=ms[k], ms=statistics.median(ms[k]), host_ms_by_pass=host[k], host_ms=statistics.median(host[k]),
                      spread_ms=max(ms[k]) - min(ms[k]))
    return out


def trace_summary(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {d}, found {files}")
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if "k_randn" in r["Kernel_Name"]]
    if len(marks) < 2:
        raise SystemExit(f"{files[0]}: fewer than two step markers")
    one = rows[marks[-2] + 1:marks[-1]]
    return dict(launches_per_step=len(one), kernel_ns_per_step=sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in one))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="passes over the contenders in each of the two orders")
    ap.add_argument("--contenders", default="parent,eager,graph,graph_deferred")
    ap.add_argument("--shapes", default=",".join("x".join(str(v) for v in s) for s in SHAPES))
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--trace", default=None, choices=("parent", "eager", "graph", "graph_deferred"))
    ap.add_argument("--shape", default="8x173x100")
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--merge", default=None)
    a = ap.parse_args()
    if a.merge:
        doc = {}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc["kernel_trace"] = dict(shape=a.shape, precision=a.precision, **{k: trace_summary(d) for k, d in (kv.split("=") for kv in a.merge.split(","))})
        print(json.dumps(doc["kernel_trace"]))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("train_graph_time.py measures on the GPU; there is none here")
    if a.trace:
        step, finish = build(a.trace, *(int(v) for v in a.shape.split("x")), a.precision)
        for _ in range(a.warmup + 3):
            native.randn((4,), DEV)
            step()
        native.randn((4,), DEV)
        finish()
        torch.cuda.synchronize()
        return
    names = a.contenders.split(",")
    # the first second of work on a fresh process runs slower for every contender (clocks, allocator): spend it before the first window
    settle = build(names[0], *SHAPES[0], "fp32")[0]
    for _ in range(100):
        settle()
    torch.cuda.synchronize()
    del settle
    results = []
    for shape in a.shapes.split(","):
        B, T, S = (int(v) for v in shape.split("x"))
        for precision in a.precisions.split(","):
            r = dict(B=B, T=T, S=S, precision=precision, contenders=contest({k: build(k, B, T, S, precision) for k in names}, a.reps, a.warmup, a.rounds))
            print(json.dumps(r), flush=True)
            results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, rounds=a.rounds, schedule=SCHED,
                           model="hidden 160, heads 4, n_mels 80, layers 4, window 64, dropout 0.2; features as context", results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
