#!/usr/bin/env python3
"""One whole training step -- forward + backward + optimiser + the next forward's pack -- of EdgeDiffusionDecoder(kernels="generic",
autograd=True) with FusedAdamW (clip, AdamW and the blob refresh in one pass) against the path before it on the same decoder:
clip_grad_norm_ + torch.optim.AdamW (torch's default implementation) + the re-pack.

    python scratch/optim_time.py [--out profiles/optim_time.json] [--reps 20] [--shapes 8x173x100,64x512x256]
    python scratch/optim_time.py --trace fused|torch [--shapes 8x173x100]      # the process to put under rocprofv3 --kernel-trace
    python scratch/optim_time.py --merge fused=DIR,torch=DIR --out profiles/optim_time.json

scratch/train_time.py's protocol: default model (hidden 160, 4 heads, 80 mels, 4 layers, window 64), 5 warm-up steps, medians of 20
steps between hipEvents, both orders of the two contenders, the spread between orders recorded.  The optimiser is never timed in
a loop of its own: its 11 MB of state would sit in cache.  --trace runs warmed steps with one k_randn launch in front of each as a
marker; --merge counts the launches between the last two markers of each kernel trace (launches per step) and takes k_opt_adamw's
duration from the fused one (achieved bytes/s against the 28 B per element it moves: p, g, m, v in, p, m, v out; the mirror
into the blob is another 4)."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "edge-diffusion-tts_amd"))
from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, FusedAdamW, native, synth_state_dict  # noqa: E402

DEV = "cuda"
HYPER = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def make(cfg, fused):
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True)
    dec.load_state_dict(synth_state_dict(cfg, 0))
    dec = dec.to(DEV).train()
    if fused:
        opt = FusedAdamW(dec.parameters(), max_norm=cfg.grad_clip, **HYPER)
        opt.attach_decoder(dec)
    else:
        opt = torch.optim.AdamW(dec.parameters(), **HYPER)
    return dec, opt


def make_step(dec, opt, sch, cfg, B, T, S, fused, marker=False):
    g = torch.Generator().manual_seed(B + T)
    x0 = torch.randn(B, T, cfg.n_mels, generator=g).to(DEV)
    noise = torch.randn(B, T, cfg.n_mels, generator=g).to(DEV)
    feats = torch.randn(B, S, cfg.semantic_dim, generator=g).to(DEV)
    t = torch.randint(1, 1000, (B,), generator=g).to(DEV)
    si = torch.zeros(B, dtype=torch.long, device=DEV)
    params = list(dec.parameters())

    def step():
        if marker:
            native.randn((1,), DEV)
        opt.zero_grad(set_to_none=True)
        x_t, _ = sch.q_sample(x0, t, noise)
        v = dec(x_t, t, sem_features=feats, step_idx=si)
        F.mse_loss(v, sch.get_v_target(x0, noise, t)).backward()
        if fused:
            opt.step()
        else:
            torch.nn.utils.clip_grad_norm_(params, cfg.grad_clip)
            opt.step()
        dec._ensure_packed()  # the next forward's pack belongs to this step (nothing to do after a mirrored step)

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
    by_name = {}
    for r in one:
        name = re.sub(r"^void ", "", r["Kernel_Name"]).split("<")[0].split("(edtts")[0].split("(float")[0]
        n, ns = by_name.get(name, (0, 0))
        by_name[name] = (n + 1, ns + int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    tail = ("k_opt_", "k_copy", "k_transpose", "multi_tensor", "lpnorm", "CatArray", "reduce_kernel", "fillBuffer", "copyBuffer")
    return dict(launches_per_step=len(one), kernel_ns_per_step=sum(v[1] for v in by_name.values()),
                optimiser_and_pack_kernels={k: dict(launches=v[0], ns=v[1]) for k, v in sorted(by_name.items()) if any(t in k for t in tail)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="8x173x100,64x512x256")
    ap.add_argument("--trace", default=None, choices=("fused", "torch"))
    ap.add_argument("--merge", default=None)
    a = ap.parse_args()
    if a.merge:
        with open(a.out) as f:
            doc = json.load(f)
        doc["kernel_trace"] = {k: trace_summary(d) for k, d in (kv.split("=") for kv in a.merge.split(","))}
        n = doc["stepped_elements"]
        ad = [v for k, v in doc["kernel_trace"]["fused"]["optimiser_and_pack_kernels"].items() if "k_opt_adamw" in k]
        if ad:
            doc["k_opt_adamw_ns"] = ad[0]["ns"]
            doc["k_opt_adamw_bytes_per_s_at_28B"] = 28.0 * n / (ad[0]["ns"] * 1e-9)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(json.dumps(doc["kernel_trace"]))
        return
    cfg = CFG(device=DEV, dropout=0.0)
    sch = DiffusionSchedule(cfg.diff_steps).to(DEV)
    pairs = {"fused": make(cfg, True), "torch": make(cfg, False)}
    results = []
    for shape in a.shapes.split(","):
        B, T, S = (int(v) for v in shape.split("x"))
        if a.trace:
            step = make_step(*pairs[a.trace], sch, cfg, B, T, S, a.trace == "fused", marker=True)
            for _ in range(a.warmup + 3):
                step()
            native.randn((1,), DEV)
            torch.cuda.synchronize()
            continue
        steps = {k: make_step(*pairs[k], sch, cfg, B, T, S, k == "fused") for k in pairs}
        for s in steps.values():
            for _ in range(a.warmup):
                s()
        torch.cuda.synchronize()
        ms = {"fused": [], "torch": []}
        for order in (("fused", "torch"), ("torch", "fused")):
            for k in order:
                ms[k].append(statistics.median(timed(steps[k], a.reps)))
        r = dict(B=B, T=T, S=S, fused_ms_by_order=ms["fused"], torch_ms_by_order=ms["torch"], fused_ms=statistics.median(ms["fused"]),
                 torch_ms=statistics.median(ms["torch"]))
        r["order_spread_ms"] = max(abs(ms["fused"][0] - ms["fused"][1]), abs(ms["torch"][0] - ms["torch"][1]))
        r["torch_minus_fused_ms"] = r["torch_ms"] - r["fused_ms"]
        r["fused_is_faster_by_more_than_the_spread"] = r["torch_minus_fused_ms"] > r["order_spread_ms"]
        print(json.dumps(r))
        results.append(r)
    if a.out and results:
        dec = pairs["fused"][0]
        stepped = sum(p.numel() for p in dec.parameters() if p.grad is not None)
        with open(a.out, "w") as f:
            json.dump(dict(model="hidden 160, heads 4, n_mels 80, layers 4, window 64, fp32; features as context", device=torch.cuda.get_device_name(0),
                           step="forward + backward + clip + AdamW + the next forward's pack", reps=a.reps, warmup=a.warmup,
                           parameters=sum(p.numel() for p in dec.parameters()), stepped_elements=stepped, chunk=native.optim_chunk_size(),
                           results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
