#!/usr/bin/env python3
"""DiffusionObjective (prepare + loss + backward to d_pred: 5 launches) against the torch composition it replaces -- normalize_mel,
randn_like, q_sample, get_v_target, F.mse_loss with its autograd backward, and the metrics predict_x0_from_v, F.mse_loss,
F.cosine_similarity(...).mean() kept on the device (the reference ends each with .item(); no contender here synchronises).

    python scratch/objective_time.py [--out profiles/objective_time.json] [--reps 20] [--inner 20]
    python scratch/objective_time.py --trace fused|torch [--shape 8x173]     # the process to put under rocprofv3 --kernel-trace --stats
    python scratch/objective_time.py --merge fused=DIR,torch=DIR --out profiles/objective_time.json

Shapes B x T = 8 x 173 and 64 x 512 at M = 80, padded and at a live fraction of 0.66 (lengths spread evenly over [0.32 T, T]; the
torch contender then masks the loss as tests/train_ragged_util.py: masked_loss does and keeps its statistics over the padding).
Protocol of scratch/train_time.py: 5 warm-up rounds, medians of `reps` windows between hipEvents (a window is `inner` calls: one
call is tens of microseconds), both orders of the two contenders, the spread between orders recorded.  The whole step -- objective +
EdgeDiffusionDecoder(kernels="generic", autograd=True) forward and backward + FusedAdamW -- is timed the same way with either
objective in it (default model: hidden 160, 4 heads, 80 mels, 4 layers, window 64; S = 100 / 256 context features).
--trace runs warmed calls with one k_randn launch in front of each as a marker; --merge counts the launches between the last two
markers of each kernel trace and sums their durations (bytes/s against the 16 B per mel element the fused path needs: mel in, x_t
out, pred in, d_pred out; its unit gradient and the mel's second read are 12 more)."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "edge-diffusion-tts_amd"))
from edge_diffusion_tts_amd import (CFG, DiffusionObjective, DiffusionSchedule, EdgeDiffusionDecoder, FusedAdamW, native,  # noqa: E402
                                    synth_state_dict)

DEV = "cuda"
M = 80
SHAPES = ((8, 173, 100), (64, 512, 256))
HYPER = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def normalize_mel(mel):
    mean = mel.mean(dim=1, keepdim=True)
    std = mel.std(dim=1, keepdim=True).clamp_min(1e-5)
    return (mel - mean) / std, mean, std


def inputs(B, T, live):
    g = torch.Generator().manual_seed(B + T)
    mel = (torch.randn(B, T, M, generator=g) * 1.5 - 4.0).to(DEV)
    pred = torch.randn(B, T, M, generator=g).to(DEV).requires_grad_(True)
    t = torch.randint(1, 1000, (B,), generator=g).to(DEV)
    lens = None
    if live < 1.0:  # evenly spread over [2 live - 1, 1] T: mean live fraction `live`
        lo = 2.0 * live - 1.0
        lens = torch.tensor([max(2, round(T * (lo + (1.0 - lo) * (i + 0.5) / B))) for i in range(B)]).to(DEV)
    return mel, pred, t, lens


def torch_objective(sch, mel, pred_of, t, lens):
    """The reference's expressions (train_v2.py:112-154); with lengths, the mask users write today."""
    mel_n, _, _ = normalize_mel(mel)
    noise = torch.randn_like(mel_n)
    x_t, _ = sch.q_sample(mel_n, t, noise)
    v = pred_of(x_t)
    target = sch.get_v_target(mel_n, noise, t)
    if lens is None:
        loss = F.mse_loss(v, target)
    else:
        m = (torch.arange(mel.shape[1], device=mel.device)[None, :] < lens[:, None])[..., None].to(v.dtype)
        loss = (((v - target) * m) ** 2).sum() / (lens.sum() * mel.shape[2]).to(v.dtype)
    with torch.no_grad():
        x0 = sch.predict_x0_from_v(x_t, t, v)
        metrics = (F.mse_loss(x0, mel_n), F.cosine_similarity(x0.flatten(1), mel_n.flatten(1), dim=1).mean())
    return loss, metrics


def fused_objective(obj, mel, pred_of, t, lens, seeds):
    prep = obj.prepare(mel, t, lens, seeds=seeds)
    loss = obj.loss(pred_of(prep.x_t), prep)
    return loss, (obj.last_metrics["x0_mse"], obj.last_metrics["x0_cos"])


def objective_calls(sch, B, T, live, marker=False):
    """{"fused": call, "torch": call}: the objective alone, on a fixed prediction, backward to d_pred."""
    mel, pred, t, lens = inputs(B, T, live)
    obj = DiffusionObjective(sch)
    seeds = native.seed_tensor(list(range(1, B + 1)), B, DEV)

    def run(which):
        if marker:
            native.randn((4,), DEV)
        pred.grad = None
        if which == "fused":
            loss, _ = fused_objective(obj, mel, lambda x_t: pred, t, lens, seeds)
        else:
            loss, _ = torch_objective(sch, mel, lambda x_t: pred, t, lens)
        loss.backward()

    return {k: (lambda k=k: run(k)) for k in ("fused", "torch")}


def step_calls(sch, cfg, B, T, S, live):
    """The whole training step with either objective in it."""
    mel, _, t, lens = inputs(B, T, live)
    g = torch.Generator().manual_seed(S)
    feats = torch.randn(B, S, cfg.semantic_dim, generator=g).to(DEV)
    si = torch.zeros(B, dtype=torch.long, device=DEV)
    seeds = native.seed_tensor(list(range(1, B + 1)), B, DEV)
    s_len = None if lens is None else (lens * S // T).clamp(min=1)
    out = {}
    for which in ("fused", "torch"):
        dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, train_lengths=lens is not None)
        dec.load_state_dict(synth_state_dict(cfg, 0))
        dec = dec.to(DEV).train()
        opt = FusedAdamW(dec.parameters(), max_norm=cfg.grad_clip, **HYPER)
        opt.attach_decoder(dec)
        obj = DiffusionObjective(sch)
        kw = {} if lens is None else dict(x_lengths=lens, sem_lengths=s_len)

        def step(which=which, dec=dec, opt=opt, obj=obj, kw=kw):
            opt.zero_grad(set_to_none=True)
            pred_of = lambda x_t: dec(x_t, t, sem_features=feats, step_idx=si, **kw)
            if which == "fused":
                loss, _ = fused_objective(obj, mel, pred_of, t, lens, seeds)
            else:
                loss, _ = torch_objective(sch, mel, pred_of, t, lens)
            loss.backward()
            opt.step()

        out[which] = step
    return out


def timed(call, reps, inner):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            call()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return out


def contest(calls, reps, inner, warmup):
    for c in calls.values():
        for _ in range(warmup):
            c()
    torch.cuda.synchronize()
    ms = {"fused": [], "torch": []}
    for order in (("fused", "torch"), ("torch", "fused")):
        for k in order:
            ms[k].append(statistics.median(timed(calls[k], reps, inner)))
    r = dict(fused_ms_by_order=ms["fused"], torch_ms_by_order=ms["torch"], fused_ms=statistics.median(ms["fused"]),
             torch_ms=statistics.median(ms["torch"]))
    r["order_spread_ms"] = max(abs(ms["fused"][0] - ms["fused"][1]), abs(ms["torch"][0] - ms["torch"][1]))
    r["torch_minus_fused_ms"] = r["torch_ms"] - r["fused_ms"]
    r["fused_is_faster_by_more_than_the_spread"] = r["torch_minus_fused_ms"] > r["order_spread_ms"]
    return r


def trace_summary(d, elements):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {d}, found {files}")
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if "k_randn" in r["Kernel_Name"]]
    if len(marks) < 2:
        raise SystemExit(f"{files[0]}: fewer than two call markers")
    one = rows[marks[-2] + 1:marks[-1]]
    by_name = {}
    for r in one:
        name = r["Kernel_Name"].replace("void ", "").split("(")[0].split("<")[0]
        n, ns = by_name.get(name, (0, 0))
        by_name[name] = (n + 1, ns + int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    ns = sum(v[1] for v in by_name.values())
    return dict(launches_per_call=len(one), kernel_ns_per_call=ns, bytes_per_s_at_16B_per_element=16.0 * elements / (ns * 1e-9),
                kernels={k: dict(launches=v[0], ns=v[1]) for k, v in sorted(by_name.items())})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", default=None, choices=("fused", "torch"))
    ap.add_argument("--shape", default="8x173")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--no-step", action="store_true", help="skip the whole-step timing")
    a = ap.parse_args()
    B0, T0 = (int(v) for v in a.shape.split("x"))
    if a.merge:
        with open(a.out) as f:
            doc = json.load(f)
        doc["kernel_trace"] = dict(shape=[B0, T0, M], **{k: trace_summary(d, B0 * T0 * M) for k, d in (kv.split("=") for kv in a.merge.split(","))})
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(json.dumps(doc["kernel_trace"]))
        return
    if not torch.cuda.is_available():
        raise SystemExit("objective_time.py measures on the GPU; there is none here")
    cfg = CFG(device=DEV, dropout=0.0)
    sch = DiffusionSchedule(cfg.diff_steps).to(DEV)
    if a.trace:
        call = objective_calls(sch, B0, T0, 1.0, marker=True)[a.trace]
        for _ in range(a.warmup + 3):
            call()
        native.randn((4,), DEV)
        torch.cuda.synchronize()
        return
    # the first second of work on a fresh process runs slower for every contender (clocks, allocator): spend it before the first window
    settle = step_calls(sch, cfg, *SHAPES[0], 1.0)
    for _ in range(100):
        settle["fused"]()
        settle["torch"]()
    torch.cuda.synchronize()
    del settle
    results = []
    for B, T, S in SHAPES:
        for live in (1.0, 0.66):
            r = dict(B=B, T=T, M=M, live_fraction=live, what="objective: prepare + loss + backward to d_pred")
            r.update(contest(objective_calls(sch, B, T, live), a.reps, a.inner, a.warmup))
            print(json.dumps(r), flush=True)
            results.append(r)
            if a.no_step:
                continue
            r = dict(B=B, T=T, S=S, M=M, live_fraction=live, what="whole step: objective + decoder forward and backward + FusedAdamW")
            r.update(contest(step_calls(sch, cfg, B, T, S, live), a.reps, 1, a.warmup))
            print(json.dumps(r), flush=True)
            results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, inner_calls_per_window=a.inner, warmup=a.warmup,
                           model="hidden 160, heads 4, n_mels 80, layers 4, window 64, fp32; features as context", results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
