#!/usr/bin/env python3
"""One training step's decoder part on EdgeDiffusionDecoder(kernels="generic", autograd=True, matmul_dtype="bf16", attn_dtype="bf16")
with tape_dtype "f32" (off) and "bf16" (on), and the same step on another build of the library (the parent commit's, off only):
scratch/train_time.py's step, 5 warm-up steps, medians of 20 hipEvent times.  Every measurement is a process of its own; the driver
alternates them, once in ascending and once in descending order.  DESIGN.md section 28.

    python scratch/train_tape_bf16_time.py --drive [--parent-lib PATH] [--out profiles/train_tape_bf16_time.json]
                                           [--shapes 8x173x100,64x512x256] [--reps 20]
    python scratch/train_tape_bf16_time.py --variant off|on [--shapes ...]        # one measuring process (what --drive starts)
    python scratch/train_tape_bf16_time.py --one-step off|on --shapes 64x512x256  # warmed steps only: the process to put under
                                                                                  # rocprofv3 --kernel-trace --stats
    python scratch/train_tape_bf16_time.py --kernel-stats off=CSV on=CSV --steps 6  # fold such runs' kernel_stats CSVs into the table

EDTTS_LIB=<a build without edtts_train_tape_region> runs "off" only (the export is dropped from the binding table for that process)."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS = (("forward GEMMs (k_gen_gemm16)", "k_gen_gemm16"), ("k_gen_attn16", "k_gen_attn16"), ("k_bwd_attn_dq16", "k_bwd_attn_dq16"),
          ("k_bwd_attn_dkv16", "k_bwd_attn_dkv16"), ("k_bwd_gemm16", "k_bwd_gemm16"))


def tape_bytes(shapes):
    """edtts_train_tape_bytes of the default model, off and on: host arithmetic, no GPU."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "edge-diffusion-tts_amd"))
    from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, native
    out = {}
    for shape in shapes:
        B, T, S = (int(v) for v in shape.split("x"))
        out[shape] = {t: native.train_tape_bytes(EdgeDiffusionDecoder(CFG(device="cpu"), kernels="generic", autograd=True, matmul_dtype="bf16",
                                                                      attn_dtype="bf16", tape_dtype=t).dims(), B, T, S)
                      for t in ("f32", "bf16")}
    return out


def measure(a):
    import torch
    sys.path.insert(0, HERE)
    from train_time import DEV, make_step, timed  # (it puts the package on sys.path)
    from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, native, synth_state_dict
    variant = a.one_step or a.variant
    if os.environ.get("EDTTS_LIB"):
        import ctypes
        if not hasattr(ctypes.CDLL(os.environ["EDTTS_LIB"]), "edtts_train_tape_region"):  # a build from before the option
            assert variant == "off", "that library has no bf16 tape"
            native._ABI.pop("edtts_train_tape_region")
    cfg = CFG(device=DEV, dropout=0.0)
    sch = DiffusionSchedule(cfg.diff_steps).to(DEV)
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, matmul_dtype="bf16", attn_dtype="bf16",
                               tape_dtype="bf16" if variant == "on" else "f32")
    dec.load_state_dict(synth_state_dict(cfg, 0))
    dec = dec.to(DEV).train()
    for shape in a.shapes.split(","):
        B, T, S = (int(v) for v in shape.split("x"))
        step = make_step(dec, sch, cfg, B, T, S, True)
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        if a.one_step:
            print(f"one {variant} step at {shape}: loss {float(step().detach()):.6f}")
            torch.cuda.synchronize()
            continue
        print(json.dumps(dict(shape=shape, variant=variant, ms=statistics.median(timed(step, a.reps)), loss=float(step().detach()),
                              device=torch.cuda.get_device_name(0))), flush=True)


def drive(a):
    """Alternated processes, both orders; a child that does not end well ends the run."""
    kinds = ["off", "on"] + (["parent"] if a.parent_lib else [])
    shapes = a.shapes.split(",")
    ms = {s: {k: [] for k in kinds} for s in shapes}
    loss, device = {s: {} for s in shapes}, None
    for order in (kinds, kinds[::-1]):
        for kind in order:
            env = dict(os.environ)
            if kind == "parent":
                env["EDTTS_LIB"] = os.path.abspath(a.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--variant", "off" if kind == "parent" else kind, "--shapes", a.shapes,
                   "--reps", str(a.reps), "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=240)
            if r.returncode != 0:
                sys.exit(f"{kind}: exit status {r.returncode}; stopping")
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    d = json.loads(line)
                    ms[d["shape"]][kind].append(d["ms"])
                    loss[d["shape"]][kind] = d["loss"]
                    device = d["device"]
                    print(kind, line, flush=True)
    results = []
    for s in shapes:
        B, T, S = (int(v) for v in s.split("x"))
        r = dict(B=B, T=T, S=S, context="features", loss=loss[s])
        for k in kinds:
            r[k + "_ms_by_order"], r[k + "_ms"] = ms[s][k], statistics.median(ms[s][k])
        r["spread_ms"] = max(max(v) - min(v) for v in ms[s].values())  # the largest difference between two runs of one variant
        results.append(r)
        print(json.dumps(r), flush=True)
    out = dict(model="hidden 160, heads 4, n_mels 80, layers 4, window 64; matmul_dtype and attn_dtype bf16; off / on = tape_dtype f32 / bf16; "
                     "parent = the parent commit's library (no such option)",
               device=device, reps=a.reps, warmup=a.warmup, protocol="one process per measurement, alternated, ascending then descending order",
               results=results, tape_bytes=tape_bytes(shapes))
    if a.kernel_stats:
        out["kernel_split_us_per_step"] = kernel_split(a)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def kernel_split(a):
    """{label: {group: us per step}} from rocprofv3 --kernel-trace --stats kernel_stats CSVs of --one-step runs of --steps steps."""
    table = {}
    for item in a.kernel_stats:
        label, path = item.split("=", 1)
        with open(path) as f:
            rows = list(csv.DictReader(f))
        t = {g: 0.0 for g, _ in GROUPS}
        t["everything"] = 0.0
        for r in rows:
            us = float(r["TotalDurationNs"]) / 1e3 / a.steps
            t["everything"] += us
            for g, key in GROUPS:
                if key in r["Name"]:
                    t[g] += us
        table[label] = {k: round(v, 1) for k, v in t.items()}
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="8x173x100,64x512x256")
    ap.add_argument("--variant", default=None, choices=("off", "on"))
    ap.add_argument("--one-step", default=None, choices=("off", "on"))
    ap.add_argument("--drive", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's build of the library, measured with the option off")
    ap.add_argument("--kernel-stats", nargs="*", default=[], help="label=kernel_stats.csv of a --one-step run under rocprofv3")
    ap.add_argument("--steps", type=int, default=6, help="steps in each --kernel-stats run (its --warmup + 1)")
    a = ap.parse_args()
    if a.drive:
        drive(a)
    elif a.variant or a.one_step:
        measure(a)
    elif a.kernel_stats:
        print(json.dumps(kernel_split(a), indent=1))
    else:
        print(json.dumps(tape_bytes(a.shapes.split(",")), indent=1))


if __name__ == "__main__":
    main()
