"""In-painting anywhere: what the per-frame mask costs next to the known prefix, on the default fp32 decoder
(160/4/80) at B = 64, T = 201, S = 100, cfg 1.5, strength 0.999: inpaint_teacher_refine at 10 first-order steps and inpaint_dpm_refine at
15 second-order steps, each as

  prefix        known_mel [B, 51, n_mels], overlap_len = 51            (the call the long-form pipeline makes)
  mask_prefix   keep[b, f] = f < 51 of a known_mel [B, T, n_mels]      (the same frames through the mask entry point)
  mask_middle   the middle third regenerated, both sides kept          (speech editing)

interleaved, --repeats times each after a warm-up; every timed call ends in a device synchronise.  Prints ONE JSON line with the
medians and the spread (max / min - 1) of each call's repeats.  A package that has no keep= (EDTTS_PKG_ROOT names the package
directory of a checkout of the parent commit, built there) times the prefix call alone: alternate the two processes for the
same-session comparison.  Needs a GPU: there is no CPU path.
Usage (GPU box): python scratch/inpaint_mask_time.py [--repeats 12]"""
import argparse
import inspect
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("EDTTS_PKG_ROOT", os.path.join(REPO, "edge-diffusion-tts_amd")))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=201)
    ap.add_argument("--S", type=int, default=100)
    ap.add_argument("--overlap", type=int, default=51)
    ap.add_argument("--cfg", type=float, default=1.5)
    ap.add_argument("--repeats", type=int, default=12)
    a = ap.parse_args()
    import torch
    from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, InpaintSampler, native, synth_state_dict
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = CFG(device="cuda")
    dec = EdgeDiffusionDecoder(cfg)
    dec.load_state_dict(synth_state_dict(cfg, 0, max_pos=dec.max_len, max_ctx_pos=dec.max_context_len))
    dec = dec.to("cuda").eval()
    smp = InpaintSampler(cfg, DiffusionSchedule(cfg.diff_steps).to("cuda"), dec)
    has_keep = "keep" in inspect.signature(InpaintSampler.inpaint_dpm_refine).parameters
    B, T, S, ov, M = a.B, a.T, a.S, a.overlap, cfg.n_mels
    g = torch.Generator().manual_seed(1)
    xc = torch.randn(B, T, M, generator=g).cuda()
    sem = torch.randn(B, S, cfg.semantic_dim, generator=g).cuda()
    known = torch.randn(B, T, M, generator=g).cuda()
    tail = known[:, :ov].contiguous()
    seeds = native.seed_tensor(list(range(B)), B, "cuda")
    samplers = {"first_order_10": lambda kn, o, **kw: smp.inpaint_teacher_refine(xc, sem, kn, o, 0.999, 10, a.cfg, seeds=seeds, **kw),
                "dpmpp2_15": lambda kn, o, **kw: smp.inpaint_dpm_refine(xc, sem, kn, o, 0.999, 15, 2, a.cfg, seeds=seeds, **kw)}
    calls = {}
    for name, fn in samplers.items():
        calls[name + "/prefix"] = lambda fn=fn: fn(tail, ov)
        if has_keep:
            k_prefix = torch.zeros(B, T, dtype=torch.bool, device="cuda")
            k_prefix[:, :ov] = True
            k_middle = torch.ones(B, T, dtype=torch.bool, device="cuda")
            k_middle[:, T // 3:2 * T // 3] = False
            calls[name + "/mask_prefix"] = lambda fn=fn, k=k_prefix: fn(known, 0, keep=k)
            calls[name + "/mask_middle"] = lambda fn=fn, k=k_middle: fn(known, 0, keep=k)
    t = {k: [] for k in calls}
    for fn in calls.values():  # warm-up of every call
        fn()
        torch.cuda.synchronize()
    for _ in range(a.repeats):  # interleaved
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[k].append(time.perf_counter() - t0)
    res = {"package": os.path.relpath(os.path.dirname(os.path.abspath(native.__file__)), REPO), "has_keep": has_keep, "B": B, "T": T, "S": S, "overlap": ov,
           "cfg_scale": a.cfg, "repeats": a.repeats,
           "calls": {k: {"ms_median": round(1e3 * median(v), 3), "ms_min": round(1e3 * min(v), 3), "ms_max": round(1e3 * max(v), 3),
                         "spread": round(max(v) / min(v) - 1, 4)} for k, v in t.items()}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
