"""Batched long-form synthesis: N utterances (default 64) of 4..12 s (seeded) through the reference's sliding
window (2.0 s chunks = 201 frames, 0.5 s = 51 frames of overlap, default fp32 decoder) three ways:
  (a) generate_long one utterance after another,
  (b) the same on --streams torch streams of one thread (utterance n on stream n % streams),
  (c) one generate_long_batch call.
Each (mode, steps, cfg_scale) case runs in a child process of its own under a time limit (--case-timeout s): a warm-up run, then
--repeats timed runs, each ending in a device synchronise; prints one JSON line per case (median utterances/s and mel frames/s).
The first case that times out or fails stops the run (exit status nonzero); no further case is started.
--profile-chunk I: instead, one generate_long_batch chunk index I alone (for rocprofv3 --kernel-trace --stats).
Usage (GPU box): python scratch/longform_batch_throughput.py [--steps 10,150] [--cfg 1.0,1.5] [--modes a,b,c]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "edge-diffusion-tts_amd"), REPO]


def setup(a):
    import torch
    from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, InpaintSampler, synth_state_dict
    cfg = CFG(device="cuda")
    dec = EdgeDiffusionDecoder(cfg)
    dec.load_state_dict(synth_state_dict(cfg, 0, max_pos=dec.max_len, max_ctx_pos=dec.max_context_len))
    dec = dec.cuda().eval()
    smp = InpaintSampler(cfg, DiffusionSchedule(cfg.diff_steps).to("cuda"), dec)
    g = torch.Generator().manual_seed(a.seed)
    secs = (4.0 + 8.0 * torch.rand(a.N, generator=g)).tolist()
    sr, hop = cfg.sample_rate, cfg.hop_length
    chunk_s, ov_s = int(2.0 * sr), int(0.5 * sr)  # the reference's sample counts (inference_pipeline.py:221-225)
    chunk_f, ov_f = chunk_s // hop + 1, ov_s // hop + 1  # centred mel frames: 201 / 51
    utts = []
    for n, s in enumerate(secs):
        samples = int(s * sr)
        frames = samples // hop + 1
        feats = torch.randn(1, samples // 320 + 1, cfg.semantic_dim, generator=g).cuda()
        k = InpaintSampler.chunk_plan(frames, chunk_f, ov_f, hop, chunk_s, ov_s, samples)[0]
        stats = [(torch.zeros(1, 1, cfg.n_mels, device="cuda"), torch.full((1, 1, cfg.n_mels), 0.5, device="cuda"))] * k
        utts.append(dict(feats=feats, frames=frames, samples=samples, stats=stats, seed=1000 + 10 * n))
    geo = dict(chunk_frames=chunk_f, overlap_frames=ov_f, chunk_samples=chunk_s, overlap_samples=ov_s)
    return torch, smp, utts, geo


def run_case(a):
    torch, smp, utts, geo = setup(a)
    mode, steps, scale = a.case.split(",")
    steps, scale = int(steps), float(scale)
    kw = dict(strength=0.999, steps=steps, cfg_scale=scale, chunk_samples=geo["chunk_samples"], overlap_samples=geo["overlap_samples"])

    def one(u):
        return smp.generate_long(u["feats"], u["frames"], geo["chunk_frames"], geo["overlap_frames"], u["stats"], seed=u["seed"],
                                 total_samples=u["samples"], **kw)
    streams = [torch.cuda.Stream() for _ in range(a.streams)] if mode == "b" else None

    def run():
        if mode == "a":
            for u in utts:
                one(u)
        elif mode == "b":
            main = torch.cuda.current_stream()
            for s in streams:
                s.wait_stream(main)
            for n, u in enumerate(utts):
                with torch.cuda.stream(streams[n % len(streams)]):
                    one(u)
        else:
            smp.generate_long_batch([u["feats"] for u in utts], [u["frames"] for u in utts], geo["chunk_frames"], geo["overlap_frames"],
                                    [u["stats"] for u in utts], seeds=[u["seed"] for u in utts],
                                    total_samples=[u["samples"] for u in utts], **kw)
        torch.cuda.synchronize()
    run()  # warm-up (workspaces, packing, kernel attributes)
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        run()
        times.append(time.perf_counter() - t0)
    med = sorted(times)[len(times) // 2]
    frames = sum(u["frames"] for u in utts)
    print(json.dumps({"mode": mode, "steps": steps, "cfg_scale": scale, "N": len(utts), "streams": a.streams if mode == "b" else 1,
                      "seconds_median": round(med, 3), "seconds_all": [round(t, 3) for t in times],
                      "utterances_per_s": round(len(utts) / med, 2), "mel_frames_per_s": round(frames / med, 1)}), flush=True)


def profile_chunk(a):
    """Chunk index --profile-chunk of the batch alone: the batched teacher call of that index (every live row), after one warm-up."""
    torch, smp, utts, geo = setup(a)
    from edge_diffusion_tts_amd import native
    steps, scale = (int(a.steps.split(",")[0]), float(a.cfg.split(",")[0]))
    i = a.profile_chunk
    plans = smp.plan_long_batch([u["feats"].shape[1] for u in utts], [u["frames"] for u in utts], geo["chunk_frames"],
                                geo["overlap_frames"], [u["stats"] for u in utts], [u["seed"] for u in utts],
                                chunk_samples=geo["chunk_samples"], overlap_samples=geo["overlap_samples"],
                                total_samples=[u["samples"] for u in utts])
    live = [n for n in range(len(utts)) if plans[n]["n_chunks"] > i]
    rows = [plans[n]["slices"][i] for n in live]
    S = max(b - r for r, b in rows)
    sem = torch.zeros(len(live), S, smp.cfg.semantic_dim, device="cuda")
    for j, (n, (r, b)) in enumerate(zip(live, rows)):
        sem[j, :b - r] = utts[n]["feats"][0, r:b]
    s_len = torch.tensor([b - r for r, b in rows])
    seeds = [utts[n]["seed"] + 2 * i for n in live]
    M, T, ov = smp.cfg.n_mels, geo["chunk_frames"], geo["overlap_frames"]
    known = torch.randn(len(live), ov, M, device="cuda") if i > 0 else None
    for _ in range(2):  # warm-up, then the call to look at
        xc = native.randn_rows((len(live), T, M), "cuda", [v + 1 for v in seeds], stream_id=0x53)
        smp.inpaint_teacher_refine(xc, sem, known, ov if known is not None else 0, 0.999, steps, scale, sem_lengths=s_len, seeds=seeds)
        torch.cuda.synchronize()
    print(json.dumps({"profile_chunk": i, "rows": len(live), "S": S, "steps": steps, "cfg_scale": scale}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", default="10,150")
    ap.add_argument("--cfg", default="1.0,1.5")
    ap.add_argument("--modes", default="a,b,c")
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--case-timeout", type=float, default=600.0, help="seconds per (mode, steps, cfg) child process")
    ap.add_argument("--case", help=argparse.SUPPRESS)
    ap.add_argument("--profile-chunk", type=int)
    a = ap.parse_args()
    if a.case:
        return run_case(a)
    if a.profile_chunk is not None:
        return profile_chunk(a)
    for steps in a.steps.split(","):
        for scale in a.cfg.split(","):
            for mode in a.modes.split(","):
                cmd = [sys.executable, os.path.abspath(__file__), "--case", f"{mode},{steps},{scale}", "--N", str(a.N), "--seed",
                       str(a.seed), "--streams", str(a.streams), "--repeats", str(a.repeats)]
                # A case that hits its time limit or fails in any way ends the run: nothing more is started on a card that may be
                # faulted or hung.  Rerun the remaining cases on their own (--steps / --cfg / --modes) once the cause is known.
                try:
                    r = subprocess.run(cmd, timeout=a.case_timeout, capture_output=True, text=True)
                except subprocess.TimeoutExpired:
                    print(json.dumps({"mode": mode, "steps": int(steps), "cfg_scale": float(scale), "error": f"over {a.case_timeout} s"}),
                          flush=True)
                    return 124
                if r.returncode != 0:
                    print(json.dumps({"mode": mode, "steps": int(steps), "cfg_scale": float(scale), "rc": r.returncode,
                                      "stderr": r.stderr[-600:]}), flush=True)
                    return 1
                sys.stdout.write(r.stdout)
                sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
