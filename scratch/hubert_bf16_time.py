"""HuBERT forward at 9 layers, B = 16 x 10 s and B = 1 x 2 s (16 kHz) on one GPU, alternated, median of N calls timed with events:
  (a) NativeHubert(num_layers=9), fp32 (csrc/edtts_hubert.h) -- the baseline
  (b) NativeHubert(num_layers=9, compute_dtype="bf16") (csrc/edtts_hubert16.h)
  (c) transformers HubertModel with encoder.layers truncated to 9, fp32
  (d) the same under torch.autocast("cuda", dtype=torch.bfloat16)
(b) is also reported as a fraction of the bf16 MFMA bound (16 x the fp32 MFMA peak of 157.3 TFLOP/s) of the FLOP count of DESIGN.md section 14.  The spread
of a variant is the interquartile range of its alternated calls.
--only bf16 --calls K: (b) alone, for a `rocprofv3 --kernel-trace --stats` run.  Writes JSON to argv[--out] if given."""
import argparse
import copy
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "edge-diffusion-tts_amd"))

import torch  # noqa: E402

from edge_diffusion_tts_amd import NativeHubert  # noqa: E402

PEAK_BF16 = 16 * 157.3e12
PEAK_FP32 = 157.3e12


def flops(B, T_feat, layers=9):
    """conv stack 98.0 M + positional conv 9.4 M + per layer 14.2 M + 4 T 768 (attention) per feature frame, at the defaults"""
    per = 98.0e6 + 9.44e6 + layers * (14.16e6 + 4 * T_feat * 768)
    return per * B * T_feat


def timed(fn, wav):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn(wav)
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from transformers import HubertConfig, HubertModel
    torch.manual_seed(0)
    cut = HubertModel(HubertConfig()).eval().cuda()
    n32 = NativeHubert.from_hubert(cut, 9)
    n16 = NativeHubert.from_hubert(cut, 9, compute_dtype="bf16")
    cut = copy.deepcopy(cut)
    cut.encoder.layers = cut.encoder.layers[:9]

    def autocast(w):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return cut(w, output_hidden_states=True)

    variants = {"a_native_fp32": lambda w: n32(w), "b_native_bf16": lambda w: n16(w),
                "c_torch_fp32": lambda w: cut(w, output_hidden_states=True), "d_torch_autocast": autocast}
    if args.only == "bf16":
        variants = {"b_native_bf16": variants["b_native_bf16"]}
    res = []
    with torch.no_grad():
        for B, sec in ((16, 10), (1, 2)):
            wav = 0.1 * torch.randn(B, 16000 * sec, device="cuda")
            T = n32.frames(wav.shape[1])
            for fn in variants.values():
                for _ in range(3):
                    fn(wav)
            torch.cuda.synchronize()
            ms = {k: [] for k in variants}
            for _ in range(args.calls):
                for k, fn in variants.items():
                    ms[k].append(timed(fn, wav))
            F = flops(B, T)
            row = {"B": B, "seconds": sec, "T_feat": T, "gflop_9_layers": F / 1e9, "bf16_bound_ms": F / PEAK_BF16 * 1e3,
                   "fp32_bound_ms": F / PEAK_FP32 * 1e3}
            for k, v in ms.items():
                q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
                row[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "iqr_ms": q[2] - q[0]}
            if "b_native_bf16" in row:
                row["b_native_bf16"]["fraction_of_bf16_bound"] = F / PEAK_BF16 * 1e3 / row["b_native_bf16"]["median_ms"]
            if len(variants) == 4 and B == 16:  # the two outputs at the size that is timed
                d = (n16(wav) - n32(wav)).abs()
                row["bf16_vs_fp32_native_max_abs"] = float(d.max())
            res.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"calls": args.calls, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
