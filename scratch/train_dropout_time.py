#!/usr/bin/env python3
"""One training step's decoder part with dropout -- forward + backward of the v-prediction loss, decoder.train(), dropout 0.2 -- on
EdgeDiffusionDecoder(kernels="generic", autograd=True, train_dropout=True), next to the same build at p = 0 and a torch-eager
restatement with dropout_p = 0.2 in both attentions and F.dropout at the two FFN sites (scratch/train_time.py's decoder).

    python scratch/train_dropout_time.py [--out FILE.json] [--reps 20] [--shapes 8x173x100,64x512x256] [--only-p0] [--one-step]

--only-p0   time only the p = 0 step and pass no train_dropout keyword: the form that also runs on a checkout from before the
            option existed (EDTTS_PKG_ROOT names that checkout's package directory), for the same-session comparison.
--one-step  a single warmed p = 0.2 step and nothing else (the process to put under a kernel trace)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.environ.get("EDTTS_PKG_ROOT", os.path.join(REPO, "edge-diffusion-tts_amd")))
sys.path.insert(0, HERE)
from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, synth_state_dict  # noqa: E402
import train_time as tt  # noqa: E402

DEV = "cuda"


class DropBlock(tt.Block):
    """scratch/train_time.py's block with the reference's four dropout sites."""
    p = 0.2

    def forward(self, h, ctx, cond, mask):
        B, T, H = h.shape
        p = self.p if self.training else 0.0
        q, k, v = (self.split(u) for u in self.qkv(self.norm1(h, cond)).chunk(3, dim=-1))
        a = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=p)
        h = h + self.proj(a.transpose(1, 2).reshape(B, T, H))
        q = self.split(self.q_proj(self.norm2(h)))
        k, v = (self.split(u) for u in self.kv_up(self.kv_norm(self.kv_down(ctx))).chunk(2, dim=-1))
        a = F.scaled_dot_product_attention(q, k, v, dropout_p=p)
        h = h + self.out_proj(a.transpose(1, 2).reshape(B, T, H))
        val, gate = self.up(self.norm3(h, cond)).chunk(2, dim=-1)
        return h + F.dropout(self.down(F.dropout(val * F.silu(gate), p, self.training)), p, self.training)


def ours(cfg_kw, **kw):
    cfg = CFG(device=DEV, **cfg_kw)
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, **kw)
    dec.load_state_dict(synth_state_dict(cfg, 0))
    return cfg, dec.to(DEV).train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="8x173x100,64x512x256")
    ap.add_argument("--only-p0", action="store_true")
    ap.add_argument("--one-step", action="store_true")
    a = ap.parse_args()
    decs = {}
    if a.only_p0:
        cfg, decs["ours_p0"] = ours(dict(dropout=0.0))
    else:
        cfg, decs["ours_drop"] = ours(dict(dropout=0.2), train_dropout=True)
        if not a.one_step:
            _, decs["ours_p0"] = ours(dict(dropout=0.0), train_dropout=True)
            decs["eager_p0"] = tt.EagerDecoder(cfg).to(DEV).train()
            e = tt.EagerDecoder(cfg).to(DEV).train()
            for b in e.blocks:  # (the same modules, the dropping block's forward)
                b.__class__ = DropBlock
            decs["eager_drop"] = e
    sch = DiffusionSchedule(cfg.diff_steps).to(DEV)
    results = []
    for shape in a.shapes.split(","):
        B, T, S = (int(v) for v in shape.split("x"))
        steps = {k: tt.make_step(d, sch, cfg, B, T, S, k.startswith("ours")) for k, d in decs.items()}
        for s in steps.values():
            for _ in range(a.warmup):
                s()
        torch.cuda.synchronize()
        if a.one_step:
            print(f"one step at {shape}: loss {float(steps['ours_drop']()):.4f}")
            torch.cuda.synchronize()
            continue
        ms = {k: [] for k in steps}
        for order in (list(steps), list(steps)[::-1]):
            for k in order:
                ms[k].append(statistics.median(tt.timed(steps[k], a.reps)))
        r = dict(B=B, T=T, S=S, **{k + "_ms_by_order": v for k, v in ms.items()}, **{k + "_ms": statistics.median(v) for k, v in ms.items()})
        print(json.dumps(r))
        results.append(r)
    if a.out and results:
        with open(a.out, "w") as f:
            json.dump(dict(model="hidden 160, heads 4, n_mels 80, layers 4, window 64, fp32", device=torch.cuda.get_device_name(0),
                           reps=a.reps, warmup=a.warmup, results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
