#!/usr/bin/env python3
"""tests/golden/semantic_*.npz: the REFERENCE's semantic head (models/encoder.py SemanticEncoder, models/fsq.py FSQ / FSQEncoder,
models/vq.py VectorQuantizer) run on CPU, in fp32 and in fp64 (build container only; the reference never travels to the GPU box).

    python tests/golden/make_golden_semantic.py

The reference's SemanticEncoder.__init__ downloads HuBERT, so the encoder is assembled around it: nn.Module.__init__, then cfg,
proj (the reference's layer sequence, built from torch.nn), the reference's own quantizer and a deterministic HuBERT stand-in
(edge_diffusion_tts_amd.synth.HubertStandIn).  Weights and features come from synth.synth_semantic_head / synth_hubert_features
(hash_uniform), so the files hold outputs only.  Per case:
  idx, z, z_q, perplexity, used      SemanticEncoder.forward in fp32 (z: the proj output)
  idx64, z64, zq64                   the same encoder in fp64
  margin                             per frame: FSQ min over dims |frac((zb + 1) half) - 0.5|, VQ second-best - best distance (fp64)
  dec_ids, dec                       decode_tokens on a spread of ids (fp32); dec64 in fp64
  codes                              FSQ: fsq.indices_to_codes of every id (the reference's digit order)
"""
import os
import sys
import tempfile
import types

os.environ["HF_HUB_OFFLINE"] = "1"  # before the reference package imports transformers
os.environ["TRANSFORMERS_OFFLINE"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(REPO, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "edge-diffusion-tts_amd"))
sys.path.insert(0, "/root/reference")
os.chdir(tempfile.mkdtemp(prefix="edtts_golden_"))
torch.set_num_threads(8)

from edge_diffusion_tts.models.encoder import SemanticEncoder as RefSemanticEncoder  # noqa: E402
from edge_diffusion_tts.models.fsq import FSQEncoder as RefFSQEncoder  # noqa: E402
from edge_diffusion_tts.models.vq import VectorQuantizer as RefVQ  # noqa: E402
from edge_diffusion_tts_amd.synth import HubertStandIn, synth_semantic_head  # noqa: E402

# name: (in_dim, semantic_dim, levels or None, codebook_size, B, T_feat, seed, dropout layout)
CASES = {
    "semantic_fsq_default": (768, 128, [4, 4, 3, 3, 2, 2, 2, 2], 0, 2, 120, 1, False),
    "semantic_fsq_85555": (768, 128, [8, 6, 5, 5, 5], 0, 2, 120, 2, True),
    "semantic_vq_512": (768, 128, None, 512, 2, 200, 3, False),
    "semantic_fsq_small": (256, 64, [7, 5, 3], 0, 2, 100, 4, False),
    "semantic_vq_small": (256, 64, None, 1000, 2, 200, 5, True),
}
HOP = 320  # samples per HuBERT frame


def build(in_dim, S, levels, K, seed, dropout_layout):
    proj_sd, q_sd = synth_semantic_head(in_dim, S, levels, K, seed, dropout_layout)
    mods = [nn.Linear(in_dim, S), nn.GELU(), nn.LayerNorm(S)] + ([nn.Dropout(0.2)] if dropout_layout else []) + [nn.Linear(S, S)]
    proj = nn.Sequential(*mods)
    proj.load_state_dict(proj_sd)
    vq = RefFSQEncoder(S, levels) if levels is not None else RefVQ(S, K)
    vq.load_state_dict(q_sd)
    enc = RefSemanticEncoder.__new__(RefSemanticEncoder)
    nn.Module.__init__(enc)
    enc.cfg = types.SimpleNamespace(hubert_layer=9)
    enc.hubert = HubertStandIn(in_dim, seed)
    enc.proj = proj
    enc.vq = vq
    enc.codebook_size = vq.codebook_size
    return enc.eval()


@torch.no_grad()
def run(name, in_dim, S, levels, K, B, T, seed, dropout_layout):
    wav = torch.zeros(B, T * HOP)
    out = {}
    for tag, dt in (("", torch.float32), ("64", torch.float64)):
        enc = build(in_dim, S, levels, K, seed, dropout_layout).to(dt)
        h = enc.extract_hubert(wav).to(dt)
        z = enc.proj(h)
        zq, idx, loss, ppl, used = enc.forward(wav.to(dt)) if dt == torch.float32 else enc.vq(z)
        assert torch.equal(enc.encode(wav.to(dt)) if dt == torch.float32 else enc.vq.encode(z), idx)
        out["idx" + tag], out["z" + tag], out["zq" + tag] = idx, z, zq
        if dt == torch.float32:
            out["perplexity"], out["used"] = ppl, used
        n = enc.codebook_size
        ids = torch.unique(torch.cat([torch.arange(0, n, max(1, n // 61)), torch.tensor([n - 1])]))
        if dt == torch.float64 and levels is not None:  # (indices_to_codes returns fp32 whatever the module's dtype)
            dec = enc.vq.proj_up(enc.vq.fsq.indices_to_codes(ids).double())
        else:
            dec = enc.decode_tokens(ids)
        out["dec_ids"], out["dec" + tag] = ids, dec
        if dt == torch.float64:
            if levels is not None:
                zb = torch.tanh(enc.vq.proj_down(z))
                half = (torch.tensor(levels, dtype=torch.float64) - 1) / 2
                s = (zb + 1) * half
                out["margin"] = ((s - torch.floor(s)) - 0.5).abs().min(-1).values
                out["codes"] = enc.vq.fsq.indices_to_codes(torch.arange(n)).float()
            else:
                c = enc.vq.codebook.weight
                flat = z.reshape(-1, S)
                d = flat.pow(2).sum(1, keepdim=True) - 2 * flat @ c.t() + c.pow(2).sum(1)[None]
                two = d.topk(2, dim=1, largest=False).values
                out["margin"] = (two[:, 1] - two[:, 0]).reshape(B, T)
    # the fixture has to exercise the quantizer: every FSQ dimension takes every level, VQ uses >= 100 codes
    idx = out["idx"].flatten()
    if levels is not None:
        digits, rem = [], idx.clone()
        for L in levels:  # codes_to_indices basis: the first level is the least significant digit
            digits.append(rem % L)
            rem = rem // L
        for d, L in enumerate(levels):
            assert len(torch.unique(digits[d])) == L, f"{name}: dim {d} takes {len(torch.unique(digits[d]))} of {L} levels"
    else:
        assert len(torch.unique(idx)) >= 100, f"{name}: only {len(torch.unique(idx))} distinct codes"
    m = out["margin"].flatten()
    print(f"{name}: {idx.numel()} frames, {len(torch.unique(idx))} distinct ids, used {int(out['used'])}, perplexity "
          f"{float(out['perplexity']):.2f}, fp32 vs fp64 idx mismatches {int((out['idx'] != out['idx64']).sum())}, "
          f"frames with margin < 1e-4: {int((m < 1e-4).sum())}")
    save = {k: (v.numpy() if v.dtype != torch.float64 or k in ("z64", "zq64", "dec64", "margin") else v.float().numpy())
            for k, v in out.items()}
    save["shape"] = np.array([in_dim, S, K, B, T, seed, int(dropout_layout)])
    save["levels"] = np.array(levels if levels is not None else [], dtype=np.int64)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **save)
    print(f"  {os.path.basename(path)}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    for name, args in CASES.items():
        run(name, *args)
