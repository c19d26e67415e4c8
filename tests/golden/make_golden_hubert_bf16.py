"""Generate tests/golden/hubert_small_bf16.npz: transformers' own bf16 run of the small HuBERT of hubert_small.npz.

Config, weights, waveform and lengths are read from hubert_small.npz (make_golden_hubert.py); the model is the same fp32 HubertModel in
eval mode, run under torch.autocast("cpu", dtype=torch.bfloat16) -- the yardstick of the bf16 compute path of NativeHubert
(tests/test_hubert_bf16_gpu.py: no worse than this run against the fp64 arrays of hubert_small.npz).

Stored, as fp32, for num_layers n = 0, 1, 3:
  pad16_n      hidden_states[n] of the padded batch
  solo16_n_b   hidden_states[n] of wav[b, :lengths[b]] alone

Run from the repository root: python tests/golden/make_golden_hubert_bf16.py
"""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LAYERS = (0, 1, 3)


def main():
    from transformers import HubertConfig, HubertModel
    z = np.load(os.path.join(HERE, "hubert_small.npz"))
    cfg = json.loads(bytes(z["config"]).decode())
    torch.manual_seed(0)
    model = HubertModel(HubertConfig(**cfg)).eval()
    sd = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w:")}
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"masked_spec_embed"}, res
    wav = torch.from_numpy(z["wav"].astype(np.float32))
    lengths = z["lengths"].tolist()
    out = {}
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        hs = model(wav, output_hidden_states=True).hidden_states
        for n in LAYERS:
            out[f"pad16_{n}"] = hs[n].float().numpy()
        for b, L in enumerate(lengths):
            hs = model(wav[b:b + 1, :L], output_hidden_states=True).hidden_states
            for n in LAYERS:
                out[f"solo16_{n}_{b}"] = hs[n][0].float().numpy()
    for n in LAYERS:
        ref = z[f"pad64_{n}"]
        e = out[f"pad16_{n}"].astype(np.float64) - ref
        print(f"num_layers={n}: autocast E_max {np.abs(e).max():.3e} E_rms {np.sqrt((e * e).mean()):.3e} (output rms {np.sqrt((ref * ref).mean()):.3f})")
    path = os.path.join(HERE, "hubert_small_bf16.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
