"""Generate tests/golden/hubert_small.npz: a small random HuBERT (hubert-base layout) and transformers' own outputs.

The model is transformers.HubertModel with every parameter redrawn from a seeded generator (GroupNorm / LayerNorm gains and biases and
the positional conv's weight-norm g included) and rounded to fp16-representable values, so the weights are stored losslessly as fp16
(the file stays small).  The input is a B = 3 batch of 4800 samples with per-utterance lengths 4800, 4000 and 3200.

Stored: the config (JSON), the weights ("w:" + state-dict key, fp16), wav, lengths, and for num_layers n = 0 .. 3
  pad32_n / pad64_n     hidden_states[n] of the padded batch, fp32 and fp64 (CPU)
  solo32_n_b / solo64_n_b  hidden_states[n] of wav[b, :lengths[b]] alone, fp32 and fp64

Run from the repository root: python tests/golden/make_golden_hubert.py
"""
import json
import os

import numpy as np
import torch

CONFIG = dict(conv_dim=[32] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=64,
              num_attention_heads=2, intermediate_size=128, num_hidden_layers=3, num_conv_pos_embeddings=16,
              num_conv_pos_embedding_groups=4)
LENGTHS = [4800, 4000, 3200]


def redraw(model, seed):
    """Every parameter from a seeded generator: gains around 1, biases around 0, matrices ~ 1/sqrt(fan_in), weight-norm g in [1, 3]."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "original0" in name or name.endswith("weight_g"):
                v = 1.0 + 2.0 * torch.rand(p.shape, generator=g)
            elif p.dim() == 1 and name.endswith("weight"):
                v = 1.0 + 0.2 * torch.randn(p.shape, generator=g)
            elif p.dim() == 1:
                v = 0.1 * torch.randn(p.shape, generator=g)
            else:
                fan_in = p[0].numel()
                v = torch.randn(p.shape, generator=g) / fan_in ** 0.5
            p.copy_(v.half().float())
    return model


def main():
    from transformers import HubertConfig, HubertModel
    torch.manual_seed(0)
    model = redraw(HubertModel(HubertConfig(**CONFIG)).eval(), 1234)
    g = torch.Generator().manual_seed(99)
    T = max(LENGTHS)
    wav = (0.1 * torch.randn(len(LENGTHS), T, generator=g)).half().float()
    out = {"config": np.frombuffer(json.dumps(CONFIG).encode(), dtype=np.uint8), "wav": wav.numpy().astype(np.float16),
           "lengths": np.array(LENGTHS, dtype=np.int64)}
    for k, v in model.state_dict().items():
        if k != "masked_spec_embed":
            out["w:" + k] = v.numpy().astype(np.float16)
    m64 = HubertModel(HubertConfig(**CONFIG)).eval()
    m64.load_state_dict(model.state_dict())
    m64 = m64.double()
    with torch.no_grad():
        for prec, m, x in (("32", model, wav), ("64", m64, wav.double())):
            hs = m(x, output_hidden_states=True).hidden_states
            for n in range(CONFIG["num_hidden_layers"] + 1):
                out[f"pad{prec}_{n}"] = hs[n].numpy()
            for b, L in enumerate(LENGTHS):
                hs = m(x[b:b + 1, :L], output_hidden_states=True).hidden_states
                for n in range(CONFIG["num_hidden_layers"] + 1):
                    out[f"solo{prec}_{n}_{b}"] = hs[n][0].numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hubert_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
