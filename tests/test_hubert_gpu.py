"""GPU tests of NativeHubert (csrc/edtts_hubert.h) against transformers' HubertModel.

Parity protocol (DESIGN.md sections 13 and 14): max-abs error against transformers in fp64 on the CPU is at most 4x transformers' own
fp32 error against the same fp64 run.  The small fixture (tests/golden/hubert_small.npz, tests/golden/make_golden_hubert.py) runs
without transformers; the full hubert-base shape needs it.  Invariances (batch rows, per-utterance lengths, graphs, streams) are
bitwise."""
import json
import os

import numpy as np
import pytest
import torch

from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, EdgeInference, NativeHubert, SemanticEncoder
from edge_diffusion_tts_amd.synth import synth_semantic_head, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hubert_small.npz")
BAR = 4.0


def small():
    z = np.load(GOLDEN)
    cfg = json.loads(bytes(z["config"]).decode())
    sd = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w:")}
    return z, cfg, sd


def small_model(n):
    z, cfg, sd = small()
    m = NativeHubert(cfg, n)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def redraw(model, seed):
    """Every parameter from a seeded generator (as tests/golden/make_golden_hubert.py): gains ~1, biases ~0, matrices ~1/sqrt(fan_in)."""
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
                v = torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5
            p.copy_(v)
    return model


_BASE = {}


def hubert_base():
    """HubertModel(HubertConfig()) with every parameter redrawn, and its fp64 twin (CPU)."""
    if not _BASE:
        transformers = pytest.importorskip("transformers")
        torch.manual_seed(0)
        m32 = redraw(transformers.HubertModel(transformers.HubertConfig()).eval(), 77)
        m64 = transformers.HubertModel(transformers.HubertConfig()).eval()
        m64.load_state_dict(m32.state_dict())
        _BASE["m"] = (m32, m64.double())
    return _BASE["m"]


@pytest.mark.parametrize("n", [0, 1, 3])
def test_small_fixture_against_fp64(n):
    z, cfg, sd = small()
    m = small_model(n)
    wav = torch.from_numpy(z["wav"].astype(np.float32))
    out = m(wav.to(DEV)).cpu().double()
    ref = torch.from_numpy(z[f"pad64_{n}"])
    err = float((out - ref).abs().max())
    own = float((torch.from_numpy(z[f"pad32_{n}"]).double() - ref).abs().max())
    print(f"hubert_small num_layers={n}: max-abs {err:.3e}, transformers fp32 {own:.3e}, ratio {err / own:.2f}")
    assert out.shape == ref.shape and err <= BAR * own


def test_small_fixture_ragged_and_invariance():
    z, cfg, sd = small()
    m = small_model(3)
    wav = torch.from_numpy(z["wav"].astype(np.float32)).to(DEV)
    lens = torch.from_numpy(z["lengths"])
    B, T_audio = wav.shape
    full = m(wav)
    # row b of the padded batch is the B = 1 call on that row
    for b in range(B):
        assert torch.equal(m(wav[b:b + 1].clone())[0], full[b])
    out = m(wav, lens)
    junk = wav.clone()
    for b, L in enumerate(lens.tolist()):
        junk[b, L:] = float("nan") if b % 2 else 1e4
    out_junk = m(junk, lens.to(DEV))
    assert torch.equal(out, out_junk)
    for b, L in enumerate(lens.tolist()):
        F = m.frames(L)
        solo = m(wav[b:b + 1, :L].clone())[0]
        assert solo.shape[0] == F
        assert torch.equal(out[b, :F], solo), f"row {b}"
        assert float(out[b, F:].abs().sum()) == 0.0
        ref = torch.from_numpy(z[f"solo64_3_{b}"])
        err = float((solo.cpu().double() - ref).abs().max())
        own = float((torch.from_numpy(z[f"solo32_3_{b}"]).double() - ref).abs().max())
        print(f"hubert_small ragged row {b} ({L} samples, {F} frames): max-abs {err:.3e}, transformers fp32 {own:.3e}")
        assert err <= BAR * own


@pytest.mark.parametrize("T_audio", [32000, 33333])
def test_hubert_base_shape(T_audio):
    m32, m64 = hubert_base()
    g = torch.Generator().manual_seed(T_audio)
    wav = 0.1 * torch.randn(2, T_audio, generator=g)
    with torch.no_grad():
        hs32 = m32(wav, output_hidden_states=True).hidden_states
        hs64 = m64(wav.double(), output_hidden_states=True).hidden_states
    for n in (9, 12):
        nat = NativeHubert.from_hubert(m32, n).to(DEV)
        out = nat(wav.to(DEV)).cpu().double()
        assert out.shape == hs64[n].shape and out.shape[1] == nat.frames(T_audio) == int(m32._get_feat_extract_output_lengths(T_audio))
        err = float((out - hs64[n]).abs().max())
        own = float((hs32[n].double() - hs64[n]).abs().max())
        print(f"hubert-base T_audio={T_audio} num_layers={n}: max-abs {err:.3e}, transformers fp32 {own:.3e}, ratio {err / own:.2f}")
        assert err <= BAR * own


def _vq_head(hub):
    cfg = CFG(device=DEV, use_fsq=False)
    proj_sd, q_sd = synth_semantic_head(768, cfg.semantic_dim, None, 512, 11, False)
    enc = SemanticEncoder.from_checkpoint({"encoder_proj": proj_sd, "encoder_vq": q_sd}, cfg=cfg, hubert=hub, device=DEV)
    return enc, proj_sd, q_sd


def test_tokens_through_the_semantic_encoder():
    m32, m64 = hubert_base()
    nat = NativeHubert.from_hubert(m32, 9)
    enc, proj_sd, q_sd = _vq_head(nat)
    g = torch.Generator().manual_seed(3)
    wav = 0.1 * torch.randn(2, 32000, generator=g)
    idx = enc.encode(wav.to(DEV)).cpu()
    with torch.no_grad():
        h = m64(wav.double(), output_hidden_states=True).hidden_states[9]
        p = {k: v.double() for k, v in proj_sd.items()}
        y = torch.nn.functional.gelu(h @ p["0.weight"].T + p["0.bias"])
        y = torch.nn.functional.layer_norm(y, (y.shape[-1],), p["2.weight"], p["2.bias"], 1e-5)
        zz = y @ p["3.weight"].T + p["3.bias"]
        cb = q_sd["codebook.weight"].double()
        dist = (zz * zz).sum(-1, keepdim=True) - 2 * zz @ cb.T + (cb * cb).sum(-1)
        top = dist.topk(2, dim=-1, largest=False)
    margin = top.values[..., 1] - top.values[..., 0]
    sure = margin >= 1e-4
    print(f"tokens: {int(sure.sum())} of {sure.numel()} frames with margin >= 1e-4, "
          f"{int((idx == top.indices[..., 0]).sum())} equal overall")
    assert torch.equal(idx[sure], top.indices[..., 0][sure])
    # generate_from_audio through it equals generate_mel(encode(wav)), bitwise
    cfg = CFG(device=DEV)
    cfg.codebook_size = enc.codebook_size
    dec = EdgeDiffusionDecoder(cfg)
    dec.load_state_dict(synth_state_dict(cfg, 0))
    dec = dec.to(DEV).eval()
    infer = EdgeInference(cfg, DiffusionSchedule(cfg.diff_steps).to(DEV), enc, dec)
    torch.manual_seed(5)
    out = infer.generate_from_audio(wav, num_steps=4)
    torch.manual_seed(5)
    assert torch.equal(out, infer.generate_mel(idx.to(DEV), 4))


def test_semantic_encoder_lengths():
    m = small_model(3)
    z, cfg, sd = small()
    from edge_diffusion_tts_amd import native
    ccfg = CFG(device=DEV, use_fsq=False, hubert_layer=3)
    proj_sd, q_sd = synth_semantic_head(64, ccfg.semantic_dim, None, 64, 4, False)
    enc = SemanticEncoder.from_checkpoint({"encoder_proj": proj_sd, "encoder_vq": q_sd}, cfg=ccfg, hubert=m, device=DEV)
    wav = torch.from_numpy(z["wav"].astype(np.float32)).to(DEV)
    lens = torch.from_numpy(z["lengths"])
    idx = enc.encode(wav, lens)
    for b, L in enumerate(lens.tolist()):
        F = m.frames(L)
        assert torch.equal(idx[b, :F], enc.encode(wav[b:b + 1, :L].clone())[0])
        assert int(idx[b, F:].abs().sum()) == 0
    with pytest.raises(ValueError):
        SemanticEncoder(CFG(device=DEV, hubert_layer=2), hubert=m, in_dim=64)
    assert isinstance(native.EdttsError("x"), RuntimeError)


def test_graph_capture_and_two_streams():
    m = small_model(3)
    z, cfg, sd = small()
    ccfg = CFG(device=DEV, use_fsq=False, hubert_layer=3)
    proj_sd, q_sd = synth_semantic_head(64, ccfg.semantic_dim, None, 64, 4, False)
    enc = SemanticEncoder.from_checkpoint({"encoder_proj": proj_sd, "encoder_vq": q_sd}, cfg=ccfg, hubert=m, device=DEV)
    wav = torch.from_numpy(z["wav"].astype(np.float32)).to(DEV)
    static = wav.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = enc.encode(static)  # warm-up: packs the weights, makes the workspace
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_idx = enc.encode(static)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_idx, eager)
    static.copy_(torch.flip(wav, [1]))
    graph.replay()
    want = enc.encode(static)
    torch.cuda.synchronize()
    assert torch.equal(g_idx, want)
    # two streams calling one module at once equal the calls made one after another
    a, b = wav, torch.flip(wav, [0]).contiguous()
    ra, rb = m(a), m(b)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    outs = {}
    for _ in range(3):
        with torch.cuda.stream(s1):
            outs["a"] = m(a)
        with torch.cuda.stream(s2):
            outs["b"] = m(b)
    torch.cuda.synchronize()
    assert torch.equal(outs["a"], ra) and torch.equal(outs["b"], rb)
