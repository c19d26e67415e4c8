"""GPU tests of NativeHubert(compute_dtype="bf16") (csrc/edtts_hubert16.h).

Parity protocol: the yardstick is transformers' own bf16 run -- the same fp32 HubertModel in eval mode under
torch.autocast("cpu", dtype=torch.bfloat16) -- and both are compared with the fp64 twin on the CPU:
    E_max = max|out - fp64|,  E_rms = sqrt(mean((out - fp64)^2));   bar: ours <= 1.0 x the autocast run's, for both.
No margin: the autocast run also rounds the residual stream, the norms, GELU, the softmax and the output to bf16, which this path keeps
in fp32.  The small fixture (tests/golden/hubert_small_bf16.npz, make_golden_hubert_bf16.py) runs without transformers.  Invariances
(batch rows, per-utterance lengths, graphs, streams) are bitwise, as for fp32."""
import json
import os

import numpy as np
import pytest
import torch

from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, EdgeInference, NativeHubert, SemanticEncoder
from edge_diffusion_tts_amd.synth import synth_semantic_head, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "hubert_small.npz")
GOLDEN16 = os.path.join(HERE, "golden", "hubert_small_bf16.npz")
BAR = 1.0


def errs(out, ref):
    e = out.double() - ref.double()
    return float(e.abs().max()), float((e * e).mean().sqrt())


def small():
    z = np.load(GOLDEN)
    cfg = json.loads(bytes(z["config"]).decode())
    sd = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w:")}
    return z, cfg, sd


def small_model(n, compute_dtype="bf16"):
    z, cfg, sd = small()
    m = NativeHubert(cfg, n, compute_dtype=compute_dtype)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def redraw(model, seed):
    """Every parameter from a seeded generator (as tests/test_hubert_gpu.py)."""
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
    """HubertModel(HubertConfig()) with every parameter redrawn, and its fp64 twin (CPU) -- as tests/test_hubert_gpu.py builds them."""
    if not _BASE:
        transformers = pytest.importorskip("transformers")
        torch.manual_seed(0)
        m32 = redraw(transformers.HubertModel(transformers.HubertConfig()).eval(), 77)
        m64 = transformers.HubertModel(transformers.HubertConfig()).eval()
        m64.load_state_dict(m32.state_dict())
        _BASE["m"] = (m32, m64.double())
    return _BASE["m"]


def autocast_states(m32, wav):
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        return [h.float() for h in m32(wav, output_hidden_states=True).hidden_states]


def check(tag, out, auto, ref):
    """Print ours, the autocast run's and the ratio, then hold the bar on both figures."""
    (em, er), (am, ar) = errs(out, ref), errs(auto, ref)
    print(f"{tag}: E_max ours {em:.3e} autocast {am:.3e} ratio {em / am:.3f} | E_rms ours {er:.3e} autocast {ar:.3e} ratio {er / ar:.3f}")
    assert em <= BAR * am and er <= BAR * ar, tag
    return em


@pytest.mark.parametrize("n", [0, 1, 3])
def test_small_fixture_against_autocast(n):
    z, cfg, sd = small()
    z16 = np.load(GOLDEN16)
    wav = torch.from_numpy(z["wav"].astype(np.float32))
    out = small_model(n)(wav.to(DEV)).cpu()
    ref = torch.from_numpy(z[f"pad64_{n}"])
    assert out.shape == ref.shape and out.dtype == torch.float32
    em = check(f"hubert_small bf16 num_layers={n}", out, torch.from_numpy(z16[f"pad16_{n}"]), ref)
    # the bf16 path is really taken: far from the fp32 path's error
    e32, _ = errs(small_model(n, "fp32")(wav.to(DEV)).cpu(), ref)
    print(f"hubert_small num_layers={n}: fp32 path E_max {e32:.3e}, bf16 / fp32 {em / e32:.0f}")
    assert em > 100 * e32


def test_small_fixture_ragged_and_invariance():
    z, cfg, sd = small()
    z16 = np.load(GOLDEN16)
    m = small_model(3)
    wav = torch.from_numpy(z["wav"].astype(np.float32)).to(DEV)
    lens = torch.from_numpy(z["lengths"])
    B, T_audio = wav.shape
    full = m(wav)
    for b in range(B):  # row b of the padded batch is the B = 1 call on that row
        assert torch.equal(m(wav[b:b + 1].clone())[0], full[b])
    out = m(wav, lens)
    junk = wav.clone()
    for b, L in enumerate(lens.tolist()):
        junk[b, L:] = float("nan") if b % 2 else 1e4
    assert torch.equal(out, m(junk, lens.to(DEV)))
    for b, L in enumerate(lens.tolist()):
        F = m.frames(L)
        solo = m(wav[b:b + 1, :L].clone())[0]
        assert solo.shape[0] == F
        assert torch.equal(out[b, :F], solo), f"row {b}"
        assert float(out[b, F:].abs().sum()) == 0.0
        check(f"hubert_small bf16 ragged row {b} ({L} samples, {F} frames)", solo.cpu(), torch.from_numpy(z16[f"solo16_3_{b}"]),
              torch.from_numpy(z[f"solo64_3_{b}"]))


@pytest.mark.parametrize("T_audio", [32000, 33333])
def test_hubert_base_shape(T_audio):
    m32, m64 = hubert_base()
    g = torch.Generator().manual_seed(T_audio)
    wav = 0.1 * torch.randn(2, T_audio, generator=g)
    with torch.no_grad():
        hs64 = m64(wav.double(), output_hidden_states=True).hidden_states
    hs16 = autocast_states(m32, wav)
    for n in (9, 12):
        nat = NativeHubert.from_hubert(m32, n, compute_dtype="bf16").to(DEV)
        out = nat(wav.to(DEV)).cpu()
        assert out.shape == hs64[n].shape and out.dtype == torch.float32
        em = check(f"hubert-base bf16 T_audio={T_audio} num_layers={n}", out, hs16[n], hs64[n])
        e32, _ = errs(NativeHubert.from_hubert(m32, n).to(DEV)(wav.to(DEV)).cpu(), hs64[n])
        print(f"hubert-base T_audio={T_audio} num_layers={n}: fp32 path E_max {e32:.3e}, bf16 / fp32 {em / e32:.0f}")
        assert em > 100 * e32


def _vq_head(hub):
    cfg = CFG(device=DEV, use_fsq=False)
    proj_sd, q_sd = synth_semantic_head(768, cfg.semantic_dim, None, 512, 11, False)
    enc = SemanticEncoder.from_checkpoint({"encoder_proj": proj_sd, "encoder_vq": q_sd}, cfg=cfg, hubert=hub, device=DEV)
    return enc, proj_sd, q_sd


def _head64(h, proj_sd, q_sd):
    """The VQ-512 head of tests/test_hubert_gpu.py in fp64: nearest code of every frame."""
    p = {k: v.double() for k, v in proj_sd.items()}
    y = torch.nn.functional.gelu(h.double() @ p["0.weight"].T + p["0.bias"])
    y = torch.nn.functional.layer_norm(y, (y.shape[-1],), p["2.weight"], p["2.bias"], 1e-5)
    zz = y @ p["3.weight"].T + p["3.bias"]
    cb = q_sd["codebook.weight"].double()
    dist = (zz * zz).sum(-1, keepdim=True) - 2 * zz @ cb.T + (cb * cb).sum(-1)
    return dist.argmin(-1)


def test_tokens_through_the_semantic_encoder():
    m32, m64 = hubert_base()
    nat = NativeHubert.from_hubert(m32, 9, compute_dtype="bf16")
    enc, proj_sd, q_sd = _vq_head(nat)
    ours = auto = frames = 0
    for seed in (3, 4, 5):
        g = torch.Generator().manual_seed(seed)
        wav = 0.1 * torch.randn(8, 32000, generator=g)
        idx = enc.encode(wav.to(DEV)).cpu()
        with torch.no_grad():
            want = _head64(m64(wav.double(), output_hidden_states=True).hidden_states[9], proj_sd, q_sd)
            got16 = _head64(autocast_states(m32, wav)[9], proj_sd, q_sd)
        o, a = int((idx != want).sum()), int((got16 != want).sum())
        print(f"tokens seed {seed}: {want.numel()} frames, mismatches against fp64: ours {o}, autocast {a}")
        ours, auto, frames = ours + o, auto + a, frames + want.numel()
    print(f"tokens: {frames} frames, mismatches ours {ours}, autocast {auto}")
    assert frames == 2376 and ours <= auto
    # generate_from_audio through the bf16 encoder equals generate_mel(encode(wav)), bitwise
    wav = wav[:2]
    idx = enc.encode(wav.to(DEV))
    cfg = CFG(device=DEV)
    cfg.codebook_size = enc.codebook_size
    dec = EdgeDiffusionDecoder(cfg)
    dec.load_state_dict(synth_state_dict(cfg, 0))
    dec = dec.to(DEV).eval()
    infer = EdgeInference(cfg, DiffusionSchedule(cfg.diff_steps).to(DEV), enc, dec)
    torch.manual_seed(5)
    out = infer.generate_from_audio(wav, num_steps=4)
    torch.manual_seed(5)
    assert torch.equal(out, infer.generate_mel(idx, 4))


def _small_encoder(m):
    ccfg = CFG(device=DEV, use_fsq=False, hubert_layer=3)
    proj_sd, q_sd = synth_semantic_head(64, ccfg.semantic_dim, None, 64, 4, False)
    return SemanticEncoder.from_checkpoint({"encoder_proj": proj_sd, "encoder_vq": q_sd}, cfg=ccfg, hubert=m, device=DEV)


def test_semantic_encoder_lengths():
    m = small_model(3)
    z, cfg, sd = small()
    enc = _small_encoder(m)
    assert enc.hubert is m and m.compute_dtype == "bf16"
    wav = torch.from_numpy(z["wav"].astype(np.float32)).to(DEV)
    lens = torch.from_numpy(z["lengths"])
    idx = enc.encode(wav, lens)
    for b, L in enumerate(lens.tolist()):
        F = m.frames(L)
        assert torch.equal(idx[b, :F], enc.encode(wav[b:b + 1, :L].clone())[0])
        assert int(idx[b, F:].abs().sum()) == 0
    # the same errors as fp32 for inputs without a frame
    with pytest.raises(ValueError, match="no feature frame"):
        m(wav[:, :300])
    with pytest.raises(ValueError, match="no feature frame"):
        m(wav, torch.tensor([4800, 100, 4800]))


def test_graph_capture_and_two_streams():
    m = small_model(3)
    z, cfg, sd = small()
    enc = _small_encoder(m)
    wav = torch.from_numpy(z["wav"].astype(np.float32)).to(DEV)
    static = wav.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = enc.encode(static)  # warm-up: packs the weights, makes the workspace
        eager_h = m(static)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_idx = enc.encode(static)
        g_h = m(static)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_idx, eager) and torch.equal(g_h, eager_h)
    static.copy_(torch.flip(wav, [1]))
    graph.replay()
    want, want_h = enc.encode(static), m(static)
    torch.cuda.synchronize()
    assert torch.equal(g_idx, want) and torch.equal(g_h, want_h)
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


def test_fp32_and_bf16_modules_side_by_side():
    """An fp32 and a bf16 module of the same weights coexist: separate blobs and workspace caches, the fp32 result untouched by the
    bf16 calls in between."""
    z, cfg, sd = small()
    wav = torch.from_numpy(z["wav"].astype(np.float32)).to(DEV)
    f, h = small_model(3, "fp32"), small_model(3, "bf16")
    first = f(wav)
    for k in range(10):  # more shapes than WORKSPACE_CACHE holds, through both modules
        h(wav[:, :4000 + 16 * k].contiguous())
        f(wav[:, :4000 + 16 * k].contiguous())
    assert len(f._workspaces) <= f.WORKSPACE_CACHE and len(h._workspaces) <= h.WORKSPACE_CACHE
    assert torch.equal(f(wav), first) and not torch.equal(h(wav), first)
    assert f._packed().numel() > h._packed().numel()
