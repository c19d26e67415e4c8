"""GPU tests of the semantic head (csrc/edtts_semantic.h) against the reference's own FSQ / VQ encoder (tests/golden/semantic_*.npz,
made by tests/golden/make_golden_semantic.py), plus properties and the end-to-end path into the samplers.

Parity protocol: idx equals the reference on every frame whose decision margin (fp64) is >= 1e-4; z and z_q,
on frames with equal idx, are within 4x the reference fp32's own max-abs error against its fp64 run; `used` is exact and perplexity
matches the reference's formulas on the kernel's idx to 1e-6 relative."""
import pytest
import torch

from edge_diffusion_tts_amd import CFG, DiffusionSchedule, DPMSolverPP, EdgeDiffusionDecoder, EdgeInference, FSQ, SemanticEncoder, native
from edge_diffusion_tts_amd.synth import HubertStandIn, synth_hubert_features, synth_semantic_head, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ["semantic_fsq_default", "semantic_fsq_85555", "semantic_vq_512", "semantic_fsq_small", "semantic_vq_small"]
HOP = 320


def make_encoder(g, hubert=True):
    in_dim, S, K, B, T, seed, dropout = (int(v) for v in g["shape"])
    levels = [int(v) for v in g["levels"]] or None
    proj_sd, q_sd = synth_semantic_head(in_dim, S, levels, K, seed, bool(dropout))
    key = "encoder_fsq" if levels else "encoder_vq"
    enc = SemanticEncoder.from_checkpoint({"encoder_proj": proj_sd, key: q_sd}, hubert=HubertStandIn(in_dim, seed) if hubert else None,
                                          device=DEV)
    return enc, (in_dim, S, K, B, T, seed, levels)


def ref_stats(idx, n_codes):
    """fsq.py:189-193 / vq.py:101-105 on CPU, fp32"""
    counts = torch.bincount(idx.flatten().cpu(), minlength=n_codes).float()
    probs = counts / counts.sum().clamp_min(1.0)
    return torch.exp(-(probs * torch.log(probs.clamp_min(1e-12))).sum()), (counts > 0).sum()


@pytest.mark.parametrize("case", CASES)
def test_parity_with_the_reference(golden, case):
    g = golden(case)
    enc, (in_dim, S, K, B, T, seed, levels) = make_encoder(g)
    wav = torch.zeros(B, T * HOP, device=DEV)
    zq, idx, loss, ppl, used = enc(wav)
    h = synth_hubert_features(B, T, in_dim, seed).to(DEV)
    idx2, z, zq2, _ = native.sem_encode(enc._dims(), enc._pack.get(enc._dims(), enc._slots()), h, want_z=True)
    assert torch.equal(idx, idx2) and torch.equal(zq, zq2)
    assert zq.shape == (B, T, S) and idx.shape == (B, T) and float(loss) == 0.0
    idx, zq, z = idx.cpu(), zq.cpu(), z.cpu()
    sure = g["margin"] >= 1e-4
    unsure = int((~sure).sum())
    print(f"{case}: {unsure} frames below the 1e-4 margin, {int((idx != g['idx']).sum())} idx differences in all")
    assert torch.equal(idx[sure], g["idx"][sure])
    assert unsure <= 8
    eq = idx == g["idx"]
    for name, mine, ref32, ref64 in (("z", z, g["z"], g["z64"]), ("z_q", zq, g["zq"], g["zq64"])):
        own = float((ref32.double() - ref64)[eq].abs().max())
        err = float((mine.double() - ref64)[eq].abs().max())
        print(f"  {name}: kernel max-abs {err:.3e}, reference fp32 {own:.3e}")
        assert err <= 4 * own, f"{name}: {err} > 4 x {own}"
    n_codes = enc.codebook_size
    p_ref, u_ref = ref_stats(idx, n_codes)
    assert int(used) == int(u_ref)
    assert abs(float(ppl) - float(p_ref)) <= 1e-6 * float(p_ref)
    assert torch.equal(enc.encode(wav).cpu(), idx)


@pytest.mark.parametrize("case", CASES)
def test_decode_every_code(golden, case):
    g = golden(case)
    enc, (in_dim, S, K, B, T, seed, levels) = make_encoder(g, hubert=False)
    n = enc.codebook_size
    ids = torch.arange(n, device=DEV)
    dec = enc.decode_tokens(ids).cpu()
    if levels is None:
        assert torch.equal(dec, enc.vq.codebook.weight.detach().cpu())  # the gather is bitwise
        assert torch.equal(enc.vq.decode(ids.view(4, -1) if n % 4 == 0 else ids).cpu().reshape(n, S), dec)
    else:
        up_w = enc.vq.proj_up.weight.detach().cpu().double()
        up_b = enc.vq.proj_up.bias.detach().cpu().double()
        want64 = g["codes"].double() @ up_w.t() + up_b   # proj_up of the reference's indices_to_codes, fp64
        want32 = g["codes"] @ up_w.float().t() + up_b.float()
        own = float((want32.double() - want64).abs().max())
        assert float((dec.double() - want64).abs().max()) <= max(4 * own, 1e-6)
        codes = FSQ(levels).to(DEV).indices_to_codes(ids).cpu()
        assert torch.equal(codes, g["codes"])
    sub = enc.decode_tokens(g["dec_ids"].to(DEV)).cpu()
    own = float((g["dec"].double() - g["dec64"]).abs().max())
    assert float((sub.double() - g["dec64"]).abs().max()) <= max(4 * own, 1e-6)


def test_decode_out_of_range_ids_clamp_or_raise(golden, monkeypatch):
    enc, _ = make_encoder(golden("semantic_vq_small"), hubert=False)
    ids = torch.tensor([-3, 0, 999, 1000, 5000], device=DEV)
    out = enc.decode_tokens(ids).cpu()
    w = enc.vq.codebook.weight.detach().cpu()
    assert torch.equal(out, w[[0, 0, 999, 999, 999]])
    monkeypatch.setattr(native, "CHECK_INDICES", True)
    with pytest.raises(IndexError):
        enc.decode_tokens(ids)


@pytest.mark.parametrize("case", ["semantic_fsq_default", "semantic_vq_512"])
def test_properties(golden, case):
    g = golden(case)
    enc, (in_dim, S, K, B, T, seed, levels) = make_encoder(g, hubert=False)
    h = synth_hubert_features(3, 150, in_dim, seed + 7).to(DEV)
    zq, idx, ppl, used = enc.quantize_features(h)
    zq_b, idx_b, ppl_b, used_b = enc.quantize_features(h)
    assert torch.equal(zq, zq_b) and torch.equal(idx, idx_b) and torch.equal(ppl, ppl_b) and torch.equal(used, used_b)
    for b in range(3):  # a row alone is bitwise the same row in the batch
        zq1, idx1, _, _ = enc.quantize_features(h[b:b + 1].clone())
        assert torch.equal(zq1[0], zq[b]) and torch.equal(idx1[0], idx[b])
    # lengths: a row equals the unpadded call on that row; padded frames are 0 and not counted
    lens = torch.tensor([150, 37, 101])
    zq_l, idx_l, ppl_l, used_l = enc.quantize_features(h, lens)
    kept = []
    for b, n in enumerate(lens.tolist()):
        zq1, idx1, _, _ = enc.quantize_features(h[b:b + 1, :n].clone())
        assert torch.equal(zq_l[b, :n], zq1[0]) and torch.equal(idx_l[b, :n], idx1[0])
        assert int(idx_l[b, n:].abs().sum()) == 0 and float(zq_l[b, n:].abs().sum()) == 0.0
        kept.append(idx1[0])
    p_ref, u_ref = ref_stats(torch.cat(kept), enc.codebook_size)
    assert int(used_l) == int(u_ref) and abs(float(ppl_l) - float(p_ref)) <= 1e-6 * float(p_ref)
    assert torch.equal(enc.encode_features(h, lens.to(DEV)), idx_l)
    # a captured graph replays bitwise what the eager call computed (one stream, no parallel branches)
    static_h = h.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_zq, g_idx, g_ppl, g_used = enc.quantize_features(static_h)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_zq, zq) and torch.equal(g_idx, idx) and torch.equal(g_ppl, ppl) and torch.equal(g_used, used)
    static_h.copy_(synth_hubert_features(3, 150, in_dim, seed + 8).to(DEV))
    graph.replay()
    want = enc.quantize_features(static_h)
    torch.cuda.synchronize()
    assert torch.equal(g_idx, want[1]) and torch.equal(g_zq, want[0])


def test_standalone_quantizers_match_the_head(golden):
    enc, (in_dim, S, K, B, T, seed, levels) = make_encoder(golden("semantic_fsq_default"), hubert=False)
    h = synth_hubert_features(2, 64, in_dim, 3).to(DEV)
    idx, z, zq, counts = native.sem_encode(enc._dims(), enc._pack.get(enc._dims(), enc._slots()), h, want_z=True)
    zq2, idx2, loss, ppl, used = enc.vq(z)
    assert torch.equal(idx2, idx) and torch.equal(zq2, zq) and torch.equal(enc.vq.encode(z), idx)
    # FSQ alone: tanh / round / index of proj_down(z), against torch on the same device
    u = torch.nn.functional.linear(z, enc.vq.proj_down.weight, enc.vq.proj_down.bias)
    zl, ix = enc.vq.fsq(u)
    zb = torch.tanh(u)
    half = (torch.tensor(levels, device=DEV, dtype=torch.float32) - 1) / 2
    q = torch.minimum(torch.clamp(torch.round((zb + 1) * half), min=0), half * 2) / half - 1
    frames = (q == zl).all(-1)
    assert float(frames.float().mean()) > 0.99  # (tanh may differ in the last bit next to a rounding boundary)
    basis = enc.vq.fsq._basis
    assert torch.equal(ix[frames], (torch.round((zl + 1) * half).long() * basis).sum(-1)[frames])


def test_generate_from_audio_with_the_semantic_encoder(golden):
    """SemanticEncoder -> EdgeInference.generate_from_audio equals generate_mel on the encoder's idx (bitwise)."""
    cfg = CFG(device=DEV)
    enc, (in_dim, S, K, B, T, seed, levels) = make_encoder(golden("semantic_fsq_default"))
    cfg.codebook_size = enc.codebook_size
    dec = EdgeDiffusionDecoder(cfg)
    dec.load_state_dict(synth_state_dict(cfg, 0))
    dec = dec.to(DEV).eval()
    infer = EdgeInference(cfg, DiffusionSchedule(cfg.diff_steps).to(DEV), enc, dec)
    wav = torch.zeros(2, 40 * HOP)
    torch.manual_seed(5)
    out = infer.generate_from_audio(wav, num_steps=4)
    idx = enc.encode(wav.to(DEV))
    torch.manual_seed(5)
    assert out.shape == (2, 80, cfg.n_mels) and torch.equal(out, infer.generate_mel(idx, 4))
    # z_q is accepted as sem_features by DPMSolverPP.sample
    zq, _, _, _, _ = enc(wav.to(DEV))
    x_T = torch.randn(2, 80, cfg.n_mels, device=DEV)
    x0 = DPMSolverPP(DiffusionSchedule(cfg.diff_steps).to(DEV)).sample(dec, x_T, zq, num_steps=4)
    assert x0.shape == x_T.shape and bool(torch.isfinite(x0).all())


def test_tiny_random_hubert_model():
    transformers = pytest.importorskip("transformers")
    conf = transformers.HubertConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                                     conv_dim=(32, 32), conv_stride=(5, 2), conv_kernel=(10, 3), num_conv_pos_embeddings=16,
                                     num_conv_pos_embedding_groups=4, do_stable_layer_norm=False)
    torch.manual_seed(0)
    hub = transformers.HubertModel(conf).eval()
    cfg = CFG(device=DEV, semantic_dim=64, fsq_levels=[7, 5, 3], hubert_layer=2)
    enc = SemanticEncoder(cfg, hubert=hub, in_dim=64).to(DEV).eval()
    wav = torch.randn(2, 4000, device=DEV)
    zq, idx, loss, ppl, used = enc(wav)
    n_feat = hub._get_feat_extract_output_lengths(torch.tensor(4000)).item()
    assert idx.shape == (2, n_feat) and zq.shape == (2, n_feat, 64) and bool(torch.isfinite(zq).all())
    assert int(idx.min()) >= 0 and int(idx.max()) < 105 and 1 <= int(used) <= 105
