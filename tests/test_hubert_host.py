"""Host tests of NativeHubert (no GPU): frame counts, layout checks, size queries, state-dict forms, no CPU path."""
import pytest
import torch

from edge_diffusion_tts_amd import NativeHubert, SemanticEncoder, CFG, native

transformers = pytest.importorskip("transformers")
SMALL = dict(conv_dim=[32] * 7, hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=3,
             num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)


def test_frames_match_transformers():
    model = transformers.HubertModel(transformers.HubertConfig(**SMALL))
    m = NativeHubert(model.config, 3)
    ns = list(range(400, 2000)) + list(range(2001, 200001, 997)) + [32000, 33333, 160000, 199999, 200000]
    want = model._get_feat_extract_output_lengths(torch.tensor(ns)).tolist()
    assert [m.frames(n) for n in ns] == want
    assert [native.hubert_frames(m.dims, n) for n in ns[::37]] == want[::37]
    assert m.frames(32000) == 99 and m.min_samples() == 400 and m.frames(399) == 0 and m.frames(400) == 1
    n = torch.tensor([10, 400, 5000, 40000])
    assert m.frames_of(n, 5000).tolist() == [1, 1, m.frames(5000), m.frames(5000)]


@pytest.mark.parametrize("field, value", [("do_stable_layer_norm", True), ("feat_extract_norm", "layer"), ("conv_bias", True),
                                          ("hidden_act", "relu"), ("feat_extract_activation", "gelu_new"),
                                          ("feat_proj_layer_norm", False), ("conv_pos_batch_norm", True)])
def test_unsupported_layouts_name_the_field(field, value):
    with pytest.raises(native.EdttsError, match=field):
        NativeHubert({**SMALL, field: value}, 1)


def test_unsupported_shapes_name_the_field():
    with pytest.raises(native.EdttsError, match="head_dim"):
        NativeHubert({**SMALL, "hidden_size": 1024, "num_attention_heads": 4, "num_conv_pos_embedding_groups": 4}, 1)
    with pytest.raises(native.EdttsError, match="num_attention_heads"):
        NativeHubert({**SMALL, "num_attention_heads": 3}, 1)
    with pytest.raises(ValueError, match="num_layers"):
        NativeHubert(SMALL, 4)
    d = NativeHubert({**SMALL, "conv_dim": [30] * 7}, 1).dims  # the library's own limits (conv_dim % 4)
    with pytest.raises(native.EdttsError, match="conv_dim"):
        native.hubert_packed_bytes(d)


def test_size_queries_grow():
    m = NativeHubert(transformers.HubertConfig(), 9)
    p9 = native.hubert_packed_bytes(m.dims)
    assert p9 > 4 * 90e6 / 12 * 9 / 9 and p9 > native.hubert_packed_bytes(NativeHubert(transformers.HubertConfig(), 3).dims)
    assert p9 >= 4 * sum(t.numel() for t in m.parameters()) - 4 * 128  # (weight-norm g and v fold into one tensor)
    a = native.hubert_workspace_bytes(m.dims, 1, 32000)
    assert 0 < a < native.hubert_workspace_bytes(m.dims, 2, 32000) < native.hubert_workspace_bytes(m.dims, 2, 64000)
    with pytest.raises(native.EdttsError):
        native.hubert_workspace_bytes(m.dims, 1, 399)


def _small_model():
    torch.manual_seed(0)
    return transformers.HubertModel(transformers.HubertConfig(**SMALL)).eval()


def test_state_dict_keys_and_both_weight_norm_forms():
    model = _small_model()
    with torch.no_grad():
        model.encoder.pos_conv_embed.conv.parametrizations.weight.original0.mul_(1.7)
    sd = model.state_dict()
    m = NativeHubert(model.config, 2)
    res = m.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    keys = set(m.state_dict())
    assert keys <= set(sd) and not any(k.startswith("encoder.layers.2.") for k in keys) and "masked_spec_embed" not in keys
    ref = model.encoder.pos_conv_embed.conv.weight.detach()
    assert torch.equal(m.folded_pos_conv_weight(), ref)
    # the older checkpoint form: weight_g / weight_v
    old = {}
    for k, v in sd.items():
        k = k.replace("conv.parametrizations.weight.original0", "conv.weight_g").replace("conv.parametrizations.weight.original1",
                                                                                         "conv.weight_v")
        old[k] = v
    m2 = NativeHubert(model.config.to_dict(), 2)
    res = m2.load_state_dict(old)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m2.folded_pos_conv_weight(), ref)
    # and the same fold as torch.nn.utils.weight_norm on the CPU, from the old keys
    conv = torch.nn.Conv1d(64, 64, 16, padding=8, groups=4)
    conv = torch.nn.utils.parametrizations.weight_norm(conv, name="weight", dim=2)
    with torch.no_grad():
        conv.parametrizations.weight.original0.copy_(old["encoder.pos_conv_embed.conv.weight_g"])
        conv.parametrizations.weight.original1.copy_(old["encoder.pos_conv_embed.conv.weight_v"])
    assert torch.equal(m2.folded_pos_conv_weight(), conv.weight.detach())
    for k in keys:
        assert torch.equal(m2.state_dict()[k], sd[k])


def test_from_hubert_and_semantic_encoder_wiring():
    model = _small_model()
    m = NativeHubert.from_hubert(model, 3)
    assert m.num_layers == 3 and torch.equal(m.state_dict()["encoder.layers.2.final_layer_norm.bias"],
                                             model.state_dict()["encoder.layers.2.final_layer_norm.bias"])
    with pytest.raises(ValueError, match="hubert_layer"):
        SemanticEncoder(CFG(device="cpu"), hubert=m, in_dim=64)  # default hubert_layer 9
    enc = SemanticEncoder(CFG(device="cpu", hubert_layer=3), hubert=m, in_dim=64)
    # a full encoder dict loads its hubert.* keys into the native backbone (layers past num_layers are ignored)
    full = {"hubert." + k: v for k, v in model.state_dict().items()}
    full.update({"proj." + k: v for k, v in enc.proj.state_dict().items()})
    full.update({"vq." + k: v for k, v in enc.vq.state_dict().items()})
    m3 = NativeHubert(model.config, 3)
    enc2 = SemanticEncoder.from_checkpoint({"encoder": full}, cfg=CFG(device="cpu", hubert_layer=3), hubert=m3)
    assert enc2.hubert is m3 and torch.equal(m3.folded_pos_conv_weight(), model.encoder.pos_conv_embed.conv.weight.detach())
    # lengths with a torch backbone: ValueError
    enc_t = SemanticEncoder(CFG(device="cpu", hubert_layer=3), hubert=model, in_dim=64)
    with pytest.raises(ValueError, match="NativeHubert"):
        enc_t.extract_hubert(torch.zeros(1, 4000), torch.tensor([4000]))


def test_cpu_tensors_raise():
    m = NativeHubert(SMALL, 1)
    with pytest.raises(native.EdttsError):
        m(torch.zeros(2, 4000))


def test_from_pretrained_stays_local():
    with pytest.raises(RuntimeError, match="local Hugging Face cache"):
        NativeHubert.from_pretrained("facebook/hubert-base-ls960", 9, local_files_only=True)
