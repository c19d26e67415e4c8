"""Host tests of the semantic encoder (no GPU): state-dict layouts, checkpoint loading, HuBERT handling, limits, size queries."""
import ctypes
import os
import re
import sys
import types

import pytest
import torch

from edge_diffusion_tts_amd import CFG, FSQ, FSQEncoder, SemanticEncoder, VectorQuantizer, native
from edge_diffusion_tts_amd.synth import HubertStandIn, synth_semantic_head

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the reference's state-dict keys and shapes (models/encoder.py:40-57, models/fsq.py, models/vq.py; train_v2.py:54-60)
PROJ_KEYS = {"0.weight": (128, 768), "0.bias": (128,), "2.weight": (128,), "2.bias": (128,), "3.weight": (128, 128), "3.bias": (128,)}
PROJ_KEYS_DROPOUT = {k.replace("3.", "4."): v for k, v in PROJ_KEYS.items()}
FSQ_KEYS = {"fsq._levels": (8,), "fsq._basis": (8,), "proj_down.weight": (8, 128), "proj_down.bias": (8,),
            "proj_up.weight": (128, 8), "proj_up.bias": (128,)}
VQ_KEYS = {"codebook.weight": (512, 128), "ema_cluster_size": (512,), "ema_w": (512, 128), "update_count": ()}


def shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


def test_state_dict_keys_match_the_reference():
    cfg = CFG(device="cpu")
    enc = SemanticEncoder(cfg)
    assert shapes(enc.proj.state_dict()) == PROJ_KEYS
    assert shapes(enc.vq.state_dict()) == FSQ_KEYS
    assert enc.vq.fsq._levels.dtype == torch.int32 and enc.vq.fsq._basis.tolist() == [1, 4, 16, 48, 144, 288, 576, 1152]
    assert enc.codebook_size == 2304 and enc.vq.codebook_size == 2304 and enc.vq.fsq.num_codes == 2304
    full = shapes(enc.state_dict())
    assert full == {**{"proj." + k: v for k, v in PROJ_KEYS.items()}, **{"vq." + k: v for k, v in FSQ_KEYS.items()}}
    vq = SemanticEncoder(CFG(device="cpu", use_fsq=False))
    assert shapes(vq.vq.state_dict()) == VQ_KEYS and vq.codebook_size == 512 and vq.vq.num_codes == 512
    assert shapes(SemanticEncoder(cfg, proj_dropout=True).proj.state_dict()) == PROJ_KEYS_DROPOUT
    assert shapes(FSQEncoder(64).state_dict())["proj_down.weight"] == (5, 64) and FSQEncoder(64).codebook_size == 6000
    assert shapes(FSQ([7, 5, 3]).state_dict()) == {"_levels": (3,), "_basis": (3,)} and FSQ([7, 5, 3]).num_codes == 105


@pytest.mark.parametrize("dropout", [False, True])
def test_proj_loads_either_layout(dropout):
    """The reference's own loading line, encoder.proj.load_state_dict(ckpt["encoder_proj"]), with the Linear at index 3 or 4."""
    proj_sd, q_sd = synth_semantic_head(768, 128, [4, 4, 3, 3, 2, 2, 2, 2], seed=3, dropout_layout=dropout)
    enc = SemanticEncoder(CFG(device="cpu"))
    enc.proj.load_state_dict(proj_sd)
    enc.vq.load_state_dict(q_sd)
    assert len(enc.proj) == (5 if dropout else 4)
    assert isinstance(enc.proj[3], torch.nn.Dropout) == dropout
    assert torch.equal(enc.proj.final.weight, proj_sd[("4" if dropout else "3") + ".weight"])
    assert shapes(enc.proj.state_dict()) == (PROJ_KEYS_DROPOUT if dropout else PROJ_KEYS)
    enc.proj.load_state_dict(synth_semantic_head(768, 128, [4, 4, 3, 3, 2, 2, 2, 2], seed=3, dropout_layout=not dropout)[0])
    assert len(enc.proj) == (4 if dropout else 5)


def _layouts():
    fsq_p, fsq_q = synth_semantic_head(768, 128, [8, 6, 5, 5, 5], seed=1, dropout_layout=True)
    vq_p, vq_q = synth_semantic_head(256, 64, None, 1000, seed=2)
    full_p, full_q = synth_semantic_head(768, 128, [4, 4, 3, 3, 2, 2, 2, 2], seed=3)
    full = {**{"proj." + k: v for k, v in full_p.items()}, **{"vq." + k: v for k, v in full_q.items()},
            "hubert.feature_projection.weight": torch.zeros(3)}
    return {
        "train_v2": ({"encoder_proj": fsq_p, "encoder_fsq": fsq_q, "decoder": {}}, "fsq", [8, 6, 5, 5, 5], 128, 768, 5),
        "train": ({"encoder_proj": vq_p, "encoder_vq": vq_q, "decoder": {}}, "vq", 1000, 64, 256, 4),
        "periodic": ({"encoder": full, "decoder": {}}, "fsq", [4, 4, 3, 3, 2, 2, 2, 2], 128, 768, 4),
    }


@pytest.mark.parametrize("layout", ["train_v2", "train", "periodic"])
def test_from_checkpoint_reads_every_layout(layout, tmp_path):
    ck, kind, q, S, in_dim, n_proj = _layouts()[layout]
    path = tmp_path / "ck.pt"
    torch.save(ck, path)
    for src in (ck, str(path)):
        enc = SemanticEncoder.from_checkpoint(src)
        assert enc.cfg.semantic_dim == S and enc.proj[0].in_features == in_dim and len(enc.proj) == n_proj
        assert enc.cfg.use_fsq == (kind == "fsq") and not enc.training
        if kind == "fsq":
            assert enc.cfg.fsq_levels == q and enc.vq.fsq.levels == q and isinstance(enc.vq, FSQEncoder)
            assert enc.codebook_size == int(torch.tensor(q).prod())
        else:
            assert isinstance(enc.vq, VectorQuantizer) and enc.codebook_size == q and enc.cfg.codebook_size == q
        assert enc.hubert is None  # "hubert.*" of the periodic layout is ignored without a module
        sd = ck.get("encoder_proj") or {k[5:]: v for k, v in ck["encoder"].items() if k.startswith("proj.")}
        assert all(torch.equal(enc.proj.state_dict()[k], v) for k, v in sd.items())


def test_full_encoder_dict_feeds_a_given_hubert():
    ck = _layouts()["periodic"][0]

    class Hub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.feature_projection = torch.nn.Module()
            self.feature_projection.weight = torch.nn.Parameter(torch.ones(3))

    hub = Hub()
    enc = SemanticEncoder.from_checkpoint(ck, hubert=hub)
    assert enc.hubert is hub and torch.equal(hub.feature_projection.weight, torch.zeros(3))


def _fake_transformers(monkeypatch, behaviour):
    calls = []

    class HubertModel:
        @staticmethod
        def from_pretrained(name, **kw):
            calls.append((name, kw))
            return behaviour(name, **kw)

    monkeypatch.setitem(sys.modules, "transformers", types.SimpleNamespace(HubertModel=HubertModel))
    return calls


def test_no_hubert_load_at_construction(monkeypatch):
    calls = _fake_transformers(monkeypatch, lambda *a, **k: pytest.fail("HuBERT loaded at construction"))
    SemanticEncoder(CFG(device="cpu"))
    SemanticEncoder.from_checkpoint(_layouts()["train_v2"][0])
    assert calls == []


def test_lazy_hubert_load_is_local_only(monkeypatch):
    calls = _fake_transformers(monkeypatch, lambda *a, **k: HubertStandIn(768, 0))
    enc = SemanticEncoder(CFG(device="cpu"))
    h = enc.extract_hubert(torch.zeros(2, 320 * 7))
    assert calls == [("facebook/hubert-base-ls960", {"local_files_only": True})]
    assert h.shape == (2, 7, 768) and isinstance(enc.hubert, HubertStandIn)
    enc.extract_hubert(torch.zeros(1, 320))
    assert len(calls) == 1  # loaded once


def test_missing_hubert_cache_is_a_clear_error(monkeypatch):
    def missing(*a, **k):
        raise OSError("not in the cache")

    _fake_transformers(monkeypatch, missing)
    enc = SemanticEncoder(CFG(device="cpu"))
    with pytest.raises(RuntimeError, match="never downloads"):
        enc.encode(torch.zeros(1, 3200))


def test_no_source_file_calls_from_pretrained_without_local_files_only():
    pkg = os.path.join(REPO, "edge-diffusion-tts_amd", "edge_diffusion_tts_amd")
    for root in (pkg, os.path.join(REPO, "tests"), os.path.join(REPO, "scratch")):
        for f in os.listdir(root):
            if not f.endswith(".py"):
                continue
            src = open(os.path.join(root, f)).read()
            for m in re.finditer(r"\.from_pretrained\(([^)]*)\)", src):
                assert "local_files_only=True" in m.group(1), f"{f}: {m.group(0)}"


def test_limits_are_unsupported():
    bad = [native.sem_dims(768, 100, [4, 4]), native.sem_dims(768, 144, [4, 4]), native.sem_dims(770, 128, [4, 4]),
           native.sem_dims(768, 128, [4] * 17), native.sem_dims(768, 128, [1, 4]), native.sem_dims(768, 128, codebook_size=0),
           native.sem_dims(768, 128, codebook_size=70000), native.sem_dims(768, 128, [256, 256, 256, 2])]
    for d in bad:
        with pytest.raises(native.EdttsError, match=r"code -1"):
            native.sem_packed_bytes(d)
    d = native.sem_dims(768, 128, [4, 4])
    d.quantizer = 7
    with pytest.raises(native.EdttsError, match=r"code -1"):
        native.sem_num_codes(d)


def test_size_queries():
    fsq = native.sem_dims(768, 128, [4, 4, 3, 3, 2, 2, 2, 2])
    assert native.sem_num_codes(fsq) == 2304
    assert native.sem_packed_bytes(fsq) >= 4 * (768 * 128 + 128 * 128 + 2 * 16 * 128 + 4 * 128)
    assert native.sem_num_codes(native.sem_dims(768, 128, [8, 6, 5, 5, 5])) == 6000
    vq = native.sem_dims(768, 128, codebook_size=512)
    assert native.sem_num_codes(vq) == 512
    assert native.sem_packed_bytes(vq) >= 4 * (768 * 128 + 128 * 128 + 2 * 512 * 128)
    small = native.sem_dims(256, 64, codebook_size=1000)
    assert native.sem_packed_bytes(small) < native.sem_packed_bytes(vq)
    assert native.sem_packed_bytes(native.sem_dims(0, 64, [7, 5, 3])) < native.sem_packed_bytes(native.sem_dims(256, 64, [7, 5, 3]))


def test_semantic_symbols_are_declared_and_exported():
    new = {"edtts_sem_packed_bytes", "edtts_sem_num_codes", "edtts_sem_pack", "edtts_sem_encode", "edtts_sem_decode", "edtts_sem_stats"}
    L = ctypes.CDLL(native.LIB_PATH)
    for sym in new:
        assert hasattr(L, sym), sym
    assert native.lib().edtts_version() == 400


def test_package_exports():
    import edge_diffusion_tts_amd as pkg
    for n in ("SemanticEncoder", "VectorQuantizer", "FSQ", "FSQEncoder"):
        assert n in pkg.__all__ and getattr(pkg, n) is not None
