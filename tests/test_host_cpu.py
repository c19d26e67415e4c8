"""CPU-only tests of the host layer: config surface, schedule tables, weight recipe, C-ABI library loading and
symbol export, error behaviour without a GPU.  No kernel is launched here."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, EdgeInference, TrainPhase, native, synth_state_dict
from edge_diffusion_tts_amd.synth import decoder_shapes, hash_uniform


def test_cfg_defaults_and_roundtrip():
    cfg = CFG(device="cpu")
    # the fields the sampler path reads and their reference defaults
    assert (cfg.n_mels, cfg.diff_steps, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn_mult) == (80, 1000, 160, 4, 4, 2)
    assert (cfg.attn_window_size, cfg.codebook_size, cfg.semantic_dim, cfg.use_adaln, cfg.dropout) == (64, 512, 128, True, 0.2)
    assert cfg.segment_len == 32000 and cfg.inference_steps == 4 and cfg.phase is TrainPhase.DIFFUSION
    assert cfg.ckpt_path.endswith("checkpoint_latest.pt") and os.path.isdir(cfg.out_dir) and os.path.isdir(cfg.data_root)
    d = cfg.to_dict()
    assert d["phase"] == "diffusion" and set(d) == {f.name for f in dataclasses.fields(CFG)}
    d["unknown_key"] = 1
    cfg2 = CFG.from_dict(d)
    assert cfg2.phase is TrainPhase.DIFFUSION and cfg2.to_dict() == cfg.to_dict()
    assert len(dataclasses.fields(CFG)) == 57


def test_schedule_tables_match_reference(golden):
    g = golden("schedule_tables")
    sch = DiffusionSchedule(1000)
    for name in DiffusionSchedule.TABLE_NAMES:
        assert torch.equal(getattr(sch, name), g[name]), name
    assert sch.get_schedule_for_steps(4) == [999, 749, 499, 249]
    tl = golden("timesteps")
    for n in (1, 2, 3, 4, 8, 16):
        assert sch.get_schedule_for_steps(n) == tl[f"n{n}"].tolist()


def test_schedule_light_algebra_roundtrip():
    sch = DiffusionSchedule(1000)
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn(3, 5, 80, generator=g)
    t = torch.tensor([10, 500, 900])
    xt, noise = sch.q_sample(x0, t, torch.randn(3, 5, 80, generator=g))
    assert torch.allclose(sch.predict_x0_from_eps(xt, t, noise), x0, atol=2e-3)
    v = sch.get_v_target(x0, noise, t)
    assert torch.allclose(sch.predict_x0_from_v(xt, t, v), x0, atol=1e-4)
    assert torch.allclose(sch.predict_eps_from_v(xt, t, v), noise, atol=1e-4)


def test_ddim_coefficients_are_exactly_rounded():
    sch = DiffusionSchedule(1000)
    for t, tp in ((999, 749), (749, 499), (249, 0), (315, 65), (5, -1)):
        c = sch.ddim_coefficients(t, tp)
        ab = np.float64(sch.alpha_bar[t].item())
        abp = np.float64(sch.alpha_bar[tp].item()) if tp >= 0 else np.float64(1.0)
        assert c[0] == float(np.float32(np.sqrt(np.float64(np.float32(1.0 - ab)))))
        assert c[1] == float(np.float32(np.sqrt(ab))) and c[2] == float(np.float32(np.sqrt(abp)))
        assert c[3] == float(np.float32(np.sqrt(np.float64(np.float32(1.0 - abp)))))


def test_synth_weights_are_portable_and_complete():
    cfg = CFG(device="cpu")
    a, b = synth_state_dict(cfg, 0), synth_state_dict(cfg, 0)
    assert list(a) == list(decoder_shapes(cfg)) and all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["in_proj.weight"], synth_state_dict(cfg, 1)["in_proj.weight"])
    # known answer of the counter hash (guards against platform-dependent integer behaviour)
    assert abs(float(hash_uniform((3,), 0, 0)[1]) - (-0.6672071210646784)) < 1e-15
    # tensors the reference zero-initialises are non-zero here
    for k in ("out_proj.weight", "out_proj.bias", "layers.0.norm1.proj.weight", "layers.3.norm3.proj.bias"):
        assert float(a[k].abs().max()) > 0
    assert sum(v.numel() for k, v in a.items() if not k.endswith(".pe")) == 1983440


def test_decoder_state_dict_contract():
    cfg = CFG(device="cpu")
    dec = EdgeDiffusionDecoder(cfg)
    keys = list(dec.state_dict().keys())
    assert keys == list(decoder_shapes(cfg).keys())
    assert sum(p.numel() for p in dec.parameters()) == 1983440
    # reference default init: out_proj and the AdaLN projections are zero (decoder.py:63-64, transformer.py:61-62)
    sd = dec.state_dict()
    assert float(sd["out_proj.weight"].abs().max()) == 0 and float(sd["layers.2.norm1.proj.weight"].abs().max()) == 0
    assert float(sd["layers.1.norm2.weight"].min()) == 1.0 and sd["pos_emb.pe"].shape == (1000, 160)
    res = dec.load_state_dict(synth_state_dict(cfg, 0))
    assert not res.missing_keys and not res.unexpected_keys


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(REPO, "include", "edtts.h")).read()
    declared = set(re.findall(r"\b(edtts_[a-z_0-9]+)\s*\(", header))
    assert declared == set(native.EXPORTED_SYMBOLS)
    L = ctypes.CDLL(native.LIB_PATH)
    for sym in declared:
        assert hasattr(L, sym), sym
    lib = native.lib()
    assert lib.edtts_version() == 400


def test_slot_names_cover_the_state_dict():
    cfg = CFG(device="cpu")
    names = native.slot_names(cfg.layers)
    keys = set(decoder_shapes(cfg).keys()) | {"time_freqs"}
    assert set(names) == keys and len(names) == len(keys)


def test_size_queries_and_unsupported_dims():
    cfg = CFG(device="cpu")
    dec = EdgeDiffusionDecoder(cfg)
    assert native.packed_bytes(dec.dims()) > 4 * 1983440
    small = native.workspace_bytes(dec.dims(), 1, 256, 128, 4)
    big = native.workspace_bytes(dec.dims(), 256, 512, 256, 4)
    assert big > 100 * small > 0
    bad = EdgeDiffusionDecoder(CFG(hidden=96, heads=4, device="cpu"))   # 96/4 = 24: head_dim % 16 == 8 but no instance
    ws = native.workspace_bytes(bad.dims(), 1, 32, 16, 1)                # layout queries work for any hidden % 32 == 0
    assert ws > 0
    with pytest.raises(native.EdttsError, match="need hidden"):
        native.workspace_bytes(EdgeDiffusionDecoder(CFG(hidden=100, heads=4, device="cpu")).dims(), 1, 32, 16, 1)


def test_no_cpu_fallback():
    cfg = CFG(device="cpu")
    dec = EdgeDiffusionDecoder(cfg)
    with pytest.raises(ValueError):
        dec(torch.zeros(1, 32, 80), torch.zeros(1, dtype=torch.long))
    with pytest.raises(native.EdttsError, match="HIP device"):
        dec(torch.zeros(1, 32, 80), torch.zeros(1, dtype=torch.long), torch.zeros(1, 16, dtype=torch.long))
    sch = DiffusionSchedule(1000)
    with pytest.raises(native.EdttsError, match="HIP device"):
        sch.get_ddim_step(torch.zeros(1, 4, 80), torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long), torch.zeros(1, 4, 80))
    with pytest.raises(native.EdttsError, match="HIP device"):
        sch.ddpm_step(torch.zeros(1, 4, 80), torch.zeros(1, dtype=torch.long), torch.zeros(1, 4, 80))
    infer = EdgeInference(cfg, sch, None, dec)
    with pytest.raises(native.EdttsError):
        infer.generate_mel(torch.zeros(1, 16, dtype=torch.long), 4)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(REPO, "edge-diffusion-tts_amd", "edge_diffusion_tts_amd")
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            assert not re.search(r"^\s*(from|import)\s+\.*oracle", src, re.M), f
            assert "edtts_oracle" not in src, f


def test_checkpoint_interop(tmp_path):
    """Reference checkpoint layouts (train.py:291-297, train_v2.py:335-341), `_orig_mod.` prefixes left by torch.compile,
    FSQ-sized codebooks, fp16/fp64 tensors."""
    cfg = CFG(device="cpu")
    sd = synth_state_dict(cfg, 4)
    # compiled-module prefix + a non-persistent RoPE buffer that older snapshots carried
    ck = {"decoder": {"_orig_mod." + k: v.double() for k, v in sd.items()}, "cfg": cfg.to_dict(), "encoder_proj": {}, "encoder_vq": {}}
    ck["decoder"]["_orig_mod.layers.0.cross_attn.rope.cos_cached"] = torch.zeros(1, 1, 8, 40)
    path = tmp_path / "edge_model_final.pt"
    torch.save(ck, path)
    dec = EdgeDiffusionDecoder.from_checkpoint(str(path))
    for k, v in dec.state_dict().items():
        assert torch.equal(v, sd[k]) and v.dtype == torch.float32, k
    # FSQ runs: 2304 semantic codes, config still says 512 (config.py:97,100; train_v2.py:246)
    cfg2 = CFG(device="cpu", codebook_size=2304)
    sd2 = synth_state_dict(cfg2, 5)
    dec2 = EdgeDiffusionDecoder.from_checkpoint({"decoder": sd2, "cfg": CFG(device="cpu").to_dict()})
    assert dec2.cfg.codebook_size == 2304 and dec2.dims().codebook_size == 2304
    # bare state-dict, strict mismatch still raises
    with pytest.raises(RuntimeError):
        EdgeDiffusionDecoder(cfg).load_state_dict({k: v for k, v in sd.items() if "ffn" not in k})


def test_decoder_without_adaln_uses_plain_rmsnorm_keys():
    """CFG(use_adaln=False): the reference builds RMSNorm for norm1 / norm3 (layers/transformer.py:101-104,119-122); the state-dict
    keys follow, and the kernels' AdaLN slots are fed the gain plus an all-zero modulation projection."""
    cfg = CFG(use_adaln=False, device="cpu")
    dec = EdgeDiffusionDecoder(cfg)
    keys = set(dec.state_dict())
    assert "layers.0.norm1.weight" in keys and "layers.3.norm3.weight" in keys
    assert not any(".norm1.proj." in k or ".norm3.norm." in k for k in keys)
    res = dec.load_state_dict(synth_state_dict(cfg, 4))
    assert not res.missing_keys and not res.unexpected_keys
    slots = dec._state_tensors()
    assert set(native.slot_names(cfg.layers)) <= set(slots)
    assert float(slots["layers.1.norm3.proj.weight"].abs().max()) == 0.0 and slots["layers.1.norm3.proj.bias"].shape == (320,)
    assert torch.equal(slots["layers.2.norm1.norm.weight"], dec.state_dict()["layers.2.norm1.weight"])


def test_build_depends_on_every_kernel_source(tmp_path):
    """build() must rebuild when ANY file under csrc/ or include/ is newer than the library (round 2's list named three of five)."""
    import __graft_entry__ as G
    srcs = {os.path.basename(p) for p in G._sources()}
    assert {"edtts_kernels.hip", "edtts_device.h", "edtts_bf16.h", "edtts_melpost.h", "edtts.h"} <= srcs
    listed = {f for d in ("edge-diffusion-tts_amd/csrc", "include") for f in os.listdir(os.path.join(REPO, d)) if f.endswith((".hip", ".h"))}
    assert listed <= srcs
    # the check is by CONTENT (the snapshot to the GPU box does not keep mtime order): one changed byte in any header -> stale
    h0 = G._source_hash()
    real_open = open
    bf = os.path.join(REPO, "edge-diffusion-tts_amd", "csrc", "edtts_bf16.h")

    class _Patched:
        def __call__(self, path, mode="r", *a, **k):
            f = real_open(path, mode, *a, **k)
            if os.path.abspath(path) == bf and "b" in mode:
                data = f.read() + b"\n// edit"
                f.close()
                import io
                return io.BytesIO(data)
            return f

    import builtins
    builtins.open = _Patched()
    try:
        assert G._source_hash() != h0
    finally:
        builtins.open = real_open
    assert G._source_hash() == h0


def test_every_kernel_header_is_compiled_exactly_once():
    """The library is ONE translation unit: edtts_kernels.hip and the headers its #include "..." lines reach.  _sources() hashes every
    file under csrc/, so a header nothing includes would make the build stamp depend on text that is never compiled; and the units
    carry no include guard, their order being the file map.  A plain text scan -- which is why no #include "..." may stand behind an
    #if: the scan (and a reader) would count a header that only some builds compile."""
    csrc = os.path.join(REPO, "edge-diffusion-tts_amd", "csrc")
    seen, conditional = [], []

    def walk(path):
        depth = 0
        with open(path) as f:
            lines = f.read().split("\n")
        for line in lines:
            d = re.match(r'[ \t]*#[ \t]*(if|ifdef|ifndef|endif|include)\b[ \t]*(?:"([^"]+)")?', line)
            if not d:
                continue
            if d.group(1) == "endif":
                depth -= 1
            elif d.group(1) != "include":
                depth += 1
            elif d.group(2):
                target = os.path.normpath(os.path.join(os.path.dirname(path), d.group(2)))
                assert os.path.exists(target), (path, d.group(2))
                seen.append(target)
                if depth:
                    conditional.append((os.path.basename(path), d.group(2)))
                if os.path.dirname(target) == csrc and seen.count(target) == 1:
                    walk(target)
        assert depth == 0, path

    walk(os.path.join(csrc, "edtts_kernels.hip"))
    headers = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h"))
    assert os.path.join(csrc, "edtts_device.h") in headers
    assert conditional == [], "#include \"...\" lines behind a preprocessor condition"
    assert [h for h in headers if h not in seen] == [], "headers under csrc/ that edtts_kernels.hip never reaches"
    assert sorted({h for h in seen if seen.count(h) > 1}) == [], "headers included more than once"


def test_no_product_kernel_uses_scratch():
    """The compile's -Rpass-analysis=kernel-resource-usage report (kept next to the library by build()): every kernel of the shipped
    library lives in registers -- a spilling instance is a build error (round 2 shipped one with 76 B/lane)."""
    import __graft_entry__ as G
    sample = ("x.hip:1:1: remark: Function Name: _Z3foo [-Rpass-analysis=kernel-resource-usage]\n"
              "x.hip:1:1: remark:     VGPRs: 256 [-Rpass-analysis=kernel-resource-usage]\n"
              "x.hip:1:1: remark:     AGPRs: 256 [-Rpass-analysis=kernel-resource-usage]\n"
              "x.hip:1:1: remark:     ScratchSize [bytes/lane]: 76 [-Rpass-analysis=kernel-resource-usage]\n"
              "x.hip:1:1: remark:     VGPRs Spill: 18 [-Rpass-analysis=kernel-resource-usage]\n")
    assert G.kernel_resources(sample) == {"_Z3foo": {"vgpr": 256, "agpr": 256, "scratch": 76, "spill": 18}}
    with pytest.raises(RuntimeError, match="scratch"):
        G.check_no_scratch(sample)
    if not os.path.exists(G.RESOURCE_LOG):
        pytest.skip("library not built by build() in this checkout")
    res = G.kernel_resources(open(G.RESOURCE_LOG).read())
    layer = [k for k in res if "k_layer" in k]
    assert len(layer) >= 12 and all(v.get("scratch", 0) <= 64 for v in res.values())
    assert all(v.get("spill", 0) == 0 or v.get("scratch", 0) == 0 for v in res.values())  # "spills" only into free AGPRs, never to memory
    # a reserved-but-unused emergency slot (ScratchSize > 0, zero spills, no scratch_* instruction: build() checks the assembly) is
    # tolerated for at most a couple of cold instances -- never for the headline kernels
    reserved = [k for k, v in res.items() if v.get("scratch", 0) > 0]
    assert len(reserved) <= 2 and all(res[k]["scratch"] <= 64 for k in reserved), reserved
    assert not any("CfgILi160ELi4ELi80ELi2EEE" in k for k in reserved)
    # the rule itself: an assembly with a scratch instruction fails, one without passes
    asm_ok, asm_bad = "_Z3foo:\n\tv_mov_b32 v0, v1\n\ts_endpgm\n", "_Z3foo:\n\tscratch_store_dword off, v0, s0\n\ts_endpgm\n"
    nospill = sample.replace("VGPRs Spill: 18", "VGPRs Spill: 0")
    G.check_no_scratch(nospill.replace("]: 76", "]: 36"), asm_ok)  # an untouched emergency slot passes
    with pytest.raises(RuntimeError, match="scratch instructions"):
        G.check_no_scratch(nospill.replace("]: 76", "]: 16"), asm_bad)
    with pytest.raises(RuntimeError, match="76 B/lane"):
        G.check_no_scratch(nospill, asm_ok)  # more than an emergency slot
    # the product library carries no experiment instantiations (two-launch layer halves, stand-alone attention kernels)
    assert not any("k_attn16" in k for k in res)
    assert not any(re.search(r"k_layerIN5edtts3CfgI[^E]*EELi\dELi[12]E", k) for k in res), "PART_ATTN / PART_FFN instances in the product build"


def test_inline_mfma_hazard_rule():
    """build() walks the device assembly for instructions that touch the destination registers of an inline-assembly MFMA block
    (the 64-frame bf16 instance accumulates into AGPRs it names itself, so hipcc's hazard recogniser does not cover them) before
    the MFMA has left the pipe."""
    import __graft_entry__ as G
    block = ("_Z3foo:\n\t;;#ASMSTART\n\ts_nop 1\n\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]\n"
             "\tv_mfma_f32_16x16x32_bf16 a[4:7], v[0:3], v[8:11], a[4:7]\n\t;;#ASMEND\n")
    early = block + "\tv_add_f32 v1, v2, v3\n\tv_accvgpr_read_b32 v9, a5\n\ts_endpgm\n"
    assert G.inline_mfma_hazards(early) == [("_Z3foo", 8, "v_accvgpr_read_b32 v9, a5")]
    fenced = block + "\ts_nop 15\n\ts_nop 15\n\tv_accvgpr_read_b32 v9, a5\n\ts_endpgm\n"
    assert G.inline_mfma_hazards(fenced) == []
    chained = block + "\t;;#ASMSTART\n\tv_mfma_f32_16x16x32_bf16 a[8:11], v[0:3], v[4:7], a[8:11]\n\t;;#ASMEND\n\ts_endpgm\n"
    assert G.inline_mfma_hazards(chained) == []  # the next block accumulates into other registers
    clobber = block + "\tv_accvgpr_write_b32 a2, v0\n\ts_endpgm\n"
    assert len(G.inline_mfma_hazards(clobber)) == 1


def test_workspace_cache_evicts_least_recently_used():
    """decoder.workspace(): bounded cache, least-recently-USED entry dropped first (round 2 cleared the whole cache, which could free
    a workspace a captured graph still replays into; those are pinned -- GPU test test_samplers_are_graph_capturable)."""
    cfg = CFG(device="cpu")
    dec = EdgeDiffusionDecoder(cfg)
    dec.WORKSPACE_CACHE = 3
    a = dec.workspace(1, 32, 16, 1, "cpu")
    b = dec.workspace(2, 32, 16, 1, "cpu")
    c = dec.workspace(3, 32, 16, 1, "cpu")
    assert dec.workspace(1, 32, 16, 1, "cpu") is a  # a becomes the most recently used
    d = dec.workspace(4, 32, 16, 1, "cpu")          # evicts b, the least recently used
    assert dec.workspace(1, 32, 16, 1, "cpu") is a and dec.workspace(3, 32, 16, 1, "cpu") is c and dec.workspace(4, 32, 16, 1, "cpu") is d
    assert dec.workspace(2, 32, 16, 1, "cpu") is not b and len(dec._workspaces) == 3
    assert a.dtype == torch.uint8 and not bool(a.any())


def test_longform_chunk_count_follows_the_reference_sample_arithmetic():
    """inference_pipeline.py:221-236 fixes the SAMPLE counts (2.0 s / 0.5 s at 16 kHz = 32000 / 8000) and derives the frame counts
    through a centred mel transform (frames = samples // hop + 1 = 201 / 51 at hop 160).  Rebuilding samples from those frame
    counts over-states them (51 * 160 = 8160) and loses a chunk whenever (N - 8000) lies less than 160 samples above a multiple of
    24000; with the sample counts handed over, the chunk count is the reference's for every length."""
    import math
    from edge_diffusion_tts_amd.longform import InpaintSampler
    sr, hop = 16000, 160
    cs, ov = int(2.0 * sr), int(0.5 * sr)
    cf, of = cs // hop + 1, ov // hop + 1
    assert (cf, of) == (201, 51)
    lost = 0
    for N in list(range(40000, 40000 + 24000, 37)) + [8000 + 24000 * k + d for k in (1, 2, 5) for d in (-1, 0, 1, 100, 159, 160, 161)]:
        total_frames = N // hop + 1
        ref = int(math.ceil((N - ov) / (cs - ov)))
        n, c, h = InpaintSampler.chunk_plan(total_frames, cf, of, hop, chunk_samples=cs, overlap_samples=ov, total_samples=N)
        assert (n, c, h) == (max(1, ref), cs, cs - ov), N
        lost += InpaintSampler.chunk_plan(total_frames, cf, of, hop)[0] != max(1, ref)
    assert lost > 0  # (the frame-derived default does differ on this geometry: that is what the arguments are for)
    with pytest.raises(ValueError):
        InpaintSampler.chunk_plan(100, 50, 10, hop, chunk_samples=8000, overlap_samples=8000)


def test_build_time_instance_list():
    """Further fp32 decoder shapes are a build option (EDTTS_INSTANCES -> -D flags for the dispatch), not a source edit."""
    import __graft_entry__ as G
    assert G.instance_flags("") == [] and G.instance_flags("160x4x80") == []  # built-in shapes are not repeated
    f = G.instance_flags("192x6x80, 128x4x80,192x6x80")
    assert f[0] == "-DEDTTS_EXTRA_INSTANCES(lo,...)=EDTTS_X(lo,192,6,80,__VA_ARGS__) EDTTS_X(lo,128,4,80,__VA_ARGS__)"
    assert f[1] == '-DEDTTS_EXTRA_NAMES=", 192/6/80, 128/4/80"'
    for bad in ("100x4x80", "192x5x80", "192x6x81", "96x4x80x1", "abc"):
        with pytest.raises(ValueError):
            G.instance_flags(bad)
    # the product build carries the default list, and the flags are part of the stale check
    assert all(x in G.FLAGS for x in G.instance_flags(os.environ.get("EDTTS_INSTANCES", G.DEFAULT_INSTANCES)))
    # bf16 shapes: head_dim 32 and hidden % 64 == 0 only
    f16 = G.instance_flags("128x4x80,256x8x80", bf16=True)
    assert f16 == ["-DEDTTS_EXTRA_INSTANCES16(lo,...)=EDTTS_X16(lo,128,4,80,__VA_ARGS__)", '-DEDTTS_EXTRA_NAMES16=", 128/4/80"']
    for bad in ("160x4x80", "96x3x80", "128x4x81", "128x8x80"):
        with pytest.raises(ValueError):
            G.instance_flags(bad, bf16=True)
    assert all(x in G.FLAGS for x in G.instance_flags(os.environ.get("EDTTS_INSTANCES_BF16", G.DEFAULT_INSTANCES_BF16), bf16=True))


def test_pinned_workspaces_can_be_released(monkeypatch):
    """Workspaces handed out during graph capture are pinned (a replay writes into them); release_pinned() drops them once the
    graphs are gone, and a decoder that accumulates more pins than its cache warns."""
    import warnings
    dec = EdgeDiffusionDecoder(CFG(device="cpu"))
    monkeypatch.setattr(native, "workspace_bytes", lambda *a: 64)
    fake = {"on": False}
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: fake["on"])

    class Fake(torch.Tensor):
        is_cuda = True
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: torch.Tensor._make_subclass(Fake, torch.empty(4)))
    fake["on"] = True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for i in range(dec.WORKSPACE_CACHE + 1):
            dec.workspace(1 + i, 32, 16, 4, "cpu")
    assert len(dec._pinned_workspaces) == dec.WORKSPACE_CACHE + 1 and any("pinned" in str(x.message) for x in w)
    assert dec.release_pinned(B=1) == 1 and dec.release_pinned() == dec.WORKSPACE_CACHE
    assert not dec._pinned_workspaces and not dec._workspaces


def test_run_time_switches_and_scratch_query_need_no_gpu():
    """The library's host-only entry points: the two run-time switches return the previous value and ignore values outside their
    domain; edtts_dsconv_scratch_floats says which shapes run as one kernel (no scratch) -- the stride / kernel-size condition of
    include/edtts.h; the workspace query covers the sub-batch form of a sampler call (never smaller than the one-piece form)."""
    L = native.lib()
    prev = L.edtts_set_substreams(1)
    assert L.edtts_set_substreams(0) == 1 and L.edtts_set_substreams(99) == 1  # queries: unchanged
    assert L.edtts_set_substreams(2) == 1 and L.edtts_set_substreams(prev) == 2
    prevc = L.edtts_set_coop(0)
    assert L.edtts_set_coop(7) == 0 and L.edtts_set_coop(22) == 0 and L.edtts_set_coop(-1) == 22
    L.edtts_set_coop(prevc)
    # how many sub-batches a call shape is cut into (1024 SIMDs assumed without a device): two rounds of waves each, at least two, at most the setting
    d160, d256 = EdgeDiffusionDecoder(CFG(device="cpu")).dims(), EdgeDiffusionDecoder(CFG(hidden=256, heads=8, layers=8, device="cpu"), max_len=1024).dims()
    old = L.edtts_set_substreams(4)
    assert [native.substreams_for(d160, b, 512) for b in (1, 64, 127, 128, 256, 384, 512, 2048)] == [1, 1, 1, 2, 2, 3, 4, 4]
    assert native.substreams_for(d256, 256, 1024) == 4 and native.substreams_for(d160, 256, 1000) == 4 and native.substreams_for(d160, 3, 99999) == 3
    L.edtts_set_substreams(2)
    assert native.substreams_for(d160, 512, 512) == 2
    L.edtts_set_substreams(1)
    assert native.substreams_for(d160, 512, 512) == 1
    L.edtts_set_substreams(old)
    need = ctypes.c_size_t(123)
    L.edtts_dsconv_scratch_floats(4, 80, 160, 512, 3, 1, 8, ctypes.byref(need))
    assert need.value == 0                                    # the reference's shape class: one kernel
    L.edtts_dsconv_scratch_floats(4, 80, 160, 512, 3, 2, 8, ctypes.byref(need))
    assert need.value == 0                                    # 127 * 2 + 3 <= 260
    L.edtts_dsconv_scratch_floats(4, 80, 160, 512, 3, 3, 8, ctypes.byref(need))
    assert need.value == 4 * 160 * 171 + 2 * 4 * 8            # stride 3: the three-kernel path, T_out = (512 + 2 - 3) // 3 + 1
    L.edtts_dsconv_scratch_floats(4, 96, 160, 512, 3, 1, 8, ctypes.byref(need))
    assert need.value == 4 * 160 * 512 + 2 * 4 * 8            # more input channels than the fused kernel holds
    dec = EdgeDiffusionDecoder(CFG(device="cpu"))
    a, b = native.workspace_bytes(dec.dims(), 255, 512, 256, 4), native.workspace_bytes(dec.dims(), 256, 512, 256, 4)
    assert b > a > 255 * 512 * 160 * 4 * 7                    # h + two sets of q, k, v^T at least
