"""Host tests (no GPU) of _cache.PackedBlob and _cache.WorkspaceCache, the two pieces of host state every module keeps in front of
the kernels, and of copying the modules that are built on them.  The pack calls are counting stand-ins, the
tensors are CPU tensors and the streams are stand-ins that carry a handle, as in test_concurrency_host.py."""
import copy
import pickle
import warnings
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

from edge_diffusion_tts_amd import CFG, FSQ, EdgeDiffusionDecoder, NativeHubert, SemanticEncoder, native
from edge_diffusion_tts_amd._cache import PackedBlob, WorkspaceCache
from edge_diffusion_tts_amd.encoder import FSQEncoder, VectorQuantizer

SMALL = dict(conv_dim=[32] * 7, hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=3,
             num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)  # (tests/test_hubert_host.py)


class Counting:
    """Stand-ins for a byte-count query and a pack call: they count, and the pack writes the call's number into the blob."""
    def __init__(self, nbytes=8):
        self.nbytes, self.queries, self.packs, self.key = nbytes, 0, 0, None

    def nbytes_of(self, key):
        self.queries += 1
        return self.nbytes

    def pack(self, key, tensors, blob):
        self.key = key
        self.packs += 1
        self.packed = tensors
        blob.fill_(self.packs)


def make_blob(**kw):
    c = Counting(**kw)
    return c, PackedBlob(c.nbytes_of, c.pack)


# ------------------------------------------------------------------------------------------------------------------ PackedBlob
def test_one_pack_per_change_of_version_storage_device_or_key():
    c, pb = make_blob()
    w = [torch.zeros(3), torch.ones(2, 2)]
    blob = pb.get("k", w)
    assert c.packs == 1 and c.key == "k" and blob.dtype == torch.uint8 and blob.numel() == 8 and int(blob[0]) == 1
    assert [t.data_ptr() for t in c.packed] == [t.data_ptr() for t in w]
    assert pb.get("k", w) is blob and pb.get("k", list(w)) is blob and c.packs == 1  # hits hand out the same object
    with torch.no_grad():
        w[1].add_(1.0)                      # version
    assert pb.get("k", w) is blob and c.packs == 2 and int(blob[0]) == 2
    w[0] = w[0].clone()                     # storage
    assert pb.get("k", w) is blob and c.packs == 3
    assert pb.get("k2", w) is blob and c.packs == 4    # key
    assert pb.get("k2", w) is blob and c.packs == 4
    meta = [t.to("meta") for t in w]        # device (the only other one a host has: its tensors have no storage)
    on_meta = pb.get("k2", meta)
    assert c.packs == 5 and on_meta is not blob and on_meta.device.type == "meta"
    assert pb.get("k2", meta) is on_meta and c.packs == 5
    c.nbytes = 24                           # a size change re-allocates on the next pack, and only then
    assert pb.get("k2", meta) is on_meta
    assert pb.get("k3", w).numel() == 24 and c.packs == 6


def test_signature_invalidate_current_and_commit():
    c, pb = make_blob()
    w = [torch.zeros(3), torch.ones(2)]
    assert pb.sig is None and pb.current("k", w) is None
    blob = pb.get("k", w)
    assert pb.sig == PackedBlob.signature("k", w) and pb.sig != PackedBlob.signature("other", w)
    assert pb.current("k", w) is blob and pb.current("other", w) is None and c.packs == 1
    pb.invalidate()
    assert pb.current("k", w) is None
    assert pb.get("k", w) is blob and pb.get("k", w) is blob and c.packs == 2   # exactly one re-pack
    assert pb.sig == PackedBlob.signature("k", w)
    with torch.no_grad():
        w[0].mul_(2.0)
    assert pb.current("k", w) is None and pb.sig != PackedBlob.signature("k", w)
    pb.commit("k", w)                       # (what FusedAdamW does after writing the new values into the blob itself)
    assert pb.current("k", w) is blob and pb.sig == PackedBlob.signature("k", w)
    assert pb.get("k", w) is blob and c.packs == 2
    assert pb._event is None and not pb._waited   # CPU tensors record no event


def test_tensors_to_pack_are_built_on_a_miss_only():
    c, pb = make_blob()
    w, built = [torch.zeros(3)], []

    def packs():
        built.append(1)
        return [w[0] * 2.0, torch.ones(1)]
    pb.get("k", w, packs=packs)
    pb.get("k", w, packs=packs)
    assert len(built) == 1 and c.packs == 1 and len(c.packed) == 2
    with torch.no_grad():
        w[0].add_(1.0)
    pb.get("k", w, packs=packs)
    assert len(built) == 2 and c.packs == 2


def test_dtype_and_device_mismatches_keep_their_texts():
    c, pb = make_blob()
    with pytest.raises(native.EdttsError, match=r"^weight 1: expected fp32 on cpu, got torch.float64 on cpu$"):
        pb.get("k", [torch.zeros(3), torch.zeros(3, dtype=torch.float64)])
    with pytest.raises(native.EdttsError, match=r"^weight 1: expected fp32 on cpu, got torch.float32 on meta$"):
        pb.get("k", [torch.zeros(3), torch.zeros(3, device="meta")])
    with pytest.raises(native.EdttsError, match=r"^weight out_proj.bias: expected fp32 on cpu, got torch.float16 on cpu$"):
        pb.get("k", [torch.zeros(3), torch.zeros(3).half()], names=["in_proj.weight", "out_proj.bias"])
    h = PackedBlob(c.nbytes_of, c.pack, "NativeHubert weight")
    with pytest.raises(native.EdttsError, match=r"^NativeHubert weight 0: expected fp32 on cpu, got torch.int32 on cpu$"):
        h.get("k", [torch.zeros(3)], packs=lambda: [torch.zeros(3, dtype=torch.int32)])
    assert c.packs == 0 and pb.blob is None and pb.sig is None
    # ... and through the modules: the decoder names the slot, the heads and HuBERT give the index
    dec = EdgeDiffusionDecoder(CFG(device="cpu"))
    dec.out_proj.bias.data = dec.out_proj.bias.data.double()
    with pytest.raises(native.EdttsError, match=r"^weight out_proj.bias: expected fp32 on cpu, got torch.float64 on cpu$"):
        dec._ensure_packed()
    enc = SemanticEncoder(CFG(device="cpu"))
    enc.proj[0].bias.data = enc.proj[0].bias.data.half()
    with pytest.raises(native.EdttsError, match=r"^weight 1: expected fp32 on cpu, got torch.float16 on cpu$"):
        enc.encode_features(torch.zeros(1, 4, 768))
    hub = NativeHubert(SMALL, 2)
    hub._get("feature_extractor.conv_layers.0.layer_norm.weight").data = torch.ones(32, dtype=torch.float64)
    with pytest.raises(native.EdttsError, match=r"^NativeHubert weight 1: expected fp32 on cpu, got torch.float64 on cpu$"):
        hub._packed()


# -------------------------------------------------------------------------------------------------------------- WorkspaceCache
class FakeStream:
    def __init__(self, handle):
        self.cuda_stream = handle


class Owner:
    WORKSPACE_CACHE = 8


def made(log):
    def alloc():
        log.append(1)
        return torch.zeros(4)
    return alloc


def test_one_workspace_per_head_and_stream():
    cache, owner, log = WorkspaceCache(), Owner(), []
    s1, s2 = FakeStream(0x1000), FakeStream(0x2000)
    default = cache.get(owner, (1, 32), "cpu", None, made(log))
    a = cache.get(owner, (1, 32), "cpu", s1, made(log))
    b = cache.get(owner, (1, 32), "cpu", s2, made(log))
    other = cache.get(owner, (2, 32), "cpu", s1, made(log))
    assert len({id(t) for t in (default, a, b, other)}) == 4 and len(log) == 4
    assert cache.get(owner, (1, 32), "cpu", FakeStream(0x1000), made(log)) is a and cache.get(owner, (1, 32), "cpu", s2, made(log)) is b
    assert cache.get(owner, (1, 32), "cpu", None, made(log)) is default and cache.get(owner, (2, 32), "cpu", s1, made(log)) is other
    assert len(log) == 4
    assert list(cache.entries) == [(1, 32, 0x1000), (1, 32, 0x2000), (1, 32, None), (2, 32, 0x1000)]  # least recently used first
    assert not cache.pinned


def test_lru_bound_is_read_from_the_owner_and_holds_under_threads():
    """test_concurrency_host.py's recipe: eight threads with a stream each ask for two heads, against a bound of 4."""
    cache, owner, errors = WorkspaceCache(), Owner(), []
    owner.WORKSPACE_CACHE = 4               # (set on the instance, as the tests set dec.WORKSPACE_CACHE)
    heads = [(b, 32, 16) for b in (1, 2)]

    def work(i):
        s = FakeStream(0x100 * (i + 1))
        for r in range(40):
            head = heads[r % 2]
            ws = cache.get(owner, head, "cpu", s, lambda: torch.zeros(4))
            tag = getattr(ws, "_test_owner", None)
            if tag is None:
                ws._test_owner = (i, head)
            elif tag != (i, head):
                errors.append(f"thread {i} {head} got the workspace of {tag}")
            if len(cache.entries) > 4:
                errors.append("cache over its bound")

    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(work, range(8)))
    assert not errors, errors[:5]
    assert len(cache.entries) == 4
    owner.WORKSPACE_CACHE = 16              # with room for all of them every thread keeps one object per head
    first = [[cache.get(owner, h, "cpu", FakeStream(0x100 * (i + 1)), lambda: torch.zeros(4)) for h in heads] for i in range(8)]
    again = [[cache.get(owner, h, "cpu", FakeStream(0x100 * (i + 1)), lambda: torch.zeros(4)) for h in heads] for i in range(8)]
    assert all(x is y for f, a in zip(first, again) for x, y in zip(f, a)) and len(cache.entries) == 16


def test_pins_survive_eviction_are_released_by_predicate_and_warn(monkeypatch):
    """While a stream captures, what is handed out is pinned (test_host_cpu.py's stand-ins for a capturing GPU stream)."""
    class Fake(torch.Tensor):
        is_cuda = True
    capturing = {"on": True}
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing["on"])
    alloc = lambda: torch.Tensor._make_subclass(Fake, torch.empty(4))
    cache, owner = WorkspaceCache(), Owner()
    owner.WORKSPACE_CACHE = 3
    s = FakeStream(0x10)
    pinned = cache.get(owner, (1, 8), "cpu", s, alloc)
    capturing["on"] = False
    for b in range(2, 12):                  # eviction pressure: ten more heads through a cache of three
        cache.get(owner, (b, 8), "cpu", s, alloc)
    assert len(cache.entries) == 3 and cache.pinned == {(1, 8, 0x10)}
    assert cache.get(owner, (1, 8), "cpu", s, alloc) is pinned
    capturing["on"] = True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for b in (2, 3):
            cache.get(owner, (b, 9), "cpu", s, alloc)
        assert len(cache.pinned) == 3 and not w            # as many as the bound: no warning yet
        cache.get(owner, (4, 9), "cpu", s, alloc)
    assert [str(x.message) for x in w] == ["Owner: 4 workspaces are pinned by captured graphs (more than WORKSPACE_CACHE = 3); call "
                                           "release_pinned() for shapes whose graphs are gone"]
    assert w[0].category is RuntimeWarning
    assert cache.release_pinned(lambda k: k[1] == 9 and k[0] > 2) == 2
    assert cache.pinned == {(1, 8, 0x10), (2, 9, 0x10)} and (3, 9, 0x10) not in cache.entries and (2, 9, 0x10) in cache.entries
    assert cache.release_pinned(lambda k: True) == 2 and not cache.pinned
    assert (1, 8, 0x10) not in cache.entries


def test_native_hubert_releases_pins_by_shape(monkeypatch):
    class Fake(torch.Tensor):
        is_cuda = True
    hub = NativeHubert(SMALL, 2)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    monkeypatch.setattr(torch, "empty", lambda *a, _e=torch.empty, **k: torch.Tensor._make_subclass(Fake, _e(4)))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for b in range(hub.WORKSPACE_CACHE + 1):
            hub.workspace(1 + b, 4800 + 320 * (b % 2), "cpu")
    assert len(hub._pinned) == hub.WORKSPACE_CACHE + 1 and len(w) == 1 and str(w[0].message).startswith("NativeHubert: 9 workspaces are pinned")
    assert hub.release_pinned(B=1) == 1 and hub.release_pinned(T_audio=5120) == 4 and hub.release_pinned() == 4
    assert not hub._pinned and not hub._workspaces


# --------------------------------------------------------------------------------------------------------------------- copies
def test_copies_of_the_two_classes_start_empty():
    c, pb = make_blob()
    pb.get("k", [torch.zeros(3)])
    cache = WorkspaceCache()
    cache.get(Owner(), (1,), "cpu", None, lambda: torch.zeros(4))
    cache.pinned.add((1, None))
    for twin in (copy.deepcopy(pb), copy.copy(pb)):
        assert twin.blob is None and twin.sig is None and twin._event is None and not twin._waited and twin._lock is not pb._lock
        assert twin.get("k", [torch.zeros(3)]) is not pb.blob
    for twin in (copy.deepcopy(cache), copy.copy(cache), pickle.loads(pickle.dumps(cache))):
        assert not twin.entries and not twin.pinned and twin._lock is not cache._lock and twin.entries is not cache.entries
    twin = pickle.loads(pickle.dumps(PackedBlob(native.sem_packed_bytes, native.sem_pack, "w")))
    assert (twin._nbytes_of, twin._pack, twin._what) == (native.sem_packed_bytes, native.sem_pack, "w") and twin.blob is None


def _same_call(f, g):
    """the same library call, with the same bound keywords where it is a functools.partial"""
    return getattr(f, "func", f) is getattr(g, "func", g) and getattr(f, "keywords", None) == getattr(g, "keywords", None)


def _caches(m):
    return [v for mod in m.modules() for v in vars(mod).values() if isinstance(v, (PackedBlob, WorkspaceCache))]


@pytest.mark.parametrize("make, n_caches", [
    (lambda: FSQ([8, 5, 5]), 1),
    (lambda: FSQEncoder(16, [8, 5, 5], autograd=True), 3),
    (lambda: VectorQuantizer(16, 32), 2),
    (lambda: SemanticEncoder(CFG(device="cpu")), 5),
    (lambda: SemanticEncoder(CFG(device="cpu", use_fsq=False, codebook_size=64), autograd=True, train_vq=True), 4),
    (lambda: NativeHubert(SMALL, 2), 2),
    (lambda: NativeHubert(SMALL, 2, compute_dtype="bf16"), 2),
    (lambda: EdgeDiffusionDecoder(CFG(device="cpu"), kernels="generic", autograd=True), 2),
], ids=["FSQ", "FSQEncoder", "VectorQuantizer", "SemanticEncoder-fsq", "SemanticEncoder-vq", "NativeHubert", "NativeHubert-bf16",
        "EdgeDiffusionDecoder"])
def test_modules_copy_and_pickle(make, n_caches):
    m = make()
    mine = _caches(m)
    assert len(mine) == n_caches
    for twin in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert type(twin) is type(m)
        sd, sd2 = m.state_dict(), twin.state_dict()
        assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
        assert all(a.data_ptr() != b.data_ptr() for a, b in zip(m.parameters(), twin.parameters()))
        theirs = _caches(twin)
        assert [type(x) for x in theirs] == [type(x) for x in mine]
        for a, b in zip(mine, theirs):
            assert a is not b and a._lock is not b._lock
            if isinstance(b, PackedBlob):
                assert b.blob is None and b._event is None and _same_call(a._nbytes_of, b._nbytes_of) and _same_call(a._pack, b._pack)
            else:
                assert b.entries is not a.entries and b.pinned is not a.pinned and not b.entries
