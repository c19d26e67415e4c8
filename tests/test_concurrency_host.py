"""Several streams and threads on one decoder, host side: the workspace cache keys on the stream and on the sub-batch cut, and
stays consistent under a thread pool.  No GPU needed: streams are stand-ins that carry a handle, and the cut is a host query
(include/edtts.h: edtts_substreams_for)."""
import copy
from concurrent.futures import ThreadPoolExecutor

import torch

from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, native


class FakeStream:
    """What decoder.workspace() reads of a torch stream: its handle."""
    def __init__(self, handle):
        self.cuda_stream = handle


def test_stream_keyword_keys_the_workspace():
    dec = EdgeDiffusionDecoder(CFG(device="cpu"))
    default = dec.workspace(1, 32, 16, 1, "cpu")
    s1, s2 = FakeStream(0x1000), FakeStream(0x2000)
    a = dec.workspace(1, 32, 16, 1, "cpu", stream=s1)
    b = dec.workspace(1, 32, 16, 1, "cpu", stream=s2)
    assert a is not b and a is not default and b is not default
    assert a.data_ptr() != b.data_ptr()
    # each stream keeps its own, and the call without a stream still gets the one it had
    assert dec.workspace(1, 32, 16, 1, "cpu", stream=FakeStream(0x1000)) is a
    assert dec.workspace(1, 32, 16, 1, "cpu", stream=s2) is b
    assert dec.workspace(1, 32, 16, 1, "cpu") is default
    assert a.numel() == b.numel() == default.numel() and not bool(a.any()) and not bool(b.any())
    # release_pinned still selects by (B, T, S): the stream is part of the key, not of its head
    assert all(k[:3] == (1, 32, 16) for k in dec._workspaces)


def test_cut_setting_keys_the_workspace():
    """A setting change (edtts_set_substreams) never hands out a workspace that served another cut; the byte count covers every
    cut, so it does not change with the setting."""
    dec = EdgeDiffusionDecoder(CFG(device="cpu"))
    B, T, S = 128, 512, 256  # (two rounds of waves: the smallest batch the default setting cuts)
    prev = native.set_substreams(1)
    try:
        assert native.substreams_for(dec.dims(), B, T) == 1
        one = dec.workspace(B, T, S, 4, "cpu")
        bytes_one = native.workspace_bytes(dec.dims(), B, T, S, 4)
        native.set_substreams(4)
        assert native.substreams_for(dec.dims(), B, T) == 2
        cut = dec.workspace(B, T, S, 4, "cpu")
        assert cut is not one and native.workspace_bytes(dec.dims(), B, T, S, 4) == bytes_one == cut.numel()
        assert dec.workspace(B, T, S, 4, "cpu") is cut
        native.set_substreams(1)
        assert dec.workspace(B, T, S, 4, "cpu") is one
        # a batch too small to cut has one layout under every setting: one workspace
        small = dec.workspace(2, T, S, 4, "cpu")
        native.set_substreams(4)
        assert dec.workspace(2, T, S, 4, "cpu") is small
    finally:
        native.set_substreams(prev)


def test_workspace_cache_is_thread_safe():
    """Eight threads, each with a stream of its own, ask for workspaces of two shapes.  With room for all of them every thread
    gets one object per shape for good; with a small cache that keeps evicting, no thread ever gets a workspace another thread's
    stream was handed, and the cache never grows past its bound."""
    shapes = [(b, 32, 16, 1) for b in (1, 2)]

    def run(dec, rounds):
        errors = []

        def work(i):
            s = FakeStream(0x100 * (i + 1))
            mine = {}
            for r in range(rounds):
                shape = shapes[r % len(shapes)]
                ws = dec.workspace(*shape, "cpu", stream=s)
                owner = getattr(ws, "_test_owner", None)
                if owner is None:
                    ws._test_owner = (i, shape)
                elif owner != (i, shape):
                    errors.append(f"thread {i} {shape} got the workspace of {owner}")
                mine.setdefault(shape, []).append(ws)
                if len(dec._workspaces) > dec.WORKSPACE_CACHE:
                    errors.append("cache over its bound")
            return mine

        with ThreadPoolExecutor(max_workers=8) as pool:
            results = list(pool.map(work, range(8)))
        assert not errors, errors[:5]
        assert len(dec._workspaces) <= dec.WORKSPACE_CACHE
        return results

    dec = EdgeDiffusionDecoder(CFG(device="cpu"))
    dec.WORKSPACE_CACHE = 16
    for mine in run(dec, 100):
        assert all(all(w is ws[0] for w in ws) for ws in mine.values())
    assert len(dec._workspaces) == 16
    small = EdgeDiffusionDecoder(CFG(device="cpu"))
    small.WORKSPACE_CACHE = 4
    run(small, 40)


def test_decoder_copies_get_their_own_lock():
    dec = EdgeDiffusionDecoder(CFG(device="cpu"))
    dec.workspace(1, 32, 16, 1, "cpu")
    twin = copy.deepcopy(dec)
    assert twin._blob is not dec._blob and twin._blob._lock is not dec._blob._lock and twin._blob._event is None
    assert twin._ws is not dec._ws and twin._ws._lock is not dec._ws._lock
    assert twin.workspace(1, 32, 16, 1, "cpu") is not dec.workspace(1, 32, 16, 1, "cpu")
    assert torch.equal(twin.in_proj.weight, dec.in_proj.weight)
