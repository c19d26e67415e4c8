"""FusedAdamW without a GPU: the chunk table, where the generic blob keeps each slot, the checkpoint format, the argument errors."""
import copy
import ctypes as C

import pytest
import torch

from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, FusedAdamW, native, optim

from train_util import CASES


def test_chunks_cover_every_element_once_in_order():
    chunk = optim.CHUNK
    assert chunk == native.optim_chunk_size() and chunk % 4 == 0 and chunk >= 64
    numels = [0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]
    table = optim.build_chunks(numels)
    covered = [0] * len(numels)
    last = -1
    for ti, off, cnt in table:
        assert ti >= last, "chunks are in tensor order"
        last = ti
        assert off % 4 == 0 and 1 <= cnt <= chunk
        assert off == covered[ti], "chunks of a tensor are in order, without gaps or overlaps"
        covered[ti] += cnt
    assert covered == numels
    assert not any(ti == 0 for ti, _, _ in table), "a tensor without elements has no chunk"
    assert len(table) == sum((n + chunk - 1) // chunk for n in numels)
    assert optim.build_chunks([]) == []
    assert native.optim_scratch_bytes(len(table), 2) > native.optim_scratch_bytes(1, 1) >= C.sizeof(native.EdttsOptimState)


def _dims(name, kernels="generic", compute_dtype="f32"):
    kw = CASES[name][0]
    return EdgeDiffusionDecoder(CFG(device="cpu", **kw), kernels=kernels, compute_dtype=compute_dtype)


@pytest.mark.parametrize("name", sorted(CASES))
def test_slot_dest_covers_the_blob_disjointly(name):
    dec = _dims(name)
    dims, names = dec.dims(), native.slot_names(dec.cfg.layers)
    total = native.packed_bytes(dims) // 4
    shapes = {k: tuple(v.shape) for k, v in dec._state_tensors().items()}
    spans, transposed = [], []
    for i, slot in enumerate(names):
        off, rows, cols, tr = native.generic_slot_dest(dims, i)
        shape = shapes[slot]
        assert rows * cols == int(torch.Size(shape).numel()), slot
        assert (rows, cols) == (shape if len(shape) == 2 else (1, shape[0])), slot
        assert 0 <= off and off + rows * cols <= total, slot
        spans.append((off, off + rows * cols, slot))
        if tr:
            transposed.append(slot)
    spans.sort()
    for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
        assert a1 <= b0, (an, bn)
    want = ["time_emb.1.weight", "time_emb.3.weight"] + [f"layers.{l}.{n}.proj.weight" for l in range(dec.cfg.layers) for n in ("norm1", "norm3")]
    assert sorted(transposed) == sorted(want)
    # every parameter of the decoder has a destination
    table = dec._mirror_map()
    assert set(table) == {k for k, _ in dec.named_parameters()}
    with pytest.raises(native.EdttsError, match="slot"):
        native.generic_slot_dest(dims, len(names))


def test_slot_dest_is_for_generic_fp32_dims_only():
    for dec in (EdgeDiffusionDecoder(CFG(device="cpu")), EdgeDiffusionDecoder(CFG(device="cpu"), kernels="auto"),
                EdgeDiffusionDecoder(CFG(device="cpu", hidden=256, heads=8), compute_dtype="bf16")):
        with pytest.raises(native.EdttsError, match=r"code -1"):
            native.generic_slot_dest(dec.dims(), 0)
        assert dec._mirror_map() is None
        assert FusedAdamW(dec.parameters(), lr=1e-3).attach_decoder(dec) is False


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(5, 3, generator=g).requires_grad_(True), torch.randn(7, generator=g).requires_grad_(True)]


def test_state_dict_round_trips_through_torch_adamw():
    ref_p = _params()
    ref = torch.optim.AdamW([dict(params=ref_p[:1], weight_decay=0.05), dict(params=ref_p[1:], weight_decay=0.0)], lr=2e-3, betas=(0.8, 0.95))
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        for p in ref_p:
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    sd = ref.state_dict()
    ours_p = _params()
    ours = FusedAdamW([dict(params=ours_p[:1]), dict(params=ours_p[1:])], lr=1.0)
    ours.load_state_dict(copy.deepcopy(sd))  # (torch's load_state_dict keeps the tensors it is given)
    assert ours._read_step() == 3
    assert all(set(st) == {"exp_avg", "exp_avg_sq"} for st in ours.state.values())
    back = ours.state_dict()
    assert back["param_groups"] == sd["param_groups"]
    assert set(back["state"]) == set(sd["state"])
    for k, st in sd["state"].items():
        assert set(back["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(back["state"][k]["step"]) == float(st["step"]) == 3.0
        assert back["state"][k]["step"].dtype == st["step"].dtype and back["state"][k]["step"].dim() == 0
        assert torch.equal(back["state"][k]["exp_avg"], st["exp_avg"]) and torch.equal(back["state"][k]["exp_avg_sq"], st["exp_avg_sq"])
    # ... and back into torch: a fresh AdamW loaded from OUR dict continues exactly as the original does
    new_p = [p.detach().clone().requires_grad_(True) for p in ref_p]
    new = torch.optim.AdamW([dict(params=new_p[:1]), dict(params=new_p[1:])], lr=1.0)
    new.load_state_dict(copy.deepcopy(back))
    for p, q in zip(ref_p, new_p):
        p.grad = torch.randn(p.shape, generator=g)
        q.grad = p.grad.clone()
    ref.step()
    new.step()
    for p, q in zip(ref_p, new_p):
        assert torch.equal(p, q)
    # a fresh FusedAdamW: step 0, no state, the AdamW group keys
    fresh = FusedAdamW(_params(), lr=1e-3).state_dict()
    assert fresh["state"] == {} and set(fresh["param_groups"][0]) == set(sd["param_groups"][0])


def test_load_state_dict_rejects_unequal_steps_and_unbuilt_variants():
    ps = _params()
    ref = torch.optim.AdamW(ps, lr=1e-3)
    ps[0].grad = torch.ones_like(ps[0])
    ref.step()
    ps[1].grad = torch.ones_like(ps[1])
    ref.step()  # steps 2 and 1
    ours = FusedAdamW(_params(), lr=1e-3)
    with pytest.raises(ValueError, match="one step counter"):
        ours.load_state_dict(ref.state_dict())
    ams = torch.optim.AdamW(_params(), lr=1e-3, amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        ours.load_state_dict(ams.state_dict())


def test_argument_errors():
    with pytest.raises(ValueError, match="learning rate"):
        FusedAdamW(_params(), lr=-1.0)
    with pytest.raises(ValueError, match="betas"):
        FusedAdamW(_params(), lr=1e-3, betas=(1.0, 0.9))
    with pytest.raises(ValueError, match="max_norm"):
        FusedAdamW(_params(), lr=1e-3, max_norm=-1.0)
    # no CPU fallback: a step on CPU tensors raises (and creates no state)
    ps = _params()
    opt = FusedAdamW(ps, lr=1e-3, max_norm=1.0)
    assert opt.step() is None  # no gradient anywhere: nothing to do, as torch
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(native.EdttsError, match="HIP device"):
        opt.step()
    assert all(torch.equal(a, b) for a, b in zip(before, ps)) and not any(len(s) for s in opt.state.values())
    with pytest.raises(ValueError, match="closure"):
        opt.step(lambda: 0.0)
    # dtype and layout are checked before the device for no tensor: the messages name them (the device check comes first on CPU)
    chk = FusedAdamW._check

    class _Fake:
        is_cuda, dtype, device = True, torch.float64, "cuda:0"

        def is_contiguous(self):
            return True

    with pytest.raises(native.EdttsError, match="float32"):
        chk(_Fake(), "parameter")
    fake = _Fake()
    fake.dtype = torch.float32
    fake.is_contiguous = lambda: False
    with pytest.raises(native.EdttsError, match="contiguous"):
        chk(fake, "parameter")
    # the library's own argument checks need no GPU either
    L = native.lib()
    t = (native.EdttsOptimTensor * 1)()
    g = (native.EdttsOptimGroup * 1)()
    with pytest.raises(native.EdttsError, match="code -2"):
        L.edtts_optim_step(t, 1, g, 1, 1.0, 0, None, 0, None)       # no scratch
    t[0].numel, t[0].p = 4, 16
    with pytest.raises(native.EdttsError, match="NULL p, g, m, v"):
        L.edtts_optim_step(t, 1, g, 1, 1.0, 0, 16, 1 << 20, None)   # g, m, v missing (rejected before any pointer is used)
    with pytest.raises(native.EdttsError, match="flag"):
        L.edtts_optim_step(t, 1, g, 1, 1.0, 64, 16, 1 << 20, None)
    with pytest.raises(ValueError, match="decay"):
        opt.attach_ema(torch.nn.Linear(2, 2), torch.nn.Linear(2, 2), decay=1.5)
    with pytest.raises(ValueError, match="differ"):
        opt.attach_ema(torch.nn.Linear(2, 2), torch.nn.Linear(3, 2))
