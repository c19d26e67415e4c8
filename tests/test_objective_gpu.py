"""DiffusionObjective on the GPU against the oracle of tests/objective_util.py, and the bitwise clauses of the contract in
include/edtts.h ("training objective") / DESIGN.md section 25.  Bar, as in tests/test_train_gpu.py: every quantity
E <= MARGIN * max(E_ref, median E_ref) against the fp64 oracle, E_ref the fp32 oracle's error (a scalar's floored at one fp32 ulp).
Run on the GPU box: python -m pytest tests -m gpu."""
import pytest
import torch

import objective_util as U
from edge_diffusion_tts_amd import DiffusionObjective, DiffusionSchedule, EdgeDiffusionDecoder, FusedAdamW, native
from train_util import check_against_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEEDS = (11, 2 ** 63 + 5, 7)  # (one beyond int64: a seed is any 64-bit pattern)


def cu(t):
    return None if t is None else t.to(DEV)


@pytest.fixture(scope="module")
def schedule():
    return DiffusionSchedule(U.T_DIFF).to(DEV)


def objective(schedule, kind="v", **kw):
    return DiffusionObjective(schedule, prediction="eps" if kind == "eps" else "v", **kw)


def run(obj, inp, kind, lengths=True, seeds=None, grad=True, factor=None, parts=True):
    """prepare -> the loss of `kind` on the case's recorded predictions -> backward.  Everything stays on the device."""
    B = inp["mel"].shape[0]
    mel, t = cu(inp["mel"]), cu(inp["t"])
    lens = cu(inp["lengths"]) if lengths is True else cu(lengths) if lengths is not None and lengths is not False else None
    noise = dict(seeds=list(seeds[:B])) if seeds is not None else dict(noise=cu(inp["noise"]))
    prep = obj.prepare(mel, t, lens, parts=parts, **noise)
    pred = cu(inp["pred"]).requires_grad_(grad)
    pred2 = cu(inp["pred2"]).requires_grad_(grad and kind == "consistency")
    if kind in ("v", "eps"):
        loss = obj.loss(pred, prep)
    elif kind == "distill":
        loss = obj.distill_loss(pred, pred2, prep)
    else:
        loss = obj.consistency_loss(pred, prep, pred2, obj.prepare(mel, cu(inp["t2"]), like=prep))
    if grad:
        (loss if factor is None else loss * factor).backward()
    out = dict(loss=loss.detach(), x_t=prep.x_t, x0_mse=obj.last_metrics["x0_mse"], x0_cos=obj.last_metrics["x0_cos"],
               terms=obj.last_metrics["terms"][:3 if kind == "consistency" else 1])
    if obj.normalize:
        out.update(mean=prep.mean, std=prep.std)
    if parts:
        out.update(target=prep.target, noise=prep.noise, mel_n=prep.mel_n)
    if grad:
        out["d_pred"] = pred.grad
        if kind == "consistency":
            out["d_pred2"] = pred2.grad
    return out


def cpu(d):
    return {k: v.detach().cpu() for k, v in d.items()}


def assert_same(a, b, what=""):
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    for k in a:
        x, y = a[k].detach().cpu(), b[k].detach().cpu()
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what} {k}: {int((x != y).sum())} elements differ"


def garbage(inp, nan=float("nan")):
    """A copy of the case with every padded frame of mel, noise, pred and pred2 overwritten."""
    out = dict(inp)
    for k in ("mel", "noise", "pred", "pred2"):
        out[k] = inp[k].masked_fill(~U.frame_mask(inp["lengths"], inp[k].shape[1]), nan)
    return out


# ------------------------------------------------------------------------------------------------------------ 1. noise
@pytest.mark.parametrize("name", ["O1", "O2", "O3"])
def test_noise_is_the_rows_philox_stream(schedule, name):
    inp = U.case(name)
    B, T, M = inp["mel"].shape
    obj = objective(schedule)
    want = native.randn_rows((B, T * M), DEV, list(SEEDS[:B]), stream_id=0x54).view(B, T, M)
    full = obj.prepare(cu(inp["mel"]), cu(inp["t"]), seeds=list(SEEDS[:B]), parts=True)
    assert torch.equal(full.noise, want)
    assert full.seeds.dtype == torch.int64 and full.seeds.is_cuda
    lens = cu(inp["lengths"])
    prep = obj.prepare(cu(inp["mel"]), cu(inp["t"]), lens, seeds=list(SEEDS[:B]), parts=True)
    live = U.frame_mask(lens, T)
    assert torch.equal(prep.noise, want * live)
    # the seeds of obj.generator: a CPU generator's draws, repeatable, and a different batch every call
    obj.generator = torch.Generator().manual_seed(3)
    a = obj.prepare(cu(inp["mel"]), cu(inp["t"]), lens)
    b = obj.prepare(cu(inp["mel"]), cu(inp["t"]), lens)
    obj.generator = torch.Generator().manual_seed(3)
    c = obj.prepare(cu(inp["mel"]), cu(inp["t"]), lens)
    assert torch.equal(a.seeds, c.seeds) and torch.equal(a.x_t, c.x_t) and not torch.equal(a.seeds, b.seeds)
    # row b is the row alone with its seed: in its padded length, and trimmed to its frames (another T M: maybe the other path)
    for b_, L in enumerate(inp["lengths"].tolist()):
        solo = obj.prepare(cu(inp["mel"][b_:b_ + 1]).contiguous(), cu(inp["t"][b_:b_ + 1]), lens[b_:b_ + 1], seeds=[SEEDS[b_]], parts=True)
        for k in ("x_t", "noise", "mel_n", "target", "mean", "std"):
            assert torch.equal(getattr(solo, k)[0], getattr(prep, k)[b_]), (b_, k)
        trimmed = obj.prepare(cu(inp["mel"][b_:b_ + 1, :L]).contiguous(), cu(inp["t"][b_:b_ + 1]), seeds=[SEEDS[b_]], parts=True)
        for k in ("x_t", "noise", "mel_n", "target"):
            assert torch.equal(getattr(trimmed, k)[0], getattr(prep, k)[b_, :L]), (b_, k, "trimmed")


# ------------------------------------------------------------------------------------------------------------ 2. accuracy
@pytest.mark.parametrize("kind", U.KINDS)
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_against_the_fp64_oracle(schedule, name, kind):
    """Injected noise, garbage in the padding.  Worst ratio measured on MI355X: DESIGN.md section 25."""
    inp = U.case(name)
    o64, o32 = U.pair(name, kind)
    obj = objective(schedule, kind)
    got = cpu(run(obj, garbage(inp), kind))
    for k in ("noise", "mel_n"):
        got.pop(k)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    U.check(got, o64, o32, f"{name} {kind}")
    # a non-unit upstream factor reaches the gradient through k_obj_scale
    grads = ("d_pred", "d_pred2") if kind == "consistency" else ("d_pred",)
    got = cpu(run(obj, inp, kind, factor=0.25, parts=False))
    U.check({k: got[k] for k in grads + ("loss",)}, o64, o32, f"{name} {kind} x 0.25", scale={k: 0.25 for k in grads})


@pytest.mark.parametrize("kind", ["v", "consistency"])
def test_without_lengths_against_the_padded_oracle(schedule, kind):
    o64, o32 = U.pair("O1", kind, False)
    got = cpu(run(objective(schedule, kind), U.case("O1"), kind, lengths=False))
    for k in ("noise", "mel_n"):
        got.pop(k)
    U.check(got, o64, o32, f"O1 padded {kind}")


# ------------------------------------------------------------------------------------------------------------ 3. ragged clauses
@pytest.mark.parametrize("kind", U.KINDS)
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_padding_and_scratch_contents_change_no_bit(schedule, name, kind):
    inp = U.case(name)
    obj = objective(schedule, kind)
    clean = cpu(run(obj, garbage(inp, 0.0), kind))
    assert obj._ws.entries
    for ws in obj._ws.entries.values():
        ws.fill_(0xFF)
    dirty = cpu(run(obj, garbage(inp), kind))
    assert_same(clean, dirty, f"{name} {kind}")
    assert all(bool(torch.isfinite(v).all()) for v in dirty.values())
    # exactly 0 past the lengths (and, for the gradient, past the aligned length Tm)
    lens, T = inp["lengths"], inp["mel"].shape[1]
    tm = U._tm(kind, T, inp["pred"].shape[1], inp["pred2"].shape[1])
    for k in ("x_t", "target", "noise", "mel_n"):
        assert float(dirty[k].masked_select(~U.frame_mask(lens, T)).abs().sum()) == 0.0, k
    for k in ("d_pred", "d_pred2"):
        if k in dirty:
            dead = ~U.frame_mask(lens.clamp(max=tm), dirty[k].shape[1])
            assert float(dirty[k].masked_select(dead).abs().sum()) == 0.0, k
            assert float(dirty[k].abs().max()) > 0


@pytest.mark.parametrize("kind", ["v", "eps", "consistency"])
@pytest.mark.parametrize("name", ["O1", "O2", "O2-long"])
def test_full_lengths_are_the_call_without_lengths(schedule, name, kind):
    inp = U.case(name)
    B, T, _ = inp["mel"].shape
    obj = objective(schedule, kind)
    assert_same(run(obj, inp, kind, lengths=False), run(obj, inp, kind, lengths=torch.full((B,), T)), f"{name} {kind}")


# ------------------------------------------------------------------------------------------------------------ 4. reproducibility
def test_two_calls_give_the_same_bits(schedule):
    inp = U.case("O2")
    obj = objective(schedule)
    for kind in ("v", "consistency"):
        assert_same(run(obj, inp, kind, seeds=SEEDS), run(obj, inp, kind, seeds=SEEDS), kind)
    a, b = run(obj, inp, "v", seeds=SEEDS), run(obj, inp, "v", seeds=SEEDS[::-1])
    assert not torch.equal(a["x_t"], b["x_t"])


def test_streams_have_a_scratch_each_and_split_batches_agree(schedule):
    """The batch and its two halves (rows 0 .. 1 | row 2 of O1, the row order kept), issued on two streams at once: each is bitwise
    its serial run, every stream has a scratch of its own in the WorkspaceCache, and the halves' sums add up to the batch's loss."""
    inp = U.case("O1")
    halves = [{k: v[:2] for k, v in inp.items()}, {k: v[2:] for k, v in inp.items()}]
    obj = objective(schedule)
    serial = [cpu(run(obj, h, "consistency", seeds=SEEDS[i * 2:])) for i, h in enumerate(halves)]
    serial_full = cpu(run(obj, inp, "consistency", seeds=SEEDS))
    n_serial = len(obj._ws.entries)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    out = []
    for rounds in range(2):  # all four calls are in flight before the first result is read
        for i, s in enumerate(streams):
            with torch.cuda.stream(s):
                out.append(run(obj, halves[i], "consistency", seeds=SEEDS[i * 2:]) if rounds == 0 else run(obj, inp, "consistency", seeds=SEEDS))
    torch.cuda.synchronize()
    for i in range(2):
        assert_same(serial[i], out[i], f"half {i}")
        assert_same(serial_full, out[2 + i], f"batch on stream {i}")
    keys = list(obj._ws.entries)
    assert len(keys) == n_serial + 4 and len({k[-1] for k in keys}) == 3, keys  # (2 shapes) x (the default stream + two more)
    n = [float(h["lengths"].sum()) for h in halves]
    for k in ("loss", "x0_mse"):
        both = (serial[0][k].double() * n[0] + serial[1][k].double() * n[1]) / (n[0] + n[1])
        assert abs(float(both) - float(serial_full[k])) <= 4 * 2.0 ** -23 * abs(float(both)), k


# ------------------------------------------------------------------------------------------------------------ 5. composition
def decoder_chain(name, optimiser=False, sync=False):
    """mel -> prepare -> the decoder (autograd) -> loss -> backward [-> FusedAdamW.step]: (gradients, loss, decoder)."""
    cfg, sd, inp, t_len, s_len, oinp = U.chain_inputs(name)
    ragged = t_len is not None
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, train_lengths=ragged)
    dec.load_state_dict(sd)
    dec = dec.to(DEV).eval()
    opt = None
    if optimiser:
        opt = FusedAdamW(dec.parameters(), lr=2e-3, weight_decay=0.01, max_norm=0.5)
        assert opt.attach_decoder(dec) is True
    wait = torch.cuda.synchronize if sync else (lambda: None)
    obj = DiffusionObjective(DiffusionSchedule(U.T_DIFF).to(DEV), normalize=not ragged)
    t, lens = cu(inp["t"]), cu(t_len)
    f = None if inp["f"] is None else cu(inp["f"]).requires_grad_(True)
    wait()
    prep = obj.prepare(cu(oinp["mel"]), t, lens, noise=cu(oinp["noise"]))
    wait()
    kw = dict(x_lengths=lens, sem_lengths=cu(s_len)) if ragged else {}
    pred = dec(prep.x_t, t, cu(inp["sem"]), cu(inp["si"]), f, **kw)
    wait()
    loss = obj.loss(pred, prep)
    wait()
    loss.backward()
    got = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in dec.named_parameters()}
    if f is not None:
        got["d_sem_features"] = f.grad.detach().clone()
    if opt is not None:
        wait()
        opt.step()
    return got, loss.detach(), dec


@pytest.mark.parametrize("name", ["G2", "R1"])
def test_decoder_gradients_through_the_objective(name):
    g64, e_ref, med, l64 = U.chain_pair(name)
    got, loss, _ = decoder_chain(name)
    assert abs(float(loss) - float(l64)) <= 1e-4 * abs(float(l64))  # (the decoder's forward tolerance, tests/test_generic_gpu.py)
    check_against_oracle(got, g64, e_ref, med, f"{name} chain")


def test_a_whole_step_never_waits_for_the_host():
    """prepare, decoder, loss, backward and FusedAdamW.step() enqueued back to back give bitwise the parameters of the same step
    with a device synchronisation between all of them."""
    _, _, a = decoder_chain("R1", optimiser=True, sync=False)
    _, _, b = decoder_chain("R1", optimiser=True, sync=True)
    cfg, sd, *_ = U.chain_inputs("R1")
    moved = 0
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), k
        assert bool(torch.isfinite(p).all()), k
        moved += int(not torch.equal(p.detach().cpu(), sd[k]))
    assert moved > 40


@pytest.mark.parametrize("name", ["O1", "O2"])
def test_prepare_loss_and_scale_replay_from_a_graph(schedule, name):
    """prepare + loss + the backward's k_obj_scale captured once (the decoder and the optimiser stay outside):
    a replay on new contents of the same buffers is bitwise the eager call."""
    inp = U.case(name)
    B = inp["mel"].shape[0]
    obj = objective(schedule)
    mel, t, lens = cu(inp["mel"]), cu(inp["t"]), cu(inp["lengths"])
    seeds = native.seed_tensor(list(SEEDS[:B]), B, DEV)
    pred = cu(inp["pred"]).requires_grad_(True)

    def step():
        prep = obj.prepare(mel, t, lens, seeds=seeds)
        loss = obj.loss(pred, prep)
        (d,) = torch.autograd.grad(loss * 0.5, pred)
        return dict(x_t=prep.x_t, loss=loss.detach(), d_pred=d, **{k: v for k, v in obj.last_metrics.items()})

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # the warm-up: the schedule's tables and the scratch exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    assert obj._ws.pinned
    with torch.no_grad():  # new contents: another prediction, other seeds, other timesteps, shorter rows
        pred.copy_(cu(inp["pred2"][:, :pred.shape[1]]))
        seeds.copy_(native.seed_tensor([5, 6, 7][:B], B, DEV))
        t.copy_(cu(inp["t2"]))
        lens.copy_((lens - 1).clamp(min=2))
    graph.replay()
    torch.cuda.synchronize()
    replayed = cpu(captured)
    assert_same(replayed, cpu(step()), name)
    assert float(replayed["d_pred"].abs().max()) > 0
    del graph
    assert obj.release_pinned_workspaces() >= 1


# ------------------------------------------------------------------------------------------------------------ 6. no grad
@pytest.mark.parametrize("kind", U.KINDS)
def test_no_grad_gives_the_same_bits_and_writes_no_gradient(schedule, kind, monkeypatch):
    inp = U.case("O2")
    obj = objective(schedule, kind)
    with_grad = run(obj, inp, kind)
    units = []
    real = native.objective_loss

    def spy(*a, **k):
        out = real(*a, **k)
        units.append(out[1:])
        return out

    monkeypatch.setattr(native, "objective_loss", spy)
    with torch.no_grad():
        without = run(obj, inp, kind, grad=False)
    assert units == [(None, None)]
    assert not without["loss"].requires_grad
    for k in ("d_pred", "d_pred2"):
        with_grad.pop(k, None)
    assert_same(with_grad, without, kind)
    # predictions that need no gradient, grad mode on: the same
    assert_same(without, run(obj, inp, kind, grad=False), kind)
    assert units[-1] == (None, None)
