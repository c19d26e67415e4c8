"""A whole training step as one graph, on the GPU: the key stream, dropout keys read from device memory, the
resident optimiser step with its device-side learning rate, blobs under capture and GraphedTrainStep.  Everything here is a
bitwise comparison (a replay is the eager step it stands for; a device key is the by-value seed) except the schedule, whose bound is
derived at its test.  Shapes: the small cases of tests/train_util.py and tests/sem_train_util.py.
Run on the GPU box: python -m pytest tests -m gpu."""
import copy

import pytest
import torch

import sem_train_util as SU
from edge_diffusion_tts_amd import (CFG, DiffusionObjective, DiffusionSchedule, EdgeDiffusionDecoder, FusedAdamW, GraphedTrainStep, KeyStream,
                                    SemanticEncoder, native, optim, synth_state_dict)
from edge_diffusion_tts_amd.synth import synth_hubert_features, synth_semantic_head
from train_util import CASES, case

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = 0.2
SEED = 0x5EED0123456789AB & (2 ** 63 - 1)
BF16 = dict(matmul_dtype="bf16", attn_dtype="bf16", tape_dtype="bf16")


def cu(t):
    return None if t is None else t.to(DEV)


# ---------------------------------------------------------------------------------------------- 1. the key stream
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_device_keys_equal_the_host_recomputation(n):
    """n: the edges of the one block's stride loop (256 threads).  Advance r writes keys_at(r) and leaves the counter at r + 1."""
    ks = KeyStream(SEED, n_slots=n - n // 2, n_rows=n // 2, device=DEV)
    for r in range(4):
        assert ks.counter() == r
        ks.advance()
        assert ks.keys.tolist() == ks.keys_at(r), (n, r)
        assert ks.counter() == r + 1
    assert ks.rows().shape == (n // 2,) and ks.rows().dtype == torch.int64 and bool((ks.keys >= 0).all())
    if n > 1:
        assert ks.slot(0).data_ptr() == ks.keys.data_ptr() and ks.rows().data_ptr() == ks.keys.data_ptr() + 8 * (n - n // 2)
    assert ks.keys_at(3) != ks.keys_at(2)


# ---------------------------------------------------------------------------------------------- 2. device key = by-value seed
class OneKey:
    """A stand-in for a KeyStream whose every slot holds one given seed (what take() hands to a forward)."""

    def __init__(self, seed):
        self.key = torch.tensor([seed], dtype=torch.int64, device=DEV)

    def take(self, owner, first_slot=0):
        return self.key


def decoder(name, ragged=False, **kw):
    cfg, sd, inp = case(name)
    cfg = copy.copy(cfg)
    cfg.dropout = P
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, train_dropout=True, train_lengths=ragged, **kw)
    dec.load_state_dict(sd)
    return dec.to(DEV).train(), inp


def decoder_step(dec, inp, lens):
    """One forward and backward: (eps, {name: gradient}, d_x, d_sem_features)."""
    dec.zero_grad(set_to_none=True)
    x = cu(inp["x"]).requires_grad_(True)
    f = None if inp["f"] is None else cu(inp["f"]).requires_grad_(True)
    eps = dec(x, cu(inp["t"]), cu(inp["sem"]), cu(inp["si"]), f, x_lengths=lens[0], sem_lengths=lens[1])
    ((eps - cu(inp["target"])) ** 2).mean().backward()
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in dec.named_parameters()}
    return eps.detach().clone(), grads, x.grad.clone(), None if f is None else f.grad.clone()


DTYPES = {"fp32": {}, "matmul_bf16": dict(matmul_dtype="bf16"), "matmul_attn_bf16": dict(matmul_dtype="bf16", attn_dtype="bf16"), "all_bf16": BF16}


@pytest.mark.parametrize("name,ragged,dt", [(n, False, d) for n in ("G2", "G4") for d in DTYPES] + [("G2", True, "fp32"), ("G4", True, "all_bf16")])
def test_decoder_with_a_device_key_is_bitwise_the_by_value_seed(name, ragged, dt):
    dec, inp = decoder(name, ragged, **DTYPES[dt])
    _, B, T, S, _, _ = CASES[name]
    lens = (None, None)
    if ragged:
        lens = (torch.tensor([T - 3 * b for b in range(B)], device=DEV), torch.tensor([max(S - 2 * b, 1) for b in range(B)], device=DEV))
    dec.dropout_generator = torch.Generator().manual_seed(99)
    want = decoder_step(dec, inp, lens)
    seed = dec.last_dropout_seed
    assert seed is not None
    dec.dropout_keys = (OneKey(seed), 0)
    got = decoder_step(dec, inp, lens)
    assert dec.last_dropout_seed is None
    assert torch.equal(got[0], want[0])
    assert set(got[1]) == set(want[1])
    for k, g in want[1].items():
        assert (g is None) == (got[1][k] is None), k
        assert g is None or torch.equal(got[1][k], g), k
    assert torch.equal(got[2], want[2]) and (want[3] is None or torch.equal(got[3], want[3]))
    # ... and the masks act, and another key gives another result
    dec.dropout_keys = (OneKey(seed ^ 1), 0)
    assert not torch.equal(decoder_step(dec, inp, lens)[0], want[0])


@pytest.mark.parametrize("name", ["G2", "G4"])
def test_mask_writers_with_a_device_key(name):
    dec, _ = decoder(name)
    _, B, T, S, _, _ = CASES[name]
    dims = dec.dims()
    for seed in (SEED, 7):
        key = torch.tensor([seed], dtype=torch.int64, device=DEV)
        for site in range(4):
            layer = site % dec.cfg.layers
            assert torch.equal(native.dropout_mask(dims, site, layer, B, T, S, P, key, DEV), native.dropout_mask(dims, site, layer, B, T, S, P, seed, DEV))
    key = torch.tensor([7], dtype=torch.int64, device=DEV)
    assert bool(native.dropout_mask(dims, 2, 0, B, T, S, 0.0, key, DEV).all())  # p = 0 keeps everything


@pytest.mark.parametrize("name,T", [("H3", 5), ("H2", 33)])
def test_semantic_head_with_a_device_key_is_bitwise_the_by_value_seed(name, T):
    in_dim, S, levels, p, B, _, proj_sd, q_sd, x, C = SU.case(name)
    cfg = CFG(device=DEV, use_fsq=True, semantic_dim=S, fsq_levels=list(levels), dropout=p)
    enc = SemanticEncoder(cfg, in_dim=in_dim, proj_dropout=True, autograd=True, train_dropout=True)
    enc.proj.load_state_dict(proj_sd)
    enc.vq.load_state_dict(q_sd)
    enc = enc.to(DEV).train()
    h, C = cu(x[:, :T].contiguous()), cu(C[:, :T].contiguous())

    def step():
        enc.zero_grad(set_to_none=True)
        zq, idx, _, _ = enc.quantize_features(h)
        (zq * C).sum().backward()
        return zq.detach().clone(), idx.clone(), [q.grad.clone() for q in enc.get_trainable_params()]

    enc.dropout_generator = torch.Generator().manual_seed(5)
    want = step()
    seed = enc.last_dropout_seed
    enc.dropout_keys = (OneKey(seed), 0)
    got = step()
    assert enc.last_dropout_seed is None
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert len(got[2]) == 10 and all(torch.equal(a, b) for a, b in zip(got[2], want[2]))
    enc.dropout_keys = (OneKey(seed ^ 1), 0)
    assert not torch.equal(step()[0], want[0])
    key = torch.tensor([seed], dtype=torch.int64, device=DEV)
    assert torch.equal(native.sem_dropout_mask(enc._dims(), B, T, p, key, DEV), native.sem_dropout_mask(enc._dims(), B, T, p, seed, DEV))


# ---------------------------------------------------------------------------------------------- 3. resident step = classic step
def optimiser_world(capturable, lr=3e-3):
    """A G2 student decoder (blob mirrored), an EMA teacher decoder (blob mirrored) and four loose tensors of 1, 3, one chunk and one
    chunk + 1 elements in a second group; gradients are set by hand."""
    cfg, sd, _ = case("G2")
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True)
    dec.load_state_dict(sd)
    teacher = EdgeDiffusionDecoder(cfg, kernels="generic")
    teacher.load_state_dict(sd)
    dec, teacher = dec.to(DEV), teacher.to(DEV)
    g = torch.Generator().manual_seed(3)
    chunk = native.optim_chunk_size()
    loose = [torch.nn.Parameter(torch.randn(n, generator=g).to(DEV)) for n in (1, 3, chunk, chunk + 1)]
    opt = FusedAdamW([{"params": list(dec.parameters())}, {"params": loose, "lr": lr if isinstance(lr, float) else lr.clone(), "weight_decay": 0.1}],
                     lr=lr if isinstance(lr, float) else lr.clone(), max_norm=1.0, skip_nonfinite=True, zero_grads=True, capturable=capturable)
    assert opt.attach_decoder(dec)
    opt.attach_ema(dec, teacher, 0.9)
    dec._ensure_packed()
    teacher._ensure_packed()
    return dec, teacher, loose, opt


def set_grads(params, step, poison=False):
    g = torch.Generator().manual_seed(100 + step)
    for i, p in enumerate(params):
        v = torch.randn(p.shape, generator=g).to(DEV)
        if poison and i == 2:
            v.view(-1)[0] = float("inf")
        if p.grad is None:
            p.grad = v
        else:
            p.grad.copy_(v)


def world_state(dec, teacher, loose, opt):
    out = {"p." + k: v.detach().clone() for k, v in dec.named_parameters()}
    out.update({"t." + k: v.detach().clone() for k, v in teacher.named_parameters()})
    out.update({f"loose.{i}": v.detach().clone() for i, v in enumerate(loose)})
    for i, p in enumerate(list(dec.parameters()) + loose):
        out[f"m.{i}"], out[f"v.{i}"] = opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()
        out[f"g.{i}"] = p.grad.clone()
    out["blob"], out["teacher_blob"] = dec._packed.clone(), teacher._packed.clone()
    out["state"] = opt._scratch[:32].clone()
    return out


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("mode", ["float_lr", "tensor_lr", "nonfinite"])
def test_resident_step_is_bitwise_the_classic_step(mode):
    tensor_lr = mode == "tensor_lr"
    classic = optimiser_world(False)
    resident = optimiser_world(True, torch.tensor(3e-3, dtype=torch.float64, device=DEV) if tensor_lr else 3e-3)
    lrs = (3e-3, 1e-3, 2.5e-4)
    for step in range(3):
        poison = mode == "nonfinite" and step == 1
        for dec, teacher, loose, opt in (classic, resident):
            set_grads(list(dec.parameters()) + loose, step, poison)
        if tensor_lr:  # the classic optimiser's group lr changed as the tensors are filled
            for g in classic[3].param_groups:
                g["lr"] = lrs[step]
            for g in resident[3].param_groups:
                g["lr"].fill_(lrs[step])
        before = world_state(*resident) if step else None
        na, nb = classic[3].step(), resident[3].step()
        assert torch.equal(na, nb), step
        a, b = world_state(*classic), world_state(*resident)
        same(a, b)
        if poison:  # nothing changes but the skip counter (and the norm that says why)
            assert resident[3].skipped_steps() == 1 and int(b["state"][:8].view(torch.int64)) == 1
            for k in before:
                if k != "state":
                    assert torch.equal(before[k], b[k]), k
        if tensor_lr:
            assert resident[3].current_lr() == [lrs[step]] * 2
    assert resident[3].skipped_steps() == (1 if mode == "nonfinite" else 0)
    # the blobs the steps kept current are the parameters: an eval forward packs nothing and equals a fresh decoder's
    for dec, teacher, loose, opt in (classic, resident):
        assert dec._mirror_target() is not None and teacher._mirror_target() is not None


def test_a_skipped_step_advances_the_schedule():
    total, warmup, base, low = 10, 2, 1e-3, 1e-6
    p = torch.nn.Parameter(torch.ones(5, device=DEV))
    opt = FusedAdamW([p], lr=base, skip_nonfinite=True, zero_grads=True, capturable=True)
    opt.device_lr_schedule("cosine", base, low, warmup, total)
    for n in range(5):
        p.grad = torch.full((5,), float("nan") if n in (1, 2) else 0.5, device=DEV)
        before = p.detach().clone()
        opt.step()
        assert abs(opt.current_lr()[0] - optim.cosine_lr(n, total, warmup, base, low)) <= 8 * 2.0 ** -53 * base, n
        assert torch.equal(p.detach(), before) == (n in (0, 1, 2))  # (n = 0: the warm-up's lr is 0; n = 1, 2: skipped)
    assert opt.skipped_steps() == 2 and opt._read_step() == 3


# ---------------------------------------------------------------------------------------------- 4. the schedule
def test_device_schedule_matches_the_python_formula():
    """Bound |d| <= 8 * 2^-53 * base_lr: the device and Python each round the products and the sum (two roundings at the scale of
    base_lr can differ) and the two cos() may differ by a few ulps of a value <= 1, scaled by 0.5 (base_lr - min_lr) <= base_lr."""
    total, warmup, base, low = 12, 4, 3e-4, 1e-6
    p = torch.nn.Parameter(torch.ones(3, device=DEV))
    opt = FusedAdamW([p], lr=123.0, zero_grads=True, capturable=True)
    opt.device_lr_schedule("cosine", base, low, warmup, total)
    want_n = {0, 1, warmup - 1, warmup, (warmup + total) // 2, total, total + 5}
    seen = {}
    for n in range(total + 6):
        p.grad = torch.full((3,), 0.25, device=DEV)
        opt.step()
        if n in want_n:
            seen[n] = opt.current_lr()[0]
    assert set(seen) == want_n
    for n, lr in sorted(seen.items()):
        want = optim.cosine_lr(n, total, warmup, base, low)
        print(f"n={n}: device {lr!r} python {want!r} diff {abs(lr - want):.3e}")
        assert abs(lr - want) <= 8 * 2.0 ** -53 * base, (n, lr, want)
    assert seen[0] == 0.0 and seen[total + 5] > seen[total]  # past total_steps the same formula goes on (the cosine turns up again)


# ---------------------------------------------------------------------------------------------- 5. - 6. the whole step
E2E_IN_DIM, SEM_DIM = 64, 16  # (the head's kernels need semantic_dim % 16 == 0: G2 with semantic_dim 16 in place of 7)


class World:
    """The G2 decoder (autograd, dropout 0.2, lengths), the FSQ head on synthetic HuBERT features, DiffusionObjective("v") seeded
    from the key stream, an EMA teacher and FusedAdamW(capturable) with clipping and the cosine schedule."""

    def __init__(self, attach=True, two=False, **kw):
        gkw, self.B, self.T, self.S, _, _ = CASES["G2"]
        cfg = CFG(device=DEV, use_fsq=True, **dict(gkw, semantic_dim=SEM_DIM), dropout=P)
        sd = synth_state_dict(cfg, 0)
        self.dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, train_dropout=True, train_lengths=True, **kw)
        self.dec.load_state_dict(sd)
        self.teacher = EdgeDiffusionDecoder(cfg, kernels="generic", **kw)
        self.teacher.load_state_dict(sd)
        proj_sd, q_sd = synth_semantic_head(E2E_IN_DIM, SEM_DIM, cfg.fsq_levels, seed=6, dropout_layout=True)
        self.enc = SemanticEncoder(cfg, in_dim=E2E_IN_DIM, proj_dropout=True, autograd=True, train_dropout=True)
        self.enc.proj.load_state_dict(proj_sd)
        self.enc.vq.load_state_dict(q_sd)
        self.dec, self.enc, self.teacher = self.dec.to(DEV).train(), self.enc.to(DEV).train(), self.teacher.to(DEV).eval()
        self.two = two
        self.keys = KeyStream(SEED, n_slots=3 if two else 2, n_rows=self.B, device=DEV)
        self.enc.dropout_keys, self.dec.dropout_keys = (self.keys, 0), (self.keys, 1)  # (the decoder's second forward: slot 2)
        self.obj = DiffusionObjective(DiffusionSchedule(cfg.diff_steps).to(DEV), "v")
        self.params = list(self.dec.parameters()) + self.enc.get_trainable_params()
        self.opt = FusedAdamW(self.params, lr=1e-3, max_norm=1.0, zero_grads=True, capturable=True)
        if attach:
            assert self.opt.attach_decoder(self.dec)
        self.opt.attach_ema(self.dec, self.teacher, 0.95)
        self.opt.device_lr_schedule("cosine", 2e-3, 1e-6, 2, 10)
        self.teacher._ensure_packed()
        self.cfg = cfg

    def batch(self, i):
        g = torch.Generator().manual_seed(1000 + i)
        B, T, S = self.B, self.T, self.S
        mel = torch.randn(B, T, self.cfg.n_mels, generator=g) * 2.0 - 4.0
        t = torch.randint(0, 1000, (B,), generator=g)
        t2 = torch.randint(0, 1000, (B,), generator=g)
        si = torch.randint(0, 16, (B,), generator=g)
        h = synth_hubert_features(B, S, E2E_IN_DIM, 300 + i)
        xl = torch.tensor([T - (i + b) % 4 for b in range(B)])
        sl = torch.tensor([S - (i + 2 * b) % 3 for b in range(B)])
        return tuple(cu(v) for v in (mel, t, t2, si, h, xl, sl))

    def fn(self, mel, t, t2, si, h, xl, sl):
        zq, _, _, _, _ = self.enc.forward_features(h, sl)
        prep = self.obj.prepare(mel, t, lengths=xl, seeds=self.keys.rows())
        pred = self.dec(prep.x_t, t, sem_features=zq, step_idx=si, x_lengths=xl, sem_lengths=sl)
        if not self.two:
            return self.obj.loss(pred, prep)
        prep2 = self.obj.prepare(mel, t2, like=prep)
        pred2 = self.dec(prep2.x_t, t2, sem_features=zq, step_idx=si, x_lengths=xl, sem_lengths=sl)
        return self.obj.consistency_loss(pred, prep, pred2, prep2)

    def eager(self, i, optimizer_step=True):
        self.keys.advance()
        loss = self.fn(*self.batch(i))
        loss.backward()
        return loss.detach().clone(), (self.opt.step().clone() if optimizer_step else None)

    def state(self):
        out = {"p." + k: v.detach().clone() for k, v in self.dec.named_parameters()}
        out.update({"e." + k: v.detach().clone() for k, v in self.enc.named_parameters()})
        out.update({"t." + k: v.detach().clone() for k, v in self.teacher.named_parameters()})
        for i, p in enumerate(self.params):
            if p in self.opt.state:
                out[f"m.{i}"], out[f"v.{i}"] = self.opt.state[p]["exp_avg"].clone(), self.opt.state[p]["exp_avg_sq"].clone()
        out["blob"], out["teacher_blob"] = self.dec._ensure_packed().clone(), self.teacher._packed.clone()
        out["opt"] = self.opt._scratch[:32].clone()
        out["lr"] = torch.tensor(self.opt.current_lr(), dtype=torch.float64)
        out["counter"] = torch.tensor([self.keys.counter()])
        return out


VARIANTS = {"mirrored": {}, "repack_in_graph": dict(attach=False), "bf16": BF16, "consistency": dict(two=True)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_graphed_step_is_bitwise_the_eager_step(variant):
    eager, graphed = World(**VARIANTS[variant]), World(**VARIANTS[variant])
    want = [eager.eager(i) for i in range(4)]
    step = GraphedTrainStep(graphed.fn, graphed.opt, graphed.batch(0), keys=graphed.keys, warmup=1)
    seen = []
    for i in (1, 2, 3):
        loss, norm = step(*graphed.batch(i))
        assert torch.equal(loss, want[i][0]) and torch.equal(norm, want[i][1]), (variant, i, float(loss), float(want[i][0]))
        seen.append(graphed.keys.keys.tolist())
        assert seen[-1] == graphed.keys.keys_at(i), i  # the keys move: replay i drew the keys of counter i
    assert len({tuple(k) for k in seen}) == 3 and all(len(set(k)) == len(k) for k in seen)
    assert float(want[3][0]) != float(want[2][0]) and bool(torch.isfinite(want[3][0]))
    same(eager.state(), graphed.state())
    assert graphed.keys.counter() == 4 and graphed.opt._read_step() == 4
    # no stale blob: an eval forward of the trained decoder is the forward of a fresh decoder loaded from its state_dict
    mel, t, _, si, h, xl, sl = graphed.batch(7)
    f = cu(torch.randn(graphed.B, graphed.S, SEM_DIM, generator=torch.Generator().manual_seed(1)))
    fresh = EdgeDiffusionDecoder(graphed.cfg, kernels="generic", **{k: v for k, v in VARIANTS[variant].items() if k.endswith("_dtype")})
    fresh.load_state_dict(graphed.dec.state_dict())
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        got = graphed.dec.eval()(mel, t, sem_features=f, step_idx=si, x_lengths=xl, sem_lengths=sl)
        ref = fresh(mel, t, sem_features=f, step_idx=si, x_lengths=xl, sem_lengths=sl)
    assert torch.equal(got, ref)
    with torch.no_grad():  # ... and the head's blobs follow its parameters too
        a = graphed.enc.eval().quantize_features(h, sl)[0]
        b = eager.enc.eval().quantize_features(h, sl)[0]
    assert torch.equal(a, b)


@pytest.mark.parametrize("scoped", [True, False])
def test_a_blob_that_is_current_when_the_capture_starts_is_packed_in_the_graph(scoped, monkeypatch):
    """The rule itself, not the version bumps of a warm-up: an eval forward right before the capture leaves every blob current, so
    only a pack INSIDE the graph keeps replay 2 from reading replay 1's parameters.  Inside capture_scope() each blob is packed once
    per graph; in a plain capture at every trainable get() (the head's backward asks again)."""
    from edge_diffusion_tts_amd._cache import capture_scope
    import contextlib
    eager, graphed = World(attach=False), World(attach=False)
    want = [eager.eager(i) for i in range(4)]
    w = graphed
    w.eager(0)
    static = [v.clone() for v in w.batch(1)]
    mel, t, _, si, h, xl, sl = static
    with torch.no_grad():  # validation between the warm-up and the capture: every blob is packed eagerly and is current
        w.dec.eval()(mel, t, sem_features=torch.zeros(w.B, w.S, SEM_DIM, device=DEV), step_idx=si, x_lengths=xl, sem_lengths=sl)
        w.enc.eval().quantize_features(h, sl)
    w.dec.train(), w.enc.train()
    assert w.dec._blob.sig == w.dec._blob.signature(w.dec.dims(), w.dec._slot_tensors()[1])
    assert w.enc._pack.sig == w.enc._pack.signature(w.enc._dims(), w.enc._slots())
    packs = {"decoder": 0, "head": 0}
    real_dec, real_sem = w.dec._blob._pack, w.enc._pack._pack  # (the blobs' own pack calls)
    monkeypatch.setattr(w.dec._blob, "_pack", lambda *a, **k: (packs.__setitem__("decoder", packs["decoder"] + 1), real_dec(*a, **k))[1])
    monkeypatch.setattr(w.enc._pack, "_pack", lambda *a, **k: (packs.__setitem__("head", packs["head"] + 1), real_sem(*a, **k))[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with (capture_scope() if scoped else contextlib.nullcontext()), torch.cuda.graph(graph):
        w.keys.advance()
        loss = w.fn(*static)
        loss.backward()
        norm = w.opt.step()
    assert packs == {"decoder": 1, "head": 1 if scoped else 2}, packs
    monkeypatch.undo()
    for i in (1, 2, 3):
        for dst, src in zip(static, w.batch(i)):
            dst.copy_(src)
        graph.replay()
        w.opt.replay_bookkeeping()
        assert torch.equal(loss, want[i][0]) and torch.equal(norm, want[i][1]), (i, float(loss), float(want[i][0]))
    same(eager.state(), w.state())


def test_first_slot_is_honoured():
    """dropout_keys = (stream, first_slot): the module's n-th forward since advance() reads slot first_slot + n."""
    dec, inp = decoder("G2")
    ks = KeyStream(SEED, n_slots=6, device=DEV)
    ks.advance()
    dec.dropout_keys = (ks, 3)
    a = decoder_step(dec, inp, (None, None))[0]
    b = decoder_step(dec, inp, (None, None))[0]
    assert not torch.equal(a, b)
    dec.dropout_keys = None
    for got, slot in ((a, 3), (b, 4)):
        dec.dropout_keys = (OneKey(ks.keys_at(0)[slot]), 0)
        assert torch.equal(decoder_step(dec, inp, (None, None))[0], got), slot
    dec.dropout_keys = (ks, 3)
    ks.advance()  # the cursor returns to first_slot, the keys are new
    c = decoder_step(dec, inp, (None, None))[0]
    dec.dropout_keys = (OneKey(ks.keys_at(1)[3]), 0)
    assert torch.equal(decoder_step(dec, inp, (None, None))[0], c)
    dec.dropout_keys = (ks, 5)
    ks.advance()
    decoder_step(dec, inp, (None, None))
    with pytest.raises(RuntimeError, match="slot 6"):
        decoder_step(dec, inp, (None, None))


def test_deferred_bookkeeping_is_applied_by_finish():
    eager, graphed = World(), World()
    for i in range(3):
        eager.eager(i)
    step = GraphedTrainStep(graphed.fn, graphed.opt, graphed.batch(0), keys=graphed.keys, bookkeeping=False)
    versions = [p._version for p in graphed.dec.parameters()]
    for i in (1, 2):
        step(*graphed.batch(i))
    assert [p._version for p in graphed.dec.parameters()] == versions  # a replay bumps nothing
    step.finish()
    assert all(p._version > v for p, v in zip(graphed.dec.parameters(), versions) if p.grad is not None)
    same(eager.state(), graphed.state())


def test_accumulation_replays_equal_the_eager_sequence():
    eager, graphed = World(), World()
    eager.eager(0)
    want = [eager.eager(1, False), eager.eager(2, False), eager.eager(3, True)]
    step = GraphedTrainStep(graphed.fn, graphed.opt, graphed.batch(0), keys=graphed.keys, accumulate=True)
    for i in (1, 2):
        (loss,) = step(*graphed.batch(i), optimizer_step=False)
        assert torch.equal(loss, want[i - 1][0]), i
    loss, norm = step(*graphed.batch(3))
    assert torch.equal(loss, want[2][0]) and torch.equal(norm, want[2][1])
    same(eager.state(), graphed.state())
    assert graphed.opt._read_step() == 2 and graphed.keys.counter() == 4


# ---------------------------------------------------------------------------------------------- 7. errors
def test_capture_errors_are_clear():
    p = torch.nn.Parameter(torch.ones(7, device=DEV))
    opt = FusedAdamW([p], lr=1e-3, zero_grads=True, capturable=True)
    p.grad = torch.ones(7, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="run one eager step first"):
            opt.step()
    opt.step()  # the eager first step: state and table
    before = p.detach().clone()
    p.grad = torch.ones(7, device=DEV)  # a new gradient tensor: another pointer
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match=r"changed under graph capture \(tensor 0: g\)"):
            opt.step()
    torch.cuda.synchronize()
    assert torch.equal(p.detach(), before)
    opt.step()  # outside a capture the same change uploads again
    assert not torch.equal(p.detach(), before) and opt._read_step() == 2
    # a parameter that gets its first gradient under capture: refused before its state is allocated
    a, b = torch.nn.Parameter(torch.ones(4, device=DEV)), torch.nn.Parameter(torch.ones(4, device=DEV))
    opt2 = FusedAdamW([a, b], lr=1e-3, zero_grads=True, capturable=True)
    a.grad = torch.ones(4, device=DEV)
    opt2.step()
    b.grad = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="gradient for the first time"):
            opt2.step()
    assert b not in opt2.state or "exp_avg" not in opt2.state[b]
    with pytest.raises(native.EdttsError, match="0-dim fp64"):
        q = torch.nn.Parameter(torch.ones(3, device=DEV))
        q.grad = torch.ones(3, device=DEV)
        FusedAdamW([q], lr=torch.tensor(1e-3, device=DEV), capturable=True).step()
