"""Training the VQ head on the GPU: SemanticEncoder(train_vq=True) / VectorQuantizer(autograd=True) against
the CPU oracle of tests/vq_train_util.py.  The bar is the project's: every float within MARGIN x max(E_ref, median E_ref) of the fp64
oracle, E_ref being the fp32 oracle's own error; idx must equal the oracles' on EVERY frame (the cases are chosen so that no argmin
is close: tests/test_vq_train_host.py).  Run on the GPU box: python -m pytest tests -m gpu.

Every test prints the ratios it asserts on; DESIGN.md section 23 is where the worst one per case is recorded."""
import copy

import pytest
import torch

import train_util as TU
import vq_train_util as U
from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, native
from edge_diffusion_tts_amd.encoder import SemanticEncoder, VectorQuantizer

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cu(t):
    return None if t is None else t.to(DEV)


def make(name, dropout=False, gen=None, train=True, reset_every=100):
    """(module, its VectorQuantizer, canonical name -> parameter name, features on the device, C on the device) of a case; dropout:
    the case's p with train_dropout (a Dropout-layout case without it runs with p = 0)"""
    in_dim, S, K, p, B, T, proj_sd, q_sd, x, C = U.case(name)
    if in_dim == 0:
        enc = VectorQuantizer(S, K, commit=U.COMMIT, decay=U.DECAY, epsilon=U.EPSILON, reset_unused_every=reset_every, autograd=True)
        enc.load_state_dict(q_sd)
        vq, names = enc, U.param_names(0, False, "")
    else:
        layout = p is not None
        cfg = CFG(device=DEV, use_fsq=False, codebook_size=K, semantic_dim=S, vq_commit=U.COMMIT, dropout=p if dropout else 0.0)
        enc = SemanticEncoder(cfg, in_dim=in_dim, proj_dropout=layout, autograd=True, train_vq=True, train_dropout=layout and dropout)
        enc.proj.load_state_dict(proj_sd)
        enc.vq.load_state_dict(q_sd)
        vq, names = enc.vq, U.param_names(in_dim, layout)
        vq.reset_unused_every = reset_every
        assert (vq.commit, vq.decay, vq.epsilon) == (U.COMMIT, U.DECAY, U.EPSILON)
        if gen is not None:
            enc.dropout_generator = torch.Generator().manual_seed(gen)
    enc = enc.to(DEV)
    enc.train(train)
    return enc, vq, names, cu(x), cu(C)


def call(enc, x, lengths=None):
    """(z_q, idx, vq_loss, perplexity, used) of a call"""
    return enc(x, lengths) if isinstance(enc, VectorQuantizer) else enc.forward_features(x, lengths)


def step(enc, vq, names, x, C, lengths=None, with_zq=True, leaf=False, loss_w=U.LOSS_W):
    """forward, (z_q . C).sum() [with_zq] + loss_w vq_loss, backward: the oracle's result dict (idx and z_q of the whole batch)"""
    enc.zero_grad(set_to_none=True)
    xin = x.clone().requires_grad_(True) if leaf else x
    zq, idx, loss, ppl, used = call(enc, xin, lengths)
    assert not idx.requires_grad
    obj = loss_w * loss
    if with_zq:
        assert zq.grad_fn is not None
        obj = obj + (zq * C).sum()
    obj.backward()
    params = dict(enc.named_parameters())
    out = {"g." + k: (None if params[n].grad is None else params[n].grad.detach().clone()) for k, n in names.items()}
    if leaf:
        out["g.d_z"] = xin.grad.detach().reshape(-1, xin.shape[-1]).clone()
    out.update(idx=idx.detach().clone(), zq=zq.detach().clone(), loss=loss.detach().clone(), ppl=ppl.clone(), used=used.clone(),
               ecs=vq.ema_cluster_size.clone(), ema_w=vq.ema_w.clone(), cb=vq.codebook.weight.detach().clone(), count=int(vq.update_count))
    return out


def floats(out, keys=None):
    return {k: v for k, v in out.items() if (k.startswith("g.") or k in U.FLOAT_KEYS) and (keys is None or k in keys)}


def same_bits(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert not a[k].is_floating_point() or bool(torch.isfinite(a[k]).all()), (what, k)
            assert torch.equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k)


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_forward(name):
    """Training mode, no dropout: idx equals both oracles on every frame, z_q is bitwise edtts_sem_encode's, the counts are exact and
    vq_loss is within the bar of fp64."""
    in_dim, S, K, p, B, T = U.CASES[name]
    r64, r32, e_ref, med = U.oracle(name, steps=2)
    enc, vq, names, x, C = make(name)
    dims = enc._dims()
    blob = enc._pack.get(dims, enc._slots())
    xa = native._aligned(x)
    idx0, _, zq0, counts0 = native.sem_encode(dims, blob, xa)
    tape = torch.empty(native.sem_vq_tape_bytes(dims, B, T), dtype=torch.uint8, device=DEV)
    idx, zq, counts, loss = native.sem_vq_encode_train(dims, blob, xa, tape, None, True, U.COMMIT, None)
    assert torch.equal(r64[0]["idx"], r32[0]["idx"])
    assert torch.equal(idx.cpu().reshape(-1), r64[0]["idx"]), int((idx.cpu().reshape(-1) != r64[0]["idx"]).sum())
    assert torch.equal(idx, idx0) and torch.equal(zq, zq0) and torch.equal(counts, counts0)
    assert torch.equal(counts.cpu().long(), torch.bincount(r64[0]["idx"], minlength=K))
    U.check({"loss": loss}, r64[0], e_ref[0], med[0], f"{name} forward")
    _, _, _, loss_eval = native.sem_vq_encode_train(dims, blob, xa, tape, None, False, U.COMMIT, None)
    assert float(loss_eval) == 0.0
    # the module: the same forward, then the EMA update
    zq_m, idx_m, loss_m, ppl, used = call(enc, x)
    assert torch.equal(zq_m.reshape(zq.shape), zq) and torch.equal(idx_m.reshape(idx.shape), idx) and torch.equal(loss_m, loss)
    assert zq_m.grad_fn is not None and loss_m.grad_fn is not None
    assert int(used) == len(torch.unique(r64[0]["idx"]))


@pytest.mark.parametrize("with_zq", [True, False])
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_gradients(name, with_zq):
    """(z_q . C).sum() + w vq_loss, and vq_loss alone (d z_q absent: what train.py's decoder, fed tokens, leaves): every proj gradient,
    codebook.weight.grad and V3's d_z within the bar; rows of unused codes exactly 0.  V2 and V5 under their dropout seed."""
    in_dim, S, K, p, B, T = U.CASES[name]
    gen, seed = (U.DROP_GENS[name][0], U.DROP_SEEDS[name][0]) if name in U.DROP_GENS else (None, None)
    r64, r32, e_ref, med = U.oracle(name, drop_seed=seed, with_zq=with_zq)
    enc, vq, names, x, C = make(name, dropout=gen is not None, gen=gen)
    got = step(enc, vq, names, x, C, with_zq=with_zq, leaf=not in_dim)
    if gen is not None:
        assert enc.last_dropout_seed == seed
    assert torch.equal(r64[0]["idx"], r32[0]["idx"]) and torch.equal(got["idx"].cpu().reshape(-1), r64[0]["idx"])
    grads = {k: v for k, v in floats(got).items() if k.startswith("g.")}
    assert len(grads) == (2 if not in_dim else 7) and all(v is not None for v in grads.values())
    unused = torch.bincount(r64[0]["idx"], minlength=K) == 0
    assert bool(unused.any()) or K <= 5
    assert not bool(got["g.cb"].cpu()[unused].any())
    assert bool(got["g.cb"].cpu()[~unused].any())
    U.check(floats(got), r64[0], e_ref[0], med[0], f"{name} with_zq={with_zq}")


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_ema_update_and_the_next_forward(name):
    """After one training forward the two buffers and the codebook are within the bar of fp64 and update_count is exact; a second
    forward with no optimizer step in between quantises against the NEW codebook."""
    r64, r32, e_ref, med = U.oracle(name, steps=2)
    enc, vq, names, x, C = make(name)
    start = {k: v.detach().clone() for k, v in vq.state_dict().items()}
    a = step(enc, vq, names, x, C, leaf=not U.CASES[name][0])
    assert a["count"] == 1 and vq._count_host == 1
    for k, key in (("ecs", "ema_cluster_size"), ("ema_w", "ema_w"), ("cb", "codebook.weight")):
        assert not torch.equal(a[k], start[key]), k
    U.check(floats(a, U.FLOAT_KEYS), r64[0], e_ref[0], med[0], f"{name} step 1")
    b = step(enc, vq, names, x, C, leaf=not U.CASES[name][0])
    assert b["count"] == 2
    assert torch.equal(r64[1]["idx"], r32[1]["idx"]) and torch.equal(b["idx"].cpu().reshape(-1), r64[1]["idx"])
    assert not torch.equal(r64[1]["idx"], r64[0]["idx"]) or name in ("V1", "V5")  # (there no frame changes its code: z_q below decides)
    e_zq = U.rel_err(b["zq"].reshape(r64[1]["zq"].shape), r64[1]["zq"])
    bar = max(U.rel_err(r32[1]["zq"], r64[1]["zq"]), med[1])
    stale = U.rel_err(a["zq"].reshape(r64[1]["zq"].shape), r64[1]["zq"])
    print(f"{name} step 2 z_q: E {e_zq:.2e}, bar {U.MARGIN * bar:.2e}; the first step's z_q is {stale:.2e} away")
    assert e_zq <= U.MARGIN * bar < stale
    U.check(floats(b), r64[1], e_ref[1], med[1], f"{name} step 2")
    # a loaded update_count is re-read
    sd = vq.state_dict()
    sd["update_count"] = torch.tensor(41)
    vq.load_state_dict(sd)
    step(enc, vq, names, x, C)
    assert int(vq.update_count) == 42 and vq._count_host == 42


@pytest.mark.parametrize("name", U.MULTI)
def test_three_steps_with_a_reset(name):
    """reset_unused_every = 2, an SGD update of every parameter between the steps, the same reset_generator seed on both sides:
    after every step idx is equal and the buffers, the codebook and every gradient are within the bar; the reset rows are bitwise
    the chosen frames of z."""
    in_dim, S, K, p, B, T = U.CASES[name]
    r64, r32, e_ref, med = U.oracle(name, steps=3, reset_unused_every=2, sgd=True)
    enc, vq, names, x, C = make(name, reset_every=2)
    vq.reset_generator = torch.Generator().manual_seed(U.RESET_GEN)
    params = dict(enc.named_parameters())
    for s in range(3):
        with torch.no_grad():
            z = x.reshape(-1, S) if not in_dim else enc._head(x, None, False, False, want_z=True)[1].reshape(-1, S)
        got = step(enc, vq, names, x, C, leaf=not in_dim)
        assert torch.equal(r64[s]["idx"], r32[s]["idx"]) and torch.equal(got["idx"].cpu().reshape(-1), r64[s]["idx"]), s
        assert got["count"] == r64[s]["count"] == s + 1
        U.check(floats(got), r64[s], e_ref[s], med[s], f"{name} step {s + 1}")
        if s == 1:
            rows, dead = r64[s]["rows"], r64[s]["dead"]
            assert r64[s]["reset"] and 0 < len(rows) < K and torch.equal(rows, r32[s]["rows"]) and torch.equal(dead, r32[s]["dead"])
            for k in ("cb", "ema_w"):
                assert torch.equal(got[k][cu(dead)], z[cu(rows)]), k
            assert bool((got["ecs"][cu(dead)] == 1.0).all())
        with torch.no_grad():
            for n in names.values():
                params[n].sub_(U.LR * params[n].grad)


@pytest.mark.parametrize("dropout", [False, True])
def test_ragged_batch(dropout):
    """V2 with lengths [50, 17, 1]: NaN features past the lengths change no bit of any output, gradient or buffer against a run with
    finite garbage there, and everything is within the bar of the oracle on the concatenated valid frames."""
    name, lengths = "V2", U.V2_LENGTHS
    gen, seed = (U.DROP_GENS[name][0], U.DROP_SEEDS[name][0]) if dropout else (None, None)
    n = torch.tensor(lengths, dtype=torch.int64)
    runs = []
    for fill in (float("nan"), 3.5):
        enc, vq, names, x, C = make(name, dropout=dropout, gen=gen)
        xin = x.clone()
        for b, ln in enumerate(lengths):
            xin[b, ln:] = fill
        runs.append(step(enc, vq, names, xin, C, n))
    same_bits(runs[0], runs[1], "NaN against finite garbage past the lengths")
    got = runs[0]
    r64, r32, e_ref, med = U.oracle(name, drop_seed=seed, lengths=lengths)
    sel = r64[0]["sel"]
    assert torch.equal(r64[0]["idx"], r32[0]["idx"]) and torch.equal(got["idx"].cpu().reshape(-1)[sel], r64[0]["idx"])
    for b, ln in enumerate(lengths):
        assert not bool(got["zq"][b, ln:].any()) and not bool(got["idx"][b, ln:].any())
    assert int(got["used"]) == len(torch.unique(r64[0]["idx"]))
    U.check(floats(got), r64[0], e_ref[0], med[0], f"{name} lengths {lengths} dropout {dropout}")


@pytest.mark.parametrize("name", ["V1", "V4"])
def test_two_runs_are_bitwise_equal(name):
    runs = []
    for _ in range(2):
        enc, vq, names, x, C = make(name)
        a = step(enc, vq, names, x, C)
        b = step(enc, vq, names, x, C)
        runs.append((a, b))
    same_bits(runs[0][0], runs[1][0], "first step")
    same_bits(runs[0][1], runs[1][1], "second step")


@pytest.mark.parametrize("name", ["V3", "V4"])
def test_eval_mode_under_grad(name):
    """vq_loss is exactly 0, no buffer changes, and the gradient is the straight-through one."""
    in_dim, S, K, p, B, T = U.CASES[name]
    r64, r32, e_ref, med = U.oracle(name, training=False)
    enc, vq, names, x, C = make(name, train=False)
    start = {k: v.detach().clone() for k, v in vq.state_dict().items()}
    got = step(enc, vq, names, x, C, leaf=not in_dim)
    assert float(got["loss"]) == 0.0 and got["count"] == 0
    for k, v in vq.state_dict().items():
        assert torch.equal(v, start[k]), k
    assert torch.equal(got["idx"].cpu().reshape(-1), r64[0]["idx"])
    if not in_dim:
        assert torch.equal(got["g.d_z"], C.reshape(-1, S))
    assert got["g.cb"] is None or not bool(got["g.cb"].any())
    got["g.cb"] = torch.zeros(K, S) if got["g.cb"] is None else got["g.cb"]
    U.check({k: v for k, v in floats(got).items() if k.startswith("g.")}, r64[0], e_ref[0], med[0], f"{name} eval")


@pytest.mark.parametrize("name", ["V3", "V4"])
def test_no_frames(name):
    """M = 0 through the C ABI: loss 0, counts 0, zero gradients, and an EMA update that only decays -- no division by zero."""
    in_dim, S, K, p, B, T = U.CASES[name]
    enc, vq, names, x, C = make(name)
    dims = enc._dims()
    blob, tblob = enc._pack.get(dims, enc._slots()), enc._tpack.get(dims, enc._slots())
    x0 = torch.empty(0, 7, in_dim or S, device=DEV)
    tape = torch.empty(native.sem_vq_tape_bytes(dims, 0, 7), dtype=torch.uint8, device=DEV)
    idx, zq, counts, loss = native.sem_vq_encode_train(dims, blob, x0, tape, None, True, U.COMMIT, None)
    assert float(loss) == 0.0 and not bool(counts.any()) and idx.shape == (0, 7)
    grads = [torch.full_like(t, float("nan")) for t in enc._slots()]
    native.sem_vq_backward(dims, blob, tblob, tape, x0, idx, None, zq, torch.ones((), device=DEV), U.COMMIT, grads)
    assert all(not bool(g.any()) for g in grads)
    ecs, ema_w, cb = vq.ema_cluster_size.clone(), vq.ema_w.clone(), vq.codebook.weight.detach().clone()
    native.sem_vq_ema_update(dims, idx, x0.new_empty(0, 7, S), None, counts, U.DECAY, U.EPSILON, ecs, ema_w, cb)
    ecs, ema_w, cb = ecs.cpu(), ema_w.cpu(), cb.cpu()  # (IEEE products and quotients: the CPU's are the same)
    assert torch.equal(ecs, vq.ema_cluster_size.cpu() * U.DECAY) and torch.equal(ema_w, vq.ema_w.cpu() * U.DECAY)
    assert bool(torch.isfinite(cb).all()) and torch.equal(cb, ema_w / ecs.clamp_min(U.EPSILON)[:, None])


def test_parameter_written_between_forward_and_backward_raises():
    """The EMA's own write into the codebook does not fire the check; an optimizer-style write does."""
    enc, vq, names, x, C = make("V4")
    zq, idx, loss, _, _ = call(enc, x)
    other = call(enc, 0.5 * x + 0.25)  # a second training forward (its EMA update included) in between changes nothing
    ((zq * C).sum() + loss).backward()
    assert other[0].grad_fn is not None and enc.vq.codebook.weight.grad is not None
    zq, idx, loss, _, _ = call(enc, x)
    with torch.no_grad():
        enc.proj[0].bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified"):
        loss.backward()


def test_head_into_decoder_one_backward():
    """SemanticEncoder(train_vq=True) -> EdgeDiffusionDecoder(autograd=True) through sem_features on train_util case G4:
    loss = mse + 0.1 vq_loss, one backward, every gradient within the bar of the composed oracle."""
    cfg, sd, inp, proj_sd, q_sd, h = U.e2e_case()
    cfg = copy.copy(cfg)
    cfg.use_fsq, cfg.dropout = False, 0.0
    enc = SemanticEncoder(cfg, in_dim=U.E2E_IN_DIM, autograd=True, train_vq=True)
    enc.proj.load_state_dict(proj_sd)
    enc.vq.load_state_dict(q_sd)
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True)
    dec.load_state_dict(sd)
    enc, dec = enc.to(DEV).train(), dec.to(DEV).train()
    x = cu(inp["x"]).requires_grad_(True)
    zq, idx, vq_loss, ppl, used = enc.forward_features(cu(h))
    out = dec(x, cu(inp["t"]), sem_features=zq, step_idx=cu(inp["si"]))
    (((out - cu(inp["target"])) ** 2).mean() + U.E2E_LOSS_W * vq_loss).backward()
    g64, e_ref, med, idx64, idx32, gap, loss64 = U.e2e_oracle()
    assert float(gap.min()) >= U.MIN_GAP and torch.equal(idx64, idx32)
    assert torch.equal(idx.cpu().reshape(-1), idx64), int((idx.cpu().reshape(-1) != idx64).sum())
    print(f"vq_loss {float(vq_loss.detach()):.7f}, fp64 oracle {float(loss64):.7f}")
    got = {k: p.grad for k, p in dec.named_parameters()}
    got["d_x"] = x.grad
    params = dict(enc.named_parameters())
    got.update({"head." + k: params[n].grad for k, n in U.param_names(U.E2E_IN_DIM, False).items()})
    assert len(enc.get_trainable_params()) == 7 and all(p.grad is not None for p in enc.get_trainable_params())
    assert int(enc.vq.update_count) == 1
    TU.check_against_oracle(got, g64, e_ref, med, "VQ head into G4")
