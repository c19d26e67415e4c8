"""Training the semantic head on the GPU: SemanticEncoder / FSQEncoder with autograd=True against the CPU
oracle of tests/sem_train_util.py.  The bar is the project's: every gradient within MARGIN x max(E_ref, median E_ref) of the fp64
oracle, E_ref being the fp32 oracle's own error; idx must equal the oracles' on EVERY frame (the cases are chosen so that no FSQ
decision is close: tests/test_sem_train_host.py).  Run on the GPU box: python -m pytest tests -m gpu.

Every test prints the ratios it asserts on; DESIGN.md section 21 is where the worst one per case is recorded."""
import copy

import numpy as np
import pytest
import torch

import dropout_util as D
import sem_train_util as U
import train_util as TU
from conftest import max_abs
from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, native, synth_state_dict
from edge_diffusion_tts_amd.encoder import FSQEncoder, SemanticEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL = 1e-4  # DESIGN.md section 20's bar for a dropped forward against the masked fp32 oracle


def cu(t):
    return None if t is None else t.to(DEV)


def make(name, train_dropout=None, gen=None, train=True, p=None):
    """(module, canonical name -> parameter name, features on the device, C on the device) of a case"""
    in_dim, S, levels, cp, B, T, proj_sd, q_sd, x, C = U.case(name)
    if in_dim == 0:
        enc = FSQEncoder(S, levels, autograd=True)
        enc.load_state_dict(q_sd)
        names = U.param_names(0, False, "")
    else:
        layout = cp is not None
        cfg = CFG(device=DEV, use_fsq=True, fsq_levels=list(levels), semantic_dim=S, dropout=(cp if p is None else p) if layout else 0.0)
        enc = SemanticEncoder(cfg, in_dim=in_dim, proj_dropout=layout, autograd=True, train_dropout=layout if train_dropout is None else train_dropout)
        enc.proj.load_state_dict(proj_sd)
        enc.vq.load_state_dict(q_sd)
        names = U.param_names(in_dim, layout)
        if gen is not None:
            enc.dropout_generator = torch.Generator().manual_seed(gen)
    enc = enc.to(DEV)
    enc.train(train)
    return enc, names, cu(x), cu(C)


def call(enc, x, lengths=None):
    """(z_q, idx) of a differentiable call"""
    if isinstance(enc, FSQEncoder):
        out = enc(x)
    else:
        out = enc.quantize_features(x, lengths)
    return out[0], out[1]


def step(enc, names, x, C, lengths=None, leaf=False):
    """forward, (z_q . C).sum(), backward: ({canonical name: gradient}, z_q, idx)"""
    enc.zero_grad(set_to_none=True)
    xin = x.clone().requires_grad_(True) if leaf else x
    zq, idx = call(enc, xin, lengths)
    assert zq.grad_fn is not None and not idx.requires_grad
    (zq * C).sum().backward()
    params = dict(enc.named_parameters())
    got = {k: (None if params[n].grad is None else params[n].grad.detach().clone()) for k, n in names.items()}
    if leaf:
        got["d_z"] = xin.grad.detach().clone()
    return got, zq.detach(), idx


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_gradients_against_the_oracle(name):
    """.eval(): no dropout in any case.  Six proj tensors and four quantizer tensors (H4: the four and d_z)."""
    enc, names, x, C = make(name, train=False)
    got, zq, idx = step(enc, names, x, C, leaf=name == "H4")
    g64, e_ref, med, zq32, idx64, idx32, margin = U.oracle_pair(name)
    assert float(margin.min()) >= U.MIN_MARGIN and torch.equal(idx64, idx32)
    assert torch.equal(idx.cpu(), idx64), int((idx.cpu() != idx64).sum())
    assert max_abs(zq.cpu(), zq32) < FWD_TOL
    assert all(v is not None for v in got.values()) and len(got) == (5 if name == "H4" else 10)
    if name != "H4":  # the features get no gradient (the reference detaches them), HuBERT none
        h = x.clone().requires_grad_(True)
        call(enc, h)[0].sum().backward()
        assert h.grad is None
    U.check_against_oracle(got, g64, e_ref, med, name)


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_training_forward_is_bitwise_the_inference_forward_without_dropout(name):
    in_dim, S, levels, p, B, T, proj_sd, q_sd, x, C = U.case(name)
    enc, names, x, C = make(name, train=False)
    with torch.no_grad():
        zq0, idx0 = call(enc, x)
        assert zq0.grad_fn is None
    ref_grads = None
    # .eval(); then training mode with proj[3].p = 0 (Dropout layout) or without a Dropout (the four-module proj, FSQEncoder)
    variants = [("eval", False, None), ("p = 0", True, 0.0) if p is not None else ("train", True, None)]
    for what, train, pp in variants:
        e2, names2, _, _ = make(name, train=train, p=pp)
        got, zq, idx = step(e2, names2, x, C)
        assert torch.equal(zq, zq0) and torch.equal(idx, idx0), what
        if ref_grads is None:
            ref_grads = got
        for k in got:
            assert torch.equal(got[k], ref_grads[k]), (what, k)
    # EdttsDropout{p = 0} through the C ABI: the undropped launches
    dims = enc._dims()
    slots = [t.detach() for t in enc._slots()]
    blob, tblob = enc._pack.get(dims, enc._slots()), enc._tpack.get(dims, enc._slots())
    xa = native._aligned(x)
    Bx, Tx = xa.shape[0], xa.shape[1]
    outs = []
    for drop in (None, (0.0, 99)):
        tape = torch.empty(native.sem_train_tape_bytes(dims, Bx, Tx), dtype=torch.uint8, device=DEV)
        idx, zq, counts = native.sem_encode_train(dims, blob, xa, tape, None, True, drop)
        grads = [torch.empty_like(t) for t in slots]
        native.sem_backward(dims, blob, tblob, tape, xa, None, C.reshape(Bx, Tx, -1).contiguous(), grads, None, drop)
        outs.append((idx, zq, counts, grads))
    assert torch.equal(outs[0][0].reshape(idx0.shape), idx0) and torch.equal(outs[0][1].reshape(zq0.shape), zq0)
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)
    for a, b in zip(outs[0][3], outs[1][3]):
        assert torch.equal(a, b)
    for i, k in enumerate(U.KEYS if in_dim else U.KEYS[6:]):  # slot order
        assert torch.equal(outs[0][3][i], ref_grads[k]), k


@pytest.mark.parametrize("name", ["H2", "H3"])
def test_mask_kernel_equals_the_numpy_restatement(name):
    in_dim, S, levels, p, B, T = U.CASES[name]
    dims = native.sem_dims(in_dim, S, levels)
    for seed in U.DROP_SEEDS[name]:
        got = native.sem_dropout_mask(dims, B, T, p, seed, DEV).cpu().numpy()
        want = U.head_keep(seed, p, B * T, S)
        assert got.shape == want.shape and got.dtype == np.uint8
        assert np.array_equal(got, want.astype(np.uint8)), (name, seed, int((got != want).sum()))
        assert 0 < got.mean() < 1
    assert bool(native.sem_dropout_mask(dims, B, T, 0.0, 7, DEV).all())  # p = 0 keeps everything


@pytest.mark.parametrize("name,which", [("H2", 0), ("H2", 1), ("H3", 0), ("H3", 1)])
def test_dropout_forward_and_gradients_against_the_masked_oracle(name, which):
    gen, seed = U.DROP_GENS[name][which], U.DROP_SEEDS[name][which]
    enc, names, x, C = make(name, gen=gen)
    got, zq, idx = step(enc, names, x, C)
    assert enc.last_dropout_seed == seed
    g64, e_ref, med, zq32, idx64, idx32, margin = U.oracle_pair(name, seed)
    assert float(margin.min()) >= U.MIN_MARGIN and torch.equal(idx64, idx32)
    assert torch.equal(idx.cpu(), idx64), int((idx.cpu() != idx64).sum())
    err = max_abs(zq.cpu(), zq32)
    with torch.no_grad():
        zq_eval = call(enc.eval(), x)[0]
    moved = float(((zq - zq_eval).abs().amax(-1) > 0).float().mean())
    print(f"{name} gen {gen}: z_q vs the masked fp32 oracle {err:.2e}; frames whose z_q differs from the eval forward: {moved:.2f}")
    assert err < FWD_TOL, err
    assert moved > 0.5, moved
    U.check_against_oracle(got, g64, e_ref, med, f"{name} p={U.CASES[name][3]} gen {gen}")


def test_dropout_needs_the_option_and_follows_the_generator():
    enc, names, x, C = make("H2", train_dropout=False)
    with pytest.raises(ValueError, match=r"train_dropout=True.*\.eval\(\)"):
        call(enc, x)
    with torch.no_grad():  # not differentiable: the inference forward, no dropout, no seed
        call(enc, x)
    assert enc.last_dropout_seed is None
    a, _, _, _ = make("H2", gen=5)
    b, _, _, _ = make("H2", gen=5)
    ga, za, _ = step(a, names, x, C)
    gb, zb, _ = step(b, names, x, C)
    assert a.last_dropout_seed == b.last_dropout_seed == D.seeds_of(5)[0] and torch.equal(za, zb)
    _, zc, _ = step(a, names, x, C)  # the next draw
    assert a.last_dropout_seed == D.seeds_of(5, 2)[1] and not torch.equal(za, zc)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def test_backward_is_deterministic_and_owns_its_tape():
    """H5 (three uneven dW slabs): two backwards are bitwise equal; a second training forward between a forward and its backward
    changes nothing; a parameter written between them raises."""
    enc, names, x, C = make("H5")
    a, _, _ = step(enc, names, x, C)
    b, _, _ = step(enc, names, x, C)
    enc.zero_grad(set_to_none=True)
    zq, _ = call(enc, x)
    other, _ = call(enc, 0.5 * x + 0.25)
    assert other.grad_fn is not None
    (zq * C).sum().backward()
    params = dict(enc.named_parameters())
    for k, n in names.items():
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], params[n].grad), k
    zq, _ = call(enc, x)
    with torch.no_grad():
        enc.proj[0].bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified"):
        zq.sum().backward()


@pytest.mark.parametrize("dropout", [False, True])
def test_ragged_batch(dropout):
    """H2 with lengths [50, 17, 1]: the gradients of the three trimmed utterances concatenated; z_q 0 past the lengths; row 1 bitwise
    its solo run."""
    name, lengths = "H2", U.H2_LENGTHS
    gen, seed = (U.DROP_GENS[name][0], U.DROP_SEEDS[name][0]) if dropout else (None, None)
    enc, names, x, C = make(name, gen=gen, train=dropout)
    n = torch.tensor(lengths, dtype=torch.int64)
    xin = x.clone()
    for b, ln in enumerate(lengths):
        xin[b, ln:] = float("nan")  # frames past the lengths are not read
    got, zq, idx = step(enc, names, xin, C, n)
    g64, e_ref, med, zq32, idx64, idx32, margin = U.oracle_pair(name, seed, lengths)
    assert float(margin.min()) >= U.MIN_MARGIN and torch.equal(idx64, idx32)
    sel = torch.cat([torch.arange(ln) + b * x.shape[1] for b, ln in enumerate(lengths)])
    assert torch.equal(idx.cpu().reshape(-1)[sel], idx64.reshape(-1))
    for b, ln in enumerate(lengths):
        assert not bool(zq[b, ln:].any()) and not bool(idx[b, ln:].any())
    assert max_abs(zq.cpu().reshape(-1, zq.shape[-1])[sel], zq32[0]) < FWD_TOL
    U.check_against_oracle(got, g64, e_ref, med, f"{name} lengths {lengths} dropout {dropout}")
    if not dropout:  # (with dropout the mask is keyed by the batch row: a solo run draws row 0's)
        with torch.no_grad():
            solo = call(enc, x[1:2, :lengths[1]])[0]
        assert torch.equal(zq[1, :lengths[1]], solo[0])


def _e2e_modules(dropout):
    cfg, sd, inp, proj_sd, q_sd, h = U.e2e_case()
    cfg = copy.copy(cfg)
    cfg.dropout = U.E2E_P if dropout else 0.0
    enc = SemanticEncoder(cfg, in_dim=U.E2E_IN_DIM, proj_dropout=True, autograd=True, train_dropout=dropout)
    enc.proj.load_state_dict(proj_sd)
    enc.vq.load_state_dict(q_sd)
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, train_dropout=dropout)
    dec.load_state_dict(sd)
    enc, dec = enc.to(DEV).train(), dec.to(DEV).train()
    if dropout:
        enc.dropout_generator = torch.Generator().manual_seed(U.E2E_GENS[0])
        dec.dropout_generator = torch.Generator().manual_seed(U.E2E_GENS[1])
    return cfg, inp, enc, dec, cu(h)


@pytest.mark.parametrize("dropout", [False, True])
def test_head_into_decoder_one_backward(dropout):
    """SemanticEncoder(autograd=True) -> EdgeDiffusionDecoder(autograd=True) through sem_features: one loss.backward() trains both, as
    train_v2.train_step does.  Against the composed oracle (with both train_dropout: the composed masked oracle)."""
    cfg, inp, enc, dec, h = _e2e_modules(dropout)
    x = cu(inp["x"]).requires_grad_(True)
    zq, idx, vq_loss, ppl, used = enc.forward_features(h)
    assert float(vq_loss) == 0.0 and zq.grad_fn is not None
    out = dec(x, cu(inp["t"]), sem_features=zq, step_idx=cu(inp["si"]))
    ((out - cu(inp["target"])) ** 2).mean().backward()
    if dropout:
        assert enc.last_dropout_seed == D.seeds_of(U.E2E_GENS[0])[0] and dec.last_dropout_seed == D.seeds_of(U.E2E_GENS[1])[0]
    g64, e_ref, med, idx64, idx32, margin = U.e2e_oracle(dropout)
    assert float(margin.min()) >= U.MIN_MARGIN and torch.equal(idx64, idx32)
    assert torch.equal(idx.cpu(), idx64), int((idx.cpu() != idx64).sum())
    got = {k: p.grad for k, p in dec.named_parameters()}
    got["d_x"] = x.grad
    params = dict(enc.named_parameters())
    got.update({"head." + k: params[n].grad for k, n in U.param_names(U.E2E_IN_DIM, True).items()})
    assert len(enc.get_trainable_params()) == 10 and all(p.grad is not None for p in enc.get_trainable_params())
    TU.check_against_oracle(got, g64, e_ref, med, f"head into G4, dropout {dropout}")


def test_golden_head_into_reference_decoder(golden):
    """The reference's own FSQEncoder behind a proj written as train_v2.py:54-60 (its Dropout replaced by the contract's mask),
    feeding the reference's decoder under the v-prediction objective (tests/golden/make_golden_train_head.py): the fixture's fp64
    gradients are the arbiter, its fp32 gradients the yardstick."""
    g = golden("train_head")
    hidden, heads, layers, sem_dim, in_dim = (int(v) for v in g["cfg"])
    levels = [int(v) for v in g["levels"]]
    p = float(g["p"])
    cfg = CFG(device=DEV, hidden=hidden, heads=heads, layers=layers, dropout=p, semantic_dim=sem_dim, use_fsq=True, fsq_levels=levels)
    enc = SemanticEncoder(cfg, in_dim=in_dim, proj_dropout=True, autograd=True, train_dropout=True)
    enc.proj.load_state_dict({k[len("w.proj."):]: g[k] for k in g if k.startswith("w.proj.")})
    enc.vq.load_state_dict({k[len("w.fsq."):]: g[k] for k in g if k.startswith("w.fsq.")})
    enc = enc.to(DEV).train()
    enc.dropout_generator = torch.Generator().manual_seed(int(g["gen"]))
    dcfg = copy.copy(cfg)
    dcfg.dropout = 0.0
    dec = EdgeDiffusionDecoder(dcfg, kernels="generic", autograd=True)
    dec.load_state_dict(synth_state_dict(dcfg, 7))
    dec = dec.to(DEV).train()
    sch = DiffusionSchedule(cfg.diff_steps).to(DEV)
    x0, noise, t, h = cu(g["x0"]), cu(g["noise"]), cu(g["t"]), cu(g["h"])
    x_t, _ = sch.q_sample(x0, t, noise)
    zq, idx, _, _, _ = enc.forward_features(h)
    assert enc.last_dropout_seed == int(g["seed"])
    assert torch.equal(idx.cpu(), g["idx"])
    v_pred = dec(x_t, t, sem_features=zq, step_idx=torch.zeros(len(t), dtype=torch.long, device=DEV))
    loss = torch.nn.functional.mse_loss(v_pred, sch.get_v_target(x0, noise, t))
    loss.backward()
    names = sorted(k[4:] for k in g if k.startswith("g64."))
    got = {"decoder." + k: v.grad for k, v in dec.named_parameters()}
    got.update({"encoder.proj." + k: v.grad for k, v in enc.proj.named_parameters()})
    got.update({"encoder.fsq." + k: v.grad for k, v in enc.vq.named_parameters()})
    assert sorted(k for k, v in got.items() if v is not None) == names
    e_ref = {k: TU.rel_err(g["g32." + k], g["g64." + k]) for k in names}
    med = float(torch.tensor(sorted(e_ref.values())).median())
    TU.check_against_oracle({k: got[k] for k in names}, {k: g["g64." + k] for k in names}, e_ref, med, "golden head")
