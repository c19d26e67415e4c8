"""bf16 attention on the GPU: EdgeDiffusionDecoder(kernels="generic", attn_dtype="bf16"), with and without matmul_dtype="bf16",
against the fp64 oracle with the bars of tests/train_bf16_util.py (autocast's own error is the yardstick, never the kernels'
output), and the bitwise clauses of the fp32 path: training forward = inference forward, reproducible backward, batch independence,
ragged padding, dropout masks, the optimiser's blob mirror.  It mirrors tests/test_train_bf16_gpu.py clause for clause, on that file's
cases plus A1 / A2 of tests/attn_bf16_util.py.  DESIGN.md section 27.  Run on the GPU box: python -m pytest tests -m gpu."""
import copy

import numpy as np
import pytest
import torch

import attn_bf16_util as AU
import dropout_util as D
import train_bf16_util as U
import train_ragged_util as R
from attn_bf16_util import case
from edge_diffusion_tts_amd import DiffusionSchedule, DPMSolverPP, EdgeDiffusionDecoder, FusedAdamW, native
from train_util import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
MATMULS = ["bf16", "f32"]  # the gradient and forward clauses run with both; everything else with both options on
VARIANT = {"bf16": "both", "f32": "attn"}  # the model whose bars a run is held to
GRAD_CASES = [(n, False) for n in CASES] + [("G4", True), ("A1", False), ("A2", False)]


def cu(t):
    return None if t is None else t.to(DEV)


def make(cfg, sd, autograd=True, matmul_dtype="bf16", attn_dtype="bf16", dropout=None, **kw):
    if dropout is not None:
        cfg = copy.copy(cfg)  # (the case functions cache their cfg)
        cfg.dropout = dropout
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=autograd, matmul_dtype=matmul_dtype, attn_dtype=attn_dtype,
                               train_dropout=dropout is not None, **kw)
    dec.load_state_dict(sd)
    dec = dec.to(DEV)
    if dropout is not None:
        dec.dropout_generator = torch.Generator().manual_seed(U.DROP_GEN)
        return dec.train()
    return dec.eval()


def leaves(inp):
    x = cu(inp["x"]).requires_grad_(True)
    f = None if inp["f"] is None else cu(inp["f"]).requires_grad_(True)
    return x, f


def forward(dec, inp, x=None, f=None, which="", **kw):
    return dec(cu(inp["x"]) if x is None else x, cu(inp["t" + which]), cu(inp["sem"]), cu(inp["si"]), cu(inp["f"]) if f is None else f, **kw)


def loss_of(dec, inp, x, f, which=""):
    return ((forward(dec, inp, x, f, which) - cu(inp["target" + which])) ** 2).mean()


def collect(dec, x, f):
    got = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in dec.named_parameters()}
    got["d_x"] = x.grad.detach().clone()
    if f is not None:
        got["d_sem_features"] = f.grad.detach().clone()
    return got


def assert_same(a, b, what=""):
    assert set(a) == set(b)
    for k in a:
        if a[k] is None:
            assert b[k] is None, k
        else:
            assert torch.equal(a[k], b[k]), f"{what} {k}: {int((a[k] != b[k]).sum())} elements differ"


# ------------------------------------------------------------------------------------------------------------ 1. gradients
@pytest.mark.parametrize("matmul_dtype", MATMULS)
@pytest.mark.parametrize("name, two", GRAD_CASES)
def test_gradients_against_the_fp64_oracle(name, two, matmul_dtype):
    """Per tensor E <= 2 max(E_A, median E_A) and median E <= median E_A, E_A being autocast's error.  Measured: DESIGN.md section 27."""
    cfg, sd, inp = case(name)
    dec = make(cfg, sd, matmul_dtype=matmul_dtype)
    x, f = leaves(inp)
    loss = loss_of(dec, inp, x, f)
    if two:
        loss = loss + loss_of(dec, inp, x, f, "2")
    loss.backward()
    U.check_grads(collect(dec, x, f), AU.grad_yardsticks(name, two, VARIANT[matmul_dtype]),
                  f"{name}{' two forwards' if two else ''} matmul {matmul_dtype}")


# ------------------------------------------------------------------------------------------------------------ 2. forward
@pytest.mark.parametrize("matmul_dtype", MATMULS)
@pytest.mark.parametrize("name", list(CASES) + ["A1", "A2"])
def test_forward(name, matmul_dtype):
    cfg, sd, inp = case(name)
    kw = dict(matmul_dtype=matmul_dtype)
    train, infer, f32 = make(cfg, sd, **kw), make(cfg, sd, autograd=False, **kw), make(cfg, sd, autograd=False, attn_dtype="f32", **kw)
    with torch.no_grad():
        eps = forward(infer, inp)
        U.check_output(eps, AU.forward_yardsticks(name, VARIANT[matmul_dtype]), f"{name} eps matmul {matmul_dtype}")
        assert torch.equal(forward(train, inp), eps)
        assert not torch.equal(forward(f32, inp), eps)  # the option is not a no-op
    a = forward(train, inp)  # the training forward (it keeps a tape): bitwise the inference forward of the same dtypes
    assert a.grad_fn is not None
    assert torch.equal(a.detach(), eps)


# ------------------------------------------------------------------------------------------------------------ 3. sampler
@pytest.mark.parametrize("name", ["G2", "G4"])
def test_dpm_solver_on_the_same_decoder(name):
    cfg, sd, _ = case(name)
    dec = make(cfg, sd)  # the decoder object a trainer validates with
    x_T, f = U.sampler_inputs(name)
    solver = DPMSolverPP(DiffusionSchedule(cfg.diff_steps).to(DEV), order=2)
    out = solver.sample(dec, cu(x_T), cu(f), num_steps=U.SAMPLER_STEPS)
    U.check_output(out, AU.sampler_yardsticks(name, "both"), f"{name} DPM-Solver++ order 2, {U.SAMPLER_STEPS} steps")
    plain = solver.sample(make(cfg, sd, autograd=False, attn_dtype="f32"), cu(x_T), cu(f), num_steps=U.SAMPLER_STEPS)
    assert not torch.equal(out, plain)


# ------------------------------------------------------------------------------------------------------------ 4. determinism
def test_backward_is_reproducible_and_reads_no_workspace():
    cfg, sd, inp = case("G4")
    dec = make(cfg, sd)
    x, f = leaves(inp)
    loss = loss_of(dec, inp, x, f)
    loss.backward(retain_graph=True)
    a = collect(dec, x, f)
    dec.zero_grad(set_to_none=True)
    x.grad = f.grad = None
    loss.backward()  # the same tape again
    assert_same(a, collect(dec, x, f), "second backward")
    dec.zero_grad(set_to_none=True)
    x, f = leaves(inp)
    loss = loss_of(dec, inp, x, f)
    other = dec(cu(inp["target"]), cu(inp["t2"]), None, cu(inp["si"]), cu(inp["f"]) * 0.5)  # overwrites the shared workspace
    assert other.grad_fn is not None
    loss.backward()
    assert_same(a, collect(dec, x, f), "forward in between")


@pytest.mark.parametrize("name", ["G4", "A1"])  # (A1: 200 frames = three full 64-query blocks and one of 8 per utterance)
def test_eps_rows_do_not_depend_on_the_batch(name):
    cfg, sd, inp = case(name)
    dec = make(cfg, sd, autograd=False)
    with torch.no_grad():
        eps = forward(dec, inp)
        solo = dec(cu(inp["x"][:1]), cu(inp["t"][:1]), None, cu(inp["si"][:1]), cu(inp["f"][:1]))
    assert torch.equal(solo[0], eps[0])


# ------------------------------------------------------------------------------------------------------------ 5. ragged
def garbage(inp, t_len, s_len, nan=True):
    out = dict(inp)
    fill = float("nan") if nan else 0.0
    out["x"] = inp["x"].masked_fill(~R.frame_mask(t_len, inp["x"].shape[1]), fill)
    out["f"] = inp["f"].masked_fill(~R.frame_mask(s_len, inp["f"].shape[1]), fill)
    return out


def test_ragged_gradients_against_the_ragged_fp64_oracle():
    cfg, sd, inp, t_len, s_len = R.case(U.RAGGED_CASE)
    g = garbage(inp, t_len, s_len)
    dec = make(cfg, sd, train_lengths=True)
    x, f = leaves(g)
    eps = forward(dec, g, x, f, x_lengths=t_len, sem_lengths=s_len)
    R.masked_loss(eps, cu(inp["target"]), cu(t_len)).backward()
    got = collect(dec, x, f)
    U.check_grads(got, AU.ragged_yardsticks("both"), U.RAGGED_CASE)
    T, S = x.shape[1], f.shape[1]
    assert float(got["d_x"].masked_select(~R.frame_mask(cu(t_len), T)).abs().sum()) == 0.0
    assert float(got["d_sem_features"].masked_select(~R.frame_mask(cu(s_len), S)).abs().sum()) == 0.0
    assert float(eps.detach().masked_select(~R.frame_mask(cu(t_len), T)).abs().sum()) == 0.0


def test_ragged_input_gradients_are_the_solo_calls():
    cfg, sd, inp, t_len, s_len = R.case(U.RAGGED_CASE)
    g = garbage(inp, t_len, s_len)
    dec = make(cfg, sd, train_lengths=True)
    x, f = leaves(g)
    eps = forward(dec, g, x, f, x_lengths=t_len, sem_lengths=s_len)
    d_eps = cu(torch.randn(eps.shape, generator=torch.Generator().manual_seed(9)))
    eps.backward(d_eps.masked_fill(~R.frame_mask(cu(t_len), eps.shape[1]), float("nan")))
    solo = make(cfg, sd)
    for b in range(len(t_len)):
        Tb, Sb = int(t_len[b]), int(s_len[b])
        xb = cu(inp["x"][b:b + 1, :Tb]).requires_grad_(True)
        fb = cu(inp["f"][b:b + 1, :Sb]).requires_grad_(True)
        e = solo(xb, cu(inp["t"][b:b + 1]), None, cu(inp["si"][b:b + 1]), fb)
        assert torch.equal(e.detach()[0], eps.detach()[b, :Tb])
        e.backward(d_eps[b:b + 1, :Tb])
        assert torch.equal(x.grad[b, :Tb], xb.grad[0]), b
        assert torch.equal(f.grad[b, :Sb], fb.grad[0]), b
        assert float(xb.grad.abs().max()) > 0 and float(fb.grad.abs().max()) > 0


def test_ragged_padding_is_never_read():
    """native level.  Run A: zeros in all padding, tape and scratch zero-filled.  Run B: NaN in the padding of x, sem_features and
    d_eps, tape and scratch pre-filled with 0xFF bytes.  Every output bit is the same."""
    cfg, sd, inp, t_len, s_len = R.case(U.RAGGED_CASE)
    dec = make(cfg, sd, train_lengths=True)
    dims, packed = dec.dims(), dec._ensure_packed()
    B, T, _ = inp["x"].shape
    S = inp["f"].shape[1]
    names, params = dec._named_params()
    tl, sl = cu(t_len), cu(s_len)
    d_eps0 = 2.0 * torch.randn(B, T, cfg.n_mels, generator=torch.Generator().manual_seed(3))
    outs = []
    for nan in (False, True):
        g = garbage(inp, t_len, s_len, nan)
        fill = 0xFF if nan else 0
        ws = dec.workspace(B, T, S, B, DEV)
        tape = torch.full((native.train_tape_bytes(dims, B, T, S),), fill, dtype=torch.uint8, device=DEV)
        scratch = torch.full((native.train_scratch_bytes(dims, B, T, S),), fill, dtype=torch.uint8, device=DEV)
        x, f = cu(g["x"]), cu(g["f"])
        eps = native.decoder_forward_train(dims, packed, ws, tape, x, cu(inp["t"]), cu(inp["si"]), None, f, S, None, tl, sl)
        d_eps = cu(d_eps0.masked_fill(~R.frame_mask(t_len, T), float("nan") if nan else 0.0))
        out = {n: torch.full_like(p, float("nan")) for n, p in zip(names, params) if dec._enters_output(n, True, inp["si"] is not None)}
        slots = [out.get(dec._slot_param(n)) for n in native.slot_names(cfg.layers)]
        d_x, d_f = torch.full_like(x, float("nan")), torch.full_like(f, float("nan"))
        native.decoder_backward(dims, packed, ws, tape, x, cu(inp["t"]), cu(inp["si"]), None, f, S, d_eps, slots, d_x, d_f, None, tl, sl,
                                scratch=scratch)
        assert native.index_errors(ws) == 0
        out.update(eps=eps, d_x=d_x, d_sem_features=d_f)
        outs.append(out)
    assert_same(outs[0], outs[1], U.RAGGED_CASE)
    for k, v in outs[1].items():
        assert bool(torch.isfinite(v).all()), k
        assert float(v.abs().max()) > 0, k


# ------------------------------------------------------------------------------------------------------------ 6. dropout
def test_dropout_masks_and_gradients_against_the_masked_oracle():
    name, p = U.DROP_CASE, U.DROP_P
    cfg, sd, inp = case(name)
    _, B, T, S, _, _ = CASES[name]
    dec = make(cfg, sd, dropout=p)
    x, f = leaves(inp)
    eps = forward(dec, inp, x, f)
    seed = dec.last_dropout_seed
    assert (seed,) == U.drop_seeds()
    ((eps - cu(inp["target"])) ** 2).mean().backward()
    U.check_grads(collect(dec, x, f), AU.dropout_yardsticks("both"), f"{name} p={p}")
    with torch.no_grad():
        assert not torch.equal(forward(dec.eval(), inp), eps.detach())  # the masks act
    # the masks are the library's Philox contract, whatever the attn_dtype and matmul_dtype
    d16, d32 = dec.dims(), make(cfg, sd, matmul_dtype="f32", attn_dtype="f32").dims()
    assert d16.compute_dtype == d32.compute_dtype | native.EDTTS_MATMUL_BF16 | native.EDTTS_ATTN_BF16
    for layer in range(cfg.layers):
        for site in range(4):
            got = native.dropout_mask(d16, site, layer, B, T, S, p, seed, DEV)
            assert torch.equal(got, native.dropout_mask(d32, site, layer, B, T, S, p, seed, DEV))
            if site in (D.SITE_ATTN, D.SITE_CROSS):
                want = D.attn_keep(seed, p, layer, site, B, cfg.heads, T, T if site == D.SITE_ATTN else S)
            else:
                want = D.row_keep(seed, p, layer, site, B * T, cfg.ffn_mult * cfg.hidden if site == D.SITE_ACT else cfg.hidden)
            assert np.array_equal(got.cpu().numpy(), want.astype(np.uint8)), (layer, site)


# ------------------------------------------------------------------------------------------------------------ 7. optimiser
def test_fused_adamw_mirrors_into_the_same_blob():
    cfg, sd, inp = case("G4")
    dec = make(cfg, sd)
    opt = FusedAdamW(dec.parameters(), lr=2e-3, weight_decay=0.01, max_norm=0.5)
    assert opt.attach_decoder(dec) is True
    x, f = leaves(inp)
    loss_of(dec, inp, x, f).backward()
    before = {k: p.detach().clone() for k, p in dec.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    assert sum(not torch.equal(p.detach(), before[k]) for k, p in dec.named_parameters()) > 10
    names, tensors = dec._slot_tensors()
    fresh = torch.full((native.packed_bytes(dec.dims()),), 0xA5, dtype=torch.uint8, device=DEV)
    native.pack_weights(dec.dims(), [t.contiguous() for t in tensors], fresh)
    assert torch.equal(dec._packed, fresh)  # the blob is current: byte for byte a pack of the stepped parameters
    twin = make(cfg, dec.state_dict(), autograd=False)
    with torch.no_grad():
        assert torch.equal(forward(dec, inp, which="2"), forward(twin, inp, which="2"))
