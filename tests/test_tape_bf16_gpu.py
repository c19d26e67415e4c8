"""bf16 activation storage on the GPU: EdgeDiffusionDecoder(kernels="generic", matmul_dtype="bf16", attn_dtype="bf16",
tape_dtype="bf16") against the same decoder with tape_dtype="f32", built from the same state dict.  Every comparison is torch.equal:
the four narrowed buffers are read only by loaders that round to bf16, and rounding is idempotent (the argument
is restated on the CPU in tests/test_tape_bf16_host.py).  The accuracy bars of sections 26 / 27 therefore carry over unrestated.
Run on the GPU box: python -m pytest tests -m gpu."""
import copy

import pytest
import torch

import attn_bf16_util as AU
import tape_bf16_util as TU
import train_bf16_util as U
import train_ragged_util as R
from attn_bf16_util import case
from edge_diffusion_tts_amd import DiffusionSchedule, DPMSolverPP, EdgeDiffusionDecoder, FusedAdamW, native

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAPES = ("bf16", "f32")


def cu(t):
    return None if t is None else t.to(DEV)


def make(cfg, sd, tape_dtype, autograd=True, dropout=None, **kw):
    if dropout is not None:
        cfg = copy.copy(cfg)  # (the case functions cache their cfg)
        cfg.dropout = dropout
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=autograd, matmul_dtype="bf16", attn_dtype="bf16", tape_dtype=tape_dtype,
                               train_dropout=dropout is not None, **kw)
    dec.load_state_dict(sd)
    dec = dec.to(DEV)
    if dropout is not None:
        dec.dropout_generator = torch.Generator().manual_seed(U.DROP_GEN)
        return dec.train()
    return dec.eval()


def pair(cfg, sd, **kw):
    """(the decoder with bf16 storage, its fp32-storage twin)."""
    on, off = (make(cfg, sd, t, **kw) for t in TAPES)
    assert on.dims().compute_dtype == off.dims().compute_dtype | native.EDTTS_TAPE_BF16
    return on, off


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
    live = 0
    for k in a:
        if a[k] is None:
            assert b[k] is None, k
        else:
            assert torch.equal(a[k], b[k]), f"{what} {k}: {int((a[k] != b[k]).sum())} elements differ"
            live += 1
    assert live > 10, what


def grads(dec, inp, two=False):
    x, f = leaves(inp)
    loss = loss_of(dec, inp, x, f)
    if two:
        loss = loss + loss_of(dec, inp, x, f, "2")
    loss.backward()
    got = collect(dec, x, f)
    got["loss"] = loss.detach().clone()
    return got


# ------------------------------------------------------------------------------------------------------------ 1. eps
@pytest.mark.parametrize("name", TU.NAMES)
def test_eps_of_both_forwards_is_bitwise_the_fp32_tapes(name):
    cfg, sd, inp = case(name)
    on, off = pair(cfg, sd)
    infer_on, infer_off = pair(cfg, sd, autograd=False)
    with torch.no_grad():
        eps = forward(infer_off, inp)
        assert torch.equal(forward(infer_on, inp), eps)  # the inference forward: the workspace's buffers at half width
    a, b = forward(on, inp), forward(off, inp)  # the training forward: the tape's
    assert a.grad_fn is not None and b.grad_fn is not None
    assert torch.equal(a.detach(), b.detach()) and torch.equal(a.detach(), eps)
    assert bool(torch.isfinite(eps).all()) and float(eps.abs().max()) > 0


@pytest.mark.parametrize("name", TU.NAMES)
def test_dpm_solver_sample_is_bitwise_the_fp32_tapes(name):
    """DPMSolverPP.sample takes semantic features; the cases that feed token ids (G1, G5, A2) get features drawn here for it."""
    cfg, sd, inp = case(name)
    B, T, S = AU.shape(name)
    x_T = inp["x"]
    f = inp["f"] if inp["f"] is not None else torch.randn(B, S, cfg.semantic_dim, generator=torch.Generator().manual_seed(B * 1000 + S))
    solver = DPMSolverPP(DiffusionSchedule(cfg.diff_steps).to(DEV), order=2)
    outs = [solver.sample(d, cu(x_T), cu(f), num_steps=U.SAMPLER_STEPS) for d in pair(cfg, sd)]
    assert torch.equal(outs[0], outs[1])
    assert bool(torch.isfinite(outs[0]).all()) and not torch.equal(outs[0], cu(x_T))


# ------------------------------------------------------------------------------------------------------------ 2. gradients
@pytest.mark.parametrize("name, two", [(n, False) for n in TU.NAMES] + [("G4", True)])
def test_every_gradient_is_bitwise_the_fp32_tapes(name, two):
    cfg, sd, inp = case(name)
    on, off = pair(cfg, sd)
    a, b = grads(on, inp, two), grads(off, inp, two)
    assert_same(a, b, f"{name}{' two forwards' if two else ''}")
    assert float(a["d_x"].abs().max()) > 0 and all(bool(torch.isfinite(v).all()) for v in a.values() if v is not None)


def test_two_backwards_of_one_tape_are_bitwise_equal():
    cfg, sd, inp = case("G4")
    dec = make(cfg, sd, "bf16")
    x, f = leaves(inp)
    loss = loss_of(dec, inp, x, f)
    loss.backward(retain_graph=True)
    a = collect(dec, x, f)
    dec.zero_grad(set_to_none=True)
    x.grad = f.grad = None
    other = dec(cu(inp["target"]), cu(inp["t2"]), None, cu(inp["si"]), cu(inp["f"]) * 0.5)  # overwrites the shared workspace, not the tape
    assert other.grad_fn is not None
    loss.backward()  # the same tape again
    assert_same(a, collect(dec, x, f), "second backward")


# ------------------------------------------------------------------------------------------------------------ 3. ragged
def garbage(inp, t_len, s_len, nan=True):
    out = dict(inp)
    fill = float("nan") if nan else 0.0
    out["x"] = inp["x"].masked_fill(~R.frame_mask(t_len, inp["x"].shape[1]), fill)
    out["f"] = inp["f"].masked_fill(~R.frame_mask(s_len, inp["f"].shape[1]), fill)
    return out


def ragged_run(dec, cfg, inp, t_len, s_len, nan):
    """native level, as tests/test_attn_bf16_gpu.py: NaN (or zeros) in all padding of x, sem_features and d_eps; tape and scratch
    pre-filled with 0xFF bytes (0xFFFF is a bf16 NaN, 0xFFFFFFFF an fp32 one) or zeros."""
    dims, packed = dec.dims(), dec._ensure_packed()
    B, T, _ = inp["x"].shape
    S = inp["f"].shape[1]
    names, params = dec._named_params()
    tl, sl = cu(t_len), cu(s_len)
    d_eps0 = 2.0 * torch.randn(B, T, cfg.n_mels, generator=torch.Generator().manual_seed(3))
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
    return out


def test_ragged_with_nan_padding_and_a_0xff_tape_is_bitwise_the_fp32_tapes():
    cfg, sd, inp, t_len, s_len = R.case(U.RAGGED_CASE)
    on, off = pair(cfg, sd, train_lengths=True)
    want = ragged_run(off, cfg, inp, t_len, s_len, nan=True)
    got = ragged_run(on, cfg, inp, t_len, s_len, nan=True)
    clean = ragged_run(on, cfg, inp, t_len, s_len, nan=False)  # zeros everywhere instead: nothing past the counts is ever loaded
    assert_same(got, want, U.RAGGED_CASE)
    assert_same(got, clean, U.RAGGED_CASE + " 0xFF tape against a zeroed one")
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
        assert float(v.abs().max()) > 0, k


# ------------------------------------------------------------------------------------------------------------ 4. dropout
def test_dropout_gradients_and_masks_are_bitwise_the_fp32_tapes():
    name, p = U.DROP_CASE, U.DROP_P
    cfg, sd, inp = case(name)
    B, T, S = AU.shape(name)
    on, off = pair(cfg, sd, dropout=p)
    runs = []
    for dec in (on, off):
        x, f = leaves(inp)
        eps = forward(dec, inp, x, f)
        assert (dec.last_dropout_seed,) == U.drop_seeds()
        ((eps - cu(inp["target"])) ** 2).mean().backward()
        got = collect(dec, x, f)
        got["eps"] = eps.detach().clone()
        runs.append(got)
    assert_same(runs[0], runs[1], f"{name} p={p}")
    with torch.no_grad():
        assert not torch.equal(forward(on.eval(), inp), runs[0]["eps"])  # the masks act
    seed = on.last_dropout_seed
    for layer in range(cfg.layers):
        for site in range(4):
            a = native.dropout_mask(on.dims(), site, layer, B, T, S, p, seed, DEV)
            assert torch.equal(a, native.dropout_mask(off.dims(), site, layer, B, T, S, p, seed, DEV)), (layer, site)
            assert 0 < int(a.sum()) < a.numel()


# ------------------------------------------------------------------------------------------------------------ 5. the tape itself
@pytest.mark.parametrize("name", ["G2", "A1"])  # G2: hidden 50, 2-byte stores on odd rows; A1: hidden 64, 8-byte stores throughout
def test_narrowed_regions_hold_the_rounded_fp32_regions(name):
    """Isolates the store epilogues from the loaders: after one training forward each narrowed region of the bf16 tape is, bit for
    bit, the fp32 tape's region rounded to bf16, and every other region is that tape's region unchanged."""
    cfg, sd, inp = case(name)
    B, T, S = AU.shape(name)
    tapes = {}
    for dec in pair(cfg, sd):
        dims, packed = dec.dims(), dec._ensure_packed()
        ws = dec.workspace(B, T, S, B, DEV)
        tape = torch.full((native.train_tape_bytes(dims, B, T, S),), 0xFF, dtype=torch.uint8, device=DEV)
        sem = None if inp["f"] is not None else cu(inp["sem"])
        native.decoder_forward_train(dims, packed, ws, tape, cu(inp["x"]), cu(inp["t"]), cu(inp["si"]), sem, cu(inp["f"]), S, None, None, None)
        torch.cuda.synchronize()
        tapes[dec.tape_dtype] = (tape, dims)
    for layer in range(cfg.layers):
        for which in native.TAPE_REGIONS:
            a = TU.tape_region(*tapes["bf16"], cfg, B, T, S, layer, which)
            b = TU.tape_region(*tapes["f32"], cfg, B, T, S, layer, which)
            assert a.shape == b.shape
            if which in TU.NARROWED:
                assert a.dtype == torch.bfloat16 and b.dtype == torch.float32
                want = b.to(torch.bfloat16)  # round to nearest even
                assert torch.equal(a.view(torch.int16), want.view(torch.int16)), f"{name} layer {layer} {which}: " \
                    f"{int((a.view(torch.int16) != want.view(torch.int16)).sum())} of {a.numel()} elements differ"
                assert not torch.equal(want.float(), b)  # (the rounding is not a no-op on these values)
            else:
                assert a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32)), (layer, which)
            assert bool(torch.isfinite(a.float()).all()), (layer, which)  # every element was written over the 0xFF fill


# ------------------------------------------------------------------------------------------------------------ 6. optimiser
def test_fused_adamw_step_gives_the_same_blob_bytes():
    cfg, sd, inp = case("G4")
    blobs = []
    for dec in pair(cfg, sd):
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
        blobs.append(dec._packed.clone())
    assert torch.equal(blobs[0], blobs[1])
