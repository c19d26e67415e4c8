"""Training on ragged batches on the GPU: EdgeDiffusionDecoder(kernels="generic", autograd=True, train_lengths=True) against the
ragged oracle of tests/train_ragged_util.py (one oracle call per trimmed utterance), and the bitwise clauses of the contract in
include/edtts.h ("training on ragged batches") / DESIGN.md section 22.  Bar as in tests/test_train_gpu.py: per gradient tensor
E <= MARGIN * max(E_ref, median E_ref) against the fp64 oracle.  Run on the GPU box: python -m pytest tests -m gpu."""
import copy

import pytest
import torch

import dropout_util as D
from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, SemanticEncoder, native
from edge_diffusion_tts_amd.synth import synth_hubert_features, synth_semantic_head
from train_ragged_util import RAGGED, case, frame_mask, masked_loss, ragged_pair
from train_util import check_against_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
DROP_P, DROP_GEN = 0.2, 31


def cu(t):
    return None if t is None else t.to(DEV)


def make(cfg, sd, autograd=True, train_lengths=True, dropout=False):
    if dropout:
        cfg = copy.copy(cfg)
        cfg.dropout = DROP_P
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=autograd, train_lengths=train_lengths and autograd,
                               train_dropout=dropout)
    dec.load_state_dict(sd)
    dec = dec.to(DEV)
    if dropout:
        dec.dropout_generator = torch.Generator().manual_seed(DROP_GEN)
        return dec.train()
    return dec.eval()


def garbage(inp, t_len, s_len, nan=True):
    """A copy of the inputs with the padding overwritten: NaN in x / sem_features / target, 2**62 and -1 in sem_idx."""
    out = dict(inp)
    B, T = inp["x"].shape[:2]
    live_t = frame_mask(t_len, T)
    fill = float("nan") if nan else 0.0
    out["x"] = inp["x"].masked_fill(~live_t, fill)
    if inp["f"] is not None:
        out["f"] = inp["f"].masked_fill(~frame_mask(s_len, inp["f"].shape[1]), fill)
    if inp["sem"] is not None:
        S = inp["sem"].shape[1]
        dead = ~frame_mask(s_len, S)[..., 0]
        bad = torch.where(torch.arange(S)[None, :] % 2 == 0, torch.tensor(2 ** 62), torch.tensor(-1)).expand(B, S)
        out["sem"] = torch.where(dead, bad if nan else torch.zeros_like(bad), inp["sem"])
    return out


def collect(dec, x, f):
    got = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in dec.named_parameters()}
    got["d_x"] = x.grad.detach().clone()
    if f is not None:
        got["d_sem_features"] = f.grad.detach().clone()
    return got


def run(name, dec=None, inp=None, lens=None, dropout=False, between=None):
    """One ragged forward and backward through the module: (decoder, gradients, eps)."""
    cfg, sd, inp0, t_len, s_len = case(name)
    inp = inp or inp0
    if lens is not None:
        t_len, s_len = lens
    dec = dec or make(cfg, sd, dropout=dropout)
    dec.zero_grad(set_to_none=True)
    x = cu(inp["x"]).requires_grad_(True)
    f = None if inp["f"] is None else cu(inp["f"]).requires_grad_(True)
    eps = dec(x, cu(inp["t"]), cu(inp["sem"]), cu(inp["si"]), f, x_lengths=t_len, sem_lengths=s_len)
    loss = masked_loss(eps, cu(inp0["target"]), cu(t_len))
    if between is not None:
        between(dec)
    loss.backward()
    return dec, collect(dec, x, f), eps.detach()


def assert_same(a, b, what=""):
    assert set(a) == set(b)
    for k in a:
        if a[k] is None:
            assert b[k] is None, k
        else:
            assert torch.equal(a[k], b[k]), f"{what} {k}: {int((a[k] != b[k]).sum())} elements differ"


# ------------------------------------------------------------------------------------------------------------ the oracle bar
@pytest.mark.parametrize("name", sorted(RAGGED))
def test_gradients_against_the_ragged_fp64_oracle(name):
    """Garbage in all padding (NaN, out-of-range ids).  Worst ratio measured on MI355X: DESIGN.md section 22."""
    cfg, sd, inp, t_len, s_len = case(name)
    g64, e_ref, med, eps32 = ragged_pair(name)
    _, got, eps = run(name, inp=garbage(inp, t_len, s_len))
    assert float((eps.cpu() - eps32).abs().max()) <= 1e-4  # tests/test_generic_gpu.py's forward tolerance
    check_against_oracle(got, g64, e_ref, med, name)
    for k, v in got.items():
        if v is not None:
            assert bool(torch.isfinite(v).all()), k


def test_gradients_with_dropout_against_the_masked_ragged_oracle():
    drop = (DROP_P, D.seeds_of(DROP_GEN)[0])
    cfg, sd, inp, t_len, s_len = case("R1")
    g64, e_ref, med, eps32 = ragged_pair("R1", drop)
    dec, got, eps = run("R1", inp=garbage(inp, t_len, s_len), dropout=True)
    assert dec.last_dropout_seed == drop[1]
    assert float((eps.cpu() - eps32).abs().max()) <= 1e-4
    check_against_oracle(got, g64, e_ref, med, "R1 dropout")


# ------------------------------------------------------------------------------------------------------------ bitwise clauses
@pytest.mark.parametrize("name", sorted(RAGGED))
def test_forward_is_the_inference_forward_with_lengths(name):
    cfg, sd, inp, t_len, s_len = case(name)
    inp = garbage(inp, t_len, s_len)
    train, infer = make(cfg, sd), make(cfg, sd, autograd=False)
    args = (cu(inp["x"]), cu(inp["t"]), cu(inp["sem"]), cu(inp["si"]), cu(inp["f"]))
    a = train(*args, x_lengths=t_len, sem_lengths=s_len)
    assert a.grad_fn is not None
    b = infer(*args, x_lengths=t_len, sem_lengths=s_len)
    assert torch.equal(a.detach(), b)
    assert float(a.detach().masked_select(~frame_mask(cu(t_len), a.shape[1])).abs().sum()) == 0.0


@pytest.mark.parametrize("name", ["R1", "R2"])
def test_input_gradients_are_the_solo_calls(name):
    """d_x[b, :T_b] / d_sem_features[b, :S_b] are bitwise those of utterance b alone through the pad-free path (B = 1, T_b, S_b, no
    lengths) given d_eps[b, :T_b], and exactly 0 past the lengths."""
    cfg, sd, inp, t_len, s_len = case(name)
    g = garbage(inp, t_len, s_len)
    dec = make(cfg, sd)
    x, f = cu(g["x"]).requires_grad_(True), cu(g["f"]).requires_grad_(True)
    eps = dec(x, cu(inp["t"]), None, cu(inp["si"]), f, x_lengths=t_len, sem_lengths=s_len)
    d_eps = cu(torch.randn(eps.shape, generator=torch.Generator().manual_seed(9)))
    eps.backward(d_eps.masked_fill(~frame_mask(cu(t_len), eps.shape[1]), float("nan")))
    solo = make(cfg, sd, train_lengths=False)
    for b in range(len(t_len)):
        Tb, Sb = int(t_len[b]), int(s_len[b])
        xb = cu(inp["x"][b:b + 1, :Tb]).requires_grad_(True)
        fb = cu(inp["f"][b:b + 1, :Sb]).requires_grad_(True)
        e = solo(xb, cu(inp["t"][b:b + 1]), None, cu(inp["si"][b:b + 1]), fb)
        assert torch.equal(e.detach()[0], eps.detach()[b, :Tb])
        e.backward(d_eps[b:b + 1, :Tb])
        assert torch.equal(x.grad[b, :Tb], xb.grad[0]), (name, b)
        assert torch.equal(f.grad[b, :Sb], fb.grad[0]), (name, b)
        assert float(xb.grad.abs().max()) > 0 and float(fb.grad.abs().max()) > 0
        assert float(x.grad[b, Tb:].abs().sum()) == 0.0 and float(f.grad[b, Sb:].abs().sum()) == 0.0


@pytest.mark.parametrize("name", ["R2", "R3"])
def test_padding_is_never_read(name):
    """native level.  Run A: zeros in all padding, tape and scratch zero-filled.  Run B: NaN in the padding of x, sem_features and
    d_eps, 2**62 / -1 in the padding of sem_idx, tape and scratch pre-filled with 0xFF bytes.  Every output bit is the same."""
    cfg, sd, inp, t_len, s_len = case(name)
    dec = make(cfg, sd)
    dims, packed = dec.dims(), dec._ensure_packed()
    B, T, _ = inp["x"].shape
    S = inp["f"].shape[1] if inp["f"] is not None else inp["sem"].shape[1]
    names, params = dec._named_params()
    tl, sl = cu(t_len), cu(s_len)
    d_eps0 = 2.0 * (torch.randn(B, T, cfg.n_mels, generator=torch.Generator().manual_seed(3)))
    outs = []
    for nan in (False, True):
        g = garbage(inp, t_len, s_len, nan)
        fill = 0xFF if nan else 0
        ws = dec.workspace(B, T, S, B, DEV)
        tape = torch.full((native.train_tape_bytes(dims, B, T, S),), fill, dtype=torch.uint8, device=DEV)
        scratch = torch.full((native.train_scratch_bytes(dims, B, T, S),), fill, dtype=torch.uint8, device=DEV)
        x, f, sem = cu(g["x"]), cu(g["f"]), cu(g["sem"])
        eps = native.decoder_forward_train(dims, packed, ws, tape, x, cu(inp["t"]), cu(inp["si"]), sem, f, S, None, tl, sl)
        d_eps = cu(d_eps0.masked_fill(~frame_mask(t_len, T), float("nan") if nan else 0.0))
        out = {n: torch.full_like(p, float("nan")) for n, p in zip(names, params)
               if dec._enters_output(n, f is not None, inp["si"] is not None)}
        slots = [out.get(dec._slot_param(n)) for n in native.slot_names(cfg.layers)]
        d_x = torch.full_like(x, float("nan"))
        d_f = None if f is None else torch.full_like(f, float("nan"))
        native.decoder_backward(dims, packed, ws, tape, x, cu(inp["t"]), cu(inp["si"]), sem, f, S, d_eps, slots, d_x, d_f, None, tl, sl,
                                scratch=scratch)
        assert native.index_errors(ws) == 0
        out.update(eps=eps, d_x=d_x)
        if d_f is not None:
            out["d_sem_features"] = d_f
        outs.append(out)
    assert_same(outs[0], outs[1], name)
    for k, v in outs[1].items():
        assert bool(torch.isfinite(v).all()), k
        assert float(v.abs().max()) > 0, k


def test_full_lengths_are_no_lengths():
    cfg, sd, inp, t_len, s_len = case("R2")
    B, T = inp["x"].shape[:2]
    full = (torch.full((B,), T), torch.full((B,), inp["f"].shape[1]))
    dec, a, eps_a = run("R2", lens=full)
    plain = make(cfg, sd, train_lengths=False)
    plain.zero_grad(set_to_none=True)
    x, f = cu(inp["x"]).requires_grad_(True), cu(inp["f"]).requires_grad_(True)
    eps_b = plain(x, cu(inp["t"]), None, cu(inp["si"]), f)
    masked_loss(eps_b, cu(inp["target"]), cu(full[0])).backward()
    assert torch.equal(eps_a, eps_b.detach())
    assert_same(a, collect(plain, x, f), "full lengths")


def test_backward_is_reproducible():
    cfg, sd, inp, t_len, s_len = case("R2")
    dec, a, _ = run("R2")
    _, b, _ = run("R2", dec=dec)
    other = []

    def between(d):  # another ragged forward (other lengths: it overwrites the shared workspace) between a forward and its backward
        other.append(d(cu(inp["target"]), cu(inp["t"]), None, cu(inp["si"]), cu(inp["f"]) * 0.5, x_lengths=t_len.flip(0),
                       sem_lengths=s_len.flip(0)))

    _, c, _ = run("R2", dec=dec, between=between)
    assert other[0].grad_fn is not None
    assert_same(a, b, "second backward")
    assert_same(a, c, "forward in between")


def test_dropout_rows_do_not_depend_on_the_other_utterances():
    """Masks are keyed by the padded layout: utterance 0's eps, d_x and d_sem_features rows are bitwise unchanged when utterance 1's
    lengths and contents change (same seed, the same d_eps rows for utterance 0)."""
    cfg, sd, inp, t_len, s_len = case("R1")
    inp2 = dict(inp)
    inp2["x"] = inp["x"].clone()
    inp2["f"] = inp["f"].clone()
    inp2["x"][1] = inp["x"][1].flip(0) * 1.5
    inp2["f"][1] = float("nan")
    inp2["f"][1, :4] = 0.25
    t2, s2 = t_len.clone(), s_len.clone()
    t2[1], s2[1] = 33, 4
    a, b = _rows_of_utterance0(cfg, sd, inp, t_len, s_len), _rows_of_utterance0(cfg, sd, inp2, t2, s2)
    for u, v in zip(a[:3], b[:3]):
        assert torch.equal(u, v) and float(u.abs().max()) > 0
    assert not torch.equal(a[3], b[3])  # (utterance 1 did change)


def _rows_of_utterance0(cfg, sd, inp, t_len, s_len):
    """(eps[0], d_x[0], d_sem_features[0], eps[1]) of a dropout forward and backward whose d_eps does not depend on the batch."""
    dec = make(cfg, sd, dropout=True)
    x = cu(inp["x"]).requires_grad_(True)
    f = cu(inp["f"]).requires_grad_(True)
    eps = dec(x, cu(inp["t"]), None, cu(inp["si"]), f, x_lengths=t_len, sem_lengths=s_len)
    d_eps = cu(torch.randn(eps.shape, generator=torch.Generator().manual_seed(9)))
    eps.backward(d_eps)
    assert dec.last_dropout_seed == D.seeds_of(DROP_GEN)[0]
    return eps.detach()[0].clone(), x.grad[0].clone(), f.grad[0].clone(), eps.detach()[1].clone()


# ------------------------------------------------------------------------------------------------------------ the chain
def test_ragged_head_into_ragged_decoder():
    """SemanticEncoder(autograd=True) with lengths -> the ragged decoder through sem_features.  One loss.backward() gives the head
    bitwise the gradients of the same chain cut in two (the decoder on a detached leaf, then z_q.backward(leaf.grad)); an AdamW step
    on both modules' parameters lowers the masked loss on the same batch."""
    cfg, sd, inp, t_len, s_len = case("R2")
    B, S, in_dim = inp["f"].shape[0], inp["f"].shape[1], 64
    proj_sd, q_sd = synth_semantic_head(in_dim, cfg.semantic_dim, cfg.fsq_levels, seed=6, dropout_layout=True)
    enc = SemanticEncoder(cfg, in_dim=in_dim, proj_dropout=True, autograd=True)
    enc.proj.load_state_dict(proj_sd)
    enc.vq.load_state_dict(q_sd)
    enc = enc.to(DEV).eval()
    dec = make(cfg, sd)
    h = cu(synth_hubert_features(B, S, in_dim, 100))
    tl, sl = cu(t_len), cu(s_len)
    x, t, si, target = cu(inp["x"]), cu(inp["t"]), cu(inp["si"]), cu(inp["target"])

    def loss_of(zq):
        return masked_loss(dec(x, t, sem_features=zq, step_idx=si, x_lengths=tl, sem_lengths=sl), target, tl)

    head = enc.get_trainable_params()
    zq = enc.forward_features(h, sl)[0]
    assert zq.grad_fn is not None
    loss0 = loss_of(zq)
    loss0.backward()
    one = [p.grad.clone() for p in head]
    dec_one = {k: p.grad.clone() for k, p in dec.named_parameters() if p.grad is not None}
    assert all(float(g.abs().max()) > 0 for g in one)
    for p in head:
        p.grad = None
    dec.zero_grad(set_to_none=True)
    zq = enc.forward_features(h, sl)[0]
    leaf = zq.detach().requires_grad_(True)
    loss_of(leaf).backward()
    assert float(leaf.grad.masked_select(~frame_mask(sl, S)).abs().sum()) == 0.0
    zq.backward(leaf.grad)
    for g, p in zip(one, head):
        assert torch.equal(g, p.grad)
    for k, p in dec.named_parameters():
        if p.grad is not None:
            assert torch.equal(dec_one[k], p.grad), k
    params = head + list(dec.parameters())
    opt = torch.optim.AdamW(params, lr=1e-3)
    opt.step()
    with torch.no_grad():
        loss1 = loss_of(enc.forward_features(h, sl)[0])
    print(f"masked loss {float(loss0.detach()):.6f} -> {float(loss1):.6f}")
    assert float(loss1) < float(loss0.detach())
