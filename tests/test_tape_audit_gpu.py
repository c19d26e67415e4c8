"""The stage audit of the generic training forward on the GPU: one native.decoder_forward_train into a tape
pre-filled with 0xFF bytes, then every launch of GenericLauncher::ctx / ::forward compared element by element with the fp64
evaluation of the operands that the tape itself holds (tests/tape_audit_util.py: references, bars and their derivation; the host file
shows that the references are the oracle, that the bars can be met and that they catch each kind of fault).  Every option set that
the library accepts, the head dims of k_gen_attn16<4 .. 7> that no other test reaches, dropout, and ragged batches with NaN padding.
Run on the GPU box: python -m pytest tests -m gpu."""
import copy

import pytest
import torch

import dropout_util as DU
import tape_audit_util as TA
import tape_bf16_util as TU
import train_bf16_util as U
import train_ragged_util as R
from edge_diffusion_tts_amd import EdgeDiffusionDecoder, native

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = {o: "mm%d-att%d-tape%d" % o for o in TA.OPTION_SETS}
opt_sets = pytest.mark.parametrize("opts", TA.OPTION_SETS, ids=lambda o: IDS[o])


def cu(t):
    return None if t is None else t.to(DEV)


def make(cs, opts, autograd=True, dropout=None, **kw):
    cfg = cs.cfg
    if dropout is not None:
        cfg = copy.copy(cfg)  # (the case functions cache their cfg)
        cfg.dropout = dropout
    mm, att, tp = ("bf16" if on else "f32" for on in opts)
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=autograd, matmul_dtype=mm, attn_dtype=att, tape_dtype=tp,
                               train_dropout=dropout is not None, **kw)
    dec.load_state_dict(cs.sd)
    return dec.to(DEV).eval()


def padded(cs):
    """The case's inputs with NaN in all padding (a case without lengths: as they are)."""
    inp = dict(cs.inp)
    if cs.t_len is not None:
        inp["x"] = inp["x"].masked_fill(~R.frame_mask(cs.t_len, cs.T), float("nan"))
        inp["f"] = inp["f"].masked_fill(~R.frame_mask(cs.s_len, cs.S), float("nan"))
    return inp


def run(cs, opts, drop=None, **kw):
    """One training forward into a 0xFF tape -> (the tape as tape_audit_util's dict of fp64 CPU tensors, eps, the decoder)."""
    dec = make(cs, opts, dropout=None if drop is None else drop[0], **kw)
    dims, packed = dec.dims(), dec._ensure_packed()
    cfg, B, T, S, inp = cs.cfg, cs.B, cs.T, cs.S, padded(cs)
    ws = dec.workspace(B, T, S, B, DEV)
    tape = torch.full((native.train_tape_bytes(dims, B, T, S),), 0xFF, dtype=torch.uint8, device=DEV)  # (NaN in both element types)
    sem = None if inp["f"] is not None else cu(inp["sem"])
    eps = native.decoder_forward_train(dims, packed, ws, tape, cu(inp["x"]), cu(inp["t"]), cu(inp["si"]), sem, cu(inp["f"]), S, drop,
                                       cu(cs.t_len), cu(cs.s_len))
    torch.cuda.synchronize()
    assert native.index_errors(ws) == 0

    def region(layer, which):
        r = TU.tape_region(tape, dims, cfg, B, T, S, layer, which)
        assert r.dtype == (torch.bfloat16 if opts.tape and which in TU.NARROWED else torch.float32), which
        return r.to(torch.float64).cpu()

    tp = {w: region(0, w) for w in native.TAPE_GLOBALS}
    tp["layers"] = [{w: region(l, w) for w in native.TAPE_REGIONS} for l in range(cfg.layers)]
    tp["eps"] = eps.reshape(B * T, -1).to(torch.float64).cpu()
    return tp, eps, dec


# ------------------------------------------------------------------------------------------------------------ 1. every stage, every option set
@opt_sets
@pytest.mark.parametrize("name", TA.PLAIN)
def test_every_stage_is_within_its_bar(name, opts):
    cs = TA.case(name)
    tp, eps, _ = run(cs, opts)
    TA.check(TA.audit(cs, opts, tp), f"{name} {IDS[opts]}")
    assert bool(torch.isfinite(eps).all()) and float(eps.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ 2. dropout
@opt_sets
@pytest.mark.parametrize("name", TA.DROPPED)
def test_every_stage_is_within_its_bar_under_dropout(name, opts):
    """The multipliers are the library's own masks (native.dropout_mask, which tests/test_dropout_gpu.py shows equal to dropout_util's)
    times dropout_util's scale."""
    cs = TA.case(name)
    p, seed = U.DROP_P, U.drop_seeds()[0]
    tp, eps, dec = run(cs, opts, drop=(p, seed))
    mult = {(l, site): native.dropout_mask(dec.dims(), site, l, cs.B, cs.T, cs.S, p, seed, DEV).to(torch.float64).cpu() * DU.scale(p)
            for l in range(cs.cfg.layers) for site in range(4)}
    assert all(0 < int((m != 0).sum()) < m.numel() for m in mult.values())
    TA.check(TA.audit(cs, opts, tp, mult), f"{name} p={p} {IDS[opts]}")
    plain, _, _ = run(cs, opts)
    assert not torch.equal(plain["eps"], tp["eps"])  # the masks act


# ------------------------------------------------------------------------------------------------------------ 3. ragged
@opt_sets
@pytest.mark.parametrize("name", TA.RAGGED)
def test_every_live_element_of_a_ragged_batch_is_within_its_bar(name, opts):
    """NaN in all padding of x and sem_features, 0xFF in the tape: only live rows are compared (and must have been written), the
    references read keys < T_b and < S_b only, eps rows past T_b are exactly 0."""
    cs = TA.case(name)
    tp, eps, _ = run(cs, opts, train_lengths=True)
    TA.check(TA.audit(cs, opts, tp), f"{name} {IDS[opts]}")
    dead = ~R.frame_mask(cs.t_len, cs.T).expand_as(eps)
    assert bool(torch.isfinite(eps).all()) and not bool(eps.cpu()[dead].any()) and int(dead.sum()) > 0


# ------------------------------------------------------------------------------------------------------------ 4. inference == training, bitwise
@opt_sets
@pytest.mark.parametrize("name", list(TA.DCASES))
def test_inference_forward_is_bitwise_the_training_forward(name, opts):
    """The clause that tests/test_train_gpu.py and its bf16 successors hold for the head dims of their cases, at 56, 72, 90 and 104."""
    cs = TA.case(name)
    inp = cs.inp
    _, eps, _ = run(cs, opts)
    with torch.no_grad():
        got = make(cs, opts, autograd=False)(cu(inp["x"]), cu(inp["t"]), cu(inp["sem"]), cu(inp["si"]), cu(inp["f"]))
    assert torch.equal(got, eps)
