"""Training on ragged batches, host side (no GPU): the new C entry points, the train_lengths option's validation, and the ragged
oracle of tests/train_ragged_util.py -- that it is the plain oracle at full lengths, and that the cases are not vacuous (an oracle
whose attentions see the padding lands far outside the GPU bar)."""
import ctypes
import re

import pytest
import torch

from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, native
from train_ragged_util import RAGGED, case, padded_grads, ragged_grads, ragged_pair
from train_util import case as plain_case, oracle_grads, rel_err

NEW_SYMBOLS = ("edtts_decoder_forward_train_len", "edtts_decoder_backward_len")


def test_new_symbols_are_declared_exported_and_bound():
    L = native.lib()
    assert L.edtts_version() == 400
    for sym in NEW_SYMBOLS:
        assert hasattr(L, sym), sym


def test_plain_size_queries_are_unchanged():
    """Lengths add no region to the tape or the scratch: the byte counts recorded before the _len entry points existed."""
    gen = EdgeDiffusionDecoder(CFG(device="cpu"), kernels="generic").dims()
    recorded = {(2, 64, 32): (4175104, 1037312), (3, 50, 25): (4901632, 1227008), (8, 173, 100): (45756416, 13760256),
                (64, 512, 256): (1063952384, 271654912)}
    for (B, T, S), (tape, scratch) in recorded.items():
        assert native.train_tape_bytes(gen, B, T, S) == tape, (B, T, S)
        assert native.train_scratch_bytes(gen, B, T, S) == scratch, (B, T, S)


def test_argument_errors_come_before_any_pointer_is_looked_at():
    L = native.lib()
    d = EdgeDiffusionDecoder(CFG(device="cpu"), kernels="generic").dims()
    bad = native.EdttsDropout(1.0, 1)
    calls = ((L.edtts_decoder_forward_train_len, (d, None, None, None, 2, 64, 32, None, None, None, None, None, None)),
             (L.edtts_decoder_backward_len, (d, None, None, None, 2, 64, 32, None, None, None, None, None, None, None, 0, None, None, None)))
    for fn, head in calls:
        with pytest.raises(native.EdttsError, match="dropout p=1"):
            fn(ctypes.byref(head[0]), *head[1:], ctypes.byref(bad), None, None, None)
        with pytest.raises(ValueError, match="Either sem_idx or sem_features"):
            fn(ctypes.byref(head[0]), *head[1:], None, None, None, None)
    comp = EdgeDiffusionDecoder(CFG(device="cpu"), kernels="compiled").dims()
    for fn, head in calls:
        with pytest.raises(native.EdttsError, match="generic kernels only"):
            fn(ctypes.byref(comp), *head[1:], None, None, None, None)


def test_option_validation():
    cfg = CFG(device="cpu", dropout=0.0)
    with pytest.raises(ValueError, match="train_lengths=True needs autograd=True"):
        EdgeDiffusionDecoder(cfg, kernels="generic", train_lengths=True)
    x, t, sem = torch.zeros(2, 8, cfg.n_mels), torch.zeros(2, dtype=torch.long), torch.zeros(2, 4, dtype=torch.long)
    # without the option: the old refusal
    old = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True)
    assert old.train_lengths is False
    with pytest.raises(ValueError, match="x_lengths / sem_lengths"):
        old(x, t, sem, x_lengths=torch.tensor([8, 3]))
    # with it: native.lengths' errors, before the library is reached
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, train_lengths=True)
    with pytest.raises(ValueError, match="expected dtype torch.int64"):
        dec(x, t, sem, x_lengths=torch.tensor([8, 3], dtype=torch.int32))
    with pytest.raises(ValueError, match=r"expected shape \[2\]"):
        dec(x, t, sem, sem_lengths=torch.tensor([4]))
    with pytest.raises(ValueError, match=r"x_lengths: lengths must be in \[1, 8\]"):
        dec(x, t, sem, x_lengths=torch.tensor([9, 3]))
    with pytest.raises(ValueError, match=r"sem_lengths: lengths must be in \[1, 4\]"):
        dec(x, t, sem, sem_lengths=torch.tensor([0, 4]))
    # a good CPU call reaches the library's device check
    with pytest.raises(native.EdttsError, match="no CPU fallback"):
        dec(x, t, sem, x_lengths=torch.tensor([8, 3]), sem_lengths=torch.tensor([4, 1]))
    both = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True, train_dropout=True, train_lengths=True)
    assert both.train_dropout and both.train_lengths


def test_full_lengths_are_the_plain_oracle():
    for name in ("G2", "G1"):
        cfg, sd, inp = plain_case(name)
        B, T = inp["x"].shape[:2]
        S = inp["f"].shape[1] if inp["f"] is not None else inp["sem"].shape[1]
        loss, g, eps = ragged_grads(cfg, sd, inp, torch.full((B,), T), torch.full((B,), S), torch.float64)
        loss0, g0 = oracle_grads(cfg, sd, inp, torch.float64)
        assert abs(float(loss) - float(loss0)) <= 1e-13 * abs(float(loss0))
        assert set(g) == set(g0)
        for k, v in g0.items():
            assert (v is None) == (g[k] is None), k
            if v is not None:
                assert rel_err(g[k], v) < 1e-12, (name, k)


@pytest.mark.parametrize("name", sorted(RAGGED))
def test_cases_are_not_vacuous(name):
    """An fp64 oracle whose attentions see the padding (no lengths, loss over the live frames) is E > 1e-2 away from the ragged one on
    the weights of both attentions: a backward that ignored the key counts could not pass the GPU bar.  And every fp64 gradient of
    the ragged oracle is non-zero, with exact zeros past the lengths in the input gradients."""
    cfg, sd, inp, t_len, s_len = case(name)
    g64, e_ref, med, _ = ragged_pair(name)
    gp = padded_grads(cfg, sd, inp, t_len, torch.float64)
    assert set(gp) == set(g64)
    attn = [k for k in g64 if g64[k] is not None and re.search(r"\.(attn|cross_attn)\..*weight$", k)]
    assert len(attn) == cfg.layers * 7, attn
    for k in attn:
        e = rel_err(gp[k], g64[k])
        print(f"{name} {k}: padded vs ragged E {e:.2e}")
        assert e > 1e-2, (name, k, e)
    for k, v in g64.items():
        if v is not None:
            assert float(v.abs().max()) > 0, (name, k)
    for b in range(len(t_len)):
        assert float(g64["d_x"][b, int(t_len[b]):].abs().sum()) == 0
        assert float(g64["d_x"][b, :int(t_len[b])].abs().min(dim=-1).values.max()) > 0
        if "d_sem_features" in g64:
            assert float(g64["d_sem_features"][b, int(s_len[b]):].abs().sum()) == 0
    assert med > 0 and all(v >= 0 for v in e_ref.values())
