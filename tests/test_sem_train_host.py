"""Host-side tests of the semantic head's training path: the conditions the GPU tests rely on, the mask
restatement, the C ABI surface and the constructor errors.  No GPU."""
import os

import numpy as np
import pytest
import torch

import dropout_util as D
import sem_train_util as U
from edge_diffusion_tts_amd import CFG, native
from edge_diffusion_tts_amd.encoder import FSQEncoder, SemanticEncoder

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("edtts_sem_train_packed_bytes", "edtts_sem_train_pack", "edtts_sem_train_tape_bytes", "edtts_sem_train_scratch_bytes",
               "edtts_sem_encode_train", "edtts_sem_backward", "edtts_sem_dropout_mask")


def _variants(name):
    out = [(None, None)] + [(s, None) for s in U.DROP_SEEDS.get(name, ())]
    if name == "H2":
        out += [(None, U.H2_LENGTHS), (U.DROP_SEEDS["H2"][0], U.H2_LENGTHS)]
    return out


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_margin_condition(name):
    """Every FSQ coordinate of every frame has an fp64 decision margin >= 1e-4, and the fp32 and fp64 oracle agree on every idx --
    without dropout, under each dropout seed the GPU tests use and for the trimmed utterances of the ragged test."""
    for drop_seed, lengths in _variants(name):
        _, e_ref, med, _, idx64, idx32, margin = U.oracle_pair(name, drop_seed, lengths)
        print(f"{name} drop_seed={drop_seed} lengths={lengths}: min margin {float(margin.min()):.2e}, median E_ref {med:.2e}")
        assert float(margin.min()) >= U.MIN_MARGIN
        assert torch.equal(idx64, idx32)
        assert len(torch.unique(idx64)) > 1 or idx64.numel() < 4


def test_mask_known_answer():
    """The head's mask restatement against fields computed by hand from one Philox known answer (Random123's kat_vectors: counter
    and key all ones -> 408f276d 41c83b0e a20bc7c6 6d5451fd), and its placement: the stream word, c0 = n >> 3, c1 = m, field n & 7."""
    ones = 0xFFFFFFFF
    words = D.philox4x32_10((ones, ones), (ones, ones, ones, ones))
    assert [int(w) for w in words] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    by_hand = [0x276D, 0x408F, 0x3B0E, 0x41C8, 0xC7C6, 0xA20B, 0x51FD, 0x6D54]
    assert [int(D.field(words, j)) for j in range(8)] == by_hand
    # one row of the head's site, rebuilt from single draws
    seed, p, rows, width = 0x1234567890ABCDEF, 0.2, 5, 24
    keep = U.head_keep(seed, p, rows, width)
    thr = D.threshold(p)
    assert thr == 13107
    for m in (0, 4):
        for n in (0, 7, 8, 23):
            w = D.philox4x32_10((seed & ones, seed >> 32), (n >> 3, m, 0x40000, 0))
            assert bool(keep[m, n]) == (int(D.field(w, n & 7)) >= thr)
    # another stream word gives another mask: the decoder's site 2 of layer 0 (0x30002) with the same positions
    assert not np.array_equal(keep, D.row_keep(seed, p, 0, D.SITE_ACT, rows, width))
    frac = U.head_keep(7, 0.5, 64, 128).mean()
    assert 0.45 < frac < 0.55
    mult = U.head_multiplier(7, 0.5, 2, 32, 128, torch.float64)
    assert set(mult.unique().tolist()) == {0.0, 2.0}


def test_c_abi_surface():
    L = native.lib()
    for sym in NEW_SYMBOLS:
        assert hasattr(L, sym), sym
    with open(os.path.join(REPO, "include", "edtts.h")) as f:
        assert "0x40000" in f.read()
    assert native.SEM_DROP_STREAM == U.SEM_STREAM == 0x40000


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_tape_and_scratch_bytes(name):
    """tape = 4 (2 M S + 16 M) bytes with a proj, 4 * 16 M without; scratch = 4 (32 M + 2 M S [+ 4 M S + 2 M]
    + part) with every term rounded up to 4 floats and part the largest partial-sum buffer."""
    in_dim, S, levels, p, B, T = U.CASES[name]
    dims = native.sem_dims(in_dim, S, levels)
    M = B * T
    assert native.sem_train_tape_bytes(dims, B, T) == 4 * ((2 * M * S if in_dim else 0) + 16 * M)
    r4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
    rows = native.train_dw_slab_rows(M)
    ns = (M + rows - 1) // rows
    part = 0
    if ns > 1:
        part = ns * max([S * 16] + ([S * S, S * in_dim] if in_dim else []))
    part = max(part, (M + 255) // 256 * S)
    if in_dim:
        part = max(part, B * ((T + 63) // 64) * 3 * S)
    want = 2 * r4(16 * M) + 2 * r4(M * S) + ((4 * r4(M * S) + r4(2 * M)) if in_dim else 0) + r4(part)
    assert native.sem_train_scratch_bytes(dims, B, T) == 4 * want
    # the training blob: Wu^T, Wd^T (one 16-wide tile row / column each) and W3^T, in 16 x 16 fragment tiles
    nt = S // 16
    assert native.sem_train_packed_bytes(dims) == 4 * 256 * (2 * nt + (nt * nt if in_dim else 0))
    # ... and the inference blob is what it was
    assert native.sem_packed_bytes(dims) == native.sem_packed_bytes(native.sem_dims(in_dim, S, levels))


def test_argument_errors_before_pointers():
    """VQ dims, a wrong slot count and an invalid p are reported with every pointer NULL."""
    L = native.lib()
    import ctypes as C
    vq = native.sem_dims(64, 32, None, 128)
    out = C.c_size_t(0)
    for fn, args in ((L.edtts_sem_train_packed_bytes, (C.byref(vq), C.byref(out))),
                     (L.edtts_sem_train_tape_bytes, (C.byref(vq), 1, 1, C.byref(out))),
                     (L.edtts_sem_encode_train, (C.byref(vq), None, None, 1, 1, None, None, None, None, None, None, None)),
                     (L.edtts_sem_backward, (C.byref(vq), None, None, None, None, 1, 1, None, None, None, 0, None, None, None, None))):
        with pytest.raises(native.EdttsError, match="FSQ quantizer only"):
            fn(*args)
    fsq = native.sem_dims(64, 32, [3, 3])
    with pytest.raises(native.EdttsError, match="expected 10 gradient slots"):
        L.edtts_sem_backward(C.byref(fsq), None, None, None, None, 1, 1, None, None, None, 4, None, None, None, None)
    for p in (1.0, -0.1, 0.999995):
        bad = native.EdttsDropout(p, 1)
        with pytest.raises(native.EdttsError, match="dropout p="):
            L.edtts_sem_encode_train(C.byref(fsq), None, None, 1, 1, None, None, None, None, None, C.byref(bad), None)
        with pytest.raises(native.EdttsError, match="dropout p="):
            L.edtts_sem_dropout_mask(C.byref(fsq), 1, 1, C.byref(bad), None, None)
    alone = native.sem_dims(0, 32, [3, 3])
    with pytest.raises(native.EdttsError, match="no dropout site"):
        L.edtts_sem_encode_train(C.byref(alone), None, None, 1, 1, None, None, None, None, None, C.byref(native.EdttsDropout(0.5, 1)), None)
    with pytest.raises(native.EdttsError, match="NULL pointer"):
        L.edtts_sem_encode_train(C.byref(fsq), None, None, 1, 1, None, None, None, None, None, None, None)


def test_constructor_errors():
    fsq = CFG(device="cpu", use_fsq=True, fsq_levels=[3, 3], semantic_dim=32, dropout=0.1)
    vq = CFG(device="cpu", use_fsq=False, semantic_dim=32, codebook_size=64)
    with pytest.raises(ValueError, match="VQ path"):
        SemanticEncoder(vq, in_dim=64, autograd=True)
    with pytest.raises(ValueError, match="needs autograd=True"):
        SemanticEncoder(fsq, in_dim=64, proj_dropout=True, train_dropout=True)
    with pytest.raises(ValueError, match="Dropout layout"):
        SemanticEncoder(fsq, in_dim=64, autograd=True, train_dropout=True)
    for p in (1.0, -0.5, 0.999995):
        with pytest.raises(ValueError, match="outside"):
            SemanticEncoder(CFG(device="cpu", use_fsq=True, fsq_levels=[3, 3], semantic_dim=32, dropout=p), in_dim=64, proj_dropout=True,
                            autograd=True, train_dropout=True)
    enc = SemanticEncoder(fsq, in_dim=64, proj_dropout=True, autograd=True, train_dropout=True)
    assert enc.last_dropout_seed is None and enc.dropout_generator is None
    want = [p for p in enc.proj.parameters()] + [p for p in enc.vq.parameters()]
    got = enc.get_trainable_params()
    assert len(got) == len(want) == 10 and all(a is b for a, b in zip(got, want)) and all(p.requires_grad for p in got)
    assert SemanticEncoder(fsq, in_dim=64).autograd is False and FSQEncoder(32, [3, 3]).autograd is False
    # without train_dropout, a differentiable training-mode call with p > 0 names both ways out (raised before any device work)
    plain = SemanticEncoder(fsq, in_dim=64, proj_dropout=True, autograd=True).train()
    with pytest.raises(ValueError, match=r"train_dropout=True.*\.eval\(\)"):
        plain.quantize_features(torch.zeros(1, 2, 64))


def test_oracle_reproduces_the_reference_head_gradients(golden):
    """tests/golden/train_head.npz (the reference's FSQEncoder behind train_v2's proj, into the reference's decoder, one backward):
    the composed CPU oracle -- sem_train_util's head with the contract's mask into oracle.decoder_forward -- gives its fp64 gradients
    to 1e-10."""
    from edge_diffusion_tts_amd import synth_state_dict
    from oracle import edtts_oracle as O
    g = golden("train_head")
    hidden, heads, layers, sem_dim, in_dim = (int(v) for v in g["cfg"])
    levels = [int(v) for v in g["levels"]]
    p, seed = float(g["p"]), int(g["seed"])
    assert seed == D.seeds_of(int(g["gen"]))[0] and float(g["margin"]) >= U.MIN_MARGIN
    dt = torch.float64
    cfg = CFG(device="cpu", hidden=hidden, heads=heads, layers=layers, dropout=0.0, semantic_dim=sem_dim)
    sd = {k: (v.to(dt).requires_grad_(True) if v.is_floating_point() and "pos_emb" not in k else v) for k, v in synth_state_dict(cfg, 7).items()}
    w = U.weights_of({k[len("w.proj."):]: g[k] for k in g if k.startswith("w.proj.")}, {k[len("w.fsq."):]: g[k] for k in g if k.startswith("w.fsq.")})
    w = {k: v.to(dt).requires_grad_(True) for k, v in w.items()}
    B, S = g["h"].shape[0], g["h"].shape[1]
    zq, idx, _ = U.head_forward(w, g["h"].to(dt), levels, U.head_multiplier(seed, p, B, S, sem_dim, dt))
    assert torch.equal(idx, g["idx"])
    tabs = {k: v.to(dt) for k, v in O.schedule_tables(cfg.diff_steps).items()}
    t = g["t"]
    sab, s1m = tabs["sqrt_alpha_bar"][t][:, None, None], tabs["sqrt_one_minus_alpha_bar"][t][:, None, None]
    x0, noise = g["x0"].to(dt), g["noise"].to(dt)
    out = O.decoder_forward(sd, sab * x0 + s1m * noise, t, None, torch.zeros(len(t), dtype=torch.long), zq, heads=heads, window=cfg.attn_window_size)
    loss = torch.nn.functional.mse_loss(out, sab * noise - s1m * x0)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss64"])) <= 1e-12 * abs(float(g["loss64"]))
    got = {"decoder." + k: v.grad for k, v in sd.items() if v.is_floating_point() and v.requires_grad and v.grad is not None}
    last = {"w1": "proj.0.weight", "b1": "proj.0.bias", "lng": "proj.2.weight", "lnb": "proj.2.bias", "w3": "proj.4.weight", "b3": "proj.4.bias",
            "wd": "fsq.proj_down.weight", "bd": "fsq.proj_down.bias", "wu": "fsq.proj_up.weight", "bu": "fsq.proj_up.bias"}
    got.update({"encoder." + last[k]: v.grad for k, v in w.items()})
    names = sorted(k[4:] for k in g if k.startswith("g64."))
    assert sorted(got) == names and sum(n.startswith("encoder.") for n in names) == 10
    worst = max(U.rel_err(got[k], g["g64." + k]) for k in names)
    print(f"composed oracle vs the reference's fp64 gradients: worst relative error {worst:.2e}")
    assert worst <= 1e-10
