"""Training support, host side (no GPU): the oracle under torch.autograd against the reference's own gradients
(tests/golden/train_grads.npz, made by tests/golden/make_golden_train.py), the autograd option's validation, and the C ABI's new
entry points."""
import ctypes

import pytest
import torch

from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, native, synth_state_dict
from oracle import edtts_oracle as O
from train_util import oracle_grads, rel_err

NEW_SYMBOLS = ("edtts_train_tape_bytes", "edtts_train_scratch_bytes", "edtts_train_dw_slab_rows", "edtts_decoder_forward_train",
               "edtts_decoder_backward")


def golden_objective(g, dtype):
    """The fixture's decoder, inputs and v-prediction objective (train_v2.train_step) on the oracle."""
    hidden, heads, layers = (int(v) for v in g["cfg"])
    cfg = CFG(device="cpu", hidden=hidden, heads=heads, layers=layers, dropout=0.0)
    sd = synth_state_dict(cfg, 7)
    tabs = {k: v.to(dtype) for k, v in O.schedule_tables(cfg.diff_steps).items()}
    t = g["t"]
    sab = tabs["sqrt_alpha_bar"][t][:, None, None]  # (the reference's fp32 tables, cast: what its fp64 run reads)
    s1m = tabs["sqrt_one_minus_alpha_bar"][t][:, None, None]
    x0, noise = g["x0"].to(dtype), g["noise"].to(dtype)
    inp = dict(x=sab * x0 + s1m * noise, t=t, si=torch.zeros(len(t), dtype=torch.long), sem=None, f=g["feats"])
    v_target = sab * noise - s1m * x0
    return cfg, sd, inp, lambda fwd, x: torch.nn.functional.mse_loss(fwd(t), v_target)


def test_oracle_autograd_reproduces_the_reference_gradients(golden):
    g = golden("train_grads")
    out = {}
    for dtype in (torch.float64, torch.float32):
        cfg, sd, inp, loss_fn = golden_objective(g, dtype)
        out[dtype] = oracle_grads(cfg, sd, inp, dtype, loss_fn=loss_fn)
    loss64, g64 = out[torch.float64]
    loss32, g32 = out[torch.float32]
    names = sorted(k[4:] for k in g if k.startswith("g64."))
    assert names == sorted(k for k, v in g64.items() if v is not None and k not in ("d_x", "d_sem_features"))
    assert abs(float(loss64) - float(g["loss64"])) <= 1e-12 * abs(float(g["loss64"]))
    assert abs(float(loss32) - float(g["loss64"])) <= 2 * max(abs(float(g["loss32"]) - float(g["loss64"])), 2.0 ** -24 * float(g["loss64"]))
    e_or, e_ref = {}, {}
    for k in names:
        ref64 = g["g64." + k]
        assert rel_err(g64[k], ref64) < 1e-11, k  # the two fp64 runs are one arbiter
        e_ref[k] = rel_err(g["g32." + k], ref64)
        e_or[k] = rel_err(g32[k], ref64)
        print(f"{k}: oracle fp32 {e_or[k]:.2e}  reference fp32 {e_ref[k]:.2e}  ratio {e_or[k] / e_ref[k]:.2f}")
    med = float(torch.tensor(sorted(e_ref.values())).median())
    print(f"worst: oracle {max(e_or.values()):.2e} reference {max(e_ref.values()):.2e}; median reference error {med:.2e}")
    # Every tensor: the oracle's fp32 error within 2x the reference's own.  The floor is the median of the reference's errors over
    # the tensors, as in tests/test_train_gpu.py: E is measured in units of the tensor's largest element, whose fp32 ulp is 2^-24 = 6e-8,
    # so a reference error that happens to be about one ulp (8.8e-8 for layers.1.cross_attn.kv_norm.weight) says nothing about what
    # another fp32 evaluation order of the same arithmetic gives; the median (2.3e-7) is what this arithmetic typically costs.
    bad = {k: (e_or[k], e_ref[k]) for k in names if not e_or[k] <= 2 * max(e_ref[k], med)}
    assert not bad, bad


def test_autograd_needs_generic_fp32():
    cfg = CFG(device="cpu")
    for kernels in ("compiled", "auto"):
        with pytest.raises(ValueError, match="kernels='generic'"):
            EdgeDiffusionDecoder(cfg, kernels=kernels, autograd=True)
    with pytest.raises(ValueError):
        EdgeDiffusionDecoder(CFG(device="cpu", hidden=256, heads=8), compute_dtype="bf16", kernels="compiled", autograd=True)
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True)
    assert dec.autograd and all(p.requires_grad for p in dec.parameters())
    assert not any(b.requires_grad for b in dec.buffers())


def test_call_time_errors_of_the_autograd_branch():
    cfg = CFG(device="cpu")  # dropout 0.2
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True)
    x, t, sem = torch.zeros(1, 8, cfg.n_mels), torch.zeros(1, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(ValueError, match=r"cfg\.dropout = 0 or call \.eval\(\)"):
        dec.train()(x, t, sem)
    dec.eval()
    with pytest.raises(ValueError, match="x_lengths / sem_lengths"):
        dec(x, t, sem, x_lengths=torch.tensor([8]))
    with pytest.raises(ValueError, match="x_lengths / sem_lengths"):
        dec(x, t, sem, sem_lengths=torch.tensor([4]))
    with pytest.raises(ValueError, match="Either sem_idx or sem_features"):
        dec(x, t)


def test_default_decoder_is_untouched():
    cfg = CFG(device="cpu")
    for kernels in ("compiled", "generic", "auto"):
        dec = EdgeDiffusionDecoder(cfg, kernels=kernels)
        assert dec.autograd is False and dec.kernels == kernels and dec.compute_dtype == "f32"
        assert not any(p.requires_grad for p in dec.parameters())
        d, e = dec.dims(), EdgeDiffusionDecoder(cfg, kernels=kernels, autograd=False).dims()
        assert all(getattr(d, n) == getattr(e, n) for n, _ in native.EdttsDims._fields_)
        assert d.compute_dtype == native.KERNELS[kernels]
    assert EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True).dims().compute_dtype == native.KERNELS["generic"]
    # without autograd the call is the inference forward even under grad mode: on the CPU it reaches the library's device check
    dec = EdgeDiffusionDecoder(cfg, kernels="generic").eval()
    with pytest.raises(native.EdttsError, match="no CPU fallback"):
        dec(torch.zeros(1, 8, 80, requires_grad=True), torch.zeros(1, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long))


def test_new_symbols_are_declared_exported_and_bound():
    L = native.lib()
    assert L.edtts_version() == 400
    for sym in NEW_SYMBOLS:
        assert hasattr(L, sym), sym  # present in the built library


def test_tape_and_scratch_sizes_and_refusals():
    gen = EdgeDiffusionDecoder(CFG(device="cpu"), kernels="generic").dims()
    a = native.train_tape_bytes(gen, 2, 64, 32)
    assert a > 0 and native.train_tape_bytes(gen, 4, 64, 32) > a and native.train_scratch_bytes(gen, 2, 64, 32) > 0
    # exactly the regions of DESIGN.md section 19, each rounded up to 64 floats
    c = CFG(device="cpu")
    up = lambda n: (n + 63) // 64 * 64
    for B, T, S in ((2, 64, 32), (3, 50, 25), (8, 173, 100)):
        H, M, CS, FH = c.hidden, B * T, B * S, c.ffn_mult * c.hidden
        per_layer = (up(CS * (H // 2)) + up(CS * 2 * H) + 3 * up(M * H) + up(M * 3 * H) + 3 * up(M * H) + 2 * up(M * c.heads) + up(M * FH))
        floats = up(B * c.layers * 4 * H + B * H) + up(CS * H) + c.layers * per_layer + up(M * H)
        assert native.train_tape_bytes(gen, B, T, S) == 4 * floats, (B, T, S)
    for d, msg in ((EdgeDiffusionDecoder(CFG(device="cpu")).dims(), "generic kernels only"),
                   (EdgeDiffusionDecoder(CFG(device="cpu"), kernels="auto").dims(), "generic kernels only")):
        with pytest.raises(native.EdttsError, match=msg):
            native.train_tape_bytes(d, 2, 64, 32)
        out = ctypes.c_size_t(0)
        with pytest.raises(native.EdttsError, match=msg):
            native.lib().edtts_train_scratch_bytes(ctypes.byref(d), 2, 64, 32, ctypes.byref(out))
    bf = EdgeDiffusionDecoder(CFG(device="cpu"), kernels="generic").dims()
    bf.compute_dtype = 1 | 0x100
    with pytest.raises(native.EdttsError, match="fp32 only"):
        native.train_tape_bytes(bf, 2, 64, 32)
    # the dW row sum: slabs of at least 256 rows, at most 32 slabs
    assert native.train_dw_slab_rows(750) == 256 and native.train_dw_slab_rows(64 * 512) == 1024
