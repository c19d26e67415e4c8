"""The generic (run-time-shape) fp32 kernels on the GPU: decoder shapes that have no compiled instance against the CPU oracle, the
samplers on top of them, agreement with the fused kernels where both exist, determinism and mode selection.
Run on the GPU box: python -m pytest tests -m gpu."""
import pytest
import torch

from conftest import max_abs
from edge_diffusion_tts_amd import (CFG, DiffusionSchedule, EdgeDiffusionDecoder, EdgeInference, native, synth_state_dict)
from oracle import edtts_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL = 1e-4  # single forward vs the fp32 oracle
E2E_TOL = 1e-3  # end to end, outside the t=999 amplification band


def make(cfg, kernels="generic", seed=0):
    dec = EdgeDiffusionDecoder(cfg, kernels=kernels)
    sd = synth_state_dict(cfg, seed, max_pos=dec.max_len, max_ctx_pos=dec.max_context_len)
    dec.load_state_dict(sd)
    return dec.to(DEV).eval(), sd


def cu(t):
    return None if t is None else t.to(DEV)


def amplification_band(x_T, eps0, k=4.0):
    """The elements whose first-step x0 is not safely clamped at t=999: there eps rounding is amplified 64171x."""
    ab = O.schedule_tables(1000)["alpha_bar"][999].double()
    return (x_T.double() - torch.sqrt(1 - ab) * eps0.double()).abs() < 3.0 * torch.sqrt(ab) * k


def e2e_check(ours, ref, band, what):
    err = (ours.double() - ref.double()).abs()
    out = float(err[~band].max())
    print(f"{what}: outside the band max {out:.2e}; in band {int(band.sum())} elements")
    assert out <= E2E_TOL, (what, out)


# (cfg kwargs, B, T, S, context from features?, step_idx given?)
SHAPES = [
    (dict(hidden=224, heads=7, attn_window_size=64), 2, 70, 37, False, True),
    (dict(hidden=100, heads=4, n_mels=100, semantic_dim=24, attn_window_size=None), 2, 33, 17, True, False),
    (dict(hidden=96, heads=4, attn_window_size=5, ffn_mult=3, use_adaln=False), 3, 50, 25, False, True),
    (dict(hidden=256, heads=2), 2, 64, 31, False, True),
    (dict(hidden=50, heads=5, n_mels=45, semantic_dim=7, layers=2, attn_window_size=3), 2, 19, 9, True, True),
]


@pytest.mark.parametrize("kw, B, T, S, feats, with_step", SHAPES, ids=lambda v: str(v) if isinstance(v, dict) else None)
def test_forward_vs_oracle_on_shapes_without_instance(kw, B, T, S, feats, with_step):
    cfg = CFG(device=DEV, **kw)
    dec, sd = make(cfg)
    g = torch.Generator().manual_seed(B * 1000 + T)
    x = torch.randn(B, T, cfg.n_mels, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    si = torch.randint(0, 16, (B,), generator=g) if with_step else None
    sem = None if feats else torch.randint(0, cfg.codebook_size, (B, S), generator=g)
    f = torch.randn(B, S, cfg.semantic_dim, generator=g) if feats else None
    eps = dec(cu(x), cu(t), cu(sem), cu(si), cu(f)).cpu()
    ref = O.decoder_forward(sd, x, t, sem, si, f, heads=cfg.heads, window=cfg.attn_window_size)
    err = max_abs(eps, ref)
    print(f"generic forward {kw}: max-abs {err:.2e} (|ref| max {float(ref.abs().max()):.2f})")
    assert eps.shape == ref.shape and err < FWD_TOL, err
    assert float(ref.abs().max()) > 0.1  # a real signal, not a degenerate all-zero comparison


@pytest.mark.parametrize("hidden, heads", [(160, 4), (256, 8)])
def test_generic_matches_fused(hidden, heads):
    cfg = CFG(device=DEV, hidden=hidden, heads=heads)
    fused, _ = make(cfg, "compiled")
    gen, _ = make(cfg, "generic")
    g = torch.Generator().manual_seed(hidden)
    B, T, S = 3, 75, 41
    x = torch.randn(B, T, 80, generator=g).to(DEV)
    t = torch.randint(0, 1000, (B,), generator=g).to(DEV)
    si = torch.randint(0, 16, (B,), generator=g).to(DEV)
    sem = torch.randint(0, cfg.codebook_size, (B, S), generator=g).to(DEV)
    assert max_abs(gen(x, t, sem, si), fused(x, t, sem, si)) < FWD_TOL


def test_generic_matches_fused_full_size():
    """B=256, T=512 (131072 rows): catches 32-bit index overflow in the generic kernels."""
    cfg = CFG(device=DEV)
    fused, _ = make(cfg, "compiled")
    gen, _ = make(cfg, "generic")
    g = torch.Generator().manual_seed(7)
    B, T, S = 256, 512, 256
    x = torch.randn(B, T, 80, generator=g).to(DEV)
    t = torch.randint(0, 1000, (B,), generator=g).to(DEV)
    si = torch.randint(0, 16, (B,), generator=g).to(DEV)
    sem = torch.randint(0, cfg.codebook_size, (B, S), generator=g).to(DEV)
    a = gen(x, t, sem, si)
    b = fused(x, t, sem, si)
    err = float((a - b).abs().max())
    assert bool(torch.isfinite(a).all()) and err < FWD_TOL, err
    # per-utterance rows really differ (every row was computed, none left over from another)
    assert float((a[-1] - a[0]).abs().max()) > 0.1


def _infer(cfg, dec, diff_steps=None):
    return EdgeInference(cfg, DiffusionSchedule(diff_steps or cfg.diff_steps).to(DEV), torch.nn.Identity(), dec)


@pytest.mark.parametrize("kw", [dict(hidden=224, heads=7), dict(hidden=50, heads=5, n_mels=45, semantic_dim=7, layers=2)])
def test_generate_mel_vs_oracle(kw):
    cfg = CFG(device=DEV, **kw)
    dec, sd = make(cfg)
    g = torch.Generator().manual_seed(11)
    B, S = 2, 29
    sem = torch.randint(0, cfg.codebook_size, (B, S), generator=g)
    x_T = torch.randn(B, 2 * S, cfg.n_mels, generator=g)
    out = _infer(cfg, dec).generate_mel(cu(sem), 4, x_T=cu(x_T)).cpu()
    tr = []
    ref = O.generate_mel(sd, O.schedule_tables(1000)["alpha_bar"], sem, x_T, 4, heads=cfg.heads, window=cfg.attn_window_size, trace=tr)
    e2e_check(out, ref, amplification_band(x_T, tr[0]["eps"]), f"generic generate_mel {kw}")


def test_sample_ddpm_vs_oracle():
    cfg = CFG(device=DEV, hidden=96, heads=4, attn_window_size=5, ffn_mult=3, diff_steps=50)
    dec, sd = make(cfg)
    infer = _infer(cfg, dec)
    g = torch.Generator().manual_seed(3)
    B, S, n = 2, 21, 6
    sem = torch.randint(0, cfg.codebook_size, (B, S), generator=g)
    x_T = torch.randn(B, 2 * S, 80, generator=g)
    noise = torch.randn(n, B, 2 * S, 80, generator=g)
    out = infer.sample_ddpm(cu(sem), n, x_T=cu(x_T), noise=cu(noise)).cpu()
    ref = O.sample_ddpm(sd, O.schedule_tables(50), sem, x_T, noise, n, heads=cfg.heads, window=cfg.attn_window_size)
    scale = float(ref.abs().max())
    assert bool(torch.isfinite(out).all()) and max_abs(out, ref) < 2e-4 * max(scale, 1.0), (max_abs(out, ref), scale)
    # in-kernel Philox noise on an odd element count (scalar tail path): deterministic per seed
    cfg2 = CFG(device=DEV, hidden=50, heads=5, n_mels=45, semantic_dim=7, layers=2, diff_steps=50)
    inf2 = _infer(cfg2, make(cfg2)[0])
    s2 = torch.randint(0, cfg2.codebook_size, (3, 7), generator=g).to(DEV)
    x2 = torch.randn(3, 14, 45, generator=g).to(DEV)
    a, b = inf2.sample_ddpm(s2, 3, x_T=x2, seed=5), inf2.sample_ddpm(s2, 3, x_T=x2, seed=5)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and not torch.equal(a, inf2.sample_ddpm(s2, 3, x_T=x2, seed=6))


def test_dpm_solver_pp_order2_vs_oracle():
    from edge_diffusion_tts_amd import DPMSolverPP
    cfg = CFG(device=DEV, hidden=100, heads=4, n_mels=100, semantic_dim=24, attn_window_size=None)
    dec, sd = make(cfg)
    sch = DiffusionSchedule(cfg.diff_steps).to(DEV)
    g = torch.Generator().manual_seed(5)
    x_T = torch.randn(2, 40, 100, generator=g)
    f = torch.randn(2, 20, 24, generator=g)
    out = DPMSolverPP(sch, order=2).sample(dec, cu(x_T), cu(f), num_steps=5, max_t=950).cpu()
    ref = O.dpmpp_sample(sd, O.schedule_tables(1000), x_T, f, 5, order=2, max_t=950, heads=cfg.heads, window=None)
    assert max_abs(out, ref) < FWD_TOL, max_abs(out, ref)


def test_inpaint_with_guidance_vs_oracle():
    from edge_diffusion_tts_amd import InpaintSampler
    cfg = CFG(device=DEV, hidden=100, heads=4, n_mels=100, semantic_dim=24, attn_window_size=16)
    dec, sd = make(cfg)
    smp = InpaintSampler(cfg, DiffusionSchedule(cfg.diff_steps).to(DEV), dec)
    g = torch.Generator().manual_seed(8)
    B, T, S, ov, n = 2, 48, 24, 7, 4
    f = torch.randn(B, S, 24, generator=g)
    known = torch.randn(B, ov, 100, generator=g)
    x_coarse = torch.randn(B, T, 100, generator=g)
    noise = torch.randn(B, T, 100, generator=g)
    noise_k = torch.randn(n, B, ov, 100, generator=g)
    out = smp.inpaint_teacher_refine(cu(x_coarse), cu(f), cu(known), ov, 0.5, n, 1.5, noise=cu(noise), noise_k=cu(noise_k)).cpu()
    ref = O.inpaint_teacher_refine(sd, O.schedule_tables(1000), x_coarse, f, noise, known, ov, 0.5, n, 1.5, noise_k,
                                   heads=cfg.heads, window=cfg.attn_window_size)
    assert max_abs(out, ref) < 5e-4, max_abs(out, ref)
    assert torch.equal(out[:, :ov], known)


@pytest.mark.parametrize("kw", [dict(hidden=224, heads=7), dict(hidden=50, heads=5, n_mels=45, semantic_dim=7, layers=2)])
def test_sampler_tail_is_the_stepwise_update_bitwise(kw):
    """Fused-loop generate_mel == decoder.forward + DiffusionSchedule.get_ddim_step step by step, bitwise (the tail kernel runs the
    same per-element DDIM helper as the standalone update)."""
    cfg = CFG(device=DEV, **kw)
    dec, _ = make(cfg)
    infer = _infer(cfg, dec)
    g = torch.Generator().manual_seed(4)
    B, S = 3, 13
    sem = torch.randint(0, cfg.codebook_size, (B, S), generator=g).to(DEV)
    x = torch.randn(B, 2 * S, cfg.n_mels, generator=g).to(DEV)
    one = infer.generate_mel(sem, 1, x_T=x)
    tt = torch.full((B,), 999, device=DEV)
    _, x0 = infer.schedule.get_ddim_step(x, tt, torch.full((B,), 0, device=DEV), dec(x, tt, sem, torch.zeros(B, dtype=torch.long, device=DEV)))
    assert torch.equal(one, x0)
    fused = infer.generate_mel(sem, 4, x_T=x)
    for i, t in enumerate([999, 749, 499, 249]):
        tt = torch.full((B,), t, device=DEV)
        eps = dec(x, tt, sem, torch.full((B,), i, device=DEV))
        x, x0 = infer.schedule.get_ddim_step(x, tt, torch.full((B,), max(t - 250, 0), device=DEV), eps)
    assert torch.equal(fused, x0)


def test_deterministic_batch_invariant_and_graph_capturable():
    cfg = CFG(device=DEV, hidden=224, heads=7)
    dec, _ = make(cfg)
    infer = _infer(cfg, dec)
    g = torch.Generator().manual_seed(9)
    B, S = 6, 45
    sem = torch.randint(0, cfg.codebook_size, (B, S), generator=g).to(DEV)
    x = torch.randn(B, 2 * S, 80, generator=g).to(DEV)
    a = infer.generate_mel(sem, 4, x_T=x)
    assert torch.equal(a, infer.generate_mel(sem, 4, x_T=x))
    solo = infer.generate_mel(sem[4:5].contiguous(), 4, x_T=x[4:5].contiguous())
    assert torch.equal(solo[0], a[4])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = infer.generate_mel(sem, 4, x_T=x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_g, a)


def test_mode_selection_and_index_errors():
    g = torch.Generator().manual_seed(2)
    B, S = 2, 20
    for kw, same_as in ((dict(), "compiled"), (dict(hidden=224, heads=7), "generic")):
        cfg = CFG(device=DEV, **kw)
        auto, _ = make(cfg, "auto")
        ref, _ = make(cfg, same_as)
        sem = torch.randint(0, cfg.codebook_size, (B, S), generator=g).to(DEV)
        x = torch.randn(B, 2 * S, 80, generator=g).to(DEV)
        assert torch.equal(_infer(cfg, auto).generate_mel(sem, 4, x_T=x), _infer(cfg, ref).generate_mel(sem, 4, x_T=x)), kw
    cfg = CFG(device=DEV, hidden=224, heads=7)
    dec, _ = make(cfg)
    x = torch.zeros(1, 32, 80, device=DEV)
    t = torch.tensor([5], device=DEV)
    bad = torch.zeros(1, 16, dtype=torch.long, device=DEV)
    bad[0, 3] = cfg.codebook_size
    old = native.CHECK_INDICES
    native.CHECK_INDICES = True
    try:
        with pytest.raises(IndexError, match="sem_idx"):
            dec(x, t, bad, None)
        with pytest.raises(IndexError, match="step_idx"):
            dec(x, t, torch.zeros_like(bad), torch.tensor([16], device=DEV))
    finally:
        native.CHECK_INDICES = old
    # the compiled mode still refuses the shape (unchanged behaviour)
    with pytest.raises(native.EdttsError, match="192/6/80"):
        make(cfg, "compiled")[0](x, t, torch.zeros_like(bad), None)


def test_library_noise_for_unaligned_shapes():
    """native.randn on element counts / offsets that are not multiples of 4 (n_mels = 45) draws the same per-element values as an
    aligned call over the same global elements."""
    full = native.randn((3 * 14 * 45,), DEV, seed=4, elem_offset=0)
    part = native.randn((1, 14, 45), DEV, seed=4, elem_offset=14 * 45)
    assert torch.equal(part.flatten(), full[14 * 45: 2 * 14 * 45])
