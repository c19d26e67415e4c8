"""In-painting with DPM-Solver++ on the GPU: InpaintSampler.inpaint_dpm_refine against a composition of the
oracle's own functions on every kernel family, and its bitwise properties -- equal to the multistep sampler when nothing is
injected or guided, deterministic, row b of a ragged batch equal to the call on utterance b alone, capturable, and
generate_long_batch(solver="dpmpp") equal to generate_long per utterance.  Run on the GPU box: python -m pytest tests -m gpu."""
import pytest
import torch

from conftest import max_abs
from edge_diffusion_tts_amd import CFG, DiffusionSchedule, DPMSolverPP, EdgeDiffusionDecoder, InpaintSampler, native, synth_state_dict
from oracle import edtts_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, T, S, OV, STEPS, STRENGTH = 3, 41, 20, 5, 5, 0.5
# the bar test_gpu_parity.py holds DPMSolverPP.sample to against the oracle (FWD_TOL); its bar for inpaint_teacher_refine, 5e-4, is the
# wider of the two, so a result inside this one meets both
TOL = 1e-4

CONFIGS = {
    "32/2/80": (dict(hidden=32, heads=2), {}),
    "160/4/80": ({}, {}),
    "generic 50/5/45": (dict(hidden=50, heads=5, n_mels=45, semantic_dim=7, layers=2), dict(kernels="generic")),
    "bf16 64/2/80": (dict(hidden=64, heads=2), dict(compute_dtype="bf16")),
}
_made, _refs = {}, {}


def make(name):
    """(sampler, the decoder's state dict on the CPU, cfg); one per configuration for the whole module."""
    if name not in _made:
        ckw, dkw = CONFIGS[name]
        cfg = CFG(device=DEV, **ckw)
        dec = EdgeDiffusionDecoder(cfg, **dkw)
        sd = synth_state_dict(cfg, 0, max_pos=dec.max_len, max_ctx_pos=dec.max_context_len)
        dec.load_state_dict(sd)
        dec = dec.to(DEV).eval()
        _made[name] = (InpaintSampler(cfg, DiffusionSchedule(cfg.diff_steps).to(DEV), dec), sd, cfg)
    return _made[name]


def inputs(cfg, seed=3):
    g = torch.Generator().manual_seed(seed)
    return dict(x_coarse=torch.randn(B, T, cfg.n_mels, generator=g).clamp(-3, 3), sem=torch.randn(B, S, cfg.semantic_dim, generator=g),
                known=torch.randn(B, OV, cfg.n_mels, generator=g), noise=torch.randn(B, T, cfg.n_mels, generator=g),
                noise_k=torch.randn(STEPS, B, OV, cfg.n_mels, generator=g))


def oracle_dpm(sd, cfg, d, order, scale, *, known=True, step_idx=0, dtype=torch.float32, rows=slice(None)):
    """inpaint_dpm_refine composed from the oracle's functions (CPU): the start point and the per-step blend of its
    inpaint_teacher_refine / inpaint_loop, the guidance combine of inpaint_loop, the times of dpmpp_timesteps and the x0 / update
    expressions as dpmpp_sample has them.  dtype float64: the arbiter run (fp64 weights, tables and arithmetic, the fp32 run's times)."""
    tabs32 = O.schedule_tables(cfg.diff_steps)
    tabs = tabs32 if dtype == torch.float32 else O.schedule_tables(cfg.diff_steps, dtype)
    sd = sd if dtype == torch.float32 else O.cast_sd(sd, dtype)
    a_t, s_t, lam = tabs["sqrt_alpha_bar"], tabs["sqrt_one_minus_alpha_bar"], tabs["lambda_t"]
    kw = dict(heads=cfg.heads, window=cfg.attn_window_size)
    t_start = int(cfg.diff_steps * STRENGTH)
    ts = O.dpmpp_timesteps(tabs32["lambda_t"], STEPS, t_start)
    x_coarse, sem, noise = d["x_coarse"][rows].to(dtype), d["sem"][rows].to(dtype), d["noise"][rows].to(dtype)
    known_mel, noise_k = d["known"][rows].to(dtype), d["noise_k"][:, rows].to(dtype)
    n = x_coarse.shape[0]
    x = a_t[t_start] * x_coarse + s_t[t_start] * noise
    x0_hist, t_hist = [], []
    for i, t in enumerate(ts):
        tt = torch.full((n,), t, dtype=torch.long)
        si = torch.full((n,), i if step_idx == "index" else step_idx, dtype=torch.long)
        if known:
            x[:, :OV] = a_t[t] * known_mel + s_t[t] * noise_k[i]
        v = O.decoder_forward(sd, x, tt, None, si, sem, **kw)
        if scale != 1.0:
            vu = O.decoder_forward(sd, x, tt, None, si, torch.zeros_like(sem), **kw)
            v = vu + scale * (v - vu)
        x0 = torch.clamp(a_t[t] * x - s_t[t] * v, -3, 3)
        tp = ts[i + 1] if i < len(ts) - 1 else 0
        h = lam[tp] - lam[t]
        if order == 1 or len(x0_hist) == 0:
            x = (s_t[tp] / s_t[t]) * x + a_t[tp] * (1 - torch.exp(-h)) * x0
        elif order == 2 or len(x0_hist) == 1:
            r = (lam[t_hist[-1]] - lam[tp]) / h
            d1 = (1 / r) * (x0 - x0_hist[-1])
            x = (s_t[tp] / s_t[t]) * x + a_t[tp] * (1 - torch.exp(-h)) * x0 + a_t[tp] * ((1 - torch.exp(-h)) / h + 1) * d1 * 0.5
        else:
            p = [x0] + x0_hist[-2:]
            d1 = p[0] - p[1]
            d2 = p[0] - 2 * p[1] + p[2]
            x = ((s_t[tp] / s_t[t]) * x + a_t[tp] * (1 - torch.exp(-h)) * p[0] + a_t[tp] * ((1 - torch.exp(-h)) / h + 1) * d1 * 0.5
                 + a_t[tp] * ((1 - torch.exp(-h)) / (h ** 2) + 0.5 / h + 0.5) * d2 / 6)
        x0_hist, t_hist = (x0_hist + [x0])[-2:], (t_hist + [tp])[-2:]
    if known:
        x[:, :OV] = known_mel
    return x


def reference(name, order, scale, rows=slice(None)):
    """The fp32 oracle run of a case: computed once, shared by the tests that need it, never written to."""
    key = (name, order, scale, str(rows))
    if key not in _refs:
        smp, sd, cfg = make(name)
        _refs[key] = oracle_dpm(sd, cfg, inputs(cfg), order, scale, rows=rows)
    return _refs[key]


def run(smp, d, order, scale, rows=slice(None), **kw):
    cu = lambda t: t[rows].to(DEV).contiguous()
    return smp.inpaint_dpm_refine(cu(d["x_coarse"]), cu(d["sem"]), cu(d["known"]), OV, STRENGTH, STEPS, order, scale, noise=cu(d["noise"]),
                                  noise_k=d["noise_k"][:, rows].to(DEV).contiguous(), **kw)


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("scale", [1.0, 1.5])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_parity_fused_fp32(order, scale):
    smp, sd, cfg = make("32/2/80")
    d = inputs(cfg)
    out = run(smp, d, order, scale).cpu()
    ref = reference("32/2/80", order, scale)
    err = max_abs(out, ref)
    print(f"inpaint_dpm_refine 32/2/80 order {order} cfg {scale}: max-abs {err:.2e} vs the oracle composition")
    assert err < TOL
    assert torch.equal(out[:, :OV], d["known"])


def test_parity_generic_scalar_tail():
    smp, sd, cfg = make("generic 50/5/45")
    d = inputs(cfg)
    for order, scale in ((2, 1.5), (3, 1.0)):
        out = run(smp, d, order, scale).cpu()
        err = max_abs(out, reference("generic 50/5/45", order, scale))
        print(f"inpaint_dpm_refine generic 50/5/45 order {order} cfg {scale}: max-abs {err:.2e}")
        assert err < TOL
        assert torch.equal(out[:, :OV], d["known"])


def test_parity_cooperative_b1():
    """B = 1, T = 41 on the default decoder: two 32-frame tiles, far fewer than SIMDs / 8 -- the cooperative 16-frame instance."""
    smp, sd, cfg = make("160/4/80")
    d = inputs(cfg)
    old = native.set_coop(-1)
    try:
        out = run(smp, d, 2, 1.5, rows=slice(0, 1)).cpu()
        native.set_coop(0)
        forced_off = run(smp, d, 2, 1.5, rows=slice(0, 1)).cpu()
    finally:
        native.set_coop(old)
    err = max_abs(out, reference("160/4/80", 2, 1.5, rows=slice(0, 1)))
    print(f"inpaint_dpm_refine 160/4/80 B=1 (cooperative) order 2 cfg 1.5: max-abs {err:.2e}")
    assert err < TOL
    assert torch.equal(out, forced_off)  # the cooperative and the per-wave kernels: the same bits


def test_parity_under_two_substreams():
    """native.set_substreams(2) at the smallest batch that the cutting samplers then cut.  The in-painting samplers run their batch in
    one piece on the caller's stream (the guided pass shares x with the conditional one), so the setting must not change a bit; the
    batch is the three-utterance case repeated, and so is its reference."""
    smp, sd, cfg = make("32/2/80")
    d = inputs(cfg)
    old = native.set_substreams(2)
    try:
        dims = smp.decoder.dims()
        big = next(b for b in range(2, 1 << 14) if native.substreams_for(dims, b, T) >= 2)
        assert native.substreams_for(dims, big - 1, T) == 1
        rep = -(-big // B)
        tile = lambda t, dim=0: torch.cat([t] * rep, dim=dim).narrow(dim, 0, big).to(DEV).contiguous()
        out = smp.inpaint_dpm_refine(tile(d["x_coarse"]), tile(d["sem"]), tile(d["known"]), OV, STRENGTH, STEPS, 2, 1.0,
                                     noise=tile(d["noise"]), noise_k=tile(d["noise_k"], 1)).cpu()
    finally:
        native.set_substreams(old)
    ref = torch.cat([reference("32/2/80", 2, 1.0)] * rep)[:big]
    err = max_abs(out, ref)
    print(f"inpaint_dpm_refine 32/2/80 B={big} under set_substreams(2): max-abs {err:.2e}")
    assert err < TOL
    assert torch.equal(out[:B], run(smp, d, 2, 1.0).cpu())
    assert native.set_substreams(old) == old


def test_parity_bf16_against_the_first_order_sampler():
    """The bf16 instance carries its rounding through the same number of decoder passes in both samplers, and the update behind it
    is fp32 in both: its error against the fp32 oracle may be no larger than 1.5 x that of inpaint_teacher_refine at the same shape
    and step count, measured here."""
    smp, sd, cfg = make("bf16 64/2/80")
    d = inputs(cfg)
    cu = lambda t: t.to(DEV).contiguous()
    err_new = max_abs(run(smp, d, 2, 1.5).cpu(), reference("bf16 64/2/80", 2, 1.5))
    old = smp.inpaint_teacher_refine(cu(d["x_coarse"]), cu(d["sem"]), cu(d["known"]), OV, STRENGTH, STEPS, 1.5, noise=cu(d["noise"]),
                                     noise_k=cu(d["noise_k"])).cpu()
    ref_old = O.inpaint_teacher_refine(sd, O.schedule_tables(cfg.diff_steps), d["x_coarse"], d["sem"], d["noise"], d["known"], OV, STRENGTH,
                                       STEPS, 1.5, d["noise_k"], heads=cfg.heads, window=cfg.attn_window_size)
    err_old = max_abs(old, ref_old)
    print(f"bf16 64/2/80, {STEPS} steps, cfg 1.5: inpaint_dpm_refine {err_new:.3e}, inpaint_teacher_refine {err_old:.3e} vs the fp32 oracle")
    assert err_new <= 1.5 * err_old


# ------------------------------------------------------------------------------------------------ bitwise properties
@pytest.mark.parametrize("name, orders", [("32/2/80", (1, 2, 3)), ("generic 50/5/45", (2, 3))])
def test_equals_the_multistep_sampler(name, orders):
    smp, sd, cfg = make(name)
    d = inputs(cfg)
    cu = lambda t: t.to(DEV).contiguous()
    t_start = int(cfg.diff_steps * STRENGTH)
    x_T = smp._refine_start(cu(d["x_coarse"]), t_start, cu(d["noise"]), 0, None)
    for order in orders:
        out, x0s = smp.inpaint_dpm_refine(cu(d["x_coarse"]), cu(d["sem"]), None, 0, STRENGTH, STEPS, order, 1.0, noise=cu(d["noise"]),
                                          step_idx="index", return_intermediates=True)
        want, want_x0s = DPMSolverPP(smp.schedule, order=order).sample(smp.decoder, x_T, cu(d["sem"]), num_steps=STEPS, max_t=t_start,
                                                                       return_intermediates=True)
        assert torch.equal(out, want), (name, order, max_abs(out.cpu(), want.cpu()))
        assert len(x0s) == STEPS and all(torch.equal(a, b) for a, b in zip(x0s, want_x0s)), (name, order)


def test_deterministic():
    smp, sd, cfg = make("32/2/80")
    d = inputs(cfg)
    assert torch.equal(run(smp, d, 3, 1.5), run(smp, d, 3, 1.5))
    cu = lambda t: t.to(DEV).contiguous()
    lib = [smp.inpaint_dpm_refine(cu(d["x_coarse"]), cu(d["sem"]), cu(d["known"]), OV, STRENGTH, STEPS, 2, 1.5, seed=11) for _ in range(2)]
    assert torch.equal(lib[0], lib[1]) and bool(torch.isfinite(lib[0]).all()) and torch.equal(lib[0][:, :OV].cpu(), d["known"])
    other = smp.inpaint_dpm_refine(cu(d["x_coarse"]), cu(d["sem"]), cu(d["known"]), OV, STRENGTH, STEPS, 2, 1.5, seed=12)
    assert not torch.equal(lib[0], other)


def nan_past(x, n):
    x = x.clone()
    for b, k in enumerate(n):
        x[b, k:] = float("nan")
    return x


@pytest.mark.parametrize("name", ["32/2/80", "160/4/80", "generic 50/5/45", "bf16 64/2/80"])
def test_ragged_rows_equal_their_solo_calls(name):
    smp, sd, cfg = make(name)
    d = inputs(cfg)
    tl, sl, seeds = [41, 33, 7], [20, 16, 3], [5, 2 ** 40 + 1, 77]
    x = nan_past(d["x_coarse"], tl).to(DEV)
    f = nan_past(d["sem"], sl).to(DEV)
    kn = d["known"].to(DEV)
    for order, scale in ((2, 1.5), (3, 1.0)):
        out = smp.inpaint_dpm_refine(x, f, kn, OV, STRENGTH, STEPS, order, scale, x_lengths=torch.tensor(tl), sem_lengths=torch.tensor(sl),
                                     seeds=seeds)
        assert native.index_errors(smp.decoder.workspace(B, T, S, STEPS, x.device)) == 0
        for b in range(B):
            solo = smp.inpaint_dpm_refine(x[b:b + 1, :tl[b]].contiguous(), f[b:b + 1, :sl[b]].contiguous(), kn[b:b + 1], OV, STRENGTH, STEPS,
                                          order, scale, seed=seeds[b])
            assert torch.equal(out[b, :tl[b]], solo[0]), (name, order, scale, b, max_abs(out[b, :tl[b]].cpu(), solo[0].cpu()))
            assert bool((out[b, tl[b]:] == 0).all()), (name, b, "nonzero past the length")
            assert torch.equal(out[b, :OV], kn[b])


def test_overlap_longer_than_a_row():
    smp, sd, cfg = make("32/2/80")
    d = inputs(cfg)
    cu = lambda t: t.to(DEV).contiguous()
    short = [41, 3, 20]
    with pytest.raises(ValueError, match="overlap_len = 5"):
        smp.inpaint_dpm_refine(cu(d["x_coarse"]), cu(d["sem"]), cu(d["known"]), OV, STRENGTH, STEPS, 2, 1.0, x_lengths=torch.tensor(short),
                               seeds=[1, 2, 3])
    ws = smp.decoder.workspace(B, T, S, STEPS, torch.device(DEV, 0))
    native.index_errors(ws)  # clear
    kn = d["known"].clone()
    kn[1, 3:] = float("nan")  # the known frames the short row does not have: never read
    out = smp.inpaint_dpm_refine(nan_past(d["x_coarse"], short).to(DEV), cu(d["sem"]), kn.to(DEV), OV, STRENGTH, STEPS, 2, 1.5,
                                 x_lengths=torch.tensor(short, device=DEV), seeds=[1, 2, 3])
    torch.cuda.synchronize()
    assert native.index_errors(ws) & native.EDTTS_IDX_LEN
    assert bool(torch.isfinite(out).all()) and bool((out[1, 3:] == 0).all()) and bool((out[2, 20:] == 0).all())
    assert torch.equal(out[1, :3].cpu(), d["known"][1, :3])  # the final force of the frames it has
    assert torch.equal(out[0, :OV].cpu(), d["known"][0])


def test_graph_capture_replays_the_eager_result():
    smp, sd, cfg = make("160/4/80")
    d = inputs(cfg)
    cu = lambda t: t.to(DEV).contiguous()
    x, f, kn, nz = cu(d["x_coarse"]), cu(d["sem"]), cu(d["known"]), cu(d["noise"])
    mixes = [([41, 33, 7], [20, 16, 3]), ([9, 41, 30], [4, 20, 11])]
    tl_dev, sl_dev = torch.tensor(mixes[0][0], device=DEV), torch.tensor(mixes[0][1], device=DEV)
    sd_dev = native.seed_tensor([5, 6, 7], B, DEV)

    def call(tl, sl):
        return smp.inpaint_dpm_refine(x, f, kn, OV, STRENGTH, STEPS, 2, 1.5, noise=nz, x_lengths=tl, sem_lengths=sl, seeds=sd_dev)
    eager = [call(torch.tensor(a), torch.tensor(b)) for a, b in mixes]
    call(tl_dev, sl_dev)  # warm-up with the device tensors
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        static_out = call(tl_dev, sl_dev)
    for (a, b), e in zip(mixes, eager):
        tl_dev.copy_(torch.tensor(a))
        sl_dev.copy_(torch.tensor(b))
        static_out.fill_(7.0)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, e)
    del gr
    smp.decoder.release_pinned()


# ------------------------------------------------------------------------------------------------ long-form
HOP, SR = 160, 16000


def test_generate_long_batch_dpmpp_is_generate_long_per_utterance():
    smp, sd, cfg = make("160/4/80")
    rows, totals = (40, 60, 25), (70, 110, 41)  # 2, 3 and 1 chunks of 41 frames, 5 of them shared with the previous chunk
    g = torch.Generator().manual_seed(41)
    feats = [torch.randn(1, r, cfg.semantic_dim, generator=g).to(DEV) for r in rows]
    stats = [[(torch.randn(1, 1, cfg.n_mels, generator=g).to(DEV) * 0.1, (torch.rand(1, 1, cfg.n_mels, generator=g) + 0.5).to(DEV))
              for _ in range(InpaintSampler.chunk_plan(t, T, OV, HOP)[0])] for t in totals]
    assert [len(s) for s in stats] == [2, 3, 1]
    seeds = [5, 2 ** 40, 99]
    kw = dict(strength=0.6, steps=STEPS, cfg_scale=1.5, hop_length=HOP, sample_rate=SR)
    out = smp.generate_long_batch(feats, totals, T, OV, stats, seeds=seeds, solver="dpmpp", order=2, **kw)
    for n in range(3):
        alone = smp.generate_long(feats[n], totals[n], T, OV, stats[n], seed=seeds[n], solver="dpmpp", order=2, **kw)
        assert out[n].shape == alone.shape == (cfg.n_mels, totals[n])
        assert torch.equal(out[n], alone), (n, max_abs(out[n].cpu(), alone.cpu()))
        assert bool(torch.isfinite(out[n]).all()) and float(out[n].min()) >= 0.0
    plain = smp.generate_long_batch(feats, totals, T, OV, stats, seeds=seeds, **kw)
    ddim = smp.generate_long_batch(feats, totals, T, OV, stats, seeds=seeds, solver="ddim", **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, ddim))
    assert not torch.equal(plain[0], out[0])  # (the other solver is really another sampler)
