"""Batched long-form synthesis on the GPU: every row of a ragged, per-row-seeded in-painting call is bitwise
the call on that utterance alone, on every kernel family; padding is never read and outputs past the lengths are exact zeros;
the defaults are unchanged; the lengths are read at run time (graph replay); and generate_long_batch gives each utterance bitwise
its generate_long.  Run on the GPU box: python -m pytest tests -m gpu."""
import pytest
import torch

from conftest import max_abs
from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, InpaintSampler, native, synth_state_dict
from edge_diffusion_tts_amd.longform import linspace_times

pytestmark = pytest.mark.gpu
DEV = "cuda"
OV = 12


def make(cfg, seed=0, **kw):
    dec = EdgeDiffusionDecoder(cfg, **kw)
    sd = synth_state_dict(cfg, seed, max_pos=dec.max_len, max_ctx_pos=dec.max_context_len)
    dec.load_state_dict(sd)
    dec = dec.to(DEV).eval()
    return InpaintSampler(cfg, DiffusionSchedule(cfg.diff_steps).to(DEV), dec)


def lens(B, full, seed, lo=1):
    """Lengths in [lo, full] that include lo, the maximum and values that are not multiples of 16 or 32 (test_ragged_gpu.lens)."""
    fixed = [lo, full, max(lo, full - 17), min(full, max(lo, 33)), max(lo, full // 2 + 5)]
    g = torch.Generator().manual_seed(seed)
    extra = torch.randint(lo, full + 1, (max(0, B - len(fixed)),), generator=g).tolist()
    return torch.tensor((fixed + extra)[:B], dtype=torch.int64)


def nan_past(x, n):
    x = x.clone()
    for b, k in enumerate(n.tolist()):
        x[b, k:] = float("nan")
    return x


def inputs(cfg, B, T, S, seed, known):
    g = torch.Generator().manual_seed(seed)
    tl = lens(B, T, seed, lo=OV if known else 1)
    sl = lens(B, S, seed + 1)
    x = nan_past(torch.randn(B, T, cfg.n_mels, generator=g), tl).to(DEV)
    f = nan_past(torch.randn(B, S, cfg.semantic_dim, generator=g), sl).to(DEV)
    kn = torch.randn(B, OV, cfg.n_mels, generator=g).to(DEV) if known else None
    seeds = [1000 * seed + 7 * b + 3 for b in range(B)]
    return x, f, kn, tl, sl, seeds


def assert_rows(out, solo_of, n, what):
    for b, k in enumerate(n.tolist()):
        solo = solo_of(b)
        assert solo.shape[1] == k
        assert torch.equal(out[b, :k], solo[0]), (what, b, k, max_abs(out[b, :k].cpu(), solo[0].cpu()))
        assert bool((out[b, k:] == 0).all()), (what, b, "nonzero past the length")


def check_teacher(smp, cfg, B, T, S, seed, known, scale, steps=3):
    x, f, kn, tl, sl, seeds = inputs(cfg, B, T, S, seed, known)
    ov = OV if known else 0
    out = smp.inpaint_teacher_refine(x, f, kn, ov, 0.5, steps, scale, x_lengths=tl, sem_lengths=sl, seeds=seeds)
    assert native.index_errors(smp.decoder.workspace(B, T, S, steps, x.device)) == 0

    def solo(b):
        k, s = int(tl[b]), int(sl[b])
        return smp.inpaint_teacher_refine(x[b:b + 1, :k], f[b:b + 1, :s], None if kn is None else kn[b:b + 1], ov, 0.5, steps, scale,
                                          seed=seeds[b])
    assert_rows(out, solo, tl, ("teacher", known, scale))


def check_student(smp, cfg, B, T, S, seed, known, steps=3):
    _, f, kn, tl, sl, seeds = inputs(cfg, B, T, S, seed, known)
    ov = OV if known else 0
    out = smp.inpaint_student_sample((B, T, cfg.n_mels), f, kn, ov, steps, x_lengths=tl, sem_lengths=sl, seeds=seeds)

    def solo(b):
        k, s = int(tl[b]), int(sl[b])
        return smp.inpaint_student_sample((1, k, cfg.n_mels), f[b:b + 1, :s], None if kn is None else kn[b:b + 1], ov, steps,
                                          seed=seeds[b])
    assert_rows(out, solo, tl, ("student", known))


def check_all(smp, cfg, B, T, S, seed):
    for known in (False, True):
        check_student(smp, cfg, B, T, S, seed, known)
        for scale in (1.0, 2.5):
            check_teacher(smp, cfg, B, T, S, seed + 1, known, scale)


@pytest.mark.parametrize("B", [6, 80])  # 80 x 7 tiles of 32 frames: the 32-frame instance; 6: the 16-frame one
def test_solo_equality_fused_per_wave(B):
    smp = make(CFG(device=DEV))
    old = native.set_coop(0)
    try:
        check_all(smp, smp.cfg, B, 200, 100, seed=B)
    finally:
        native.set_coop(old)


def test_solo_equality_32_2_80():
    """The instance whose in-painting tail used to reserve 68 B/lane of private segment with lengths."""
    cfg = CFG(device=DEV, hidden=32, heads=2)
    check_all(make(cfg), cfg, 6, 200, 100, seed=32)


@pytest.mark.parametrize("B, inst", [(3, 14), (20, 24), (40, 22)])
def test_solo_equality_cooperative_automatic(B, inst):
    """Automatic mode at T = 200 (7 tiles of 32 frames per utterance on 1 024 SIMDs): B = 3 runs the 16-frame 4-wave instance, 20 the
    32-frame 4-wave one, 40 the 32-frame 2-wave one (what a 64-utterance long-form batch runs on); the solo calls run the first."""
    smp = make(CFG(device=DEV))
    old = native.set_coop(-1)
    try:
        simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
        t32 = B * 7
        want = 14 if 8 * t32 <= simds else (24 if 4 * t32 <= simds else (22 if 2 * t32 <= simds else 0))
        if simds == 1024:
            assert want == inst
        check_all(smp, smp.cfg, B, 200, 100, seed=B)
    finally:
        native.set_coop(old)


def test_solo_equality_bf16():
    cfg = CFG(device=DEV, hidden=64, heads=2)
    check_all(make(cfg, compute_dtype="bf16"), cfg, 5, 160, 80, seed=64)


@pytest.mark.parametrize("kw", [dict(hidden=100, heads=4, n_mels=100, semantic_dim=24),              # vector inject
                                dict(hidden=50, heads=5, n_mels=45, semantic_dim=7, layers=2)])    # scalar inject (45 mels)
def test_solo_equality_generic(kw):
    cfg = CFG(device=DEV, **kw)
    check_all(make(cfg, kernels="generic"), cfg, 5, 70, 37, seed=kw["n_mels"])


def test_defaults_are_the_existing_call():
    """No new keyword: bitwise the plain edtts_sample_inpaint entry point (called here directly); full lengths and one seed per row
    at B = 1: bitwise the scalar seed."""
    import ctypes as C
    smp = make(CFG(device=DEV))
    cfg = smp.cfg
    B, T, S, n = 3, 96, 48, 3
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, T, cfg.n_mels, generator=g).to(DEV)
    f = torch.randn(B, S, cfg.semantic_dim, generator=g).to(DEV)
    kn = torch.randn(B, OV, cfg.n_mels, generator=g).to(DEV)
    for scale in (1.0, 2.5):
        out = smp.inpaint_teacher_refine(x, f, kn, OV, 0.5, n, scale, seed=9)
        # the same call through the old entry point
        nz = native.randn(tuple(x.shape), DEV, seed=9, stream_id=0x52)
        sab = smp.schedule._host_t["sqrt_alpha_bar"][500].to(DEV)
        s1m = smp.schedule._host_t["sqrt_one_minus_alpha_bar"][500].to(DEV)
        xr = (sab * x + s1m * nz).contiguous()
        times = linspace_times(500, n)
        t_all = torch.tensor(times, dtype=torch.int64, device=DEV)
        s_all = torch.zeros(n, dtype=torch.int64, device=DEV)
        cf = (C.c_float * (4 * n))(*smp._coefs(times))
        dec = smp.decoder
        ws = dec.workspace(B, T, S, n, DEV)
        guided = scale != 1.0
        ws_u = dec.workspace(B, T, S, n, DEV, tag="uncond") if guided else None
        zeros = torch.zeros_like(f) if guided else None
        v_u = torch.empty_like(xr) if guided else None
        native.lib().edtts_sample_inpaint(C.byref(dec.dims()), dec._ensure_packed().data_ptr(), ws.data_ptr(),
                                          None if ws_u is None else ws_u.data_ptr(), B, T, S, f.data_ptr(),
                                          None if zeros is None else zeros.data_ptr(), xr.data_ptr(), n, t_all.data_ptr(),
                                          s_all.data_ptr(), cf, kn.data_ptr(), OV, None, C.c_uint64(9), float(scale),
                                          None if v_u is None else v_u.data_ptr(), native._stream(DEV))
        assert torch.equal(out, xr), scale
        one = smp.inpaint_teacher_refine(x[:1], f[:1], kn[:1], OV, 0.5, n, scale, seed=9)
        per_row = smp.inpaint_teacher_refine(x[:1], f[:1], kn[:1], OV, 0.5, n, scale, seeds=[9], x_lengths=torch.tensor([T]),
                                             sem_lengths=torch.tensor([S]))
        assert torch.equal(one, per_row), scale
        assert torch.equal(one, out[:1]), scale
    st = smp.inpaint_student_sample((1, T, cfg.n_mels), f[:1], kn[:1], OV, 4, seed=5)
    assert torch.equal(st, smp.inpaint_student_sample((1, T, cfg.n_mels), f[:1], kn[:1], OV, 4, seeds=[5]))


@pytest.mark.parametrize("shape", [(5, 37, 80), (3, 45), (4, 8, 3), (2, 1)])
def test_randn_rows_rows_are_randn(shape):
    seeds = [0, 1, 2 ** 63 + 5, 123456789, 77][:shape[0]]
    for sid in (0x51, 0x53):
        rows = native.randn_rows(shape, DEV, seeds, stream_id=sid, scale=0.5)
        assert rows.shape == shape
        for b, s in enumerate(seeds):
            assert torch.equal(rows[b], native.randn(shape[1:], DEV, seed=s, stream_id=sid, scale=0.5)), (shape, b)
    long = native.randn_rows((2, 100), DEV, [3, 4], stream_id=0x52)
    short = native.randn_rows((2, 37), DEV, [3, 4], stream_id=0x52)
    assert torch.equal(long[:, :37], short)  # a longer row begins with the shorter one's draws
    with pytest.raises(native.EdttsError):
        native.randn_rows((2, 8), DEV, [1, 2], stream_id=0x10000)


def test_clamped_lengths_and_short_rows_are_flagged():
    smp = make(CFG(device=DEV))
    cfg = smp.cfg
    B, T, S, n = 3, 64, 32, 2
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, T, cfg.n_mels, generator=g).to(DEV)
    f = torch.randn(B, S, cfg.semantic_dim, generator=g).to(DEV)
    kn = torch.randn(B, OV, cfg.n_mels, generator=g).to(DEV)
    ws = smp.decoder.workspace(B, T, S, n, x.device)
    native.index_errors(ws)  # clear
    bad_t = torch.tensor([0, T + 1, 40], dtype=torch.int64, device=DEV)
    bad_s = torch.tensor([S + 3, 0, 7], dtype=torch.int64, device=DEV)
    out = smp.inpaint_teacher_refine(x, f, None, 0, 0.5, n, 1.5, x_lengths=bad_t, sem_lengths=bad_s, seeds=[1, 2, 3])
    torch.cuda.synchronize()
    assert native.index_errors(ws) & native.EDTTS_IDX_LEN
    ok = smp.inpaint_teacher_refine(x, f, None, 0, 0.5, n, 1.5, x_lengths=torch.tensor([1, T, 40]), sem_lengths=torch.tensor([S, 1, 7]),
                                    seeds=[1, 2, 3])
    assert torch.equal(out, ok)
    assert native.index_errors(ws) == 0
    # a row shorter than the known overlap: its solo call would refuse; flagged, and only its own frames are written
    short = torch.tensor([T, 5, 40], dtype=torch.int64, device=DEV)
    out = smp.inpaint_teacher_refine(x, f, kn, OV, 0.5, n, 1.0, x_lengths=short, seeds=[1, 2, 3])
    torch.cuda.synchronize()
    assert native.index_errors(ws) & native.EDTTS_IDX_LEN
    assert bool(torch.isfinite(out).all()) and bool((out[1, 5:] == 0).all())
    assert torch.equal(out[1, :5], kn[1, :5])  # the final force of the frames it has
    old = native.CHECK_INDICES
    native.CHECK_INDICES = True
    try:
        with pytest.raises(IndexError, match="length"):
            smp.inpaint_teacher_refine(x, f, kn, OV, 0.5, n, 1.0, x_lengths=short, seeds=[1, 2, 3])
    finally:
        native.CHECK_INDICES = old


def test_graph_replays_with_new_lengths():
    smp = make(CFG(device=DEV))
    cfg = smp.cfg
    B, T, S, n = 4, 96, 48, 3
    x, f, kn, _, _, seeds = inputs(cfg, B, T, S, 31, True)
    x, f = torch.nan_to_num(x, nan=0.25), torch.nan_to_num(f, nan=0.5)
    mixes = [(lens(B, T, 32, lo=OV), lens(B, S, 33)), (torch.flip(lens(B, T, 34, lo=OV), [0]), torch.flip(lens(B, S, 35), [0]))]
    tl_dev, sl_dev = mixes[0][0].to(DEV), mixes[0][1].to(DEV)
    sd_dev = native.seed_tensor(seeds, B, DEV)
    noise = torch.randn(B, T, cfg.n_mels, generator=torch.Generator().manual_seed(36)).to(DEV)

    def call(tl, sl):
        return smp.inpaint_teacher_refine(x, f, kn, OV, 0.5, n, 1.5, noise=noise, x_lengths=tl, sem_lengths=sl, seeds=sd_dev)
    eager = [call(a, b) for a, b in mixes]
    call(tl_dev, sl_dev)  # warm-up with the device tensors
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        static_out = call(tl_dev, sl_dev)
    for _ in range(2):
        for (a, b), e in zip(mixes, eager):
            tl_dev.copy_(a)
            sl_dev.copy_(b)
            static_out.fill_(7.0)
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_out, e)
    del gr
    smp.decoder.release_pinned()


# ------------------------------------------------------------------------------------------------ generate_long_batch
HOP, SR, CHUNK = 160, 16000, 48


def long_batch_inputs(cfg, rows, totals, seed):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(1, r, cfg.semantic_dim, generator=g).to(DEV) for r in rows]
    smp_plan = InpaintSampler.chunk_plan
    stats = []
    for t in totals:
        k = smp_plan(t, CHUNK, OV, HOP)[0]
        stats.append([(torch.randn(1, 1, cfg.n_mels, generator=g).to(DEV) * 0.1, (torch.rand(1, 1, cfg.n_mels, generator=g) + 0.5).to(DEV))
                      for _ in range(k)])
    return feats, stats


@pytest.mark.parametrize("scale", [1.0, 1.5])
def test_generate_long_batch_is_generate_long_per_utterance(scale):
    smp = make(CFG(device=DEV))
    # one single-chunk utterance (40 frames), one whose last slice is cut short by its features (150 frames, 70 rows), and others
    rows, totals = (128, 30, 70, 128, 128), (100, 40, 150, 230, 75)
    feats, stats = long_batch_inputs(smp.cfg, rows, totals, 41)
    plans = smp.plan_long_batch(rows, totals, CHUNK, OV, stats, [0] * 5, hop_length=HOP, sample_rate=SR)
    assert plans[1]["n_chunks"] == 1
    last = plans[2]["slices"][-1]
    full = InpaintSampler.latent_slices(plans[2]["n_chunks"], (CHUNK - OV) * HOP, CHUNK * HOP, SR)[-1]
    assert last[1] == 70 < full[1] and last[1] - last[0] < full[1] - full[0]
    seeds = [5, 17, 2 ** 40, 3, 99]
    out = smp.generate_long_batch(feats, totals, CHUNK, OV, stats, seeds=seeds, strength=0.6, steps=3, cfg_scale=scale,
                                  hop_length=HOP, sample_rate=SR)
    assert len(out) == 5
    for n in range(5):
        alone = smp.generate_long(feats[n], totals[n], CHUNK, OV, stats[n], strength=0.6, steps=3, cfg_scale=scale, seed=seeds[n],
                                  hop_length=HOP, sample_rate=SR)
        assert out[n].shape == alone.shape == (smp.cfg.n_mels, totals[n])
        assert torch.equal(out[n], alone), (n, max_abs(out[n].cpu(), alone.cpu()))


def test_generate_long_batch_with_the_golden_utterance(golden):
    """The longform_stitch.npz utterance, with the reference's draws, in a batch with two utterances on library draws: its entry meets
    test_longform_stitch's tolerance against the reference loop, the others are bitwise their generate_long."""
    g = golden("longform_stitch")
    smp = make(CFG(device=DEV))
    cu = lambda a: torch.as_tensor(a).to(DEV)
    n_chunks = g["latent_slices"].shape[0]
    draws = [{k: cu(g[f"c{c}_{k}"]) for k in ("x_coarse", "noise", "noise_k") if f"c{c}_{k}" in g} for c in range(n_chunks)]
    stats = [(cu(g[f"c{c}_mean"]), cu(g[f"c{c}_std"])) for c in range(n_chunks)]
    steps, strength, scale = g["params"].tolist()
    total, chunk, ov, hop_len, sr = (int(v) for v in g["geometry"].tolist())
    z = cu(g["z_q_global"])
    others_t = (130, 60)
    gen = torch.Generator().manual_seed(51)
    others = [torch.randn(1, 128, z.shape[2], generator=gen).to(DEV) for _ in others_t]
    ostats = [[stats[0]] * InpaintSampler.chunk_plan(t, chunk, ov, hop_len)[0] for t in others_t]
    out = smp.generate_long_batch([others[0], z, others[1]], [others_t[0], total, others_t[1]], chunk, ov, [ostats[0], stats, ostats[1]],
                                  seeds=[8, 0, 9], strength=strength, steps=int(steps), cfg_scale=scale, hop_length=hop_len,
                                  sample_rate=sr, draws=[None, draws, None])
    ref = torch.as_tensor(g["final_mel"])
    err = max_abs(out[1].cpu(), ref)
    print(f"golden utterance in a batch of 3: max-abs {err:.2e} of a {float(ref.abs().max()):.3f} peak")
    assert out[1].shape == ref.shape and err <= 5e-4 * float(ref.abs().max())
    for j, n in ((0, 0), (2, 1)):
        alone = smp.generate_long(others[n], others_t[n], chunk, ov, ostats[n], strength=strength, steps=int(steps), cfg_scale=scale,
                                  seed=(8, 9)[n], hop_length=hop_len, sample_rate=sr)
        assert torch.equal(out[j], alone), j


def parent_inputs(smp):
    """The inputs of tests/golden/longform_parent.npz: seeded generate_long outputs of the parent commit (before generate_long became
    generate_long_batch of one utterance), made with exactly this construction."""
    cfg = smp.cfg
    g = torch.Generator().manual_seed(7)
    feats = torch.randn(1, 460, cfg.semantic_dim, generator=g).cuda()
    cases = []
    for total, chunk, ov, steps, extra in ((230, 48, 12, 3, {}),
                                           (900, 201, 51, 10, dict(chunk_samples=32000, overlap_samples=8000, total_samples=143900))):
        k = InpaintSampler.chunk_plan(total, chunk, ov, 160, extra.get("chunk_samples"), extra.get("overlap_samples"),
                                      extra.get("total_samples"))[0]
        stats = [(torch.randn(1, 1, cfg.n_mels, generator=g).cuda() * 0.1, torch.full((1, 1, cfg.n_mels), 0.7).cuda()) for _ in range(k)]
        for scale in (1.0, 1.5):
            for seed in (4, 2 ** 40 + 3):
                cases.append((f"{total}_{scale}_{seed}", dict(total_frames=total, chunk_frames=chunk, overlap_frames=ov, chunk_stats=stats,
                                                              strength=0.6, steps=steps, cfg_scale=scale, seed=seed, hop_length=160,
                                                              sample_rate=16000, **extra)))
    return feats, cases


def test_generate_long_is_bitwise_the_parent(golden):
    import hashlib
    g = golden("longform_parent")
    smp = make(CFG(device=DEV))
    feats, cases = parent_inputs(smp)
    assert g["sha256"].shape == (len(cases), 32)
    got = {}
    for (key, kw), digest in zip(cases, g["sha256"]):
        out = smp.generate_long(feats, **kw).cpu().contiguous()
        got[key] = out
        assert hashlib.sha256(out.numpy().tobytes()).digest() == bytes(digest.tolist()), key
    assert torch.equal(got["230_1.0_4"], g["mel_230_1.0_4"])
    assert torch.equal(got["230_1.5_1099511627779"], g["mel_230_1.5_1099511627779"])
    # ... and the same utterance twice in one batch, with two seeds
    kw = dict(cases[2][1])
    both = smp.generate_long_batch([feats, feats], [kw.pop("total_frames")] * 2, kw.pop("chunk_frames"), kw.pop("overlap_frames"),
                                   [kw.pop("chunk_stats")] * 2, seeds=[4, 2 ** 40 + 3], **{k: v for k, v in kw.items() if k != "seed"})
    assert torch.equal(both[0].cpu(), got["230_1.5_4"]) and torch.equal(both[1].cpu(), got["230_1.5_1099511627779"])
