"""In-painting anywhere on the GPU: the three in-painting samplers with keep= on every kernel family -- parity
with a composition of the oracle's functions, and the bitwise contract of include/edtts.h: a prefix mask is the prefix call, kept
frames are known_mel, the degenerate masks, data that is never read, row independence, determinism and graph capture.
Run on the GPU box: python -m pytest tests -m gpu."""
import pytest
import torch

import inpaint_mask_util as U
from conftest import max_abs
from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, InpaintSampler, native, synth_state_dict
from inpaint_mask_util import B, N_STUDENT, S, S_LEN, SEEDS, STEPS, STRENGTH, T, T_LEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL, TOL_TEACHER = 1e-4, 5e-4  # the bars of test_inpaint_dpm_gpu.py (student, DPM) and test_gpu_parity.py (inpaint_teacher_refine)
ALL = list(U.CONFIGS)
OV = 5
_made, _refs = {}, {}


def make(name):
    """(sampler, the decoder's state dict on the CPU, cfg, the case's CPU inputs); one per configuration for the whole module."""
    if name not in _made:
        ckw, dkw = U.CONFIGS[name]
        cfg = CFG(device=DEV, **ckw)
        dec = EdgeDiffusionDecoder(cfg, **dkw)
        sd = synth_state_dict(cfg, 0, max_pos=dec.max_len, max_ctx_pos=dec.max_context_len)
        dec.load_state_dict(sd)
        dec = dec.to(DEV).eval()
        _made[name] = (InpaintSampler(cfg, DiffusionSchedule(cfg.diff_steps).to(DEV), dec), sd, cfg, U.inputs(cfg))
    return _made[name]


def reference(key, fn):
    """An oracle run: computed once, shared by the tests that need it, never written to."""
    if key not in _refs:
        _refs[key] = fn()
    return _refs[key]


def cu(t):
    return t.to(DEV).contiguous()


def samplers(smp, d, scale=1.5, order=2):
    """The three samplers as functions of (known, keep-or-overlap keywords, rows): every other argument is the case's."""
    def student(known, rows=slice(None), frames=T, **kw):
        x0 = cu(d["x_init"][rows, :frames])
        return smp.inpaint_student_sample(tuple(x0.shape), cu(d["sem"][rows]), known, num_steps=N_STUDENT, x_init=x0, **kw)

    def teacher(known, rows=slice(None), frames=T, **kw):
        return smp.inpaint_teacher_refine(cu(d["x_coarse"][rows, :frames]), cu(d["sem"][rows]), known, strength=STRENGTH, steps=STEPS,
                                          cfg_scale=scale, noise=cu(d["noise"][rows, :frames]), **kw)

    def dpm(known, rows=slice(None), frames=T, **kw):
        return smp.inpaint_dpm_refine(cu(d["x_coarse"][rows, :frames]), cu(d["sem"][rows]), known, strength=STRENGTH, steps=STEPS,
                                      order=order, cfg_scale=scale, noise=cu(d["noise"][rows, :frames]), **kw)
    return {"student": student, "teacher": teacher, "dpm": dpm}


def n_steps(which):
    return N_STUDENT if which == "student" else STEPS


def ragged():
    return dict(x_lengths=torch.tensor(T_LEN), sem_lengths=torch.tensor(S_LEN), seeds=SEEDS)


def live(keep):
    """keep with the frames at or past T_LEN cleared."""
    m = keep.clone()
    for b, n in enumerate(T_LEN):
        m[b, n:] = False
    return m


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", U.FP32)
def test_parity_student_and_teacher(name):
    smp, sd, cfg, d = make(name)
    keep = U.keep_mask()
    fn = samplers(smp, d)
    out = fn["student"](cu(d["known"]), keep=cu(keep), noise_k=cu(d["noise_k"][:N_STUDENT])).cpu()
    err = max_abs(out, reference((name, "student"), lambda: U.oracle_student(sd, cfg, d, keep)))
    print(f"inpaint_student_sample keep= {name}: max-abs {err:.2e} vs the oracle composition")
    assert err < TOL
    assert torch.equal(out[keep], d["known"][keep])
    out = fn["teacher"](cu(d["known"]), keep=cu(keep), noise_k=cu(d["noise_k"])).cpu()
    err = max_abs(out, reference((name, "teacher"), lambda: U.oracle_teacher(sd, cfg, d, keep, 1.5)))
    print(f"inpaint_teacher_refine keep= {name} cfg 1.5: max-abs {err:.2e} vs the oracle composition")
    assert err < TOL_TEACHER
    assert torch.equal(out[keep], d["known"][keep])


@pytest.mark.parametrize("name, cases", [("32/2/80", ((1, 1.0), (2, 1.5), (3, 1.0), (3, 1.5))), ("160/4/80", ((2, 1.5),)),
                                         ("generic 50/5/45", ((2, 1.5), (3, 1.0)))])
def test_parity_dpm(name, cases):
    smp, sd, cfg, d = make(name)
    keep = U.keep_mask()
    for order, scale in cases:
        out = samplers(smp, d, scale, order)["dpm"](cu(d["known"]), keep=cu(keep), noise_k=cu(d["noise_k"])).cpu()
        err = max_abs(out, reference((name, "dpm", order, scale), lambda: U.oracle_dpm(sd, cfg, d, keep, order, scale)))
        print(f"inpaint_dpm_refine keep= {name} order {order} cfg {scale}: max-abs {err:.2e} vs the oracle composition")
        assert err < TOL
        assert torch.equal(out[keep], d["known"][keep])


def test_parity_ragged_rows_against_the_oracle_on_each_utterance():
    """The oracle has no lengths: row b of the ragged call is held to the oracle run on utterance b alone (its own frames, feature
    rows and mask), with the noise injected."""
    name = "160/4/80"
    smp, sd, cfg, d = make(name)
    keep = U.keep_mask()
    out = samplers(smp, d, 1.5, 2)["dpm"](cu(d["known"]), keep=cu(keep), noise_k=cu(d["noise_k"]), x_lengths=torch.tensor(T_LEN),
                                          sem_lengths=torch.tensor(S_LEN)).cpu()
    for b in range(B):
        ref = reference((name, "dpm solo", b), lambda: U.oracle_dpm(sd, cfg, d, keep, 2, 1.5, rows=slice(b, b + 1), frames=T_LEN[b],
                                                                     sem_rows=S_LEN[b]))
        err = max_abs(out[b:b + 1, :T_LEN[b]], ref)
        print(f"inpaint_dpm_refine keep= {name} row {b} of a ragged batch: max-abs {err:.2e} vs the oracle on that utterance")
        assert err < TOL
        assert bool((out[b, T_LEN[b]:] == 0).all())


# ------------------------------------------------------------------------------------------------ 1. prefix equivalence
@pytest.mark.parametrize("name", ALL)
def test_prefix_mask_is_the_prefix_call(name):
    smp, sd, cfg, d = make(name)
    keep = torch.zeros(B, T, dtype=torch.bool)
    keep[:, :OV] = True
    known = d["known"].clone()
    known[:, OV:] = float("nan")  # (never read)
    for which, orders in (("student", (2,)), ("teacher", (2,)), ("dpm", (1, 2, 3))):
        for order in orders:
            fn = samplers(smp, d, 1.5, order)[which]
            # ragged, per-row seeds, in-kernel Philox noise
            want = fn(cu(d["known"][:, :OV]), overlap_len=OV, **ragged())
            got = fn(cu(known), keep=cu(keep), **ragged())
            assert torch.equal(got, want), (name, which, order, "ragged + seeds", max_abs(got.cpu(), want.cpu()))
            # injected noise
            nk = d["noise_k"][:n_steps(which)]
            want = fn(cu(d["known"][:, :OV]), overlap_len=OV, noise_k=cu(nk[:, :, :OV]))
            got = fn(cu(known), keep=cu(keep), noise_k=cu(nk))
            assert torch.equal(got, want), (name, which, order, "injected noise")
            # one seed: the draws are keyed by the element of the whole tensor, so the two agree for B = 1
            one = slice(1, 2)
            want = fn(cu(d["known"][one, :OV]), rows=one, overlap_len=OV, seed=11)
            got = fn(cu(known[one]), rows=one, keep=cu(keep[one]), seed=11)
            assert torch.equal(got, want), (name, which, order, "B = 1, seed")
            assert bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------ 2, 3, 4, 6
@pytest.mark.parametrize("name", ALL)
def test_kept_frames_unread_data_and_determinism(name):
    smp, sd, cfg, d = make(name)
    keep = U.keep_mask()
    lv = live(keep)
    known_nan = d["known"].clone()
    known_nan[~lv] = float("nan")  # frames that are not kept, and kept ones past the lengths
    for which in ("student", "teacher", "dpm"):
        fn = samplers(smp, d)[which]
        nk = d["noise_k"][:n_steps(which)]
        nk_nan = nk.clone()
        nk_nan[:, ~lv] = float("nan")
        a = fn(cu(d["known"]), keep=cu(keep), **ragged())
        assert torch.equal(a, fn(cu(d["known"]), keep=cu(keep), **ragged())), (name, which, "two calls differ")
        assert torch.equal(a, fn(cu(known_nan), keep=cu(keep), **ragged())), (name, which, "known_mel read where it is not kept")
        assert torch.equal(a.cpu()[lv], d["known"][lv]), (name, which, "kept frames are not known_mel")
        assert bool(torch.isfinite(a).all())
        for b, n in enumerate(T_LEN):
            assert bool((a[b, n:] == 0).all()), (name, which, b, "nonzero past the length")
        assert not torch.equal(a, fn(cu(d["known"]), keep=cu(keep), **{**ragged(), "seeds": [1, 2, 3]}))  # (the seeds are really used)
        c = fn(cu(d["known"]), keep=cu(keep), noise_k=cu(nk), **ragged())
        assert torch.equal(c, fn(cu(known_nan), keep=cu(keep.to(torch.uint8) * 7), noise_k=cu(nk_nan), **ragged())), (name, which, "noise_k")
        assert torch.equal(c.cpu()[lv], d["known"][lv])


@pytest.mark.parametrize("name", ALL)
def test_degenerate_masks(name):
    smp, sd, cfg, d = make(name)
    nan = torch.full_like(d["known"], float("nan"))
    for which in ("student", "teacher", "dpm"):
        fn = samplers(smp, d)[which]
        none = fn(None, **ragged())
        zero = fn(cu(nan), keep=torch.zeros(B, T, dtype=torch.bool, device=DEV), **ragged())
        assert torch.equal(zero, none), (name, which, "all-zero keep")
        ones = fn(cu(d["known"]), keep=torch.ones(B, T, dtype=torch.uint8, device=DEV), seeds=SEEDS)
        assert torch.equal(ones.cpu(), d["known"]), (name, which, "all-ones keep")


# ------------------------------------------------------------------------------------------------ 5. row independence
@pytest.mark.parametrize("name", ALL)
def test_ragged_rows_equal_their_solo_calls(name):
    smp, sd, cfg, d = make(name)
    keep = U.keep_mask()
    for which, order, scale in (("student", 2, 1.0), ("teacher", 2, 1.5), ("dpm", 2, 1.5), ("dpm", 3, 1.0)):
        fn = samplers(smp, d, scale, order)[which]
        out = fn(cu(d["known"]), keep=cu(keep), **ragged())
        assert native.index_errors(smp.decoder.workspace(B, T, S, n_steps(which), out.device)) == 0
        for b in range(B):
            n = T_LEN[b]
            one = slice(b, b + 1)
            solo = smp_solo(smp, d, which, order, scale, b, cu(d["known"][one, :n]), cu(keep[one, :n]))
            assert torch.equal(out[b, :n], solo[0]), (name, which, order, b, max_abs(out[b, :n].cpu(), solo[0].cpu()))
            assert bool((out[b, n:] == 0).all())


def smp_solo(smp, d, which, order, scale, b, known, keep):
    """The call on utterance b alone: its first T_LEN[b] frames and S_LEN[b] feature rows, seed = SEEDS[b]."""
    one, n = slice(b, b + 1), T_LEN[b]
    sem = cu(d["sem"][one, :S_LEN[b]])
    if which == "student":
        x0 = cu(d["x_init"][one, :n])
        return smp.inpaint_student_sample(tuple(x0.shape), sem, known, num_steps=N_STUDENT, x_init=x0, seed=SEEDS[b], keep=keep)
    xc, nz = cu(d["x_coarse"][one, :n]), cu(d["noise"][one, :n])
    if which == "teacher":
        return smp.inpaint_teacher_refine(xc, sem, known, strength=STRENGTH, steps=STEPS, cfg_scale=scale, noise=nz, seed=SEEDS[b], keep=keep)
    return smp.inpaint_dpm_refine(xc, sem, known, strength=STRENGTH, steps=STEPS, order=order, cfg_scale=scale, noise=nz, seed=SEEDS[b],
                                  keep=keep)


# ------------------------------------------------------------------------------------------------ 7. capture
@pytest.mark.parametrize("name", ["160/4/80", "generic 50/5/45", "bf16 64/2/80"])
def test_graph_capture_replays_the_eager_result(name):
    smp, sd, cfg, d = make(name)
    keep_dev = cu(U.keep_mask())
    other = torch.roll(U.keep_mask(), 7, dims=1)
    known = cu(d["known"])
    tl_dev, sl_dev = torch.tensor(T_LEN, device=DEV), torch.tensor(S_LEN, device=DEV)
    sd_dev = native.seed_tensor(SEEDS, B, DEV)
    d = {k: cu(v) for k, v in d.items()}  # (no host-to-device copy inside the capture)
    for which in ("teacher", "dpm"):
        fn = samplers(smp, d)[which]
        eager =[fn(known, keep=cu(m), x_lengths=torch.tensor(T_LEN), sem_lengths=torch.tensor(S_LEN), seeds=SEEDS) for m in (U.keep_mask(), other)]
        assert not torch.equal(eager[0], eager[1])
        call = lambda: fn(known, keep=keep_dev, x_lengths=tl_dev, sem_lengths=sl_dev, seeds=sd_dev)
        call()  # warm-up with the device tensors
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            static_out = call()
        for m, e in zip((U.keep_mask(), other), eager):  # the graph reads the mask at replay: a new mask needs no new capture
            keep_dev.copy_(m)
            static_out.fill_(7.0)
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_out, e), (name, which)
        keep_dev.copy_(U.keep_mask())
        del gr
    smp.decoder.release_pinned()


# ------------------------------------------------------------------------------------------------ edit
@pytest.mark.parametrize("refine", ["dpmpp", "ddim", None])
def test_edit_keeps_everything_outside_the_regenerated_stretch(refine):
    smp, sd, cfg, d = make("160/4/80")
    regen = [[(12, 30)], [(0, 9), (20, 25)], [(4, 10)]]
    free = U.keep_mask() & False
    for b, row in enumerate(regen):
        for lo, hi in row:
            free[b, lo:hi] = True
    mel = cu(d["known"])
    out = smp.edit(mel, cu(d["sem"]), regen, refine=refine, steps=STEPS, strength=STRENGTH, cfg_scale=1.5, seeds=SEEDS)
    assert out.shape == mel.shape and bool(torch.isfinite(out).all())
    assert torch.equal(out.cpu()[~free], d["known"][~free])
    assert not bool((out.cpu()[free] == d["known"][free]).any())
    assert torch.equal(out, smp.edit(mel, cu(d["sem"]), regen, refine=refine, steps=STEPS, strength=STRENGTH, cfg_scale=1.5, seeds=SEEDS))
    if refine == "dpmpp":  # the student sample, then the refinement under the same mask
        keep = cu(~free)
        x = smp.inpaint_student_sample(tuple(mel.shape), cu(d["sem"]), mel, seeds=SEEDS, keep=keep)
        want = smp.inpaint_dpm_refine(x, cu(d["sem"]), mel, 0, STRENGTH, STEPS, 2, 1.5, seeds=SEEDS, keep=keep)
        assert torch.equal(out, want)
