"""In-painting anywhere (keep= of the in-painting samplers, InpaintSampler.keep_mask and .edit), host side: the two new C symbols in
the table, the header and the library, the entry points' argument errors that return before any device call, every ValueError of the
Python surface, keep_mask, and edit's call sequence with the launches stubbed.  No GPU needed."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import inpaint_mask_util as U
from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, InpaintSampler, native
from edge_diffusion_tts_amd.schedule import DiffusionSchedule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"edtts_sample_inpaint_mask_len": "edtts_sample_inpaint_len",
         "edtts_sample_inpaint_multistep_mask_len": "edtts_sample_inpaint_multistep_len"}


def sampler():
    cfg = CFG(device="cpu")
    return InpaintSampler(cfg, DiffusionSchedule(cfg.diff_steps), EdgeDiffusionDecoder(cfg)), cfg


def test_symbols_are_in_the_table_the_header_and_the_library():
    header = open(os.path.join(REPO, "include", "edtts.h")).read()
    lib = ctypes.CDLL(native.LIB_PATH)  # (dlopen only: no device call)
    norm = lambda text: [re.sub(r"\s+", " ", p.strip()) for p in text.split(",")]
    for sym, base in PAIRS.items():
        assert sym in native.EXPORTED_SYMBOLS and getattr(lib, sym) is not None
        params = norm(re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)", header).group(1))
        want = norm(re.search(r"\bint\s+" + base + r"\s*\(([^)]*)\)", header).group(1))
        # the arguments of the prefix entry point, with the mask where it has the overlap length
        assert want.count("int overlap_len") == 1
        assert params == ["const uint8_t* keep" if p == "int overlap_len" else p for p in want]
        kind, args = native._ABI[sym]
        bkind, bargs = native._ABI[base]
        i = want.index("int overlap_len")
        assert kind == bkind and args == bargs[:i] + (ctypes.c_void_p,) + bargs[i + 1:]
    assert lib.edtts_version() == 400  # (an added export did not move it before either)


def test_the_masks_of_the_gpu_tests_cover_what_they_should():
    keep = U.keep_mask()
    for b in range(U.B):
        n = U.T_LEN[b]
        for m in (keep[b], keep[b, :n]):
            assert 0.2 <= float(m.float().mean()) <= 0.8, b
    k0 = keep[0].tolist()
    assert k0[0] and k0[U.T - 1]                                   # frame 0, the last frame
    assert k0[9:12] == [False, True, False]                        # one isolated kept frame
    assert k0[24:27] == [True, False, True]                        # one isolated free frame
    for b in (1, 2):                                               # a kept run across t_len, ending the live part in a kept frame
        n = U.T_LEN[b]
        assert n < U.T and bool(keep[b, n - 1]) and bool(keep[b, n])
    assert keep[2].tolist()[2:5] == [False, True, False]


def _call(symbol, cfg, modes=(1, 1), **over):
    """The argument list of one *_mask_len export at B=2, S=4 with every pointer a (never dereferenced) small integer."""
    dims = EdgeDiffusionDecoder(cfg).dims()
    ptr = iter(range(64, 4096, 64))
    coef = (ctypes.c_float * 16)(*([1.0] * 16))
    coef[0], coef[8] = modes
    a = dict(dims=ctypes.byref(dims), packed=next(ptr), workspace=next(ptr), workspace_uncond=None, B=2, T=8, S=4, sem_features=next(ptr),
             zero_features=None, x=next(ptr), num_steps=2, t_all=next(ptr), step_all=next(ptr), coef_host=coef, known_mel=None,
             keep=None, noise_k=None, seed=ctypes.c_uint64(0), cfg_scale=1.0, v_uncond=None, t_len=None, s_len=None, seeds=None)
    if "multistep" in symbol:
        a.update(hist=next(ptr), x0_all=None)
    a["stream"] = None
    assert set(over) <= set(a), over
    a.update(over)
    return [ctypes.c_void_p(v) if isinstance(v, int) and k not in ("B", "T", "S", "num_steps") else v for k, v in a.items()], dims


def test_entry_points_refuse_bad_arguments_before_any_device_call():
    cfg = CFG(device="cpu")
    max_pos = EdgeDiffusionDecoder(cfg).dims().max_pos
    ARG = -2  # EDTTS_ERR_ARG
    null, both = (ARG, "NULL pointer argument"), (ARG, "known_mel and keep must both be given or both be NULL")
    table = []
    for sym in PAIRS:
        table += [
            (sym, dict(known_mel=4096), both),
            (sym, dict(keep=4096), both),
            (sym, dict(known_mel=4096, keep=8192, packed=None), null),
            (sym, dict(packed=None), null),
            (sym, dict(num_steps=0), (ARG, "num_steps=0 < 1")),
            (sym, dict(known_mel=4096, keep=8192, cfg_scale=1.5), (ARG, "cfg_scale != 1 needs workspace_uncond, zero_features and v_uncond")),
            # (no overlap length to refuse: with a mask the next failing check is the shape's)
            (sym, dict(known_mel=4096, keep=8192, T=max_pos + 1),
             (ARG, f"T={max_pos + 1} exceeds the positional table ({max_pos} rows) -- the reference raises here too")),
        ]
    multi = "edtts_sample_inpaint_multistep_mask_len"
    table += [(multi, dict(hist=None), null), (multi, dict(modes=(0, 1)), (ARG, "step 0: bad solver mode 0")),
              (multi, dict(known_mel=4096, keep=8192, modes=(2, 1)), (ARG, "step 0: bad solver mode 2"))]
    L = native.lib()
    for sym, over, (code, text) in table:
        args, _dims = _call(sym, cfg, **over)
        with pytest.raises(native.EdttsError) as e:
            getattr(L, sym)(*args)
        got = (int(re.search(r"\(code (-?\d+)\)", str(e.value)).group(1)), L.edtts_last_error().decode())
        assert got == (code, text), (sym, over, got)


def test_python_surface():
    for fn in (InpaintSampler.inpaint_student_sample, InpaintSampler.inpaint_teacher_refine, InpaintSampler.inpaint_dpm_refine,
               InpaintSampler._run):
        p = inspect.signature(fn).parameters["keep"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__
    for fn in (InpaintSampler.generate_long, InpaintSampler.generate_long_batch, InpaintSampler.plan_long_batch):
        assert "keep" not in inspect.signature(fn).parameters
    p = inspect.signature(InpaintSampler.edit).parameters
    assert list(p)[:4] == ["self", "mel_n", "sem_features", "regenerate"]
    assert (p["num_steps"].default, p["refine"].default, p["order"].default, p["cfg_scale"].default) == (4, "dpmpp", 2, 1.0)
    for k in ("num_steps", "refine", "steps", "order", "strength", "cfg_scale", "x_lengths", "sem_lengths", "seeds"):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert "keep" in inspect.signature(native.sample_inpaint).parameters


@pytest.fixture
def no_launch(monkeypatch):
    """Every door to the device raises: a check that lets a call through to one fails the test."""
    def refuse(*a, **k):
        raise AssertionError("a launch was reached")
    for name in ("randn", "randn_rows", "sample_inpaint", "lib"):
        monkeypatch.setattr(native, name, refuse)


def test_wrong_keep_arguments_raise_before_any_launch(no_launch):
    smp, cfg = sampler()
    B, T, M = 2, 41, cfg.n_mels
    x, f = torch.zeros(B, T, M), torch.zeros(B, 20, cfg.semantic_dim)
    known, keep = torch.zeros(B, T, M), torch.zeros(B, T, dtype=torch.bool)
    calls = {
        "student": lambda kn, ov=0, n=4, **kw: smp.inpaint_student_sample((B, T, M), f, kn, ov, n, **kw),
        "teacher": lambda kn, ov=0, n=4, **kw: smp.inpaint_teacher_refine(x, f, kn, ov, 0.5, n, **kw),
        "dpm": lambda kn, ov=0, n=4, **kw: smp.inpaint_dpm_refine(x, f, kn, ov, 0.5, n, 2, **kw),
    }
    for name, call in calls.items():
        for bad in (keep.to(torch.int64), keep.to(torch.float32), keep.tolist(), 1):
            with pytest.raises(ValueError, match="keep must be a bool or uint8 tensor"):
                call(known, keep=bad)
        for bad in (keep[:1], keep[:, :40], keep.reshape(B, T, 1), keep.t()):
            with pytest.raises(ValueError, match=r"keep must be \[2, 41\]"):
                call(known, keep=bad)
        with pytest.raises(ValueError, match="keep= needs known_mel"):
            call(None, keep=keep)
        for bad in (known[:, :5], known[:1], known[:, :, :M - 1]):
            with pytest.raises(ValueError, match="with keep=, known_mel must be"):
                call(bad, keep=keep)
        with pytest.raises(ValueError, match="overlap_len must be 0"):
            call(known, 5, keep=keep)
        for bad in (torch.zeros(4, B, 5, M), torch.zeros(3, B, T, M), torch.zeros(B, T, M)):
            with pytest.raises(ValueError, match="with keep=, noise_k must be"):
                call(known, keep=keep.to(torch.uint8), noise_k=bad)
    with pytest.raises(ValueError, match="refine"):
        smp.edit(known, f, [[], []], refine="euler")
    with pytest.raises(ValueError, match="intervals"):
        smp.edit(known, f, [[(0, 5)]])


def test_edit_checks_the_refinement_before_the_student_sample(no_launch):
    smp, cfg = sampler()
    known, f = torch.zeros(2, 41, cfg.n_mels), torch.zeros(2, 20, cfg.semantic_dim)
    with pytest.raises(ValueError, match="order"):
        smp.edit(known, f, [[(0, 5)], []], order=4)
    with pytest.raises(ValueError, match="steps"):
        smp.edit(known, f, [[(0, 5)], []], steps=0)
    for refine in ("dpmpp", "ddim"):
        with pytest.raises(IndexError):  # t_start = 1000: outside the tables, as the refinements themselves
            smp.edit(known, f, [[(0, 5)], []], refine=refine, strength=1.0)


def test_keep_mask():
    m = InpaintSampler.keep_mask(3, 8, [[(0, 2), (7, 8)], [], [(3, 3), (2, 6), (4, 8)]])
    assert m.dtype == torch.bool and m.shape == (3, 8) and m.device.type == "cpu"
    assert m.tolist() == [[True, True, False, False, False, False, False, True], [False] * 8,
                          [False, False, True, True, True, True, True, True]]
    assert torch.equal(InpaintSampler.keep_mask(U.B, U.T, U.KEEP, "cpu"), U.keep_mask())
    assert InpaintSampler.keep_mask(1, 4, [[(0, 4)]]).all() and InpaintSampler.keep_mask(0, 4, []).shape == (0, 4)
    for bad in ([[(0, 2)]], [[], [], [], []]):
        with pytest.raises(ValueError, match="expected 3 entries"):
            InpaintSampler.keep_mask(3, 8, bad)
    for bad in ((-1, 2), (0, 9), (5, 4)):
        with pytest.raises(ValueError, match="need 0 <= start <= end <= 8"):
            InpaintSampler.keep_mask(1, 8, [[bad]])
    for bad in (3, (1, 2, 3), ("a", "b")):
        with pytest.raises(ValueError, match="pairs"):
            InpaintSampler.keep_mask(1, 8, [[bad]])


@pytest.mark.parametrize("refine", ["dpmpp", "ddim", None])
def test_edit_call_sequence(monkeypatch, refine):
    """edit = the student sample under keep = everything outside `regenerate`, then the chosen refinement of its result under the same
    mask, with the lengths and seeds handed on.  The launches are stubbed: _run records its arguments and returns a marker."""
    smp, cfg = sampler()
    B, T, M = 2, 12, cfg.n_mels
    mel, f = torch.randn(B, T, M), torch.zeros(B, 6, cfg.semantic_dim)
    regen = [[(3, 7)], [(0, 2), (10, 12)]]
    want_keep = ~InpaintSampler.keep_mask(B, T, regen)
    tl, sl, seeds = torch.tensor([12, 9]), torch.tensor([6, 4]), [4, 5]
    log = []

    def fake_run(x, sem, times, step_idx, known_mel, overlap_len, cfg_scale, noise_k, seed, x_lengths=None, sem_lengths=None, seeds=None, *,
                 lms_rows=None, return_intermediates=False, keep=None):
        log.append(dict(x=x, sem=sem, n=len(times), t0=times[0], step_idx=step_idx, known=known_mel, ov=overlap_len, scale=cfg_scale,
                        noise_k=noise_k, tl=x_lengths, sl=sem_lengths, seeds=seeds, lms=lms_rows is not None, keep=keep))
        return torch.full((B, T, M), float(len(log)))
    monkeypatch.setattr(smp, "_run", fake_run)
    monkeypatch.setattr(native, "randn_rows", lambda shape, dev, seeds, stream_id: torch.full(shape, float(stream_id)))
    monkeypatch.setattr(native, "sample_inpaint", None)
    out = smp.edit(mel, f, regen, num_steps=3, refine=refine, steps=None if refine == "ddim" else 6, order=3, strength=0.5,
                   cfg_scale=1.5, x_lengths=tl, sem_lengths=sl, seeds=seeds)
    assert len(log) == (1 if refine is None else 2) and bool((out == len(log)).all())
    for c in log:
        assert c["known"] is mel and c["ov"] == 0 and c["noise_k"] is None and c["sem"] is f
        assert torch.equal(c["keep"], want_keep) and c["keep"].dtype == torch.bool
        assert c["tl"] is tl and c["sl"] is sl and c["seeds"] is seeds
    stu = log[0]
    assert (stu["n"], stu["t0"], stu["step_idx"], stu["scale"], stu["lms"]) == (3, cfg.diff_steps - 1, 3, 1.0, False)
    assert bool((stu["x"] == 0x51).all())  # the student's start noise: the per-row stream of inpaint_student_sample
    if refine is not None:
        ref = log[1]
        t_start = int(cfg.diff_steps * 0.5)
        sab, s1m = smp.schedule._host_t["sqrt_alpha_bar"][t_start], smp.schedule._host_t["sqrt_one_minus_alpha_bar"][t_start]
        assert torch.equal(ref["x"], sab * torch.full((B, T, M), 1.0) + s1m * torch.full((B, T, M), float(0x52)))  # q_sample of the student's result
        assert (ref["n"], ref["t0"], ref["step_idx"], ref["scale"]) == (6 if refine == "dpmpp" else 10, t_start, 0, 1.5)
        assert ref["lms"] == (refine == "dpmpp")
