"""GPU side of the HuBERT backbone's site-by-site audit (tests/hubert_audit_util.py).

For every case, shape and compute dtype one run per site, stopped there (edtts_hubert_forward_until) into a workspace and an `out`
pre-filled with 0xFF: the site's output is read where it lies and every live element must be written and within its bar of the fp64
evaluation of the operands that the runs stopped before it left behind.  Then the properties no end-to-end test reaches: both GEMM
tiles bitwise equal at every GEMM site (A1 is the smallest shape at which the launcher's own rule picks the 128 tile), the stopped
call at its last site bitwise the plain call, and the fixture's bitwise invariances on E1 and E3."""
import pytest
import torch

import hubert_audit_util as HU
from edge_diffusion_tts_amd import native

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ("F",) + HU.ECASES + ("A1",)
DTYPES = ("fp32", "bf16")
RUNS = [(c, d) for c in CASES for d in DTYPES if d == "fp32" or c in HU.BF16_LEGAL]


class Runner:
    """One (case, dtype) on the GPU: the packed blob, and stopped runs into 0xFF-filled memory."""

    def __init__(self, name, dtype):
        self.cs, self.bf, self.dt = HU.case(name), dtype == "bf16", native.HUBERT_DTYPES[dtype]
        self.m = HU.module(self.cs, dtype).to(DEV)
        self.blob, self.dims = self.m._packed(), self.m.dims
        self.pos_w = self.m.folded_pos_conv_weight().cpu()  # what the packing was given

    def run(self, sh, until, tile=0):
        """(views of the workspace, out) after a run stopped at `until`."""
        B, T_audio = sh.wav.shape
        T = HU.stage_frames(self.cs, T_audio)[-1]
        ws = torch.full((native.hubert_workspace_bytes(self.dims, B, T_audio, self.dt),), 0xFF, dtype=torch.uint8, device=DEV)
        out = torch.full((B * T * self.cs.H * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32).view(B, T, self.cs.H)
        lens = None if sh.lengths is None else sh.lengths.to(DEV)
        native.hubert_forward(self.dims, self.blob, sh.wav.to(DEV), lens, out, ws, self.dt, until=until, tile=tile)
        torch.cuda.synchronize()
        return native.hubert_workspace_views(self.dims, B, T_audio, self.dt, ws), out

    def output(self, sh, key, tile=0):
        """The output of site `key` (as stored: fp32, bf16 or int64) of a run stopped there."""
        v, out = self.run(sh, key, tile)
        site, i = key
        if site in ("conv0", "conv"):
            return v["conv"][i]
        if site in ("encnorm", "ln2", "zero"):
            return out if (site == "zero" or (site, i) == HU.last_norm(self.cs)) else v["h"]
        if site == "attn":
            return v["att16"] if self.bf else v["att"]
        return v[{"lens": "lens", "gnstat": "stats", "fpnorm": "fpnorm", "fproj": "h", "pos": "att", "qkv": "qkv", "vt": "vt", "oproj": "h",
                  "ln1": "h", "ff1": "ff", "ff2": "h"}[site]]


_RUNNERS = {}


def runner(name, dtype):
    if (name, dtype) not in _RUNNERS:
        _RUNNERS[name, dtype] = Runner(name, dtype)
    return _RUNNERS[name, dtype]


def live_rows(cs, sh, key):
    """[B, rows, 1] bool: the rows of site `key`'s output that belong to an utterance (conv stage i: its own frames at that stage)."""
    B, T_audio = sh.wav.shape
    Ts = HU.stage_frames(cs, T_audio)
    i = key[1] if key[0] == "conv" else len(cs.C) - 1
    n = torch.full((B,), Ts[i]) if sh.lengths is None else HU.stage_frames(cs, sh.lengths.clamp(HU.samples_for(cs, 1), T_audio))[i]
    return HU.rows_lt(n, Ts[i])


@pytest.mark.parametrize("name,dtype", RUNS)
def test_every_site_within_its_bar(name, dtype):
    r = runner(name, dtype)
    cs = r.cs
    for sh in HU.shapes(name):
        snap, res = {}, {}
        for key, cls, ref, bar, live in HU.sites(cs, sh, r.bf, snap, r.pos_w):
            got = r.output(sh, key).cpu().to(torch.float64).reshape(ref.shape)
            snap[key] = got
            res[key] = HU.judge(cls, got, ref, bar, live)
        assert list(res) == HU.site_list(cs, r.bf, sh.lengths is not None, sh.until)
        HU.check(res, f"hubert audit {name} {sh.tag} {dtype}")


def test_the_folded_positional_weight():
    """The weight-norm fold the packing is given (fp32, on the GPU) against the fp64 fold of the state dict."""
    for name in ("F",) + HU.ECASES:
        r = runner(name, "fp32")
        err = (r.pos_w.double() - HU.fold_pos(r.cs, torch.float64)).abs()
        worst = float((err / HU.fold_bar(r.cs)).max())
        print(f"hubert audit {name}: folded positional weight, worst error / bar {worst:.3f}")
        assert worst <= 1.0


def test_bf16_refuses_e2():
    cs = HU.case("E2")
    with pytest.raises(native.EdttsError, match="conv_dim"):
        HU.module(cs, "bf16")
    d = HU.module(cs, "fp32").dims
    for fn in (lambda: native.hubert_packed_bytes(d, 1), lambda: native.hubert_workspace_bytes(d, 1, 4000, 1),
               lambda: native.hubert_workspace_region(d, 1, 4000, 1, "h")):
        with pytest.raises(native.EdttsError, match="compute_dtype bf16 needs"):
            fn()
    # ... and the forward itself: EDTTS_ERR_UNSUPPORTED before any launch
    r = runner("E2", "fp32")
    sh = HU.shapes("E2")[0]
    ws = torch.zeros(native.hubert_workspace_bytes(d, 1, sh.wav.shape[1]), dtype=torch.uint8, device=DEV)
    out = torch.zeros(1, 1, cs.H, device=DEV)
    for kw in (dict(), dict(until=("conv0", 0))):
        with pytest.raises(native.EdttsError, match=r"\(code -1\): .*compute_dtype bf16 needs"):  # EDTTS_ERR_UNSUPPORTED
            native.hubert_forward(d, r.blob, sh.wav.to(DEV), None, out, ws, 1, **kw)


@pytest.mark.parametrize("name,dtype", RUNS)
def test_both_gemm_tiles_are_bitwise_equal(name, dtype):
    r = runner(name, dtype)
    cs = r.cs
    for sh in HU.shapes(name):
        if sh.until == ("conv0", 0):
            continue  # (no GEMM site)
        n = 0
        for key in HU.site_list(cs, r.bf, sh.lengths is not None, sh.until):
            if key[0] not in native.HUB_GEMM_SITES:
                continue
            rows = live_rows(cs, sh, key).to(DEV)
            a, b, c = (r.output(sh, key, tile) for tile in (0, 2, 4))
            a, b, c = (v[rows.expand_as(v)] for v in (a, b, c))  # (every GEMM site's output is [B][rows][channels])
            assert not bool(torch.isnan(a.float()).any()), (name, sh.tag, key)
            assert torch.equal(a, b) and torch.equal(b, c), (name, sh.tag, dtype, key)
            n += 1
        assert n == len(cs.C) - 1 + (0 if sh.until else 2 + 4 * cs.layers)
        print(f"hubert tiles {name} {sh.tag} {dtype}: {n} GEMM sites bitwise equal under tile 0, 2 and 4")


def test_the_rule_itself_picks_the_wide_tile_on_a1():
    """A1's conv1: ceil(8100 / 128) x ceil(72 / 128) x 8 = 512 tiles of 128 and N = 72 > 64: tile 0 is the 128 tile there (audited by
    test_every_site_within_its_bar), and it equals the forced 64 tile bitwise."""
    r = runner("A1", "fp32")
    sh, = HU.shapes("A1")
    T1 = HU.stage_frames(r.cs, sh.wav.shape[1])[1]
    assert T1 >= 8100 and (T1 + 127) // 128 * sh.wav.shape[0] >= 512 and r.cs.C[1] > 64
    assert (HU.stage_frames(r.cs, sh.wav.shape[1])[0] + 255) // 256 == 64  # GroupNorm chunks
    assert torch.equal(r.output(sh, ("conv", 1), 0), r.output(sh, ("conv", 1), 2))


@pytest.mark.parametrize("name,dtype", [x for x in RUNS if x[0] != "A1"])
def test_stopping_at_the_last_site_is_the_plain_forward(name, dtype):
    r = runner(name, dtype)
    for sh in HU.shapes(name):
        if sh.until is not None:
            continue
        last = native.hubert_last_site(r.dims, sh.lengths is not None)
        _, stopped = r.run(sh, last)
        B, T_audio = sh.wav.shape
        wav, lens = sh.wav.to(DEV), None if sh.lengths is None else sh.lengths.to(DEV)
        plain = torch.empty_like(stopped)
        native.hubert_forward(r.dims, r.blob, wav, lens, plain, r.m.workspace(B, T_audio, DEV), r.dt)
        called = r.m(wav, lens)
        live = live_rows(r.cs, sh, last).to(DEV).expand_as(plain)  # (rows past a count are 0 after ZERO: all rows compare)
        assert not bool(torch.isnan(plain).any())
        assert torch.equal(stopped, plain) and torch.equal(plain, called), (name, sh.tag, dtype)
        assert float(plain[~live].abs().sum()) == 0.0


@pytest.mark.parametrize("name,dtype", [(c, d) for c in ("E1", "E3") for d in DTYPES])
def test_the_fixtures_invariances_hold_on_e1_and_e3(name, dtype):
    """Batch row = the B = 1 call; ragged row = the solo call on the trimmed waveform; NaN past the lengths changes nothing."""
    r = runner(name, dtype)
    cs, m = r.cs, r.m
    sh = [s for s in HU.shapes(name) if s.tag == "ragged"][0]
    junk = sh.wav.to(DEV)
    B, T_audio = junk.shape
    read = sh.lengths.clamp(HU.samples_for(cs, 1), T_audio)  # the samples the kernels read (both clamps)
    clean = torch.where(torch.arange(T_audio)[None, :] < read[:, None], sh.wav, 0.1 * torch.ones_like(sh.wav)).to(DEV)
    assert bool(torch.isnan(junk).any()) and not bool(torch.isnan(clean).any())
    full = m(clean)
    for b in range(B):
        assert torch.equal(m(clean[b:b + 1].clone())[0], full[b]), f"row {b}"
    lens = sh.lengths.to(DEV)
    out = m(clean, lens)
    assert torch.equal(out, m(junk, lens))
    seen = []
    for b, n in enumerate(read.tolist()):
        F = m.frames(n)
        solo = m(clean[b:b + 1, :n].clone())[0]
        assert solo.shape[0] == F and torch.equal(out[b, :F], solo), f"row {b}"
        assert float(out[b, F:].abs().sum()) == 0.0
        seen.append(F)
    assert seen == [65, 65, 33, 1]


def test_refusals_of_the_new_arguments():
    r = runner("E1", "fp32")
    sh = HU.shapes("E1")[0]
    B, T_audio = sh.wav.shape
    wav = sh.wav.to(DEV)
    ws = torch.zeros(native.hubert_workspace_bytes(r.dims, B, T_audio), dtype=torch.uint8, device=DEV)
    out = torch.zeros(B, 1, r.cs.H, device=DEV)
    lens = torch.tensor([T_audio], device=DEV)

    def call(until, tile=0, lengths=None):
        native.hubert_forward(r.dims, r.blob, wav, lengths, out, ws, 0, until=until, tile=tile)

    for until, tile, lengths, words in ((("vt", 0), 0, None, "EDTTS_HUB_VT exists only under EDTTS_HUBERT_BF16"),
                                        (("lens", 0), 0, None, "EDTTS_HUB_LENS exists only with lengths"),
                                        (("zero", 0), 0, None, "EDTTS_HUB_ZERO exists only with lengths"),
                                        (("conv", 0), 0, None, "EDTTS_HUB_CONV: stop_index=0"),
                                        (("conv", 3), 0, None, "EDTTS_HUB_CONV: stop_index=3"),
                                        (("qkv", 2), 0, None, "EDTTS_HUB_QKV: stop_index=2"),
                                        (("ln2", -1), 0, None, "EDTTS_HUB_LN2: stop_index=-1"),
                                        (("fproj", 1), 0, None, "EDTTS_HUB_FPROJ has no index"),
                                        ((17, 0), 0, None, "stop_site=17"),
                                        ((-1, 0), 0, None, "stop_site=-1"),
                                        (("conv0", 0), 3, None, "tile=3"),
                                        (("conv0", 0), 8, lens, "tile=8")):
        with pytest.raises(native.EdttsError, match="edtts_hubert_forward_until.*" + words.replace("(", r"\(")):
            call(until, tile, lengths)
    call(("zero", 0), 0, lens)  # ... and what exists is accepted
    call(("ln2", 1), 4)
    torch.cuda.synchronize()
    # T0 = 4 conv0 frames leave E1's stack no output frame: the library refuses the call (the smallest audited T0 is 5)
    with pytest.raises(native.EdttsError, match="gives no output frame"):
        native.hubert_workspace_bytes(r.dims, 1, 3 * r.cs.S[0] + r.cs.K[0])
