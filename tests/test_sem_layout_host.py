"""The host side of the semantic head's training, FSQ and VQ, written once: the library answers the byte counts
and the refusals that were recorded from the library before the merge, and edtts_sem_train_region answers the layouts that
include/edtts.h documents.  No GPU: every call here returns before any HIP call."""
import ctypes as C
import json

import pytest

import sem_layout_util as LU
from edge_diffusion_tts_amd import native


def test_layouts_and_refusals_are_the_recorded_ones():
    """tests/golden/sem_train_layout.json, recorded from the parent's library through the six byte-count queries and the entry points'
    refusals: every size, every code and every text, exactly."""
    with open(LU.GOLDEN) as f:
        want = json.load(f)
    got = LU.records()
    assert len(want["layouts"]) == 10 * (1 + len(LU.EXTRA_SHAPES)) and len(want["refusals"]) == 186
    for part in ("layouts", "refusals"):
        assert sorted(got[part]) == sorted(want[part])
        for key in want[part]:
            assert got[part][key] == want[part][key], key
    # the figures read from the parent by hand
    spot = {"H1 2x37": (81920, 80512, 240464), "H4 2x33": (4096, 4224, 25472), "H5 4x175": (24576, 403200, 1268704),
            "V1 2x37": (65536, 113960, 455264), "V3 2x33": (0, 8712, 3088), "V4 4x175": (16384, 540400, 1016304)}
    for key, (blob, tape, scratch) in spot.items():
        assert want["layouts"][key] == {"blob": blob, "tape": tape, "scratch": scratch}, key
    assert want["layouts"]["V1 16x1500"]["scratch"] == 74477072
    assert all(want["layouts"][f"H{i} 0x5"]["tape"] == 0 for i in range(1, 6))


def documented(dims, B, T, vq):
    """include/edtts.h (edtts_sem_train_region) restated: ([(tape member, floats)], [(scratch member, floats)]) in memory order."""
    in_dim, S, M = dims.in_dim, dims.semantic_dim, B * T
    K = dims.codebook_size
    proj = [("y1", M * S), ("z", M * S)] if in_dim else []
    tape = proj + ([("r", M * S), ("sq", M)] if vq else [("zb", 16 * M)])
    rows = native.train_dw_slab_rows(M)
    ns = (M + rows - 1) // rows
    part = 0
    if ns > 1:  # the slab partials of a cut sum over frames: code sums [K][S], or dW of proj_down / proj_up, and proj's dW
        part = ns * S * (K if vq else 16)
        if in_dim:
            part = max(part, ns * S * max(S, in_dim))
    if not vq or in_dim:
        part = max(part, (M + 255) // 256 * S)              # bias partials
    if in_dim:
        part = max(part, B * ((T + 63) // 64) * 3 * S)      # LayerNorm partials
    wide = [(n, M * S) for n in ("a", "dam", "xh", "dy1")] + [("stat", 2 * M)] if in_dim else []
    if vq:
        scratch = [("coef", 4), ("csum", K * S)] + ([("dz", M * S)] if in_dim else []) + wide
    else:
        scratch = [("du", 16 * M), ("zql", 16 * M), ("dz", M * S), ("gm", M * S)] + wide
    return tape, scratch + [("part", part)]


@pytest.mark.parametrize("name", sorted(LU.heads()))
def test_regions_are_the_documented_layouts(name):
    """Every member's offset and extent is what the header documents, the members tile [0, total) in order without overlap (tape:
    back to back; scratch: every member on a multiple of 4 floats), and what the head does not have is refused by name."""
    dims, B0, T0, vq = LU.heads()[name]
    tape_bytes, scratch_bytes = ((native.sem_vq_tape_bytes, native.sem_vq_scratch_bytes) if vq else
                                 (native.sem_train_tape_bytes, native.sem_train_scratch_bytes))
    for B, T in ((B0, T0),) + LU.EXTRA_SHAPES:
        tape, scratch = documented(dims, B, T, vq)
        for kind, members, total, step in (("tape", tape, tape_bytes(dims, B, T), 4), ("scratch", scratch, scratch_bytes(dims, B, T), 16)):
            at = 0
            for member, floats in members:
                off, n = native.sem_train_region(dims, B, T, f"{kind}.{member}")
                assert (off, n) == (at, 4 * floats), (name, B, T, kind, member)
                at = off + (n + step - 1) // step * step
            assert at == total, (name, B, T, kind)
        if vq and dims.in_dim:  # where _VQGrad reads z for the EMA update
            assert native.sem_train_region(dims, B, T, "tape.z") == (B * T * dims.semantic_dim * 4,) * 2
        have = {f"tape.{m}" for m, _ in tape} | {f"scratch.{m}" for m, _ in scratch}
        for i, which in enumerate(native.SEM_TRAIN_REGIONS):
            if which not in have:
                label = "EDTTS_SEM_" + which.upper().replace(".", "_")
                with pytest.raises(native.EdttsError, match=rf"code -2\): edtts_sem_train_region: {label} is not a member of this head's layout"):
                    native.sem_train_region(dims, B, T, i)
    assert {"tape.r", "tape.sq", "scratch.coef", "scratch.csum"} <= have if vq else {"tape.zb", "scratch.du", "scratch.zql", "scratch.gm"} <= have


def test_region_query_refusals():
    L = native.lib()
    assert len(native.SEM_TRAIN_REGIONS) == 17 and L.edtts_version() == 400
    fsq, vq = native.sem_dims(64, 32, [3, 3]), native.sem_dims(64, 32, None, 128)
    off, n = C.c_size_t(0), C.c_size_t(0)
    for which in (-1, 17):
        with pytest.raises(native.EdttsError, match=r"edtts_sem_train_region: which=-?\d+: expected an EDTTS_SEM_TAPE_\* / EDTTS_SEM_SCRATCH_\* member"):
            native.sem_train_region(fsq, 1, 5, which)
    for args in ((None, C.byref(n)), (C.byref(off), None)):
        with pytest.raises(native.EdttsError, match="offset_bytes/bytes is NULL"):
            L.edtts_sem_train_region(C.byref(vq), 1, 5, 0, *args)
    for B, T in ((-1, 1), (1, -1), (1 << 16, 1 << 16)):
        with pytest.raises(native.EdttsError, match="out of range"):
            native.sem_train_region(vq, B, T, "tape.z")
    with pytest.raises(native.EdttsError, match="semantic_dim=24"):
        native.sem_train_region(native.sem_dims(64, 24, [3, 3]), 1, 5, "tape.z")
    with pytest.raises(native.EdttsError, match="EDTTS_SEM_FSQ with a proj"):
        native.sem_train_region(fsq, 1, 5, "tape.r")
    with pytest.raises(native.EdttsError, match="EDTTS_SEM_VQ without a proj"):
        native.sem_train_region(native.sem_dims(0, 32, None, 128), 1, 5, "scratch.dz")
