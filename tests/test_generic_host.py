"""The generic (run-time-shape) kernel path, host side: kernel-path selection, its validation and the size queries that follow
it.  No GPU needed: the size queries and the layout decision run on the host (include/edtts.h: EDTTS_KERNELS_*)."""
import pytest

from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, native


def dec(kernels="compiled", compute_dtype="f32", **kw):
    return EdgeDiffusionDecoder(CFG(device="cpu", **kw), compute_dtype=compute_dtype, kernels=kernels)


def sizes(d, B=2, T=96, S=48, rows=4):
    return native.packed_bytes(d.dims()), native.workspace_bytes(d.dims(), B, T, S, rows)


def test_kernels_option_is_validated():
    assert dec().kernels == "compiled"
    with pytest.raises(ValueError, match="kernels must be one of"):
        dec("fast")
    for k in ("generic", "auto"):
        with pytest.raises(ValueError, match="fp32 only"):
            dec(k, "bf16", hidden=256, heads=8)
    dec("compiled", "bf16", hidden=256, heads=8)  # today's bf16 path is untouched


def test_dims_carry_the_kernel_bits():
    assert dec().dims().compute_dtype == 0
    assert dec("generic").dims().compute_dtype == native.KERNELS["generic"] == 0x100
    assert dec("auto").dims().compute_dtype == native.KERNELS["auto"] == 0x200
    assert dec("compiled", "bf16", hidden=256, heads=8).dims().compute_dtype == 1


def test_shape_without_instance_sizes_on_the_generic_path():
    kw = dict(hidden=100, heads=4, n_mels=100, semantic_dim=24)
    packed, ws = sizes(dec("generic", **kw))
    assert packed > 0 and ws > 0
    assert sizes(dec("auto", **kw)) == (packed, ws)
    with pytest.raises(native.EdttsError, match="need hidden"):  # compiled mode: exactly today's refusal
        native.workspace_bytes(dec(**kw).dims(), 1, 32, 16, 1)
    # the workspace grows with the batch, the packed blob does not depend on it
    assert native.workspace_bytes(dec("generic", **kw).dims(), 8, 96, 48, 4) > ws


def test_auto_picks_the_compiled_instance_when_there_is_one():
    assert sizes(dec("auto")) == sizes(dec())  # 160/4/80: built in
    kw = dict(hidden=224, heads=7)  # no instance: the generic layout
    assert sizes(dec("auto", **kw)) == sizes(dec("generic", **kw))
    assert sizes(dec("generic", **kw)) != sizes(dec(**kw))
    # a generic call runs on the caller's stream alone (no sub-batches); the fused one cuts large batches
    assert native.substreams_for(dec("generic").dims(), 256, 512) == 1


@pytest.mark.parametrize("kw, msg", [
    (dict(hidden=100, heads=3), "hidden % heads"),
    (dict(hidden=258, heads=2), "head_dim=129 > 128"),
    (dict(ffn_mult=5), "ffn_mult"),
])
def test_generic_limits(kw, msg):
    with pytest.raises(native.EdttsError, match=msg):
        native.packed_bytes(dec("generic", **kw).dims())


def test_generic_accepts_odd_widths_and_any_window():
    for kw in (dict(hidden=50, heads=5, n_mels=45, semantic_dim=7), dict(hidden=256, heads=2, attn_window_size=None),
               dict(hidden=96, heads=4, attn_window_size=5, ffn_mult=3), dict(hidden=4, heads=1, n_mels=1, semantic_dim=1)):
        assert min(sizes(dec("generic", **kw))) > 0, kw


def test_bad_kernel_bits_are_refused_by_the_library():
    d = dec("generic", hidden=50, heads=5).dims()
    d.hidden, d.heads = 51, 3  # (the host's positional tables cannot be built for an odd width either)
    with pytest.raises(native.EdttsError, match="even hidden"):
        native.packed_bytes(d)
    d = dec().dims()
    d.compute_dtype = 0x300
    with pytest.raises(native.EdttsError, match="exclusive"):
        native.packed_bytes(d)
    d.compute_dtype = 1 | 0x100
    with pytest.raises(native.EdttsError, match="fp32 only"):
        native.packed_bytes(d)
