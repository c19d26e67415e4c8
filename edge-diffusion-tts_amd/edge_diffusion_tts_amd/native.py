"""ctypes binding of libedtts_hip.so (C ABI declared in include/edtts.h).

This is the only door between the Python host classes and the HIP kernels: no other module of the package imports ctypes or
calls lib().  Every export is bound from one table (_ABI) that tests/test_abi_host.py compares with the header.  There is NO
fallback: if the shared library is missing, or a tensor is not a contiguous tensor of the expected dtype on a HIP device, the call
raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import List, Optional, Sequence, Tuple

import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EDTTS_LIB", os.path.join(os.path.dirname(_PKG_DIR), "lib", "libedtts_hip.so"))

# bits of the index-error word (include/edtts.h: EDTTS_IDX_*)
EDTTS_IDX_SEM, EDTTS_IDX_STEP, EDTTS_IDX_LEN = 1, 2, 4


class _Dims(C.Structure):
    """A dims struct compares by value: _cache.PackedBlob keys a packed blob by the dims it was packed for."""

    def __eq__(self, other):
        return type(other) is type(self) and bytes(self) == bytes(other)

    def __hash__(self):
        return hash(bytes(self))


class EdttsDims(_Dims):
    _fields_ = [(n, C.c_int32) for n in (
        "hidden", "layers", "heads", "n_mels", "ffn_mult", "codebook_size", "semantic_dim", "window", "max_pos",
        "max_ctx_pos", "n_step_emb", "compute_dtype")]


class EdttsDropout(C.Structure):
    """include/edtts.h: EdttsDropout -- drop probability and Philox key of one training forward and its backward."""
    _fields_ = [("p", C.c_float), ("seed", C.c_uint64)]


class EdttsDropoutDev(C.Structure):
    """include/edtts.h: EdttsDropoutDev -- drop probability (host) and a pointer to the Philox key in device memory."""
    _fields_ = [("p", C.c_float), ("key", C.c_void_p)]


DROP_SITES = {"attn": 0, "cross_attn": 1, "ffn_act": 2, "ffn_out": 3}  # include/edtts.h, "Dropout masks": site ids


SEM_FSQ, SEM_VQ = 0, 1  # EdttsSemDims.quantizer (include/edtts.h: EDTTS_SEM_*)


class EdttsSemDims(_Dims):
    _fields_ = [("in_dim", C.c_int32), ("semantic_dim", C.c_int32), ("quantizer", C.c_int32), ("codebook_size", C.c_int32),
                ("n_levels", C.c_int32), ("levels", C.c_int32 * 16)]


def sem_dims(in_dim: int, semantic_dim: int, levels: Optional[Sequence[int]] = None, codebook_size: int = 0) -> EdttsSemDims:
    """Dims of a semantic head: FSQ when `levels` is given, VQ with `codebook_size` codes otherwise; in_dim 0 = no proj."""
    d = EdttsSemDims()
    d.in_dim, d.semantic_dim = int(in_dim), int(semantic_dim)
    if levels is not None:
        levels = [int(v) for v in levels]
        d.quantizer, d.n_levels = SEM_FSQ, len(levels)  # more than 16: the library rejects it with its own message
        for i, v in enumerate(levels[:16]):
            d.levels[i] = v
    else:
        d.quantizer, d.codebook_size = SEM_VQ, int(codebook_size)
    return d


class EdttsOptimState(C.Structure):
    """include/edtts.h: EdttsOptimState -- the head of an optimiser scratch."""
    _fields_ = [("step", C.c_int64), ("skipped", C.c_int64), ("total_norm", C.c_float), ("clip_coef", C.c_float), ("skip", C.c_int32),
                ("reserved", C.c_int32)]


class EdttsOptimGroup(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")]


class EdttsOptimTensor(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("p", "g", "m", "v", "ema", "mirror", "ema_mirror")] + [
        ("numel", C.c_int64), ("group", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("ema_decay", C.c_float)]


class EdttsOptimSchedule(C.Structure):
    """include/edtts.h: EdttsOptimSchedule -- the learning-rate schedule a resident step evaluates on the device."""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("base_lr", C.c_double), ("min_lr", C.c_double),
                ("warmup_steps", C.c_int64), ("total_steps", C.c_int64)]


OPT_CLIP, OPT_SKIP_NONFINITE, OPT_ZERO_GRADS, OPT_EMA_ONLY = 1, 2, 4, 8  # include/edtts.h: EDTTS_OPT_*
# layout facts for callers that read a table back as bytes (optim.py): record sizes and (name, offset, size) of every field
OPTIM_GROUP_BYTES, OPTIM_TENSOR_BYTES = C.sizeof(EdttsOptimGroup), C.sizeof(EdttsOptimTensor)
OPTIM_GROUP_LR_OFFSET = EdttsOptimGroup.lr.offset
OPTIM_TENSOR_FIELDS = tuple((n, getattr(EdttsOptimTensor, n).offset, getattr(EdttsOptimTensor, n).size) for n, _ in EdttsOptimTensor._fields_)
EDTTS_SCHED_NONE, EDTTS_SCHED_COSINE = 0, 1
KEY_STREAM = 0x50000  # include/edtts.h, "Philox stream ids": the key stream's word
EDTTS_OBJ_V, EDTTS_OBJ_EPS, EDTTS_OBJ_DISTILL, EDTTS_OBJ_CONSISTENCY = 0, 1, 2, 3  # include/edtts.h: the kinds of edtts_objective_loss
OBJ_NOISE_STREAM = 0x54  # include/edtts.h, "Philox stream ids": training q_sample noise


class EdttsHubertDims(_Dims):
    _fields_ = [("n_conv", C.c_int32), ("conv_dim", C.c_int32 * 16), ("conv_kernel", C.c_int32 * 16), ("conv_stride", C.c_int32 * 16),
                ("hidden", C.c_int32), ("heads", C.c_int32), ("intermediate", C.c_int32), ("num_layers", C.c_int32),
                ("pos_kernel", C.c_int32), ("pos_groups", C.c_int32), ("layer_norm_eps", C.c_float)]


COMPUTE_DTYPES = {"f32": 0, "fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1}
# kernel-path bits ORed into EdttsDims.compute_dtype (include/edtts.h: EDTTS_KERNELS_*): "compiled" = the shape's compiled instance
# only (an unlisted shape is EDTTS_ERR_UNSUPPORTED), "generic" = the run-time-shape fp32 kernels, "auto" = compiled when built
KERNELS = {"compiled": 0, "generic": 0x100, "auto": 0x200}
# matmul-precision bit of EdttsDims.compute_dtype (include/edtts.h): every `linear` of the generic path on bf16 MFMAs, storage fp32
EDTTS_MATMUL_BF16 = 0x400
MATMUL_DTYPES = {"f32": 0, "fp32": 0, "float32": 0, "bf16": EDTTS_MATMUL_BF16, "bfloat16": EDTTS_MATMUL_BF16}
# attention-precision bit (include/edtts.h): both attentions' contractions, forward and backward, on bf16 MFMAs, storage fp32
EDTTS_ATTN_BF16 = 0x800
ATTN_DTYPES = {"f32": 0, "fp32": 0, "float32": 0, "bf16": EDTTS_ATTN_BF16, "bfloat16": EDTTS_ATTN_BF16}
# activation-storage bit (include/edtts.h): q|k|v, the cross queries, the cross K|V and the SwiGLU output stored as bf16; only with both
# bits above
EDTTS_TAPE_BF16 = 0x1000
TAPE_DTYPES = {"f32": 0, "fp32": 0, "float32": 0, "bf16": EDTTS_TAPE_BF16, "bfloat16": EDTTS_TAPE_BF16}
# the per-layer members of the training tape, as edtts_train_tape_region names them (include/edtts.h: EDTTS_TAPE_*)
TAPE_REGIONS = ("crp", "kv", "h0", "h1", "h2", "qkv", "att1", "lse1", "qc", "att2", "lse2", "act")
(EDTTS_TAPE_CRP, EDTTS_TAPE_KV, EDTTS_TAPE_H0, EDTTS_TAPE_H1, EDTTS_TAPE_H2, EDTTS_TAPE_QKV, EDTTS_TAPE_ATT1, EDTTS_TAPE_LSE1,
 EDTTS_TAPE_QC, EDTTS_TAPE_ATT2, EDTTS_TAPE_LSE2, EDTTS_TAPE_ACT) = range(12)
TAPE_NARROWED = ("kv", "qkv", "qc", "act")  # what EDTTS_TAPE_BF16 stores as bf16
# the whole-model members (always fp32; edtts_train_tape_region answers the same for every layer)
TAPE_GLOBALS = ("cond", "tcond", "ctx", "hl")
EDTTS_TAPE_COND, EDTTS_TAPE_TCOND, EDTTS_TAPE_CTX, EDTTS_TAPE_HL = range(12, 16)
# the sites of the backward's launch list, as edtts_decoder_backward_until names them (include/edtts.h: EDTTS_BWD_*), in launch
# order: the head, the per-layer sites (layers L-1 .. 0), the tail
BWD_SITES = ("out", "fnorm", "dropdown", "down", "upre", "swiglu", "up", "n3", "op", "cross", "qp", "n2", "kvu", "kvn", "kvd", "proj",
             "self", "qkv", "n1", "inp", "sem", "ada", "step", "time")
BWD_LAYER_SITES = BWD_SITES[2:19]
# the members of the backward's scratch, as edtts_train_scratch_region names them (include/edtts.h: EDTTS_SCRATCH_*)
SCRATCH_REGIONS = ("dh", "xn", "ga", "gq", "big", "da", "stat", "delta", "dkv", "crn", "dcr", "dcp", "dctx", "dmod", "dtc", "e", "a1", "u1",
                   "du1", "part")


class EdttsError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------- the C ABI, one entry per export
# Kinds of return: a status int (0 or a negative EDTTS_ERR_*: lib() gives it _errcheck), a plain int value, a const char*.
_STATUS, _VALUE, _STR = "status", "value", "str"
EDTTS_ERR_ARG = -2  # include/edtts.h: the one error code _errcheck tells apart

vp, i32, i64, u32, u64, sz, f32, f64 = (C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_size_t, C.c_float, C.c_double)
p_vp, p_i32, p_i64, p_sz, p_f32, p_f64 = (C.POINTER(t) for t in (vp, i32, i64, sz, f32, f64))
dp, sdp, hdp, drp, ddp = (C.POINTER(t) for t in (EdttsDims, EdttsSemDims, EdttsHubertDims, EdttsDropout, EdttsDropoutDev))

# include/edtts.h in its order: name -> (kind of return, argument types).  tests/test_abi_host.py compares every entry with the
# header's prototype, so a new export is one prototype there and one line here.
_ABI = {
    "edtts_version": (_VALUE, ()),
    "edtts_last_error": (_STR, ()),
    "edtts_num_global_slots": (_VALUE, ()),
    "edtts_num_layer_slots": (_VALUE, ()),
    "edtts_global_slot_name": (_STR, (i32,)),
    "edtts_layer_slot_name": (_STR, (i32,)),
    "edtts_packed_bytes": (_STATUS, (dp, p_sz)),
    "edtts_pack_weights": (_STATUS, (dp, p_vp, i32, vp, vp)),
    "edtts_workspace_bytes": (_STATUS, (dp, i32, i32, i32, i32, p_sz)),
    "edtts_index_errors": (_STATUS, (vp, p_i32, vp)),
    "edtts_decoder_forward": (_STATUS, (dp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp)),
    "edtts_train_tape_bytes": (_STATUS, (dp, i32, i32, i32, p_sz)),
    "edtts_train_scratch_bytes": (_STATUS, (dp, i32, i32, i32, p_sz)),
    "edtts_train_dw_slab_rows": (_VALUE, (i32,)),
    "edtts_train_tape_region": (_STATUS, (dp, i32, i32, i32, i32, i32, p_sz, p_sz, p_i32)),
    "edtts_decoder_forward_train": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp)),
    "edtts_decoder_backward": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, p_vp, i32, vp, vp, vp, vp)),
    "edtts_decoder_forward_train_drop": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, drp, vp)),
    "edtts_decoder_backward_drop": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, p_vp, i32, vp, vp, vp, drp, vp)),
    "edtts_dropout_mask": (_STATUS, (dp, i32, i32, i32, i32, i32, drp, vp, vp)),
    "edtts_decoder_forward_len": (_STATUS, (dp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp)),
    "edtts_decoder_forward_train_len": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, drp, vp, vp, vp)),
    "edtts_decoder_backward_len": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, p_vp, i32, vp, vp, vp, drp, vp, vp,
                                             vp)),
    "edtts_decoder_backward_until": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, p_vp, i32, vp, vp, vp, drp, vp, vp,
                                               i32, i32, vp)),
    "edtts_train_scratch_region": (_STATUS, (dp, i32, i32, i32, i32, p_sz, p_sz)),
    "edtts_decoder_forward_train_dev": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, ddp, vp, vp, vp)),
    "edtts_decoder_backward_dev": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, p_vp, i32, vp, vp, vp, ddp, vp, vp,
                                             vp)),
    "edtts_dropout_mask_dev": (_STATUS, (dp, i32, i32, i32, i32, i32, ddp, vp, vp)),
    "edtts_ddim_step": (_STATUS, (vp, i32, vp, vp, vp, vp, i32, sz, f32, vp, vp, vp, vp)),
    "edtts_ddpm_step": (_STATUS, (vp, vp, vp, vp, i32, vp, vp, vp, i32, sz, vp, vp, vp)),
    "edtts_generate": (_STATUS, (dp, vp, vp, i32, i32, vp, vp, i32, p_i64, p_f32, vp, vp, vp)),
    "edtts_generate_len": (_STATUS, (dp, vp, vp, i32, i32, vp, vp, vp, i32, p_i64, p_f32, vp, vp, vp)),
    "edtts_sample_ddpm": (_STATUS, (dp, vp, vp, i32, i32, vp, vp, i32, vp, p_f32, vp, u64, i64, vp, vp)),
    "edtts_sample_ddpm_len": (_STATUS, (dp, vp, vp, i32, i32, vp, vp, vp, i32, vp, p_f32, vp, u64, i64, vp, vp)),
    "edtts_randn": (_STATUS, (vp, sz, u64, u32, u64, f32, vp)),
    "edtts_randn_rows": (_STATUS, (vp, i32, sz, vp, u32, f32, vp)),
    "edtts_keys_advance": (_STATUS, (vp, i32, vp, vp)),
    "edtts_keys_host": (_STATUS, (u64, u64, i64, i32, C.POINTER(u64))),
    "edtts_sample_multistep": (_STATUS, (dp, vp, vp, i32, i32, i32, vp, vp, vp, i32, p_i64, p_f32, vp, vp, vp, vp)),
    "edtts_sample_multistep_len": (_STATUS, (dp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, p_i64, p_f32, vp, vp, vp, vp)),
    "edtts_sample_inpaint": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, p_f32, vp, i32, vp, u64, f32, vp, vp)),
    "edtts_sample_inpaint_len": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, p_f32, vp, i32, vp, u64, f32, vp,
                                           vp, vp, vp, vp)),
    "edtts_sample_inpaint_multistep_len": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, p_f32, vp, i32, vp, u64, f32,
                                                     vp, vp, vp, vp, vp, vp, vp)),
    "edtts_sample_inpaint_mask_len": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, p_f32, vp, vp, vp, u64, f32, vp,
                                                vp, vp, vp, vp)),
    "edtts_sample_inpaint_multistep_mask_len": (_STATUS, (dp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, p_f32, vp, vp, vp, u64,
                                                          f32, vp, vp, vp, vp, vp, vp, vp)),
    "edtts_dsconv_scratch_floats": (_STATUS, (i32, i32, i32, i32, i32, i32, i32, p_sz)),
    "edtts_dsconv_forward": (_STATUS, (vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp)),
    "edtts_mel_to_spec": (_STATUS, (vp, vp, vp, vp, i32, i32, i32, i32, vp, vp)),
    "edtts_griffin_lim_scratch_floats": (_STATUS, (i32, i32, i32, i32, p_sz)),
    "edtts_griffin_lim": (_STATUS, (vp, i32, i32, i32, i32, vp, vp, i32, f32, f32, vp, u64, vp, vp, vp)),
    "edtts_mel_to_spec_len": (_STATUS, (vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp)),
    "edtts_griffin_lim_len": (_STATUS, (vp, i32, i32, i32, i32, vp, vp, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp)),
    "edtts_profile_enable": (_STATUS, (i32,)),
    "edtts_profile_collect": (_STATUS, (p_f64, p_i32)),  # arrays of 2
    "edtts_set_substreams": (_VALUE, (i32,)),
    "edtts_substreams_for": (_VALUE, (dp, i32, i32)),
    "edtts_set_coop": (_VALUE, (i32,)),
    "edtts_sem_packed_bytes": (_STATUS, (sdp, p_sz)),
    "edtts_sem_num_codes": (_STATUS, (sdp, p_i64)),
    "edtts_sem_pack": (_STATUS, (sdp, p_vp, i32, vp, vp)),
    "edtts_sem_encode": (_STATUS, (sdp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp)),
    "edtts_sem_decode": (_STATUS, (sdp, vp, vp, i64, vp, vp)),
    "edtts_sem_stats": (_STATUS, (vp, i64, vp, vp, vp)),
    "edtts_sem_train_packed_bytes": (_STATUS, (sdp, p_sz)),
    "edtts_sem_train_pack": (_STATUS, (sdp, p_vp, i32, vp, vp)),
    "edtts_sem_train_tape_bytes": (_STATUS, (sdp, i32, i32, p_sz)),
    "edtts_sem_train_scratch_bytes": (_STATUS, (sdp, i32, i32, p_sz)),
    "edtts_sem_encode_train": (_STATUS, (sdp, vp, vp, i32, i32, vp, vp, vp, vp, vp, drp, vp)),
    "edtts_sem_backward": (_STATUS, (sdp, vp, vp, vp, vp, i32, i32, vp, vp, p_vp, i32, vp, vp, drp, vp)),
    "edtts_sem_dropout_mask": (_STATUS, (sdp, i32, i32, drp, vp, vp)),
    "edtts_sem_encode_train_dev": (_STATUS, (sdp, vp, vp, i32, i32, vp, vp, vp, vp, vp, ddp, vp)),
    "edtts_sem_backward_dev": (_STATUS, (sdp, vp, vp, vp, vp, i32, i32, vp, vp, p_vp, i32, vp, vp, ddp, vp)),
    "edtts_sem_dropout_mask_dev": (_STATUS, (sdp, i32, i32, ddp, vp, vp)),
    "edtts_sem_vq_train_packed_bytes": (_STATUS, (sdp, p_sz)),
    "edtts_sem_vq_train_pack": (_STATUS, (sdp, p_vp, i32, vp, vp)),
    "edtts_sem_vq_tape_bytes": (_STATUS, (sdp, i32, i32, p_sz)),
    "edtts_sem_vq_scratch_bytes": (_STATUS, (sdp, i32, i32, p_sz)),
    "edtts_sem_vq_encode_train": (_STATUS, (sdp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, f64, drp, vp)),
    "edtts_sem_vq_ema_update": (_STATUS, (sdp, vp, vp, i32, i32, vp, vp, f64, f64, vp, vp, vp, vp, vp)),
    "edtts_sem_vq_backward": (_STATUS, (sdp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, f64, p_vp, i32, vp, vp, drp, vp)),
    "edtts_sem_train_region": (_STATUS, (sdp, i32, i32, i32, p_sz, p_sz)),
    "edtts_optim_chunk_size": (_VALUE, ()),
    "edtts_optim_chunk_table": (_STATUS, (p_i64, i32, i32, p_i32, p_i64, p_i32, p_i32)),
    "edtts_optim_scratch_bytes": (_STATUS, (i32, i32, p_sz)),
    "edtts_optim_step": (_STATUS, (C.POINTER(EdttsOptimTensor), i32, C.POINTER(EdttsOptimGroup), i32, f64, i32, vp, sz, vp)),
    "edtts_optim_upload": (_STATUS, (C.POINTER(EdttsOptimTensor), i32, C.POINTER(EdttsOptimGroup), i32, i32, vp, sz, p_i32, p_sz, vp)),
    "edtts_optim_step_resident": (_STATUS, (i32, i32, f64, i32, vp, sz, vp, C.POINTER(EdttsOptimSchedule), vp)),
    "edtts_generic_slot_dest": (_STATUS, (dp, i32, p_sz, p_i32, p_i32, p_i32)),
    "edtts_hubert_frames": (_STATUS, (hdp, i64, p_i64)),
    "edtts_hubert_packed_bytes": (_STATUS, (hdp, p_sz)),
    "edtts_hubert_pack": (_STATUS, (hdp, p_vp, i32, vp, vp)),
    "edtts_hubert_workspace_bytes": (_STATUS, (hdp, i32, i32, p_sz)),
    "edtts_hubert_forward": (_STATUS, (hdp, vp, vp, i32, i32, vp, vp, vp, vp)),
    "edtts_hubert_packed_bytes_dt": (_STATUS, (hdp, i32, p_sz)),
    "edtts_hubert_pack_dt": (_STATUS, (hdp, i32, p_vp, i32, vp, vp)),
    "edtts_hubert_workspace_bytes_dt": (_STATUS, (hdp, i32, i32, i32, p_sz)),
    "edtts_hubert_forward_dt": (_STATUS, (hdp, i32, vp, vp, i32, i32, vp, vp, vp, vp)),
    "edtts_hubert_forward_until": (_STATUS, (hdp, i32, vp, vp, i32, i32, vp, vp, vp, i32, i32, i32, vp)),
    "edtts_hubert_workspace_region": (_STATUS, (hdp, i32, i32, i32, i32, p_sz, p_sz)),
    "edtts_melspec": (_STATUS, (vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, i32, i32, i32, vp, vp)),
    "edtts_mel_segment_stats": (_STATUS, (vp, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp)),
    "edtts_logmel_stats": (_STATUS, (vp, i32, i32, i32, i32, vp, i32, vp, vp, vp)),
    "edtts_resample": (_STATUS, (vp, i32, i32, vp, i32, i32, i32, i32, vp, i64, vp, vp)),
    "edtts_objective_scratch_bytes": (_STATUS, (i32, i32, i32, p_sz)),
    "edtts_objective_stats": (_STATUS, (vp, i32, i32, i32, vp, vp, vp, vp)),
    "edtts_objective_prepare": (_STATUS, (vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp)),
    "edtts_objective_loss": (_STATUS, (i32, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, sz, vp, vp)),
    "edtts_objective_scale": (_STATUS, (vp, vp, sz, vp, vp)),
}
EXPORTED_SYMBOLS = tuple(_ABI)  # every symbol include/edtts.h declares (tests check that the built library exports all of them)

_lib = None


def lib() -> C.CDLL:
    """Load the HIP library (once) and bind every export from _ABI.  Raises if it has not been built -- there is no CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EdttsError(
            f"HIP extension not found at {LIB_PATH}; build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  The sampler path has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name, (kind, argtypes) in _ABI.items():
        fn = getattr(L, name)
        fn.argtypes = list(argtypes)
        fn.restype = C.c_char_p if kind == _STR else C.c_int
        if kind == _STATUS:
            fn.errcheck = _errcheck
    _lib = L
    return L


def _errcheck(rc, func, args):
    if rc != 0:
        msg = _lib.edtts_last_error().decode() if _lib is not None else "?"
        # argument errors: the reference raises ValueError / IndexError / RuntimeError for these
        if rc == EDTTS_ERR_ARG and "Either sem_idx or sem_features" in msg:
            raise ValueError(msg)
        raise EdttsError(f"{func.__name__} failed (code {rc}): {msg}")
    return rc


# ---------------------------------------------------------------------------------------------- helpers
def _dev_ptr(t: Optional[torch.Tensor], dtype: torch.dtype, name: str) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise EdttsError(f"{name}: expected a tensor on the HIP device, got {t.device} -- the MI355X sampler path has no CPU fallback")
    if t.dtype != dtype:
        raise EdttsError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise EdttsError(f"{name}: tensor must be contiguous")
    return t.data_ptr()


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _u64(v: int):
    """A Python int (a seed: any size, any sign) as the uint64 of its low 64 bits."""
    return C.c_uint64(v & 0xFFFFFFFFFFFFFFFF)


def _size_query(fn, *args, ctype=C.c_size_t) -> int:
    """fn(*args, &out) -> out: the library's size and count queries."""
    out = ctype(0)
    fn(*args, C.byref(out))
    return out.value


def _slot_ptrs(tensors: Sequence[Optional[torch.Tensor]], what: str):
    """The void* array of a slot list (fp32 device tensors, None -> NULL); `what` names an entry in error messages."""
    return (C.c_void_p * len(tensors))(*[_dev_ptr(t, torch.float32, f"{what}[{i}]") for i, t in enumerate(tensors)])


def slot_names(n_layers: int) -> List[str]:
    L = lib()
    names = [L.edtts_global_slot_name(i).decode() for i in range(L.edtts_num_global_slots())]
    per = [L.edtts_layer_slot_name(i).decode() for i in range(L.edtts_num_layer_slots())]
    for l in range(n_layers):
        names += [f"layers.{l}.{n}" for n in per]
    return names


def packed_bytes(dims: EdttsDims) -> int:
    return _size_query(lib().edtts_packed_bytes, C.byref(dims))


def workspace_bytes(dims: EdttsDims, B: int, T: int, S: int, cond_rows: int) -> int:
    return _size_query(lib().edtts_workspace_bytes, C.byref(dims), B, T, S, cond_rows)


def pack_weights(dims: EdttsDims, tensors: Sequence[torch.Tensor], packed: torch.Tensor) -> None:
    ptrs = _slot_ptrs(tensors, "weight")
    lib().edtts_pack_weights(C.byref(dims), ptrs, len(tensors), _dev_ptr(packed, torch.uint8, "packed"), _stream(packed.device))


def lengths(n: Optional[torch.Tensor], B: int, hi: int, device, name: str) -> Optional[torch.Tensor]:
    """Per-utterance lengths for the *_len entry points: None, or an int64 [B] tensor.  A CPU tensor is range-checked here
    (ValueError outside [1, hi]) and copied to `device` -- not while the stream is capturing (a host-to-device copy cannot be
    captured: pass a device tensor then).  A device tensor is passed through as it is: the kernels read it at run time (a captured
    graph serves whatever lengths are copied into it later), clamp values outside [1, hi] and set EDTTS_IDX_LEN."""
    if n is None:
        return None
    if not isinstance(n, torch.Tensor):
        raise ValueError(f"{name}: expected an int64 tensor of shape [{B}], got {type(n).__name__}")
    if n.dtype != torch.int64:
        raise ValueError(f"{name}: expected dtype torch.int64, got {n.dtype}")
    if tuple(n.shape) != (B,):
        raise ValueError(f"{name}: expected shape [{B}], got {list(n.shape)}")
    if n.is_cuda:
        if device is not None and torch.device(device).type == "cuda" and n.device != torch.device(device):
            raise ValueError(f"{name}: on {n.device}, the call runs on {device}")
        return n.contiguous()
    if B and (int(n.min()) < 1 or int(n.max()) > hi):
        raise ValueError(f"{name}: lengths must be in [1, {hi}], got [{int(n.min())}, {int(n.max())}]")
    if torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{name}: a CPU length tensor cannot be copied to the device during graph capture; "
                           "pass a device tensor (and copy new lengths into it before each replay)")
    return n.to(device)


def decoder_forward(dims: EdttsDims, packed: torch.Tensor, workspace: torch.Tensor, x: torch.Tensor, t: torch.Tensor,
                    step_idx: Optional[torch.Tensor], sem_idx: Optional[torch.Tensor], sem_features: Optional[torch.Tensor],
                    S: int, t_len: Optional[torch.Tensor] = None, s_len: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-utterance frame / token counts t_len / s_len: device int64 [B] or None (see lengths()).  Without either the plain
    export runs, with them the _len one."""
    B, T, M = x.shape
    eps = torch.empty_like(x)
    head = (C.byref(dims), packed.data_ptr(), workspace.data_ptr(), B, T, S, _dev_ptr(x, torch.float32, "x_t"),
            _dev_ptr(t, torch.int64, "t"), _dev_ptr(step_idx, torch.int64, "step_idx"), _dev_ptr(sem_idx, torch.int64, "sem_idx"),
            _dev_ptr(sem_features, torch.float32, "sem_features"))
    if t_len is None and s_len is None:
        lib().edtts_decoder_forward(*head, eps.data_ptr(), _stream(x.device))
    else:
        lib().edtts_decoder_forward_len(*head, _dev_ptr(t_len, torch.int64, "x_lengths"), _dev_ptr(s_len, torch.int64, "sem_lengths"),
                                        eps.data_ptr(), _stream(x.device))
    check_indices(workspace)
    return eps


# ---------------------------------------------------------------------------------------------- training
def train_tape_bytes(dims: EdttsDims, B: int, T: int, S: int) -> int:
    return _size_query(lib().edtts_train_tape_bytes, C.byref(dims), B, T, S)


def train_tape_region(dims: EdttsDims, B: int, T: int, S: int, layer: int, which) -> tuple:
    """(offset in bytes, bytes, bytes per element) of one member of the training tape; ``which``: a name of TAPE_REGIONS (per layer)
    or TAPE_GLOBALS (whole model: any layer in range gives the same answer), or its EDTTS_TAPE_* number (include/edtts.h:
    edtts_train_tape_region)."""
    if isinstance(which, str):
        which = (TAPE_REGIONS + TAPE_GLOBALS).index(which)
    off, n, eb = sz(), sz(), i32()
    lib().edtts_train_tape_region(C.byref(dims), B, T, S, int(layer), int(which), C.byref(off), C.byref(n), C.byref(eb))
    return int(off.value), int(n.value), int(eb.value)


def train_scratch_bytes(dims: EdttsDims, B: int, T: int, S: int) -> int:
    return _size_query(lib().edtts_train_scratch_bytes, C.byref(dims), B, T, S)


def train_scratch_region(dims: EdttsDims, B: int, T: int, S: int, which) -> tuple:
    """(offset in bytes, bytes) of one member of the backward's scratch (all fp32); ``which``: a name of SCRATCH_REGIONS or its
    EDTTS_SCRATCH_* number (include/edtts.h: edtts_train_scratch_region; a diagnostic query)."""
    if isinstance(which, str):
        which = SCRATCH_REGIONS.index(which)
    off, n = sz(), sz()
    lib().edtts_train_scratch_region(C.byref(dims), B, T, S, int(which), C.byref(off), C.byref(n))
    return int(off.value), int(n.value)


def train_dw_slab_rows(rows: int) -> int:
    """Rows per partial slab of a weight gradient that sums over `rows` rows (include/edtts.h: edtts_train_dw_slab_rows)."""
    return int(lib().edtts_train_dw_slab_rows(int(rows)))


class DropKey:
    """Dropout with its Philox key in device memory: drop probability ``p`` (a host value) and ``key``, a 1-element int64 device
    tensor (a KeyStream slot) that the kernels read when they run (include/edtts.h: EdttsDropoutDev)."""

    def __init__(self, p: float, key: torch.Tensor):
        if not isinstance(key, torch.Tensor) or key.dtype != torch.int64 or key.numel() != 1 or not key.is_cuda:
            raise EdttsError("DropKey: key must be a 1-element int64 tensor on the HIP device")
        self.p, self.key = float(p), key

    def struct(self) -> EdttsDropoutDev:
        return EdttsDropoutDev(self.p, self.key.data_ptr())


def _dropout(drop):
    """None, an EdttsDropout, a (p, seed) pair or a DropKey -> None, an EdttsDropout or an EdttsDropoutDev."""
    if drop is None or isinstance(drop, (EdttsDropout, EdttsDropoutDev)):
        return drop
    if isinstance(drop, DropKey):
        return drop.struct()
    p, seed = drop
    return EdttsDropout(float(p), int(seed))


def decoder_forward_train(dims: EdttsDims, packed: torch.Tensor, workspace: torch.Tensor, tape: torch.Tensor, x: torch.Tensor,
                          t: torch.Tensor, step_idx: Optional[torch.Tensor], sem_idx: Optional[torch.Tensor],
                          sem_features: Optional[torch.Tensor], S: int, drop=None, t_len: Optional[torch.Tensor] = None,
                          s_len: Optional[torch.Tensor] = None) -> torch.Tensor:
    """edtts_decoder_forward_train: eps, with the backward's tape written to `tape` (uint8, train_tape_bytes).  ``drop``: None (the
    plain export), or an EdttsDropout / (p, seed) pair -> edtts_decoder_forward_train_drop, or a DropKey ->
    edtts_decoder_forward_train_dev.  ``t_len`` / ``s_len``: per-utterance frame / token counts, device int64 [B] or None (see
    lengths()); with either, edtts_decoder_forward_train_len runs."""
    B, T, M = x.shape
    eps = torch.empty_like(x)
    drop = _dropout(drop)
    args = (C.byref(dims), packed.data_ptr(), workspace.data_ptr(), _dev_ptr(tape, torch.uint8, "tape"), B, T, S,
            _dev_ptr(x, torch.float32, "x_t"), _dev_ptr(t, torch.int64, "t"), _dev_ptr(step_idx, torch.int64, "step_idx"),
            _dev_ptr(sem_idx, torch.int64, "sem_idx"), _dev_ptr(sem_features, torch.float32, "sem_features"), eps.data_ptr())
    if isinstance(drop, EdttsDropoutDev):
        lib().edtts_decoder_forward_train_dev(*args, C.byref(drop), _dev_ptr(t_len, torch.int64, "x_lengths"),
                                              _dev_ptr(s_len, torch.int64, "sem_lengths"), _stream(x.device))
    elif t_len is not None or s_len is not None:
        lib().edtts_decoder_forward_train_len(*args, None if drop is None else C.byref(drop), _dev_ptr(t_len, torch.int64, "x_lengths"),
                                              _dev_ptr(s_len, torch.int64, "sem_lengths"), _stream(x.device))
    elif drop is None:
        lib().edtts_decoder_forward_train(*args, _stream(x.device))
    else:
        lib().edtts_decoder_forward_train_drop(*args, C.byref(drop), _stream(x.device))
    check_indices(workspace)
    return eps


def decoder_backward(dims: EdttsDims, packed: torch.Tensor, workspace: torch.Tensor, tape: torch.Tensor, x: torch.Tensor, t: torch.Tensor,
                     step_idx: Optional[torch.Tensor], sem_idx: Optional[torch.Tensor], sem_features: Optional[torch.Tensor], S: int,
                     d_eps: torch.Tensor, grads: Sequence[Optional[torch.Tensor]], d_x: Optional[torch.Tensor],
                     d_sem_features: Optional[torch.Tensor], drop=None, t_len: Optional[torch.Tensor] = None,
                     s_len: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None, until=None) -> None:
    """edtts_decoder_backward: writes the gradient of every non-None entry of `grads` (slot order), d_x and d_sem_features.
    ``drop``: what the forward that filled `tape` was given (None: the plain export, else edtts_decoder_backward_drop).
    ``t_len`` / ``s_len``: the lengths that forward was given (device int64 [B] or None; with either, edtts_decoder_backward_len
    runs).  ``scratch``: the caller's own (uint8, at least train_scratch_bytes) instead of one allocated here.
    ``until``: (layer, site) -- edtts_decoder_backward_until: the same launches, stopped after the last one of that site (a name of
    BWD_SITES or its EDTTS_BWD_* number; layer 0 for the head's and the tail's sites).  A diagnostic; not with a DropKey."""
    B, T, M = x.shape
    ptrs = _slot_ptrs(grads, "grad")
    nbytes = train_scratch_bytes(dims, B, T, S)
    if scratch is None:
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    elif _dev_ptr(scratch, torch.uint8, "scratch") is None or scratch.numel() < nbytes:
        raise EdttsError(f"scratch: expected at least {nbytes} bytes, got {scratch.numel()}")
    drop = _dropout(drop)
    args = (C.byref(dims), packed.data_ptr(), workspace.data_ptr(), _dev_ptr(tape, torch.uint8, "tape"), B, T, S,
            _dev_ptr(x, torch.float32, "x_t"), _dev_ptr(t, torch.int64, "t"), _dev_ptr(step_idx, torch.int64, "step_idx"),
            _dev_ptr(sem_idx, torch.int64, "sem_idx"), _dev_ptr(sem_features, torch.float32, "sem_features"),
            _dev_ptr(d_eps, torch.float32, "d_eps"), ptrs, len(grads), _dev_ptr(d_x, torch.float32, "d_x"),
            _dev_ptr(d_sem_features, torch.float32, "d_sem_features"), scratch.data_ptr())
    if until is not None:
        if isinstance(drop, EdttsDropoutDev):
            raise EdttsError("decoder_backward: until= takes an EdttsDropout or a (p, seed) pair, not a DropKey")
        layer, site = until
        if isinstance(site, str):
            site = BWD_SITES.index(site)
        lib().edtts_decoder_backward_until(*args, None if drop is None else C.byref(drop), _dev_ptr(t_len, torch.int64, "x_lengths"),
                                           _dev_ptr(s_len, torch.int64, "sem_lengths"), int(layer), int(site), _stream(x.device))
    elif isinstance(drop, EdttsDropoutDev):
        lib().edtts_decoder_backward_dev(*args, C.byref(drop), _dev_ptr(t_len, torch.int64, "x_lengths"),
                                         _dev_ptr(s_len, torch.int64, "sem_lengths"), _stream(x.device))
    elif t_len is not None or s_len is not None:
        lib().edtts_decoder_backward_len(*args, None if drop is None else C.byref(drop), _dev_ptr(t_len, torch.int64, "x_lengths"),
                                         _dev_ptr(s_len, torch.int64, "sem_lengths"), _stream(x.device))
    elif drop is None:
        lib().edtts_decoder_backward(*args, _stream(x.device))
    else:
        lib().edtts_decoder_backward_drop(*args, C.byref(drop), _stream(x.device))


def dropout_mask(dims: EdttsDims, site: int, layer: int, B: int, T: int, S: int, p: float, seed, device="cuda") -> torch.Tensor:
    """edtts_dropout_mask: the keep mask (uint8, 1 = kept) of one dropout site of one layer, from the device functions the training
    kernels call: [B, heads, T, T] (site 0), [B, heads, T, S] (1), [B * T, ffn_mult * hidden] (2) or [B * T, hidden] (3).  ``seed``: an
    int, or a 1-element int64 device tensor holding it (edtts_dropout_mask_dev)."""
    shape = {0: (B, dims.heads, T, T), 1: (B, dims.heads, T, S), 2: (B * T, dims.ffn_mult * dims.hidden), 3: (B * T, dims.hidden)}.get(int(site))
    if shape is None:
        raise ValueError(f"site must be one of 0 .. 3 (DROP_SITES), got {site!r}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise EdttsError(f"dropout_mask: expected a HIP device, got {dev} -- there is no CPU fallback")
    keep = torch.empty(shape, dtype=torch.uint8, device=dev)
    if isinstance(seed, torch.Tensor):
        drop = DropKey(p, seed).struct()
        lib().edtts_dropout_mask_dev(C.byref(dims), int(site), int(layer), B, T, S, C.byref(drop), keep.data_ptr(), _stream(dev))
    else:
        drop = EdttsDropout(float(p), int(seed))
        lib().edtts_dropout_mask(C.byref(dims), int(site), int(layer), B, T, S, C.byref(drop), keep.data_ptr(), _stream(dev))
    return keep


def generate(dims: EdttsDims, packed: torch.Tensor, workspace: torch.Tensor, sem_idx: torch.Tensor, x_T: torch.Tensor,
             timesteps: Sequence[int], coefs: Sequence[Tuple[float, float, float, float]],
             s_len: Optional[torch.Tensor] = None) -> torch.Tensor:
    """s_len: per-utterance token counts (device int64 [B] or None: the plain export); utterance b has 2 * s_len[b] frames."""
    B, S = sem_idx.shape
    n = len(timesteps)
    ts = (C.c_int64 * n)(*[int(v) for v in timesteps])
    cf = (C.c_float * (4 * n))(*[float(v) for c in coefs for v in c])
    x_work = torch.empty_like(x_T)
    x0 = torch.empty_like(x_T)
    head = (C.byref(dims), packed.data_ptr(), workspace.data_ptr(), B, S, _dev_ptr(sem_idx, torch.int64, "sem_idx"))
    tail = (_dev_ptr(x_T, torch.float32, "x_T"), n, ts, cf, x_work.data_ptr(), x0.data_ptr(), _stream(x_T.device))
    if s_len is None:
        lib().edtts_generate(*head, *tail)
    else:
        lib().edtts_generate_len(*head, _dev_ptr(s_len, torch.int64, "sem_lengths"), *tail)
    check_indices(workspace)
    return x0


def sample_ddpm(dims: EdttsDims, packed: torch.Tensor, workspace: torch.Tensor, sem_idx: torch.Tensor, x_T: torch.Tensor,
                t_all: torch.Tensor, coefs: Sequence[Tuple[float, float, float]], noise_all: Optional[torch.Tensor], seed: int,
                batch_offset: int = 0, s_len: Optional[torch.Tensor] = None) -> torch.Tensor:
    """s_len: per-utterance token counts (device int64 [B] or None: the plain export); utterance b has 2 * s_len[b] frames."""
    B, S = sem_idx.shape
    n = t_all.numel()
    cf = (C.c_float * (3 * n))(*[float(v) for c in coefs for v in c])
    out = torch.empty_like(x_T)
    head = (C.byref(dims), packed.data_ptr(), workspace.data_ptr(), B, S, _dev_ptr(sem_idx, torch.int64, "sem_idx"))
    tail = (_dev_ptr(x_T, torch.float32, "x_T"), n, _dev_ptr(t_all, torch.int64, "t_all"), cf, _dev_ptr(noise_all, torch.float32, "noise"),
            _u64(seed), C.c_int64(int(batch_offset)), out.data_ptr(), _stream(x_T.device))
    if s_len is None:
        lib().edtts_sample_ddpm(*head, *tail)
    else:
        lib().edtts_sample_ddpm_len(*head, _dev_ptr(s_len, torch.int64, "sem_lengths"), *tail)
    check_indices(workspace)
    return out


def sample_multistep(dims: EdttsDims, packed: torch.Tensor, workspace: torch.Tensor, sem_idx: Optional[torch.Tensor],
                     sem_features: Optional[torch.Tensor], S: int, x_T: torch.Tensor, timesteps: Sequence[int],
                     coefs: Sequence[Sequence[float]], want_intermediates: bool, t_len: Optional[torch.Tensor] = None,
                     s_len: Optional[torch.Tensor] = None):
    """t_len / s_len: per-utterance frame / token counts (device int64 [B] or None; without either the plain export runs)."""
    B, T, M = x_T.shape
    n = len(timesteps)
    ts = (C.c_int64 * n)(*[int(v) for v in timesteps])
    cf = (C.c_float * (8 * n))(*[float(v) for c in coefs for v in c])
    hist = torch.empty((2, B, T, M), dtype=torch.float32, device=x_T.device)
    x0_all = torch.empty((n, B, T, M), dtype=torch.float32, device=x_T.device) if want_intermediates else None
    out = torch.empty_like(x_T)
    head = (C.byref(dims), packed.data_ptr(), workspace.data_ptr(), B, T, S, _dev_ptr(sem_idx, torch.int64, "sem_idx"),
            _dev_ptr(sem_features, torch.float32, "sem_features"))
    tail = (_dev_ptr(x_T, torch.float32, "x_T"), n, ts, cf, hist.data_ptr(), None if x0_all is None else x0_all.data_ptr(),
            out.data_ptr(), _stream(x_T.device))
    if t_len is None and s_len is None:
        lib().edtts_sample_multistep(*head, *tail)
    else:
        lib().edtts_sample_multistep_len(*head, _dev_ptr(t_len, torch.int64, "x_lengths"), _dev_ptr(s_len, torch.int64, "sem_lengths"),
                                         *tail)
    check_indices(workspace)
    return out, x0_all


def sample_inpaint(dims: EdttsDims, packed: torch.Tensor, workspace: torch.Tensor, workspace_uncond: Optional[torch.Tensor],
                   sem_features: torch.Tensor, zero_features: Optional[torch.Tensor], x: torch.Tensor, t_all: torch.Tensor,
                   step_all: torch.Tensor, coefs: Optional[Sequence[float]], known_mel: Optional[torch.Tensor], overlap_len: int,
                   noise_k: Optional[torch.Tensor], seed: int, cfg_scale: float, v_uncond: Optional[torch.Tensor],
                   t_len: Optional[torch.Tensor] = None, s_len: Optional[torch.Tensor] = None, seeds: Optional[torch.Tensor] = None,
                   lms_rows: Optional[Sequence[Sequence[float]]] = None, want_intermediates: bool = False,
                   keep: Optional[torch.Tensor] = None):
    """The in-painting samplers, in place on x [B, T, n_mels]: edtts_sample_inpaint_len with `coefs` (4 floats per step, flat), or with
    `lms_rows` (8 floats per step; `coefs` is not read: None) edtts_sample_inpaint_multistep_len.  t_all / step_all: device int64
    [num_steps]; t_len / s_len / seeds: device int64 [B] or None.  With `keep` (device uint8 [B, T]; known_mel [B, T, n_mels], noise_k
    [num_steps, B, T, n_mels], overlap_len not read) the *_mask_len twin of either.  Returns (x, x0_all): every step's x0
    [num_steps, B, T, n_mels] when lms_rows and want_intermediates, else None."""
    B, T, M = x.shape
    n = t_all.numel()
    f = torch.float32
    cf = (C.c_float * (4 * n))(*coefs) if lms_rows is None else (C.c_float * (8 * n))(*[float(v) for row in lms_rows for v in row])
    args = (C.byref(dims), packed.data_ptr(), workspace.data_ptr(), None if workspace_uncond is None else workspace_uncond.data_ptr(),
            B, T, sem_features.shape[1], _dev_ptr(sem_features, f, "sem_features"), _dev_ptr(zero_features, f, "zeros"), _dev_ptr(x, f, "x"),
            n, t_all.data_ptr(), step_all.data_ptr(), cf, _dev_ptr(known_mel, f, "known_mel"),
            int(overlap_len) if keep is None else _dev_ptr(keep, torch.uint8, "keep"),
            _dev_ptr(noise_k, f, "noise_k"), _u64(seed), float(cfg_scale),
            None if v_uncond is None else v_uncond.data_ptr(), _dev_ptr(t_len, torch.int64, "x_lengths"),
            _dev_ptr(s_len, torch.int64, "sem_lengths"), _dev_ptr(seeds, torch.int64, "seeds"))
    x0_all = None
    L = lib()
    if lms_rows is None:
        (L.edtts_sample_inpaint_len if keep is None else L.edtts_sample_inpaint_mask_len)(*args, _stream(x.device))
    else:
        hist = torch.empty((2, B, T, M), dtype=f, device=x.device)
        x0_all = torch.empty((n, B, T, M), dtype=f, device=x.device) if want_intermediates else None
        fn = L.edtts_sample_inpaint_multistep_len if keep is None else L.edtts_sample_inpaint_multistep_mask_len
        fn(*args, hist.data_ptr(), None if x0_all is None else x0_all.data_ptr(), _stream(x.device))
    check_indices(workspace)
    return x, x0_all


def ddim_step(alpha_bar: torch.Tensor, x_t: torch.Tensor, t: torch.Tensor, t_prev: torch.Tensor, eps: torch.Tensor, eta: float,
              noise: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    if x_t.shape != eps.shape:
        raise EdttsError(f"x_t {tuple(x_t.shape)} and eps_pred {tuple(eps.shape)} differ")
    B = x_t.shape[0]
    check_table_index(t, alpha_bar.numel(), "t")
    check_table_index(t_prev, alpha_bar.numel(), "t_prev", lo=-alpha_bar.numel())  # negative = "before the first step"
    x_prev, x0 = torch.empty_like(x_t), torch.empty_like(x_t)
    lib().edtts_ddim_step(_dev_ptr(alpha_bar, torch.float32, "alpha_bar"), alpha_bar.numel(), _dev_ptr(x_t, torch.float32, "x_t"),
                          _dev_ptr(eps, torch.float32, "eps_pred"), _dev_ptr(t, torch.int64, "t"), _dev_ptr(t_prev, torch.int64, "t_prev"),
                          B, x_t.numel() // B, float(eta), _dev_ptr(noise, torch.float32, "noise"), x_prev.data_ptr(), x0.data_ptr(),
                          _stream(x_t.device))
    return x_prev, x0


def ddpm_step(alphas, alpha_bar, betas, post_var, x_t, t, eps, noise) -> torch.Tensor:
    B = x_t.shape[0]
    check_table_index(t, alpha_bar.numel(), "t")
    out = torch.empty_like(x_t)
    lib().edtts_ddpm_step(_dev_ptr(alphas, torch.float32, "alphas"), _dev_ptr(alpha_bar, torch.float32, "alpha_bar"),
                          _dev_ptr(betas, torch.float32, "betas"), _dev_ptr(post_var, torch.float32, "posterior_variance"),
                          alpha_bar.numel(), _dev_ptr(x_t, torch.float32, "x_t"), _dev_ptr(eps, torch.float32, "eps_pred"),
                          _dev_ptr(t, torch.int64, "t"), B, x_t.numel() // B, _dev_ptr(noise, torch.float32, "noise"), out.data_ptr(),
                          _stream(x_t.device))
    return out


def dsconv_forward(x, dw, pw, pb, gn_w, gn_b, groups: int, stride: int = 1) -> torch.Tensor:
    B, Ci, T = x.shape
    Co, ks = pw.shape[0], dw.shape[-1]
    To = (T + 2 * (ks // 2) - ks) // stride + 1
    if To < 1:
        raise EdttsError(f"dsconv: no output frames for T={T}, kernel_size={ks}, stride={stride}")
    y = torch.empty(B, Co, To, device=x.device, dtype=torch.float32)
    need = _size_query(lib().edtts_dsconv_scratch_floats, B, Ci, Co, T, ks, int(stride), groups)  # 0: the one-kernel path
    scratch = torch.empty(need, device=x.device, dtype=torch.float32) if need else None
    f = torch.float32
    lib().edtts_dsconv_forward(_dev_ptr(x, f, "x"), _dev_ptr(dw, f, "depthwise.weight"), _dev_ptr(pw, f, "pointwise.weight"),
                               _dev_ptr(pb, f, "pointwise.bias"), _dev_ptr(gn_w, f, "norm.weight"), _dev_ptr(gn_b, f, "norm.bias"),
                               B, Ci, Co, T, ks, int(stride), groups, None if scratch is None else scratch.data_ptr(), y.data_ptr(),
                               _stream(x.device))
    return y


# ---------------------------------------------------------------------------------------------- mel post-processing, audio front end
def mel_to_spec(mel: torch.Tensor, mean: Optional[torch.Tensor], std: Optional[torch.Tensor], pinv: torch.Tensor,
                t_len: Optional[torch.Tensor] = None, smooth: Optional[Tuple[int, int]] = None,
                idx_err: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mel [B, T, n_mels] (mean / std [B, n_mels] or None), pinv [n_freqs, n_mels] -> spec [B, n_freqs, T] (include/edtts.h:
    edtts_mel_to_spec).  With t_len (device int64 [B]) or smooth = (mel bins, frames) edtts_mel_to_spec_len runs; idx_err: the int32
    word a bad t_len is flagged in."""
    B, T, M = mel.shape
    f = torch.float32
    spec = torch.empty(B, pinv.shape[0], T, dtype=f, device=mel.device)
    head = (_dev_ptr(mel, f, "mel"), _dev_ptr(mean, f, "mean"), _dev_ptr(std, f, "std"), _dev_ptr(pinv, f, "pinv"), B, T, M, pinv.shape[0])
    if t_len is None and smooth is None:
        lib().edtts_mel_to_spec(*head, spec.data_ptr(), _stream(mel.device))
    else:
        kh, kw = smooth if smooth is not None else (0, 0)
        lib().edtts_mel_to_spec_len(*head, _dev_ptr(t_len, torch.int64, "lengths"), kh, kw,
                                    None if t_len is None else _dev_ptr(idx_err, torch.int32, "idx_err"), spec.data_ptr(),
                                    _stream(mel.device))
    return spec


def griffin_lim_scratch_floats(B: int, T: int, n_fft: int, hop: int) -> int:
    return _size_query(lib().edtts_griffin_lim_scratch_floats, B, T, n_fft, hop)


def griffin_lim_scratch_layout(B: int, T: int, n_fft: int, hop: int):
    """[(member, offset in floats, shape)] of the Griffin-Lim scratch in its order (csrc/edtts_melpost.h: griffin_lim_run).  The
    complex members are (re, im) pairs of floats: with B T odd they start at an odd float offset, which a complex64 view cannot."""
    bins, bt = n_fft // 2 + 1, B * T
    shapes = (("mag", (B, T, bins)), ("ang", (B, T, bins, 2)), ("tprev", (B, T, bins, 2)), ("frames", (B, T, n_fft)),
              ("wave", (B, n_fft + hop * (T - 1))))
    out, off = [], 0
    for name, shape in shapes:
        out.append((name, off, shape))
        off += math.prod(shape)
    return out


def griffin_lim_scratch_views(scratch: torch.Tensor, B: int, T: int, n_fft: int, hop: int) -> dict:
    """The five members of a scratch that griffin_lim(..., scratch=scratch) ran on, as views: mag [B, T, bins], ang and tprev
    [B, T, bins, 2] (the phases and the previous rebuilt spectrum as (re, im)), frames [B, T, n_fft], wave [B, n_fft + hop (T - 1)]
    (the padded signal; the returned waveform is its columns n_fft / 2 onwards)."""
    return {name: scratch[off:off + math.prod(shape)].view(shape) for name, off, shape in griffin_lim_scratch_layout(B, T, n_fft, hop)}


def griffin_lim(spec: torch.Tensor, n_fft: int, hop: int, window: torch.Tensor, twiddle: torch.Tensor, n_iter: int, momentum: float,
                power: float, angles0: Optional[torch.Tensor], seed: int = 0, t_len: Optional[torch.Tensor] = None,
                seeds: Optional[torch.Tensor] = None, idx_err: Optional[torch.Tensor] = None,
                scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """spec [B, n_fft // 2 + 1, T] -> wave [B, hop * (T - 1)] (include/edtts.h: edtts_griffin_lim).  angles0: fp32 [B, F, T, 2] or None
    (library draws from `seed`).  With t_len (device int64 [B]) edtts_griffin_lim_len runs: seeds (device int64 [B]) replace `seed`,
    idx_err is the int32 word a bad length is flagged in.  ``scratch``: the caller's own (fp32, at least griffin_lim_scratch_floats)
    instead of one allocated here; griffin_lim_scratch_views names what the call leaves in it."""
    B, _, T = spec.shape
    f = torch.float32
    need = griffin_lim_scratch_floats(B, T, n_fft, hop)
    if scratch is None:
        scratch = torch.empty(need, dtype=f, device=spec.device)
    elif scratch.numel() < need or _dev_ptr(scratch, f, "scratch") is None:
        raise EdttsError(f"scratch: expected at least {need} floats, got {scratch.numel()}")
    wave = torch.empty(B, hop * (T - 1), dtype=f, device=spec.device)
    head = (_dev_ptr(spec, f, "specgram"), B, T, n_fft, hop, _dev_ptr(window, f, "window"), _dev_ptr(twiddle, f, "twiddle"), n_iter,
            float(momentum), float(power), _dev_ptr(angles0, f, "angles0"))
    tail = (scratch.data_ptr(), wave.data_ptr(), _stream(spec.device))
    if t_len is None:
        lib().edtts_griffin_lim(*head, _u64(seed), *tail)
    else:
        lib().edtts_griffin_lim_len(*head, _dev_ptr(t_len, torch.int64, "lengths"), _dev_ptr(seeds, torch.int64, "seeds"),
                                    _dev_ptr(idx_err, torch.int32, "idx_err"), *tail)
    return wave


def resample(x: torch.Tensor, t_len: Optional[torch.Tensor], orig: int, new: int, width: int, taps: int, table: torch.Tensor,
             L_out: int) -> torch.Tensor:
    """x [B, L] -> y [B, L_out] through the polyphase `table` (include/edtts.h: edtts_resample); t_len: device int64 [B] or None."""
    B, L = x.shape
    y = torch.empty(B, L_out, dtype=torch.float32, device=x.device)
    lib().edtts_resample(_dev_ptr(x, torch.float32, "waveform"), B, L, _dev_ptr(t_len, torch.int64, "lengths"), orig, new, width, taps,
                         _dev_ptr(table, torch.float32, "table"), L_out, y.data_ptr(), _stream(x.device))
    return y


EDTTS_MEL_POWER, EDTTS_MEL_LOG = 0, 1  # include/edtts.h: the `mode` of edtts_melspec


def melspec(x: torch.Tensor, t_len: Optional[torch.Tensor], n_fft: int, hop: int, tables, n_mels: int, power: int, mode: int) -> torch.Tensor:
    """x [B, L] -> the mel [B, n_mels, T] (mode EDTTS_MEL_POWER) or the log-mel [B, T, n_mels] (EDTTS_MEL_LOG), T = L // hop + 1
    (include/edtts.h: edtts_melspec).  tables: (window, twiddle, fb_desc, fb_weights); t_len: device int64 [B] samples or None."""
    B, L = x.shape
    T = L // hop + 1
    f = torch.float32
    out = torch.empty((B, n_mels, T) if mode == EDTTS_MEL_POWER else (B, T, n_mels), dtype=f, device=x.device)
    window, twiddle, fb_desc, fb_weights = tables
    lib().edtts_melspec(_dev_ptr(x, f, "waveform"), B, L, _dev_ptr(t_len, torch.int64, "lengths"), n_fft, hop, _dev_ptr(window, f, "window"),
                        _dev_ptr(twiddle, f, "twiddle"), _dev_ptr(fb_desc, torch.int32, "fb_desc"), _dev_ptr(fb_weights, f, "fb_weights"),
                        n_mels, power, mode, out.data_ptr(), _stream(x.device))
    return out


def logmel_stats(logmel: torch.Tensor, L: int, t_len: Optional[torch.Tensor], hop: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean, std), each [B, 1, n_mels], of every row's own frames of the log-mel [B, T, n_mels] that melspec wrote for L-sample rows
    (include/edtts.h: edtts_logmel_stats)."""
    B, T, M = logmel.shape
    mean = torch.empty(B, 1, M, dtype=torch.float32, device=logmel.device)
    std = torch.empty_like(mean)
    lib().edtts_logmel_stats(_dev_ptr(logmel, torch.float32, "logmel"), B, T, M, L, _dev_ptr(t_len, torch.int64, "lengths"), hop,
                             mean.data_ptr(), std.data_ptr(), _stream(logmel.device))
    return mean, std


def mel_segment_stats(x: torch.Tensor, t_len: Optional[torch.Tensor], segments: torch.Tensor, n_fft: int, hop: int, tables,
                      n_mels: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean, std), each [n_seg, 1, n_mels], of the log-mel of every (row, start, end) of `segments` (device int64 [n_seg, 3]) taken
    as a waveform of its own (include/edtts.h: edtts_mel_segment_stats).  tables: as melspec."""
    B, L = x.shape
    n_seg = segments.shape[0]
    mean = torch.empty(n_seg, 1, n_mels, dtype=torch.float32, device=x.device)
    std = torch.empty_like(mean)
    window, twiddle, fb_desc, fb_weights = tables
    f = torch.float32
    lib().edtts_mel_segment_stats(_dev_ptr(x, f, "waveform"), B, L, _dev_ptr(t_len, torch.int64, "lengths"),
                                  _dev_ptr(segments, torch.int64, "segments"), n_seg, n_fft, hop, _dev_ptr(window, f, "window"),
                                  _dev_ptr(twiddle, f, "twiddle"), _dev_ptr(fb_desc, torch.int32, "fb_desc"),
                                  _dev_ptr(fb_weights, f, "fb_weights"), n_mels, mean.data_ptr(), std.data_ptr(), _stream(x.device))
    return mean, std


def randn(shape, device, seed: int = 0, stream_id: int = 0, elem_offset: int = 0, scale: float = 1.0) -> torch.Tensor:
    """scale * N(0, 1) from the library's Philox stream (seed, stream_id) at global element offset `elem_offset`: the start
    noise of a batch shard, identical to what one GPU would draw for the same rows (include/edtts.h: edtts_randn)."""
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    if not out.is_cuda:
        raise EdttsError(f"randn: expected a HIP device, got {out.device} -- the MI355X sampler path has no CPU fallback")
    if out.numel() == 0:  # the empty shard of a rank without utterances: nothing to draw (data_ptr() is NULL)
        return out
    off, n = int(elem_offset), out.numel()
    if off % 4 or n % 4:
        # the library draws whole groups of 4 elements: draw the aligned cover and cut (element values depend only on their
        # global index, so this is what an aligned call would have produced for them)
        lo, hi = off - off % 4, -(-(off + n) // 4) * 4
        cover = randn((hi - lo,), device, seed, stream_id, lo, scale)
        return cover[off - lo: off - lo + n].reshape(out.shape).clone()
    lib().edtts_randn(out.data_ptr(), out.numel(), _u64(seed), C.c_uint32(stream_id & 0xFFFFFFFF),
                      C.c_uint64(int(elem_offset)), float(scale), _stream(out.device))
    return out


def seed_tensor(seeds, B: int, device) -> torch.Tensor:
    """Per-row Philox seeds as the device uint64 [B] array the library reads (the bits of each seed in an int64 tensor): a sequence of
    B ints is copied to `device` (not while the stream is capturing); an int64 tensor of shape [B] on `device` is used as it is."""
    if isinstance(seeds, torch.Tensor):
        if seeds.dtype != torch.int64 or tuple(seeds.shape) != (B,):
            raise ValueError(f"seeds: expected an int64 tensor of shape [{B}], got {seeds.dtype} {list(seeds.shape)}")
        if not seeds.is_cuda:
            return seed_tensor(seeds.tolist(), B, device)
        if seeds.device != torch.device(device):
            raise ValueError(f"seeds: on {seeds.device}, the call runs on {device}")
        return seeds.contiguous()
    seeds = [int(s) for s in seeds]
    if len(seeds) != B:
        raise ValueError(f"seeds: expected {B} seeds (one per row), got {len(seeds)}")
    if torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("seeds: a host seed list cannot be copied to the device during graph capture; pass a device int64 tensor")
    bits = [((s & 0xFFFFFFFFFFFFFFFF) ^ (1 << 63)) - (1 << 63) for s in seeds]  # uint64 bits as int64
    return host_to_device(torch.tensor(bits, dtype=torch.int64), device)


def host_to_device(t: torch.Tensor, device) -> torch.Tensor:
    """A small host tensor on `device` without stalling the host: a pageable copy would synchronise the current stream (and with it
    a thread that enqueues for several streams), a copy from pinned memory is queued on the stream."""
    if torch.device(device).type != "cuda":
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


def randn_rows(shape, device, seeds, stream_id: int = 0, scale: float = 1.0) -> torch.Tensor:
    """[B, ...] standard normals times `scale`, one launch: row b is bitwise randn(shape[1:], seed=seeds[b], stream_id=stream_id)
    (offset 0), so a longer row begins with a shorter row's draws (include/edtts.h: edtts_randn_rows).  seeds: B ints or a device
    int64 [B] tensor (see seed_tensor)."""
    shape = tuple(int(v) for v in shape)
    if not shape:
        raise ValueError("randn_rows: shape needs a leading row dimension")
    out = torch.empty(shape, dtype=torch.float32, device=device)
    if not out.is_cuda:
        raise EdttsError(f"randn_rows: expected a HIP device, got {out.device} -- the MI355X sampler path has no CPU fallback")
    B = shape[0]
    sd = seed_tensor(seeds, B, out.device)
    if out.numel() == 0:
        return out
    lib().edtts_randn_rows(out.data_ptr(), B, out.numel() // B, sd.data_ptr(), C.c_uint32(stream_id & 0xFFFFFFFF), float(scale),
                           _stream(out.device))
    return out


CHECK_INDICES = os.environ.get("EDTTS_CHECK_INDICES", "0") == "1"


def index_errors(workspace: torch.Tensor) -> int:
    """EDTTS_IDX_* bits recorded since the last call (synchronises the current stream)."""
    flags = C.c_int(0)
    lib().edtts_index_errors(workspace.data_ptr(), C.byref(flags), _stream(workspace.device))
    return flags.value


def check_indices(workspace: torch.Tensor) -> None:
    """Debug mode (EDTTS_CHECK_INDICES=1 or native.CHECK_INDICES = True): raise IndexError where the reference would have --
    the kernels clamp out-of-range token / step indices instead of faulting (include/edtts.h: edtts_index_errors)."""
    if not CHECK_INDICES or torch.cuda.is_current_stream_capturing():
        return
    flags = index_errors(workspace)
    if flags:
        what = [n for b, n in ((EDTTS_IDX_SEM, "sem_idx outside [0, codebook_size)"), (EDTTS_IDX_STEP, "step_idx outside [0, n_step_emb)"),
                               (EDTTS_IDX_LEN, "a per-utterance length outside [1, T] / [1, S]")) if flags & b]
        raise IndexError("index out of range in the decoder call: " + "; ".join(what))


def check_table_index(t: torch.Tensor, n: int, name: str, lo: int = 0) -> None:
    if CHECK_INDICES and not torch.cuda.is_current_stream_capturing() and bool(((t < lo) | (t >= n)).any()):
        raise IndexError(f"{name}: index out of range [{lo}, {n})")


# ---------------------------------------------------------------------------------------------- optimiser step
def optim_chunk_size() -> int:
    """Elements per chunk of the optimiser's multi-tensor table (include/edtts.h: edtts_optim_chunk_size)."""
    return int(lib().edtts_optim_chunk_size())


def optim_chunk_table(numels: Sequence[int]) -> List[Tuple[int, int, int]]:
    """The library's cutting of a list of tensor sizes into chunks: [(tensor index, first element, count)], a host query."""
    n = len(numels)
    arr = (C.c_int64 * max(n, 1))(*[int(v) for v in numels])
    total = C.c_int(0)
    lib().edtts_optim_chunk_table(arr, n, 0, None, None, None, C.byref(total))
    cap = max(total.value, 1)
    ti, off, cnt = (C.c_int32 * cap)(), (C.c_int64 * cap)(), (C.c_int32 * cap)()
    lib().edtts_optim_chunk_table(arr, n, total.value, ti, off, cnt, C.byref(total))
    return [(ti[i], off[i], cnt[i]) for i in range(total.value)]


def optim_scratch_bytes(n_chunks: int, n_groups: int) -> int:
    return _size_query(lib().edtts_optim_scratch_bytes, int(n_chunks), int(n_groups))


def optim_step(tensors, n_tensors: int, groups, n_groups: int, max_norm: Optional[float], flags: int, scratch: torch.Tensor) -> None:
    """edtts_optim_step on the current stream of the scratch's device.  `tensors` / `groups`: ctypes arrays of EdttsOptimTensor /
    EdttsOptimGroup holding device pointers the caller has validated (fp32, contiguous, on that device)."""
    if max_norm is not None:
        flags |= OPT_CLIP
    lib().edtts_optim_step(tensors, n_tensors, groups, n_groups, 0.0 if max_norm is None else float(max_norm), flags,
                           _dev_ptr(scratch, torch.uint8, "scratch"), scratch.numel(), _stream(scratch.device))


def optim_upload(tensors, n_tensors: int, groups, n_groups: int, flags: int, scratch: torch.Tensor) -> Tuple[int, int]:
    """edtts_optim_upload: validate and copy the step's table into the scratch (not under capture) -> (number of chunks, byte offset
    of the EdttsOptimGroup array in the scratch)."""
    n_chunks, off = C.c_int(0), C.c_size_t(0)
    lib().edtts_optim_upload(tensors, n_tensors, groups, n_groups, flags, _dev_ptr(scratch, torch.uint8, "scratch"), scratch.numel(),
                             C.byref(n_chunks), C.byref(off), _stream(scratch.device))
    return n_chunks.value, off.value


def optim_schedule(kind: str, base_lr: float, min_lr: float, warmup_steps: int, total_steps: int) -> EdttsOptimSchedule:
    """An EdttsOptimSchedule; kind: "cosine" (train_v2.cosine_lr_schedule)."""
    kinds = {"cosine": EDTTS_SCHED_COSINE}
    if kind not in kinds:
        raise ValueError(f"schedule kind must be one of {sorted(kinds)}, got {kind!r}")
    if not float(base_lr) >= 0.0 or not float(min_lr) >= 0.0 or int(warmup_steps) < 0 or int(total_steps) < 0:
        raise ValueError(f"schedule: base_lr={base_lr} min_lr={min_lr} warmup_steps={warmup_steps} total_steps={total_steps}")
    return EdttsOptimSchedule(kinds[kind], 0, float(base_lr), float(min_lr), int(warmup_steps), int(total_steps))


def optim_step_resident(n_chunks: int, n_groups: int, max_norm: Optional[float], flags: int, scratch: torch.Tensor,
                        lr_dev: Optional[torch.Tensor] = None, sched: Optional[EdttsOptimSchedule] = None) -> None:
    """edtts_optim_step_resident on the current stream of the scratch's device: the step on the table optim_upload left in the
    scratch (capturable).  lr_dev: fp64 [n_groups] device tensor or None; sched: an EdttsOptimSchedule or None."""
    if max_norm is not None:
        flags |= OPT_CLIP
    if lr_dev is not None and (_dev_ptr(lr_dev, torch.float64, "lr_dev") is None or lr_dev.numel() != n_groups):
        raise EdttsError(f"lr_dev: expected {n_groups} fp64 values, got {lr_dev.numel()}")
    lib().edtts_optim_step_resident(int(n_chunks), int(n_groups), 0.0 if max_norm is None else float(max_norm), flags,
                                    _dev_ptr(scratch, torch.uint8, "scratch"), scratch.numel(),
                                    None if lr_dev is None else lr_dev.data_ptr(), None if sched is None else C.byref(sched),
                                    _stream(scratch.device))


# ---------------------------------------------------------------------------------------------- key stream
def keys_host(base: int, counter: int, first: int, n: int) -> List[int]:
    """edtts_keys_host: keys first .. first + n - 1 of call `counter` of the key stream with base seed `base`; no GPU call."""
    out = (C.c_uint64 * max(int(n), 1))()
    lib().edtts_keys_host(_u64(base), _u64(counter), C.c_int64(int(first)), int(n), out)
    return [int(out[i]) for i in range(int(n))]


class KeyStream:
    """A device array of 63-bit Philox keys that one launch regenerates (include/edtts.h: edtts_keys_advance): ``n_slots`` dropout
    keys followed by ``n_rows`` per-row noise seeds.  ``advance()`` is capturable: every replay of a graph that holds it writes the
    keys of the next call counter.  ``take(owner, first_slot)`` hands a module its slots -- first_slot, first_slot + 1, ... for its
    first, second, ... differentiable forward since the last ``advance()``, which returns every module's cursor to 0."""

    def __init__(self, seed: int, n_slots: int, n_rows: int = 0, device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise EdttsError(f"KeyStream: expected a HIP device, got {dev} -- there is no CPU fallback")
        if int(n_slots) < 0 or int(n_rows) < 0 or int(n_slots) + int(n_rows) < 1:
            raise ValueError(f"KeyStream: n_slots={n_slots} n_rows={n_rows}")
        self.seed, self.n_slots, self.n_rows = int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_slots), int(n_rows)
        bits = ((self.seed ^ (1 << 63)) - (1 << 63))  # the uint64 bits as an int64
        self.state = host_to_device(torch.tensor([bits, 0], dtype=torch.int64), dev)
        self.keys = torch.zeros(self.n_slots + self.n_rows, dtype=torch.int64, device=dev)
        self._cursors: dict = {}  # id(module) -> forwards it has made since the last advance()

    def advance(self) -> None:
        lib().edtts_keys_advance(self.keys.data_ptr(), self.keys.numel(), self.state.data_ptr(), _stream(self.keys.device))
        self._cursors = {}

    def slot(self, k: int) -> torch.Tensor:
        if not 0 <= int(k) < self.n_slots:
            raise IndexError(f"KeyStream: slot {k} outside [0, {self.n_slots})")
        return self.keys[int(k):int(k) + 1]

    def take(self, owner, first_slot: int = 0) -> torch.Tensor:
        """Slot first_slot + (forwards `owner` has made since the last advance())."""
        n = self._cursors.get(id(owner), 0)
        k = int(first_slot) + n
        if not 0 <= k < self.n_slots:
            raise RuntimeError(f"KeyStream: {type(owner).__name__} asks for slot {k} (first_slot {first_slot}, forward {n + 1} since "
                               f"advance()) of {self.n_slots}: one slot per differentiable forward of a step")
        self._cursors[id(owner)] = n + 1
        return self.slot(k)

    def rows(self) -> torch.Tensor:
        return self.keys[self.n_slots:]

    def keys_at(self, counter: int) -> List[int]:
        """What advance() wrote when the call counter stood at `counter`, recomputed on the host."""
        return keys_host(self.seed, counter, 0, self.n_slots + self.n_rows)

    def counter(self) -> int:
        """Calls of advance() that have run (reads the device counter: synchronises)."""
        return int(self.state[1].item()) & 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------------------------- training objective
class ObjBatch:
    """The arguments that define a prepared batch for edtts_objective_prepare / edtts_objective_loss (include/edtts.h, "training
    objective"), validated once: mel [B, T, M] fp32; t int64 [B]; tables fp32 [4, n_table]; mean / std [B, 1, M] or None; lengths and
    seeds device int64 [B] or None; noise [B, T, M] or None.  Everything contiguous on mel's device."""

    def __init__(self, mel, t, tables, mean=None, std=None, lengths=None, seeds=None, noise=None):
        f = torch.float32
        _dev_ptr(mel, f, "mel")
        if mel.dim() != 3:
            raise EdttsError(f"mel: expected [B, T, n_mels], got {list(mel.shape)}")
        B, T, M = mel.shape
        self.mel, self.t, self.tables, self.mean, self.std, self.lengths, self.seeds, self.noise = mel, t, tables, mean, std, lengths, seeds, noise
        self.B, self.T, self.M = B, T, M
        for name, v, dt, shape in (("t", t, torch.int64, (B,)), ("tables", tables, f, (4, tables.shape[-1] if tables is not None else 0)),
                                   ("mean", mean, f, (B, 1, M)), ("std", std, f, (B, 1, M)), ("lengths", lengths, torch.int64, (B,)),
                                   ("seeds", seeds, torch.int64, (B,)), ("noise", noise, f, (B, T, M))):
            if v is None:
                continue
            _dev_ptr(v, dt, name)
            if tuple(v.shape) != shape:
                raise EdttsError(f"{name}: expected shape {list(shape)}, got {list(v.shape)}")
            if v.device != mel.device:
                raise EdttsError(f"{name}: on {v.device}, the call runs on {mel.device}")
        if seeds is None and noise is None:
            raise EdttsError("objective: either seeds or noise must be given")

    def head(self):
        """(mel, B, T, n_mels, lengths, t, tables, n_table, mean, std, seeds, noise) as the two calls take them."""
        ptr = lambda v: None if v is None else v.data_ptr()
        return (self.mel.data_ptr(), self.B, self.T, self.M, ptr(self.lengths), self.t.data_ptr(), self.tables.data_ptr(),
                self.tables.shape[1], ptr(self.mean), ptr(self.std), ptr(self.seeds), ptr(self.noise))


def objective_scratch_bytes(B: int, T: int, n_mels: int) -> int:
    return _size_query(lib().edtts_objective_scratch_bytes, int(B), int(T), int(n_mels))


def objective_stats(mel: torch.Tensor, lengths: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """normalize_mel's (mean, std), each [B, 1, n_mels], over every row's live frames (include/edtts.h: edtts_objective_stats)."""
    _dev_ptr(mel, torch.float32, "mel")
    B, T, M = mel.shape
    mean = torch.empty(B, 1, M, dtype=torch.float32, device=mel.device)
    std = torch.empty_like(mean)
    lib().edtts_objective_stats(mel.data_ptr(), B, T, M, _dev_ptr(lengths, torch.int64, "lengths"), mean.data_ptr(), std.data_ptr(),
                                _stream(mel.device))
    return mean, std


def objective_prepare(batch: ObjBatch, kind: int, parts: bool = False):
    """edtts_objective_prepare: x_t, and with ``parts`` also (mel_n, noise, target), each [B, T, n_mels]."""
    x_t = torch.empty_like(batch.mel)
    extra = tuple(torch.empty_like(batch.mel) for _ in range(3)) if parts else (None, None, None)
    lib().edtts_objective_prepare(*batch.head(), int(kind), x_t.data_ptr(), *[None if e is None else e.data_ptr() for e in extra],
                                  _stream(x_t.device))
    return (x_t, *extra) if parts else x_t


def objective_loss(kind: int, batch: ObjBatch, pred: torch.Tensor, pred2: Optional[torch.Tensor], t2: Optional[torch.Tensor],
                   want_unit: bool, want_unit2: bool, scratch: torch.Tensor):
    """edtts_objective_loss -> (out fp32 [8]: loss | 3 terms | x0_mse | x0_cos | 0 | 0, unit or None, unit2 or None)."""
    f = torch.float32
    for name, p in (("pred", pred), ("pred2", pred2)):
        if p is None:
            continue
        _dev_ptr(p, f, name)
        if p.dim() != 3 or p.shape[0] != batch.B or p.shape[2] != batch.M or p.device != batch.mel.device:
            raise EdttsError(f"{name}: expected [{batch.B}, T_pred, {batch.M}] on {batch.mel.device}, got {list(p.shape)} on {p.device}")
    if t2 is not None and (_dev_ptr(t2, torch.int64, "t2") is None or tuple(t2.shape) != (batch.B,)):
        raise EdttsError(f"t2: expected shape [{batch.B}], got {list(t2.shape)}")
    out = torch.empty(8, dtype=f, device=pred.device)
    unit = torch.empty_like(pred) if want_unit else None
    unit2 = torch.empty_like(pred2) if want_unit2 else None
    ptr = lambda v: None if v is None else v.data_ptr()
    lib().edtts_objective_loss(int(kind), *batch.head(), pred.data_ptr(), pred.shape[1], ptr(pred2), 0 if pred2 is None else pred2.shape[1],
                               ptr(t2), ptr(unit), ptr(unit2), _dev_ptr(scratch, torch.uint8, "scratch"), scratch.numel(), out.data_ptr(),
                               _stream(pred.device))
    return out, unit, unit2


def objective_scale(unit: torch.Tensor, grad_out: torch.Tensor) -> torch.Tensor:
    """d_pred = unit * grad_out (a 0-dim fp32 device tensor, read on the device: no synchronisation)."""
    d = torch.empty_like(unit)
    if grad_out.numel() != 1 or grad_out.device != unit.device:
        raise EdttsError(f"grad_out: expected one element on {unit.device}, got {list(grad_out.shape)} on {grad_out.device}")
    lib().edtts_objective_scale(_dev_ptr(unit, torch.float32, "unit"), _dev_ptr(grad_out.contiguous(), torch.float32, "grad_out"),
                                unit.numel(), d.data_ptr(), _stream(unit.device))
    return d


def generic_slot_dest(dims: EdttsDims, slot: int) -> Tuple[int, int, int, bool]:
    """(offset in floats, rows, cols, transposed) of weight slot `slot` in the generic fp32 blob (include/edtts.h)."""
    off, rows, cols, tr = C.c_size_t(0), C.c_int(0), C.c_int(0), C.c_int(0)
    lib().edtts_generic_slot_dest(C.byref(dims), int(slot), C.byref(off), C.byref(rows), C.byref(cols), C.byref(tr))
    return off.value, rows.value, cols.value, bool(tr.value)


# ---------------------------------------------------------------------------------------------- semantic head
def sem_packed_bytes(dims: EdttsSemDims) -> int:
    return _size_query(lib().edtts_sem_packed_bytes, C.byref(dims))


def sem_num_codes(dims: EdttsSemDims) -> int:
    return _size_query(lib().edtts_sem_num_codes, C.byref(dims), ctype=C.c_int64)


def sem_pack(dims: EdttsSemDims, tensors: Sequence[torch.Tensor], packed: torch.Tensor) -> None:
    """Pack the head's weights (state-dict order, include/edtts.h: edtts_sem_pack) into `packed` (uint8 device tensor)."""
    ptrs = _slot_ptrs(tensors, "weight")
    lib().edtts_sem_pack(C.byref(dims), ptrs, len(tensors), _dev_ptr(packed, torch.uint8, "packed"), _stream(packed.device))


def _check_sem_width(dims: EdttsSemDims, D: int) -> None:
    want_d = dims.in_dim if dims.in_dim else dims.semantic_dim
    if D != want_d:
        raise ValueError(f"feature width {D} does not match the head's input width {want_d}")


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def sem_encode(dims: EdttsSemDims, packed: torch.Tensor, h: torch.Tensor, lengths: Optional[torch.Tensor] = None,
               want_z: bool = False, want_zq: bool = True, want_counts: bool = True):
    """h [B, T, in_dim] (or z [B, T, semantic_dim] when dims.in_dim is 0) -> (idx int64 [B, T], z or None, z_q or None,
    counts int32 [num_codes] or None), one kernel (include/edtts.h: edtts_sem_encode).  lengths: device int64 [B] or None."""
    if h.dim() != 3:
        raise ValueError(f"expected features [B, T, D], got shape {list(h.shape)}")
    B, T, D = h.shape
    _check_sem_width(dims, D)
    h = _aligned(h)
    dev = h.device
    S = dims.semantic_dim
    idx = torch.empty((B, T), dtype=torch.int64, device=dev)
    z = torch.empty((B, T, S), dtype=torch.float32, device=dev) if want_z else None
    zq = torch.empty((B, T, S), dtype=torch.float32, device=dev) if want_zq else None
    counts = torch.empty((sem_num_codes(dims),), dtype=torch.int32, device=dev) if want_counts else None
    lib().edtts_sem_encode(C.byref(dims), _dev_ptr(packed, torch.uint8, "packed"), _dev_ptr(h, torch.float32, "features"), B, T,
                           _dev_ptr(lengths, torch.int64, "lengths"), idx.data_ptr(), None if z is None else z.data_ptr(),
                           None if zq is None else zq.data_ptr(), None if counts is None else counts.data_ptr(), _stream(dev))
    return idx, z, zq, counts


def sem_decode(dims: EdttsSemDims, packed: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """idx int64 [...] -> z_q [..., semantic_dim] (include/edtts.h: edtts_sem_decode).  Ids are clamped into range; with
    EDTTS_CHECK_INDICES=1 an out-of-range id raises IndexError first."""
    idx = idx.contiguous()
    check_table_index(idx, sem_num_codes(dims), "token id")
    out = torch.empty((*idx.shape, dims.semantic_dim), dtype=torch.float32, device=idx.device)
    if idx.numel() == 0:
        return out
    lib().edtts_sem_decode(C.byref(dims), _dev_ptr(packed, torch.uint8, "packed"), _dev_ptr(idx, torch.int64, "idx"), idx.numel(),
                           out.data_ptr(), _stream(idx.device))
    return out


def sem_stats(counts: torch.Tensor):
    """counts int32 [num_codes] -> (perplexity fp32 0-dim, used int64 0-dim), both on the device (include/edtts.h: edtts_sem_stats)."""
    ppl = torch.empty((), dtype=torch.float32, device=counts.device)
    used = torch.empty((), dtype=torch.int64, device=counts.device)
    lib().edtts_sem_stats(_dev_ptr(counts, torch.int32, "counts"), counts.numel(), ppl.data_ptr(), used.data_ptr(), _stream(counts.device))
    return ppl, used


# ---------------------------------------------------------------------------------------------- semantic head, training
SEM_DROP_STREAM = 0x40000  # include/edtts.h, "Philox stream ids": the head's dropout site


def sem_train_packed_bytes(dims: EdttsSemDims) -> int:
    return _size_query(lib().edtts_sem_train_packed_bytes, C.byref(dims))


def sem_train_pack(dims: EdttsSemDims, tensors: Sequence[torch.Tensor], packed_train: torch.Tensor) -> None:
    """The training-only blob (the transposed matrices the backward streams); slots as sem_pack."""
    ptrs = _slot_ptrs(tensors, "weight")
    lib().edtts_sem_train_pack(C.byref(dims), ptrs, len(tensors), _dev_ptr(packed_train, torch.uint8, "packed_train"),
                               _stream(packed_train.device))


def sem_train_tape_bytes(dims: EdttsSemDims, B: int, T: int) -> int:
    return _size_query(lib().edtts_sem_train_tape_bytes, C.byref(dims), B, T)


def sem_train_scratch_bytes(dims: EdttsSemDims, B: int, T: int) -> int:
    return _size_query(lib().edtts_sem_train_scratch_bytes, C.byref(dims), B, T)


def _sem_train_out(dims: EdttsSemDims, h: torch.Tensor, want_counts: bool = True):
    """(B, T, idx int64 [B, T], z_q [B, T, semantic_dim], counts int32 [num_codes] or None): what a training forward of either head fills."""
    B, T, D = h.shape
    _check_sem_width(dims, D)
    idx = torch.empty((B, T), dtype=torch.int64, device=h.device)
    zq = torch.empty((B, T, dims.semantic_dim), dtype=torch.float32, device=h.device)
    counts = torch.empty((sem_num_codes(dims),), dtype=torch.int32, device=h.device) if want_counts else None
    return B, T, idx, zq, counts


def sem_encode_train(dims: EdttsSemDims, packed: torch.Tensor, h: torch.Tensor, tape: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                     want_counts: bool = True, drop=None):
    """edtts_sem_encode_train: h [B, T, in_dim] (z [B, T, semantic_dim] when dims.in_dim is 0; contiguous, 16-byte aligned) ->
    (idx, z_q, counts or None) as sem_encode, with the backward's tape written to `tape` (uint8, sem_train_tape_bytes).  ``drop``:
    None, an EdttsDropout or a (p, seed) pair."""
    B, T, idx, zq, counts = _sem_train_out(dims, h, want_counts)
    drop = _dropout(drop)
    fn = lib().edtts_sem_encode_train_dev if isinstance(drop, EdttsDropoutDev) else lib().edtts_sem_encode_train
    fn(C.byref(dims), _dev_ptr(packed, torch.uint8, "packed"), _dev_ptr(h, torch.float32, "features"), B, T,
       _dev_ptr(lengths, torch.int64, "lengths"), idx.data_ptr(), zq.data_ptr(),
       None if counts is None else counts.data_ptr(), _dev_ptr(tape, torch.uint8, "tape"),
       None if drop is None else C.byref(drop), _stream(h.device))
    return idx, zq, counts


def sem_backward(dims: EdttsSemDims, packed: torch.Tensor, packed_train: torch.Tensor, tape: torch.Tensor, h: torch.Tensor,
                 lengths: Optional[torch.Tensor], d_zq: torch.Tensor, grads: Sequence[Optional[torch.Tensor]],
                 d_z: Optional[torch.Tensor] = None, drop=None) -> None:
    """edtts_sem_backward: writes the gradient of every non-None entry of `grads` (slot order) and d_z (dims.in_dim == 0).  ``drop``:
    what the forward that filled `tape` was given."""
    B, T, _ = h.shape
    ptrs = _slot_ptrs(grads, "grad")
    scratch = torch.empty(sem_train_scratch_bytes(dims, B, T), dtype=torch.uint8, device=h.device)
    drop = _dropout(drop)
    fn = lib().edtts_sem_backward_dev if isinstance(drop, EdttsDropoutDev) else lib().edtts_sem_backward
    fn(C.byref(dims), _dev_ptr(packed, torch.uint8, "packed"), _dev_ptr(packed_train, torch.uint8, "packed_train"),
       _dev_ptr(tape, torch.uint8, "tape"), _dev_ptr(h, torch.float32, "features"), B, T,
       _dev_ptr(lengths, torch.int64, "lengths"), _dev_ptr(d_zq, torch.float32, "d_zq"), ptrs, len(grads),
       _dev_ptr(d_z, torch.float32, "d_z"), scratch.data_ptr(), None if drop is None else C.byref(drop),
       _stream(h.device))


def sem_dropout_mask(dims: EdttsSemDims, B: int, T: int, p: float, seed, device="cuda") -> torch.Tensor:
    """edtts_sem_dropout_mask: the keep mask (uint8, 1 = kept) [B * T, semantic_dim] of the head's dropout site.  ``seed``: an int, or a
    1-element int64 device tensor holding it (edtts_sem_dropout_mask_dev)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise EdttsError(f"sem_dropout_mask: expected a HIP device, got {dev} -- there is no CPU fallback")
    keep = torch.empty((B * T, dims.semantic_dim), dtype=torch.uint8, device=dev)
    if isinstance(seed, torch.Tensor):
        drop = DropKey(p, seed).struct()
        lib().edtts_sem_dropout_mask_dev(C.byref(dims), B, T, C.byref(drop), keep.data_ptr(), _stream(dev))
    else:
        drop = EdttsDropout(float(p), int(seed))
        lib().edtts_sem_dropout_mask(C.byref(dims), B, T, C.byref(drop), keep.data_ptr(), _stream(dev))
    return keep


# ---------------------------------------------------------------------------------------------- VQ head, training
def sem_vq_train_packed_bytes(dims: EdttsSemDims) -> int:
    return _size_query(lib().edtts_sem_vq_train_packed_bytes, C.byref(dims))


def sem_vq_train_pack(dims: EdttsSemDims, tensors: Sequence[torch.Tensor], packed_train: torch.Tensor) -> None:
    """The VQ head's training-only blob (the final Linear's transpose; nothing when dims.in_dim is 0); slots as sem_pack."""
    ptrs = _slot_ptrs(tensors, "weight")
    lib().edtts_sem_vq_train_pack(C.byref(dims), ptrs, len(tensors), _dev_ptr(packed_train, torch.uint8, "packed_train"),
                                  _stream(packed_train.device))


def sem_vq_tape_bytes(dims: EdttsSemDims, B: int, T: int) -> int:
    return _size_query(lib().edtts_sem_vq_tape_bytes, C.byref(dims), B, T)


def sem_vq_scratch_bytes(dims: EdttsSemDims, B: int, T: int) -> int:
    return _size_query(lib().edtts_sem_vq_scratch_bytes, C.byref(dims), B, T)


def sem_vq_encode_train(dims: EdttsSemDims, packed: torch.Tensor, h: torch.Tensor, tape: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                        training: bool = True, commit: float = 0.25, drop=None):
    """edtts_sem_vq_encode_train: h [B, T, in_dim] (z [B, T, semantic_dim] when dims.in_dim is 0; contiguous, 16-byte aligned) ->
    (idx, z_q, counts, vq_loss 0-dim) with the backward's tape written to `tape` (uint8, sem_vq_tape_bytes).  ``drop``: None, an
    EdttsDropout or a (p, seed) pair."""
    B, T, idx, zq, counts = _sem_train_out(dims, h)
    loss = torch.empty((), dtype=torch.float32, device=h.device)
    drop = _dropout(drop)
    lib().edtts_sem_vq_encode_train(C.byref(dims), _dev_ptr(packed, torch.uint8, "packed"), _dev_ptr(h, torch.float32, "features"), B, T,
                                    _dev_ptr(lengths, torch.int64, "lengths"), idx.data_ptr(), zq.data_ptr(), counts.data_ptr(),
                                    loss.data_ptr(), _dev_ptr(tape, torch.uint8, "tape"), int(bool(training)), float(commit),
                                    None if drop is None else C.byref(drop), _stream(h.device))
    return idx, zq, counts, loss


def sem_vq_ema_update(dims: EdttsSemDims, idx: torch.Tensor, z: torch.Tensor, lengths: Optional[torch.Tensor], counts: torch.Tensor,
                      decay: float, epsilon: float, ema_cluster_size: torch.Tensor, ema_w: torch.Tensor, codebook: torch.Tensor) -> None:
    """edtts_sem_vq_ema_update: the three EMA lines of VectorQuantizer._ema_update, in place on the two buffers and the codebook's
    storage.  idx [B, T], z [B, T, semantic_dim]."""
    B, T = idx.shape
    scratch = torch.empty(sem_vq_scratch_bytes(dims, B, T), dtype=torch.uint8, device=idx.device)
    f = torch.float32
    lib().edtts_sem_vq_ema_update(C.byref(dims), _dev_ptr(idx, torch.int64, "idx"), _dev_ptr(z, f, "z"), B, T,
                                  _dev_ptr(lengths, torch.int64, "lengths"), _dev_ptr(counts, torch.int32, "counts"), float(decay),
                                  float(epsilon), _dev_ptr(ema_cluster_size, f, "ema_cluster_size"), _dev_ptr(ema_w, f, "ema_w"),
                                  _dev_ptr(codebook, f, "codebook"), scratch.data_ptr(), _stream(idx.device))


def sem_vq_backward(dims: EdttsSemDims, packed: Optional[torch.Tensor], packed_train: Optional[torch.Tensor], tape: torch.Tensor,
                    h: torch.Tensor, idx: torch.Tensor, lengths: Optional[torch.Tensor], d_zq: Optional[torch.Tensor],
                    d_loss: Optional[torch.Tensor], commit: float, grads: Sequence[Optional[torch.Tensor]],
                    d_z: Optional[torch.Tensor] = None, drop=None) -> None:
    """edtts_sem_vq_backward: writes the gradient of every non-None entry of `grads` (slot order) and d_z (dims.in_dim == 0).
    d_zq / d_loss None: zero.  ``drop``: what the forward that filled `tape` was given."""
    B, T, _ = h.shape
    ptrs = _slot_ptrs(grads, "grad")
    scratch = torch.empty(sem_vq_scratch_bytes(dims, B, T), dtype=torch.uint8, device=h.device)
    drop = _dropout(drop)
    f = torch.float32
    lib().edtts_sem_vq_backward(C.byref(dims), _dev_ptr(packed, torch.uint8, "packed"), _dev_ptr(packed_train, torch.uint8, "packed_train"),
                                _dev_ptr(tape, torch.uint8, "tape"), _dev_ptr(h, f, "features"), _dev_ptr(idx, torch.int64, "idx"), B, T,
                                _dev_ptr(lengths, torch.int64, "lengths"), _dev_ptr(d_zq, f, "d_zq"), _dev_ptr(d_loss, f, "d_loss"),
                                float(commit), ptrs, len(grads), _dev_ptr(d_z, f, "d_z"), scratch.data_ptr(),
                                None if drop is None else C.byref(drop), _stream(h.device))


# the members of a head's tape and of its backward's scratch, as edtts_sem_train_region names them (include/edtts.h: EDTTS_SEM_TAPE_* /
# EDTTS_SEM_SCRATCH_*)
SEM_TRAIN_REGIONS = ("tape.y1", "tape.z", "tape.zb", "tape.r", "tape.sq", "scratch.du", "scratch.zql", "scratch.dz", "scratch.gm", "scratch.a",
                     "scratch.dam", "scratch.xh", "scratch.dy1", "scratch.stat", "scratch.part", "scratch.coef", "scratch.csum")


def sem_train_region(dims: EdttsSemDims, B: int, T: int, which) -> Tuple[int, int]:
    """(offset, bytes) of a member of the tape ("tape.*") or of the scratch ("scratch.*") of a head of either quantizer: a name of
    SEM_TRAIN_REGIONS or its EDTTS_SEM_* number.  A member the head does not have raises."""
    w = SEM_TRAIN_REGIONS.index(which) if isinstance(which, str) else int(which)
    off, n = C.c_size_t(0), C.c_size_t(0)
    lib().edtts_sem_train_region(C.byref(dims), int(B), int(T), w, C.byref(off), C.byref(n))
    return int(off.value), int(n.value)


# ---------------------------------------------------------------------------------------------- HuBERT backbone
def hubert_frames(dims: EdttsHubertDims, n_samples: int) -> int:
    return _size_query(lib().edtts_hubert_frames, C.byref(dims), int(n_samples), ctype=C.c_int64)


# compute dtypes of the HuBERT backbone (include/edtts.h: EDTTS_HUBERT_FP32 / EDTTS_HUBERT_BF16)
HUBERT_DTYPES = {"fp32": 0, "bf16": 1}


def hubert_packed_bytes(dims: EdttsHubertDims, compute_dtype: int = 0) -> int:
    if compute_dtype:
        return _size_query(lib().edtts_hubert_packed_bytes_dt, C.byref(dims), int(compute_dtype))
    return _size_query(lib().edtts_hubert_packed_bytes, C.byref(dims))


def hubert_workspace_bytes(dims: EdttsHubertDims, B: int, T_audio: int, compute_dtype: int = 0) -> int:
    if compute_dtype:
        return _size_query(lib().edtts_hubert_workspace_bytes_dt, C.byref(dims), int(compute_dtype), int(B), int(T_audio))
    return _size_query(lib().edtts_hubert_workspace_bytes, C.byref(dims), int(B), int(T_audio))


def hubert_pack(dims: EdttsHubertDims, tensors: Sequence[torch.Tensor], packed: torch.Tensor, compute_dtype: int = 0) -> None:
    """Pack the backbone's weights (include/edtts.h: edtts_hubert_pack / edtts_hubert_pack_dt, slot order there) into `packed`
    (uint8 device tensor)."""
    ptrs = _slot_ptrs(tensors, "weight")
    if compute_dtype:
        lib().edtts_hubert_pack_dt(C.byref(dims), int(compute_dtype), ptrs, len(tensors), _dev_ptr(packed, torch.uint8, "packed"),
                                   _stream(packed.device))
    else:
        lib().edtts_hubert_pack(C.byref(dims), ptrs, len(tensors), _dev_ptr(packed, torch.uint8, "packed"), _stream(packed.device))


# the sites of the backbone's launch list, as edtts_hubert_forward_until names them (include/edtts.h: EDTTS_HUB_*), in launch order
HUB_SITES = ("lens", "gnstat", "conv0", "conv", "fpnorm", "fproj", "pos", "encnorm", "qkv", "vt", "attn", "oproj", "ln1", "ff1", "ff2",
             "ln2", "zero")
HUB_LAYER_SITES = HUB_SITES[8:16]
HUB_GEMM_SITES = ("conv", "fproj", "pos", "qkv", "oproj", "ff1", "ff2")
# the members of the backbone's workspace, as edtts_hubert_workspace_region names them (include/edtts.h: EDTTS_HUB_WS_*)
HUB_WS_REGIONS = ("lens", "stats", "part", "buf0", "buf1", "h", "att", "big", "vt")
HUB_GN_CHUNK = 256  # conv0 frames per partial sum of the GroupNorm statistics (csrc/edtts_hubert.h: kGnChunk)


def hubert_last_site(dims: EdttsHubertDims, with_lengths: bool) -> Tuple[str, int]:
    """(site, index) of the last launch of a whole forward."""
    if with_lengths:
        return "zero", 0
    return ("ln2", dims.num_layers - 1) if dims.num_layers else ("encnorm", 0)


def hubert_workspace_region(dims: EdttsHubertDims, B: int, T_audio: int, compute_dtype: int, which) -> Tuple[int, int]:
    """(offset, bytes) of a workspace member (a name of HUB_WS_REGIONS or its EDTTS_HUB_WS_* number)."""
    w = HUB_WS_REGIONS.index(which) if isinstance(which, str) else int(which)
    off, n = C.c_size_t(0), C.c_size_t(0)
    lib().edtts_hubert_workspace_region(C.byref(dims), int(compute_dtype), int(B), int(T_audio), w, C.byref(off), C.byref(n))
    return int(off.value), int(n.value)


def hubert_workspace_views(dims: EdttsHubertDims, B: int, T_audio: int, compute_dtype: int, workspace: torch.Tensor) -> dict:
    """Typed views of `workspace` (uint8), one per thing a site of HUB_SITES writes (include/edtts.h, "where each site's output lies"):
    lens int64 [2][B] (conv0 frames | output frames), stats fp32 [B][2][C0], part fp64 [B][chunks][C0][2], conv: a list with stage
    i's output [B][T_i][C_i] (bf16 under compute_dtype bf16 for every stage but the last), fpnorm fp32 [B][T][C_last], h and att fp32
    [B][T][H], qkv [B][T][3H] and ff [B][T][I] (fp32; bf16 under bf16), and under bf16 att16 [B][T][H] and vt [B][heads][head_dim][Tp]."""
    bf = bool(compute_dtype)
    reg = {}
    for name in HUB_WS_REGIONS[:8 + bf]:
        off, n = hubert_workspace_region(dims, B, T_audio, compute_dtype, name)
        reg[name] = workspace[off:off + n]
    nc, H, I = dims.n_conv, dims.hidden, dims.intermediate
    Ts, n = [], int(T_audio)
    for i in range(nc):
        n = (n - dims.conv_kernel[i]) // dims.conv_stride[i] + 1
        Ts.append(n)
    T, C0 = Ts[-1], dims.conv_dim[0]

    def view(raw, dtype, *shape):
        count = 1
        for s in shape:
            count *= s
        return raw.view(dtype)[:count].view(*shape)

    f, h16 = torch.float32, torch.bfloat16
    out = dict(lens=view(reg["lens"], torch.int64, 2, B), stats=view(reg["stats"], f, B, 2, C0),
               part=view(reg["part"], torch.float64, B, (Ts[0] + HUB_GN_CHUNK - 1) // HUB_GN_CHUNK, C0, 2))
    buf = (reg["buf0"], reg["buf1"])
    out["conv"] = [view(buf[i & 1], h16 if bf and i + 1 < nc else f, B, Ts[i], dims.conv_dim[i]) for i in range(nc)]
    out["fpnorm"] = view(buf[nc & 1], f, B, T, dims.conv_dim[nc - 1])
    out["h"], out["att"] = view(reg["h"], f, B, T, H), view(reg["att"], f, B, T, H)
    out["qkv"], out["ff"] = view(reg["big"], h16 if bf else f, B, T, 3 * H), view(reg["big"], h16 if bf else f, B, T, I)
    if bf:
        out["att16"] = view(reg["att"], h16, B, T, H)
        out["vt"] = view(reg["vt"], h16, B, dims.heads, H // dims.heads, (T + 31) // 32 * 32)
    return out


def hubert_forward(dims: EdttsHubertDims, packed: torch.Tensor, wav: torch.Tensor, lengths: Optional[torch.Tensor], out: torch.Tensor,
                   workspace: torch.Tensor, compute_dtype: int = 0, until=None, tile: int = 0) -> None:
    """wav [B, T_audio] -> out [B, T_feat, hidden] on the current stream (include/edtts.h: edtts_hubert_forward / _forward_dt).

    ``until``: (site, index) -- edtts_hubert_forward_until: the same launches, stopped after the last one of that site (a name of
    HUB_SITES or its EDTTS_HUB_* number; index: the conv layer of "conv", the encoder layer of HUB_LAYER_SITES, else 0).  ``tile``:
    0 or the forced GEMM tile width (2: 64 x 64, 4: 128 x 128).  Diagnostics; the whole forward is ``until=None, tile=0``."""
    B, T = wav.shape
    args = (_dev_ptr(packed, torch.uint8, "packed"), _dev_ptr(wav, torch.float32, "wav"), B, T,
            _dev_ptr(lengths, torch.int64, "lengths"), _dev_ptr(out, torch.float32, "out"),
            _dev_ptr(workspace, torch.uint8, "workspace"), _stream(wav.device))
    if until is not None or tile:
        site, index = hubert_last_site(dims, lengths is not None) if until is None else until
        site = HUB_SITES.index(site) if isinstance(site, str) else int(site)
        lib().edtts_hubert_forward_until(C.byref(dims), int(compute_dtype), *args[:-1], site, int(index), int(tile), args[-1])
        return
    if compute_dtype:
        lib().edtts_hubert_forward_dt(C.byref(dims), int(compute_dtype), *args)
    else:
        lib().edtts_hubert_forward(C.byref(dims), *args)


def set_substreams(n: int) -> int:
    """1: every sampler call runs its batch in one piece; n >= 2 (default 4): large batches are cut into up to n sub-batches on as many
    streams (include/edtts.h: edtts_set_substreams).  Returns the previous setting."""
    return int(lib().edtts_set_substreams(int(n)))


def substreams_for(dims: EdttsDims, B: int, T: int) -> int:
    """Sub-batches a sampler call of this shape makes under the current setting."""
    return int(lib().edtts_substreams_for(C.byref(dims), int(B), int(T)))


def set_coop(mode: int) -> int:
    """-1: the cooperative layer kernel is chosen automatically for small grids (default); 0: never; 14 / 24 / 22: force an
    instance (include/edtts.h: edtts_set_coop).  Returns the previous mode."""
    return int(lib().edtts_set_coop(int(mode)))


def profile_enable(max_records: int) -> None:
    lib().edtts_profile_enable(int(max_records))


def profile_collect():
    """((ms, launches) of the fused-layer / attention-half kernels, (ms, launches) of the FFN + tail half kernels) recorded
    since the last call."""
    ms, n = (C.c_double * 2)(), (C.c_int * 2)()
    lib().edtts_profile_collect(ms, n)
    return (ms[0], n[0]), (ms[1], n[1])
