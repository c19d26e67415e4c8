/*
 * edtts.h -- C ABI of libedtts_hip.so: the MI355X (gfx950) implementation of the DDIM few-step sampler path
 * of Krabbens/edge-diffusion-tts.
 *
 * The reference has no FFI of its own (pure Python/PyTorch); the interface this library
 * sits behind is the reference's Python class API.  Each entry point below names the reference code whose
 * arithmetic it replaces (paths relative to /root/reference/edge_diffusion_tts/).  The Python host package
 * (edge-diffusion-tts_amd/edge_diffusion_tts_amd/native.py) binds these symbols with ctypes; INTEGRATION.md
 * shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is a DEVICE pointer unless the comment says "host".
 *   - all tensors are dense fp32, channel-last [B, T, n_mels] / [B, T, hidden]; indices are int64.
 *   - the caller owns every buffer (inputs, outputs, packed weights, workspace); the library never
 *     allocates device memory, never synchronises the host, and only enqueues work on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream).  All calls are graph-capturable.
 *   - return value: 0 on success, a negative EDTTS_ERR_* otherwise; edtts_last_error() returns a
 *     thread-local message for the last failing call.
 *   - threads and streams: any number of host threads may call the library at the same time, on one stream each or on several,
 *     as long as no two calls that are in flight together share a workspace or an output.  A packed blob is read-only to every
 *     call and may be shared; re-packing it must be ordered (by the caller) after every call that reads it.  The library keeps no
 *     device state outside the caller's buffers; its host state is the two run-time switches (edtts_set_substreams /
 *     edtts_set_coop, atomic: each call reads both ONCE and plans and runs under that snapshot), per-device attribute caches and
 *     the side streams of the sub-batch cut (one set per device, caller stream and thread; see below).
 *   - environment switches, read once per process: EDTTS_SUBSTREAMS=1..8 (see edtts_set_substreams, default 4);
 *     EDTTS_DSCONV_UNFUSED=1 forces the three-kernel conv path; EDTTS_DSCONV_NOGROUP=1 / EDTTS_DSCONV_WAVES8=1 select the older
 *     one-kernel forms (A/B hooks: same results within the layer's 1e-5).
 */
#ifndef EDTTS_H_
#define EDTTS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EDTTS_VERSION 400 /* 0.4.0: sub-batches on several streams (edtts_set_substreams); the workspace grew accordingly; cooperative kernels */

enum {
  EDTTS_OK = 0,
  EDTTS_ERR_UNSUPPORTED = -1, /* dims have no compiled kernel instance (and no generic path was asked for), or exceed its limits */
  EDTTS_ERR_ARG = -2,         /* null pointer / size out of range (IndexError/RuntimeError analogue) */
  EDTTS_ERR_HIP = -3          /* a HIP runtime call or launch failed              */
};

/* Bits of the index-error word (edtts_index_errors): an index the reference would have raised IndexError for was
 * clamped into range by a kernel (the kernels never fault on bad indices). */
enum {
  EDTTS_IDX_SEM = 1, /* sem_idx outside [0, codebook_size)   (nn.Embedding, models/decoder.py:88) */
  EDTTS_IDX_STEP = 2, /* step_idx outside [0, n_step_emb)     (models/decoder.py:79-80) */
  EDTTS_IDX_LEN = 4   /* a per-utterance length (edtts_*_len) outside [1, T] / [1, S]; the kernels clamp it */
};

/* Decoder hyper-parameters: the CFG fields read by models/decoder.py:17-64 plus table sizes. */
typedef struct EdttsDims {
  int32_t hidden;        /* CFG.hidden            (config.py:103) */
  int32_t layers;        /* CFG.layers                            */
  int32_t heads;         /* CFG.heads                             */
  int32_t n_mels;        /* CFG.n_mels                            */
  int32_t ffn_mult;      /* CFG.ffn_mult: 1 .. 4 (a run-time tile count of the FFN phases) */
  int32_t codebook_size; /* CFG.codebook_size: rows of token_emb  */
  int32_t semantic_dim;  /* CFG.semantic_dim: sem_proj input      */
  int32_t window;        /* CFG.attn_window_size; < 0 = full self-attention (window_size=None) */
  int32_t max_pos;       /* rows of pos_emb.pe         (decoder.py:38: 1000) */
  int32_t max_ctx_pos;   /* rows of context_pos_emb.pe (decoder.py:41: 512)  */
  int32_t n_step_emb;    /* rows of step_emb           (decoder.py:32: 16)   */
  int32_t compute_dtype; /* EDTTS_F32: everything fp32 (the reference's arithmetic).  EDTTS_BF16: contractions on bf16 MFMA with
                            fp32 accumulation; residual stream, norms, softmax and sampler updates stay fp32 (the reference's AMP
                            precedent: utils/speed_utils.py:70, train_v2.py:290).  head_dim 32 shapes only (hidden = 32 * heads, hidden % 64
                            == 0): built in 256/8/80 (BASELINE config 3) and 64/2/80, more through EDTTS_INSTANCES_BF16 at build time.
                            Kernel-path bits may be ORed in (EDTTS_KERNELS_*, below); without them a shape runs only if it is a
                            compiled kernel instance (EDTTS_ERR_UNSUPPORTED otherwise). */
} EdttsDims;

enum { EDTTS_F32 = 0, EDTTS_BF16 = 1 };

/* Kernel-path bits of EdttsDims.compute_dtype.  The fused kernels are compiled per decoder shape; the generic kernels take every
 * shape as run-time values (slower, fp32 only):
 *   EDTTS_KERNELS_GENERIC  always the generic kernels.  EDTTS_BF16 | EDTTS_KERNELS_GENERIC is EDTTS_ERR_UNSUPPORTED.
 *   EDTTS_KERNELS_AUTO     the compiled instance when there is one, the generic kernels otherwise.  With EDTTS_BF16 it is the
 *                          compiled bf16 path (never a silent fall-back to fp32).
 * Generic limits: hidden % heads == 0, hidden even, head_dim <= 128, any n_mels >= 1 and semantic_dim >= 1, MLA rank hidden / 2,
 * ffn_mult 1..4, layers <= 32, any window.  The choice is made once per dims: edtts_packed_bytes / edtts_pack_weights /
 * edtts_workspace_bytes answer for the path that will run (the generic blob holds the state-dict's [N][K] matrices), so a blob or
 * workspace must be sized and packed with the same bits as the calls that use it.  A generic call runs on `stream` alone
 * (edtts_substreams_for answers 1). */
enum { EDTTS_KERNELS_GENERIC = 0x100, EDTTS_KERNELS_AUTO = 0x200 };

/* Matmul-precision bit of EdttsDims.compute_dtype (mixed-precision training and inference on the generic kernels, DESIGN.md section
 * 26).  Legal only as EDTTS_F32 | EDTTS_KERNELS_GENERIC | EDTTS_MATMUL_BF16; every other combination that carries it -- with
 * EDTTS_BF16, without EDTTS_KERNELS_GENERIC, with EDTTS_KERNELS_AUTO whatever it would resolve to -- is EDTTS_ERR_UNSUPPORTED with a
 * message naming the bit.  With it every contraction the reference writes as a Linear -- in edtts_decoder_forward*, the training
 * forwards and backwards (dX, dW and the recomputed SwiGLU pre-activations; the _drop and _len forms too) and the samplers' eps --
 * rounds both operands to bf16 (nearest even) and multiplies on bf16 MFMAs with fp32 accumulators.  Storage does not change:
 * parameters, the packed blob, the tape, the residual stream, norms, AdaLN, biases and their gradients, softmax and both attentions,
 * the slab sums and every output stay fp32, and edtts_packed_bytes, edtts_workspace_bytes, edtts_train_tape_bytes,
 * edtts_train_scratch_bytes and edtts_generic_slot_dest answer as they do without the bit. */
enum { EDTTS_MATMUL_BF16 = 0x400 };

/* Attention-precision bit of EdttsDims.compute_dtype (the other half of mixed precision on the generic kernels).
 * Legal only as EDTTS_F32 | EDTTS_KERNELS_GENERIC | EDTTS_ATTN_BF16, with or without EDTTS_MATMUL_BF16; every other combination that
 * carries it -- with EDTTS_BF16, without EDTTS_KERNELS_GENERIC, with EDTTS_KERNELS_AUTO whatever it would resolve to -- is
 * EDTTS_ERR_UNSUPPORTED with a message naming the bit.  With it both attentions of every block, in every forward, training forward,
 * backward (the _drop and _len forms too) and sampler entry point, run their contractions on bf16 MFMAs with fp32 accumulators.
 * Rounding contract (nearest even, operands only, nothing is stored as bf16):
 *   forward   S = bf16(q) bf16(k)^T, then * log2(e) / sqrt(head_dim) in fp32 (the operands are the stored values, not pre-scaled
 *             ones); mask, running maximum, exp2, the row sum l and the log-sum-exp in fp32 from the unrounded probabilities;
 *             O = bf16(P~) bf16(v) / l, P~ the unnormalised probability (times keep * scale first under dropout)
 *   backward  delta = rowsum(dO o O) in fp32, unrounded; dP = bf16(dO) bf16(v)^T; P recomputed in fp32 from the recomputed S and the
 *             tape's log-sum-exp; dV = bf16(P o D)^T bf16(dO); dS = P o (D o dP - delta) in fp32; dQ = bf16(dS) bf16(k) / sqrt(head_dim);
 *             dK = bf16(dS)^T bf16(q) / sqrt(head_dim); all accumulators and stores fp32
 * Storage does not change: q | k | v, both attention outputs, the cross K | V rows and the log-sum-exps stay fp32 in the same layout,
 * the dropout masks (edtts_dropout_mask) do not depend on the bit, and edtts_packed_bytes, edtts_workspace_bytes,
 * edtts_train_tape_bytes, edtts_train_scratch_bytes and edtts_generic_slot_dest answer as they do without it. */
enum { EDTTS_ATTN_BF16 = 0x800 };

/* Activation-storage bit of EdttsDims.compute_dtype.  Legal only as EDTTS_F32 | EDTTS_KERNELS_GENERIC |
 * EDTTS_MATMUL_BF16 | EDTTS_ATTN_BF16 | EDTTS_TAPE_BF16; every other combination that carries it is EDTTS_ERR_UNSUPPORTED with a
 * message naming the bit (a buffer with an fp32 reader cannot be narrowed without changing results, and one rule is simpler than
 * four partial ones).  With both other bits, four activation buffers of every layer are read only by loaders that round to bf16:
 *   q|k|v         [B T][3 hidden]         written by the QKV projection, read by the self-attention, forward and backward
 *   cross q       [B T][hidden]           written by q_proj, read by the cross-attention, forward and backward
 *   cross K|V     [B S][2 hidden]         written by kv_up, read by the cross-attention, forward and backward
 *   SwiGLU output [B T][ffn_mult hidden]  written by the FFN's up projection (after its dropout), read by the down projection and dW_down
 * Storage contract: with the bit these four hold __bf16, rounded to nearest even by the conversion those loaders use
 * (v_cvt_pk_bf16_f32), with row pitches counted in elements as before (3 hidden, hidden, 2 hidden, ffn_mult hidden).  Rounding to
 * bf16 is idempotent, so every consumer forms the operand it forms without the bit: eps, every gradient and every sampler output are
 * BITWISE those of the same dims without it.  Everything else stays fp32: the residual stream and its snapshots, both attention
 * outputs (delta reads them unrounded), the kv_down rows, the context and AdaLN rows, the log-sum-exps, every gradient and output.
 * edtts_train_tape_bytes shrinks by those four regions' halves (each region stays 256-byte aligned; edtts_train_tape_region says
 * where each lies).  edtts_workspace_bytes, edtts_train_scratch_bytes, edtts_packed_bytes and edtts_generic_slot_dest answer as they do
 * without the bit: the inference forward and the samplers honour the bit through the same launch list and use the first half of the
 * workspace's q|k|v / SwiGLU buffer and of each layer's K|V buffer.  The dropout masks do not depend on the bit. */
enum { EDTTS_TAPE_BF16 = 0x1000 };

int edtts_version(void);
const char* edtts_last_error(void);

/* ---- weights ------------------------------------------------------------------------------------------
 * The decoder state-dict (key names = SURVEY.md section 8a row 5 = decoder.state_dict() of
 * models/decoder.py:17-64) is handed over as an array of device pointers, one per "slot".  Slots
 * [0, n_global) are the non-layer tensors, then n_layer slots per transformer layer.  The slot -> key-name
 * mapping is queried, so the host never hard-codes the order.  Name "time_freqs" is the one derived slot:
 * the fp32 frequency row of SinusoidalTimeEmb (layers/embeddings.py:38-41), computed by the host exactly as
 * the reference does. */
int edtts_num_global_slots(void);
int edtts_num_layer_slots(void);
const char* edtts_global_slot_name(int i); /* e.g. "token_emb.weight" */
const char* edtts_layer_slot_name(int i);  /* e.g. "attn.qkv.weight" (prefix "layers.<l>." added by the host) */

/* Size of the packed-weight blob (MFMA-fragment order GEMM operands + tables) for these dims. */
int edtts_packed_bytes(const EdttsDims* dims, size_t* out_bytes);
/* Re-pack the state-dict into `packed` (once per weight load). slots: host array of device pointers. */
int edtts_pack_weights(const EdttsDims* dims, const void* const* slots, int n_slots, void* packed, void* stream);

/* ---- workspace ----------------------------------------------------------------------------------------
 * Scratch for activations (h, two ping-pong sets of q, k, v^T), the per-call cross-attention K/V cache and the AdaLN rows.
 * cond_rows = number of (t, step_idx) rows the conditioning kernel is run for (B for a plain forward,
 * num_steps for the fused sampler).  The workspace must be ZERO-FILLED once after allocation (padding
 * lanes are read but never written) and may then be reused for any number of calls of the same shape.
 * The byte count covers every form of a call -- the batch in one piece or cut into any number of sub-batches -- so it does not
 * depend on edtts_set_substreams / edtts_set_coop, and a workspace is never too small for a call under another setting.  Its
 * LAYOUT does depend on the cut (edtts_substreams_for): each sub-batch takes its own slice, with its own padded rows.  A
 * workspace that served a call under one cut and then serves a call under another may therefore hold, in lanes the new layout
 * treats as padding (the padded frames and context rows of each slice), finite values the old layout wrote there.  Padding
 * lanes only ever meet masked scores and zero weights, so results do not change (bitwise; the GPU tests switch the cut on a
 * shared workspace); a caller that wants the zero-fill contract to hold literally keeps one workspace per cut, as the Python
 * host does.  Workspace
 * word 0 (edtts_index_errors) is per workspace: two calls in flight on two workspaces never see each other's bits. */
int edtts_workspace_bytes(const EdttsDims* dims, int B, int T, int S, int cond_rows, size_t* out_bytes);

/* Out-of-range indices: where the reference raises IndexError (token ids >= codebook_size, step_idx >= 16), the kernels clamp
 * the index -- they never fault -- and OR an EDTTS_IDX_* bit into the first word of the workspace.  This call copies that word
 * to *flags_host, clears it, and SYNCHRONISES `stream` (the one call of this library that does; not graph-capturable).  The
 * Python host calls it after every decoder / sampler call when EDTTS_CHECK_INDICES=1 and raises IndexError, as the reference
 * does (a deviation from the reference otherwise: a corrupted token stream yields a plausible mel, silently).
 * (t / t_prev of edtts_ddim_step / edtts_ddpm_step are clamped into the table too; those calls have no workspace, the host
 * checks them with a device reduction in the same debug mode.) */
int edtts_index_errors(void* workspace, int* flags_host, void* stream);

/* ---- decoder forward  (models/decoder.py:66-109, EdgeDiffusionDecoder.forward) --------------------------
 * x [B,T,n_mels], t [B] int64, step_idx [B] int64 or NULL, exactly one of sem_idx [B,S] int64 /
 * sem_features [B,S,semantic_dim] non-NULL (both NULL -> EDTTS_ERR_ARG, the reference's ValueError,
 * decoder.py:90).  Writes eps [B,T,n_mels].  T <= max_pos, S <= max_ctx_pos, step_idx < n_step_emb are the
 * reference's limits; the first two are checked here, index contents are the caller's. */
int edtts_decoder_forward(const EdttsDims* dims, const void* packed, void* workspace, int B, int T, int S,
                          const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                          const float* sem_features, float* eps, void* stream);

/* ---- training: the decoder forward with a tape, and its backward ---------------------------------------------------------
 * For train.py / train_v2.py / training/consistency.py, whose steps call decoder(x_t, t, ...) under autograd (train_v2.py
 * train_step; training/consistency.py consistency_loss calls it twice before one backward()).  First version: generic kernels
 * and fp32 only -- dims.compute_dtype must be EDTTS_F32 | EDTTS_KERNELS_GENERIC, anything else is EDTTS_ERR_UNSUPPORTED with a
 * message naming the cause -- and no per-utterance lengths (those: the *_train_len / *_backward_len calls further down).  These entry points run the decoder.eval() arithmetic (dropout off:
 * layers/attention.py and layers/transformer.py apply dropout only when training); the *_drop twins below add the dropout.  Conventions as everywhere: no allocation, no host synchronisation,
 * work only on `stream`, graph-capturable.  Every reduction has a fixed order: a backward is bitwise reproducible.
 *
 * edtts_train_tape_bytes: size of the caller-owned tape one forward_train call fills and its backward reads (per layer: the
 * residual stream at the three norms, q|k|v, both attention outputs and their log-sum-exps, the cross K|V and kv_down rows, the
 * SwiGLU output; plus the context rows, the AdaLN rows and the residual stream entering final_norm).
 * edtts_train_scratch_bytes: the backward's own scratch (gradient rows and the partial slabs of its cut reductions).
 * edtts_train_dw_slab_rows: rows per partial slab of a weight gradient summed over `rows` rows (a host query). */
int edtts_train_tape_bytes(const EdttsDims* dims, int B, int T, int S, size_t* out_bytes);
int edtts_train_scratch_bytes(const EdttsDims* dims, int B, int T, int S, size_t* out_bytes);
int edtts_train_dw_slab_rows(int rows);

/* Where one member of the tape lies (a host query, for tests and tools): *offset_bytes from the tape's start (a multiple of
 * 256, TCOND excepted: it lies right behind the AdaLN rows), *bytes = elements x *elem_bytes without the alignment padding behind it,
 * *elem_bytes = 4, or 2 for the four regions that EDTTS_TAPE_BF16 narrows when dims carries that bit.  Per-layer members, rows and
 * pitches: KV [B S][2 hidden]; CRP [B S][hidden / 2]; H0, H1, H2, QC, ATT1, ATT2 [B T][hidden]; QKV [B T][3 hidden]; LSE1, LSE2
 * [B][heads][T] (exp2 domain: m + log2 l of the scores times log2(e) / sqrt(head_dim)); ACT [B T][ffn_mult hidden].  Whole-model
 * members, always fp32 (`layer` must still be in range; the answer does not depend on it): COND [B][layers][2][2 hidden], per layer
 * the AdaLN rows of norm1 then norm3, each (1 + scale) then shift; TCOND [B][hidden]; CTX [B S][hidden]; HL [B T][hidden].
 * EDTTS_ERR_ARG for a layer or `which` out of range. */
enum {
  EDTTS_TAPE_CRP = 0,  /* kv_down rows before kv_norm */
  EDTTS_TAPE_KV = 1,   /* cross K|V rows (narrowed) */
  EDTTS_TAPE_H0 = 2,   /* the residual stream entering norm1 / norm2 / norm3 */
  EDTTS_TAPE_H1 = 3,
  EDTTS_TAPE_H2 = 4,
  EDTTS_TAPE_QKV = 5,  /* q|k|v rows (narrowed) */
  EDTTS_TAPE_ATT1 = 6, /* self-attention output and its log-sum-exp */
  EDTTS_TAPE_LSE1 = 7,
  EDTTS_TAPE_QC = 8,   /* cross-attention query rows (narrowed) */
  EDTTS_TAPE_ATT2 = 9, /* cross-attention output and its log-sum-exp */
  EDTTS_TAPE_LSE2 = 10,
  EDTTS_TAPE_ACT = 11, /* SwiGLU output (narrowed) */
  EDTTS_TAPE_COND = 12,  /* AdaLN rows of every layer */
  EDTTS_TAPE_TCOND = 13, /* t_cond, behind the AdaLN rows */
  EDTTS_TAPE_CTX = 14,   /* context rows */
  EDTTS_TAPE_HL = 15     /* the residual stream entering final_norm */
};
int edtts_train_tape_region(const EdttsDims* dims, int B, int T, int S, int layer, int which, size_t* offset_bytes, size_t* bytes,
                            int* elem_bytes);

/* models/decoder.py:66-109 as edtts_decoder_forward runs it on the generic path -- eps is bitwise that call's -- keeping on
 * `tape` what the backward needs.  Arguments as edtts_decoder_forward; the workspace is that call's (edtts_workspace_bytes with
 * cond_rows = B) and may be shared by any number of forwards: the backward never reads it. */
int edtts_decoder_forward_train(const EdttsDims* dims, const void* packed, void* workspace, void* tape, int B, int T, int S,
                                const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                                const float* sem_features, float* eps, void* stream);

/* The gradient of models/decoder.py:66-109 (time_emb / step_emb :77-80, token_emb / sem_proj + context_pos_emb :83-93, in_proj +
 * pos_emb :96-97, the blocks of layers/transformer.py:129-160 with layers/attention.py:77-123, layers/mla.py:118-194 and
 * layers/transformer.py:13-49,64-68, final_norm + out_proj :105-109) with respect to every weight, x and sem_features, given
 * d_eps [B,T,n_mels].  x, t, step_idx, sem_idx / sem_features are the forward's arguments; `tape` is the one that forward filled.
 * grad_slots: host array of n_slots device pointers in edtts_pack_weights slot order; each non-NULL entry receives that tensor's
 * gradient (written, not accumulated), a NULL entry skips it.  The entries of the positional tables and time_freqs (buffers) are
 * ignored.  What does not enter the output -- token_emb with sem_features, sem_proj with sem_idx, step_emb without step_idx -- has
 * a zero gradient: a non-NULL entry is zero-filled (a caller that mirrors torch, which leaves .grad unset there, passes NULL).
 * d_x [B,T,n_mels] and d_sem_features [B,S,semantic_dim] may be NULL.  `scratch`: edtts_train_scratch_bytes.
 * Reads only the tape, the blob and its arguments; `workspace` is not read. */
int edtts_decoder_backward(const EdttsDims* dims, const void* packed, void* workspace, const void* tape, int B, int T, int S,
                           const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                           const float* sem_features, const float* d_eps, void* const* grad_slots, int n_slots, float* d_x,
                           float* d_sem_features, void* scratch, void* stream);

/* ---- training with dropout: Philox masks in the forward and the backward ------------------------------
 * The reference's trainers run decoder.train() with CFG.dropout = 0.2, which drops at four places of every block: the
 * self-attention probabilities after the softmax (layers/attention.py:106-119), the cross-attention probabilities
 * (layers/mla.py:174-190), the SwiGLU output (layers/transformer.py:43) and the FFN's down projection (:45).  The *_drop entry
 * points run that arithmetic with masks of the library's own: torch's random stream is not reproduced.
 *
 * Dropout masks.  thr = round(p * 65536) (ties to even); valid are 0 <= p < 1 with thr <= 65535, anything else is EDTTS_ERR_ARG
 * with a message naming p.  The effective probability is p_eff = thr / 65536 (p = 0.2: 13107 / 65536).  An element is KEPT iff its
 * 16-bit field is >= thr; kept values are multiplied by 1 / (1 - p_eff).  One draw is Philox4x32-10 with key = (seed lo, seed hi) and
 * counter = (c0, c1, c2, c3) -- the rounds of the noise generator above -- and yields eight 16-bit fields: field j is bits
 * [16 (j & 1), +16) of output word j >> 1.  Site ids: 0 self-attention probabilities, 1 cross-attention probabilities, 2 after
 * SwiGLU (width ffn_mult * hidden), 3 after ffn.net.3 (width hidden).  The stream word is c2 = 0x30000 + 4 * layer + site, and
 *     sites 0, 1, utterance b, head h, query q, key k:   c0 = k >> 2, c1 = q >> 1, c3 = b * heads + h, field 4 * (q & 1) + (k & 3)
 *     sites 2, 3, row m = b * T + t, column n:           c0 = n >> 3, c1 = m,      c3 = 0,             field n & 7
 * A mask is a pure function of (seed, site, layer, position): it does not depend on tile shapes, wave counts or launch geometry,
 * the backward regenerates it instead of reading it back, and a test can rebuild it on the host.
 *
 * drop == NULL or drop->p == 0: exactly the launches of the plain entry point, bitwise its results (the plain entry points ARE these
 * calls with NULL).  The backward must be given the EdttsDropout its forward was given.  Tape and scratch sizes are those of the
 * plain calls (the dropped activations take the place of the undropped ones on the tape).  With an EdttsDropout the seed travels
 * BY VALUE in the kernel arguments: no allocation, no host synchronisation, work only on `stream`, and a captured graph replays
 * the masks it was captured with.  With an EdttsDropoutDev (the *_dev entry points below, "dropout key in device memory") the
 * kernels read the seed from device memory when they run, so a captured graph draws the masks of whatever key its replay finds.
 *
 * edtts_dropout_mask writes the keep mask of one (site, layer) as 0 / 1 bytes through the device functions the kernels call:
 * [B, heads, T, T] (site 0), [B, heads, T, S] (site 1), [B * T, ffn_mult * hidden] (site 2) or [B * T, hidden] (site 3). */
typedef struct EdttsDropout {
  float p;       /* drop probability, see above */
  uint64_t seed; /* Philox key */
} EdttsDropout;
int edtts_decoder_forward_train_drop(const EdttsDims* dims, const void* packed, void* workspace, void* tape, int B, int T, int S,
                                     const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                                     const float* sem_features, float* eps, const EdttsDropout* drop, void* stream);
int edtts_decoder_backward_drop(const EdttsDims* dims, const void* packed, void* workspace, const void* tape, int B, int T, int S,
                                const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                                const float* sem_features, const float* d_eps, void* const* grad_slots, int n_slots, float* d_x,
                                float* d_sem_features, void* scratch, const EdttsDropout* drop, void* stream);
int edtts_dropout_mask(const EdttsDims* dims, int site, int layer, int B, int T, int S, const EdttsDropout* drop, uint8_t* keep,
                       void* stream);

/* ---- per-utterance lengths (ragged batches) -----------------------------------------------------------------------------
 * The *_len entry points below take the arguments of their twins plus device int64 [B] length arrays: t_len (frames T_b) and
 * s_len (tokens S_b); where frames are 2 x tokens (edtts_generate_len, edtts_sample_ddpm_len) s_len alone.  NULL = full length
 * (T / S for every utterance); the plain entry points are these calls with NULL.  Contract, for 1 <= T_b <= T, 1 <= S_b <= S:
 *   - row b on frames [0, T_b) is bitwise what the same entry point returns for utterance b alone (B = 1, T = T_b, S = S_b, the
 *     same t / step_idx / injected noise).  In-kernel Philox noise is keyed by the element's index in the padded [B, T, n_mels]
 *     layout, as without lengths, so it does not depend on the lengths;
 *   - nothing past an utterance's lengths is read: not the padding of x / x_T, of sem_features or of sem_idx (no index check there);
 *   - every output (eps, x0, x, the multistep x0 history and intermediates) is exactly 0 on frames [T_b, T);
 *   - the lengths are read by the kernels at run time: a captured graph serves any length mix copied into the same arrays.
 * Values outside [1, T] / [1, S] are clamped into range and set EDTTS_IDX_LEN.  Workspace and blob sizes are those of the twin. */
int edtts_decoder_forward_len(const EdttsDims* dims, const void* packed, void* workspace, int B, int T, int S,
                              const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                              const float* sem_features, const int64_t* t_len, const int64_t* s_len, float* eps, void* stream);

/* ---- training on ragged batches: per-utterance lengths in the training forward and the backward ----------
 * The arguments of the *_drop twins plus t_len / s_len (device int64 [B], frames T_b / tokens S_b) before `stream`.  drop may be
 * NULL (no dropout); each length array may be NULL (full length).  The four entry points above ARE these calls with NULL lengths,
 * bitwise.  Tape and scratch sizes are those of the plain calls (edtts_train_tape_bytes / edtts_train_scratch_bytes).  Argument errors
 * are reported before any pointer is looked at.  Values outside [1, T] / [1, S] are clamped into range and set EDTTS_IDX_LEN in the
 * workspace's index-error word (the backward writes that word and nothing else of `workspace`).
 * Contract, for 1 <= T_b <= T and 1 <= S_b <= S, both independent per utterance:
 *   1. forward: eps is bitwise edtts_decoder_forward_len on the generic path with the same lengths -- so row b on frames [0, T_b)
 *      is bitwise its solo call, and eps is exactly 0 on [T_b, T);
 *   2. nothing past an utterance's lengths enters a result, in the forward or the backward: not the padding of x, sem_features,
 *      sem_idx (no index check there) or d_eps, and not the tape's or the scratch's rows past the lengths.  NaN in that padding, any
 *      int64 in the padding of sem_idx, a tape or scratch pre-filled with 0xFF bytes: no output bit changes.  (The tape's rows past
 *      the lengths hold whatever the forward's row-local steps made of the padding, or were never written; every sum over rows in
 *      the backward predicates its loads on the row being live instead of relying on a zero gradient there);
 *   3. input gradients: d_x[b, :T_b] and d_sem_features[b, :S_b] are bitwise those of the backward called on utterance b alone
 *      (B = 1, T = T_b, S = S_b, the same t / step_idx, d_eps[b, :T_b]); both are exactly 0 past the lengths;
 *   4. weight gradients are the sum over utterances of the solo gradients -- padding rows and tokens contribute exactly nothing.  Not
 *      bitwise the solo sum (the slab boundaries of the cut reductions differ), but bitwise reproducible (fixed reduction orders, no
 *      float atomics) and bitwise independent of what the padding holds;
 *   5. full lengths (T_b = T, S_b = S for all b) give bitwise the gradients of the call without lengths;
 *   6. dropout: the masks stay keyed by the padded layout (c3 = b * heads + h, c1 = b * T + t), so an utterance's masks do not
 *      depend on anybody's lengths; but because the key contains b, the solo equalities of 1 and 3 do NOT hold under dropout.
 *      2, 4 and 5 hold unchanged; 3 becomes: the rows of d_x / d_sem_features of utterance b do not depend on the other
 *      utterances' lengths or contents.
 * The lengths are read by the kernels at run time: a captured graph serves any length mix copied into the same arrays. */
int edtts_decoder_forward_train_len(const EdttsDims* dims, const void* packed, void* workspace, void* tape, int B, int T, int S,
                                    const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                                    const float* sem_features, float* eps, const EdttsDropout* drop, const int64_t* t_len,
                                    const int64_t* s_len, void* stream);
int edtts_decoder_backward_len(const EdttsDims* dims, const void* packed, void* workspace, const void* tape, int B, int T, int S,
                               const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                               const float* sem_features, const float* d_eps, void* const* grad_slots, int n_slots, float* d_x,
                               float* d_sem_features, void* scratch, const EdttsDropout* drop, const int64_t* t_len,
                               const int64_t* s_len, void* stream);

/* ---- diagnostic entry points: a backward that stops, and the scratch's members by name ------------------
 * For tests and tools that audit the backward launch by launch; a trainer needs neither.
 *
 * edtts_decoder_backward_until takes the arguments of edtts_decoder_backward_len plus (stop_layer, stop_site) before `stream`.  It
 * makes exactly the launches of that call, in the same order and with the same arguments, and returns after the last launch of the
 * named site: what the sites before it wrote -- scratch members and gradient destinations -- is bitwise what the whole call writes
 * there at that moment, and the destinations of later sites are not touched.  A site is one line of the backward's launch list, in
 * launch order: the head (OUT, FNORM; stop_layer 0), the per-layer sites DROPDOWN .. N1 for layers L-1 .. 0, and the tail (INP .. TIME;
 * stop_layer 0).  Stopping at the last site the call has is the whole call.  EDTTS_ERR_ARG: stop_layer outside [0, layers) (or not 0
 * for a head or tail site), stop_site out of range, or a site the call does not have -- DROPDOWN without dropout, ADA with neither an
 * AdaLN-projection nor a time-path gradient slot, STEP without step_idx or the step_emb slot, TIME without a time-path slot.  The
 * plain entry points do not change: no added launch, memset, synchronisation or allocation.  Graph-capturable as they are. */
enum {
  EDTTS_BWD_OUT = 0,       /* dctx zero-fill; out_proj bias sum; final-norm recompute -> xn; out_proj dW; dX -> ga */
  EDTTS_BWD_FNORM = 1,     /* final LayerNorm backward: ga -> dh, gain and bias gradients */
  EDTTS_BWD_DROPDOWN = 2,  /* (dropout only) the masked copy of dh -> gq */
  EDTTS_BWD_DOWN = 3,      /* ffn.net.3: bias sum, dW, dX -> da */
  EDTTS_BWD_UPRE = 4,      /* norm3 recompute -> xn; up projection -> big (value | gate pre-activations) */
  EDTTS_BWD_SWIGLU = 5,    /* big <- SwiGLU gradient of (big, da), in place */
  EDTTS_BWD_UP = 6,        /* ffn.net.0: bias sum, dW, dX -> ga */
  EDTTS_BWD_N3 = 7,        /* norm3 backward: dh += ..., gain gradient, dmod (dscale | dshift) */
  EDTTS_BWD_OP = 8,        /* cross out_proj: dW, dX -> ga */
  EDTTS_BWD_CROSS = 9,     /* cross-attention backward: delta, dq -> gq, dk | dv -> dkv */
  EDTTS_BWD_QP = 10,       /* norm2 recompute -> xn; q_proj dW, dX -> ga */
  EDTTS_BWD_N2 = 11,       /* norm2 backward: dh += ..., gain gradient */
  EDTTS_BWD_KVU = 12,      /* kv_norm recompute -> crn; kv_up dW, dX -> dcr */
  EDTTS_BWD_KVN = 13,      /* kv_norm backward: dcr -> dcp, gain gradient */
  EDTTS_BWD_KVD = 14,      /* kv_down: dW, dctx += dX */
  EDTTS_BWD_PROJ = 15,     /* attn.proj: bias sum, dW, dX -> ga */
  EDTTS_BWD_SELF = 16,     /* self-attention backward: delta, dq | dk | dv -> big */
  EDTTS_BWD_QKV = 17,      /* norm1 recompute -> xn; qkv dW, dX -> ga */
  EDTTS_BWD_N1 = 18,       /* norm1 backward: dh += ..., gain gradient, dmod */
  EDTTS_BWD_INP = 19,      /* in_proj: bias sum, dW, dX -> d_x */
  EDTTS_BWD_SEM = 20,      /* sem_proj gradients and d_sem_features, or the token_emb scatter; zero-fills of what does not enter */
  EDTTS_BWD_ADA = 21,      /* per layer and norm the AdaLN projections: bias sum, dW, dtc += dX */
  EDTTS_BWD_STEP = 22,     /* the step_emb scatter of dtc */
  EDTTS_BWD_TIME = 23,     /* the time MLP: recomputation (e, a1, u1) and its gradients */
  EDTTS_BWD_COUNT = 24
};
int edtts_decoder_backward_until(const EdttsDims* dims, const void* packed, void* workspace, const void* tape, int B, int T, int S,
                                 const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                                 const float* sem_features, const float* d_eps, void* const* grad_slots, int n_slots, float* d_x,
                                 float* d_sem_features, void* scratch, const EdttsDropout* drop, const int64_t* t_len,
                                 const int64_t* s_len, int stop_layer, int stop_site, void* stream);

/* Where one member of the backward's scratch lies (a host query): *offset_bytes from the scratch's start (a multiple of 256) and
 * *bytes without the alignment padding behind it; all members are fp32.  Rows and pitches: DH, XN, GA, GQ [B T][hidden]; BIG
 * [B T][max(2 ffn_mult hidden, 3 hidden)] (used at pitch 2 ffn_mult hidden by the FFN, 3 hidden by the self-attention); DA
 * [B T][ffn_mult hidden]; STAT 2 max(B T, B S) (norm_bwd's per-row statistics); DELTA [B][heads][T]; DKV [B S][2 hidden]; CRN, DCR,
 * DCP [B S][hidden / 2]; DCTX [B S][hidden]; DMOD [B][layers][2][2 hidden] (dscale | dshift, as EDTTS_TAPE_COND); DTC, E, A1, U1, DU1
 * [B][hidden]; PART the partial slabs of the cut reductions.  edtts_train_scratch_bytes is the end of PART, rounded up to 256.
 * EDTTS_ERR_ARG for `which` out of range. */
enum {
  EDTTS_SCRATCH_DH = 0, EDTTS_SCRATCH_XN = 1, EDTTS_SCRATCH_GA = 2, EDTTS_SCRATCH_GQ = 3, EDTTS_SCRATCH_BIG = 4, EDTTS_SCRATCH_DA = 5,
  EDTTS_SCRATCH_STAT = 6, EDTTS_SCRATCH_DELTA = 7, EDTTS_SCRATCH_DKV = 8, EDTTS_SCRATCH_CRN = 9, EDTTS_SCRATCH_DCR = 10,
  EDTTS_SCRATCH_DCP = 11, EDTTS_SCRATCH_DCTX = 12, EDTTS_SCRATCH_DMOD = 13, EDTTS_SCRATCH_DTC = 14, EDTTS_SCRATCH_E = 15,
  EDTTS_SCRATCH_A1 = 16, EDTTS_SCRATCH_U1 = 17, EDTTS_SCRATCH_DU1 = 18, EDTTS_SCRATCH_PART = 19
};
int edtts_train_scratch_region(const EdttsDims* dims, int B, int T, int S, int which, size_t* offset_bytes, size_t* bytes);

/* ---- dropout key in device memory --------------------------------------------------------------------
 * The *_dev twins take the arguments of edtts_decoder_forward_train_len, edtts_decoder_backward_len and edtts_dropout_mask with an
 * EdttsDropoutDev in place of the EdttsDropout: p (and with it thr and the scale) stays a host value, the Philox key is one uint64
 * in device memory (8-byte aligned; NULL is EDTTS_ERR_ARG) that every kernel which applies a mask loads once, at an address that is
 * the same for all lanes, before its first draw.  A mask stays the pure function of (key, site, layer, position) described above:
 * with *key == seed every result is bitwise the EdttsDropout call's.  The key must hold the same value when the backward runs as
 * when its forward ran.  drop == NULL or p == 0: the plain launches.  Nothing else differs: no allocation, no synchronisation, and
 * the calls are graph-capturable with a key that changes between replays (edtts_keys_advance writes such keys). */
struct EdttsDropoutDev {
  float p;             /* drop probability, as EdttsDropout.p */
  const uint64_t* key; /* device memory: the Philox key */
};
typedef struct EdttsDropoutDev EdttsDropoutDev;
int edtts_decoder_forward_train_dev(const EdttsDims* dims, const void* packed, void* workspace, void* tape, int B, int T, int S,
                                    const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                                    const float* sem_features, float* eps, const EdttsDropoutDev* drop, const int64_t* t_len,
                                    const int64_t* s_len, void* stream);
int edtts_decoder_backward_dev(const EdttsDims* dims, const void* packed, void* workspace, const void* tape, int B, int T, int S,
                               const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                               const float* sem_features, const float* d_eps, void* const* grad_slots, int n_slots, float* d_x,
                               float* d_sem_features, void* scratch, const EdttsDropoutDev* drop, const int64_t* t_len,
                               const int64_t* s_len, void* stream);
int edtts_dropout_mask_dev(const EdttsDims* dims, int site, int layer, int B, int T, int S, const EdttsDropoutDev* drop, uint8_t* keep,
                           void* stream);

/* ---- DDIM update  (schedule.py:157-202, DiffusionSchedule.get_ddim_step) --------------------------------
 * alpha_bar [n_table] fp32 table; t, t_prev [B] int64 (t_prev < 0 -> alpha_bar_prev = 1); n_per_batch =
 * T*n_mels; eta >= 0; noise [B,T,n_mels] or NULL (required when eta > 0).  Writes x_prev and x0 (clamped
 * to [-3,3]).  Same operation order as the reference: division by sqrt(ab), direction from the raw eps.
 * Alignment: with n_per_batch % 4 == 0 and all tensors 16-byte aligned the kernel moves float4s; any other combination takes a
 * scalar path with identical results (no alignment requirement on the caller). */
int edtts_ddim_step(const float* alpha_bar, int n_table, const float* x, const float* eps, const int64_t* t,
                    const int64_t* t_prev, int B, size_t n_per_batch, float eta, const float* noise,
                    float* x_prev, float* x0, void* stream);

/* ---- DDPM update  (schedule.py:204-238, DiffusionSchedule.ddpm_step) ------------------------------------
 * tables: alphas, alpha_bar, betas, posterior_variance [n_table]; noise [B,T,n_mels] is the draw the
 * reference takes from torch.randn_like (the host supplies it).  Alignment: as edtts_ddim_step. */
int edtts_ddpm_step(const float* alphas, const float* alpha_bar, const float* betas, const float* post_var,
                    int n_table, const float* x, const float* eps, const int64_t* t, int B, size_t n_per_batch,
                    const float* noise, float* x_prev, void* stream);

/* ---- whole sampler loop  (inference.py:23-53, EdgeInference.generate_mel) -------------------------------
 * sem_idx [B,S] int64; x_T [B,2S,n_mels] initial noise (already multiplied by temperature);
 * num_steps in [1, n_step_emb]; timesteps (host) int64[num_steps] as produced by
 * range(diff_steps-1, 0, -stride)[:num_steps]; coef (host) float[num_steps*4] =
 * {sqrt(1-ab_t), sqrt(ab_t), sqrt(ab_prev), sqrt(1-ab_prev)} per step (eta = 0), computed in fp32 by the
 * host with the reference's own expressions.  x_work [B,2S,n_mels] is scratch for x_t; x0_out receives the
 * last step's clamped x0 prediction (what generate_mel returns, inference.py:53).
 * The cross-attention K/V and all AdaLN rows are computed once per call; each step's final transformer
 * layer fuses final_norm + out_proj + the DDIM update. */
int edtts_generate(const EdttsDims* dims, const void* packed, void* workspace, int B, int S,
                   const int64_t* sem_idx, const float* x_T, int num_steps, const int64_t* timesteps_host,
                   const float* coef_host, float* x_work, float* x0_out, void* stream);
int edtts_generate_len(const EdttsDims* dims, const void* packed, void* workspace, int B, int S, const int64_t* sem_idx,
                       const int64_t* s_len, const float* x_T, int num_steps, const int64_t* timesteps_host, const float* coef_host,
                       float* x_work, float* x0_out, void* stream);

/* ---- full-schedule ancestral sampler  (BASELINE config 5; schedule.py:204-238 applied num_steps times) -----------
 * The loop the reference implies but never wrote: for i = 0 .. num_steps-1, t = t_first - i:
 *     eps = decoder(x, t, sem_idx, step_idx=None);   x = ddpm_step(x, t, eps)
 * with the conditioning rows of all steps and the cross-attention K/V computed once, and the DDPM update
 * fused into the last transformer layer of every step.  x_T [B,2S,n_mels]; t_all (device) int64[num_steps] =
 * the timesteps in the order they are visited; coef (host) float[num_steps*3] = {1/sqrt(alpha_t),
 * beta_t/sqrt(1-alpha_bar_t), [t>0]*sqrt(posterior_variance_t)} per step (schedule.py:227-237).
 * Noise: noise_all [num_steps,B,2S,n_mels] if non-NULL (parity runs inject the draws the oracle used),
 * otherwise standard normals from an in-kernel Philox4x32-10 generator keyed by (seed, step, GLOBAL element index), where
 * global element = batch_offset*2S*n_mels + local element: a rank that samples rows [lo, hi) of a batch passes batch_offset = lo
 * and draws what a single GPU would have drawn for those rows.  seed and step are by-value kernel arguments: a captured
 * hipGraph replays the SAME noise; to advance it, re-capture or update the kernel node parameters with a new seed.
 * The workspace must have been sized with cond_rows = num_steps.  x_out receives x after the last step. */
int edtts_sample_ddpm(const EdttsDims* dims, const void* packed, void* workspace, int B, int S,
                      const int64_t* sem_idx, const float* x_T, int num_steps, const int64_t* t_all,
                      const float* coef_host, const float* noise_all, uint64_t seed, int64_t batch_offset, float* x_out,
                      void* stream);
int edtts_sample_ddpm_len(const EdttsDims* dims, const void* packed, void* workspace, int B, int S, const int64_t* sem_idx,
                          const int64_t* s_len, const float* x_T, int num_steps, const int64_t* t_all, const float* coef_host,
                          const float* noise_all, uint64_t seed, int64_t batch_offset, float* x_out, void* stream);

/* ---- start noise  (inference.py:33: torch.randn(B, T_out, n_mels) * temperature) ---------------------------------
 * out[i] = scale * N(0,1) drawn from the Philox4x32-10 stream (seed, stream_id) at GLOBAL element index elem_offset + i, for
 * i in [0, n): a rank that owns rows [lo, hi) of a batch passes elem_offset = lo*T*n_mels and gets exactly the values a
 * single GPU would draw for those rows (shard-count-invariant, no global draw).  n and elem_offset multiples of 4; n = 0 is a
 * no-op (out may be NULL then: the empty shard of a rank that has no utterances).
 *
 * Philox stream ids.  Every draw of the library is keyed (seed, stream id, global element).  The id space is split so that two
 * draws made with one seed can never coincide:
 *     [0x00000, 0x10000)  edtts_randn callers (0 = start noise of generate_mel / sample_ddpm; the host-side long-form sampler
 *                         uses 0x51 start noise, 0x52 q_sample noise of the teacher refinement, 0x53 per-chunk coarse noise;
 *                         0x54 training q_sample noise: edtts_objective_prepare / edtts_objective_loss, element e of a row)
 *     0x10000 + step      ancestral noise of step `step` inside edtts_sample_ddpm
 *     0x20000 + step      q_sample noise of the known frames at step `step` inside edtts_sample_inpaint and
 *                         edtts_sample_inpaint_multistep_len (one sampler or the other runs on a seed: the same draws)
 *     0x30000 + 4 * layer + site   dropout masks of the training forward and backward (edtts_decoder_forward_train_drop; layers
 *                         <= 32: [0x30000, 0x30080)), keyed by position as described there, not by global element
 *     0x40000             dropout mask of the semantic head's proj (edtts_sem_encode_train), keyed by position as sites 2 and 3
 *     0x50000             the key stream (edtts_keys_advance): counter = (slot, call lo, 0x50000, call hi), see there
 * edtts_randn rejects stream_id >= 0x10000. */
int edtts_randn(float* out, size_t n, uint64_t seed, uint32_t stream_id, uint64_t elem_offset, float scale, void* stream);
/* One launch for B rows with a seed each: out [B, n_per_row], row b bitwise what edtts_randn(n_per_row, seeds[b], stream_id, offset 0,
 * scale) draws, so a longer row begins with a shorter row's draws (the host draws of a batched edtts_sample_inpaint_len call).
 * seeds: device uint64 [B].  n_per_row need not be a multiple of 4 (element e of a row is lane e & 3 of draw e >> 2, as in
 * edtts_randn); out is 16-byte aligned when it is.  B = 0 or n_per_row = 0 is a no-op. */
int edtts_randn_rows(float* out, int B, size_t n_per_row, const uint64_t* seeds, uint32_t stream_id, float scale, void* stream);

/* ---- key stream: Philox keys that a captured graph regenerates on every replay -------------------------
 * state: device uint64 [2] = (base seed, call counter c); keys: device uint64 [n].  edtts_keys_advance writes
 *     keys[i] = K(base, c, i) for i in [0, n)   and then   state[1] = c + 1
 * in one launch of one block (a block-stride loop; a barrier stands between the last read of c and its store).  With
 * w = philox4x32_10(key = (base lo, base hi), counter = (i, c lo, 0x50000, c hi)):  K = (w[0] | w[1] << 32) with bit 63 cleared --
 * 63 bits, a legal int64 row seed for edtts_objective_prepare and a key for EdttsDropoutDev.  No allocation, no host
 * synchronisation, graph-capturable: every replay finds the counter its predecessor left and writes the next keys.
 * edtts_keys_host is the same function on the host (no GPU call): out[j] = K(base, counter, first + j) for j in [0, n), so the keys
 * of any replay can be recomputed.  first + n <= 2^32. */
int edtts_keys_advance(uint64_t* keys, int n, uint64_t* state, void* stream);
int edtts_keys_host(uint64_t base, uint64_t counter, int64_t first, int n, uint64_t* out);

/* ---- multistep x0-solver sampler  (schedule.py:440-527, DPMSolverPP.sample with the updates of :339-438) -------
 * For step i = 0 .. num_steps-1 (t = timesteps_host[i], step_idx = i as in schedule.py:475-479):
 *     out = decoder(x, t, sem_idx | sem_features, step_idx=i)
 *     x0  = clamp(p0*x + p1*out, -3, 3)                       (v-prediction: p0 = sqrt(ab_t), p1 = -sqrt(1-ab_t); x0-pred: 0, 1)
 *     mode 1:  x = c0*x + c1*x0                                                               (first_order_update)
 *     mode 2:  x = c0*x + c1*x0 + cB*(rinv*(x0 - h_new))*0.5                                  (second_order_update)
 *     mode 3:  x = c0*x + c1*x0 + cB*(x0 - h_old)*0.5 + cC*(x0 - 2*h_old + h_new)/6           (third_order_update)
 * fused into the last transformer layer of each step; h_new / h_old are the previous two clamped x0 predictions.
 * coef_host: float[num_steps*8] = {mode, p0, p1, c0, c1, rinv, cB, cC} per step, computed by the host from the schedule
 * tables with the reference's expressions.  hist: scratch [2,B,T,n_mels]; x0_all: NULL or [num_steps,B,T,n_mels] to receive
 * every step's x0 (return_intermediates).  Exactly one of sem_idx / sem_features is non-NULL.  Workspace sized with
 * cond_rows = num_steps (<= n_step_emb).  x_out receives the final x. */
int edtts_sample_multistep(const EdttsDims* dims, const void* packed, void* workspace, int B, int T, int S,
                           const int64_t* sem_idx, const float* sem_features, const float* x_T, int num_steps,
                           const int64_t* timesteps_host, const float* coef_host, float* hist, float* x0_all,
                           float* x_out, void* stream);
int edtts_sample_multistep_len(const EdttsDims* dims, const void* packed, void* workspace, int B, int T, int S,
                               const int64_t* sem_idx, const float* sem_features, const int64_t* t_len, const int64_t* s_len,
                               const float* x_T, int num_steps, const int64_t* timesteps_host, const float* coef_host, float* hist,
                               float* x0_all, float* x_out, void* stream);

/* ---- long-form in-painting sampler  (/root/reference/inference_pipeline.py:97-140 inpaint_student_sample, :145-196
 * inpaint_teacher_refine) -------------------------------------------------------------------------------------------
 * A v-prediction sampler on the sem_features context with a CONSTANT step index (3 for the student, 0 for the teacher).  x [B,T,
 * n_mels] holds the start point on entry (noise, or q_sample(x_coarse, t_start) -- the host draws it) and the result on return.
 * t_all / step_all: device int64[num_steps], the timesteps in visiting order and the (constant) step index of every step.
 * For step i = 0 .. num_steps-1 (t = t_all[i], t_next = t_all[i+1] or 0):
 *     if known_mel:  x[:, :overlap_len] = sqrt_ab[t] * known_mel + sqrt_1mab[t] * noise_i        (q_sample of the previous chunk's tail)
 *     v = decoder(x, t, sem_features, step_idx)
 *     if cfg_scale != 1:  v = v_u + cfg_scale * (v - v_u),  v_u = decoder(x, t, zero_features, step_idx)   (classifier-free guidance)
 *     x0 = clamp(sqrt_ab[t] x - sqrt_1mab[t] v, -3, 3);  eps = sqrt_1mab[t] x + sqrt_ab[t] v
 *     x  = sqrt(ab[t_next]) x0 + sqrt(1 - ab[t_next]) eps
 * and finally x[:, :overlap_len] = known_mel.  The blend, the guidance combine and the update are fused into the last transformer
 * layer of the conditional pass; the context K/V of both passes is built once.
 * coef_host: float[num_steps*4] = {sqrt_ab[t], sqrt_1mab[t], sqrt(ab[t_next]), sqrt(1-ab[t_next])}.  known_mel [B,overlap_len,n_mels]
 * or NULL.  noise_k [num_steps,B,overlap_len,n_mels] (the reference's torch.randn_like draws; parity runs inject them) or NULL ->
 * in-kernel Philox keyed by (seed, step, element).  cfg_scale != 1 needs a second workspace (same size), an all-zero feature
 * tensor [B,S,semantic_dim] and a scratch v_uncond [B,T,n_mels].  Workspaces sized with cond_rows = num_steps. */
int edtts_sample_inpaint(const EdttsDims* dims, const void* packed, void* workspace, void* workspace_uncond, int B, int T, int S,
                         const float* sem_features, const float* zero_features, float* x, int num_steps,
                         const int64_t* t_all, const int64_t* step_all, const float* coef_host, const float* known_mel,
                         int overlap_len, const float* noise_k, uint64_t seed, float cfg_scale, float* v_uncond, void* stream);
/* ... with per-utterance lengths and seeds (the arguments of edtts_sample_inpaint plus three; NULL = as edtts_sample_inpaint):
 * t_len / s_len: device int64 [B] frame / token counts, as the other *_len entry points (the contract above them holds, with the
 * same t_all, steps, overlap_len and cfg_scale; the unconditional pass takes the same lengths, its zero context S_b rows).
 * seeds: device uint64 [B]: row b's in-kernel q_sample noise is Philox keyed by (seeds[b], step, element index WITHIN the row's
 * [overlap_len, n_mels] block), which is what the call on row b alone with seed = seeds[b] draws; `seed` is then unused.
 * Row b injects its first min(overlap_len, T_b) known frames, at every step and in the final force; with a known tail, T_b <
 * overlap_len is flagged with EDTTS_IDX_LEN (the call on that row alone would refuse the overlap).  With seeds = t_len = s_len =
 * NULL the results are bitwise those of edtts_sample_inpaint. */
int edtts_sample_inpaint_len(const EdttsDims* dims, const void* packed, void* workspace, void* workspace_uncond, int B, int T, int S,
                             const float* sem_features, const float* zero_features, float* x, int num_steps,
                             const int64_t* t_all, const int64_t* step_all, const float* coef_host, const float* known_mel,
                             int overlap_len, const float* noise_k, uint64_t seed, float cfg_scale, float* v_uncond,
                             const int64_t* t_len, const int64_t* s_len, const uint64_t* seeds, void* stream);

/* ---- long-form in-painting sampler with the multistep x0-solver update  (inference_pipeline.py:145-196 inpaint_teacher_refine with
 * the step of schedule.py:440-527 DPMSolverPP.sample in place of its first-order one) ----------------------------------------------
 * The arguments of edtts_sample_inpaint_len, with coef_host in edtts_sample_multistep's layout, plus that sampler's hist and x0_all.
 * For step i = 0 .. num_steps-1 (t = t_all[i], step_idx = step_all[i]: constant for the long-form pipeline, i for DPMSolverPP.sample):
 *     if known_mel:  x[:, :overlap_len] = sqrt_ab[t] * known_mel + sqrt_1mab[t] * noise_i        (q_sample of the previous chunk's tail)
 *     v = decoder(x, t, sem_features, step_idx)
 *     if cfg_scale != 1:  v = v_u + cfg_scale * (v - v_u),  v_u = decoder(x, t, zero_features, step_idx)   (classifier-free guidance)
 *     x0 = clamp(p0*x + p1*v, -3, 3)                          (model_to_x0 of a v-prediction model: p0 = sqrt_ab[t], p1 = -sqrt_1mab[t])
 *     x  = first / second / third_order_update over x0 and the previous two x0 (mode 1 / 2 / 3, as edtts_sample_multistep)
 * and finally x[:, :overlap_len] = known_mel.  Guidance combine, x0, update, history and the NEXT step's blend (after the last step:
 * the final force) are fused into the last transformer layer of the conditional pass; step 0's blend is one small launch.
 * coef_host: float[num_steps*8] = {mode, p0, p1, c0, c1, rinv, cB, cC} per step (DPMSolverPP(predict_x0=False).step_coefficients);
 * the blend takes sqrt_ab[t] = p0 and sqrt_1mab[t] = -p1 from it.  mode <= i + 1 (a step cannot use more history than there is).
 * hist: scratch [2,B,T,n_mels]; x0_all: NULL or [num_steps,B,T,n_mels] (every step's clamped x0).  noise_k [num_steps,B,overlap_len,
 * n_mels] or NULL -> Philox stream 0x20000 + i keyed by (seed, element) or, with seeds, (seeds[b], element within the row's block):
 * the draws of edtts_sample_inpaint_len.  Lengths, seeds, guidance buffers and workspaces (cond_rows = num_steps) as there: row b of
 * a ragged batch is bitwise the call on utterance b alone, frames past T_b come out 0 (in x, hist and x0_all), T_b < overlap_len is
 * flagged with EDTTS_IDX_LEN.  With known_mel = NULL, cfg_scale = 1 and step_all[i] = i the result is bitwise
 * edtts_sample_multistep_len's. */
int edtts_sample_inpaint_multistep_len(const EdttsDims* dims, const void* packed, void* workspace, void* workspace_uncond, int B, int T,
                                       int S, const float* sem_features, const float* zero_features, float* x, int num_steps,
                                       const int64_t* t_all, const int64_t* step_all, const float* coef_host, const float* known_mel,
                                       int overlap_len, const float* noise_k, uint64_t seed, float cfg_scale, float* v_uncond,
                                       const int64_t* t_len, const int64_t* s_len, const uint64_t* seeds, float* hist, float* x0_all,
                                       void* stream);

/* ---- in-painting anywhere: the two samplers above with a per-frame mask in place of the known prefix ------------------------------
 * The reference's rule does not depend on where the known frames sit (inference_pipeline.py:117-123,135-136: x[mask] = q_sample(
 * known, t) before every step, x[mask] = known after the last); its pipeline only ever fills a prefix of the mask.  These entry
 * points take the whole mask: the arguments of edtts_sample_inpaint_len / edtts_sample_inpaint_multistep_len, except that
 *     known_mel is [B,T,n_mels]                  (read at kept frames only),
 *     keep      is device uint8 [B,T] in place of overlap_len: non-zero = the frame is known,
 *     noise_k   is [num_steps,B,T,n_mels] or NULL -> Philox  (read at kept frames only).
 * keep and known_mel are both given or both NULL (one without the other: EDTTS_ERR_ARG); both NULL is the plain sampler.  There is no
 * minimum utterance length: t_len[b] in [1, T] as everywhere, and a kept frame at or past t_len[b] is ignored (those frames come out
 * 0).  Each step's q_sample and the final force are one small launch each (k_inpaint_inject_mask); the multistep tails carry no blend.
 * The whole call is one chain on the caller's stream and makes no host-to-device copy, so it can be captured.
 * Philox draws: with seeds, (seeds[b], 0x20000 + step, element f*n_mels + m within the row); without, (seed, 0x20000 + step, element
 * b*T*n_mels + f*n_mels + m).  Contract:
 *   1. keep[b][f] = (f < ov) with seeds given is bitwise the prefix entry point called with known_mel[:, :ov] and overlap_len = ov
 *      (lengths, guidance and every solver mode included); without seeds this holds for B = 1.
 *   2. Kept frames below t_len[b] come out bitwise known_mel.
 *   3. An all-zero keep is bitwise the call with known_mel = keep = NULL; an all-ones keep returns known_mel.
 *   4. known_mel and noise_k are not read at frames that are not kept or lie past t_len[b] (NaN there changes no bit).
 *   5. Row b of a ragged batch with seeds is bitwise the call on utterance b alone (its first t_len[b] frames, seed = seeds[b]).
 *   6. Two calls give equal results.
 * The entry points above are untouched: their results are bit for bit what they were. */
int edtts_sample_inpaint_mask_len(const EdttsDims* dims, const void* packed, void* workspace, void* workspace_uncond, int B, int T, int S,
                                  const float* sem_features, const float* zero_features, float* x, int num_steps,
                                  const int64_t* t_all, const int64_t* step_all, const float* coef_host, const float* known_mel,
                                  const uint8_t* keep, const float* noise_k, uint64_t seed, float cfg_scale, float* v_uncond,
                                  const int64_t* t_len, const int64_t* s_len, const uint64_t* seeds, void* stream);
int edtts_sample_inpaint_multistep_mask_len(const EdttsDims* dims, const void* packed, void* workspace, void* workspace_uncond, int B,
                                            int T, int S, const float* sem_features, const float* zero_features, float* x, int num_steps,
                                            const int64_t* t_all, const int64_t* step_all, const float* coef_host, const float* known_mel,
                                            const uint8_t* keep, const float* noise_k, uint64_t seed, float cfg_scale, float* v_uncond,
                                            const int64_t* t_len, const int64_t* s_len, const uint64_t* seeds, float* hist, float* x0_all,
                                            void* stream);

/* ---- depthwise-separable Conv1d  (layers/conv.py:25-64, DepthwiseSeparableConv.forward) -----------------
 * Standalone exported layer (named by the north star; the decoder never calls it).
 * x [B,C_in,T] channel-first; dw [C_in,k] depthwise taps (Conv1d(k, stride, padding = k/2, groups = C_in, no bias),
 * conv.py:33-41: T_out = (T + 2*(k/2) - k) / stride + 1); pw [C_out,C_in], pb [C_out]; GroupNorm(groups, eps 1e-5, affine
 * gn_w/gn_b [C_out]) then exact (erf) GELU -> y [B,C_out,T_out].
 * C_in <= 80, C_out <= 160, T_out <= 512 AND 127 * stride + ksize <= 260 (the reference's shape class: k = 3 / 5 at stride 1 or 2;
 * the raw rows of one 128-frame pass must fit the kernel's staging tile) run as ONE kernel whose intermediate never leaves
 * registers, and scratch may be NULL; every other shape (stride 3, a large ksize, more channels or frames) takes a three-kernel
 * path and needs scratch of B*C_out*T_out + 2*B*groups floats -- a NULL scratch is then EDTTS_ERR_ARG.
 * (Within the one-kernel class, the layer the reference constructs -- C_out = 160, groups = 8, stride 1, k <= 5 -- runs a
 * group-pipelined form whose stores overlap its MFMAs; the contract is the same.)
 * edtts_dsconv_scratch_floats answers for a given shape: 0 (one kernel, no scratch) or that count. */
int edtts_dsconv_scratch_floats(int B, int C_in, int C_out, int T, int ksize, int stride, int groups, size_t* out_floats);
int edtts_dsconv_forward(const float* x, const float* dw, const float* pw, const float* pb, const float* gn_w,
                         const float* gn_b, int B, int C_in, int C_out, int T, int ksize, int stride, int groups,
                         float* scratch, float* y, void* stream);

/* ---- mel post-processing  (the step after the sampler in the reference's scripts: generate_sample.py:115-145,
 * inference_pipeline.py:382-396) -----------------------------------------------------------------
 * edtts_mel_to_spec: with mean/std [B,n_mels]: denormalize_mel (utils/audio.py:17-19: mel_n * std + mean) -> exp ->; with both
 * NULL the input already is the linear mel spectrogram ->
 * torchaudio.transforms.InverseMelScale (driver "gelsd": the minimum-norm least-squares solution, i.e. multiplication by the
 * pseudo-inverse `pinv` [n_freqs,n_mels] of the transposed mel filter bank, computed once by the host) -> relu.
 * mel_n [B,T,n_mels] -> spec [B,n_freqs,T] (the reference's / torch's layout, power spectrogram).
 * edtts_griffin_lim: torchaudio.functional.griffinlim(rand_init=True, length=None): magnitude = spec^(1/power); n_iter times
 * {istft -> stft(center, reflect) -> angles = (rebuilt - m*prev) / (|.| + 1e-16), m = momentum/(1+momentum)}; final istft.
 * window [n_fft] (hann, win_length = n_fft); twiddle [n_fft/2][2] = exp(-2 pi i q / n_fft) (host table, fp64-evaluated);
 * angles0 [B,n_freqs,T,2] = the complex torch.rand draw the reference starts from (parity runs inject it) or NULL -> hashed
 * uniforms keyed by (seed, element).  scratch: edtts_griffin_lim_scratch_floats floats.  wave_out [B, hop*(T-1)].
 * Compiled for n_fft = 1024 (CFG.n_fft).  PARITY UNPINNED for these two entry points: the reference calls torchaudio, which
 * cannot be installed offline; the oracle restates torchaudio's published algorithm on torch.stft / torch.istft. */
int edtts_mel_to_spec(const float* mel_n, const float* mean, const float* stdv, const float* pinv, int B, int T, int n_mels,
                      int n_freqs, float* spec, void* stream);
int edtts_griffin_lim_scratch_floats(int B, int T, int n_fft, int hop, size_t* out_floats);
int edtts_griffin_lim(const float* spec, int B, int T, int n_fft, int hop, const float* window, const float* twiddle, int n_iter,
                      float momentum, float power, const float* angles0, uint64_t seed, float* scratch, float* wave_out,
                      void* stream);
/* ... with per-utterance frame counts (the arguments of the twin plus the ones named here; the twins remain and are unchanged):
 * t_len: device int64 [B], rows padded to the common T; row b has T_b = t_len[b] frames, clamped into [1, T]; NULL = T for every row.
 * idx_err: NULL, or one device uint32 the caller owns and zeroes once (edtts_index_errors reads and clears it, as it does a workspace):
 * a t_len[b] outside [1, T] sets EDTTS_IDX_LEN in it -- for edtts_griffin_lim_len also a T_b with hop*(T_b-1) <= n_fft/2, a row the
 * call on it alone refuses (it is computed all the same, its reflection clamped into the row).
 * edtts_mel_to_spec_len: frames t >= T_b are written as 0 and their input is never read; frames are independent, so row b is
 * bitwise the call on mel_n[b, :T_b] alone.  smooth_h x smooth_w (0 x 0: none; otherwise both odd, <= 9, mean = std = NULL, n_mels <=
 * 256) first box-filters the linear mel over smooth_h mel bins x smooth_w frames with zeros outside 0 <= m < n_mels, 0 <= t < T_b:
 * F.avg_pool2d(lin_mel, (h, w), stride=1, padding=(h/2, w/2)) (count_include_pad; inference_pipeline.py:376-399 uses 5 x 3), the
 * row's own end being the edge -- again bitwise the call on the row alone.
 * edtts_griffin_lim_len: t_len non-NULL.  Row b's padded signal is n_fft + hop*(T_b-1) long, its STFT reflects at its own end, and
 * wave_out[b] is hop*(T_b-1) samples followed by zeros up to hop*(T-1).  seeds: device uint64 [B], needed when angles0 is NULL: row
 * b's draws are keyed by (seeds[b], f*T_b + t), the element index of the call on the row alone (B = 1, T = T_b) -- so row b is
 * bitwise edtts_griffin_lim on spec[b, :, :T_b] with seed = seeds[b] (or angles0[b, :, :T_b]) in its first hop*(T_b-1) samples.
 * The [.., T] strides of spec / angles0 and the scratch size (edtts_griffin_lim_scratch_floats(B, T, ..)) are the padded batch's;
 * the scratch state of padded frames is neither written nor read.  No allocation, no host synchronisation (graph-capturable). */
int edtts_mel_to_spec_len(const float* mel_n, const float* mean, const float* stdv, const float* pinv, int B, int T, int n_mels,
                          int n_freqs, const int64_t* t_len, int smooth_h, int smooth_w, void* idx_err, float* spec, void* stream);
int edtts_griffin_lim_len(const float* spec, int B, int T, int n_fft, int hop, const float* window, const float* twiddle, int n_iter,
                          float momentum, float power, const float* angles0, const int64_t* t_len, const uint64_t* seeds,
                          void* idx_err, float* scratch, float* wave_out, void* stream);

/* ---- measurement hook (bench.py roofline leg) -----------------------------------------------------------
 * edtts_profile_enable(n > 0): from now on every transformer-layer kernel launch is bracketed by a pair of
 * hipEvents recorded on the stream it is launched on, up to n launches; n = 0 disables and releases the events.
 * A decoder layer is one fused launch (kind 0); kind 1 (the FFN + tail half of a two-launch layer, no longer built)
 * always reports 0.  edtts_profile_collect synchronises on the recorded events, returns the summed device time (ms) and
 * the launch count per kind (arrays of 2), and resets the counter.  Not graph-capturable while on.  Any thread may switch it;
 * while it is on, the bracketed launches of all threads take one lock in turn. */
int edtts_profile_enable(int max_records);
int edtts_profile_collect(double* ms_by_kind, int* launches_by_kind);

/* ---- sub-batches on several streams -------------------------------------------------------------------------
 * The sampler loops (edtts_generate, edtts_sample_multistep, edtts_sample_ddpm) cut a batch whose layer launches are at least two
 * full rounds of one wave per SIMD (B * ceil(T/32) >= 2 * 4 * #CUs: B >= 128 at T = 512 on an MI355X) into sub-batches that walk
 * the same launch sequence on several streams -- `stream` and library-owned non-blocking ones, forked from and joined back into
 * `stream` with events inside the call (graph-capturable; the caller sees ordinary stream semantics) -- so that one sub-batch's
 * waves fill the SIMDs another's finishing launch leaves idle.  How many: as many as still leave each sub-batch two rounds of
 * waves, at least two, at most n (B = 256: two at T = 512, four at T = 1024).  Results do not depend on the cut (bitwise).
 * n = 1 switches the cut off (per-kernel profiling wants launches that do not share the device); the default is 4 (environment
 * EDTTS_SUBSTREAMS at load time), the maximum 8.  Returns the previous value; values outside [1, 8] only query.
 * edtts_substreams_for: the number of sub-batches a call of that shape makes under the current setting.
 * The side streams and fork / join events are owned per (device, caller stream) and per calling thread: two caller streams never
 * share a side stream, so their cuts run independently and each call joins only its own branches.  A thread keeps up to 8 such
 * sets (the least recently used one is rebound to a new caller stream); at thread exit they pass to a pool the next thread reuses. */
int edtts_set_substreams(int n);
int edtts_substreams_for(const EdttsDims* dims, int B, int T);

/* ---- small grids: the cooperative layer kernel ---------------------------------------------------------------
 * A decoder forward whose 32-frame tiles number at most half of the device's SIMDs (B * ceil(T/32) <= 2 * #CUs: B <= 32 at
 * T = 512, and the reference's B = 1 calls) runs its transformer layers with 2 or 4 waves per frame tile (csrc/edtts_coop.h:
 * attention split by heads, GEMMs by output tiles, exchanged through LDS) instead of one; the instance is chosen from the tile
 * count.  Results are bitwise those of the one-wave kernels.  Compiled for the fp32 decoders (160, 4, 80) and (256, 8, 80; without the
 * 32-frame x 2 form, whose tile state does not fit a CU twice).
 * mode: -1 automatic (default; environment EDTTS_COOP at load time), 0 off, 14 / 24 / 22 force (16-frame tiles x 4 waves,
 * 32-frame tiles x 4 waves, 32-frame tiles x 2 waves) -- for tests and measurements.  Returns the previous mode; other values
 * only query. */
int edtts_set_coop(int mode);

/* ---- semantic head  (models/encoder.py:40-57 proj, models/fsq.py FSQEncoder, models/vq.py VectorQuantizer) --------------------
 * The trained head after the frozen HuBERT backbone: HuBERT features h [B,T,in_dim] -> z = proj(h) [B,T,semantic_dim] ->
 * FSQ or VQ tokens.  HuBERT itself stays outside the library.  All fp32, eval semantics (Dropout = identity, loss 0).
 * Limits (EDTTS_ERR_UNSUPPORTED outside): semantic_dim a multiple of 16 in [16, 128]; in_dim a multiple of 16 in [16, 4096], or 0
 * for the quantizer alone (the input is then z itself and there is no proj); FSQ: 1..16 levels, each in [2, 256], at most 2^24
 * codes; VQ: codebook_size in [1, 65536]. */
enum { EDTTS_SEM_FSQ = 0, EDTTS_SEM_VQ = 1 };
typedef struct EdttsSemDims {
  int32_t in_dim;        /* HuBERT width (768), or 0: no proj                        */
  int32_t semantic_dim;  /* CFG.semantic_dim                                         */
  int32_t quantizer;     /* EDTTS_SEM_FSQ (CFG.use_fsq) or EDTTS_SEM_VQ               */
  int32_t codebook_size; /* VQ: rows of codebook.weight                              */
  int32_t n_levels;      /* FSQ: len(CFG.fsq_levels)                                 */
  int32_t levels[16];    /* FSQ: CFG.fsq_levels; basis = cumprod([1] + levels[:-1])  */
} EdttsSemDims;
/* Packed blob: weights in MFMA-fragment order, zero-padded to 16 x 16 tiles, plus the tables the kernels read (|c|^2 of each code,
 * FSQ half-levels, levels and basis).  slots (host array of device fp32 pointers, state-dict order):
 *   with a proj (in_dim > 0): proj.0.weight [S][in_dim], proj.0.bias, LayerNorm weight, LayerNorm bias, final Linear weight [S][S],
 *   its bias; then FSQ: proj_down.weight [D][S], proj_down.bias [D], proj_up.weight [S][D], proj_up.bias [S]; or VQ:
 *   codebook.weight [K][S].  edtts_sem_num_codes: the number of token ids (prod(levels) or codebook_size). */
int edtts_sem_packed_bytes(const EdttsSemDims* dims, size_t* out_bytes);
int edtts_sem_num_codes(const EdttsSemDims* dims, int64_t* out_codes);
int edtts_sem_pack(const EdttsSemDims* dims, const void* const* slots, int n_slots, void* packed, void* stream);
/* Encode: one kernel over h.  idx [B,T] int64 (required); z [B,T,S] (proj output), z_q [B,T,S] and counts int32 [num_codes]
 * (usage, zeroed by the call, integer atomics) are optional (NULL).  Per frame, in the reference's order: FSQ u = proj_down(z),
 * zb = tanh(u), q = clamp(rint((zb+1) half), 0, L-1) / half - 1, zq_low = zb + (q - zb), idx = sum rint((zq_low+1) half) basis,
 * z_q = proj_up(zq_low); VQ dist = (|z|^2 - 2 z.c) + |c|^2, idx = the first minimum (torch.argmin), z_q = z + (c - z).
 * lengths int64 [B] or NULL: frames t >= lengths[b] (clamped into [1, T]) are not read, get idx 0 and z_q / z 0 and are not
 * counted; row b is then bitwise the call on row b alone.  h, z, z_q must be 16-byte aligned. */
int edtts_sem_encode(const EdttsSemDims* dims, const void* packed, const float* h, int B, int T, const int64_t* lengths,
                     int64_t* idx, float* z, float* z_q, int32_t* counts, void* stream);
/* Decode: idx [n] -> z_q [n,S] (FSQEncoder.decode: indices_to_codes as the reference writes it -- the LAST level is the least
 * significant digit -- then proj_up; VectorQuantizer.decode: the codebook row, bitwise).  Ids outside [0, num_codes) are clamped
 * (the host raises IndexError for them when EDTTS_CHECK_INDICES=1). */
int edtts_sem_decode(const EdttsSemDims* dims, const void* packed, const int64_t* idx, int64_t n, float* z_q, void* stream);
/* Stats: counts int32 [n_codes] -> perplexity fp32 [1] = exp(-sum p log(max(p, 1e-12))), p = counts / max(sum, 1), and used int64
 * [1] = #(counts > 0) (fsq.py:189-193, vq.py:101-105).  One block, fixed order: bitwise reproducible. */
int edtts_sem_stats(const int32_t* counts, int64_t n_codes, float* perplexity, int64_t* used, void* stream);

/* ---- training the semantic head  (train_v2.py train_step: proj and FSQEncoder are trained with the decoder) ------------------------
 * These entries train the FSQ head (EDTTS_ERR_UNSUPPORTED for EDTTS_SEM_VQ: a VQ head trains through the edtts_sem_vq_* entries
 * below), fp32; bf16 / autocast training is not built.  The straight-through estimator is FSQ.forward's: zq_low = zb + (q - zb).detach(), so d zb = d zq_low.
 *
 * edtts_sem_encode_train is edtts_sem_encode (idx, z_q, counts as there) that also writes the backward's tape, M = B * T rows:
 *     in_dim > 0:  y1 = proj.0(h) before GELU [M][S] | z [M][S] | zb = tanh(proj_down(z)) [M][16]    (2 M S + 16 M floats)
 *     in_dim = 0:  zb [M][16]                                                                     (16 M floats; z is the input)
 * Everything else (LayerNorm statistics, the LayerNorm output, zq_low, 1 - zb^2) is recomputed by the backward.  Without dropout,
 * idx and z_q are bitwise edtts_sem_encode's.
 *
 * Dropout: one more site of the mask contract above ("Dropout masks"), the nn.Dropout between LayerNorm and the last Linear of the
 * five-module proj (in_dim > 0 only; a drop with p > 0 and in_dim = 0 is EDTTS_ERR_ARG).  Stream word c2 = 0x40000; row
 * m = b * T + t, column n: c0 = n >> 3, c1 = m, c3 = 0, field n & 7 -- as sites 2 and 3.  thr, p_eff, the kept values' factor and the
 * EDTTS_ERR_ARG rule for p are the contract's.  drop == NULL or p == 0: the undropped launches, bitwise.  The backward must be
 * given what its forward was given and regenerates the mask.  edtts_sem_dropout_mask: the keep mask [B * T, S] as 0 / 1 bytes
 * through the same device function.
 *
 * The backward needs three transposed matrices (proj_up^T, proj_down^T, final Linear^T) in fragment order: a second, training-only
 * blob (edtts_sem_train_packed_bytes / edtts_sem_train_pack, slots as edtts_sem_pack); the inference blob is unchanged.
 *
 * edtts_sem_backward: d_zq [B,T,S] -> the gradient of every non-NULL entry of grad_slots (state-dict slot order, as edtts_sem_pack:
 * 10 slots with a proj, 4 without) and, with in_dim = 0, d_z [B,T,S] (optional).  h is what the forward was given.  One frame-local
 * kernel (MFMA, the transposed weights as the A operand) and then sums over frames in fixed orders -- rows ascending inside a slab
 * of edtts_train_dw_slab_rows(M) rows, slabs ascending -- without float atomics: two backwards are bitwise equal.  d_h is never
 * computed.  It reads the tape, the two blobs, h, lengths and d_zq and writes only gradients and `scratch`
 * (edtts_sem_train_scratch_bytes), so forwards that run between a forward and its backward do not disturb it.
 * lengths: as edtts_sem_encode; frames at or past lengths[b] contribute exactly nothing and get d_z 0 (h itself must be finite there:
 * the weight-gradient products multiply those rows by zeros).  Argument errors are reported before any pointer is looked at. */
int edtts_sem_train_packed_bytes(const EdttsSemDims* dims, size_t* out_bytes);
int edtts_sem_train_pack(const EdttsSemDims* dims, const void* const* slots, int n_slots, void* packed_train, void* stream);
int edtts_sem_train_tape_bytes(const EdttsSemDims* dims, int B, int T, size_t* out_bytes);
int edtts_sem_train_scratch_bytes(const EdttsSemDims* dims, int B, int T, size_t* out_bytes);
int edtts_sem_encode_train(const EdttsSemDims* dims, const void* packed, const float* h, int B, int T, const int64_t* lengths,
                           int64_t* idx, float* z_q, int32_t* counts, void* tape, const EdttsDropout* drop, void* stream);
int edtts_sem_backward(const EdttsSemDims* dims, const void* packed, const void* packed_train, const void* tape, const float* h, int B,
                       int T, const int64_t* lengths, const float* d_zq, void* const* grad_slots, int n_slots, float* d_z,
                       void* scratch, const EdttsDropout* drop, void* stream);
int edtts_sem_dropout_mask(const EdttsSemDims* dims, int B, int T, const EdttsDropout* drop, uint8_t* keep, void* stream);
/* ... with the key in device memory ("dropout key in device memory" above): bitwise the calls above when *key == seed. */
int edtts_sem_encode_train_dev(const EdttsSemDims* dims, const void* packed, const float* h, int B, int T, const int64_t* lengths,
                               int64_t* idx, float* z_q, int32_t* counts, void* tape, const EdttsDropoutDev* drop, void* stream);
int edtts_sem_backward_dev(const EdttsSemDims* dims, const void* packed, const void* packed_train, const void* tape, const float* h, int B,
                           int T, const int64_t* lengths, const float* d_zq, void* const* grad_slots, int n_slots, float* d_z,
                           void* scratch, const EdttsDropoutDev* drop, void* stream);
int edtts_sem_dropout_mask_dev(const EdttsSemDims* dims, int B, int T, const EdttsDropoutDev* drop, uint8_t* keep, void* stream);

/* ---- training the VQ head  (train.py: VectorQuantizer.forward in training mode, models/vq.py:86-93, 109-145) ----------------------
 * EDTTS_SEM_VQ only (EDTTS_ERR_UNSUPPORTED for EDTTS_SEM_FSQ), fp32.  With flat = the N valid frames of z and C the codebook the
 * forward was given:  idx = first argmin((|z|^2 - 2 z.c) + |c|^2), c = C[idx], z_q = z + (c - z), r = c - z,
 *     L = mean(r^2) over the N S valid elements, vq_loss = L + commit L  (codebook loss + commit x commitment loss: equal values),
 *     d z = G - g commit 2 r / (N S)  (G = d z_q: the straight-through estimator; g = d vq_loss),
 *     d C[k] = g 2 / (N S) sum_{m: idx[m] = k} r_m  (the gradient of z_q never reaches the codebook).
 * N = sum of the lengths clamped into [1, T] (B T without lengths), computed on the device.
 *
 * edtts_sem_vq_encode_train is edtts_sem_encode (idx, z_q, counts as there; without dropout idx and z_q are bitwise its) that also
 * writes loss[1] = L + commit L (training == 0: 0; L = the fp64 sum of the per-frame sums in a fixed order / (N S), rounded once) and
 * the backward's tape, M = B * T rows:
 *     in_dim > 0:  y1 = proj.0(h) before GELU [M][S] | z [M][S] | r [M][S] | sq [M] = sum_s r^2      (3 M S + M floats)
 *     in_dim = 0:  r [M][S] | sq [M]                                                               (M S + M floats; z is the input)
 * The tape holds r and not c because the EMA update overwrites the codebook between the forward and its backward: the backward
 * reads nothing of the codebook.  Dropout: the site of edtts_sem_encode_train (stream word 0x40000).
 *
 * edtts_sem_vq_ema_update (the caller runs it after the forward when the module trains and decay > 0), n[k] = counts[k]:
 *     ema_cluster_size = ema_cluster_size decay + (1 - decay) n;  ema_w = ema_w decay + (1 - decay) sum_{m: idx[m] = k} z_m;
 *     codebook = ema_w / max(ema_cluster_size, epsilon)[:, None]            (1 - decay is formed in double and rounded once)
 * written in place.  z [B,T,S]: the tape's z with a proj, the forward's input without one.  The inference blob is NOT refreshed:
 * the caller packs again (edtts_sem_pack) before the next encode.  The per-code sums are a one-hot GEMM on MFMA over slabs of
 * edtts_train_dw_slab_rows(M) rows, slabs added in ascending order: no float atomics, bitwise reproducible.  update_count and the
 * dead-code reset are the caller's (edge_diffusion_tts_amd/encoder.py).
 *
 * edtts_sem_vq_backward: d_zq [B,T,S] (NULL: 0) and d_loss (device scalar; NULL: 0) -> the gradient of every non-NULL entry of
 * grad_slots (state-dict slot order as edtts_sem_pack: 7 slots with a proj, 1 without) and, with in_dim = 0, d_z [B,T,S] (optional).
 * h, idx, lengths, commit, drop: what the forward was given / returned.  The training blob (edtts_sem_vq_train_packed_bytes /
 * edtts_sem_vq_train_pack, slots as edtts_sem_pack) holds the final Linear's transpose in fragment order: 0 bytes with in_dim = 0
 * (packed and packed_train may then be NULL).  Rows of unused codes in the codebook gradient are exactly 0.  One scratch size
 * (edtts_sem_vq_scratch_bytes) serves the EMA update and the backward.  Frames at or past lengths[b] contribute nothing to the
 * loss, the counts, the code sums or any gradient.  M = 0: loss 0 and zero gradients.  Argument errors are reported before any
 * pointer is looked at. */
int edtts_sem_vq_train_packed_bytes(const EdttsSemDims* dims, size_t* out_bytes);
int edtts_sem_vq_train_pack(const EdttsSemDims* dims, const void* const* slots, int n_slots, void* packed_train, void* stream);
int edtts_sem_vq_tape_bytes(const EdttsSemDims* dims, int B, int T, size_t* out_bytes);
int edtts_sem_vq_scratch_bytes(const EdttsSemDims* dims, int B, int T, size_t* out_bytes);
int edtts_sem_vq_encode_train(const EdttsSemDims* dims, const void* packed, const float* h, int B, int T, const int64_t* lengths,
                              int64_t* idx, float* z_q, int32_t* counts, float* loss, void* tape, int training, double commit,
                              const EdttsDropout* drop, void* stream);
int edtts_sem_vq_ema_update(const EdttsSemDims* dims, const int64_t* idx, const float* z, int B, int T, const int64_t* lengths,
                            const int32_t* counts, double decay, double epsilon, float* ema_cluster_size, float* ema_w,
                            float* codebook, void* scratch, void* stream);
int edtts_sem_vq_backward(const EdttsSemDims* dims, const void* packed, const void* packed_train, const void* tape, const float* h,
                          const int64_t* idx, int B, int T, const int64_t* lengths, const float* d_zq, const float* d_loss,
                          double commit, void* const* grad_slots, int n_slots, float* d_z, void* scratch, const EdttsDropout* drop,
                          void* stream);
/* Offset and bytes of member `which` of the tape (EDTTS_SEM_TAPE_*: offsets into `tape`) or of the scratch (EDTTS_SEM_SCRATCH_*:
 * offsets into `scratch`) of a head of either quantizer for one (dims, B, T), answered by the code that lays both out.  In memory
 * order, M = B * T:
 *     FSQ tape:     y1 [M][S] | z [M][S] (both only with a proj) | zb [M][16]
 *     VQ tape:      y1 | z (both only with a proj) | r [M][S] | sq [M]
 *     FSQ scratch:  du | zql [M][16] | dz | gm [M][S] | with a proj a | dam | xh | dy1 [M][S] | stat [M][2] | part
 *     VQ scratch:   coef [4] | csum [K][S] | with a proj dz | a | dam | xh | dy1 [M][S] | stat [M][2] | part
 * Tape members follow each other directly; every scratch member starts on a multiple of 4 floats; `part` holds the partial sums of
 * the reductions.  A member the head does not have (the other quantizer's, or a proj's without a proj) is EDTTS_ERR_ARG by name, as
 * is `which` out of range.  No GPU call. */
enum {
  EDTTS_SEM_TAPE_Y1 = 0, EDTTS_SEM_TAPE_Z = 1, EDTTS_SEM_TAPE_ZB = 2, EDTTS_SEM_TAPE_R = 3, EDTTS_SEM_TAPE_SQ = 4,
  EDTTS_SEM_SCRATCH_DU = 5, EDTTS_SEM_SCRATCH_ZQL = 6, EDTTS_SEM_SCRATCH_DZ = 7, EDTTS_SEM_SCRATCH_GM = 8, EDTTS_SEM_SCRATCH_A = 9,
  EDTTS_SEM_SCRATCH_DAM = 10, EDTTS_SEM_SCRATCH_XH = 11, EDTTS_SEM_SCRATCH_DY1 = 12, EDTTS_SEM_SCRATCH_STAT = 13,
  EDTTS_SEM_SCRATCH_PART = 14, EDTTS_SEM_SCRATCH_COEF = 15, EDTTS_SEM_SCRATCH_CSUM = 16, EDTTS_SEM_REGION_COUNT = 17
};
int edtts_sem_train_region(const EdttsSemDims* dims, int B, int T, int which, size_t* offset_bytes, size_t* bytes);

/* ---- the optimiser step  (train_v2.py:299-309 and edge_diffusion_tts/train.py:160-170,245-249,279-281: clip_grad_norm_(params,
 * cfg.grad_clip) then AdamW.step(); training/consistency.py:45-50: ConsistencyTrainer.update_teacher, lerp_ over every parameter) ---
 * One pass over a list of fp32 tensors: clip by the global gradient norm, AdamW, optionally an EMA target,
 * a second copy of the new values ("mirror": the generic decoder's packed blob, so that the next forward packs nothing) and the
 * zeroing of the gradient.  Two or three launches and one small host-to-device copy per step; no host synchronisation, no
 * allocation of device memory, everything on `stream`.
 *
 * Arithmetic, per element, torch.optim.AdamW's single-tensor form in its order (host scalars are doubles, rounded to fp32 where
 * they meet a tensor):  g *= clip_coef;  p *= 1 - lr wd;  m = m + (1 - beta1)(g - m);  v = beta2 v + (1 - beta2) g g;
 *     p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),   bc1 = 1 - beta1^step, bc2 = 1 - beta2^step  (fp64, on the device);
 *     ema += (p_new - ema)(1 - ema_decay)   (lerp_);   mirror[i or its transposed place] = p_new;  ema_mirror likewise = ema_new.
 * g itself is only read (or zeroed with EDTTS_OPT_ZERO_GRADS): unlike clip_grad_norm_, the scaled gradient is not stored.
 * total_norm = sqrt(sum g^2) over every tensor of the call: fp32 sums of squares per chunk in a fixed order, the chunks added in
 * ascending order in fp64 -- no float atomics, a step is bitwise reproducible.  clip_coef = min(1, max_norm / (total_norm + 1e-6)),
 * a NaN staying a NaN as in torch.
 *
 * One device-resident step counter serves every tensor of a scratch (EdttsOptimState.step, incremented by each step before its
 * bias corrections are formed); the host never reads it on the way.  With EDTTS_OPT_SKIP_NONFINITE a step whose total_norm is not
 * finite stores nothing at all -- p, m, v, ema, the mirrors and g keep their bits, step stays -- and adds one to `skipped`.
 *
 * scratch: edtts_optim_scratch_bytes bytes for the largest number of chunks and groups a step will bring; the caller zero-fills
 * it once (step = skipped = 0) and keeps it for the optimiser's life.  It begins with an EdttsOptimState that the caller may read
 * (after ordering itself behind the stream).  A chunk is at most edtts_optim_chunk_size elements of one tensor; chunk starts are
 * multiples of that size, hence of 4.  edtts_optim_chunk_table is the step's own cutting of a list of numels, as a host query: it
 * writes the first `cap` chunks (tensor index, first element, count) and the total number of chunks (cap = 0: the count alone).
 *
 * A step may be issued while earlier ones have not run: the table of pointers travels through a pinned ring of 8 slots, ordered
 * by events (only with more than 8 steps outstanding does the host wait for the oldest copy).  Steps that share a scratch must
 * be issued on one stream, or ordered by the caller.  Tensors with numel 0 are skipped; a call without any element returns at
 * once and changes nothing.  Pointers must be 4-byte aligned; a tensor whose pointers are all 16-byte aligned takes 16-byte
 * loads and stores.  edtts_optim_step is not graph-capturable (lr is a host argument and the table is copied from the host); the
 * resident pair below is.
 *
 * Resident step.  edtts_optim_upload validates tensors / groups exactly as edtts_optim_step does and copies the same table into the
 * scratch (not capturable: EDTTS_ERR_ARG while `stream` is capturing); it returns the number of chunks, which the resident step
 * needs besides the scratch, and the byte offset of the EdttsOptimGroup array inside the scratch (where a caller may read the
 * learning rates in force).  edtts_optim_step_resident then launches the step's kernels on the table that lies in the scratch: no
 * copy, no event, no host allocation -- capturable, and bitwise edtts_optim_step on the same table.  The learning rate: with lr_dev
 * (device fp64 [n_groups]) group g takes lr_dev[g]; otherwise with sched (kind != EDTTS_SCHED_NONE) every group takes the schedule's
 * value; both may be NULL and then the uploaded lr holds.  The value is stored into the scratch's groups before the step sizes are
 * formed from it, on a skipped step too.  EDTTS_SCHED_COSINE is train_v2.cosine_lr_schedule in fp64, evaluated at
 * n = state.step + state.skipped as they stand before this step's increment (a skipped step still advances the schedule, as the
 * reference's global_step does):  n < warmup_steps: base_lr * n / max(warmup_steps, 1);  otherwise
 * min_lr + 0.5 * (base_lr - min_lr) * (1 + cos(pi * (n - warmup_steps) / max(total_steps - warmup_steps, 1))), past total_steps too.
 * EDTTS_OPT_EMA_ONLY has no resident form. */
typedef struct EdttsOptimState {
  int64_t step;      /* steps taken (skipped ones not counted)                               */
  int64_t skipped;   /* steps skipped by EDTTS_OPT_SKIP_NONFINITE                            */
  float total_norm;  /* of the last step that computed one                                   */
  float clip_coef;   /* of the last step (1 without EDTTS_OPT_CLIP)                          */
  int32_t skip;      /* 1 when the last step was skipped                                     */
  int32_t reserved;
} EdttsOptimState;
typedef struct EdttsOptimGroup {
  double lr, beta1, beta2, eps, weight_decay;
} EdttsOptimGroup;
typedef struct EdttsOptimTensor {
  float* p;           /* parameter [numel]                                                                            */
  float* g;           /* gradient                                                                                     */
  float* m;           /* exp_avg                                                                                      */
  float* v;           /* exp_avg_sq                                                                                   */
  float* ema;         /* EMA target [numel] or NULL                                                                   */
  float* mirror;      /* second destination of the new p or NULL (blob + offset in floats)                            */
  float* ema_mirror;  /* second destination of the new ema or NULL (needs ema)                                        */
  int64_t numel;
  int32_t group;      /* index into groups                                                                            */
  int32_t rows, cols; /* rows > 0: p is [rows][cols] and both mirrors hold the transpose [cols][rows]; 0, 0: plain    */
  float ema_decay;    /* in [0, 1]                                                                                    */
} EdttsOptimTensor;
enum {
  EDTTS_OPT_CLIP = 1,           /* max_norm is given (otherwise no clipping; total_norm is then only computed for SKIP_NONFINITE) */
  EDTTS_OPT_SKIP_NONFINITE = 2,
  EDTTS_OPT_ZERO_GRADS = 4,     /* g = 0 behind the update */
  EDTTS_OPT_EMA_ONLY = 8        /* no optimiser arithmetic: ema (required) and ema_mirror from p as it stands; g, m, v unused; excludes
                                   the other flags and leaves the state alone */
};
int edtts_optim_chunk_size(void);
int edtts_optim_chunk_table(const int64_t* numels, int n_tensors, int cap, int32_t* tensor, int64_t* offset, int32_t* count, int* n_chunks);
int edtts_optim_scratch_bytes(int n_chunks, int n_groups, size_t* out_bytes);
int edtts_optim_step(const EdttsOptimTensor* tensors, int n_tensors, const EdttsOptimGroup* groups, int n_groups, double max_norm, int flags,
                     void* scratch, size_t scratch_bytes, void* stream);
enum {
  EDTTS_SCHED_NONE = 0,
  EDTTS_SCHED_COSINE = 1
};
struct EdttsOptimSchedule {
  int32_t kind;         /* EDTTS_SCHED_* */
  int32_t reserved;
  double base_lr, min_lr;
  int64_t warmup_steps, total_steps;
};
typedef struct EdttsOptimSchedule EdttsOptimSchedule;
int edtts_optim_upload(const EdttsOptimTensor* tensors, int n_tensors, const EdttsOptimGroup* groups, int n_groups, int flags, void* scratch,
                       size_t scratch_bytes, int* n_chunks, size_t* groups_offset, void* stream);
int edtts_optim_step_resident(int n_chunks, int n_groups, double max_norm, int flags, void* scratch, size_t scratch_bytes, const double* lr_dev,
                              const EdttsOptimSchedule* sched, void* stream);
/* Where edtts_pack_weights puts weight slot `slot` of a generic fp32 layout (dims.compute_dtype = EDTTS_F32 | EDTTS_KERNELS_GENERIC;
 * anything else is EDTTS_ERR_UNSUPPORTED): its offset in floats, the slot's [rows][cols] (a vector: 1 x n) and whether the blob
 * holds its transpose [cols][rows] (time_emb.1 / .3 and the two AdaLN projections of a layer).  Layout arithmetic from the same
 * table the packing reads; no GPU call. */
int edtts_generic_slot_dest(const EdttsDims* dims, int slot, size_t* offset_floats, int* rows, int* cols, int* transposed);

/* ---- HuBERT backbone (transformers HubertModel, feat_extract_norm = "group", do_stable_layer_norm = False: hubert-base) ------------
 * wav [B, T_audio] fp32 -> HubertModel(wav, output_hidden_states=True).hidden_states[num_layers] [B, T_feat, hidden], eval mode, fp32.
 * Only the layers up to num_layers are packed and run; num_layers = 0 is the output of the encoder's LayerNorm.  GELU is the erf form
 * throughout.  The caller (edge_diffusion_tts_amd/hubert.py) checks the layout fields that are not numbers (feat_extract_norm,
 * do_stable_layer_norm, conv_bias, the activations, feat_proj_layer_norm, conv_pos_batch_norm).
 * Limits (EDTTS_ERR_UNSUPPORTED outside): 1..16 conv layers, conv_dim[i] % 4 == 0, conv_kernel[0] <= 64; hidden % heads == 0,
 * head_dim <= 128, hidden and intermediate % 4 == 0, (hidden / pos_groups) % 4 == 0; num_layers in [0, 256]. */
typedef struct EdttsHubertDims {
  int32_t n_conv;           /* len(config.conv_dim)                      */
  int32_t conv_dim[16];     /* config.conv_dim                           */
  int32_t conv_kernel[16];  /* config.conv_kernel                        */
  int32_t conv_stride[16];  /* config.conv_stride                        */
  int32_t hidden;           /* config.hidden_size                        */
  int32_t heads;            /* config.num_attention_heads                */
  int32_t intermediate;     /* config.intermediate_size                  */
  int32_t num_layers;       /* encoder layers to run: hidden_states[num_layers] */
  int32_t pos_kernel;       /* config.num_conv_pos_embeddings            */
  int32_t pos_groups;       /* config.num_conv_pos_embedding_groups      */
  float layer_norm_eps;     /* config.layer_norm_eps (the GroupNorm keeps nn.GroupNorm's 1e-5) */
} EdttsHubertDims;
/* Output frames of n_samples (HubertModel._get_feat_extract_output_lengths: per conv floor((n - k) / s) + 1), 0 if none. */
int edtts_hubert_frames(const EdttsHubertDims* dims, int64_t n_samples, int64_t* out_frames);
/* Packed blob: conv weights as [co][k][ci] (implicit-GEMM order; conv0 as [k0][C0]), q | k | v as one [3H][H] matrix, everything else as stored.
 * slots (host array of device fp32 pointers; state-dict tensors, modeling_hubert.py names):
 *   feature_extractor.conv_layers.0.conv.weight [C0][1][k0], .0.layer_norm.weight, .0.layer_norm.bias (the GroupNorm),
 *   feature_extractor.conv_layers.i.conv.weight [Ci][Ci-1][ki] for i = 1 .. n_conv - 1,
 *   feature_projection.layer_norm.weight, .bias, feature_projection.projection.weight [H][C_last], .bias,
 *   encoder.pos_conv_embed.conv weight [H][H / groups][pos_kernel] WITH THE WEIGHT NORM FOLDED IN (w[:, :, k] = g[k] v[:, :, k] /
 *   |v[:, :, k]|, torch._weight_norm(v, g, 2)), its bias, encoder.layer_norm.weight, .bias,
 *   then per layer l < num_layers (encoder.layers.l.): attention.q_proj.weight, .bias, k_proj.weight, .bias, v_proj.weight, .bias,
 *   out_proj.weight, .bias, layer_norm.weight, .bias, feed_forward.intermediate_dense.weight, .bias, output_dense.weight, .bias,
 *   final_layer_norm.weight, .bias.   3 + (n_conv - 1) + 8 + 16 num_layers slots. */
int edtts_hubert_packed_bytes(const EdttsHubertDims* dims, size_t* out_bytes);
int edtts_hubert_pack(const EdttsHubertDims* dims, const void* const* slots, int n_slots, void* packed, void* stream);
/* Workspace for one (B, T_audio): conv0's output [B][T0][C0] (stored, not recomputed inside conv1: 1.0 GiB at B = 16 x 10 s), the
 * conv ping-pong buffers and the encoder's [B T_feat] x (hidden | hidden | max(3 hidden, intermediate)) rows.  EDTTS_ERR_ARG when
 * T_audio gives no output frame. */
int edtts_hubert_workspace_bytes(const EdttsHubertDims* dims, int B, int T_audio, size_t* out_bytes);
/* Forward (replaces modeling_hubert.py HubertModel.forward: HubertFeatureEncoder, HubertFeatureProjection, HubertEncoder up to layer
 * num_layers; HubertPositionalConvEmbedding + HubertSamePadLayer as one zero-padded conv of T_feat outputs).  out [B, T_feat, hidden].
 * lengths int64 [B] (samples) or NULL.  With lengths, row b is bitwise the call on wav[b, :lengths[b]] alone: GroupNorm statistics
 * over its own conv0 frames, the positional conv zero-padded at its own end, attention over its own frames(lengths[b]) keys, output
 * rows past that count 0, samples past lengths[b] never read.  Values are clamped into [the shortest input with one frame, T_audio].
 * Without lengths every utterance has T_audio samples (the padded batch of the reference); each row still depends on its row only.
 * out, packed and workspace 16-byte aligned.  No allocation, no host synchronisation: graph-capturable. */
int edtts_hubert_forward(const EdttsHubertDims* dims, const void* packed, const float* wav, int B, int T_audio, const int64_t* lengths,
                         float* out, void* workspace, void* stream);
/* The backbone with a compute dtype (csrc/edtts_hubert16.h).  compute_dtype EDTTS_HUBERT_FP32: exactly the four calls above (same
 * kernels, same blob, same workspace).  EDTTS_HUBERT_BF16: the two operands of every contraction after conv0 -- conv1 .. conv_last, the
 * feature projection, the positional conv (its weight norm folded in fp32 by the caller, as above), QKV, Q K^T, P V, out_proj, the FFN
 * -- are rounded to bf16 (nearest even) and multiplied on v_mfma_f32_16x16x32_bf16 with fp32 accumulators; conv0, the GroupNorm
 * statistics, the residual stream, biases, GELU, every LayerNorm, the softmax and the output stay fp32.  slots, out, lengths and the
 * bitwise invariances are those of the fp32 calls; the blob holds the matrices as bf16 (conv weights [co][k][ci], q | k | v as one
 * [3H][H]) and conv0 / GroupNorm / biases / norm parameters as fp32, and blob and workspace belong to the dtype they were sized for.
 * Limits of the bf16 path beyond the fp32 ones (EDTTS_ERR_UNSUPPORTED, the message names the field): conv_dim[i], hidden,
 * intermediate and hidden / pos_groups multiples of 8 (a 16-byte operand chunk never straddles a conv tap), head_dim a multiple of 32.
 * Any other compute_dtype: EDTTS_ERR_ARG. */
#define EDTTS_HUBERT_FP32 0
#define EDTTS_HUBERT_BF16 1
int edtts_hubert_packed_bytes_dt(const EdttsHubertDims* dims, int compute_dtype, size_t* out_bytes);
int edtts_hubert_pack_dt(const EdttsHubertDims* dims, int compute_dtype, const void* const* slots, int n_slots, void* packed, void* stream);
int edtts_hubert_workspace_bytes_dt(const EdttsHubertDims* dims, int compute_dtype, int B, int T_audio, size_t* out_bytes);
int edtts_hubert_forward_dt(const EdttsHubertDims* dims, int compute_dtype, const void* packed, const float* wav, int B, int T_audio,
                            const int64_t* lengths, float* out, void* workspace, void* stream);
/* The backbone's launch list, site by site (a diagnostic: tests/hubert_audit_util.py audits every site against fp64).
 * edtts_hubert_forward_until takes the arguments of edtts_hubert_forward_dt plus (stop_site, stop_index, tile) before `stream`.  It
 * makes the launches of edtts_hubert_forward_dt -- same kernels, same arguments, same order -- and returns after the last launch of
 * site `stop_site`; stop_index is the conv layer (1 .. n_conv - 1) for EDTTS_HUB_CONV, the encoder layer for EDTTS_HUB_QKV ..
 * EDTTS_HUB_LN2 and 0 otherwise.  A site the call does not have is EDTTS_ERR_ARG with a message that names it: EDTTS_HUB_VT under
 * fp32, EDTTS_HUB_LENS / _ZERO without lengths, an index out of range.  tile 0 keeps the GEMM launchers' own choice of tile (128 x
 * 128 when that leaves at least two tiles per compute unit and N > 64, else 64 x 64); 2 or 4 forces the 64- or the 128-wide tile for
 * every GEMM launch of the call (results are bitwise independent of the tile); any other value is EDTTS_ERR_ARG.  The plain entry
 * points are "no stop, tile 0".  Graph capture of a stopped call is not supported.
 * Where each site's output lies (members as edtts_hubert_workspace_region names them; T_i: frames after conv stage i of T_audio
 * samples, T = T_feat, H = hidden; "16": bf16 under EDTTS_HUBERT_BF16, fp32 otherwise):
 *   LENS     lens     int64 [2][B]: conv0 frames | output frames per utterance
 *   GNSTAT   stats    fp32 [B][2][C0]: scale = gamma rstd | shift = beta - mean scale (part: fp64 [B][chunks][C0][2], chunks = ceil(T_0 / 256))
 *   CONV0    buf0     [B][T_0][C0], 16 when n_conv > 1; rows past an utterance's conv0 frames are 0
 *   CONV i   buf(i&1) [B][T_i][C_i], 16 for i < n_conv - 1, fp32 for the last stage (a LayerNorm reads it)
 *   FPNORM   buf(n_conv&1) fp32 [B][T][C_last] (the buffer the last conv did not write)
 *   FPROJ    h        fp32 [B][T][H]
 *   POS      att      fp32 [B][T][H]: h + GELU(pos_conv(h) + bias)
 *   ENCNORM  h        fp32 [B][T][H]; `out` when num_layers = 0
 *   QKV      big      [B T][3H] 16: q | k | v rows
 *   VT       vt       bf16 [B][heads][head_dim][Tp], Tp = T rounded up to 32: V^T in the key-slot order of csrc/edtts_hubert16.h inside
 *                     every 32-key chunk, zeros past an utterance's count; chunks wholly past it are not written
 *   ATTN     att      [B][T][H] 16; 64-query blocks wholly past an utterance's count are not written
 *   OPROJ    h        fp32, in place (the residual)          LN1  h  fp32, in place
 *   FF1      big      [B T][intermediate] 16                  FF2  h  fp32, in place (the residual)
 *   LN2      h        fp32, in place; `out` for the last layer
 *   ZERO     out      rows past an utterance's count set to 0
 * Rows past an utterance's frame count hold whatever the row-local steps made of the padding; nothing live reads them. */
enum {
  EDTTS_HUB_LENS = 0,     /* (lengths only) k_hub_lens */
  EDTTS_HUB_GNSTAT = 1,   /* k_hub_gn_part + k_hub_gn_final */
  EDTTS_HUB_CONV0 = 2,    /* k_hub_conv0 / k_hub_conv0_16 */
  EDTTS_HUB_CONV = 3,     /* conv stage stop_index = 1 .. n_conv - 1 */
  EDTTS_HUB_FPNORM = 4,   /* the feature projection's LayerNorm */
  EDTTS_HUB_FPROJ = 5,    /* the feature projection */
  EDTTS_HUB_POS = 6,      /* the positional conv, GELU and residual */
  EDTTS_HUB_ENCNORM = 7,  /* the encoder's LayerNorm */
  EDTTS_HUB_QKV = 8,      /* per layer from here to EDTTS_HUB_LN2 */
  EDTTS_HUB_VT = 9,       /* (bf16 only) k_hub_vt */
  EDTTS_HUB_ATTN = 10,
  EDTTS_HUB_OPROJ = 11,
  EDTTS_HUB_LN1 = 12,
  EDTTS_HUB_FF1 = 13,
  EDTTS_HUB_FF2 = 14,
  EDTTS_HUB_LN2 = 15,
  EDTTS_HUB_ZERO = 16,    /* (lengths only) k_hub_zero_past */
  EDTTS_HUB_COUNT = 17
};
int edtts_hubert_forward_until(const EdttsHubertDims* dims, int compute_dtype, const void* packed, const float* wav, int B, int T_audio,
                               const int64_t* lengths, float* out, void* workspace, int stop_site, int stop_index, int tile, void* stream);
/* Offset and extent (up to the next member: the member's bytes rounded up to 256) of workspace member `which` for one (dims,
 * compute_dtype, B, T_audio), answered by the code that lays the workspace out.  EDTTS_HUB_WS_VT exists under EDTTS_HUBERT_BF16 only
 * (EDTTS_ERR_ARG otherwise).  No GPU call. */
enum {
  EDTTS_HUB_WS_LENS = 0,
  EDTTS_HUB_WS_STATS = 1,
  EDTTS_HUB_WS_PART = 2,
  EDTTS_HUB_WS_BUF0 = 3,
  EDTTS_HUB_WS_BUF1 = 4,
  EDTTS_HUB_WS_H = 5,
  EDTTS_HUB_WS_ATT = 6,
  EDTTS_HUB_WS_BIG = 7,
  EDTTS_HUB_WS_VT = 8,
  EDTTS_HUB_WS_COUNT = 9
};
int edtts_hubert_workspace_region(const EdttsHubertDims* dims, int compute_dtype, int B, int T_audio, int which, size_t* offset_bytes,
                                  size_t* bytes);

/* ---- audio front end (the torchaudio ops the reference calls at every entry point: generate_sample.py:75-116,
 * data/collate.py:34-60, inference_pipeline.py:206-207, 354-355) -------------------------------------------------------------------
 * edtts_melspec: torchaudio.transforms.MelSpectrogram(n_fft = win_length = 1024, hop, center=True, pad_mode="reflect", periodic Hann
 * window, onesided, norm=None, mel_scale="htk", power 2 or 1) of wav [B, L] -> mode EDTTS_MEL_POWER: the mel [B, n_mels, T] (torch
 * layout); EDTTS_MEL_LOG: log(max(mel, 1e-5)) [B, T, n_mels] (frame-major, what collate.py:58-60 and normalize_mel consume).
 * T = L // hop + 1.  window [1024]; twiddle [512][2] = exp(-2 pi i q / 1024) (the Griffin-Lim table); fb_desc int32 [n_mels][3] =
 * (first bin, bin count, offset into fb_weights) of each filter's non-zero range of melscale_fbanks(513, ...), fb_weights its values.
 * lengths int64 [B] (samples) or NULL; values are clamped into [n_fft / 2 + 1, L]; row b is bitwise the call on wav[b, :lengths[b]]
 * alone (reflect padding at its own end, frames past lengths[b] // hop + 1 written as 0, samples past lengths[b] never read).
 * edtts_mel_segment_stats: per segment i = segments[i] = (row, start, end) (int64 [n_seg][3]) the mean and unbiased std (clamped at
 * 1e-5, NaN for a one-frame segment as torch.std) over the frames of the log-mel of wav[row, start : min(end, len_row)] ALONE (its own
 * reflect padding, (e - s) // hop + 1 frames) -> mean / stdv [n_seg, n_mels] (normalize_mel, utils/audio.py:10-14; the per-chunk
 * statistics of inference_pipeline.py:349-355).  Nothing else is written.  A segment of fewer than n_fft / 2 + 1 samples gives NaN.
 * edtts_logmel_stats: the same statistics of segment (b, 0, len_b) of every row, read from the log-mel [B, T, n_mels] that
 * edtts_melspec(EDTTS_MEL_LOG) wrote for the same wav, L, lengths and hop: bitwise what edtts_mel_segment_stats gives for that segment.
 * edtts_resample: torchaudio.functional.resample(resampling_method="sinc_interp_hann") with orig / new already divided by their gcd:
 * y[b][m new + p] = sum_j table[p][j] xpad[m orig + j], xpad = width zeros, x[b, :len_b], zeros; taps = 2 width + orig.  table is
 * laid out [ceil(taps / 4)][round_up(new, 16)][4] (element (p, j) at ((j / 4) Np + p) 4 + j % 4), zero outside p < new, j < taps.
 * y [B, L_out], L_out = ceil(new L / orig); lengths int64 [B] or NULL, clamped into [1, L]: row b's outputs past ceil(new len_b /
 * orig) are 0 and it is bitwise the call on x[b, :len_b] alone.  Limit: 32 orig + taps <= 16384 (EDTTS_ERR_UNSUPPORTED).
 * All four: no allocation, no host synchronisation (graph-capturable); every output one fixed-order chain, independent of B.
 * Compiled for n_fft = 1024, n_mels <= 128.  PARITY UNPINNED: torchaudio is not available offline; the tests restate its algorithm. */
enum { EDTTS_MEL_POWER = 0, EDTTS_MEL_LOG = 1 };
int edtts_melspec(const float* wav, int B, int L, const int64_t* lengths, int n_fft, int hop, const float* window, const float* twiddle,
                  const int32_t* fb_desc, const float* fb_weights, int n_mels, int power, int mode, float* out, void* stream);
int edtts_mel_segment_stats(const float* wav, int B, int L, const int64_t* lengths, const int64_t* segments, int n_seg, int n_fft, int hop,
                            const float* window, const float* twiddle, const int32_t* fb_desc, const float* fb_weights, int n_mels,
                            float* mean, float* stdv, void* stream);
int edtts_logmel_stats(const float* logmel, int B, int T, int n_mels, int L, const int64_t* lengths, int hop, float* mean, float* stdv,
                       void* stream);
int edtts_resample(const float* x, int B, int L, const int64_t* lengths, int orig, int new_freq, int width, int taps, const float* table,
                   int64_t L_out, float* y, void* stream);

/* ---- training objective  (train_v2.py:107-163, edge_diffusion_tts/train.py:143-158, training/consistency.py:60-122) ------------------
 * What stands between the decoder's prediction and the optimiser: normalize_mel, q_sample, the target, F.mse_loss with its gradient,
 * and the logging metrics, for a batch mel [B, T, n_mels] (raw log-mel with mean / stdv [B, n_mels]; already normalised with both NULL).
 *   mel_n  = (mel - mean) / stdv                         x_t    = sqrt_ab[t] mel_n + sqrt_1mab[t] noise
 *   target = sqrt_ab[t] noise - sqrt_1mab[t] mel_n  (EDTTS_OBJ_V)   or   noise  (EDTTS_OBJ_EPS)
 * every operation rounded on its own, in the reference's order.  tables: fp32 [4][n_table] = sqrt_alpha_bar | sqrt_one_minus_alpha_bar |
 * sqrt_recip_alpha_bar | sqrt_recip_alpha_bar_minus_one; t int64 [B], clamped into the table.
 * noise: a tensor [B, T, n_mels], or NULL: then element e of row b is lane e & 3 of draw e >> 2 of the Philox stream (seeds[b], 0x54),
 * bitwise edtts_randn_rows(B, T n_mels, seeds, 0x54, 1).  It is generated in registers, and edtts_objective_loss generates it again
 * instead of reading it back.  lengths int64 [B] or NULL, clamped into [1, T]: the live frames of each row.
 * edtts_objective_stats: normalize_mel's mean and unbiased std (clamped at 1e-5; NaN for a one-frame row, as torch.std) of every
 *   (row, mel bin) over the row's live frames, accumulated in fp64 in a fixed order -> mean / stdv [B, n_mels].
 * edtts_objective_prepare: x_t [B, T, n_mels], and mel_n / noise_out / target (same shape) where the pointer is not NULL.
 * edtts_objective_loss: pred [B, T_pred, n_mels]; the means run over the first Tm = min(T, T_pred[, T_pred2]) frames (the reference's
 *   "align sequence lengths"), with lengths over the sum_b min(len_b, Tm) n_mels live elements.  With x0(p, t) = sqrt_ab[t] x_t -
 *   sqrt_1mab[t] p (predict_x0_from_v; for EDTTS_OBJ_EPS predict_x0_from_eps):
 *     EDTTS_OBJ_V / EDTTS_OBJ_EPS   mse(pred, target)
 *     EDTTS_OBJ_DISTILL             mse(x0(pred, t), x0(pred2, t)), pred2 the teacher's prediction (no gradient)
 *     EDTTS_OBJ_CONSISTENCY         mse(x0_1, x0_2) + 0.5 (mse(x0_1, mel_n) + mse(x0_2, mel_n)), x0_1 = x0(pred, t), x0_2 = x0(pred2, t2)
 *                                   on x_t2 = q_sample(mel_n, t2, the same noise); x0_2 is detached in the first term
 *   unit [B, T_pred, n_mels] (and unit2 [B, T_pred2, n_mels], EDTTS_OBJ_CONSISTENCY only): d loss / d pred (d pred2) for an upstream
 *   gradient of 1; NULL: not written.  out: fp32 [8] = loss | the three terms as means (unused ones 0) | x0_mse = mse(x0_1, mel_n) |
 *   x0_cos = mean over rows of F.cosine_similarity of the flattened live elements (eps 1e-8) | 0 | 0.
 *   scratch: edtts_objective_scratch_bytes(B, max(T_pred, T_pred2), n_mels) bytes, 8-byte aligned, any contents.
 * edtts_objective_scale: d_pred[i] = unit[i] * grad_out[0] for i < n; grad_out is read on the device.
 * Contract of all calls: no allocation, no host synchronisation (graph-capturable).  Nothing past a row's length is ever loaded: NaN in
 * the padding of mel, noise, pred or pred2 or in the scratch changes no bit.  x_t, mel_n, noise_out, target, unit and unit2 are exactly
 * 0 past the lengths.  A row is bitwise the same alone or in any batch; every sum has one fixed order (per thread in quad order, lanes
 * by butterfly, waves in wave order, then in fp64 a row's chunks in ascending order and the rows in ascending order).  The float4 path
 * (all pointers 16-byte aligned, T n_mels and T_pred n_mels multiples of 4) and the per-element path give the same bits. */
enum { EDTTS_OBJ_V = 0, EDTTS_OBJ_EPS = 1, EDTTS_OBJ_DISTILL = 2, EDTTS_OBJ_CONSISTENCY = 3 };
int edtts_objective_scratch_bytes(int B, int T, int n_mels, size_t* out_bytes);
int edtts_objective_stats(const float* mel, int B, int T, int n_mels, const int64_t* lengths, float* mean, float* stdv, void* stream);
int edtts_objective_prepare(const float* mel, int B, int T, int n_mels, const int64_t* lengths, const int64_t* t, const float* tables,
                            int n_table, const float* mean, const float* stdv, const uint64_t* seeds, const float* noise, int kind,
                            float* x_t, float* mel_n, float* noise_out, float* target, void* stream);
int edtts_objective_loss(int kind, const float* mel, int B, int T, int n_mels, const int64_t* lengths, const int64_t* t,
                         const float* tables, int n_table, const float* mean, const float* stdv, const uint64_t* seeds,
                         const float* noise, const float* pred, int T_pred, const float* pred2, int T_pred2, const int64_t* t2,
                         float* unit, float* unit2, void* scratch, size_t scratch_bytes, float* out, void* stream);
int edtts_objective_scale(const float* unit, const float* grad_out, size_t n, float* d_pred, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EDTTS_H_ */
