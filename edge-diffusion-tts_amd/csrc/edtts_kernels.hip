// edtts_kernels.hip -- the one translation unit of libedtts_hip.so: gfx950 kernels + the C ABI of include/edtts.h.
//
// In this file, in order: error plumbing and the launch profiler; weight slots, the packed blob's layouts; the packing kernels; the
// decoder forward of the compiled shapes (k_cond_*, KArgs, tails, k_prologue, k_layer, + edtts_coop.h, edtts_bf16.h, k_ctx / k_ctx16);
// k_dsconv_*; the host side (workspace, settings, sub-batches, StepTail, CallCtx, Launcher / Launcher16); edtts_generic.h; the chain
// of compiled shapes (EDTTS_DISPATCH), launch_cond, the length and shape checks; the units that hold a whole subsystem each (the
// include list behind check_shapes); and the extern "C" block with the entry points of everything that is defined in this file.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "../../include/edtts.h"
#include "edtts_device.h"

using namespace edtts;

// =========================================================================================================
// error plumbing
// =========================================================================================================
static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
#define HIP_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return fail(EDTTS_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));    \
  } while (0)
#define LAUNCH_CHECK(name)                                                                              \
  do {                                                                                                  \
    hipError_t e_ = hipGetLastError();                                                                  \
    if (e_ != hipSuccess) return fail(EDTTS_ERR_HIP, "launch of %s failed: %s", name, hipGetErrorString(e_)); \
  } while (0)

// =========================================================================================================
// optional per-launch timing of the dominant kernel (bench.py roofline leg)
// =========================================================================================================
// A diagnostic that any thread may have switched on: `on` is read without the lock on every launch, the records themselves are
// taken under it (profiling serialises the launches it brackets; it is off by default)
struct Profiler {
  std::mutex mu;
  std::atomic<bool> on{false};
  std::vector<hipEvent_t> start, stop;
  int used = 0;
};
static Profiler g_prof;
#define PROF_LAUNCH(stream, launch_stmt)                                                       \
  do {                                                                                         \
    if (g_prof.on.load(std::memory_order_relaxed)) {                                           \
      std::lock_guard<std::mutex> prof_lock_(g_prof.mu);                                       \
      const bool rec_ = g_prof.used < (int)g_prof.start.size();                                \
      if (rec_) (void)hipEventRecord(g_prof.start[g_prof.used], (stream));                     \
      launch_stmt;                                                                             \
      if (rec_) (void)hipEventRecord(g_prof.stop[g_prof.used++], (stream));                    \
    } else {                                                                                   \
      launch_stmt;                                                                             \
    }                                                                                          \
  } while (0)

// =========================================================================================================
// weight slots
// =========================================================================================================
enum GlobalSlot {
  G_TOK, G_SEMP_W, G_SEMP_B, G_T1_W, G_T1_B, G_T3_W, G_T3_B, G_STEP, G_INP_W, G_INP_B, G_PE, G_CPE, G_FN_W, G_FN_B,
  G_OUT_W, G_OUT_B, G_FREQS, G_COUNT
};
static const char* const kGlobalNames[G_COUNT] = {
    "token_emb.weight", "sem_proj.weight", "sem_proj.bias", "time_emb.1.weight", "time_emb.1.bias",
    "time_emb.3.weight", "time_emb.3.bias", "step_emb.weight", "in_proj.weight", "in_proj.bias", "pos_emb.pe",
    "context_pos_emb.pe", "final_norm.weight", "final_norm.bias", "out_proj.weight", "out_proj.bias", "time_freqs"};
enum LayerSlot {
  L_N1_W, L_N1P_W, L_N1P_B, L_QKV_W, L_PROJ_W, L_PROJ_B, L_N2_W, L_QP_W, L_KVD_W, L_KVN_W, L_KVU_W, L_OP_W, L_N3_W,
  L_N3P_W, L_N3P_B, L_UP_W, L_UP_B, L_DOWN_W, L_DOWN_B, L_COUNT
};
static const char* const kLayerNames[L_COUNT] = {
    "norm1.norm.weight", "norm1.proj.weight", "norm1.proj.bias", "attn.qkv.weight", "attn.proj.weight",
    "attn.proj.bias", "norm2.weight", "cross_attn.q_proj.weight", "cross_attn.kv_down_proj.weight",
    "cross_attn.kv_norm.weight", "cross_attn.kv_up_proj.weight", "cross_attn.out_proj.weight", "norm3.norm.weight",
    "norm3.proj.weight", "norm3.proj.bias", "ffn.net.0.weight", "ffn.net.0.bias", "ffn.net.3.weight",
    "ffn.net.3.bias"};

// =========================================================================================================
// packed blob layout (offsets in floats)
// =========================================================================================================
constexpr int kMaxLayers = 32;
struct LayerLayout {
  size_t n1w, ada1T, ada1b, proj_b, n2w, n3w, ada3T, ada3b, up_b, down_b, kvd, kvn, kvu;
  size_t s_qkv;   // stream: QKV of this layer            [3HT n-tiles][HT]
  size_t s_body;  // stream: proj | q_proj | out_proj | ffn   (followed in memory by s_qkv of layer+1 / s_outp)
  size_t s_ffn;   // where the ffn part of s_body starts (entry point of the split FFN kernel)
  size_t g_proj, g_qp, g_op, g_up, g_down;  // generic layout: the state-dict's [N][K] matrices (qkv at s_qkv)
};
struct Layout {
  int GEN;   // 1: the generic run-time-shape kernels (edtts_generic.h): plain [N][K] weights, no fragment stream
  int BF16;  // 1: bf16 contractions (edtts_bf16.h): the fragment stream holds bf16 fragments of 16 outputs x 32 inputs
  int MM16;  // 1 (GEN only, EDTTS_MATMUL_BF16): every `linear` of the generic path on bf16 MFMAs (edtts_generic16.h); same blob
  int ATT16; // 1 (GEN only, EDTTS_ATTN_BF16): both attention contractions and their backward on bf16 MFMAs (edtts_generic_attn16.h)
  int TAPE16;  // 1 (MM16 and ATT16 only, EDTTS_TAPE_BF16): q|k|v, the cross queries, the cross K|V and the SwiGLU output are stored as bf16
  int H, HEADS, MEL, L, DH, DHP, HT, MT, R, RT, SD, NTOK, MAXPOS, MAXCPOS, NSTEP;
  int FM;  // ffn_mult: the FFN's hidden width is FM * H (layers/transformer.py:32-45: Linear(H, 2 FM H) -> SwiGLU -> Linear(FM H, H))
  size_t tok, semp, semp_b, t1T, t1b, t3T, t3b, step, inp, inp_b, pe, cpe, fnw, fnb, outp_b, freqs;
  LayerLayout layer[kMaxLayers];
  size_t s_outp;  // stream: final out_proj [MT n-tiles][HT]
  size_t s_ctx16; // bf16 instance: fragment stream of the context kernel, per layer kv_down (n-tile pairs) | kv_up (n-tile pairs)
  size_t total;
};
// fragments of one layer in the bf16 context stream: kv_down R x H (RT n-tiles x H/32 k-tiles) + kv_up 2H x R
static size_t ctx16_frags(const Layout& lo) { return (size_t)lo.RT * (lo.H / 32) + (size_t)2 * lo.HT * (lo.R / 32); }
constexpr size_t kFrag = 256;  // floats per fragment (64 lanes x float4)

static size_t align64(size_t v) { return (v + 63) & ~(size_t)63; }

static bool has_instance(const Layout& lo);

// Generic layout: the tables the conditioning / embedding code reads sit where the fused layout keeps them (time MLP and AdaLN
// projections transposed for k_cond_mlp / k_cond_ada); every other Linear is the state-dict's [N][K] matrix as it is.
static int make_generic_layout(const EdttsDims* d, Layout* lo) {
  if (d->ffn_mult < 1 || d->ffn_mult > 4) return fail(EDTTS_ERR_UNSUPPORTED, "ffn_mult=%d outside [1, 4]", d->ffn_mult);
  if (d->layers < 1 || d->layers > kMaxLayers) return fail(EDTTS_ERR_UNSUPPORTED, "layers=%d out of [1,%d]", d->layers, kMaxLayers);
  if (d->heads < 1 || d->hidden < 2 || d->hidden % d->heads || d->hidden % 2)
    return fail(EDTTS_ERR_UNSUPPORTED, "generic kernels: hidden=%d heads=%d: need hidden %% heads == 0 and an even hidden", d->hidden, d->heads);
  if (d->hidden / d->heads > 128)
    return fail(EDTTS_ERR_UNSUPPORTED, "generic kernels: head_dim=%d > 128 (hidden=%d heads=%d)", d->hidden / d->heads, d->hidden, d->heads);
  if (d->n_mels < 1 || d->semantic_dim < 1 || d->codebook_size < 1 || d->max_pos < 1 || d->max_ctx_pos < 1 || d->n_step_emb < 1)
    return fail(EDTTS_ERR_UNSUPPORTED, "generic kernels: n_mels=%d semantic_dim=%d codebook_size=%d and the table sizes must be >= 1",
                d->n_mels, d->semantic_dim, d->codebook_size);
  memset(lo, 0, sizeof(*lo));
  lo->GEN = 1;
  lo->H = d->hidden; lo->HEADS = d->heads; lo->MEL = d->n_mels; lo->L = d->layers;
  lo->DH = lo->H / lo->HEADS; lo->DHP = (lo->DH + 15) / 16 * 16;
  lo->R = lo->H / 2; lo->SD = d->semantic_dim; lo->NTOK = d->codebook_size;
  lo->MAXPOS = d->max_pos; lo->MAXCPOS = d->max_ctx_pos; lo->NSTEP = d->n_step_emb; lo->FM = d->ffn_mult;
  const size_t H = lo->H, R = lo->R, SD = lo->SD, MEL = lo->MEL, FH = (size_t)lo->FM * lo->H;
  size_t o = 0;
  auto take = [&](size_t n) { size_t r = o; o = align64(o + n); return r; };
  lo->tok = take((size_t)lo->NTOK * H);
  lo->semp = take(H * SD); lo->semp_b = take(H);
  lo->t1T = take(H * H); lo->t1b = take(H); lo->t3T = take(H * H); lo->t3b = take(H);
  lo->step = take((size_t)lo->NSTEP * H);
  lo->inp = take(H * MEL); lo->inp_b = take(H);
  lo->pe = take((size_t)lo->MAXPOS * H); lo->cpe = take((size_t)lo->MAXCPOS * H);
  lo->fnw = take(H); lo->fnb = take(H); lo->s_outp = take(MEL * H); lo->outp_b = take(MEL); lo->freqs = take(H / 2);
  for (int l = 0; l < lo->L; ++l) {
    LayerLayout& y = lo->layer[l];
    y.n1w = take(H); y.ada1T = take(H * 2 * H); y.ada1b = take(2 * H); y.proj_b = take(H); y.n2w = take(H);
    y.n3w = take(H); y.ada3T = take(H * 2 * H); y.ada3b = take(2 * H); y.up_b = take(2 * FH); y.down_b = take(H);
    y.kvd = take(R * H); y.kvn = take(R); y.kvu = take(2 * H * R);
    y.s_qkv = take(3 * H * H); y.g_proj = take(H * H); y.g_qp = take(H * H); y.g_op = take(H * H);
    y.g_up = take(2 * FH * H); y.g_down = take(H * FH);
  }
  lo->total = align64(o);
  return EDTTS_OK;
}

// EDTTS_MATMUL_BF16 and EDTTS_ATTN_BF16 have one legal spelling each, with or without the other; EDTTS_TAPE_BF16 only with both
// (include/edtts.h); false: the error text is set
constexpr int kMixedBits = EDTTS_MATMUL_BF16 | EDTTS_ATTN_BF16 | EDTTS_TAPE_BF16;
static bool matmul_bit_ok(const EdttsDims* d) {
  if ((d->compute_dtype & EDTTS_TAPE_BF16) && d->compute_dtype != (EDTTS_F32 | EDTTS_KERNELS_GENERIC | kMixedBits)) {
    fail(EDTTS_ERR_UNSUPPORTED,
         "compute_dtype=0x%x: EDTTS_TAPE_BF16 is legal only as EDTTS_F32 | EDTTS_KERNELS_GENERIC | EDTTS_MATMUL_BF16 | EDTTS_ATTN_BF16 | "
         "EDTTS_TAPE_BF16 (a buffer with an fp32 reader cannot be narrowed)",
         d->compute_dtype);
    return false;
  }
  const int rest = d->compute_dtype & ~kMixedBits;  // what the bits ride on
  if (!(d->compute_dtype & kMixedBits) || rest == (EDTTS_F32 | EDTTS_KERNELS_GENERIC)) return true;
  if (d->compute_dtype & EDTTS_ATTN_BF16)
    fail(EDTTS_ERR_UNSUPPORTED,
         "compute_dtype=0x%x: EDTTS_ATTN_BF16 is legal only as EDTTS_F32 | EDTTS_KERNELS_GENERIC | EDTTS_ATTN_BF16, with or without "
         "EDTTS_MATMUL_BF16",
         d->compute_dtype);
  else
    fail(EDTTS_ERR_UNSUPPORTED, "compute_dtype=0x%x: EDTTS_MATMUL_BF16 is legal only as EDTTS_F32 | EDTTS_KERNELS_GENERIC | EDTTS_MATMUL_BF16",
         d->compute_dtype);
  return false;
}

static int make_layout(const EdttsDims* d, Layout* lo) {
  if (!d) return fail(EDTTS_ERR_ARG, "dims is NULL");
  // kernel-path bits (include/edtts.h): decided here, once; packing, workspace sizing and the dispatch follow lo->GEN
  const int kbits = d->compute_dtype & (EDTTS_KERNELS_GENERIC | EDTTS_KERNELS_AUTO);
  const int dtype = d->compute_dtype & ~(EDTTS_KERNELS_GENERIC | EDTTS_KERNELS_AUTO | kMixedBits);
  const bool mm16 = (d->compute_dtype & EDTTS_MATMUL_BF16) != 0, att16 = (d->compute_dtype & EDTTS_ATTN_BF16) != 0;
  if (!matmul_bit_ok(d)) return EDTTS_ERR_UNSUPPORTED;
  if (kbits == (EDTTS_KERNELS_GENERIC | EDTTS_KERNELS_AUTO))
    return fail(EDTTS_ERR_UNSUPPORTED, "compute_dtype=0x%x: EDTTS_KERNELS_GENERIC and EDTTS_KERNELS_AUTO are exclusive", d->compute_dtype);
  if (kbits == EDTTS_KERNELS_GENERIC && dtype == EDTTS_BF16)
    return fail(EDTTS_ERR_UNSUPPORTED, "the generic kernels are fp32 only (compute_dtype=0x%x)", d->compute_dtype);
  if (kbits && dtype == EDTTS_F32) {
    bool fused = false;
    if (kbits == EDTTS_KERNELS_AUTO && d->ffn_mult >= 1 && d->ffn_mult <= 4 && d->layers >= 1 && d->layers <= kMaxLayers &&
        d->hidden % 32 == 0 && d->n_mels % 16 == 0 && d->semantic_dim % 16 == 0 && d->heads >= 1 && d->hidden % d->heads == 0) {
      Layout probe;
      memset(&probe, 0, sizeof(probe));
      probe.H = d->hidden; probe.HEADS = d->heads; probe.MEL = d->n_mels;
      fused = has_instance(probe);
    }
    if (!fused) {
      const int rc = make_generic_layout(d, lo);
      if (rc == EDTTS_OK) {
        lo->MM16 = mm16;
        lo->ATT16 = att16;
        lo->TAPE16 = (d->compute_dtype & EDTTS_TAPE_BF16) != 0;  // (matmul_bit_ok: then mm16 and att16)
      }
      return rc;
    }
  }
  // (AUTO with bf16 is the compiled bf16 path: it never falls back to fp32)
  if (d->ffn_mult < 1 || d->ffn_mult > 4) return fail(EDTTS_ERR_UNSUPPORTED, "ffn_mult=%d outside [1, 4]", d->ffn_mult);
  if (d->layers < 1 || d->layers > kMaxLayers) return fail(EDTTS_ERR_UNSUPPORTED, "layers=%d out of [1,%d]", d->layers, kMaxLayers);
  if (d->hidden % 32 || d->n_mels % 16 || d->semantic_dim % 16 || d->heads < 1 || d->hidden % d->heads)
    return fail(EDTTS_ERR_UNSUPPORTED, "hidden=%d heads=%d n_mels=%d semantic_dim=%d: need hidden%%32==0, n_mels%%16==0, semantic_dim%%16==0",
                d->hidden, d->heads, d->n_mels, d->semantic_dim);
  if (dtype != EDTTS_F32 && dtype != EDTTS_BF16)
    return fail(EDTTS_ERR_UNSUPPORTED, "compute_dtype=%d (0 = f32, 1 = bf16)", d->compute_dtype);
  if (dtype == EDTTS_BF16 && d->hidden != 32 * d->heads)
    return fail(EDTTS_ERR_UNSUPPORTED, "the bf16 instance needs head_dim 32 (hidden=%d heads=%d)", d->hidden, d->heads);
  memset(lo, 0, sizeof(*lo));
  lo->BF16 = dtype == EDTTS_BF16;
  lo->H = d->hidden; lo->HEADS = d->heads; lo->MEL = d->n_mels; lo->L = d->layers;
  lo->DH = lo->H / lo->HEADS; lo->DHP = (lo->DH + 15) / 16 * 16; lo->HT = lo->H / 16; lo->MT = lo->MEL / 16;
  lo->R = lo->H / 2; lo->RT = lo->R / 16; lo->SD = d->semantic_dim; lo->NTOK = d->codebook_size;
  lo->MAXPOS = d->max_pos; lo->MAXCPOS = d->max_ctx_pos; lo->NSTEP = d->n_step_emb; lo->FM = d->ffn_mult;
  const size_t FM = lo->FM;
  const size_t H = lo->H, HT = lo->HT, MT = lo->MT, R = lo->R, RT = lo->RT, SD = lo->SD;
  const size_t KPT = (size_t)lo->HEADS * lo->DHP / 16;  // k-tiles of the head-padded projections
  size_t o = 0;
  auto take = [&](size_t n) { size_t r = o; o = align64(o + n); return r; };
  lo->tok = take((size_t)lo->NTOK * H);
  lo->semp = take(HT * (SD / 16) * kFrag); lo->semp_b = take(H);
  lo->t1T = take(H * H); lo->t1b = take(H); lo->t3T = take(H * H); lo->t3b = take(H);
  lo->step = take((size_t)lo->NSTEP * H);
  lo->inp_b = take(H);
  lo->pe = take((size_t)lo->MAXPOS * H); lo->cpe = take((size_t)lo->MAXCPOS * H);
  lo->fnw = take(H); lo->fnb = take(H); lo->outp_b = take(lo->MEL); lo->freqs = take(H / 2);
  for (int l = 0; l < lo->L; ++l) {
    LayerLayout& y = lo->layer[l];
    y.n1w = take(H); y.ada1T = take(H * 2 * H); y.ada1b = take(2 * H); y.proj_b = take(H); y.n2w = take(H);
    y.n3w = take(H); y.ada3T = take(H * 2 * H); y.ada3b = take(2 * H); y.up_b = take(2 * FM * H); y.down_b = take(H);
    y.kvd = take(RT * HT * kFrag); y.kvn = take(R); y.kvu = take(2 * HT * RT * kFrag);
  }
  // contiguous fragment stream: inp qkv(0) body(0) qkv(1) body(1) ... body(L-1) outp  + one ring of slack
  if (lo->BF16) {
    // bf16 fragments: 16 outputs x 32 inputs = 1 KiB (= kFrag floats), see edtts_bf16.h
    const size_t KT = H / 32, MKT = (lo->MEL + 31) / 32, MTP = (MT + 1) / 2;
    lo->s_ctx16 = o; o += (size_t)lo->L * ctx16_frags(*lo) * kFrag;  // (the decoder's stream follows: ring read-ahead stays inside the blob)
    lo->inp = o; o += MKT * HT * kFrag;  // in_proj, k-major
    for (int l = 0; l < lo->L; ++l) {
      LayerLayout& y = lo->layer[l];
      y.s_qkv = o; o += 3 * HT * KT * kFrag;  // q pairs | k pairs | v pairs
      y.s_body = o;
      y.s_ffn = o + 3 * HT * KT * kFrag;      // proj (k-major) | q_proj (pairs) | out_proj (k-major)
      o = y.s_ffn + (FM * HT / 2) * (4 * KT + HT) * kFrag;  // per down k-tile (32 hidden features): up value/gate of its two hidden tiles, then the down fragments
    }
    lo->s_outp = o; o += MTP * 2 * KT * kFrag;  // final out_proj as n-tile pairs (the last pair may be half empty)
    o += 8 * HT * kFrag;  // the LDS ring prefetches NS phases (of HT fragments) past the last consumed one
  } else {
  lo->inp = o; o += HT * MT * kFrag;  // in_proj, n-tile pairs: the prologue kernel streams inp | qkv(0)
  for (int l = 0; l < lo->L; ++l) {
    LayerLayout& y = lo->layer[l];
    y.s_qkv = o; o += 3 * HT * HT * kFrag;
    y.s_body = o;
    y.s_ffn = o + (KPT * HT /*proj*/ + HT * HT /*q_proj*/ + KPT * HT /*out_proj*/) * kFrag;
    o = y.s_ffn + (FM * HT * 3 * HT /*ffn: per hidden 16-tile 2 HT up + HT down fragments*/) * kFrag;
  }
  lo->s_outp = o; o += MT * HT * kFrag;
  o += 4 * HT * kFrag;  // the stream stages two phases (+ slot padding) past the last consumed fragment
  }
  lo->total = align64(o);
  return EDTTS_OK;
}

// The layout of a call that trains (edtts_generic_bwd.h) or asks where a trainable slot lies: the generic fp32 path only
// (fp32 storage; EDTTS_MATMUL_BF16 and EDTTS_ATTN_BF16 pass through to make_layout, which allows them exactly here)
static int train_layout(const EdttsDims* dims, const char* who, Layout* lo) {
  if (!dims) return fail(EDTTS_ERR_ARG, "dims is NULL");
  if (!matmul_bit_ok(dims)) return EDTTS_ERR_UNSUPPORTED;
  const int kbits = dims->compute_dtype & (EDTTS_KERNELS_GENERIC | EDTTS_KERNELS_AUTO);
  const int dtype = dims->compute_dtype & ~(EDTTS_KERNELS_GENERIC | EDTTS_KERNELS_AUTO | kMixedBits);
  if (kbits != EDTTS_KERNELS_GENERIC)
    return fail(EDTTS_ERR_UNSUPPORTED, "%s: training runs on the generic kernels only (compute_dtype=0x%x lacks EDTTS_KERNELS_GENERIC)", who,
                dims->compute_dtype);
  if (dtype != EDTTS_F32) return fail(EDTTS_ERR_UNSUPPORTED, "%s: training is fp32 only (compute_dtype=0x%x)", who, dims->compute_dtype);
  return make_layout(dims, lo);
}

// =========================================================================================================
// packing kernels
// =========================================================================================================
struct PackArgs {
  const float* src;
  int ld, N, K;      // source row stride, logical rows / cols
  int NT, KT;        // packed tile counts
  int rowmode;       // 0 identity, 1 ffn-up interleave (tile 2j = value rows 16j.., tile 2j+1 = gate rows N/2+16j..)
  int colmode;       // 0 identity, 1 head padding (packed col hd*DHP+dd <- hd*DH+dd; the 8-wide remainder tile is permuted, see k_pack_gemm)
  int dstmode;       // 0 n-major, 1 k-major, 2 ffn-up inside the ffn stream, 3 ffn-down inside the ffn stream
  int DH, DHP;
  float* dst;
  int scale_rows;    // rows [0, scale_rows) are multiplied by `scale` (the attention query rows carry log2(e)/sqrt(head_dim))
  float scale;
};
__global__ void k_pack_gemm(PackArgs a) {
  const int tile = blockIdx.x, lane = threadIdx.x;
  const int nt = tile / a.KT, kt = tile % a.KT;
  const int fq = lane & 15, g = lane >> 4;
  int n = 16 * nt + fq, row;
  bool rok;
  if (a.rowmode == 1) {
    const int j = nt >> 1, gate = nt & 1;
    row = gate * (a.N / 2) + 16 * j + fq;
    rok = true;
  } else {
    row = n;
    rok = n < a.N;
  }
  f4 v;
  for (int r = 0; r < 4; ++r) {
    const int k = 16 * kt + 4 * g + r;
    int col = k;
    bool cok = k < a.K;
    if (a.colmode == 1) {
      const int hd = k / a.DHP, dd = k % a.DHP;
      const int full = a.DH & ~15;  // features covered by whole 16-wide k-tiles
      if (dd < full) {
        cok = true;
        col = hd * a.DH + dd;
      } else {
        // the 8-feature remainder tile: feature full + 2g + r sits at (lane group g, MFMA step r) for r < 2, so that the
        // projection only issues 2 of the tile's 4 MFMA steps (edtts_device.h: attention_fused, kRemSteps)
        const int kk = dd - full;  // = 4g + r
        cok = (kk & 3) < 2 && full + 2 * (kk >> 2) + (kk & 3) < a.DH;
        col = hd * a.DH + full + 2 * (kk >> 2) + (kk & 3);
      }
    }
    v[r] = (rok && cok) ? a.src[(size_t)row * a.ld + col] * (row < a.scale_rows ? a.scale : 1.0f) : 0.f;
  }
  size_t frag;
  const int S3 = 2 * a.KT + a.NT;  // fragments per ffn hidden tile (valid when KT == NT == HT for mode 2; see host)
  switch (a.dstmode) {
    case 0: frag = (size_t)nt * a.KT + kt; break;
    case 1: frag = (size_t)kt * a.NT + nt; break;
    case 4: frag = (size_t)(nt >> 1) * (2 * a.KT) + 2 * kt + (nt & 1); break;           // n-tile pairs interleaved per k-tile (gemm_phase_pair)
    case 2: frag = (size_t)(nt >> 1) * (3 * a.KT) + 2 * kt + (nt & 1); break;           // up: [j][kt][value | gate], then down NT
    default: frag = (size_t)kt * (3 * a.NT) + 2 * a.NT + nt; break;                       // down: k-tile kt = hidden tile j
  }
  (void)S3;
  stg4(a.dst + (frag * 64 + lane) * 4, v);
}
__global__ void k_copy(const float* src, float* dst, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}
// dst[k][n] = src[n][k]   (src [N][K])
__global__ void k_transpose(const float* src, float* dst, int N, int K) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)N * K) {
    int k = (int)(i / N), n = (int)(i % N);
    dst[i] = src[(size_t)n * K + k];
  }
}
// ffn up bias in stream order: [j][value 16 | gate 16]
__global__ void k_pack_upbias(const float* src, float* dst, int H2 /* = 2H hidden */) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 2 * H2) {
    int j = i / 32, w = i % 32;
    dst[i] = (w < 16) ? src[16 * j + w] : src[H2 + 16 * j + (w - 16)];
  }
}

// bf16 fragments (edtts_bf16.h): tile (nt, kt) = 16 outputs x 32 inputs; lane (n = lane & 15, g = lane >> 4) holds the 8 inputs
// k = 32 kt + slot(g, j), slot(g, j) = j < 4 ? 4 g + j : 16 + 4 g + (j - 4)
struct PackArgs16 {
  const float* src;
  int ld, N, K;     // source row stride, logical rows / cols
  int NT, KT;       // packed tile counts
  int mode;         // 0 n-tile pairs [nt/2][kt][nt%2]; 1 k-major [kt][nt]; 2 ffn up (tile = 2*hidden tile + value|gate); 3 ffn down
  int blk, upfr;    // ffn stream: fragments per down k-tile block, up fragments per block
  unsigned short* dst;
  int scale_rows;
  float scale;
};
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float v) {
  const __bf16 b = (__bf16)v;  // v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN
  return __builtin_bit_cast(unsigned short, b);
}
__global__ void k_pack_gemm16(PackArgs16 a) {
  const int tile = blockIdx.x, lane = threadIdx.x;
  const int nt = tile / a.KT, kt = tile % a.KT;
  const int fq = lane & 15, g = lane >> 4;
  int row;
  bool rok;
  size_t frag;
  if (a.mode == 2) {
    const int jh = nt >> 1, gate = nt & 1;
    row = gate * (a.N / 2) + 16 * jh + fq;
    rok = true;
    frag = (size_t)(jh >> 1) * a.blk + (size_t)(jh & 1) * (a.upfr / 2) + 2 * kt + gate;
  } else {
    row = 16 * nt + fq;
    rok = row < a.N;
    if (a.mode == 0) frag = (size_t)(nt >> 1) * (2 * a.KT) + 2 * kt + (nt & 1);
    else if (a.mode == 1) frag = (size_t)kt * a.NT + nt;
    else frag = (size_t)kt * a.blk + a.upfr + nt;
  }
  unsigned short v[8];
  for (int j = 0; j < 8; ++j) {
    const int k = 32 * kt + (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4));
    const float w = (rok && k < a.K) ? a.src[(size_t)row * a.ld + k] * (row < a.scale_rows ? a.scale : 1.0f) : 0.f;
    v[j] = f32_to_bf16_bits(w);
  }
  unsigned short* d = a.dst + (frag * 64 + lane) * 8;
  for (int j = 0; j < 8; ++j) d[j] = v[j];
}

// =========================================================================================================
// conditioning kernel: one block per (t, step_idx) row
// =========================================================================================================
constexpr int kMaxHostRows = 32;
struct CondArgs {
  const int64_t* t;         // device rows, or null -> t_host / step_host (by-value, graph-capturable)
  const int64_t* step_idx;  // may be null
  int use_host, host_has_step;
  int t_host[kMaxHostRows], step_host[kMaxHostRows];
  int H, L, n_step;
  const float *freqs, *t1T, *t1b, *t3T, *t3b, *step;
  const float* blob;
  unsigned ada1T[kMaxLayers], ada1b[kMaxLayers], ada3T[kMaxLayers], ada3b[kMaxLayers];  // offsets (floats) -- blob < 16 GiB
  float* cond;   // [rows][L][2][2H]
  float* tcond;  // [rows][H] scratch
  unsigned* err; // index-error word of the workspace
};
// stage 1: t_cond row = Linear(GELU(Linear(sinus(t)))) + step_emb[step_idx]      (one block per row)
__global__ __launch_bounds__(256) void k_cond_mlp(CondArgs a) {
  extern __shared__ float sm[];
  float* e = sm;        // [H] sinusoidal embedding
  float* u = sm + a.H;  // [H] hidden of the MLP
  const int row = blockIdx.x, tid = threadIdx.x, H = a.H, half = H / 2;
  const float tf = a.use_host ? (float)a.t_host[row] : (float)a.t[row];
  for (int j = tid; j < H; j += blockDim.x) {
    const float arg = tf * a.freqs[j < half ? j : j - half];  // embeddings.py:42
    e[j] = j < half ? sinf(arg) : cosf(arg);                  // cat[sin, cos], embeddings.py:43
  }
  __syncthreads();
  for (int n = tid; n < H; n += blockDim.x) {
    float acc = a.t1b[n];
#pragma unroll 8
    for (int k = 0; k < H; ++k) acc = fmaf(e[k], a.t1T[(size_t)k * H + n], acc);
    u[n] = 0.5f * acc * (1.0f + erff(acc * 0.70710678118654752440f));  // exact GELU (decoder.py:29)
  }
  __syncthreads();
  long sidx = -1;
  if (a.use_host ? a.host_has_step : (a.step_idx != nullptr)) {
    sidx = a.use_host ? (long)a.step_host[row] : (long)a.step_idx[row];
    if (sidx < 0 || sidx >= a.n_step) {  // the reference raises IndexError (F7): clamp (never fault), leave a mark for the host
      if (tid == 0) atomicOr(a.err, (unsigned)EDTTS_IDX_STEP);
      sidx = sidx < 0 ? 0 : a.n_step - 1;
    }
  }
  for (int n = tid; n < H; n += blockDim.x) {
    float acc = a.t3b[n];
#pragma unroll 8
    for (int k = 0; k < H; ++k) acc = fmaf(u[k], a.t3T[(size_t)k * H + n], acc);
    if (sidx >= 0) acc += a.step[(size_t)sidx * H + n];
    a.tcond[(size_t)row * H + n] = acc;
  }
}
// stage 2: AdaLN rows (1 + scale | shift) = proj(t_cond) for every (row, layer, norm1|norm3)   (transformer.py:64-66)
__global__ __launch_bounds__(256) void k_cond_ada(CondArgs a) {
  extern __shared__ float sm[];
  const int row = blockIdx.x, lw = blockIdx.y, l = lw >> 1, which = lw & 1, H = a.H;
  for (int k = threadIdx.x; k < H; k += blockDim.x) sm[k] = a.tcond[(size_t)row * H + k];
  __syncthreads();
  const float* WT = a.blob + (which ? a.ada3T[l] : a.ada1T[l]);
  const float* bb = a.blob + (which ? a.ada3b[l] : a.ada1b[l]);
  float* out = a.cond + (((size_t)row * a.L + l) * 2 + which) * 2 * H;
  for (int n = blockIdx.z * blockDim.x + threadIdx.x; n < 2 * H; n += gridDim.z * blockDim.x) {
    float acc = bb[n];
#pragma unroll 8
    for (int k = 0; k < H; ++k) acc = fmaf(sm[k], WT[(size_t)k * 2 * H + n], acc);
    out[n] = n < H ? 1.0f + acc : acc;  // first half = scale (stored as 1+scale), second = shift
  }
}

// =========================================================================================================
// shared kernel argument block
// =========================================================================================================
struct KArgs {
  int B, T, Tp, S, Sp, window, max_pos, max_cpos, n_tok, SD, L;
  // inputs / outputs
  const float* x;  // [B][T][MEL]
  float* h;
  // q / k / v^T ping-pong between layers: a launch reads the set its predecessor wrote (q, k, vT) and writes the OTHER set
  // (q_out, k_out, vT_out) -- blocks of one launch run at different times, and a block's QKV tail must not overwrite K/V halo
  // rows that a neighbouring block of the same launch has yet to read for its self-attention.
  const float *q, *k, *vT;
  float *q_out, *k_out, *vT_out;
  float *kc, *vcT;  // cross K / V^T cache: kernel-specific base (k_ctx: whole cache; k_layer: this layer's slice)
  // in-painting multistep tail (TAIL_VLMS): the known frames blended into the NEXT step's x (these three fields fill 24 bytes that had
  // no reader, so every later field keeps its kernel-argument offset and the other kernels' code is unchanged)
  const float* known;               // [B][inj_frames][MEL] or null: no blend
  const unsigned long long* seeds;  // per-row Philox seeds [B] or null: `seed`, keyed by the element of the whole [B][inj_frames][MEL] tensor
  int inj_frames, inj_mel;          // overlap_len, n_mels
  const int64_t* sem_idx;
  const float* sem_feat;
  const float* cond;  // row base: [L][2][2H] per row
  int cond_bstride;   // floats between batch rows (0 = one row shared by the batch)
  int layer;
  int ffn_tiles;  // 16-wide tiles of the FFN's hidden width: ffn_mult * H / 16
  int diag_skip;  // diagnostic builds only: the wave selector of EDTTS_STAMPS (STAMPX), the slot base of EDTTS_WAVELOG
  unsigned long long* stamps;  // EDTTS_STAMPS builds only: s_memtime stamps of block 0 / wave 0 (see edtts_debug_set_stamps)
  // weights
  const float *tok, *semp, *semp_b, *cpe, *inp, *inp_b, *pe;
  const float *n1w, *proj_b, *n2w, *n3w, *up_b, *down_b, *fnw, *fnb, *outp_b;
  const float* stream;
  // tail outputs
  float *eps, *x_prev, *x0;
  float c_s1m, c_sab, c_sabp, c_dir;      // DDIM tail scalars
  float p_coef1, p_coef2, p_sd;           // DDPM tail scalars (schedule.py:227-237)
  const float* noise;                     // DDPM tail: injected noise [B,T,MEL] of this step, or null -> Philox
                                          // (TAIL_VLMS: p_coef1 / p_coef2 = the blend's c_known / c_noise, noise = its [B,inj_frames,MEL]
                                          //  draws or null -> Philox (seed | seeds, step))
  unsigned long long seed;
  unsigned long long philox_base;         // global element index of this shard's element 0 (batch_offset * T * MEL)
  unsigned step;
  LmsCoef lms;                            // multistep-solver tail
  VpredCoef vp;                           // v-prediction in-painting sampler tail
  const float* v_uncond;                  // ... its unconditional prediction (classifier-free guidance), or null
  const float *h_new, *h_old;             // previous x0 predictions (may alias x0_hist: read before write, same lane)
  float *x0_hist, *x0_all;                // where this step's x0 goes (history slot; optional intermediates)
  const int64_t *t_len, *s_len;           // per-utterance frame / token counts [B] of this (sub-)batch, or null: T / S for all
  int t_dbl;                              // t_len holds token counts: frames = 2 x tokens (edtts_generate_len / edtts_sample_ddpm_len)
};

// Per-utterance lengths (edtts_*_len).  Utterance b has n_b = len[b] valid rows, clamped into [1, full] (the entry
// point flags out-of-range values with EDTTS_IDX_LEN); dbl: len holds token counts and n_b = 2 x clamp(len[b], 1, full / 2).  Without
// lengths every utterance has the batch-wide `full`.  b is wave-uniform, so this is one scalar load per wave.
EDTTS_DEV int utt_len_of(int64_t v, int full, bool dbl) {
  const int hi = dbl ? full >> 1 : full;
  const int n = v < 1 ? 1 : (v > hi ? hi : (int)v);
  return dbl ? 2 * n : n;
}
EDTTS_DEV int utt_len(const int64_t* len, int b, int full, bool dbl = false) {
  if (len == nullptr) return full;
  return utt_len_of(len[__builtin_amdgcn_readfirstlane(b)], full, dbl);
}
// ... for an utterance index that differs between lanes (the generic path's elementwise kernels)
EDTTS_DEV int utt_len_lane(const int64_t* len, int b, int full, bool dbl = false) {
  return len == nullptr ? full : utt_len_of(len[b], full, dbl);
}
// Rows [0, live_end(n_b)) are the 32-row tiles the utterance's solo call computes; its key chunks (32 keys) never reach past them.
EDTTS_DEV int live_end(int n) { return (n + 31) & ~31; }

// block -> wave tile mapping with an XCD-aware remap: the hardware deals consecutive block ids round-robin over the 8
// XCDs; remapping gives every XCD a contiguous range of frame tiles, so the K/V halo rows a tile shares with its
// neighbours are served by that XCD's L2 (speed only; correctness does not depend on placement).
EDTTS_DEV int remap_block(int bid, int nblk) {
  const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, idx = bid >> 3;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}

struct TileId {
  int b, m0;
  bool valid;  // false: a padding wave of the last block (no block-level synchronisation in these kernels: it just exits)
};
EDTTS_DEV TileId wave_tile(int B, int Tp, int waves_per_block, int wave_frames) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tpu = Tp / wave_frames;
  int w = remap_block(blockIdx.x, gridDim.x) * waves_per_block + wave;
  TileId t;
  t.valid = w < B * tpu;
  w = t.valid ? w : B * tpu - 1;
  t.b = w / tpu;
  t.m0 = (w - t.b * tpu) * wave_frames;
  return t;
}

// ---------------------------------------------------------------------------------------------------------
// QKV of one layer from the normalised tile hn: stores q, k row-major [B][Tp][H] and v transposed [B][VR][Tp]
// (layers/attention.py:91-93: rows of qkv.weight are q | k | v, each head-major)
// ---------------------------------------------------------------------------------------------------------
template <class C>
EDTTS_DEV void qkv_tail(WStream<C>& ring0, const f4 (&hn)[C::HT][C::NF], const KArgs& a, int b, int m0, int lane) {
  constexpr int NF = C::NF;
  static_assert(C::HT % 2 == 0, "hidden must be a multiple of 32 (n-tile pairs)");
  // The tail's stores sit in the same in-order vmcnt queue as the ring's loads: a fragment requested right behind a store burst cannot
  // be consumed before the stores are acknowledged.  Nothing but the normalised tile is live here, so the tail runs on a ring of twice
  // the length (twice the distance between a request and its use): the old ring's slots are its first half.  (Round 4, same device,
  // three interleaved runs: k_layer 0.9084-0.9121 ms against 0.9133-0.9165 with the kernel's own ring.)
  constexpr int RN0 = WStream<C>::RN_;
  static_assert((2 * C::HT) % (2 * RN0) == 0, "a pair phase must be a whole number of turns of the doubled ring");
  FragRing<2 * RN0> ring;
  ring.rs = ring0.rs; ring.soff = ring0.soff; ring.voff = ring0.voff;
#pragma unroll
  for (int i = 0; i < RN0; ++i) ring.r[i] = ring0.at(i);
#pragma unroll
  for (int i = RN0; i < 2 * RN0; ++i) ring.r[i] = ring.frag(i);
  __builtin_amdgcn_sched_barrier(0);
  const int fq = lane & 15, g = lane >> 4;
  const size_t rowbase = (size_t)b * a.Tp + m0 + fq;
  // One loop per output so that the number of stores between two ring waits is a compile-time fact of each loop: the
  // s_waitcnt pass sizes vmcnt(N) for the path with the FEWEST later memory operations, and on gfx9 stores count in vmcnt
  // too -- with the q/k/v^T cases (2 / 2 / 8 stores) behind run-time branches of one loop it emitted vmcnt(9), which on the
  // v^T path forces eight more ring loads to have landed than necessary (the stores ate the prefetch depth).
#pragma unroll
  for (int which = 0; which < 3; ++which) {
    for (int nt = 0; nt < C::HT; nt += 2) {
      // two n-tiles per phase (pair-interleaved stream): four accumulator chains without the split-K sum of gemm_phase
      f4 acc[2][NF];
#pragma unroll
      for (int ft = 0; ft < NF; ++ft) acc[0][ft] = acc[1][ft] = splat(0.f);
      gemm_phase_pair<C::HT>(ring, hn, acc[0], acc[1]);
      // streaming stores: the q / k / v^T rows are consumed by the NEXT launch (plain stores measured the same: 0.9225-0.9242 vs
      // 0.9197-0.9227 ms per launch)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (which < 2) {
          float* dst = (which == 0 ? a.q_out : a.k_out) + rowbase * C::H + 16 * (nt + u) + 4 * g;
#pragma unroll
          for (int ft = 0; ft < NF; ++ft) {
            __builtin_nontemporal_store(acc[u][ft], reinterpret_cast<f4*>(dst + (size_t)ft * 16 * C::H));
          }
        } else {
          float* dst = a.vT_out + ((size_t)b * C::VR + 16 * (nt + u) + 4 * g) * a.Tp + m0 + fq;
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int ft = 0; ft < NF; ++ft) {
              __builtin_nontemporal_store(acc[u][ft][r], dst + (size_t)r * a.Tp + 16 * ft);
            }
        }
      }
    }
  }
}

// =========================================================================================================
// prologue: h = in_proj(x) + pe ; AdaRMSNorm(layer 0) ; QKV(layer 0)
// =========================================================================================================
template <class C>
__global__ __launch_bounds__(C::THREADS) void k_prologue(KArgs a) {
  constexpr int NF = C::NF;
  const TileId tl = wave_tile(a.B, a.Tp, C::WAVES, C::WF);
  if (!tl.valid) return;
  const int lane = threadIdx.x & 63, fq = lane & 15, g = lane >> 4;
  const int b = tl.b, m0 = tl.m0;
  const int Tb = utt_len(a.t_len, b, a.T, a.t_dbl);
  if (m0 >= live_end(Tb)) return;  // a tile the utterance's solo call does not have
  WStream<C> ring;
  ring.prime(a.stream, lane);
  f4 xin[C::MT][NF];
#pragma unroll
  for (int ft = 0; ft < NF; ++ft) {
    const int f = m0 + 16 * ft + fq;
#pragma unroll
    for (int t = 0; t < C::MT; ++t)
      xin[t][ft] = f < Tb ? ldg4(a.x + ((size_t)b * a.T + f) * C::MEL + 16 * t + 4 * g) : splat(0.f);
  }
  // h = (in_proj(x) + bias) + pe   (decoder.py:96-97).  The HT*MT in_proj fragments head the kernel's stream (n-tile pairs per
  // k-tile) and are consumed as ONE ring phase, so they are prefetched like every other weight.  The accumulators start at the
  // bias; the positional row is added after the GEMM (one rounding at its magnitude, as in the reference).
  f4 h[C::HT][NF];
#pragma unroll
  for (int nt = 0; nt < C::HT; ++nt) {
    const f4 bias = ldg4(a.inp_b + 16 * nt + 4 * g);
#pragma unroll
    for (int ft = 0; ft < NF; ++ft) h[nt][ft] = bias;
  }
  {
    constexpr int N = C::HT * C::MT;
    static_assert(N % WStream<C>::RN_ == 0 && C::HT % 2 == 0, "in_proj must be a whole number of ring turns");
#pragma unroll
    for (int nt = 0; nt < C::HT; nt += 2)
#pragma unroll
      for (int kt = 0; kt < C::MT; ++kt) {
        const int i = nt * C::MT + 2 * kt;
        const f4& fa = ring.at(i);
        const f4& fb = ring.at(i + 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int ft = 0; ft < NF; ++ft) h[nt][ft] = EDTTS_MFMA(fa[r], xin[kt][ft][r], h[nt][ft]);
#pragma unroll
          for (int ft = 0; ft < NF; ++ft) h[nt + 1][ft] = EDTTS_MFMA(fb[r], xin[kt][ft][r], h[nt + 1][ft]);
        }
        ring.template refill_after<N>(i);
        ring.template refill_after<N>(i + 1);
      }
    ring.advance(N);
  }
#pragma unroll
  for (int ft = 0; ft < NF; ++ft) {
    int f = m0 + 16 * ft + fq;
    f = f < a.max_pos ? f : a.max_pos - 1;
#pragma unroll
    for (int nt = 0; nt < C::HT; ++nt) h[nt][ft] += ldg4(a.pe + (size_t)f * C::H + 16 * nt + 4 * g);  // embeddings.py:142
  }
  {  // (padding waves have returned)
    float* hp = a.h + ((size_t)b * a.Tp + m0 + fq) * C::H + 4 * g;
#pragma unroll
    for (int nt = 0; nt < C::HT; ++nt)
#pragma unroll
      for (int ft = 0; ft < NF; ++ft) stg4(hp + 16 * nt + (size_t)ft * 16 * C::H, h[nt][ft]);
  }
  f4 hn[C::HT][NF];
  const float* mod = a.cond + (size_t)b * a.cond_bstride;  // layer 0, norm1
  rms_norm_tile<C::HT, NF>(h, a.n1w, mod, g, hn);
  qkv_tail<C>(ring, hn, a, b, m0, lane);
}

// =========================================================================================================
// transformer layer kernel
// =========================================================================================================
enum { TAIL_QKV = 0, TAIL_EPS = 1, TAIL_DDIM = 2, TAIL_DDPM = 3, TAIL_LMS = 4, TAIL_VPRED = 5, TAIL_VLMS = 6 };

// What the last layer of a decoder forward does with its eps tile (one f4 = 4 mel bins of one frame at element index idx):
// store it, or run the sampler's elementwise update on it right away.
template <int TAIL>
EDTTS_DEV void tail_apply(const KArgs& a, size_t idx, f4 ev, bool blend = false) {
  if (TAIL == TAIL_EPS) {
    stg4(a.eps + idx, ev);
  } else if (TAIL == TAIL_LMS) {
    const f4 xv = ldg4(a.x + idx);
    f4 hn = splat(0.f), ho = splat(0.f);
    if (a.lms.mode >= 2) hn = ldg4(a.h_new + idx);
    if (a.lms.mode >= 3) ho = ldg4(a.h_old + idx);
    f4 x0, xn;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v0, vn;
      lms_elem(xv[r], ev[r], hn[r], ho[r], a.lms, v0, vn);
      x0[r] = v0;
      xn[r] = vn;
    }
    stg4(a.x0_hist + idx, x0);
    if (a.x0_all) stg4(a.x0_all + idx, x0);
    stg4(a.x_prev + idx, xn);
  } else if (TAIL == TAIL_VLMS) {
    // in-painting multistep step: the guidance combine of TAIL_VPRED (a select, for its reason), then TAIL_LMS's update on the
    // combined v -- the same lms_elem call, so with no guidance the two tails run the same arithmetic
    const bool guided = a.v_uncond != nullptr;
    const f4 xv = ldg4(a.x + idx);
    const f4 vu = ldg4((guided ? a.v_uncond : a.x) + idx);
    f4 hn = splat(0.f), ho = splat(0.f);
    if (a.lms.mode >= 2) hn = ldg4(a.h_new + idx);
    if (a.lms.mode >= 3) ho = ldg4(a.h_old + idx);
    f4 x0, xn;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = guided ? cfg_combine(ev[r], vu[r], a.vp.cfg) : ev[r];
      float v0, vn;
      lms_elem(xv[r], v, hn[r], ho[r], a.lms, v0, vn);
      x0[r] = v0;
      xn[r] = vn;
    }
    stg4(a.x0_hist + idx, x0);
    if (a.x0_all) stg4(a.x0_all + idx, x0);
    if (!blend) stg4(a.x_prev + idx, xn);  // (a blended frame: tail_store writes the next step's q_sample there instead)
  } else if (TAIL == TAIL_VPRED) {
    // v-prediction step of the in-painting samplers, optionally with classifier-free guidance (inference_pipeline.py:125-132,179-192)
    // Without guidance the combine's result is discarded by a select, not skipped by a branch: with the branch and per-utterance
    // lengths, the 32/2/80 instance split a 16-SGPR kernel-argument tuple and left its 64-byte spill slot in the private segment
    // (DESIGN.md section 12).  The unguided load reads x again (any valid row would do).
    const bool guided = a.v_uncond != nullptr;
    const f4 xv = ldg4(a.x + idx);
    const f4 vu = ldg4((guided ? a.v_uncond : a.x) + idx);
    f4 v, xn;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = guided ? cfg_combine(ev[r], vu[r], a.vp.cfg) : ev[r];
#pragma unroll
    for (int r = 0; r < 4; ++r) xn[r] = vpred_elem(xv[r], v[r], a.vp);
    stg4(a.x_prev + idx, xn);
  } else if (TAIL == TAIL_DDPM) {
    // ancestral DDPM update (schedule.py:222-238): mean + [t>0] * sqrt(posterior variance) * noise
    const f4 xv = ldg4(a.x + idx);
    const f4 nz = a.noise ? ldg4(a.noise + idx) : philox_normal4(a.seed, a.step, (a.philox_base + idx) >> 2);
    const DdpmCoef cf{a.p_coef1, a.p_coef2, a.p_sd};
    f4 xp;
#pragma unroll
    for (int r = 0; r < 4; ++r) xp[r] = ddpm_elem(xv[r], ev[r], nz[r], cf);
    stg4(a.x_prev + idx, xp);
  } else {
    // DDIM update, same operation order as schedule.py:189-199 (no fma contraction)
    const f4 xv = ldg4(a.x + idx);
    f4 x0, xp;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v0, vp;
      ddim_elem(xv[r], ev[r], a.c_s1m, a.c_sab, a.c_sabp, a.c_dir, v0, vp);
      x0[r] = v0;
      xp[r] = vp;
    }
    stg4(a.x0 + idx, x0);
    stg4(a.x_prev + idx, xp);
  }
}
// ... and for a frame past its utterance's length (edtts_*_len): zeros wherever tail_apply would have stored
template <int TAIL>
EDTTS_DEV void tail_zero(const KArgs& a, size_t idx) {
  const f4 z = splat(0.f);
  if (TAIL == TAIL_EPS) {
    stg4(a.eps + idx, z);
  } else if (TAIL == TAIL_LMS || TAIL == TAIL_VLMS) {
    stg4(a.x0_hist + idx, z);
    if (a.x0_all) stg4(a.x0_all + idx, z);
    stg4(a.x_prev + idx, z);
  } else if (TAIL == TAIL_DDIM) {
    stg4(a.x0 + idx, z);
    stg4(a.x_prev + idx, z);
  } else {
    stg4(a.x_prev + idx, z);
  }
}
// tail of frame f < T of utterance b (Tb frames valid) at element idx
// TAIL_VLMS, frame f < min(inj_frames, T_b) of a call with a known tail: what the NEXT step starts from there is not the update but
// q_sample(known, t_next) (k_inpaint_inject's values: the same draws and the same qsample_elem), after the last step the known frames
// themselves (c_noise = 0); tail_apply has left x_prev alone there.  idx is a multiple of 4 and inj_mel % 4 == 0 (the callers' vector paths), so a quad lies in one frame.
EDTTS_DEV void vlms_blend(const KArgs& a, size_t idx) {
  const size_t row = (size_t)a.T * a.inj_mel, b = idx / row, r = idx - b * row;  // r: element within the row's [inj_frames][MEL] block
  const size_t ki = b * ((size_t)a.inj_frames * a.inj_mel) + r;
  const f4 kv = ldg4(a.known + ki);
  f4 o = kv;
  if (a.p_coef2 != 0.f) {
    const unsigned long long sd = a.seeds ? a.seeds[b] : a.seed;
    const f4 nz = a.noise ? ldg4(a.noise + ki) : philox_normal4(sd, a.step, (a.seeds ? r : ki) >> 2);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = qsample_elem(kv[e], a.p_coef1, nz[e], a.p_coef2);
  }
  stg4(a.x_prev + idx, o);
}
template <int TAIL>
EDTTS_DEV void tail_store(const KArgs& a, int f, int Tb, size_t idx, f4 ev) {
  if constexpr (TAIL == TAIL_VLMS) {
    const bool blend = a.known != nullptr && f < Tb && f < a.inj_frames;
    if (f < Tb) tail_apply<TAIL>(a, idx, ev, blend);
    else tail_zero<TAIL>(a, idx);
    if (blend) vlms_blend(a, idx);
  } else {
    if (f < Tb) tail_apply<TAIL>(a, idx, ev);
    else tail_zero<TAIL>(a, idx);
  }
}

struct QGlobal {  // q rows in global memory, row-major [Tp][H]: buffer loads (descriptor base = row m0 of the utterance)
  __amdgpu_buffer_rsrc_t rs;
  unsigned v4, v2;  // this lane's byte offsets: row fq, feature quad 4 g / pair 2 g
  int H;
  EDTTS_DEV QGlobal(const float* row_m0, int H_, int fq, int g) : rs(make_rsrc(row_m0)), v4((unsigned)(fq * H_ + 4 * g) * 4u), v2((unsigned)(fq * H_ + 2 * g) * 4u), H(H_) {}
  EDTTS_DEV f4 q4(int ft, int col) const { return bufld4(rs, v4, (unsigned)(ft * 16 * H + col) * 4u); }
  EDTTS_DEV f2 q2(int ft, int col) const { return bufld2(rs, v2, (unsigned)(ft * 16 * H + col) * 4u); }
};
struct QLds {  // q tile in this wave's LDS region, [32][ld]
  const float* b4;  // row fq, column 4 g
  const float* b2;  // row fq, column 2 g
  int ld;
  EDTTS_DEV QLds(const float* tile, int ld_, int fq, int g) : b4(tile + fq * ld_ + 4 * g), b2(tile + fq * ld_ + 2 * g), ld(ld_) {}
  EDTTS_DEV f4 q4(int ft, int col) const { return *reinterpret_cast<const f4*>(b4 + ft * 16 * ld + col); }
  EDTTS_DEV f2 q2(int ft, int col) const { return *reinterpret_cast<const f2*>(b2 + ft * 16 * ld + col); }
};

// Where the residual tile waits while a branch accumulates (measured on one MI355X, B=256, T=512, whole generate_mel call):
//   in LDS, next to the (unpadded) cross-attention q tiles -- 160 KiB per block at H = 160 (Cfg::Q_IN_LDS)           16.42 ms
//   in LDS, with the cross-attention q rows going through global memory (this wave's dead self-attention q rows)     16.53 ms
//   in the wave's own rows of the h buffer (global), q tiles padded in LDS                                           16.6 ms
// The first form is used where it fits, the second otherwise (hidden 256: four waves x 32 KiB of residual tiles).
template <class C, int TAIL>
EDTTS_DEV void layer_tile(const KArgs& a, float* smem, int wave, int lane, int b, int m0, int Tb, int Sb) {
  constexpr int NF = C::NF;
  const int fq = lane & 15, g = lane >> 4;
  // this wave's parking place for the residual tile, in REGISTER layout (element [nt][ft] of lane l at ((nt*NF + ft)*64 + l) * 16 B:
  // conflict-free b128 accesses, no padding)
  f4* const stash = reinterpret_cast<f4*>(smem) + (size_t)wave * C::HT * NF * 64 + lane;
  constexpr int QLDS = C::H;  // q rows unpadded: stash + q tiles fill the CU's 160 KiB exactly at H = 160 (q is read a few times per head)
  float* qtile = smem + (size_t)C::WAVES * C::HT * NF * 256 + (size_t)wave * C::WF * QLDS;  // (only touched when C::Q_IN_LDS)
  const size_t rowbase = (size_t)b * a.Tp + m0 + fq;

  STAMPX(a.stamps, 0, a.diag_skip);
  WStream<C> ring;
  ring.prime(a.stream, lane);

  // Residual stream: every branch (self-attention, cross-attention, FFN) is accumulated by the MFMAs into a tile that starts at the
  // branch's bias (or 0) and is added to the residual ONCE at the end of the branch -- as the reference does (x = x + f(x),
  // transformer.py:146,151,158).  Accumulating the ~640 products of a layer straight into the residual would round each partial
  // sum at the residual's magnitude (|h| ~ 2..8, ulp 2.4e-7 .. 4.8e-7) instead of the branch's (~0.1..1): measured on MI355X, that
  // alone put the decoder's error vs the fp64 arbiter at 3.8e-6 max (the reference's own fp32: 1.1e-6); with the branches apart it
  // is 1.0e-6 max / 1.9e-7 rms, i.e. at the reference's level.  While a branch accumulates, the residual tile is parked (see
  // the note above the kernel) rather than held in 16*NF*HT more registers.
  f4 h[C::HT][NF];
  float* const hp = a.h + rowbase * C::H + 4 * g;
  auto park_h = [&]() {
#pragma unroll
    for (int nt = 0; nt < C::HT; ++nt)
#pragma unroll
      for (int ft = 0; ft < NF; ++ft) stash[(nt * NF + ft) * 64] = h[nt][ft];
  };
  auto add_parked_h = [&]() {  // h (the finished branch) += residual
#pragma unroll
    for (int nt = 0; nt < C::HT; ++nt)
#pragma unroll
      for (int ft = 0; ft < NF; ++ft) h[nt][ft] += stash[(nt * NF + ft) * 64];
  };
  // ---- x = x + attn(norm1(x, cond))   (transformer.py:142-146; q/k/v were produced by the previous kernel) ----
  {
    // the residual goes from the h buffer straight to its parking place (the loads fly together with the first head's q / K / V^T)
    // (the same move by LDS-DMA, past the registers, measured 0.9293 against 0.9281 ms: not worth a hidden DMA)
#pragma unroll
    for (int nt = 0; nt < C::HT; ++nt)
#pragma unroll
      for (int ft = 0; ft < NF; ++ft) h[nt][ft] = ldg4(hp + 16 * nt + (size_t)ft * 16 * C::H);
    park_h();
    // branch tile starts at the projection bias (attention.py:123); the residual itself stays parked until the branch is done
    // (a lambda, like zero_h below, because hipcc schedules the hidden-32 / 192 / 256 instances differently around a plain loop)
    auto init_proj_bias = [&]() {
#pragma unroll
      for (int nt = 0; nt < C::HT; ++nt) {
        const f4 pb = ldg4(a.proj_b + 16 * nt + 4 * g);
#pragma unroll
        for (int ft = 0; ft < NF; ++ft) h[nt][ft] = pb;
      }
    };
    init_proj_bias();
    QGlobal ql(a.q + ((size_t)b * a.Tp + m0) * C::H, C::H, fq, g);
    attention_fused<C, true, O_FUSED>(ql, a.k + (size_t)b * a.Tp * C::H, a.vT + (size_t)b * C::VR * a.Tp, a.Tp, Tb, a.window, m0, lane, ring, h,
                                      nullptr, []() {}, a.stamps ? a.stamps + 8 : nullptr, a.diag_skip);  // (no O^T parking place; unused slot)
    add_parked_h();
    STAMPX(a.stamps, 1, a.diag_skip);
  }
  // ---- x = x + cross_attn(norm2(x), context)   (transformer.py:151, mla.py:118-194) --------------------------
  {
    {
      f4 hn[C::HT][NF];
      rms_norm_tile<C::HT, NF>(h, a.n2w, nullptr, g, hn);
      park_h();
      for (int nt = 0; nt < C::HT; nt += 2) {
        f4 acc[2][NF];
#pragma unroll
        for (int ft = 0; ft < NF; ++ft) acc[0][ft] = acc[1][ft] = splat(0.f);
        gemm_phase_pair<C::HT>(ring, hn, acc[0], acc[1]);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int ft = 0; ft < NF; ++ft) {
            // without room in LDS the cross-attention q rows take the place of this wave's self-attention q rows (read by this
            // wave only, and consumed)
            if (C::Q_IN_LDS) stg4(qtile + (16 * ft + fq) * QLDS + 16 * (nt + u) + 4 * g, acc[u][ft]);
            else stg4(const_cast<float*>(a.q) + (rowbase + 16 * ft) * C::H + 16 * (nt + u) + 4 * g, acc[u][ft]);
          }
      }
    }
    STAMPX(a.stamps, 2, a.diag_skip);
    auto zero_h = [&]() {
#pragma unroll
      for (int nt = 0; nt < C::HT; ++nt)
#pragma unroll
        for (int ft = 0; ft < NF; ++ft) h[nt][ft] = splat(0.f);
    };
    zero_h();
    if constexpr (C::Q_IN_LDS) {
      QLds ql(qtile, QLDS, fq, g);
      attention_fused<C, false, O_FUSED>(ql, a.kc + (size_t)b * a.Sp * C::H, a.vcT + (size_t)b * C::VR * a.Sp, a.Sp, Sb, -1, m0, lane, ring, h,
                                         nullptr, []() {}, a.stamps ? a.stamps + 40 : nullptr, a.diag_skip);
    } else {
      QGlobal ql(a.q + ((size_t)b * a.Tp + m0) * C::H, C::H, fq, g);
      attention_fused<C, false, O_FUSED>(ql, a.kc + (size_t)b * a.Sp * C::H, a.vcT + (size_t)b * C::VR * a.Sp, a.Sp, Sb, -1, m0, lane, ring, h,
                                         nullptr, []() {});
    }
    add_parked_h();
    STAMPX(a.stamps, 3, a.diag_skip);
  }
  // ---- x = x + ffn(norm3(x, cond))   (transformer.py:154-158, :13-49) ----------------------------------------
  {
    f4 hn[C::HT][NF];
    const float* mod = a.cond + (size_t)b * a.cond_bstride + ((size_t)a.layer * 2 + 1) * 2 * C::H;
    rms_norm_tile<C::HT, NF>(h, a.n3w, mod, g, hn);
    park_h();
#pragma unroll
    for (int nt = 0; nt < C::HT; ++nt) {
      const f4 db = ldg4(a.down_b + 16 * nt + 4 * g);
#pragma unroll
      for (int ft = 0; ft < NF; ++ft) h[nt][ft] = db;
    }
    for (int j = 0; j < a.ffn_tiles; ++j) {  // (ffn_mult * HT hidden tiles: 2 HT for the reference's default)
      const f4 vb = ldg4(a.up_b + 32 * j + 4 * g), gb = ldg4(a.up_b + 32 * j + 16 + 4 * g);
      f4 v[NF], gt[NF], act[NF];
#pragma unroll
      for (int ft = 0; ft < NF; ++ft) v[ft] = gt[ft] = splat(0.f);
      gemm_phase_pair<C::HT>(ring, hn, v, gt);
      __builtin_amdgcn_sched_barrier(0);  // one VALU clump between the two MFMA phases: every MFMA<->VALU switch costs ~8 cycles
#pragma unroll
      for (int ft = 0; ft < NF; ++ft) act[ft] = swiglu_tile(v[ft], gt[ft], vb, gb);  // (edtts_coop.h shares it: transformer.py:21-23)
      __builtin_amdgcn_sched_barrier(0);
      ktile_phase<C::HT>(ring, act, h);
    }
    add_parked_h();
    STAMPX(a.stamps, 4, a.diag_skip);
  }
  // ---- tail ---------------------------------------------------------------------------------------------------
  if (TAIL == TAIL_QKV) {
    {  // (padding waves have returned)
      float* hp = a.h + rowbase * C::H + 4 * g;
#pragma unroll
      for (int nt = 0; nt < C::HT; ++nt)
#pragma unroll
        for (int ft = 0; ft < NF; ++ft) stg4(hp + 16 * nt + (size_t)ft * 16 * C::H, h[nt][ft]);
    }
    // h has been stored: normalise in place (the function is alias-safe) instead of keeping a second 16*NF*HT-register tile
    const float* mod = a.cond + (size_t)b * a.cond_bstride + ((size_t)(a.layer + 1) * 2) * 2 * C::H;
    rms_norm_tile<C::HT, NF>(h, a.n1w, mod, g, h);
    qkv_tail<C>(ring, h, a, b, m0, lane);
  } else {
    f4 hn[C::HT][NF];
    layer_norm_tile<C::HT, NF>(h, a.fnw, a.fnb, g, hn);
#pragma unroll
    for (int nt = 0; nt < C::MT; ++nt) {
      const f4 ob = ldg4(a.outp_b + 16 * nt + 4 * g);
      f4 e[NF];
#pragma unroll
      for (int ft = 0; ft < NF; ++ft) e[ft] = splat(0.f);
      gemm_phase<C::HT>(ring, hn, e);
#pragma unroll
      for (int ft = 0; ft < NF; ++ft) {
        const int f = m0 + 16 * ft + fq;
        if (f >= a.T) continue;
        const size_t idx = ((size_t)b * a.T + f) * C::MEL + 16 * nt + 4 * g;
        tail_store<TAIL>(a, f, Tb, idx, e[ft] + ob);
      }
    }
  }
  STAMPX(a.stamps, 5, a.diag_skip);
#ifdef EDTTS_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stores drained
#endif
  STAMPX(a.stamps, 6, a.diag_skip);
}

// the sampler tail's zeros for a whole skipped tile (frames m0 .. m0 + WF - 1 below T)
template <class C, int TAIL>
EDTTS_DEV void tail_zero_tile(const KArgs& a, int b, int m0, int lane) {
  const int fq = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ft = 0; ft < C::NF; ++ft) {
    const int f = m0 + 16 * ft + fq;
    if (f >= a.T) continue;
#pragma unroll
    for (int nt = 0; nt < C::MT; ++nt) tail_zero<TAIL>(a, ((size_t)b * a.T + f) * C::MEL + 16 * nt + 4 * g);
  }
}
template <class C, int TAIL>
__global__ __launch_bounds__(C::THREADS, 1) void k_layer(KArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const TileId tl = wave_tile(a.B, a.Tp, C::WAVES, C::WF);
  if (!tl.valid) return;
  const int Tb = utt_len(a.t_len, tl.b, a.T, a.t_dbl);
  if (tl.m0 >= live_end(Tb)) {  // a tile the utterance's solo call does not have: only the sampler tail's zeros are left to store
    if constexpr (TAIL != TAIL_QKV) tail_zero_tile<C, TAIL>(a, tl.b, tl.m0, lane);
    return;
  }
  const int Sb = utt_len(a.s_len, tl.b, a.S);
#ifdef EDTTS_WAVELOG  // diagnostic builds: when and where every wave of the launch ran (scratch/wavelog.py)
  const unsigned long long wl_r0 = __builtin_amdgcn_s_memrealtime(), wl_c0 = __builtin_amdgcn_s_memtime();
#endif
  layer_tile<C, TAIL>(a, smem, wave, lane, tl.b, tl.m0, Tb, Sb);
#ifdef EDTTS_WAVELOG
  if (a.stamps && lane == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned long long* p = a.stamps + 6 * ((size_t)a.diag_skip + (size_t)tl.b * (a.Tp / C::WF) + tl.m0 / C::WF);
    p[0] = wl_r0; p[1] = wl_c0; p[2] = __builtin_amdgcn_s_memrealtime(); p[3] = __builtin_amdgcn_s_memtime();
    p[4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID: wave, simd, pipe, cu, sh, se
    p[5] = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
  }
#endif
}

#include "edtts_coop.h"
#include "edtts_bf16.h"

// =========================================================================================================
// context kernel: ctx = token_emb[sem_idx] (or sem_proj(features)) + pe_ctx ; per layer K / V^T cache
// =========================================================================================================
struct CtxArgs {
  int B, S, Sp, L, SD, n_tok, max_cpos;
  const int64_t* sem_idx;
  const float* sem_feat;
  const float *tok, *semp, *semp_b, *cpe;
  const float* blob;
  unsigned kvd[kMaxLayers], kvn[kMaxLayers], kvu[kMaxLayers];
  float *kc, *vcT;  // [L][B][Sp][H], [L][B][VR][Sp]
  unsigned* err;    // index-error word of the workspace
  const float* stream16;  // k_ctx16: bf16 fragment stream (Layout::s_ctx16)
  const int64_t* s_len;   // per-utterance token counts [B], or null: S for all (rows past them: token id 0 / zero features, as in the solo call)
};
template <class C>  // always instantiated with NF = 2 (32 context tokens per wave)
__global__ __launch_bounds__(64 * kCtxWaves) void k_ctx(CtxArgs a) {
  const TileId tl = wave_tile(a.B, a.Sp, kCtxWaves, 32);
  if (!tl.valid) return;  // no block-level synchronisation in this kernel
  const int lane = threadIdx.x & 63, fq = lane & 15, g = lane >> 4;
  const int b = tl.b, m0 = tl.m0;
  const int Sb = utt_len(a.s_len, b, a.S);
  if (m0 >= live_end(Sb)) return;  // context rows no key chunk of the utterance reaches
  f4 ctx[C::HT][2];
  if (a.sem_feat != nullptr) {
    // context = sem_proj(sem_features)   (decoder.py:83-85)
    const int KT = a.SD / 16;
    const f4* wp = reinterpret_cast<const f4*>(a.semp) + lane;
#pragma unroll
    for (int nt = 0; nt < C::HT; ++nt) ctx[nt][0] = ctx[nt][1] = ldg4(a.semp_b + 16 * nt + 4 * g);
    for (int kt = 0; kt < KT; ++kt) {
      f4 xin[2];
#pragma unroll
      for (int ft = 0; ft < 2; ++ft) {
        const int s = m0 + 16 * ft + fq;
        xin[ft] = s < Sb ? ldg4(a.sem_feat + ((size_t)b * a.S + s) * a.SD + 16 * kt + 4 * g) : splat(0.f);
      }
#pragma unroll
      for (int nt = 0; nt < C::HT; ++nt) {
        const f4 w = wp[(nt * KT + kt) * 64];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ctx[nt][0] = EDTTS_MFMA(w[r], xin[0][r], ctx[nt][0]);
          ctx[nt][1] = EDTTS_MFMA(w[r], xin[1][r], ctx[nt][1]);
        }
      }
    }
  } else {
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) {
      const int s = m0 + 16 * ft + fq;
      long tk = s < Sb ? (long)a.sem_idx[(size_t)b * a.S + s] : 0;
      if (tk < 0 || tk >= a.n_tok) {  // nn.Embedding would raise IndexError: clamp (never fault) and leave a mark for the host
        atomicOr(a.err, (unsigned)EDTTS_IDX_SEM);
        tk = tk < 0 ? 0 : a.n_tok - 1;
      }
      const float* row = a.tok + (size_t)tk * C::H + 4 * g;
#pragma unroll
      for (int nt = 0; nt < C::HT; ++nt) ctx[nt][ft] = ldg4(row + 16 * nt);  // decoder.py:88
    }
  }
#pragma unroll
  for (int ft = 0; ft < 2; ++ft) {
    int s = m0 + 16 * ft + fq;
    s = s < a.max_cpos ? s : a.max_cpos - 1;
    const float* row = a.cpe + (size_t)s * C::H + 4 * g;
#pragma unroll
    for (int nt = 0; nt < C::HT; ++nt) ctx[nt][ft] += ldg4(row + 16 * nt);  // decoder.py:93
  }
  // (small grids: gridDim.y blocks share a token tile's layers -- the embedding above is recomputed per block, the layers are not)
  const int lpb = (a.L + (int)gridDim.y - 1) / (int)gridDim.y;
  const int l_end = ((int)blockIdx.y + 1) * lpb < a.L ? ((int)blockIdx.y + 1) * lpb : a.L;
  for (int l = (int)blockIdx.y * lpb; l < l_end; ++l) {
    // c = RMSNorm_R(kv_down(ctx))   (mla.py:144-145)
    f4 c[C::RT][2];
    {
      FragRing<C::HT> ring;
      ring.prime(a.blob + a.kvd[l], lane);
#pragma unroll
      for (int nt = 0; nt < C::RT; ++nt) {
        c[nt][0] = c[nt][1] = splat(0.f);
        gemm_phase<C::HT>(ring, ctx, c[nt]);
      }
    }
    f4 cn[C::RT][2];
    rms_norm_tile<C::RT, 2>(c, a.blob + a.kvn[l], nullptr, g, cn);
    // kv = kv_up(c): first H outputs = K, second H = V   (mla.py:150-153)
    FragRing<C::RT> ring;
    ring.prime(a.blob + a.kvu[l], lane);
    float* kdst = a.kc + (((size_t)l * a.B + b) * a.Sp + m0 + fq) * C::H + 4 * g;
    float* vdst = a.vcT + (((size_t)l * a.B + b) * C::VR + 4 * g) * a.Sp + m0 + fq;
    for (int nt = 0; nt < 2 * C::HT; ++nt) {
      f4 acc[2] = {splat(0.f), splat(0.f)};
      gemm_phase<C::RT>(ring, cn, acc);
      if (nt < C::HT) {
        stg4(kdst + 16 * nt, acc[0]);
        stg4(kdst + 16 * nt + 16 * C::H, acc[1]);
      } else {
        float* d = vdst + (size_t)(16 * (nt - C::HT)) * a.Sp;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          d[(size_t)r * a.Sp] = acc[0][r];
          d[(size_t)r * a.Sp + 16] = acc[1][r];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// bf16 context kernel: the same embedding / positional / kv_down -> RMSNorm -> kv_up chain (mla.py:144-153) with both
// projections on v_mfma_f32_16x16x32_bf16 (fp32 accumulate, fp32 norm), weights through the block-shared LDS ring of
// edtts_bf16.h.  A wave owns 32 context tokens; per layer 12 phases at H = 256: 4 of kv_down (an n-tile pair over all k-tiles
// each), 8 of kv_up (two n-tile pairs = two heads each; K heads first, then V heads).  K comes out of the usual product
// (C/D = [feature][token] -> one 16-byte K-image store per lane and token tile), V^T out of the SWAPPED product (activations as A:
// C/D = [token][feature] -> one 16-byte V^T-image store per lane and d-tile), as in qkv_tail16.
// ---------------------------------------------------------------------------------------------------------
template <class C>
__global__ __launch_bounds__(C::THREADS, 1) void k_ctx16(CtxArgs a) {
  using namespace edtts16;
  extern __shared__ __attribute__((aligned(16))) f4 ring_lds_ctx16[];
  constexpr int RT = C::R / 16, RK = C::R / 32, KT = C::KT;
  static_assert(C::NF == 2 && C::R % 32 == 0 && 2 * KT == C::PH && C::PH % (2 * RK) == 0, "context kernel geometry");
  constexpr int PPP = C::PH / (2 * RK);  // kv_up n-tile pairs (= heads) per phase
  static_assert(C::HEADS % PPP == 0, "K heads and V heads do not share a phase");
  const TileId tl = wave_tile(a.B, a.Sp, C::WAVES, 32);
  const bool valid = tl.valid;  // (a padding wave works on a copy of the last tile -- ring barriers and DMAs -- and stores nothing)
  const int lane = threadIdx.x & 63, fq = lane & 15, g = lane >> 4;
  const int b = tl.b, m0 = tl.m0;
  // (per-utterance lengths: rows past Sb take token id 0 / zero features as in the solo call; the wave stays in the ring even past
  // live_end(Sb) -- its rows are never read then, but leaving would break the block's ring barriers)
  const int Sb = utt_len(a.s_len, b, a.S);
  LdsRing<C> ring;
  ring.start(a.stream16, ring_lds_ctx16, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane);
  f4 ctx[C::HT][2];
  if (a.sem_feat != nullptr) {
    // context = sem_proj(sem_features)   (decoder.py:83-85): once per call, fp32 fragments as in k_ctx
    const int SKT = a.SD / 16;
    const f4* wp = reinterpret_cast<const f4*>(a.semp) + lane;
#pragma unroll
    for (int nt = 0; nt < C::HT; ++nt) ctx[nt][0] = ctx[nt][1] = ldg4(a.semp_b + 16 * nt + 4 * g);
    for (int kt = 0; kt < SKT; ++kt) {
      f4 xin[2];
#pragma unroll
      for (int ft = 0; ft < 2; ++ft) {
        const int s = m0 + 16 * ft + fq;
        xin[ft] = s < Sb ? ldg4(a.sem_feat + ((size_t)b * a.S + s) * a.SD + 16 * kt + 4 * g) : splat(0.f);
      }
#pragma unroll
      for (int nt = 0; nt < C::HT; ++nt) {
        const f4 w = wp[(nt * SKT + kt) * 64];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ctx[nt][0] = EDTTS_MFMA(w[r], xin[0][r], ctx[nt][0]);
          ctx[nt][1] = EDTTS_MFMA(w[r], xin[1][r], ctx[nt][1]);
        }
      }
    }
  } else {
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) {
      const int s = m0 + 16 * ft + fq;
      long tk = s < Sb ? (long)a.sem_idx[(size_t)b * a.S + s] : 0;
      if (tk < 0 || tk >= a.n_tok) {  // nn.Embedding would raise IndexError: clamp (never fault) and leave a mark for the host
        atomicOr(a.err, (unsigned)EDTTS_IDX_SEM);
        tk = tk < 0 ? 0 : a.n_tok - 1;
      }
      const float* row = a.tok + (size_t)tk * C::H + 4 * g;
#pragma unroll
      for (int nt = 0; nt < C::HT; ++nt) ctx[nt][ft] = ldg4(row + 16 * nt);  // decoder.py:88
    }
  }
#pragma unroll
  for (int ft = 0; ft < 2; ++ft) {
    int s = m0 + 16 * ft + fq;
    s = s < a.max_cpos ? s : a.max_cpos - 1;
    const float* row = a.cpe + (size_t)s * C::H + 4 * g;
#pragma unroll
    for (int nt = 0; nt < C::HT; ++nt) ctx[nt][ft] += ldg4(row + 16 * nt);  // decoder.py:93
  }
  bf8 xin[KT][2];  // the context tile as the B operand of kv_down (the same for every layer)
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) xin[kt][ft] = pack8(ctx[2 * kt][ft], ctx[2 * kt + 1][ft]);
  const size_t hstride = (size_t)32 * a.Sp;
  // (small grids: gridDim.y blocks share a token tile's layers -- the embedding above is recomputed per block, the layers are not)
  const int lpb = (a.L + (int)gridDim.y - 1) / (int)gridDim.y;
  const int l_end = ((int)blockIdx.y + 1) * lpb < a.L ? ((int)blockIdx.y + 1) * lpb : a.L;
  for (int l = (int)blockIdx.y * lpb; l < l_end; ++l) {
    // c = RMSNorm_R(kv_down(ctx))   (mla.py:144-145)
    f4 c[RT][2];
#pragma unroll
    for (int p = 0; p < RT / 2; ++p) {
      c[2 * p][0] = c[2 * p][1] = c[2 * p + 1][0] = c[2 * p + 1][1] = splat(0.f);
      gemm16_pair<KT, false>(ring, xin, c[2 * p], c[2 * p + 1]);
    }
    bf8 cn[RK][2];
    {
      float rs[2];
#pragma unroll
      for (int ft = 0; ft < 2; ++ft) {
        float ss = 0.f;
#pragma unroll
        for (int t = 0; t < RT; ++t) ss += hsum(c[t][ft] * c[t][ft]);
        rs[ft] = rsqrtf(group_sum(ss) * (1.0f / C::R) + 1e-6f);
      }
      const float* w = a.blob + a.kvn[l];
#pragma unroll
      for (int kt = 0; kt < RK; ++kt) {
        const f4 w0 = ldg4(w + 32 * kt + 4 * g), w1 = ldg4(w + 32 * kt + 16 + 4 * g);
#pragma unroll
        for (int ft = 0; ft < 2; ++ft) cn[kt][ft] = pack8(c[2 * kt][ft] * rs[ft] * w0, c[2 * kt + 1][ft] * rs[ft] * w1);
      }
    }
    // kv = kv_up(c): first H outputs = K, second H = V   (mla.py:150-153)
    __bf16* const kimg = reinterpret_cast<__bf16*>(a.kc) + ((size_t)l * a.B + b) * a.Sp * C::H;
    __bf16* const vimg = reinterpret_cast<__bf16*>(a.vcT) + ((size_t)l * a.B + b) * a.Sp * C::H;
    for (int ph = 0; ph < 2 * C::HEADS / PPP; ++ph) {
      const lds_cf4_t fr = phase_base(ring.acquire());
      f4 fg[C::PH];
#pragma unroll
      for (int i = 0; i < C::PH; ++i) fg[i] = fr[i * 64];
      __builtin_amdgcn_sched_barrier(0);
      const bool isv = ph >= C::HEADS / PPP;  // (wave-uniform)
#pragma unroll
      for (int pp = 0; pp < PPP; ++pp) {
        const int head = (isv ? ph - C::HEADS / PPP : ph) * PPP + pp;
        f4 acc[2][2] = {{splat(0.f), splat(0.f)}, {splat(0.f), splat(0.f)}};
        if (!isv) {
#pragma unroll
          for (int kt = 0; kt < RK; ++kt)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
              for (int ft = 0; ft < 2; ++ft)
                acc[u][ft] = EDTTS_MFMA16(as_bf8(fg[pp * 2 * RK + 2 * kt + u]), cn[kt][ft], acc[u][ft]);
          // K image [head][token tile][16 tokens][32 slots]
          __bf16* d = kimg + head * hstride + (size_t)(m0 >> 4) * 512 + fq * 32 + 8 * g;
          if (valid)
#pragma unroll
            for (int ft = 0; ft < 2; ++ft) *reinterpret_cast<f4*>(d + ft * 512) = as_f4(pack8(acc[0][ft], acc[1][ft]));
        } else {
#pragma unroll
          for (int kt = 0; kt < RK; ++kt)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
              for (int ft = 0; ft < 2; ++ft)
                acc[u][ft] = EDTTS_MFMA16(cn[kt][ft], as_bf8(fg[pp * 2 * RK + 2 * kt + u]), acc[u][ft]);  // C/D = [token 4g+r of tile ft][feature 16u + fq]
          // V^T image [head][32-token chunk][d-tile u][16 d][32 token slots]; token 16 t + 4 g + r of the chunk sits at slot 8 g + 4 t + r
          __bf16* d = vimg + head * hstride + (size_t)(m0 >> 5) * 1024 + fq * 32 + 8 * g;
          if (valid)
#pragma unroll
            for (int u = 0; u < 2; ++u) *reinterpret_cast<f4*>(d + u * 512) = as_f4(pack8(acc[u][0], acc[u][1]));
        }
      }
    }
  }
  ring.drain();
}

// =========================================================================================================
// depthwise-separable conv (standalone exported layer, conv.py:25-64) -- simple, not on the timed path
// =========================================================================================================
// z[b][co][t] = pb[co] + sum_ci pw[co][ci] * (sum_j dw[ci][j] * x[b][ci][t + j - k/2])
// One block = (utterance b, 64 frames): the depthwise taps go into an LDS tile [Cip][64 + 4] (Cip = C_in rounded up to 16, the
// padding rows zero), the pointwise 1x1 conv is a [C_out x C_in] x [C_in x 64] GEMM on v_mfma_f32_16x16x4_f32 (exact fp32):
// each of the four waves owns 16 frames; A = pw rows (one float4 of 4 consecutive ci per lane and 16-wide k-tile, MFMA step r
// contracts ci = 16 kt + 4 g + r), B = the depthwise tile read from LDS once per wave and kept in registers for all co tiles.
constexpr int kDsTileT = 64, kDsLd = kDsTileT + 4;
__global__ __launch_bounds__(256) void k_dsconv_pw(const float* __restrict__ x, const float* __restrict__ dw, const float* __restrict__ pw,
                                                   const float* __restrict__ pb, int B, int Ci, int Co, int Tin, int T, int ks, int stride,
                                                   float* __restrict__ z) {  // T = output frames, Tin = input frames
  extern __shared__ float dsm[];  // [Cip][kDsLd]
  const int b = blockIdx.y, t0 = blockIdx.x * kDsTileT, pad = ks / 2;
  const int Cip = (Ci + 15) & ~15;
  for (int i = threadIdx.x; i < Cip * kDsTileT; i += blockDim.x) {
    const int ci = i / kDsTileT, tl = i % kDsTileT, tt = t0 + tl;
    float acc = 0.f;
    if (ci < Ci && tt < T) {
      const float* xr = x + ((size_t)b * Ci + ci) * Tin;
      for (int j = 0; j < ks; ++j) {
        const int ts = tt * stride + j - pad;  // Conv1d(stride, padding = k/2), layers/conv.py:33-41
        if (ts >= 0 && ts < Tin) acc = fmaf(xr[ts], dw[ci * ks + j], acc);
      }
    }
    dsm[ci * kDsLd + tl] = acc;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fq = lane & 15, g = lane >> 4;
  const int tl = 16 * wave + fq, tt = t0 + tl;
  const int KT = Cip >> 4;
  constexpr int kMaxKT = 16;  // C_in <= 256 (checked by the host)
  f4 bt[kMaxKT];
#pragma unroll
  for (int kt = 0; kt < kMaxKT; ++kt) {
    if (kt < KT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bt[kt][r] = dsm[(16 * kt + 4 * g + r) * kDsLd + tl];
    }
  }
  for (int co0 = 0; co0 < Co; co0 += 16) {
    const int row = co0 + fq;
    const float* wr = pw + (size_t)(row < Co ? row : Co - 1) * Ci;
    f4 acc = splat(0.f);
#pragma unroll
    for (int kt = 0; kt < kMaxKT; ++kt) {
      if (kt < KT) {
        const int c0 = 16 * kt + 4 * g;
        f4 a;
        if (row < Co && c0 + 3 < Ci && (Ci & 3) == 0) a = ldg4(wr + c0);
        else {
#pragma unroll
          for (int r = 0; r < 4; ++r) a[r] = (row < Co && c0 + r < Ci) ? wr[c0 + r] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = EDTTS_MFMA(a[r], bt[kt][r], acc);
      }
    }
    if (tt < T) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + 4 * g + r;
        if (co < Co) z[((size_t)b * Co + co) * T + tt] = acc[r] + pb[co];
      }
    }
  }
}
// per (b, group) mean / rstd over (Co/groups)*T contiguous elements: two passes (mean, then centred sum of squares -- as accurate
// as the reference's GroupNorm), float4 loads, wave-shuffle + one LDS hop reductions, fixed order (deterministic)
EDTTS_DEV float block_sum256(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();  // (red may still be read by the previous call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void k_dsconv_stats(const float* __restrict__ z, int Co, int T, int groups, float* __restrict__ stats) {
  __shared__ float red[4];
  const int bg = blockIdx.x, n = (Co / groups) * T;
  const float* p = z + (size_t)bg * n;  // groups are contiguous channel ranges
  const bool vec = ((n & 3) == 0) && ((((size_t)bg * n) & 3) == 0);
  float s = 0.f;
  if (vec) for (int i = threadIdx.x; i < (n >> 2); i += 256) s += hsum(ldg4(p + 4 * i));
  else for (int i = threadIdx.x; i < n; i += 256) s += p[i];
  const float mu = block_sum256(s, red) / n;
  float v = 0.f;
  if (vec) for (int i = threadIdx.x; i < (n >> 2); i += 256) {
    const f4 d = ldg4(p + 4 * i) - mu;
    v += hsum(d * d);
  }
  else for (int i = threadIdx.x; i < n; i += 256) {
    const float d = p[i] - mu;
    v += d * d;
  }
  const float var = block_sum256(v, red) / n;
  if (threadIdx.x == 0) {
    stats[2 * bg] = mu;
    stats[2 * bg + 1] = rsqrtf(var + 1e-5f);
  }
}
// y = GELU(GroupNorm(z)): one block per (b, channel), float4 along time
__global__ __launch_bounds__(128) void k_dsconv_norm(const float* __restrict__ z, const float* __restrict__ stats, const float* __restrict__ gw,
                                                     const float* __restrict__ gb, int Co, int T, int groups, float* __restrict__ y) {
  const size_t bc = blockIdx.x;
  const int co = (int)(bc % Co);
  const size_t b = bc / Co;
  const size_t bg = b * groups + co / (Co / groups);
  const float mu = stats[2 * bg], rs = stats[2 * bg + 1], w = gw[co], bb = gb[co];
  const float* zr = z + (size_t)bc * T;
  float* yr = y + (size_t)bc * T;
  auto f = [&](float v) {
    v = (v - mu) * rs * w + bb;
    return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
  };
  if ((T & 3) == 0) {
    for (int i = threadIdx.x; i < (T >> 2); i += 128) {
      const f4 v = ldg4(zr + 4 * i);
      stg4(yr + 4 * i, f4{f(v[0]), f(v[1]), f(v[2]), f(v[3])});
    }
  } else {
    for (int i = threadIdx.x; i < T; i += 128) yr[i] = f(zr[i]);
  }
}

// ---------------------------------------------------------------------------------------------------------
// Fused depthwise-separable conv: ONE block per utterance keeps z = pointwise(depthwise(x)) + bias in REGISTERS between the GEMM
// and the GroupNorm, so HBM sees exactly the algorithmic traffic (x once in, y once out).  512 threads = 8 waves (two per SIMD, 256
// registers each: the z tile of C_out = 160, T_out = 512 is 160 of them).  The pointwise weights are staged in LDS once per block
// ([C_out][C_in + 4]: conflict-free 16-byte reads); a pass covers 128 output frames (wave w owns frames 16 w .. 16 w + 15 of the
// pass) whose depthwise taps go through a second LDS tile [Cip][128 + 4].  The 1x1 conv runs on v_mfma_f32_16x16x4_f32 with TIME on
// the MFMA rows (A = depthwise tile, B = weights): the C/D registers of a lane are then 4 CONSECUTIVE frames of one channel = one
// 16-byte store per (channel tile, pass), and a channel's statistics need two cross-lane adds instead of four.
// GroupNorm statistics: per-wave per-channel sums -> LDS [8][C_out] -> per channel -> per group, all in fixed order
// (deterministic), mean first and then the centred sum of squares (two passes over the register tile, as accurate as the
// reference's GroupNorm).  Shape limits (else edtts_dsconv_forward takes the three-kernel path): C_in <= 16 KT, C_out <= 16 CT,
// T_out <= 128 NP.
// ---------------------------------------------------------------------------------------------------------
constexpr int kDfT = 128;  // frames per pass of the eight-wave form (any stride whose raw rows fit: 127 * stride + ksize <= 260)
constexpr int kDfTWide = 256;  // ... of the sixteen-wave form (stride 1, ksize <= 5: 255 + ksize <= 260): four waves per SIMD (128 registers: the z
                               // tile of a wave is 80 of them) overlap one wave's staging, taps and stores with another's MFMAs -- round 4
constexpr int kDfXld = 260;  // raw input frames per pass and channel: 127 * stride + ksize <= 260; 4 rows apart = 16 banks apart: the four lane groups of a depthwise read (rows 4 g + r) fall on disjoint banks
constexpr int kDfTapLd = 5;   // depthwise taps per channel kept in LDS by the sixteen-wave form (ksize <= 5 there; odd = conflict-free over channels)
template <int KT, int CT>
constexpr int dsconv_fused_lds_floats() { return 16 * CT * (16 * KT + 4) + 16 * KT * kDfXld + 16 * KT * kDfTapLd; }
// erf(x) by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7 absolute, far inside the layer's 1e-5 budget): 1 rcp + 1 exp2 + 7 VALU
// against ~35 instructions of the library erff -- the GELU of 21 M outputs is 19 us of chip-wide VALU time with the latter.
EDTTS_DEV float erf_as(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float e = fast_exp2(ax * ax * -1.4426950408889634f);
  const float r = fmaf(-p * t, e, 1.0f);
  return copysignf(r, x);
}
// F.gelu (erf form) in one piece: with erf(x) = sign(x) (1 - q(t) e^{-x^2}), t = 1 / (1 + 0.3275911 |x|) (erf_as above),
// 0.5 v (1 + erf(v / sqrt 2)) = max(v, 0) - |v| g,  g = 0.5 q(t) e^{-v^2 / 2}: no sign transfer, no 1 + erf -- 12 VALU + rcp + exp2.
EDTTS_DEV float gelu_as(float v) {
  const float av = fabsf(v);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f * 0.70710678118654752440f, av, 1.0f));
  float q = fmaf(0.5f * 1.061405429f, t, 0.5f * -1.453152027f);
  q = fmaf(q, t, 0.5f * 1.421413741f);
  q = fmaf(q, t, 0.5f * -0.284496736f);
  q = fmaf(q, t, 0.5f * 0.254829592f);
  const float e = fast_exp2(v * v * (-0.5f * 1.4426950408889634f));
  return fmaf(-av, q * t * e, fmaxf(v, 0.f));
}
#ifdef EDTTS_DS_STAMPS  // diagnostic build (-DEDTTS_EXPERIMENTS): s_memtime of wave 0 of every block at the phase boundaries of k_dsconv_fused
__device__ unsigned long long g_ds_stamps[1024 * 16];
#define DS_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x < 1024) g_ds_stamps[blockIdx.x * 16 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
extern "C" int edtts_debug_read_ds_stamps(unsigned long long* host) { return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_ds_stamps), sizeof(g_ds_stamps)); }
#else
#define DS_STAMP(i) do { } while (0)
#endif
#if defined(EDTTS_DS_STAMPS) && EDTTS_DS_STAMPS == 2  // sub-phases of ONE walk step (tile 3) of k_dsconv_grouped instead of the per-tile stamps
#define DS_SUB(t, i) do { if ((t) == 3) DS_STAMP(i); } while (0)
#define DS_TILE(t) do { } while (0)
#else
#define DS_SUB(t, i) do { } while (0)
#define DS_TILE(t) DS_STAMP(2 + (t))
#endif
template <int KT, int CT, int NP, int TP>
__global__ __launch_bounds__(TP * 4) void k_dsconv_fused(const float* __restrict__ x, const float* __restrict__ dw, const float* __restrict__ pw,
                                                             const float* __restrict__ pb, const float* __restrict__ gw, const float* __restrict__ gb,
                                                             int Ci, int Co, int T, int To, int ks, int stride, int groups, float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float dsm_all[];
  constexpr int kDfT = TP, kDfWaves = TP / 16, kDfThreads = 64 * kDfWaves;  // (shadow the eight-wave constants)
  constexpr int Cip = 16 * KT, WLD = Cip + 4;
  float* wsm = dsm_all;                  // [16 CT][WLD] pointwise weights (rows >= Co and columns >= Ci zero)
  float* xs = dsm_all + 16 * CT * WLD;   // [Cip][kDfXld] raw input frames of the current pass (zero outside [0, T)); reused for the statistics
  const int b = blockIdx.x, pad = ks / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fq = lane & 15, g = lane >> 4;
  const int cpg = Co / groups;
  const int nin = (kDfT - 1) * stride + ks;  // input frames one pass reads per channel (<= 260, checked by the host)
  for (int i = threadIdx.x; i < 16 * CT * Cip; i += kDfThreads) {
    const int co = i / Cip, ci = i % Cip;
    wsm[co * WLD + ci] = (co < Co && ci < Ci) ? pw[(size_t)co * Ci + ci] : 0.f;
  }
  // Sixteen-wave form (round 4): a wave requests ALL its rows of a pass in one burst (its 5 channels x 5 segments
  // are in flight together instead of three load -> LDS round trips), and the rows of pass p + 1 are requested BEFORE the taps and
  // MFMAs of pass p and parked in registers until the staging tile is free -- the second pass's z registers are not live yet.  The
  // depthwise taps then come from LDS: a global load inside the pass would make its s_waitcnt wait for the whole burst (in-order vmcnt).
  constexpr bool BURST = TP == kDfTWide;
  constexpr int SEG = (kDfXld + 63) / 64;
  constexpr int NB = (Cip + 2 * kDfWaves - 1) / (2 * kDfWaves);
  float* dws = xs + Cip * kDfXld;        // [Cip][kDfTapLd] depthwise taps (BURST)
  float vrow[BURST ? NB : 1][2][SEG];
  auto rows_request = [&](int p) {
    const int t0 = p * kDfT * stride - pad;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int ci = wave + (2 * i + h) * kDfWaves;
        const float* xr = x + ((size_t)b * Ci + (ci < Ci ? ci : 0)) * T;  // (wave-uniform)
#pragma unroll
        for (int u = 0; u < SEG; ++u) {
          const int tl = lane + 64 * u, ts = t0 + tl;
          vrow[BURST ? i : 0][h][u] = (ci < Ci && tl < nin && ts >= 0 && ts < T) ? xr[ts] : 0.f;
        }
      }
  };
  auto rows_park = [&]() {
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int ci = wave + (2 * i + h) * kDfWaves;
#pragma unroll
        for (int u = 0; u < SEG; ++u) {
          const int tl = lane + 64 * u;
          if (ci < Cip && tl < kDfXld) xs[ci * kDfXld + tl] = vrow[BURST ? i : 0][h][u];
        }
      }
  };
  DS_STAMP(0);
#ifdef EDTTS_DS_STAMPS
  if (threadIdx.x == 0) g_ds_stamps[blockIdx.x * 16 + 14] = __builtin_amdgcn_s_memrealtime();  // (100 MHz, one counter for the whole chip)
#endif
  if constexpr (BURST) {
    rows_request(0);
    for (int i = threadIdx.x; i < Cip * kDfTapLd; i += kDfThreads) {
      const int ci = i / kDfTapLd, j = i % kDfTapLd;
      dws[i] = (ci < Ci && j < ks) ? dw[ci * ks + j] : 0.f;
    }
  }
  f4 acc[CT][NP];  // lane (fq, g): channel 16 ct + fq, frames 128 p + 16 wave + 4 g + r
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[ct][p] = splat(0.f);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int tb = p * kDfT;
    if (tb >= To) break;  // (uniform)
    if (p) __syncthreads();  // the previous pass has been read
    if constexpr (BURST) {
      rows_park();
      DS_STAMP(1 + 4 * p);
      __syncthreads();  // (also covers the weight and tap tiles on the first pass)
      DS_STAMP(2 + 4 * p);
      if (p + 1 < NP && (p + 1) * kDfT < To) rows_request(p + 1);
    } else {  // raw rows of this pass: wave w stages channels w, w + 8, ...; a row is 5 wave-contiguous loads along time, two rows per batch
      const int t0 = tb * stride - pad;
      for (int c0 = wave; c0 < Cip; c0 += 2 * kDfWaves) {
        float v[2][SEG];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int ci = c0 + h * kDfWaves;
          const float* xr = x + ((size_t)b * Ci + (ci < Ci ? ci : 0)) * T;  // (wave-uniform)
#pragma unroll
          for (int u = 0; u < SEG; ++u) {
            const int tl = lane + 64 * u, ts = t0 + tl;
            v[h][u] = (ci < Ci && tl < nin && ts >= 0 && ts < T) ? xr[ts] : 0.f;
          }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int ci = c0 + h * kDfWaves;
#pragma unroll
          for (int u = 0; u < SEG; ++u) {
            const int tl = lane + 64 * u;
            if (ci < Cip && tl < kDfXld) xs[ci * kDfXld + tl] = v[h][u];
          }
        }
      }
      __syncthreads();  // (also covers the weight tile on the first pass)
    }
    f4 at[KT];  // A operand = depthwise output: rows = this wave's 16 frames (lane fq), k = input channel 16 kt + 4 g + r
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) at[kt] = splat(0.f);
    // Conv1d(stride, padding = k/2), layers/conv.py:33-41 (rows >= Ci are zero).  The tap loop is the OUTER one: its trip count is
    // a run-time value, and with it innermost the 4 KT channel sums were 4 KT separate little loops, each a serial chain of
    // LDS + global latencies (40 % of the kernel's time); a tap now issues 4 KT independent load pairs.  Same sums, tap by tap.
    for (int j = 0; j < ks; ++j) {
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ci = 16 * kt + 4 * g + r;
          const float tap = BURST ? dws[ci * kDfTapLd + j] : dw[(ci < Ci ? ci : 0) * ks + j];
          at[kt][r] = fmaf(xs[ci * kDfXld + (16 * wave + fq) * stride + j], tap, at[kt][r]);
        }
    }
    DS_STAMP(3 + 4 * p);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      if (16 * ct >= Co) break;  // (uniform)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const f4 w = *reinterpret_cast<const f4*>(wsm + (16 * ct + fq) * WLD + 16 * kt + 4 * g);  // B operand: column = channel 16 ct + fq
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[ct][p] = EDTTS_MFMA(at[kt][r], w[r], acc[ct][p]);
      }
    }
  }
  DS_STAMP(9);
  // z = acc + bias
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int co = 16 * ct + fq;
    const float bias = co < Co ? pb[co] : 0.f;
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[ct][p] += bias;
  }
  // ---- GroupNorm statistics, deterministic order ----
  float* wsum = xs;                          // [waves][16 CT]
  float* chs = xs + kDfWaves * 16 * CT;      // [16 CT] per-channel totals
  float* gst = chs + 16 * CT;                // [groups][2]: mean, rstd (groups <= C_out <= 16 CT)
  float* gws = gst + 2 * 16 * CT;            // [2][16 CT] GroupNorm weight, bias: read from LDS in the store phase -- a global load there makes
                                             // every channel tile wait for the previous tile's stores (in-order vmcnt)
  auto channel_reduce = [&](auto centred_tag) {
    constexpr bool centred = decltype(centred_tag)::value;  // (compile-time: the plain-sum pass must not carry the centring arithmetic)
    __syncthreads();  // xs / wsum free
    if (!centred && threadIdx.x < 16 * CT) {
      gws[threadIdx.x] = threadIdx.x < Co ? gw[threadIdx.x] : 0.f;
      gws[16 * CT + threadIdx.x] = threadIdx.x < Co ? gb[threadIdx.x] : 0.f;
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int co = 16 * ct + fq;
      const float mu = (centred && co < Co) ? gst[2 * (co / cpg)] : 0.f;
      float s = 0.f;
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int to = p * kDfT + 16 * wave + 4 * g + r;
          if (to < To && co < Co) {
            if (centred) {
              const float d = acc[ct][p][r] - mu;
              s += d * d;
            } else {
              s += acc[ct][p][r];
            }
          }
        }
      s += __shfl_xor(s, 16, 64);  // over the four lane groups (frames 4 g + r of the wave's 16)
      s += __shfl_xor(s, 32, 64);
      if (g == 0) wsum[wave * 16 * CT + co] = s;
    }
    __syncthreads();
    if (threadIdx.x < 16 * CT) {
      float s = 0.f;
      for (int w = 0; w < kDfWaves; ++w) s += wsum[w * 16 * CT + threadIdx.x];
      chs[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < groups) {
      float s = 0.f;
      for (int c = 0; c < cpg; ++c) s += chs[threadIdx.x * cpg + c];
      const float m = s / (float)(cpg * To);
      if (centred) gst[2 * threadIdx.x + 1] = rsqrtf(m + 1e-5f);
      else gst[2 * threadIdx.x] = m;
    }
    __syncthreads();
  };
  channel_reduce(std::integral_constant<bool, false>{});
  DS_STAMP(10);
  channel_reduce(std::integral_constant<bool, true>{});
  DS_STAMP(11);
  // ---- y = GELU(GroupNorm(z)): 16-byte stores where the row allows it ----
  const bool vec = (To & 3) == 0;
  int fq_e = fq;  // a fresh opaque copy of the lane's channel coordinate: hipcc otherwise keeps the ten channel indices of the bias
  asm volatile("" : "+v"(fq_e));  // section alive (as 64-bit pairs) through the statistics and spills them in the sixteen-wave form
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int co = 16 * ct + fq_e;
    if (co >= Co) continue;
    const float mu = gst[2 * (co / cpg)], rs = gst[2 * (co / cpg) + 1], w = gws[co], bb = gws[16 * CT + co];
    float* yr = y + ((size_t)b * Co + co) * To;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int t0 = p * kDfT + 16 * wave + 4 * g;
      f4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = (acc[ct][p][r] - mu) * rs * w + bb;
        o[r] = 0.5f * v * (1.0f + erf_as(v * 0.70710678118654752440f));
      }
      if (vec && t0 + 3 < To) stg4(yr + t0, o);
      else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (t0 + r < To) yr[t0 + r] = o[r];
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // one channel tile at a time (the z tile leaves no registers for hoisted work)
  }
  DS_STAMP(12);
#ifdef EDTTS_DS_STAMPS
  __builtin_amdgcn_s_waitcnt(0);
  DS_STAMP(13);
  if (threadIdx.x == 0) g_ds_stamps[blockIdx.x * 16 + 15] = __builtin_amdgcn_s_memrealtime();
#endif
}

// ---------------------------------------------------------------------------------------------------------
// Group-pipelined form of the fused kernel (round 4), for the layer the reference builds (conv.py:47-48: GroupNorm(min(8, C_out))
// -> C_out = 160: 8 groups of 20 channels; stride 1, ksize <= 5).  k_dsconv_fused holds the whole z tile until the statistics of
// ALL groups are known, so every byte of y is stored in the last 5 us of a block's 53 (s_memrealtime stamps, scratch/ds_stamps.py)
// and the kernel then waits 10 us for 84 MB of dirty lines to reach HBM.  GroupNorm groups are independent, though.  Here a wave
// first computes the depthwise output of its 2 x 16 frames for all input channels (the MFMA A operand: 40 registers), then walks the
// output-channel tiles in order: as soon as the last tile of a group has been computed, its statistics are taken (every wave reduces
// its own frames to a mean and the centred squares about it, ONE exchange of the sixteen pairs through LDS, exact combination in a
// fixed order -- as accurate as the reference's two-pass GroupNorm, deterministic) and every tile whose groups are complete is
// normalised, activated and STORED while the MFMAs of the next tile run: they are issued between the partial-sum write and its
// barrier, so the barrier does not idle the matrix pipe.  At most three z tiles (24 registers) are live.  Same shape limits as the
// sixteen-wave fused form, plus C_out == 16 CT and groups == 16 CT / CPG.  VEC: see the template parameter.
// ---------------------------------------------------------------------------------------------------------
template <int KT, int CT>
constexpr int dsconv_grouped_lds_floats(int ng) { return dsconv_fused_lds_floats<KT, CT>() + 3 * 16 * CT + ng * 2 * (kDfTWide / 16); }
template <int I, int N, class F>
EDTTS_DEV void dsg_static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    dsg_static_for<I + 1, N>(f);
  }
}
template <int CPG, int NG>
constexpr int dsg_first_completing(int t) {
  for (int grp = 0; grp < NG; ++grp)
    if ((CPG * grp + CPG - 1) / 16 == t) return grp;
  return -1;
}
template <int CTRL>
EDTTS_DEV float dpp_add(float v) {  // v + (v of the lane the DPP control selects), inside a row of 16 lanes
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
EDTTS_DEV float row_sum16(float v) {  // over the 16 lanes of a DPP row, the same value (bitwise) in all of them
  v = dpp_add<0xB1>(v);
  v = dpp_add<0x4E>(v);
  v = dpp_add<0x141>(v);
  return dpp_add<0x140>(v);
}
EDTTS_DEV float wave_sum64(float v) {  // over all 64 lanes, the same value (bitwise) in every lane; no LDS round trips (ds_bpermute)
  v = group_sum(v);        // the four lane groups
  v = dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]: lane ^ 1
  v = dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]: lane ^ 2
  v = dpp_add<0x141>(v);   // row_half_mirror: the other quad of the half row (the quads are uniform by now)
  v = dpp_add<0x140>(v);   // row_mirror: the other half row
  return v;
}
template <int KT, int CT, int CPG, bool VEC>  // VEC: T_out % 4 == 0 -- a lane's four frames are all inside or all outside: 16-byte stores, no scalar tail path
__global__ __launch_bounds__(kDfTWide * 4) void k_dsconv_grouped(const float* __restrict__ x, const float* __restrict__ dw, const float* __restrict__ pw,
                                                                  const float* __restrict__ pb, const float* __restrict__ gw, const float* __restrict__ gb,
                                                                  int Ci, int T, int To, int ks, float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float dsm_all[];
  constexpr int TP = kDfTWide, NP = 2, WAVES = TP / 16, THREADS = 64 * WAVES, Cip = 16 * KT, WLD = Cip + 4, Co = 16 * CT, NG = Co / CPG;
  static_assert(Co % CPG == 0 && CPG >= 16 && CPG % 4 == 0, "a channel tile meets at most two groups");
  float* wsm = dsm_all;                  // [Co][WLD] pointwise weights (columns >= Ci zero)
  float* xs = wsm + Co * WLD;            // [Cip][kDfXld] raw input frames of the current pass
  float* dws = xs + Cip * kDfXld;        // [Cip][kDfTapLd] depthwise taps
  float* chp = dws + Cip * kDfTapLd;     // [3][Co] pointwise bias, GroupNorm weight, GroupNorm bias
  float* part = chp + 3 * Co;            // [NG][2][WAVES] per-wave partial sums: plain, centred squares
  const int b = blockIdx.x, pad = ks / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fq = lane & 15, g = lane >> 4;
  const int nin = TP - 1 + ks;
  constexpr int SEG = (kDfXld + 63) / 64, NB = (Cip + 2 * WAVES - 1) / (2 * WAVES);
  float vrow[NB][2][SEG];
  auto rows_request = [&](int p) {
    const int t0 = p * TP - pad;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if ((2 * i + h) * WAVES >= Cip) continue;  // (compile-time: past the last channel for every wave)
        const int ci = wave + (2 * i + h) * WAVES;
        const float* xr = x + ((size_t)b * Ci + (ci < Ci ? ci : 0)) * T;  // (wave-uniform)
#pragma unroll
        for (int u = 0; u < SEG; ++u) {
          const int tl = lane + 64 * u, ts = t0 + tl;
          vrow[i][h][u] = (ci < Ci && tl < nin && ts >= 0 && ts < T) ? xr[ts] : 0.f;
        }
      }
  };
  auto rows_park = [&]() {
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if ((2 * i + h) * WAVES >= Cip) continue;
        const int ci = wave + (2 * i + h) * WAVES;
#pragma unroll
        for (int u = 0; u < SEG; ++u) {
          const int tl = lane + 64 * u;
          if (ci < Cip && tl < kDfXld) xs[ci * kDfXld + tl] = vrow[i][h][u];
        }
      }
  };
  DS_STAMP(0);
#ifdef EDTTS_DS_STAMPS
  if (threadIdx.x == 0) g_ds_stamps[blockIdx.x * 16 + 14] = __builtin_amdgcn_s_memrealtime();
#endif
  rows_request(0);
  {  // pointwise weights: all of a thread's loads in flight at once (as a loop of load -> LDS store round trips this took 5 us)
    constexpr int NWV = (Co * Cip + THREADS - 1) / THREADS;
    float wv[NWV];
#pragma unroll
    for (int k = 0; k < NWV; ++k) {
      const int i = threadIdx.x + k * THREADS, co = i / Cip, ci = i % Cip;
      wv[k] = (i < Co * Cip && ci < Ci) ? pw[(size_t)co * Ci + ci] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NWV; ++k) {
      const int i = threadIdx.x + k * THREADS, co = i / Cip, ci = i % Cip;
      if (i < Co * Cip) wsm[co * WLD + ci] = wv[k];
    }
  }
  for (int i = threadIdx.x; i < Cip * kDfTapLd; i += THREADS) {
    const int ci = i / kDfTapLd, j = i % kDfTapLd;
    dws[i] = (ci < Ci && j < ks) ? dw[ci * ks + j] : 0.f;
  }
  if (threadIdx.x < Co) {
    chp[threadIdx.x] = pb[threadIdx.x];
    chp[Co + threadIdx.x] = gw[threadIdx.x];
    chp[2 * Co + threadIdx.x] = gb[threadIdx.x];
  }
  // ---- depthwise output of this wave's frames (rows fq of pass p: frame TP p + 16 wave + fq), all input channels; the first PRE channel
  // tiles' MFMAs of pass 0 run while the rows of pass 1 are in flight ----
  constexpr int PRE = 2;
  const int tbase = 16 * wave + 4 * g;
  f4 at[NP][KT];  // A operand: k = input channel 16 kt + 4 g + r
  f4 acc[CT][NP];  // lane (fq, g) of tile t: channel 16 t + fq, frames TP p + 16 wave + 4 g + r
  auto taps = [&](int p) {
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) at[p][kt] = splat(0.f);
    for (int j = 0; j < ks; ++j) {  // Conv1d(padding = k/2), layers/conv.py:33-41; tap loop outermost (see k_dsconv_fused)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ci = 16 * kt + 4 * g + r;
          at[p][kt][r] = fmaf(xs[ci * kDfXld + 16 * wave + fq + j], dws[ci * kDfTapLd + j], at[p][kt][r]);
        }
    }
    if (TP * p + 16 * wave + fq >= To) {  // rows past the last output frame feed zeros: their accumulators stay exactly 0 (see the statistics)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) at[p][kt] = splat(0.f);
    }
  };
  auto chain = [&](int t, int p) {  // one pass of tile t: bias as the accumulator input
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const f4 w = *reinterpret_cast<const f4*>(wsm + (16 * t + fq) * WLD + 16 * kt + 4 * g);  // B operand: column = channel 16 t + fq
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][p] = EDTTS_MFMA(at[p][kt][r], w[r], acc[t][p]);
    }
  };
  rows_park();
  __syncthreads();  // (also covers the weight, tap and per-channel tiles)
  DS_STAMP(12);
  if (TP < To) rows_request(1);
  taps(0);
#pragma unroll
  for (int t = 0; t < PRE; ++t) {
    acc[t][0] = acc[t][1] = splat(0.f);  // (the pointwise bias joins in the statistics and in the epilogue's shift: no accumulator set-up)
    chain(t, 0);
  }
  if (TP < To) {  // (uniform)
    __syncthreads();  // pass 0 has been read
    rows_park();
    __syncthreads();
    taps(1);
#pragma unroll
    for (int t = 0; t < PRE; ++t) chain(t, 1);
  } else {
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) at[1][kt] = splat(0.f);
  }
  DS_STAMP(1);
  const bool two_passes = TP < To;
  auto tile_mfma = [&](int t) {  // two independent accumulator chains (the passes), interleaved
    __builtin_amdgcn_sched_barrier(0);  // (its weight fragments must not be hoisted over the store / statistics code before it: 20 registers)
    acc[t][0] = acc[t][1] = splat(0.f);
    f4 w[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) w[kt] = *reinterpret_cast<const f4*>(wsm + (16 * t + fq) * WLD + 16 * kt + 4 * g);
    if (two_passes) {  // (uniform; ONE branch per tile, not one per MFMA)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc[t][0] = EDTTS_MFMA(at[0][kt][r], w[kt][r], acc[t][0]);
          acc[t][1] = EDTTS_MFMA(at[1][kt][r], w[kt][r], acc[t][1]);
        }
    } else {
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][0] = EDTTS_MFMA(at[0][kt][r], w[kt][r], acc[t][0]);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  // Frames of this lane past To (only when To is not a multiple of the 16-frame rows): their accumulators are exactly 0 (zero A rows), so the
  // sums run over all eight values unmasked and the terms of the invalid frames are taken out again.
  float n_inv = 0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int over = TP * p + tbase + 4 - To;
    n_inv += (float)(over < 0 ? 0 : (over > 4 ? 4 : over));
  }
  // sums over this lane's frames of tile t if the lane's channel belongs to group grp, else 0: z, or (z - m)^2
  // (a lane without any valid frame contributes exactly 0, not the rounding residue of eight bias terms added and taken out again:
  // with T = 1 there are 1 200 such lanes beside 20 values)
  const bool some_valid = n_inv < 8.f;
  float s8[CT];  // this lane's sum over its frames of tile t (taken once per tile: a tile serves two groups)
  auto lane_sum = [&](int t, int grp) {
    const int c = 16 * t + fq;
    return (some_valid && c >= CPG * grp && c < CPG * (grp + 1)) ? s8[t] : 0.f;
  };
  auto lane_sq = [&](int t, int grp, float m) {
    const float mb = m - chp[16 * t + fq];  // z - m = acc - (m - bias); frames past To: acc = 0 exactly
    float sum = -n_inv * mb * mb;
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = acc[t][p][r] - mb;
        sum = fmaf(d, d, sum);
      }
    const int c = 16 * t + fq;
    return (some_valid && c >= CPG * grp && c < CPG * (grp + 1)) ? sum : 0.f;
  };
  // frames of wave w (both passes) inside [0, To)
  auto wave_frames_in = [&](int w) {
    int n = 0;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int left = To - (TP * p + 16 * w);
      n += left < 0 ? 0 : (left > 16 ? 16 : left);
    }
    return n;
  };
  // (reciprocals once: an IEEE divide is ten instructions, and the statistics would run nineteen of them per group)
  const float n_own = (float)(CPG * wave_frames_in(wave));
  const float nw_lane = (float)(CPG * wave_frames_in(fq));  // values of wave fq (see the combine below)
  const float inv_n_own = n_own > 0.f ? 1.0f / n_own : 0.f;
  float mu_g[NG], rs_g[NG];  // (wave-uniform)
  const float inv_n_el = 1.0f / (float)(CPG * To);
  auto store_tile = [&](int t) {
    const int c = 16 * t + fq, gl = 16 * t / CPG, gh = (16 * t + 15) / CPG;
    const bool low = c < CPG * (gl + 1);
    const float mu = low ? mu_g[gl] : mu_g[gh], rs = low ? rs_g[gl] : rs_g[gh];
    const float sc = rs * chp[Co + c], sh = fmaf(chp[c] - mu, sc, chp[2 * Co + c]);  // (acc + bias - mu) rs w + b as one fma per value
    float* yr = y + ((size_t)b * Co + c) * To;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int t0 = TP * p + tbase;
      f4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        o[r] = gelu_as(fmaf(acc[t][p][r], sc, sh));  // F.gelu (erf form), conv.py:64
      }
      if constexpr (VEC) {
        if (t0 < To) stg4(yr + t0, o);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (t0 + r < To) yr[t0 + r] = o[r];
      }
    }
  };
  // (compile-time walk: every tile / group index below is a constant, so the live z tiles and the group statistics stay in registers)
  // Statistics of a group with ONE block-wide exchange: every wave reduces its own frames to (sum, centred squares about its OWN mean),
  // and the sixteen pairs are combined exactly (Chan, Golub & LeVeque: M2 = sum_w M2_w + n_w (mean_w - mean)^2) in a fixed order --
  // as accurate as the reference's two passes.
  dsg_static_for<0, CT>([&](auto tc) {
    constexpr int t = decltype(tc)::value;
    constexpr int gfirst = dsg_first_completing<CPG, NG>(t);  // first group whose last tile is t (-1: none)
    if constexpr (t >= PRE && dsg_first_completing<CPG, NG>(t - 1) < 0) tile_mfma(t);  // (else issued before the walk, or under the previous step's barrier)
    {
      float sum = (8.f - n_inv) * chp[16 * t + fq];  // the bias of this lane's valid frames (frames past To: acc = 0 exactly)
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r) sum += acc[t][p][r];
      s8[t] = sum;
    }
    dsg_static_for<0, NG>([&](auto gc) {
      constexpr int grp = decltype(gc)::value;
      if constexpr ((CPG * grp + CPG - 1) / 16 == t) {  // groups whose last tile is t
        constexpr int t_first = CPG * grp / 16;
        DS_SUB(t, 2);
        float s = 0.f;
        dsg_static_for<t_first, t + 1>([&](auto uc) { s += lane_sum(decltype(uc)::value, grp); });
        s = wave_sum64(s);
        const float m_own = s * inv_n_own;
        DS_SUB(t, 3);
        float s2 = 0.f;
        dsg_static_for<t_first, t + 1>([&](auto uc) { s2 += lane_sq(decltype(uc)::value, grp, m_own); });
        s2 = wave_sum64(s2);
        if (lane == 0) {
          part[(grp * 2 + 0) * WAVES + wave] = m_own;
          part[(grp * 2 + 1) * WAVES + wave] = s2;
        }
        DS_SUB(t, 4);
        if constexpr (t + 1 < CT && t + 1 >= PRE && grp == gfirst) tile_mfma(t + 1);  // the next tile's MFMAs under the barrier
        DS_SUB(t, 5);
        __syncthreads();
        DS_SUB(t, 6);
        // lane fq of every row takes wave fq's pair; two 16-lane DPP sums instead of two 16-term loops in every lane (fixed tree order)
        static_assert(WAVES == 16, "one wave per lane of a DPP row");
        const float mw = part[(grp * 2 + 0) * WAVES + fq], m2w = part[(grp * 2 + 1) * WAVES + fq];
        const float mu = row_sum16(nw_lane * mw) * inv_n_el;
        const float dm = mw - mu;
        const float m2 = row_sum16(fmaf(nw_lane * dm, dm, m2w));
        // (wave-uniform values: into SGPRs, or sixteen VGPRs stay live through the walk)
        mu_g[grp] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(mu)));
        rs_g[grp] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(rsqrtf(m2 * inv_n_el + 1e-5f))));  // GroupNorm eps (torch default), biased variance
      }
    });
    DS_SUB(t, 7);
    // tiles whose last group has just been completed
    dsg_static_for<0, t + 1>([&](auto uc) {
      constexpr int tt = decltype(uc)::value;
      if constexpr ((CPG * ((16 * tt + 15) / CPG) + CPG - 1) / 16 == t) store_tile(tt);
    });
    DS_SUB(t, 8);
    DS_TILE(t);
  });
#ifdef EDTTS_DS_STAMPS
  __builtin_amdgcn_s_waitcnt(0);
  DS_STAMP(13);
  if (threadIdx.x == 0) g_ds_stamps[blockIdx.x * 16 + 15] = __builtin_amdgcn_s_memrealtime();
#endif
}

// =========================================================================================================
// host side
// =========================================================================================================
struct Workspace {
  size_t err, h, q, k, vT, kc, vcT, cond, total;  // offsets in floats (err = 0: the index-error word heads every workspace)
  size_t g_xn, g_big, g_att, g_ctx, g_cr, g_kv, g_eps;  // generic path: norm output, QKV / FFN hidden, attention output, context
                                                       // rows, kv_down rows, per-layer K|V cache, eps before the sampler tail
  int Tp, Sp, VR;
  unsigned* errp;  // where kernels record clamped indices: word 0 of the CALLER's workspace, also for a sub-batch's slice of it
};
// largest frames-per-wave of any fused kernel instance (32; the 16-frame ones split such a tile): the padded length Tp is a
// multiple of it
constexpr int kWaveFrames = 32;

static void make_workspace(const Layout& lo, int B, int T, int S, int cond_rows, Workspace* w) {
  const size_t H = lo.H;
  if (lo.GEN) {  // plain row-major activations, no padding
    memset(w, 0, sizeof(*w));
    w->Tp = T; w->Sp = S; w->VR = lo.H;
    const size_t M = (size_t)B * T, CS = (size_t)B * S, FH = (size_t)lo.FM * H;
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o = align64(o + n); return r; };
    w->err = take(64);
    w->h = take(M * H); w->g_xn = take(M * H); w->g_big = take(M * (FH > 3 * H ? FH : 3 * H)); w->g_att = take(M * H);
    w->g_ctx = take(CS * H); w->g_cr = take(CS * lo.R); w->g_kv = take((size_t)lo.L * CS * 2 * H); w->g_eps = take(M * lo.MEL);
    w->cond = take((size_t)cond_rows * lo.L * 2 * 2 * H + (size_t)cond_rows * H);
    w->total = o;
    w->errp = nullptr;
    return;
  }
  w->Tp = (T + kWaveFrames - 1) / kWaveFrames * kWaveFrames;
  w->Sp = (S + 31) / 32 * 32;
  w->VR = (lo.HEADS - 1) * lo.DH + lo.DHP;
  size_t o = 0;
  auto take = [&](size_t n) { size_t r = o; o = align64(o + n); return r; };
  w->err = take(64);  // word 0: EDTTS_IDX_* bits set by kernels that had to clamp an out-of-range index
  const size_t es = lo.BF16 ? 2 : 1;  // q / k / v^T and the cross cache hold bf16 in the bf16 instance: half the floats
  w->h = take((size_t)B * w->Tp * H);
  w->q = take((size_t)2 * B * w->Tp * H / es);  // two sets each (ping-pong between layers)
  w->k = take((size_t)2 * B * w->Tp * H / es);
  w->vT = take((size_t)2 * B * w->VR * w->Tp / es);
  w->kc = take((size_t)lo.L * B * w->Sp * H / es);
  w->vcT = take((size_t)lo.L * B * w->VR * w->Sp / es);
  w->cond = take((size_t)cond_rows * lo.L * 2 * 2 * H + (size_t)cond_rows * H);  // AdaLN rows + t_cond scratch
  w->total = o;
  w->errp = nullptr;
}

// SIMDs of the current device = waves of the layer kernels in flight at a time (one per SIMD: they need > 256 registers)
// (one cache entry per device ordinal, filled by whichever thread asks first: the value is a property of the device, so a race
// only queries it twice)
static int device_simds() {
  static std::atomic<int> n[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 1024;
  int v = n[dev].load(std::memory_order_relaxed);
  if (!v) {
    int cus = 0;
    v = (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) ? 4 * cus : 1024;
    n[dev].store(v, std::memory_order_relaxed);
  }
  return v;
}

// ---------------------------------------------------------------------------------------------------------
// Sub-batches on several streams.  A layer launch of a large batch is a whole number of rounds of one wave per SIMD, and every
// launch ends with SIMDs idling while the last waves finish (round 3, B=256, T=512: 3.7 % of the kernel, the spread of the
// sum of four wave lifetimes over 1024 SIMDs); the next launch cannot start before, because it reads K / V rows of its
// neighbours.  Utterances are independent, though: the samplers cut a large batch into up to kMaxSub sub-batches (substreams_for)
// that walk the same launch sequence on one stream each (the caller's and library-owned ones, forked and joined with events:
// capturable), so one sub-batch's waves fill the SIMDs another's finishing launch leaves idle.  Each sub-batch is an ordinary call on
// its own slice of the caller's workspace; results do not depend on the cut (every utterance is computed alone, bitwise).
// ---------------------------------------------------------------------------------------------------------
constexpr int kMaxSub = 8;
struct SubBatches {
  int n;                 // number of sub-batches: 1 (no cut) .. kMaxSub
  int B[kMaxSub], off[kMaxSub];
  Workspace ws[kMaxSub];
  size_t base[kMaxSub];  // float offset of slice j in the caller's workspace
  size_t cond;           // float offset of the conditioning rows (shared by the slices)
  size_t total;          // floats
};
static std::atomic<int> g_coop{[] { const char* e = getenv("EDTTS_COOP"); return e ? atoi(e) : -1; }()};
static std::atomic<int> g_substreams{[] { const char* e = getenv("EDTTS_SUBSTREAMS"); const int v = e ? atoi(e) : 4; return v < 1 ? 1 : (v > kMaxSub ? kMaxSub : v); }()};
// The two run-time switches as one call sees them.  edtts_set_* may run on any thread at any time; every entry point that plans or
// launches a decoder takes ONE snapshot (a Settings object on its stack) and everything below it -- the cut, the workspace slices,
// the kernel choice of every step -- reads the snapshot, so a call never mixes two settings.
struct Settings {
  int substreams, coop;
};
static thread_local const Settings* t_settings = nullptr;
struct SettingsScope {
  Settings snap;
  const Settings* prev;
  SettingsScope() : snap{g_substreams.load(std::memory_order_relaxed), g_coop.load(std::memory_order_relaxed)}, prev(t_settings) {
    t_settings = &snap;
  }
  ~SettingsScope() { t_settings = prev; }
};
static Settings current_settings() {
  return t_settings ? *t_settings : Settings{g_substreams.load(std::memory_order_relaxed), g_coop.load(std::memory_order_relaxed)};
}

static void plan_sub(const Layout& lo, int B, int T, int S, int cond_rows, int n, SubBatches* sb) {
  sb->n = n;
  if (n == 1) {
    make_workspace(lo, B, T, S, cond_rows, &sb->ws[0]);
    sb->B[0] = B; sb->off[0] = 0; sb->base[0] = 0; sb->cond = sb->ws[0].cond; sb->total = sb->ws[0].total;
    return;
  }
  size_t o = 0;
  int off = 0;
  for (int j = 0; j < n; ++j) {
    sb->B[j] = B / n + (j < B % n ? 1 : 0);
    sb->off[j] = off;
    off += sb->B[j];
    make_workspace(lo, sb->B[j], T, S, 1, &sb->ws[j]);
    sb->base[j] = o;
    o += sb->ws[j].total;
  }
  sb->cond = o;
  sb->total = align64(o + (size_t)cond_rows * lo.L * 2 * 2 * lo.H + (size_t)cond_rows * lo.H);
}
// The cut a sampler call makes: as many sub-batches (at most g_substreams) as still leave each one TWO rounds of waves -- measured:
// B=256, T=1024 bf16 (8 rounds) 33.0 ms at two, 31.8 at four, 32.7 at six, 33.0 at eight; B=512, T=512 fp32 (8 rounds) 30.37 at two,
// 30.31 at four; B=256, T=512 fp32 (4 rounds) the same at two and four -- but two halves of ONE round each where the batch has only two
// rounds (B=128, T=512 fp32: 7.88 ms in one piece, 7.74 cut).
static int substreams_for(const Layout& lo, int B, int T, int S) {
  if (lo.GEN) return 1;  // the generic path runs on the caller's stream alone: a captured graph has no parallel branches
  Workspace w;
  make_workspace(lo, 1, T, S, 1, &w);
  const long waves = (long)B * (w.Tp / 32), slots = device_simds();
  const int max_sub = current_settings().substreams;
  if (max_sub < 2 || B < 2 || waves < 2 * slots) return 1;
  long n = waves / (2 * slots);
  if (n < 2) n = 2;
  if (n > max_sub) n = max_sub;
  if (n > B) n = B;
  return (int)n;
}
static void plan_call(const Layout& lo, int B, int T, int S, int cond_rows, float* wsb, SubBatches* sb) {
  plan_sub(lo, B, T, S, cond_rows, substreams_for(lo, B, T, S), sb);
  for (int j = 0; j < sb->n; ++j) sb->ws[j].errp = reinterpret_cast<unsigned*>(wsb);
}

// Side streams: one set per (device, caller stream) and thread, so that two caller streams -- on one thread or on two -- never
// share a side stream or an event (a shared set would chain one caller's sub-batches behind another's, and a capture on one caller
// stream would pull the other's work into its graph).  A thread keeps at most kSideSets sets and reuses the least recently used
// one for a new caller stream; at thread exit its sets go to a process-wide pool that the next thread draws from, so a server
// that starts a thread per request does not create streams without bound.  (No HIP call at thread exit: the sets are handed
// over, not destroyed.)
struct SideStream {
  int dev = -1;                    // device the streams and events belong to (-1: nothing created yet)
  hipStream_t caller = nullptr;    // caller stream the set serves (valid when bound)
  bool bound = false;
  unsigned long long last_use = 0;
  hipStream_t s[kMaxSub - 1] = {};
  hipEvent_t fork = nullptr, join[kMaxSub - 1] = {};
};
constexpr int kSideSets = 8;
static std::mutex g_side_pool_mu;
static std::vector<SideStream>& side_pool() {
  static auto* pool = new std::vector<SideStream>;  // (never destroyed: a thread may exit after static destruction began)
  return *pool;
}
struct ThreadSides {
  SideStream set[kSideSets];
  unsigned long long tick = 0;
  ~ThreadSides() {
    std::lock_guard<std::mutex> lock(g_side_pool_mu);
    for (SideStream& sd : set)
      if (sd.dev >= 0) release(sd);
  }
  static void release(SideStream& sd) {  // (caller holds g_side_pool_mu)
    sd.bound = false;
    side_pool().push_back(sd);
    sd = SideStream();
  }
  SideStream& get(int dev, hipStream_t caller) {
    SideStream* pick = nullptr;
    for (SideStream& sd : set) {
      if (sd.bound && sd.dev == dev && sd.caller == caller) { pick = &sd; break; }
      if (!pick || (pick->bound && (!sd.bound || sd.last_use < pick->last_use))) pick = &sd;
    }
    if (!(pick->bound && pick->dev == dev && pick->caller == caller)) {
      if (pick->dev != dev) {  // streams of another device (or none): trade them for a pooled set of this device, if any
        std::lock_guard<std::mutex> lock(g_side_pool_mu);
        if (pick->dev >= 0) release(*pick);
        auto& pool = side_pool();
        for (size_t i = 0; i < pool.size(); ++i)
          if (pool[i].dev == dev) {
            *pick = pool[i];
            pool.erase(pool.begin() + (long)i);
            break;
          }
      }
      pick->caller = caller;
      pick->bound = true;
    }
    pick->last_use = ++tick;
    return *pick;
  }
};
static thread_local ThreadSides g_sides;
// RAII: fork the side streams off the caller's stream, join them back when the call returns (also on its error paths, so that a
// stream capture is never left with a dangling branch).  Every stream and event is created BEFORE the fork is recorded, and `n`
// counts the side streams that have been forked so far, so that the destructor joins exactly those.
struct ForkJoin {
  hipStream_t st[kMaxSub];
  SideStream* side = nullptr;
  int n = 1;
  int init(const SubBatches& sb, hipStream_t main) {
    for (int j = 0; j < kMaxSub; ++j) st[j] = main;
    if (sb.n < 2) return EDTTS_OK;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(EDTTS_ERR_UNSUPPORTED, "device ordinal %d out of range", dev);
    SideStream& sd = g_sides.get(dev, main);
    sd.dev = dev;
    if (!sd.fork) HIP_TRY(hipEventCreateWithFlags(&sd.fork, hipEventDisableTiming));
    for (int j = 0; j + 1 < sb.n; ++j) {
      if (!sd.s[j]) HIP_TRY(hipStreamCreateWithFlags(&sd.s[j], hipStreamNonBlocking));
      if (!sd.join[j]) HIP_TRY(hipEventCreateWithFlags(&sd.join[j], hipEventDisableTiming));
    }
    HIP_TRY(hipEventRecord(sd.fork, main));
    side = &sd;
    for (int j = 0; j + 1 < sb.n; ++j) {
      HIP_TRY(hipStreamWaitEvent(sd.s[j], sd.fork, 0));
      st[j + 1] = sd.s[j];
      n = j + 2;
    }
    return EDTTS_OK;
  }
  ~ForkJoin() {
    if (side)
      for (int j = 0; j + 1 < n; ++j) {
        (void)hipEventRecord(side->join[j], side->s[j]);
        (void)hipStreamWaitEvent(st[0], side->join[j], 0);
      }
  }
};

// Philox stream ids (the `step` word of the counter) are split into disjoint domains so that no two draws of one seed can meet
// (include/edtts.h, "Philox stream ids"): [0, 0x10000) belongs to edtts_randn callers, the samplers' per-step draws live above it.
constexpr unsigned kStreamDdpmStep = 0x10000u;     // + step index: ancestral noise of edtts_sample_ddpm
constexpr unsigned kStreamInpaintStep = 0x20000u;  // + step index: q_sample noise of edtts_sample_inpaint's known frames
struct DdpmStepArgs {
  const float* noise;
  unsigned long long seed, base;
  unsigned step;  // stream id (kStreamDdpmStep + step index)
};
struct VpredStepArgs {
  VpredCoef k;
  const float* v_uncond;
};
struct LmsStepArgs {
  LmsCoef k;
  const float *h_new, *h_old;
  float *x0_hist, *x0_all;
};
struct BlendStepArgs {  // TAIL_VLMS: the known frames' q_sample for the next step (k_inpaint_inject's arguments); known = null: none
  const float *known, *noise;
  int frames, mel;
  float c_known, c_noise;
  unsigned long long seed;
  const unsigned long long* seeds;
  unsigned step;  // stream id (kStreamInpaintStep + the next step's index)
};
// What the last layer of a decoder forward does with its output: return eps (TAIL_EPS) or take one sampler step
struct StepTail {
  int kind = TAIL_EPS;
  float* eps = nullptr;         // TAIL_EPS: the decoder output
  float* x_prev = nullptr;      // every sampler kind: the updated sample
  float* x0 = nullptr;          // TAIL_DDIM: the x0 prediction
  const float* coef = nullptr;  // TAIL_DDIM: 4 scalars, TAIL_DDPM: 3
  DdpmStepArgs ddpm{};
  LmsStepArgs lms{};
  VpredStepArgs vp{};  // (TAIL_VLMS reads its cfg and v_uncond, and lms)
  BlendStepArgs blend{};
};
static void set_tail_args(const StepTail& t, KArgs* a) {
  if (t.kind == TAIL_EPS) {
    a->eps = t.eps;
    return;
  }
  a->x_prev = t.x_prev;
  if (t.kind == TAIL_LMS || t.kind == TAIL_VLMS) {
    a->lms = t.lms.k; a->h_new = t.lms.h_new; a->h_old = t.lms.h_old; a->x0_hist = t.lms.x0_hist; a->x0_all = t.lms.x0_all;
    if (t.kind == TAIL_LMS) return;
    a->vp = t.vp.k; a->v_uncond = t.vp.v_uncond;
    a->known = t.blend.known; a->noise = t.blend.noise; a->inj_frames = t.blend.frames; a->inj_mel = t.blend.mel;
    a->p_coef1 = t.blend.c_known; a->p_coef2 = t.blend.c_noise; a->seed = t.blend.seed; a->seeds = t.blend.seeds; a->step = t.blend.step;
  } else if (t.kind == TAIL_VPRED) {
    a->vp = t.vp.k; a->v_uncond = t.vp.v_uncond;
  } else if (t.kind == TAIL_DDPM) {
    a->p_coef1 = t.coef[0]; a->p_coef2 = t.coef[1]; a->p_sd = t.coef[2];
    a->noise = t.ddpm.noise; a->seed = t.ddpm.seed; a->philox_base = t.ddpm.base; a->step = t.ddpm.step;
  } else {
    a->x0 = t.x0;
    a->c_s1m = t.coef[0]; a->c_sab = t.coef[1]; a->c_sabp = t.coef[2]; a->c_dir = t.coef[3];
  }
}
// f(std::integral_constant<int, TAIL_*>) for the run-time tail kind: picks the kernel instance of that kind
template <class F>
static int with_tail(int kind, F&& f) {
  switch (kind) {
    case TAIL_QKV: return f(std::integral_constant<int, TAIL_QKV>{});
    case TAIL_EPS: return f(std::integral_constant<int, TAIL_EPS>{});
    case TAIL_LMS: return f(std::integral_constant<int, TAIL_LMS>{});
    case TAIL_DDPM: return f(std::integral_constant<int, TAIL_DDPM>{});
    case TAIL_VPRED: return f(std::integral_constant<int, TAIL_VPRED>{});
    case TAIL_VLMS: return f(std::integral_constant<int, TAIL_VLMS>{});
    default: return f(std::integral_constant<int, TAIL_DDIM>{});
  }
}
// ... and its kin for the other run-time values that name a kernel instance:
// f(std::bool_constant<b>) for a run-time flag
template <class F>
static int with_flag(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
// f(Elem<float>) or f(Elem<__bf16>) for the element type of a buffer (bf16: whether it holds __bf16)
template <class T>
struct Elem {
  using type = T;
};
template <class F>
static int with_elem(bool bf16, F&& f) {
  return bf16 ? f(Elem<__bf16>{}) : f(Elem<float>{});
}
// f(std::integral_constant<int, DT>) for DT = ceil(head_dim / 16) in 1 .. MAX: the smallest head-dim tile count that holds the head
template <int MAX, int DT = 1, class F>
static int with_head_tiles(int head_dim, F&& f) {
  if constexpr (DT > MAX) {
    return fail(EDTTS_ERR_UNSUPPORTED, "generic kernels: head_dim=%d > %d", head_dim, 16 * MAX);
  } else {
    if ((head_dim + 15) / 16 == DT) return f(std::integral_constant<int, DT>{});
    return with_head_tiles<MAX, DT + 1>(head_dim, f);
  }
}
#define TRY_G(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)
// ... for every kind (the hipFuncSetAttribute lists)
template <class F>
static int for_each_tail(F&& f) {
  for (int kind : {TAIL_QKV, TAIL_EPS, TAIL_DDIM, TAIL_DDPM, TAIL_LMS, TAIL_VPRED, TAIL_VLMS}) TRY_G(with_tail(kind, f));
  return EDTTS_OK;
}
// per-utterance frame / token counts of a (sub-)batch: device int64 [B] each, or null (edtts_*_len)
struct Lens {
  const int64_t *t = nullptr, *s = nullptr;
  bool t_dbl = false;  // t holds token counts (frames = 2 x tokens)
  Lens at(int off) const { return Lens{t ? t + off : nullptr, s ? s + off : nullptr, t_dbl}; }
};
// What every launch of one (sub-)batch shares: shapes, weights, its workspace slice, lengths and stream
struct CallCtx {
  const Layout& lo;
  const float* blob;
  Workspace ws;
  float* wsb;  // base of the (sub-)batch's workspace slice
  int B, T, S, window;
  Lens ln;
  hipStream_t st;
};

#ifdef EDTTS_STAMPS
static unsigned long long* g_stamps_fwd = nullptr;  // diagnostic builds only, see edtts_debug_set_stamps
#endif
#ifdef EDTTS_WAVELOG
static unsigned long long* g_wavelog = nullptr;  // diagnostic builds only: [layer launches of ONE forward][8192 waves][6]
static thread_local int g_wavelog_base = 0;       // first wave index of the sub-batch being launched
#endif

// CtxArgs of a context-cache launch (fp32 and bf16 instances)
static CtxArgs ctx_args(const CallCtx& c, const int64_t* sem_idx, const float* sem_feat) {
  const Layout& lo = c.lo;
  CtxArgs a;
  memset(&a, 0, sizeof(a));
  a.B = c.B; a.S = c.S; a.Sp = c.ws.Sp; a.L = lo.L; a.SD = lo.SD; a.n_tok = lo.NTOK; a.max_cpos = lo.MAXCPOS;
  a.sem_idx = sem_idx; a.sem_feat = sem_feat; a.s_len = c.ln.s;
  a.tok = c.blob + lo.tok; a.semp = c.blob + lo.semp; a.semp_b = c.blob + lo.semp_b; a.cpe = c.blob + lo.cpe; a.blob = c.blob;
  for (int l = 0; l < lo.L; ++l) {
    a.kvd[l] = (unsigned)lo.layer[l].kvd; a.kvn[l] = (unsigned)lo.layer[l].kvn; a.kvu[l] = (unsigned)lo.layer[l].kvu;
  }
  a.kc = c.wsb + c.ws.kc; a.vcT = c.wsb + c.ws.vcT;
  a.err = c.ws.errp ? c.ws.errp : reinterpret_cast<unsigned*>(c.wsb + c.ws.err);
  return a;
}

// KArgs of one forward of the fused kernels (fp32 and bf16 instances).  ES: element size of the q / k / v^T sets and the cross cache
// in floats' halves -- the bf16 instance holds bf16 there, half as many floats.
template <int ES>
struct ForwardArgs {
  KArgs a;
  const CallCtx& c;
  size_t qk_set, v_set;  // floats per q / k set and per v^T set
  ForwardArgs(const CallCtx& c_, const float* x, const float* cond_row, int cond_bstride) : c(c_) {
    const Layout& lo = c.lo;
    const float* blob = c.blob;
    memset(&a, 0, sizeof(a));
    a.B = c.B; a.T = c.T; a.Tp = c.ws.Tp; a.S = c.S; a.Sp = c.ws.Sp; a.window = c.window; a.max_pos = lo.MAXPOS;
    a.max_cpos = lo.MAXCPOS; a.n_tok = lo.NTOK; a.SD = lo.SD; a.L = lo.L; a.ffn_tiles = lo.FM * lo.HT;
    a.h = c.wsb + c.ws.h;
    a.inp = blob + lo.inp; a.inp_b = blob + lo.inp_b; a.pe = blob + lo.pe;
    a.fnw = blob + lo.fnw; a.fnb = blob + lo.fnb; a.outp_b = blob + lo.outp_b;
#ifdef EDTTS_STAMPS
    {
      auto env = [](const char* n, int d) { const char* e = getenv(n); return e ? atoi(e) : d; };
      a.diag_skip = env("EDTTS_STAMP_HEAD", 1) | (env("EDTTS_STAMP_WAVE", 0) << 8) | (env("EDTTS_STAMP_BLOCK", 8) << 16);
    }
#endif
    a.x = x; a.cond = cond_row; a.cond_bstride = cond_bstride;
    a.t_len = c.ln.t; a.s_len = c.ln.s; a.t_dbl = c.ln.t_dbl;
    qk_set = (size_t)c.B * c.ws.Tp * lo.H / ES;
    v_set = (size_t)c.B * c.ws.VR * c.ws.Tp / ES;
    set_qkv(1, 0);  // the prologue writes set 0
    a.n1w = blob + lo.layer[0].n1w; a.stream = blob + lo.inp; a.layer = 0;  // stream: inp | qkv(0)
  }
  void set_qkv(int in_set, int out_set) {
    const Workspace& ws = c.ws;
    a.q = c.wsb + ws.q + in_set * qk_set; a.k = c.wsb + ws.k + in_set * qk_set; a.vT = c.wsb + ws.vT + in_set * v_set;
    a.q_out = c.wsb + ws.q + out_set * qk_set; a.k_out = c.wsb + ws.k + out_set * qk_set; a.vT_out = c.wsb + ws.vT + out_set * v_set;
  }
  // layer l's fields; returns the tail kind of its launch (TAIL_QKV but for the last layer)
  int layer(int l, const StepTail& tail) {
    const Layout& lo = c.lo;
    const LayerLayout& y = lo.layer[l];
    a.layer = l;
    set_qkv(l & 1, (l + 1) & 1);  // layer l reads set l%2 and its QKV tail writes set (l+1)%2
    a.proj_b = c.blob + y.proj_b; a.n2w = c.blob + y.n2w; a.n3w = c.blob + y.n3w; a.up_b = c.blob + y.up_b;
    a.down_b = c.blob + y.down_b; a.stream = c.blob + y.s_body;
    a.kc = c.wsb + c.ws.kc + (size_t)l * c.B * c.ws.Sp * lo.H / ES;
    a.vcT = c.wsb + c.ws.vcT + (size_t)l * c.B * c.ws.VR * c.ws.Sp / ES;
#ifdef EDTTS_WAVELOG
    a.stamps = g_wavelog ? g_wavelog + (size_t)6 * 8192 * l : nullptr;
    a.diag_skip = g_wavelog_base;
#endif
#ifdef EDTTS_STAMPS
    a.stamps = g_stamps_fwd ? g_stamps_fwd + 128 * l : nullptr;
#endif
    if (l + 1 < lo.L) {
      a.n1w = c.blob + lo.layer[l + 1].n1w;
      return TAIL_QKV;
    }
    set_tail_args(tail, &a);
    return tail.kind;
  }
};

// kernels with > 64 KiB of dynamic LDS need the opt-in attribute: LN::set_attrs() once per device
// (one flag per device ordinal, so that a process driving several GPUs opts in on each)
template <class LN>
static int set_attrs_once() {
  static std::atomic<bool> done[64];  // (two threads may both set the attributes: hipFuncSetAttribute is idempotent)
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return fail(EDTTS_ERR_UNSUPPORTED, "device ordinal %d out of range", dev);
  if (done[dev].load(std::memory_order_acquire)) return EDTTS_OK;
  TRY_G(LN::set_attrs());
  done[dev].store(true, std::memory_order_release);
  return EDTTS_OK;
}

template <class C>
struct Launcher {
  // One wave of these kernels per SIMD, on EVERY CU: an instance that needs fewer than 257 registers (the 16-frames-per-wave ones
  // after round 3's register savings: 232) would otherwise be packed two waves per SIMD onto HALF of the CUs by the dispatcher
  // (measured: B=32, T=512 at 0.232 ms per layer launch instead of 0.155).  Every launch therefore claims a quarter of the CU's
  // 160 KiB of LDS per wave, whether it uses it or not.
  static size_t occupancy_lds() { return (size_t)C::WAVES * 40 * 1024; }
  static size_t ring_lds() { return occupancy_lds(); }
  template <class CC> static size_t stash_lds() { return (size_t)CC::WAVES * CC::HT * CC::NF * 1024; }  // residual parking place
  static size_t layer_lds() {
    const size_t need = stash_lds<C>() + (C::Q_IN_LDS ? (size_t)C::WAVES * C::WF * C::H * sizeof(float) : 0);
    return need > occupancy_lds() ? need : occupancy_lds();
  }
  static int grid(int B, int Tp) { return (B * (Tp / C::WF) + C::WAVES - 1) / C::WAVES; }
  static int ctx_grid(int B, int Sp) { return (B * (Sp / 32) + kCtxWaves - 1) / kCtxWaves; }
  using C2 = Cfg<C::H, C::HEADS, C::MEL, 2>;  // geometry of the context kernel
  // the 16-frames-per-wave instance for small grids (built for the default decoder)
  static constexpr bool HAS_SMALL = C::NF == 2 && (C::H == 160 || C::H == 256);
  using Small = Cfg<C::H, C::HEADS, C::MEL, 1>;
  // one wave of these kernels fills a SIMD (> 256 registers): the device runs 4 * #CUs of them at a time (1024 on an MI355X)
  static int wave_slots() { return device_simds(); }

  static int ctx(const CallCtx& c, const int64_t* sem_idx, const float* sem_feat) {
    const CtxArgs a = ctx_args(c, sem_idx, sem_feat);
    // one block per token tile group walks all layers -- unless that leaves most of the chip idle (B = 1: one block): then the
    // layers of a tile go to separate blocks
    const int gx = ctx_grid(c.B, c.ws.Sp);
    const int gy = (gx * 4 <= wave_slots() / 4) ? c.lo.L : 1;
    hipLaunchKernelGGL(k_ctx<C2>, dim3(gx, gy), dim3(64 * kCtxWaves), 0, c.st, a);
    LAUNCH_CHECK("k_ctx");
    return EDTTS_OK;
  }

  // The cooperative layer kernel (edtts_coop.h: W waves per frame tile) serves the grids that leave SIMDs idle; compiled for the
  // default decoder.  Which instance, by the number t32 of 32-frame tiles against the device's SIMD count (bitwise the same results
  // in every case):
  //     8 t32 <= SIMDs   16-frame tiles, four waves each      (B = 1, T = 256: 64 waves instead of 16)
  //     4 t32 <= SIMDs   32-frame tiles, four waves each
  //     2 t32 <= SIMDs   32-frame tiles, two waves each       (B = 32, T = 512: 1024 waves that keep k_layer's 8 MFMAs per fragment)
  //     else             k_layer, one wave per 32-frame tile
  static constexpr bool HAS_COOP = C::NF == 2 && ((C::H == 160 && C::HEADS == 4) || (C::H == 256 && C::HEADS == 8)) && C::MEL == 80;
  static constexpr bool HAS_CO22 = HAS_COOP && Coop<C, 2>::FITS;
  static int coop_choice(int B, int Tp) {  // 0: none; 14: NF 1, W 4; 24: NF 2, W 4; 22: NF 2, W 2
    int co = current_settings().coop;  // (edtts_set_coop: 0 switches the cooperative kernel off, 14 / 24 / 22 force an instance)
    if (co < 0) {
      const int t32 = B * (Tp / 32), slots = wave_slots();
      co = 8 * t32 <= slots ? 14 : (4 * t32 <= slots ? 24 : (2 * t32 <= slots ? 22 : 0));
    }
    return (co == 22 && !HAS_CO22) ? 0 : co;
  }
  // one decoder forward given conditioning rows + context cache already in the workspace
  template <int COW = 0>
  static int forward(const CallCtx& c, const float* x, const float* cond_row, int cond_bstride, const StepTail& tail) {
    if constexpr (HAS_COOP && COW == 0) {
      const int co = coop_choice(c.B, c.ws.Tp);
      if (co == 14) return Launcher<Small>::template forward<4>(c, x, cond_row, cond_bstride, tail);
      if (co == 24) return forward<4>(c, x, cond_row, cond_bstride, tail);
      if constexpr (HAS_CO22) {
        if (co == 22) return forward<2>(c, x, cond_row, cond_bstride, tail);
      }
    }
    // Small grids: with 32 frames per wave fewer waves than SIMDs would be launched (B = 32 at T = 512: 512 waves for 1024 SIMDs;
    // B = 1: 8) -- the 16-frames-per-wave instance doubles the number of waves.  Same arithmetic per frame, bitwise.
    if constexpr (HAS_SMALL && COW == 0) {
      if (2 * c.B * (c.ws.Tp / C::WF) <= wave_slots())  // ... as long as the doubled wave count still runs in one round
        return Launcher<Small>::template forward<0>(c, x, cond_row, cond_bstride, tail);
    }
    ForwardArgs<1> f(c, x, cond_row, cond_bstride);
    const KArgs& a = f.a;
    const hipStream_t st = c.st;
    const int g = grid(c.B, c.ws.Tp);
    if constexpr (COW != 0) {
      hipLaunchKernelGGL((k_prologue_co<C, COW>), dim3(c.B * (c.ws.Tp / C::WF)), dim3(64 * COW), C::HT * C::NF * 1024, st, a);
    } else {
      hipLaunchKernelGGL(k_prologue<C>, dim3(g), dim3(C::THREADS), ring_lds(), st, a);
    }
    LAUNCH_CHECK("k_prologue");
    for (int l = 0; l < c.lo.L; ++l) {
      TRY_G(with_tail(f.layer(l, tail), [&](auto t) -> int {
        constexpr int TL = decltype(t)::value;
        if constexpr (COW != 0) {
          using CO = Coop<C, COW>;
          const int tiles = c.B * (c.ws.Tp / C::WF);
          PROF_LAUNCH(st, hipLaunchKernelGGL((k_layer_co<C, TL, COW>), dim3((tiles + CO::TILES - 1) / CO::TILES), dim3(CO::THREADS), CO::LDS_BYTES, st, a));
        } else {
          PROF_LAUNCH(st, hipLaunchKernelGGL((k_layer<C, TL>), dim3(g), dim3(C::THREADS), layer_lds(), st, a));
        }
        LAUNCH_CHECK("k_layer");
        return EDTTS_OK;
      }));
    }
    return EDTTS_OK;
  }

  static int set_attrs() {  // (through set_attrs_once)
    if constexpr (HAS_SMALL) TRY_G(Launcher<Small>::set_attrs());
    const int lds = (int)layer_lds();
    HIP_TRY(hipFuncSetAttribute((const void*)k_prologue<C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ring_lds()));
    return for_each_tail([&](auto t) -> int {
      constexpr int TL = decltype(t)::value;
      HIP_TRY(hipFuncSetAttribute((const void*)k_layer<C, TL>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      if constexpr (HAS_COOP) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_layer_co<Small, TL, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, Coop<Small, 4>::LDS_BYTES));
        HIP_TRY(hipFuncSetAttribute((const void*)k_layer_co<C, TL, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, Coop<C, 4>::LDS_BYTES));
        if constexpr (HAS_CO22)
          HIP_TRY(hipFuncSetAttribute((const void*)k_layer_co<C, TL, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, Coop<C, 2>::LDS_BYTES));
      }
      return EDTTS_OK;
    });
  }
};

// ---- bf16 instance (edtts_bf16.h) ----------------------------------------------------------------------------
// frame tiles per wave of the hidden-256 bf16 instance: 2 = four waves per block, 1 = eight (two per SIMD)
constexpr int kNF16 = 2;
template <class C>
struct Launcher16 {
  static int grid(int B, int Tp) { return (B * (Tp / C::WF) + C::WAVES - 1) / C::WAVES; }
  // Small grids: the 16-frames-per-wave instance (two independent four-wave blocks per CU, bitwise the same results) when the
  // 32-frame waves would leave half of the SIMDs without one (B * T <= 16 k frames on an MI355X).
  static constexpr bool HAS_SMALL = C::NF == 2 && C::H == 256;
  using Small = edtts16::Cfg16<C::H, C::HEADS, C::MEL, 1>;
  static int simds() { return device_simds(); }
  static int set_attrs() {  // the weight ring takes > 64 KiB of dynamic LDS (through set_attrs_once)
    if constexpr (HAS_SMALL) TRY_G(Launcher16<Small>::set_attrs());
    const int lds = C::LDS_BYTES;
    HIP_TRY(hipFuncSetAttribute((const void*)edtts16::k_prologue16<C>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    if constexpr (C::NF == 2) HIP_TRY(hipFuncSetAttribute((const void*)k_ctx16<C>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return for_each_tail([&](auto t) -> int {
      HIP_TRY(hipFuncSetAttribute((const void*)edtts16::k_layer16<C, decltype(t)::value>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      return EDTTS_OK;
    });
  }
  static int ctx(const CallCtx& c, const int64_t* sem_idx, const float* sem_feat) {
    if constexpr (C::NF == 2) {  // (the context cache is always built by the 32-token-per-wave launcher)
      CtxArgs a = ctx_args(c, sem_idx, sem_feat);
      a.stream16 = c.blob + c.lo.s_ctx16;
      hipLaunchKernelGGL((k_ctx16<C>), dim3((c.B * (c.ws.Sp / 32) + C::WAVES - 1) / C::WAVES), dim3(C::THREADS), C::LDS_BYTES, c.st, a);
      LAUNCH_CHECK("k_ctx16");
      return EDTTS_OK;
    } else {
      return fail(EDTTS_ERR_UNSUPPORTED, "internal: context cache requested from the 16-frame launcher");
    }
  }
  static int forward(const CallCtx& c, const float* x, const float* cond_row, int cond_bstride, const StepTail& tail) {
    if constexpr (HAS_SMALL) {
      if (2 * c.B * (c.ws.Tp / C::WF) <= simds())  // (round 4: forced at B = 256, T = 1024 it runs 49.2 ms per call against 33.6)
        return Launcher16<Small>::forward(c, x, cond_row, cond_bstride, tail);
    }
    ForwardArgs<2> f(c, x, cond_row, cond_bstride);
    const KArgs& a = f.a;
    const hipStream_t st = c.st;
    const int g = grid(c.B, c.ws.Tp);
    hipLaunchKernelGGL(edtts16::k_prologue16<C>, dim3(g), dim3(C::THREADS), C::LDS_BYTES, st, a);
    LAUNCH_CHECK("k_prologue16");
    for (int l = 0; l < c.lo.L; ++l) {
      TRY_G(with_tail(f.layer(l, tail), [&](auto t) -> int {
        PROF_LAUNCH(st, hipLaunchKernelGGL((edtts16::k_layer16<C, decltype(t)::value>), dim3(g), dim3(C::THREADS), C::LDS_BYTES, st, a));
        LAUNCH_CHECK("k_layer16");
        return EDTTS_OK;
      }));
    }
    return EDTTS_OK;
  }
};

#include "edtts_generic.h"

// compiled decoder shapes: (hidden, heads, n_mels).  EDTTS_FUSED_CHAIN(lo, MISS16, MISS32, body) runs `body` with LN = the fused
// launcher of lo's shape, or the statement MISS16 / MISS32 when none is compiled; EDTTS_DISPATCH adds the generic launcher (lo.GEN)
// and has_instance() -- the predicate make_layout decides EDTTS_KERNELS_AUTO with -- walks the same chain.
#ifdef EDTTS_FAST_BUILD  // scratch builds (-DEDTTS_EXPERIMENTS): the default decoder's fp32 instance only
#define EDTTS_FUSED_CHAIN(lo, MISS16, MISS32, ...)                                                       \
    if (!(lo).BF16 && (lo).H == 160 && (lo).HEADS == 4 && (lo).MEL == 80) { using LN = Launcher<Cfg<160, 4, 80>>; __VA_ARGS__; } \
    else if ((lo).BF16) { MISS16; }                                                                      \
    else { MISS32; }
static int no_instance16(const Layout&) { return fail(EDTTS_ERR_UNSUPPORTED, "EDTTS_FAST_BUILD: only the 160/4/80 fp32 instance is compiled"); }
static int no_instance32(const Layout&) { return fail(EDTTS_ERR_UNSUPPORTED, "EDTTS_FAST_BUILD: only the 160/4/80 fp32 instance is compiled"); }
#else
// Further fp32 shapes are a BUILD option, not a source edit: EDTTS_INSTANCES="192x6x80,128x4x80" in the environment of
// __graft_entry__.build() becomes -DEDTTS_EXTRA_INSTANCES(lo,...)=EDTTS_X(lo,192,6,80,__VA_ARGS__)... (hidden % 32 == 0, head_dim % 16
// in {0, 8}, n_mels % 16 == 0; the build's no-scratch gate rejects a shape whose tiles do not fit the register file).
#ifndef EDTTS_EXTRA_INSTANCES
#define EDTTS_EXTRA_INSTANCES(lo, ...)
#define EDTTS_EXTRA_NAMES ""
#endif
// ... and bf16 shapes (head_dim 32, hidden % 64 == 0: the bf16 kernels identify a head with one 32-wide k-tile): EDTTS_INSTANCES_BF16
#ifndef EDTTS_EXTRA_INSTANCES16
#define EDTTS_EXTRA_INSTANCES16(lo, ...)
#define EDTTS_EXTRA_NAMES16 ""
#endif
#define EDTTS_X16(lo, HH, HD, MM, ...) else if ((lo).H == HH && (lo).HEADS == HD && (lo).MEL == MM) { using LN = Launcher16<edtts16::Cfg16<HH, HD, MM>>; __VA_ARGS__; }
#define EDTTS_X(lo, HH, HD, MM, ...) else if ((lo).H == HH && (lo).HEADS == HD && (lo).MEL == MM) { using LN = Launcher<Cfg<HH, HD, MM>>; __VA_ARGS__; }
#define EDTTS_FUSED_CHAIN(lo, MISS16, MISS32, ...)                                                       \
    if ((lo).BF16) {                                                                                     \
      if ((lo).H == 256 && (lo).HEADS == 8 && (lo).MEL == 80) { using LN = Launcher16<edtts16::Cfg16<256, 8, 80, kNF16>>; __VA_ARGS__; } \
      else if ((lo).H == 64 && (lo).HEADS == 2 && (lo).MEL == 80) { using LN = Launcher16<edtts16::Cfg16<64, 2, 80>>; __VA_ARGS__; } \
      EDTTS_EXTRA_INSTANCES16(lo, __VA_ARGS__)                                                           \
      else { MISS16; }                                                                                   \
    }                                                                                                    \
    else if ((lo).H == 160 && (lo).HEADS == 4 && (lo).MEL == 80) { using LN = Launcher<Cfg<160, 4, 80>>; __VA_ARGS__; } \
    else if ((lo).H == 256 && (lo).HEADS == 8 && (lo).MEL == 80) { using LN = Launcher<Cfg<256, 8, 80>>; __VA_ARGS__; }     \
    else if ((lo).H == 32 && (lo).HEADS == 2 && (lo).MEL == 80) { using LN = Launcher<Cfg<32, 2, 80>>; __VA_ARGS__; }       \
    else if ((lo).H == 64 && (lo).HEADS == 4 && (lo).MEL == 16) { using LN = Launcher<Cfg<64, 4, 16>>; __VA_ARGS__; }       \
    EDTTS_EXTRA_INSTANCES(lo, __VA_ARGS__)                                                               \
    else { MISS32; }
static int no_instance16(const Layout& lo) {
  return fail(EDTTS_ERR_UNSUPPORTED, "no bf16 kernel instance for hidden=%d heads=%d n_mels=%d "
              "(compiled: 256/8/80, 64/2/80" EDTTS_EXTRA_NAMES16 "; more: EDTTS_INSTANCES_BF16 at build time)", lo.H, lo.HEADS, lo.MEL);
}
static int no_instance32(const Layout& lo) {
  return fail(EDTTS_ERR_UNSUPPORTED, "no kernel instance for hidden=%d heads=%d n_mels=%d "
              "(compiled: 160/4/80, 256/8/80, 32/2/80, 64/4/16" EDTTS_EXTRA_NAMES "; more: EDTTS_INSTANCES at build time)", lo.H, lo.HEADS, lo.MEL);
}
#endif
#define EDTTS_DISPATCH(lo, ...)                                                                          \
  do {                                                                                                   \
    if ((lo).GEN) { using LN = GenericLauncher; __VA_ARGS__; }                                           \
    else { EDTTS_FUSED_CHAIN(lo, return no_instance16(lo), return no_instance32(lo), __VA_ARGS__) }      \
  } while (0)
static bool has_instance(const Layout& lo) {
  EDTTS_FUSED_CHAIN(lo, return false, return false, return true)
}

static int launch_cond16(const Layout& lo, const CondArgs& a, int rows, hipStream_t stream);  // edtts_generic16.h
static int launch_cond(const Layout& lo, const float* blob, const int64_t* t, const int64_t* step_idx, const int64_t* t_host,
                       int rows, float* cond, float* wsb, hipStream_t st) {
  CondArgs a;
  memset(&a, 0, sizeof(a));
  a.t = t; a.step_idx = step_idx; a.H = lo.H; a.L = lo.L; a.n_step = lo.NSTEP;
  if (t_host) {  // fused sampler: row i = (timesteps[i], step index i), inference.py:38-40
    if (rows > kMaxHostRows) return fail(EDTTS_ERR_ARG, "num_steps=%d > %d", rows, kMaxHostRows);
    a.use_host = 1; a.host_has_step = 1;
    for (int i = 0; i < rows; ++i) { a.t_host[i] = (int)t_host[i]; a.step_host[i] = i; }
  }
  a.freqs = blob + lo.freqs; a.t1T = blob + lo.t1T; a.t1b = blob + lo.t1b; a.t3T = blob + lo.t3T; a.t3b = blob + lo.t3b;
  a.step = blob + lo.step; a.blob = blob;
  for (int l = 0; l < lo.L; ++l) {
    a.ada1T[l] = (unsigned)lo.layer[l].ada1T; a.ada1b[l] = (unsigned)lo.layer[l].ada1b;
    a.ada3T[l] = (unsigned)lo.layer[l].ada3T; a.ada3b[l] = (unsigned)lo.layer[l].ada3b;
  }
  a.cond = cond;
  a.err = reinterpret_cast<unsigned*>(wsb);  // Workspace::err = 0
  a.tcond = cond + (size_t)rows * lo.L * 2 * 2 * lo.H;  // scratch right behind the rows (see make_workspace)
  if (lo.MM16) return launch_cond16(lo, a, rows, st);  // the same rows with their products on bf16 MFMAs
  hipLaunchKernelGGL(k_cond_mlp, dim3(rows), dim3(256), 2 * lo.H * sizeof(float), st, a);
  LAUNCH_CHECK("k_cond_mlp");
  hipLaunchKernelGGL(k_cond_ada, dim3(rows, 2 * lo.L, (2 * lo.H + 255) / 256), dim3(256), lo.H * sizeof(float), st, a);
  LAUNCH_CHECK("k_cond_ada");
  return EDTTS_OK;
}

// Per-utterance lengths outside [1, T] / [1, S] (edtts_*_len): the kernels clamp them (utt_len); this marks the index-error word.
// t_min > 1: frame counts below it are flagged too (edtts_sample_inpaint_len: an utterance shorter than the known overlap)
extern "C" __global__ __launch_bounds__(256) void k_len_check(const int64_t* t_len, const int64_t* s_len, int B, int T, int S, int t_min, unsigned* err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  if ((t_len && (t_len[i] < t_min || t_len[i] > T)) || (s_len && (s_len[i] < 1 || s_len[i] > S))) atomicOr(err, (unsigned)EDTTS_IDX_LEN);
}
static int launch_len_check(const int64_t* t_len, const int64_t* s_len, int B, int T, int S, float* wsb, hipStream_t st, int t_min = 1) {
  if (!t_len && !s_len) return EDTTS_OK;
  hipLaunchKernelGGL(k_len_check, dim3((B + 255) / 256), dim3(256), 0, st, t_len, s_len, B, T, S, t_min, reinterpret_cast<unsigned*>(wsb));
  LAUNCH_CHECK("k_len_check");
  return EDTTS_OK;
}

static int check_shapes(const Layout& lo, int B, int T, int S) {
  if (B < 1 || T < 1 || S < 1) return fail(EDTTS_ERR_ARG, "B=%d T=%d S=%d must be positive", B, T, S);
  if (T > lo.MAXPOS) return fail(EDTTS_ERR_ARG, "T=%d exceeds the positional table (%d rows) -- the reference raises here too", T, lo.MAXPOS);
  if (S > lo.MAXCPOS) return fail(EDTTS_ERR_ARG, "S=%d exceeds the context positional table (%d rows)", S, lo.MAXCPOS);
  return EDTTS_OK;
}

// The units that hold a whole subsystem each -- kernels, host helpers, extern "C" entry points -- included here, behind the
// launchers and the pre-launch steps above that their entry points call (launch_cond, launch_len_check, check_shapes, EDTTS_DISPATCH)
// Every header of this directory is included exactly once, in dependency order (tests/test_host_cpu.py checks it by a text scan), so
// the units carry no include guard: a second inclusion is a redefinition error, not a silent no-op.
#include "edtts_melpost.h"       // mel -> spectrogram, Griffin-Lim (edtts_audio.h uses its FFT)
#include "edtts_generic_bwd.h"   // training the decoder; drop_state, which edtts_semantic_bwd.h calls
#include "edtts_generic16.h"     // ... and both on bf16 MFMAs (EDTTS_MATMUL_BF16) <- edtts_generic.h, edtts_generic_bwd.h, edtts_bf16.h
#include "edtts_generic_attn16.h"  // ... their attention on bf16 MFMAs (EDTTS_ATTN_BF16) <- edtts_generic.h, edtts_generic_bwd.h, edtts_bf16.h
#include "edtts_semantic.h"      // SemanticEncoder: proj, FSQ / VQ <- edtts_generic.h: DropArgs
#include "edtts_semantic_bwd.h"  // ... its training <- edtts_generic_bwd.h: k_bwd_*, drop_state
#include "edtts_hubert.h"        // NativeHubert: the fp32 kernels
#include "edtts_hubert16.h"      // ... the bf16 MFMA kernels <- edtts_hubert.h: gelu, HEPI_*
#include "edtts_hubert_host.h"   // ... layout, workspace, packing, launch list, edtts_hubert_* <- both; edtts_generic.h: k_gen_norm, attn
#include "edtts_audio.h"         // MelSpectrogram, log-mel statistics, Resample <- edtts_melpost.h: melpost::cplx
#include "edtts_optim.h"         // FusedAdamW: k_opt_*, edtts_optim_*
#include "edtts_keys.h"          // KeyStream: k_keys_advance, edtts_keys_* <- edtts_device.h: philox4x32_10
#include "edtts_objective.h"     // DiffusionObjective: k_obj_*, edtts_objective_*
#include "edtts_samplers.h"      // the samplers: step kernels, step loops, edtts_generate*, edtts_sample_*, edtts_randn*
#include "edtts_debug.h"         // edtts_profile_*, the diagnostic builds' exports (g_prof, g_stamps_fwd, g_wavelog are defined above)

extern "C" {

int edtts_version(void) { return EDTTS_VERSION; }
const char* edtts_last_error(void) { return g_err; }
int edtts_num_global_slots(void) { return G_COUNT; }
int edtts_num_layer_slots(void) { return L_COUNT; }
const char* edtts_global_slot_name(int i) { return (i >= 0 && i < G_COUNT) ? kGlobalNames[i] : nullptr; }
const char* edtts_layer_slot_name(int i) { return (i >= 0 && i < L_COUNT) ? kLayerNames[i] : nullptr; }

int edtts_packed_bytes(const EdttsDims* dims, size_t* out_bytes) {
  Layout lo;
  int rc = make_layout(dims, &lo);
  if (rc) return rc;
  if (!out_bytes) return fail(EDTTS_ERR_ARG, "out_bytes is NULL");
  if (lo.total >= ((size_t)1 << 32)) return fail(EDTTS_ERR_UNSUPPORTED, "packed blob too large");
  *out_bytes = lo.total * sizeof(float);
  return EDTTS_OK;
}

int edtts_workspace_bytes(const EdttsDims* dims, int B, int T, int S, int cond_rows, size_t* out_bytes) {
  Layout lo;
  int rc = make_layout(dims, &lo);
  if (rc) return rc;
  if (!out_bytes || B < 1 || T < 1 || S < 1 || cond_rows < 1) return fail(EDTTS_ERR_ARG, "bad workspace query (B=%d T=%d S=%d rows=%d)", B, T, S, cond_rows);
  // room for either form of a sampler call: the batch in one piece, or cut into sub-batches (plan_call)
  SubBatches one, two;
  plan_sub(lo, B, T, S, cond_rows, 1, &one);
  size_t total = one.total;
  for (int n = 2; n <= kMaxSub && n <= B && !lo.GEN; ++n) {
    plan_sub(lo, B, T, S, cond_rows, n, &two);
    if (two.total > total) total = two.total;
  }
  *out_bytes = total * sizeof(float);
  return EDTTS_OK;
}

static int pack_gemm(hipStream_t st, const float* src, int ld, int N, int K, int NT, int KT, int rowmode, int colmode,
                     int dstmode, int DH, int DHP, float* dst, int scale_rows = 0, float scale = 1.0f) {
  PackArgs p{src, ld, N, K, NT, KT, rowmode, colmode, dstmode, DH, DHP, dst, scale_rows, scale};
  hipLaunchKernelGGL(k_pack_gemm, dim3(NT * KT), dim3(64), 0, st, p);
  LAUNCH_CHECK("k_pack_gemm");
  return EDTTS_OK;
}
static int pack_gemm16(hipStream_t st, const float* src, int ld, int N, int K, int NT, int KT, int mode, float* dst, int blk = 0,
                       int upfr = 0, int scale_rows = 0, float scale = 1.0f) {
  PackArgs16 p{src, ld, N, K, NT, KT, mode, blk, upfr, reinterpret_cast<unsigned short*>(dst), scale_rows, scale};
  hipLaunchKernelGGL(k_pack_gemm16, dim3(NT * KT), dim3(64), 0, st, p);
  LAUNCH_CHECK("k_pack_gemm16");
  return EDTTS_OK;
}
static int copy_f(hipStream_t st, const float* src, float* dst, size_t n) {
  hipLaunchKernelGGL(k_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst, n);
  LAUNCH_CHECK("k_copy");
  return EDTTS_OK;
}
static int transpose_f(hipStream_t st, const float* src, float* dst, int N, int K) {
  hipLaunchKernelGGL(k_transpose, dim3((unsigned)(((size_t)N * K + 255) / 256)), dim3(256), 0, st, src, dst, N, K);
  LAUNCH_CHECK("k_transpose");
  return EDTTS_OK;
}

// generic layout (make_generic_layout): where a weight slot goes -- offset in floats, the slot's [rows][cols], and whether the blob
// holds its transpose (the matrices the conditioning kernels read).  pack_generic and edtts_generic_slot_dest both read this.
struct SlotDest {
  size_t off, rows, cols;
  bool tr;
};
static SlotDest generic_slot_dest(const Layout& lo, int slot) {
  const size_t H = lo.H, R = lo.R, SD = lo.SD, MEL = lo.MEL, FH = (size_t)lo.FM * lo.H;
  if (slot < G_COUNT) {
    switch (slot) {
      case G_TOK: return {lo.tok, (size_t)lo.NTOK, H, false};
      case G_SEMP_W: return {lo.semp, H, SD, false};
      case G_SEMP_B: return {lo.semp_b, 1, H, false};
      case G_T1_W: return {lo.t1T, H, H, true};
      case G_T1_B: return {lo.t1b, 1, H, false};
      case G_T3_W: return {lo.t3T, H, H, true};
      case G_T3_B: return {lo.t3b, 1, H, false};
      case G_STEP: return {lo.step, (size_t)lo.NSTEP, H, false};
      case G_INP_W: return {lo.inp, H, MEL, false};
      case G_INP_B: return {lo.inp_b, 1, H, false};
      case G_PE: return {lo.pe, (size_t)lo.MAXPOS, H, false};
      case G_CPE: return {lo.cpe, (size_t)lo.MAXCPOS, H, false};
      case G_FN_W: return {lo.fnw, 1, H, false};
      case G_FN_B: return {lo.fnb, 1, H, false};
      case G_OUT_W: return {lo.s_outp, MEL, H, false};
      case G_OUT_B: return {lo.outp_b, 1, MEL, false};
      default: return {lo.freqs, 1, H / 2, false};  // G_FREQS
    }
  }
  const LayerLayout& y = lo.layer[(slot - G_COUNT) / L_COUNT];
  switch ((slot - G_COUNT) % L_COUNT) {
    case L_N1_W: return {y.n1w, 1, H, false};
    case L_N1P_W: return {y.ada1T, 2 * H, H, true};
    case L_N1P_B: return {y.ada1b, 1, 2 * H, false};
    case L_QKV_W: return {y.s_qkv, 3 * H, H, false};
    case L_PROJ_W: return {y.g_proj, H, H, false};
    case L_PROJ_B: return {y.proj_b, 1, H, false};
    case L_N2_W: return {y.n2w, 1, H, false};
    case L_QP_W: return {y.g_qp, H, H, false};
    case L_KVD_W: return {y.kvd, R, H, false};
    case L_KVN_W: return {y.kvn, 1, R, false};
    case L_KVU_W: return {y.kvu, 2 * H, R, false};
    case L_OP_W: return {y.g_op, H, H, false};
    case L_N3_W: return {y.n3w, 1, H, false};
    case L_N3P_W: return {y.ada3T, 2 * H, H, true};
    case L_N3P_B: return {y.ada3b, 1, 2 * H, false};
    case L_UP_W: return {y.g_up, 2 * FH, H, false};
    case L_UP_B: return {y.up_b, 1, 2 * FH, false};
    case L_DOWN_W: return {y.g_down, H, FH, false};
    default: return {y.down_b, 1, H, false};  // L_DOWN_B
  }
}
static int pack_generic(const Layout& lo, const void* const* slots, float* blob, hipStream_t st) {
  for (int i = 0; i < G_COUNT + lo.L * L_COUNT; ++i) {
    const SlotDest d = generic_slot_dest(lo, i);
    if (d.tr) TRY_G(transpose_f(st, (const float*)slots[i], blob + d.off, (int)d.rows, (int)d.cols));
    else TRY_G(copy_f(st, (const float*)slots[i], blob + d.off, d.rows * d.cols));
  }
  return EDTTS_OK;
}

int edtts_pack_weights(const EdttsDims* dims, const void* const* slots, int n_slots, void* packed, void* stream) {
  Layout lo;
  TRY_G(make_layout(dims, &lo));
  if (!slots || !packed) return fail(EDTTS_ERR_ARG, "slots/packed is NULL");
  if (n_slots != G_COUNT + lo.L * L_COUNT) return fail(EDTTS_ERR_ARG, "expected %d weight slots, got %d", G_COUNT + lo.L * L_COUNT, n_slots);
  for (int i = 0; i < n_slots; ++i)
    if (!slots[i]) return fail(EDTTS_ERR_ARG, "weight slot %d is NULL", i);
  hipStream_t st = (hipStream_t)stream;
  float* blob = (float*)packed;
  auto G = [&](int i) { return (const float*)slots[i]; };
  const int H = lo.H, HT = lo.HT, MT = lo.MT, R = lo.R, RT = lo.RT, SD = lo.SD, DH = lo.DH, DHP = lo.DHP, FM = lo.FM;
  const int KPT = lo.HEADS * DHP / 16;
  HIP_TRY(hipMemsetAsync(blob, 0, lo.total * sizeof(float), st));
  if (lo.GEN) return pack_generic(lo, slots, blob, st);
  TRY_G(copy_f(st, G(G_TOK), blob + lo.tok, (size_t)lo.NTOK * H));
  TRY_G(pack_gemm(st, G(G_SEMP_W), SD, H, SD, HT, SD / 16, 0, 0, 0, DH, DHP, blob + lo.semp));
  TRY_G(copy_f(st, G(G_SEMP_B), blob + lo.semp_b, H));
  TRY_G(transpose_f(st, G(G_T1_W), blob + lo.t1T, H, H));
  TRY_G(copy_f(st, G(G_T1_B), blob + lo.t1b, H));
  TRY_G(transpose_f(st, G(G_T3_W), blob + lo.t3T, H, H));
  TRY_G(copy_f(st, G(G_T3_B), blob + lo.t3b, H));
  TRY_G(copy_f(st, G(G_STEP), blob + lo.step, (size_t)lo.NSTEP * H));
  const int KT16 = H / 32, MKT16 = (lo.MEL + 31) / 32, MTP16 = (MT + 1) / 2;  // bf16 fragment grid (edtts_bf16.h)
  if (lo.BF16) TRY_G(pack_gemm16(st, G(G_INP_W), lo.MEL, H, lo.MEL, HT, MKT16, 1, blob + lo.inp));  // k-major, head of the stream
  else
  TRY_G(pack_gemm(st, G(G_INP_W), lo.MEL, H, lo.MEL, HT, MT, 0, 0, 4, DH, DHP, blob + lo.inp));  // n-tile pairs, head of the stream
  TRY_G(copy_f(st, G(G_INP_B), blob + lo.inp_b, H));
  TRY_G(copy_f(st, G(G_PE), blob + lo.pe, (size_t)lo.MAXPOS * H));
  TRY_G(copy_f(st, G(G_CPE), blob + lo.cpe, (size_t)lo.MAXCPOS * H));
  TRY_G(copy_f(st, G(G_FN_W), blob + lo.fnw, H));
  TRY_G(copy_f(st, G(G_FN_B), blob + lo.fnb, H));
  if (lo.BF16) TRY_G(pack_gemm16(st, G(G_OUT_W), H, lo.MEL, H, 2 * MTP16, KT16, 0, blob + lo.s_outp));  // n-tile pairs (rows >= n_mels: zero)
  else
  TRY_G(pack_gemm(st, G(G_OUT_W), H, lo.MEL, H, MT, HT, 0, 0, 0, DH, DHP, blob + lo.s_outp));
  TRY_G(copy_f(st, G(G_OUT_B), blob + lo.outp_b, lo.MEL));
  TRY_G(copy_f(st, G(G_FREQS), blob + lo.freqs, H / 2));
  for (int l = 0; l < lo.L; ++l) {
    const LayerLayout& y = lo.layer[l];
    auto W = [&](int i) { return (const float*)slots[G_COUNT + l * L_COUNT + i]; };
    TRY_G(copy_f(st, W(L_N1_W), blob + y.n1w, H));
    TRY_G(transpose_f(st, W(L_N1P_W), blob + y.ada1T, 2 * H, H));
    TRY_G(copy_f(st, W(L_N1P_B), blob + y.ada1b, 2 * H));
    TRY_G(copy_f(st, W(L_PROJ_B), blob + y.proj_b, H));
    TRY_G(copy_f(st, W(L_N2_W), blob + y.n2w, H));
    TRY_G(copy_f(st, W(L_N3_W), blob + y.n3w, H));
    TRY_G(transpose_f(st, W(L_N3P_W), blob + y.ada3T, 2 * H, H));
    TRY_G(copy_f(st, W(L_N3P_B), blob + y.ada3b, 2 * H));
    hipLaunchKernelGGL(k_pack_upbias, dim3((2 * FM * H + 255) / 256), dim3(256), 0, st, W(L_UP_B), blob + y.up_b, FM * H);
    LAUNCH_CHECK("k_pack_upbias");
    TRY_G(copy_f(st, W(L_DOWN_B), blob + y.down_b, H));
    TRY_G(pack_gemm(st, W(L_KVD_W), H, R, H, RT, HT, 0, 0, 0, DH, DHP, blob + y.kvd));
    TRY_G(copy_f(st, W(L_KVN_W), blob + y.kvn, R));
    TRY_G(pack_gemm(st, W(L_KVU_W), R, 2 * H, R, 2 * HT, RT, 0, 0, 0, DH, DHP, blob + y.kvu));
    // fragment stream
    // the query rows carry the softmax scale: scores come out of K Q^T in the exp2 domain, log2(e) / sqrt(head_dim)
    const float qscale = 1.4426950408889634f / sqrtf((float)DH);
    if (lo.BF16) {
      float* c16 = blob + lo.s_ctx16 + (size_t)l * ctx16_frags(lo) * kFrag;
      TRY_G(pack_gemm16(st, W(L_KVD_W), H, R, H, RT, KT16, 0, c16));                                   // kv_down as n-tile pairs
      TRY_G(pack_gemm16(st, W(L_KVU_W), R, 2 * H, R, 2 * HT, R / 32, 0, c16 + (size_t)RT * KT16 * kFrag));  // kv_up: K heads | V heads
      TRY_G(pack_gemm16(st, W(L_QKV_W), H, 3 * H, H, 3 * HT, KT16, 0, blob + y.s_qkv, 0, 0, H, qscale));  // q | k | v as n-tile pairs
      float* s16 = blob + y.s_body;
      TRY_G(pack_gemm16(st, W(L_PROJ_W), H, H, H, HT, KT16, 1, s16));                       // k-major: k-tile = head
      s16 += (size_t)HT * KT16 * kFrag;
      TRY_G(pack_gemm16(st, W(L_QP_W), H, H, H, HT, KT16, 0, s16, 0, 0, H, qscale));
      s16 += (size_t)HT * KT16 * kFrag;
      TRY_G(pack_gemm16(st, W(L_OP_W), H, H, H, HT, KT16, 1, s16));
      s16 += (size_t)HT * KT16 * kFrag;
      const int blk = 4 * KT16 + HT;  // per down k-tile: value/gate fragments of its two hidden tiles, then HT down fragments
      TRY_G(pack_gemm16(st, W(L_UP_W), H, 2 * FM * H, H, 2 * FM * HT, KT16, 2, s16, blk, 4 * KT16));
      TRY_G(pack_gemm16(st, W(L_DOWN_W), FM * H, H, FM * H, HT, FM * HT / 2, 3, s16, blk, 4 * KT16));
      continue;
    }
    TRY_G(pack_gemm(st, W(L_QKV_W), H, 3 * H, H, 3 * HT, HT, 0, 0, 4, DH, DHP, blob + y.s_qkv, H, qscale));  // n-tile pairs
    float* s = blob + y.s_body;
    TRY_G(pack_gemm(st, W(L_PROJ_W), H, H, lo.HEADS * DHP, HT, KPT, 0, 1, 1, DH, DHP, s));
    s += (size_t)KPT * HT * kFrag;
    TRY_G(pack_gemm(st, W(L_QP_W), H, H, H, HT, HT, 0, 0, 4, DH, DHP, s, H, qscale));
    s += (size_t)HT * HT * kFrag;
    TRY_G(pack_gemm(st, W(L_OP_W), H, H, lo.HEADS * DHP, HT, KPT, 0, 1, 1, DH, DHP, s));
    s += (size_t)KPT * HT * kFrag;
    TRY_G(pack_gemm(st, W(L_UP_W), H, 2 * FM * H, H, 2 * FM * HT, HT, 1, 0, 2, DH, DHP, s));     // value/gate tiles interleaved
    TRY_G(pack_gemm(st, W(L_DOWN_W), FM * H, H, FM * H, HT, FM * HT, 0, 0, 3, DH, DHP, s));  // k-tile j after its up tiles
  }
  return EDTTS_OK;
}

int edtts_decoder_forward(const EdttsDims* dims, const void* packed, void* workspace, int B, int T, int S, const float* x,
                          const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx, const float* sem_features,
                          float* eps, void* stream) {
  return edtts_decoder_forward_len(dims, packed, workspace, B, T, S, x, t, step_idx, sem_idx, sem_features, nullptr, nullptr, eps, stream);
}

int edtts_decoder_forward_len(const EdttsDims* dims, const void* packed, void* workspace, int B, int T, int S, const float* x,
                              const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx, const float* sem_features,
                              const int64_t* t_len, const int64_t* s_len, float* eps, void* stream) {
  const SettingsScope settings;
  Layout lo;
  TRY_G(make_layout(dims, &lo));
  if (!sem_idx && !sem_features) return fail(EDTTS_ERR_ARG, "Either sem_idx or sem_features must be provided");
  if (!packed || !workspace || !x || !t || !eps) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  TRY_G(check_shapes(lo, B, T, S));
  hipStream_t st = (hipStream_t)stream;
  const float* blob = (const float*)packed;
  float* wsb = (float*)workspace;
  Workspace ws;
  make_workspace(lo, B, T, S, B, &ws);
  TRY_G(launch_len_check(t_len, s_len, B, T, S, wsb, st));
  TRY_G(launch_cond(lo, blob, t, step_idx, nullptr, B, wsb + ws.cond, wsb, st));
  const int bstride = lo.L * 2 * 2 * lo.H;
  const CallCtx c{lo, blob, ws, wsb, B, T, S, dims->window, Lens{t_len, s_len}, st};
  StepTail tail;
  tail.eps = eps;
  EDTTS_DISPATCH(lo, {
    TRY_G(set_attrs_once<LN>());
    TRY_G(LN::ctx(c, sem_features ? nullptr : sem_idx, sem_features));
    TRY_G(LN::forward(c, x, wsb + ws.cond, bstride, tail));
  });
  return EDTTS_OK;
}

// the one-kernel path: the reference's shape class, and the raw rows of one 128-frame pass must fit the staging tile
static bool dsconv_takes_fused_path(int C_in, int C_out, int To, int ksize, int stride) {
  static const bool no_fused = [] { const char* e = getenv("EDTTS_DSCONV_UNFUSED"); return e && e[0] == '1'; }();
  return !no_fused && C_in <= 80 && C_out <= 160 && To <= 512 && (kDfT - 1) * stride + ksize <= 260;
}

int edtts_dsconv_scratch_floats(int B, int C_in, int C_out, int T, int ksize, int stride, int groups, size_t* out_floats) {
  if (!out_floats) return fail(EDTTS_ERR_ARG, "out_floats is NULL");
  if (B < 1 || C_in < 1 || C_out < 1 || T < 1 || ksize < 1 || stride < 1 || groups < 1) return fail(EDTTS_ERR_ARG, "bad sizes");
  const int To = (T + 2 * (ksize / 2) - ksize) / stride + 1;
  if (To < 1) return fail(EDTTS_ERR_ARG, "no output frames (T=%d, kernel %d, stride %d)", T, ksize, stride);
  *out_floats = dsconv_takes_fused_path(C_in, C_out, To, ksize, stride) ? 0 : (size_t)B * C_out * To + (size_t)2 * B * groups;
  return EDTTS_OK;
}

int edtts_dsconv_forward(const float* x, const float* dw, const float* pw, const float* pb, const float* gn_w, const float* gn_b,
                         int B, int C_in, int C_out, int T, int ksize, int stride, int groups, float* scratch, float* y, void* stream) {
  if (!x || !dw || !pw || !pb || !gn_w || !gn_b || !y) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (B < 1 || C_in < 1 || C_out < 1 || T < 1 || ksize < 1 || stride < 1 || groups < 1 || C_out % groups) return fail(EDTTS_ERR_ARG, "bad sizes");
  if (C_in > 256) return fail(EDTTS_ERR_UNSUPPORTED, "C_in=%d > 256 (the depthwise tile is kept in registers per wave)", C_in);
  const int To = (T + 2 * (ksize / 2) - ksize) / stride + 1;  // torch.nn.Conv1d output length
  if (To < 1) return fail(EDTTS_ERR_ARG, "no output frames (T=%d, kernel %d, stride %d)", T, ksize, stride);
  hipStream_t st = (hipStream_t)stream;
  // Fused path (z never leaves the registers of one 512-thread block per utterance): the reference's own shape class
  // (C_in <= 80, C_out <= 160, T_out <= 512) -- HBM traffic = x in + y out.
  if (dsconv_takes_fused_path(C_in, C_out, To, ksize, stride)) {
    static std::atomic<bool> attr_done[64];
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const int lds = dsconv_fused_lds_floats<5, 10>() * (int)sizeof(float);
    auto kern = k_dsconv_fused<5, 10, 4, kDfT>;
    auto kern_wide = k_dsconv_fused<5, 10, 2, kDfTWide>;
    auto kern_grp = (To & 3) == 0 ? k_dsconv_grouped<5, 10, 20, true> : k_dsconv_grouped<5, 10, 20, false>;  // C_out = 160, GroupNorm(8): the layer conv.py builds
    const int lds_grp = dsconv_grouped_lds_floats<5, 10>(8) * (int)sizeof(float);
    if (dev >= 0 && dev < 64 && !attr_done[dev].load(std::memory_order_acquire)) {
      HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      HIP_TRY(hipFuncSetAttribute((const void*)kern_wide, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      HIP_TRY(hipFuncSetAttribute((const void*)k_dsconv_grouped<5, 10, 20, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_grp));
      HIP_TRY(hipFuncSetAttribute((const void*)k_dsconv_grouped<5, 10, 20, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_grp));
      attr_done[dev].store(true, std::memory_order_release);
    }
    static const bool no_wide = [] { const char* e = getenv("EDTTS_DSCONV_WAVES8"); return e && e[0] == '1'; }();  // (A/B hook)
    static const bool no_grp = [] { const char* e = getenv("EDTTS_DSCONV_NOGROUP"); return e && e[0] == '1'; }();  // (A/B hook)
    if (!no_grp && !no_wide && C_out == 160 && groups == 8 && stride == 1 && kDfTWide - 1 + ksize <= kDfXld)
      hipLaunchKernelGGL(kern_grp, dim3(B), dim3(kDfTWide * 4), lds_grp, st, x, dw, pw, pb, gn_w, gn_b, C_in, T, To, ksize, y);
    else if (!no_wide && stride == 1 && kDfTWide - 1 + ksize <= kDfXld)  // (measured and rejected: taps read straight from global memory instead of the staging tile, 85 vs 77.5 us)
      hipLaunchKernelGGL(kern_wide, dim3(B), dim3(kDfTWide * 4), lds, st, x, dw, pw, pb, gn_w, gn_b, C_in, C_out, T, To, ksize, stride, groups, y);
    else
      hipLaunchKernelGGL(kern, dim3(B), dim3(kDfT * 4), lds, st, x, dw, pw, pb, gn_w, gn_b, C_in, C_out, T, To, ksize, stride, groups, y);
    LAUNCH_CHECK("k_dsconv_fused");
    return EDTTS_OK;
  }
  if (!scratch) return fail(EDTTS_ERR_ARG, "this shape takes the three-kernel path: scratch required (edtts_dsconv_scratch_floats: B*C_out*T_out + 2*B*groups floats)");
  float* z = scratch;
  float* stats = scratch + (size_t)B * C_out * To;
  const int Cip = (C_in + 15) & ~15;
  hipLaunchKernelGGL(k_dsconv_pw, dim3((To + kDsTileT - 1) / kDsTileT, B), dim3(256), (size_t)Cip * kDsLd * sizeof(float), st, x, dw, pw, pb,
                     B, C_in, C_out, T, To, ksize, stride, z);
  LAUNCH_CHECK("k_dsconv_pw");
  hipLaunchKernelGGL(k_dsconv_stats, dim3(B * groups), dim3(256), 0, st, z, C_out, To, groups, stats);
  LAUNCH_CHECK("k_dsconv_stats");
  hipLaunchKernelGGL(k_dsconv_norm, dim3((unsigned)((size_t)B * C_out)), dim3(128), 0, st, z, stats, gn_w, gn_b, C_out, To, groups, y);
  LAUNCH_CHECK("k_dsconv_norm");
  return EDTTS_OK;
}

int edtts_index_errors(void* workspace, int* flags_host, void* stream) {
  if (!workspace || !flags_host) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  hipStream_t st = (hipStream_t)stream;
  unsigned v = 0;
  HIP_TRY(hipMemcpyAsync(&v, workspace, sizeof(v), hipMemcpyDeviceToHost, st));  // Workspace::err = 0
  HIP_TRY(hipStreamSynchronize(st));
  if (v) HIP_TRY(hipMemsetAsync(workspace, 0, sizeof(v), st));
  *flags_host = (int)v;
  return EDTTS_OK;
}

int edtts_set_coop(int mode) {
  if (mode == -1 || mode == 0 || mode == 14 || mode == 24 || mode == 22) return g_coop.exchange(mode);
  return g_coop.load();
}

int edtts_set_substreams(int n) {
  if (n >= 1 && n <= kMaxSub) return g_substreams.exchange(n);
  return g_substreams.load();
}

int edtts_substreams_for(const EdttsDims* dims, int B, int T) {
  const SettingsScope settings;
  Layout lo;
  if (make_layout(dims, &lo) || B < 1 || T < 1) return 1;
  return substreams_for(lo, B, T, (T + 1) / 2);
}

int edtts_generic_slot_dest(const EdttsDims* dims, int slot, size_t* offset_floats, int* rows, int* cols, int* transposed) {
  Layout lo;
  TRY_G(train_layout(dims, "edtts_generic_slot_dest", &lo));
  if (!offset_floats || !rows || !cols || !transposed) return fail(EDTTS_ERR_ARG, "edtts_generic_slot_dest: NULL pointer argument");
  if (slot < 0 || slot >= G_COUNT + lo.L * L_COUNT) return fail(EDTTS_ERR_ARG, "edtts_generic_slot_dest: slot %d of %d", slot, G_COUNT + lo.L * L_COUNT);
  const SlotDest d = generic_slot_dest(lo, slot);
  *offset_floats = d.off;
  *rows = (int)d.rows;
  *cols = (int)d.cols;
  *transposed = d.tr ? 1 : 0;
  return EDTTS_OK;
}

}  // extern "C"
