// edtts_hubert16.h -- the bf16 compute path of the HuBERT backbone (included by edtts_kernels.hip after edtts_hubert.h).
//
// Same forward as edtts_hubert.h with the two operands of every contraction after conv0 rounded to bf16 (round to nearest even,
// v_cvt_pk_bf16_f32) and the products on v_mfma_f32_16x16x32_bf16 with fp32 accumulators:
//   conv1 .. conv_last, feature projection, positional conv, QKV, out_proj, FFN     k_hub_gemm16<EPI, TW, XBF, YBF>
//   Q K^T and P V                                                                    k_hub_vt + k_hub_attn16<KT>
// fp32, on the kernels of edtts_hubert.h and edtts_generic.h: the GroupNorm statistics, the residual stream h, every LayerNorm,
// biases, GELU, residual adds, the softmax (max, exp2, row sum, normalisation), the output.  conv0 itself is the fp32 arithmetic of
// k_hub_conv0; only its store differs (k_hub_conv0_16).
//
// An intermediate that only a GEMM (or the attention) reads is STORED as bf16 -- rounding at the producer's store is rounding at
// the consumer's staging: conv0's output, the outputs of conv1 .. conv_{last-1}, the q | k | v rows, the attention output, the FFN
// intermediate.  What a norm or a residual reads stays fp32: the last conv's output, the feature projection's LayerNorm output, h,
// the positional conv's output.
//
// k_hub_gemm16: the tiling of k_hub_gemm (block 32 TW x 32 TW, four waves of 16 TW x 16 TW, two LDS buffers, one barrier per K
// tile, the next tile's global loads in flight during the MFMAs) with K tiles of 32 = one MFMA per 16 x 16 sub-tile.  LDS rows
// are [row][32 k] bf16 at a pitch of 40 (80 bytes): lane (fq, g) reads its operand -- k = 8 g .. 8 g + 7 of row fq -- as one
// ds_read_b128, and the 16 rows of a lane group start 20 banks apart (all 64 banks once).  A 16-byte chunk of 8 k never straddles
// two taps (Cin % 8 == 0); K needs no multiple of 32: chunks past K are staged as zeros.  Every output element is one k-ordered
// chain of MFMA steps whatever its tile, the tile size or the batch: bitwise independent of B, T and TW, no atomics, no split-K.
//
// k_hub_attn16: one wave = 16 queries of one (utterance, head), four waves per block, 32 keys per step.  S^T = K Q^T (K rows as the
// A operand, Q rows as B, both one 16-byte load per lane and k-tile): lane (g, i) holds the scores of query i against keys 4 g + r
// of two 16-key tiles.  Online softmax in fp32 on those registers.  The eight probabilities of a lane, converted pairwise, ARE the
// B operand of O^T += V^T P^T when the 32 keys of the step are assigned to the operand's k slots as
//     slot 8 g + j  <->  key 4 g + j (j < 4),  16 + 4 g + (j - 4) (j >= 4)
// (the contraction order of an MFMA is free), so P never leaves registers.  V^T comes from k_hub_vt, which writes
// [utterance][head][d][key slot] with exactly that order inside every 32-key chunk and zeros for keys past the utterance's count:
// the A operand is one 16-byte load per lane, and neither K rows nor V rows past the count are read.
namespace edtts_hub {

constexpr int kBK16 = 32;         // GEMM K tile (one MFMA k-step)
constexpr int kLD16 = kBK16 + 8;  // LDS row pitch (bf16): 80 bytes, conflict-free b128 fragment reads

typedef __bf16 bf4v __attribute__((ext_vector_type(4)));

EDTTS_DEV bf8 zero_bf8() { return edtts16::as_bf8(splat(0.f)); }
EDTTS_DEV bf8 ldg_bf8p(const __bf16* p) { return *reinterpret_cast<const bf8*>(p); }

struct HGemm16Args {
  const void* X;             // fp32 or bf16 (XBF); utterance b, group g, row r, channel c: X[b xbs + r ldrow + g xg + c]
  long long xbs;
  int ldrow, Cin, stride, pad, xg;
  const int64_t* nvalid;     // input rows of utterance b that exist (others read as 0): nvalid[b], or Tin for all
  int Tin;
  const __bf16* W;           // [G][N][K], K contiguous
  int K;
  const float* bias;         // [G][N] or null
  void* Y;                   // fp32 or bf16 (YBF): Y[b ybs + m ldy + g N + n]
  const float* R;            // residual (fp32), same indexing as Y (may be Y)
  long long ybs;
  int ldy, M, N, ntn;        // ntn: N tiles per group
};

template <int EPI, int TW, bool XBF, bool YBF>
__global__ __launch_bounds__(256) void k_hub_gemm16(HGemm16Args a) {
  constexpr int BT = 32 * TW;
  __shared__ __attribute__((aligned(16))) __bf16 lds[2][2][BT][kLD16];  // [buffer][X | W][row][k]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fq = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, grp = blockIdx.y / a.ntn, n0 = (blockIdx.y - grp * a.ntn) * BT, m0 = blockIdx.x * BT;
  const size_t xoff = (size_t)b * a.xbs + (size_t)grp * a.xg;
  const float* X32 = (const float*)a.X + xoff;
  const __bf16* X16 = (const __bf16*)a.X + xoff;
  const __bf16* W = a.W + (size_t)grp * a.N * a.K;
  const int nval = a.nvalid ? (int)a.nvalid[b] : a.Tin;
  // loader: rows lr + 64 i (i < TW / 2) of both operands, the 8 k at offset lk of the tile
  constexpr int NL = TW / 2;
  const int lr = tid >> 2, lk = 8 * (tid & 3);
  int tap = lk / a.Cin, ci = lk - tap * a.Cin;
  const int wm = 16 * TW * (w >> 1), wn = 16 * TW * (w & 1);
  f4 acc[TW][TW];
#pragma unroll
  for (int t = 0; t < TW; ++t)
#pragma unroll
    for (int u = 0; u < TW; ++u) acc[t][u] = splat(0.f);
  bf8 xv[NL], wv[NL];
  auto load = [&](int k0) {
    const bool kok = k0 + lk < a.K;  // (K % 8 == 0: the whole chunk or none of it)
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int m = m0 + lr + 64 * i, src = m * a.stride + tap - a.pad;
      xv[i] = zero_bf8();
      if (kok && m < a.M && src >= 0 && src < nval) {
        const size_t at = (size_t)src * a.ldrow + ci;
        if (XBF) xv[i] = ldg_bf8p(X16 + at);
        else xv[i] = edtts16::pack8(ldg4(X32 + at), ldg4(X32 + at + 4));
      }
      const int n = n0 + lr + 64 * i;
      wv[i] = (kok && n < a.N) ? ldg_bf8p(W + (size_t)n * a.K + k0 + lk) : zero_bf8();
    }
    ci += kBK16;
    while (ci >= a.Cin) { ci -= a.Cin; ++tap; }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      *reinterpret_cast<bf8*>(&lds[buf][0][lr + 64 * i][lk]) = xv[i];
      *reinterpret_cast<bf8*>(&lds[buf][1][lr + 64 * i][lk]) = wv[i];
    }
  };
  const int nk = (a.K + kBK16 - 1) / kBK16;
  load(0);
  store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load((kt + 1) * kBK16);
    bf8 fa[TW], fb[TW];
#pragma unroll
    for (int t = 0; t < TW; ++t) fa[t] = *reinterpret_cast<const bf8*>(&lds[buf][1][wn + 16 * t + fq][8 * g]);
#pragma unroll
    for (int u = 0; u < TW; ++u) fb[u] = *reinterpret_cast<const bf8*>(&lds[buf][0][wm + 16 * u + fq][8 * g]);
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
      for (int u = 0; u < TW; ++u) acc[t][u] = EDTTS_MFMA16(fa[t], fb[u], acc[t][u]);
    if (kt + 1 < nk) store(buf ^ 1);
    __syncthreads();
  }
  // epilogue: acc[t][u] lane (g, fq) holds Y[m = m0 + wm + 16 u + fq][n = n0 + wn + 16 t + 4 g + r]
  const size_t yoff = (size_t)b * a.ybs + (size_t)grp * a.N;
  float* Y32 = (float*)a.Y + yoff;
  __bf16* Y16 = (__bf16*)a.Y + yoff;
  const float* R = a.R ? a.R + yoff : nullptr;
  const float* bias = a.bias ? a.bias + (size_t)grp * a.N : nullptr;
#pragma unroll
  for (int t = 0; t < TW; ++t) {
    const int n = n0 + wn + 16 * t + 4 * g;
    if (n >= a.N) continue;  // (N % 4 == 0: n + 3 < N)
    const f4 bv = bias ? ldg4(bias + n) : splat(0.f);
#pragma unroll
    for (int u = 0; u < TW; ++u) {
      const int m = m0 + wm + 16 * u + fq;
      if (m >= a.M) continue;
      f4 o = acc[t][u] + bv;
      if (EPI == HEPI_GELU || EPI == HEPI_GELU_RESID) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = gelu(o[r]);
      }
      const size_t off = (size_t)m * a.ldy + n;
      if (EPI == HEPI_RESID || EPI == HEPI_GELU_RESID) o = ldg4(R + off) + o;  // h + f(h): the reference's residual order
      if (YBF) *reinterpret_cast<edtts16::f2s*>(Y16 + off) = edtts16::pack4(o);
      else stg4(Y32 + off, o);
    }
  }
}

// k_hub_conv0 with a bf16 store: the same fp32 arithmetic, four channels per thread, rounded once where conv1 would round them
__global__ __launch_bounds__(256) void k_hub_conv0_16(const float* wav, int T_audio, const float* w0, int C0, int k0, int s0,
                                                      const int64_t* len0, int T0, const float* stats, __bf16* y, int B) {
  const unsigned C4 = C0 / 4, n = (unsigned)B * T0 * C4;  // (< 2^31: checked by the host; 32-bit index arithmetic)
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const unsigned row = i / C4, b = row / T0, t = row - b * T0;
    const int c = 4 * (int)(i - row * C4);
    f4 o = splat(0.f);
    if ((int)t < (len0 ? (int)len0[b] : T0)) {
      const float* xp = wav + (size_t)b * T_audio + (size_t)t * s0;
      f4 v = splat(0.f);
      for (int j = 0; j < k0; ++j) {
        const f4 wj = ldg4(w0 + (size_t)j * C0 + c);
        const float xj = xp[j];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaf(wj[r], xj, v[r]);
      }
      const f4 sc = ldg4(stats + (size_t)b * 2 * C0 + c), sh = ldg4(stats + (size_t)b * 2 * C0 + C0 + c);
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = gelu(fmaf(v[r], sc[r], sh[r]));
    }
    *reinterpret_cast<edtts16::f2s*>(y + (size_t)row * C0 + c) = edtts16::pack4(o);
  }
}

// fp32 [co][ci][k] (state dict) -> bf16 [co][k][ci]; k = 1: a plain conversion
__global__ __launch_bounds__(256) void k_hub_pack16(const float* src, __bf16* dst, int co, int ci, int k) {
  const size_t n = (size_t)co * ci * k;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % ci);
    const size_t r = i / ci;
    const int j = (int)(r % k);
    const size_t o = r / k;
    dst[i] = (__bf16)src[(o * ci + c) * k + j];
  }
}

// ---- attention ------------------------------------------------------------------------------------------------------------------
struct HAttn16Args {
  const __bf16* qkv;   // row b T + i: q | k | v, each [heads][DH]
  __bf16* vt;          // [B][heads][DH][Tp], Tp = T rounded up to 32; inside a 32-key chunk in slot order (see the file comment)
  __bf16* o;           // row b T + i, [heads][DH]
  const int64_t* len;  // per-utterance frame counts [B], or null: T for all
  int H, heads, DH, T, Tp;
  float scale;         // log2(e) / sqrt(head_dim): scores in the exp2 domain
};
EDTTS_DEV int slot_key(int p) { return ((p & 4) ? 16 : 0) + 4 * (p >> 3) + (p & 3); }

// one block per (32-key chunk, head, utterance); keys past the utterance's count are written as zeros and not read
__global__ __launch_bounds__(256) void k_hub_vt(HAttn16Args a) {
  const int j0 = blockIdx.x * 32, hd = blockIdx.y, b = blockIdx.z;
  const int Tk = utt_len(a.len, b, a.T);
  if (j0 >= Tk) return;
  const __bf16* v = a.qkv + (size_t)b * a.T * 3 * a.H + 2 * a.H + hd * a.DH;
  __bf16* vt = a.vt + ((size_t)b * a.heads + hd) * a.DH * a.Tp + j0;
  for (int i = threadIdx.x; i < 4 * a.DH; i += 256) {
    const int d = i % a.DH, g = i / a.DH;
    bf8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = j0 + slot_key(8 * g + j);
      o[j] = key < Tk ? v[(size_t)key * 3 * a.H + d] : (__bf16)0.f;
    }
    *reinterpret_cast<bf8*>(vt + (size_t)d * a.Tp + 8 * g) = o;
  }
}

template <int KT>  // head_dim = 32 KT
__global__ __launch_bounds__(256) void k_hub_attn16(HAttn16Args a) {
  constexpr int DT = 2 * KT;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, fq = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 64 + 16 * w, hd = blockIdx.y, b = blockIdx.z;
  // Per-utterance counts: a tile of queries wholly past the count has no solo counterpart and stores nothing (its rows feed
  // row-local steps only and the output's rows past the count are zeroed at the end of the forward).
  const int Tk = utt_len(a.len, b, a.T);
  if (q0 >= Tk) return;
  const int qi = q0 + fq, ld = 3 * a.H;
  const bool qok = qi < a.T;
  const __bf16* base = a.qkv + (size_t)b * a.T * ld + hd * a.DH;
  const __bf16* qrow = base + (size_t)(qok ? qi : 0) * ld + 8 * g;
  bf8 bq[KT];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) bq[kt] = qok ? ldg_bf8p(qrow + 32 * kt) : zero_bf8();
  const __bf16* kb = base + a.H + 8 * g;
  const __bf16* vt = a.vt + (((size_t)b * a.heads + hd) * a.DH + fq) * a.Tp + 8 * g;
  f4 acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) acc[t] = splat(0.f);
  float m = -1e30f, l = 0.f;
  for (int j0 = 0; j0 < Tk; j0 += 32) {
    f4 sc[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int kj = j0 + 16 * tt + fq;
      const bool kok = kj < Tk;
      const __bf16* krow = kb + (size_t)(kok ? kj : 0) * ld;
      sc[tt] = splat(0.f);
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) sc[tt] = EDTTS_MFMA16(kok ? ldg_bf8p(krow + 32 * kt) : zero_bf8(), bq[kt], sc[tt]);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = j0 + 16 * tt + 4 * g + r;
        sc[tt][r] = key < Tk ? sc[tt][r] * a.scale : -INFINITY;
        mx = fmaxf(mx, sc[tt][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);
    const float alpha = exp2f(m - mn);
    float ps = 0.f;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sc[tt][r] = exp2f(sc[tt][r] - mn);
        ps += sc[tt][r];
      }
    ps += __shfl_xor(ps, 16);
    ps += __shfl_xor(ps, 32);
    l = l * alpha + ps;
    m = mn;
    const bf8 pb = edtts16::pack8(sc[0], sc[1]);  // slot 8 g + j: keys 4 g + j | 16 + 4 g + (j - 4)
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      acc[t] *= alpha;
      acc[t] = EDTTS_MFMA16(ldg_bf8p(vt + (size_t)16 * t * a.Tp + j0), pb, acc[t]);
    }
  }
  if (!qok) return;
  const float inv = 1.0f / l;
  __bf16* orow = a.o + (size_t)(b * a.T + qi) * a.H + hd * a.DH + 4 * g;
#pragma unroll
  for (int t = 0; t < DT; ++t)  // acc[t] lane (g, i) holds O^T[d = 16 t + 4 g + r][i]
    *reinterpret_cast<edtts16::f2s*>(orow + 16 * t) = edtts16::pack4(acc[t] * inv);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// The blob of the bf16 path: HubLayout's tensors in HubLayout's order, offsets in floats; a matrix that feeds an MFMA is bf16 (half
// the floats), conv0 / GroupNorm / biases / norm parameters stay fp32.
static int hub_layout16(const EdttsHubertDims* d, HubLayout& L) {
  const int rc = hub_layout(d, L);
  if (rc != EDTTS_OK) return rc;
  for (int i = 0; i < L.nc; ++i)
    if (L.C[i] % 8) return fail(EDTTS_ERR_UNSUPPORTED, "conv_dim[%d]=%d: compute_dtype bf16 needs a multiple of 8", i, L.C[i]);
  if (L.H % 8) return fail(EDTTS_ERR_UNSUPPORTED, "hidden_size=%d: compute_dtype bf16 needs a multiple of 8", L.H);
  if (L.DH % 32)
    return fail(EDTTS_ERR_UNSUPPORTED, "head_dim=%d (hidden_size=%d / num_attention_heads=%d): compute_dtype bf16 needs a multiple of 32",
                L.DH, L.H, L.heads);
  if (L.I % 8) return fail(EDTTS_ERR_UNSUPPORTED, "intermediate_size=%d: compute_dtype bf16 needs a multiple of 8", L.I);
  if (L.Cg % 8)
    return fail(EDTTS_ERR_UNSUPPORTED, "num_conv_pos_embedding_groups=%d: compute_dtype bf16 needs hidden_size / groups a multiple of 8", L.pg);
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += al64(n); return at; };
  auto half = [&](size_t n) { return take((n + 1) / 2); };
  L.conv0 = take((size_t)L.C[0] * L.k[0]);
  L.gn_w = take(L.C[0]);
  L.gn_b = take(L.C[0]);
  for (int i = 1; i < L.nc; ++i) L.conv[i] = half((size_t)L.C[i] * L.k[i] * L.C[i - 1]);
  const int CL = L.C[L.nc - 1];
  L.fp_w = take(CL); L.fp_b = take(CL);
  L.proj_w = half((size_t)L.H * CL); L.proj_b = take(L.H);
  L.pos_w = half((size_t)L.H * L.pk * L.Cg); L.pos_b = take(L.H);
  L.enc_w = take(L.H); L.enc_b = take(L.H);
  const size_t l0 = o;
  L.qkv_w = half((size_t)3 * L.H * L.H); L.qkv_b = take(3 * L.H);
  L.o_w = half((size_t)L.H * L.H); L.o_b = take(L.H);
  L.ln1_w = take(L.H); L.ln1_b = take(L.H);
  L.ff1_w = half((size_t)L.I * L.H); L.ff1_b = take(L.I);
  L.ff2_w = half((size_t)L.H * L.I); L.ff2_b = take(L.H);
  L.ln2_w = take(L.H); L.ln2_b = take(L.H);
  L.layer = o - l0;
  L.total = l0 + (size_t)L.L * L.layer;
  return EDTTS_OK;
}

struct HubWs16 {
  int T[kMaxConv];
  int nch, Tp;
  size_t lens, stats, part, buf0, buf1, h, att, big, vt, total;  // bytes
};
// element size of conv stage i's output: bf16 when the next conv reads it, fp32 when the feature projection's LayerNorm does
static size_t hub_esz16(const HubLayout& L, int i) { return i + 1 < L.nc ? 2 : 4; }
static int hub_ws16(const HubLayout& L, int B, int T_audio, HubWs16& W) {
  HubWs W32;
  const int rc = hub_ws(L, B, T_audio, W32);  // (the frame counts and the fp32 path's argument checks)
  if (rc != EDTTS_OK) return rc;
  W = HubWs16{};
  for (int i = 0; i < L.nc; ++i) W.T[i] = W32.T[i];
  W.nch = W32.nch;
  const int T = W.T[L.nc - 1];
  W.Tp = (T + 31) & ~31;
  size_t s0 = 0, s1 = 0;
  for (int i = 0; i < L.nc; ++i) {
    const size_t sz = (size_t)B * W.T[i] * L.C[i] * hub_esz16(L, i);
    if (i % 2 == 0) s0 = sz > s0 ? sz : s0;
    else s1 = sz > s1 ? sz : s1;
  }
  const size_t fp = (size_t)B * T * L.C[L.nc - 1] * 4;
  if (L.nc % 2 == 1) s1 = fp > s1 ? fp : s1;
  else s0 = fp > s0 ? fp : s0;
  const size_t M = (size_t)B * T, wide = (size_t)(3 * L.H > L.I ? 3 * L.H : L.I);
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += al256(n); return at; };
  W.lens = take((size_t)2 * B * 8);
  W.stats = take((size_t)B * L.C[0] * 2 * 4);
  W.part = take((size_t)B * W.nch * L.C[0] * 2 * 8);
  W.buf0 = take(s0);
  W.buf1 = take(s1);
  W.h = take(M * L.H * 4);
  W.att = take(M * L.H * 4);   // the positional conv's output (fp32), then every layer's attention output (bf16)
  W.big = take(M * wide * 2);  // q | k | v rows, then the FFN intermediate (bf16)
  W.vt = take((size_t)B * L.H * W.Tp * 2);
  W.total = o;
  return EDTTS_OK;
}

template <int EPI, bool XBF, bool YBF>
static int hub_gemm16(hipStream_t st, HGemm16Args a, int B, int G, int tile = 0) {
  if (hub_wide_tile(a.M, a.N, G, B, tile)) {  // the rule of hub_gemm: below two 128-tiles per CU the 64-wide tile
    a.ntn = (a.N + 127) / 128;
    hipLaunchKernelGGL((k_hub_gemm16<EPI, 4, XBF, YBF>), dim3((a.M + 127) / 128, a.ntn * G, B), dim3(256), 0, st, a);
  } else {
    a.ntn = (a.N + 63) / 64;
    hipLaunchKernelGGL((k_hub_gemm16<EPI, 2, XBF, YBF>), dim3((a.M + 63) / 64, a.ntn * G, B), dim3(256), 0, st, a);
  }
  LAUNCH_CHECK("k_hub_gemm16");
  return EDTTS_OK;
}
// a plain row-major GEMM: Y[M][N] = epi(X[M][K] W[N][K]^T)
template <int EPI, bool XBF, bool YBF>
static int hub_dense16(hipStream_t st, const void* X, const __bf16* W, const float* bias, void* Y, const float* R, int M, int N, int K,
                       int tile = 0) {
  HGemm16Args a{};
  a.X = X; a.ldrow = K; a.Cin = K; a.stride = 1; a.Tin = M;
  a.W = W; a.K = K; a.bias = bias; a.Y = Y; a.R = R; a.ldy = N; a.M = M; a.N = N;
  return hub_gemm16<EPI, XBF, YBF>(st, a, 1, 1, tile);
}

static int hub_pack16(const HubLayout& L, const void* const* slots, void* packed, hipStream_t st) {
  float* P = (float*)packed;
  const float* const* s = (const float* const*)slots;
  int i = 0;
  auto copy = [&](size_t off, size_t n) -> int {
    HIP_TRY(hipMemcpyAsync(P + off, s[i++], n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return EDTTS_OK;
  };
  auto mat = [&](size_t off, int co, int ci, int k) -> int {
    hipLaunchKernelGGL(k_hub_pack16, dim3(hub_grid((size_t)co * ci * k)), dim3(256), 0, st, s[i++], (__bf16*)(P + off), co, ci, k);
    LAUNCH_CHECK("k_hub_pack16");
    return EDTTS_OK;
  };
  const int H = L.H, CL = L.C[L.nc - 1];
  hipLaunchKernelGGL(k_hub_pack_conv, dim3(hub_grid((size_t)L.C[0] * L.k[0])), dim3(256), 0, st, s[i++], P + L.conv0, 1, L.C[0], L.k[0]);
  LAUNCH_CHECK("k_hub_pack_conv");
  TRY_G(copy(L.gn_w, L.C[0]));
  TRY_G(copy(L.gn_b, L.C[0]));
  for (int c = 1; c < L.nc; ++c) TRY_G(mat(L.conv[c], L.C[c], L.C[c - 1], L.k[c]));
  TRY_G(copy(L.fp_w, CL));
  TRY_G(copy(L.fp_b, CL));
  TRY_G(mat(L.proj_w, H, CL, 1));
  TRY_G(copy(L.proj_b, H));
  TRY_G(mat(L.pos_w, H, L.Cg, L.pk));
  TRY_G(copy(L.pos_b, H));
  TRY_G(copy(L.enc_w, H));
  TRY_G(copy(L.enc_b, H));
  for (int l = 0; l < L.L; ++l) {
    const size_t b0 = (size_t)l * L.layer;
    for (int p = 0; p < 3; ++p) {  // q, k, v -> one [3H][H] matrix and a [3H] bias
      hipLaunchKernelGGL(k_hub_pack16, dim3(hub_grid((size_t)H * H)), dim3(256), 0, st, s[i++],
                         (__bf16*)(P + b0 + L.qkv_w) + (size_t)p * H * H, H, H, 1);
      LAUNCH_CHECK("k_hub_pack16");
      TRY_G(copy(b0 + L.qkv_b + (size_t)p * H, H));
    }
    TRY_G(mat(b0 + L.o_w, H, H, 1));
    TRY_G(copy(b0 + L.o_b, H));
    TRY_G(copy(b0 + L.ln1_w, H));
    TRY_G(copy(b0 + L.ln1_b, H));
    TRY_G(mat(b0 + L.ff1_w, L.I, H, 1));
    TRY_G(copy(b0 + L.ff1_b, L.I));
    TRY_G(mat(b0 + L.ff2_w, H, L.I, 1));
    TRY_G(copy(b0 + L.ff2_b, H));
    TRY_G(copy(b0 + L.ln2_w, H));
    TRY_G(copy(b0 + L.ln2_b, H));
  }
  return EDTTS_OK;
}

// The bf16 forward's launch list, with the stop sites of hub_forward32 (and EDTTS_HUB_VT).
static int hub_forward16(const HubLayout& L, const void* packed, const float* wav, int B, int T_audio, const int64_t* lengths, float* out,
                         void* workspace, hipStream_t st, const HubStop stop = HubStop{}) {
  HubWs16 ws;
  TRY_G(hub_ws16(L, B, T_audio, ws));
  const int tile = stop.tile;
  const float* P = (const float*)packed;
  auto PW = [&](size_t off) { return (const __bf16*)(P + off); };
  char* wb = (char*)workspace;
  const int T = ws.T[L.nc - 1], H = L.H, M = B * T;
  int64_t *len0 = nullptr, *flen = nullptr;
  if (lengths) {
    len0 = (int64_t*)(wb + ws.lens);
    flen = len0 + B;
    ConvGeo geo{};
    geo.n = L.nc;
    for (int i = 0; i < L.nc; ++i) { geo.k[i] = L.k[i]; geo.s[i] = L.s[i]; }
    hipLaunchKernelGGL(k_hub_lens, dim3((B + 63) / 64), dim3(64), 0, st, lengths, B, T_audio, hub_min_samples(L), geo, len0, flen);
    LAUNCH_CHECK("k_hub_lens");
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_LENS, 0);
  }
  float* stats = (float*)(wb + ws.stats);
  void* buf[2] = {wb + ws.buf0, wb + ws.buf1};
  float *h = (float*)(wb + ws.h), *att = (float*)(wb + ws.att);
  __bf16 *att16 = (__bf16*)(wb + ws.att), *big = (__bf16*)(wb + ws.big), *vt = (__bf16*)(wb + ws.vt);
  // conv0 + GroupNorm + GELU -> buf[0] (bf16 when a conv reads it)
  double* part = (double*)(wb + ws.part);
  hipLaunchKernelGGL(k_hub_gn_part, dim3((L.C[0] + 63) / 64, ws.nch, B), dim3(256), 0, st, wav, T_audio, P + L.conv0, L.C[0], L.k[0],
                     L.s[0], len0, ws.T[0], part);
  LAUNCH_CHECK("k_hub_gn_part");
  hipLaunchKernelGGL(k_hub_gn_final, dim3((B * L.C[0] + 255) / 256), dim3(256), 0, st, part, ws.nch, L.C[0], len0, ws.T[0], 1e-5f,
                     P + L.gn_w, P + L.gn_b, stats, B);
  LAUNCH_CHECK("k_hub_gn_final");
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_GNSTAT, 0);
  const dim3 g0(hub_grid((size_t)B * ws.T[0] * L.C[0] / 4));
  if (L.nc > 1) {
    hipLaunchKernelGGL(k_hub_conv0_16, g0, dim3(256), 0, st, wav, T_audio, P + L.conv0, L.C[0], L.k[0], L.s[0], len0, ws.T[0], stats,
                       (__bf16*)buf[0], B);
    LAUNCH_CHECK("k_hub_conv0_16");
  } else {
    hipLaunchKernelGGL(k_hub_conv0, g0, dim3(256), 0, st, wav, T_audio, P + L.conv0, L.C[0], L.k[0], L.s[0], len0, ws.T[0], stats,
                       (float*)buf[0], B);
    LAUNCH_CHECK("k_hub_conv0");
  }
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_CONV0, 0);
  for (int c = 1; c < L.nc; ++c) {
    HGemm16Args a{};
    a.X = buf[(c - 1) & 1]; a.xbs = (long long)ws.T[c - 1] * L.C[c - 1]; a.ldrow = L.C[c - 1]; a.Cin = L.C[c - 1]; a.stride = L.s[c];
    a.Tin = ws.T[c - 1];
    a.W = PW(L.conv[c]); a.K = L.k[c] * L.C[c - 1];
    a.Y = buf[c & 1]; a.ybs = (long long)ws.T[c] * L.C[c]; a.ldy = L.C[c]; a.M = ws.T[c]; a.N = L.C[c];
    if (c + 1 < L.nc) TRY_G((hub_gemm16<HEPI_GELU, true, true>(st, a, B, 1, tile)));
    else TRY_G((hub_gemm16<HEPI_GELU, true, false>(st, a, B, 1, tile)));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_CONV, c);
  }
  // feature projection: LayerNorm (fp32) -> Linear (+ bias) -> h
  const int CL = L.C[L.nc - 1];
  float* feat = (float*)buf[(L.nc - 1) & 1];
  float* fn = (float*)buf[L.nc & 1];
  TRY_G(hub_norm(st, feat, fn, M, CL, P + L.fp_w, P + L.fp_b, L.eps));
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_FPNORM, 0);
  TRY_G((hub_dense16<HEPI_BIAS, false, false>(st, fn, PW(L.proj_w), P + L.proj_b, h, nullptr, M, H, CL, tile)));
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_FPROJ, 0);
  {
    HGemm16Args a{};
    a.X = h; a.xbs = (long long)T * H; a.ldrow = H; a.Cin = L.Cg; a.stride = 1; a.pad = L.pk / 2; a.xg = L.Cg;
    a.nvalid = flen; a.Tin = T;
    a.W = PW(L.pos_w); a.K = L.pk * L.Cg; a.bias = P + L.pos_b;
    a.Y = att; a.R = h; a.ybs = (long long)T * H; a.ldy = H; a.M = T; a.N = L.Cg;
    TRY_G((hub_gemm16<HEPI_GELU_RESID, false, false>(st, a, B, L.pg, tile)));
  }
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_POS, 0);
  TRY_G(hub_norm(st, att, L.L ? h : out, M, H, P + L.enc_w, P + L.enc_b, L.eps));
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_ENCNORM, 0);
  HAttn16Args aa{big, vt, att16, flen, H, L.heads, L.DH, T, ws.Tp, 1.4426950408889634f / sqrtf((float)L.DH)};
  for (int l = 0; l < L.L; ++l) {
    const size_t y = (size_t)l * L.layer;
    TRY_G((hub_dense16<HEPI_BIAS, false, true>(st, h, PW(y + L.qkv_w), P + y + L.qkv_b, big, nullptr, M, 3 * H, H, tile)));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_QKV, l);
    hipLaunchKernelGGL(k_hub_vt, dim3(ws.Tp / 32, L.heads, B), dim3(256), 0, st, aa);
    LAUNCH_CHECK("k_hub_vt");
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_VT, l);
    const dim3 grid((T + 63) / 64, L.heads, B);
    TRY_G(with_head_tiles<8>(L.DH, [&](auto dt) -> int {  // head_dim = 32 KT: an even count of 16-wide tiles (hub_layout16)
      constexpr int DT = decltype(dt)::value;
      if constexpr (DT % 2 == 0) {
        hipLaunchKernelGGL(k_hub_attn16<DT / 2>, grid, dim3(256), 0, st, aa);
        LAUNCH_CHECK("k_hub_attn16");
        return EDTTS_OK;
      } else {
        return fail(EDTTS_ERR_UNSUPPORTED, "head_dim=%d: compute_dtype bf16 needs a multiple of 32 up to 128", L.DH);
      }
    }));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_ATTN, l);
    TRY_G((hub_dense16<HEPI_RESID, true, false>(st, att16, PW(y + L.o_w), P + y + L.o_b, h, h, M, H, H, tile)));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_OPROJ, l);
    TRY_G(hub_norm(st, h, h, M, H, P + y + L.ln1_w, P + y + L.ln1_b, L.eps));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_LN1, l);
    TRY_G((hub_dense16<HEPI_GELU, false, true>(st, h, PW(y + L.ff1_w), P + y + L.ff1_b, big, nullptr, M, L.I, H, tile)));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_FF1, l);
    TRY_G((hub_dense16<HEPI_RESID, true, false>(st, big, PW(y + L.ff2_w), P + y + L.ff2_b, h, h, M, H, L.I, tile)));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_FF2, l);
    TRY_G(hub_norm(st, h, l + 1 < L.L ? h : out, M, H, P + y + L.ln2_w, P + y + L.ln2_b, L.eps));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_LN2, l);
  }
  if (flen) {
    hipLaunchKernelGGL(k_hub_zero_past, dim3(hub_grid((size_t)M * H / 4)), dim3(256), 0, st, out, flen, B, T, H);
    LAUNCH_CHECK("k_hub_zero_past");
  }
  return EDTTS_OK;
}

static int hub_dtype(int compute_dtype) {
  if (compute_dtype != EDTTS_HUBERT_FP32 && compute_dtype != EDTTS_HUBERT_BF16)
    return fail(EDTTS_ERR_ARG, "compute_dtype=%d: expected EDTTS_HUBERT_FP32 (0) or EDTTS_HUBERT_BF16 (1)", compute_dtype);
  return EDTTS_OK;
}

}  // namespace edtts_hub

extern "C" {

int edtts_hubert_packed_bytes_dt(const EdttsHubertDims* dims, int compute_dtype, size_t* out_bytes) {
  TRY_G(edtts_hub::hub_dtype(compute_dtype));
  if (compute_dtype == EDTTS_HUBERT_FP32) return edtts_hubert_packed_bytes(dims, out_bytes);
  edtts_hub::HubLayout L;
  TRY_G(edtts_hub::hub_layout16(dims, L));
  if (!out_bytes) return fail(EDTTS_ERR_ARG, "out_bytes is NULL");
  *out_bytes = L.total * sizeof(float);
  return EDTTS_OK;
}

int edtts_hubert_workspace_bytes_dt(const EdttsHubertDims* dims, int compute_dtype, int B, int T_audio, size_t* out_bytes) {
  TRY_G(edtts_hub::hub_dtype(compute_dtype));
  if (compute_dtype == EDTTS_HUBERT_FP32) return edtts_hubert_workspace_bytes(dims, B, T_audio, out_bytes);
  edtts_hub::HubLayout L;
  TRY_G(edtts_hub::hub_layout16(dims, L));
  if (!out_bytes) return fail(EDTTS_ERR_ARG, "out_bytes is NULL");
  if (B < 1 || T_audio < 1) return fail(EDTTS_ERR_ARG, "B=%d T_audio=%d: need >= 1", B, T_audio);
  edtts_hub::HubWs16 W;
  TRY_G(edtts_hub::hub_ws16(L, B, T_audio, W));
  *out_bytes = W.total;
  return EDTTS_OK;
}

int edtts_hubert_pack_dt(const EdttsHubertDims* dims, int compute_dtype, const void* const* slots, int n_slots, void* packed, void* stream) {
  using namespace edtts_hub;
  TRY_G(hub_dtype(compute_dtype));
  if (compute_dtype == EDTTS_HUBERT_FP32) return edtts_hubert_pack(dims, slots, n_slots, packed, stream);
  HubLayout L;
  TRY_G(hub_layout16(dims, L));
  const int want = 3 + (L.nc - 1) + 8 + 16 * L.L;
  if (!slots || !packed) return fail(EDTTS_ERR_ARG, "slots/packed is NULL");
  if (n_slots != want) return fail(EDTTS_ERR_ARG, "expected %d weight slots, got %d", want, n_slots);
  for (int i = 0; i < n_slots; ++i)
    if (!slots[i]) return fail(EDTTS_ERR_ARG, "weight slot %d is NULL", i);
  if (!hub_al16(packed)) return fail(EDTTS_ERR_ARG, "packed must be 16-byte aligned");
  return hub_pack16(L, slots, packed, (hipStream_t)stream);
}

int edtts_hubert_forward_dt(const EdttsHubertDims* dims, int compute_dtype, const void* packed, const float* wav, int B, int T_audio,
                            const int64_t* lengths, float* out, void* workspace, void* stream) {
  using namespace edtts_hub;
  TRY_G(hub_dtype(compute_dtype));
  if (compute_dtype == EDTTS_HUBERT_FP32) return edtts_hubert_forward(dims, packed, wav, B, T_audio, lengths, out, workspace, stream);
  HubLayout L;
  TRY_G(hub_layout16(dims, L));
  if (!packed || !wav || !out || !workspace) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (B < 1 || T_audio < 1) return fail(EDTTS_ERR_ARG, "B=%d T_audio=%d: need >= 1", B, T_audio);
  if (!hub_al16(packed) || !hub_al16(out) || !hub_al16(workspace)) return fail(EDTTS_ERR_ARG, "packed, out and workspace must be 16-byte aligned");
  return hub_forward16(L, packed, wav, B, T_audio, lengths, out, workspace, (hipStream_t)stream);
}

int edtts_hubert_forward_until(const EdttsHubertDims* dims, int compute_dtype, const void* packed, const float* wav, int B, int T_audio,
                               const int64_t* lengths, float* out, void* workspace, int stop_site, int stop_index, int tile, void* stream) {
  using namespace edtts_hub;
  TRY_G(hub_dtype(compute_dtype));
  const bool bf16 = compute_dtype == EDTTS_HUBERT_BF16;
  HubLayout L;
  TRY_G(bf16 ? hub_layout16(dims, L) : hub_layout(dims, L));
  if (!packed || !wav || !out || !workspace) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (B < 1 || T_audio < 1) return fail(EDTTS_ERR_ARG, "B=%d T_audio=%d: need >= 1", B, T_audio);
  if (!hub_al16(packed) || !hub_al16(out) || !hub_al16(workspace)) return fail(EDTTS_ERR_ARG, "packed, out and workspace must be 16-byte aligned");
  HubStop stop;
  stop.site = stop_site; stop.index = stop_index; stop.tile = tile;
  TRY_G(hub_stop_check(L, bf16, lengths != nullptr, stop));
  if (bf16) return hub_forward16(L, packed, wav, B, T_audio, lengths, out, workspace, (hipStream_t)stream, stop);
  return hub_forward32(L, packed, wav, B, T_audio, lengths, out, workspace, (hipStream_t)stream, stop);
}

int edtts_hubert_workspace_region(const EdttsHubertDims* dims, int compute_dtype, int B, int T_audio, int which, size_t* offset_bytes,
                                  size_t* bytes) {
  using namespace edtts_hub;
  TRY_G(hub_dtype(compute_dtype));
  const bool bf16 = compute_dtype == EDTTS_HUBERT_BF16;
  HubLayout L;
  TRY_G(bf16 ? hub_layout16(dims, L) : hub_layout(dims, L));
  if (!offset_bytes || !bytes) return fail(EDTTS_ERR_ARG, "offset_bytes/bytes is NULL");
  if (B < 1 || T_audio < 1) return fail(EDTTS_ERR_ARG, "B=%d T_audio=%d: need >= 1", B, T_audio);
  // the members' offsets in layout order, closed by the total: a member reaches up to the next one's offset
  size_t at[EDTTS_HUB_WS_COUNT + 1];
  int n = 0;
  if (bf16) {
    HubWs16 W;
    TRY_G(hub_ws16(L, B, T_audio, W));
    const size_t o[] = {W.lens, W.stats, W.part, W.buf0, W.buf1, W.h, W.att, W.big, W.vt, W.total};
    for (size_t v : o) at[n++] = v;
  } else {
    HubWs W;
    TRY_G(hub_ws(L, B, T_audio, W));
    const size_t o[] = {W.lens, W.stats, W.part, W.buf0, W.buf1, W.h, W.att, W.big, W.total};
    for (size_t v : o) at[n++] = v;
  }
  if (which < 0 || which >= n - 1)
    return fail(EDTTS_ERR_ARG, "edtts_hubert_workspace_region: which=%d: expected an EDTTS_HUB_WS_* member in [0, %d)%s", which, n - 1,
                bf16 ? "" : " (EDTTS_HUB_WS_VT exists only under EDTTS_HUBERT_BF16)");
  *offset_bytes = at[which];
  *bytes = at[which + 1] - at[which];
  return EDTTS_OK;
}

}  // extern "C"
