// edtts_hubert16.h -- the kernels of the HuBERT backbone's bf16 compute path (included by edtts_kernels.hip after edtts_hubert.h;
// edtts_hubert_host.h launches them).
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

}  // namespace edtts_hub
