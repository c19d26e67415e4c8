// edtts_hubert.h -- the HuBERT backbone forward: 16 kHz waveform -> hidden_states[num_layers] (included by edtts_kernels.hip).
// The fp32 kernels and what both compute dtypes share; the bf16 kernels are in edtts_hubert16.h, the host side (layout, workspace,
// packing, the launch list, the entry points) in edtts_hubert_host.h.
//
// transformers' HubertModel (feat_extract_norm = "group", post-LN encoder: the hubert-base layout) in eval mode, fp32:
//   conv0  Conv1d(1, C0, k0, s0) -> GroupNorm(C0, C0) -> GELU       k_hub_gn_part + k_hub_gn_final (per-utterance statistics, fp64,
//                                                                    fixed order)
//                                                                    + k_hub_conv0 (recomputes the conv, normalises, GELU, stores)
//   conv_i Conv1d(C_{i-1}, C_i, k_i, s_i) -> GELU                    k_hub_gemm<HEPI_GELU>: implicit GEMM, K = k_i C_{i-1}
//   feature projection LayerNorm(C_last) -> Linear(C_last, H)        k_gen_norm<NORM_LAYER> + k_hub_gemm<HEPI_BIAS>
//   h += GELU(pos_conv(h)), LayerNorm                                k_hub_gemm<HEPI_GELU_RESID> per group (K = pos_k x H / groups)
//   num_layers x post-LN layer: QKV, attention, out_proj + residual, LayerNorm, FFN (GELU) + residual, LayerNorm
//                                                                    k_hub_gemm, k_gen_attn<DT> (window -1), k_gen_norm
//   rows past each utterance's frame count -> 0                      k_hub_zero_past
//
// Activations are time-major [B][T][C].  The im2col row of output frame t of a conv with stride s is then the span of rows
// s t .. s t + k - 1, i.e. K = k C contiguous floats at row stride s C: every conv after the first is a GEMM against the weight
// packed [co][k][ci] (k_hub_pack_conv).  The positional conv is the same with stride 1, padding pos_k / 2 and one GEMM per group
// (the group's 48 input channels at column offset 48 g), zero rows outside [0, frames_b) -- its own end for each utterance.
//
// k_hub_gemm: Y = epi(X W^T) on v_mfma_f32_16x16x4_f32; block tile 32 TW x 32 TW (TW = 4: 128 x 128, TW = 2: 64 x 64 for grids too
// small to fill the device, or N <= 64), four waves of 16 TW x 16 TW, K tiles of 16 staged global -> registers -> LDS ([row][k], padded to 20
// floats) with the next tile's loads in flight during the current tile's MFMAs (two LDS buffers, one barrier per K tile).  Within a
// 16-wide k-block lane group g holds k = 4 g .. 4 g + 3 (one ds_read_b128 per operand serves four MFMA steps).  Every output element
// is the same k-ordered chain whatever its tile, its tile size or the batch it is in: results are bitwise independent of B, T and TW.
namespace edtts_hub {

constexpr int kMaxConv = 16;  // feature-encoder conv layers
constexpr int kMaxK0 = 64;    // conv0 kernel width (taps staged in LDS)
constexpr int kBK = 16;       // GEMM K tile
constexpr int kLDK = kBK + 4; // LDS row pitch (floats): conflict-free b128 fragment reads

enum { HEPI_BIAS = 0, HEPI_GELU = 1, HEPI_RESID = 2, HEPI_GELU_RESID = 3 };

EDTTS_DEV float gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

struct HGemmArgs {
  const float* X;            // utterance b, group g, row r, channel c: X[b xbs + r ldrow + g xg + c]
  long long xbs;
  int ldrow, Cin, stride, pad, xg;
  const int64_t* nvalid;     // input rows of utterance b that exist (others read as 0): nvalid[b], or Tin for all
  int Tin;
  const float* W;            // [G][N][K], K contiguous
  int K;
  const float* bias;         // [G][N] or null
  float* Y;                  // Y[b ybs + m ldy + g N + n]
  const float* R;            // residual, same indexing as Y (may be Y)
  long long ybs;
  int ldy, M, N, ntn;        // ntn: N tiles per group
};

// X row m of the implicit GEMM reads input row m stride + tap - pad, channel ci, for k = tap Cin + ci (Cin % 4 == 0: a 4-wide k
// chunk never straddles two taps).  TW: 16 x 16 sub-tiles per wave along M and along N.
template <int EPI, int TW>
__global__ __launch_bounds__(256) void k_hub_gemm(HGemmArgs a) {
  constexpr int BT = 32 * TW;
  __shared__ float lds[2][2][BT][kLDK];  // [buffer][X | W][row][k]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fq = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, grp = blockIdx.y / a.ntn, n0 = (blockIdx.y - grp * a.ntn) * BT, m0 = blockIdx.x * BT;
  const float* X = a.X + (size_t)b * a.xbs + (size_t)grp * a.xg;
  const float* W = a.W + (size_t)grp * a.N * a.K;
  const int nval = a.nvalid ? (int)a.nvalid[b] : a.Tin;
  // loader: rows lr + 64 i (i < TW / 2) of both operands, k offset lk of the tile
  constexpr int NL = TW / 2;
  const int lr = tid >> 2, lk = 4 * (tid & 3);
  int tap = lk / a.Cin, ci = lk - tap * a.Cin;
  const int wm = 16 * TW * (w >> 1), wn = 16 * TW * (w & 1);
  f4 acc[TW][TW];
#pragma unroll
  for (int t = 0; t < TW; ++t)
#pragma unroll
    for (int u = 0; u < TW; ++u) acc[t][u] = splat(0.f);
  f4 xv[NL], wv[NL];
  auto load = [&](int k0) {
    const bool kok = k0 + lk < a.K;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int m = m0 + lr + 64 * i, src = m * a.stride + tap - a.pad;
      xv[i] = (kok && m < a.M && src >= 0 && src < nval) ? ldg4(X + (size_t)src * a.ldrow + ci) : splat(0.f);
      const int n = n0 + lr + 64 * i;
      wv[i] = (kok && n < a.N) ? ldg4(W + (size_t)n * a.K + k0 + lk) : splat(0.f);
    }
    ci += kBK;
    while (ci >= a.Cin) { ci -= a.Cin; ++tap; }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      *reinterpret_cast<f4*>(&lds[buf][0][lr + 64 * i][lk]) = xv[i];
      *reinterpret_cast<f4*>(&lds[buf][1][lr + 64 * i][lk]) = wv[i];
    }
  };
  const int nk = (a.K + kBK - 1) / kBK;
  load(0);
  store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load((kt + 1) * kBK);
    f4 fa[TW], fb[TW];
#pragma unroll
    for (int t = 0; t < TW; ++t) fa[t] = *reinterpret_cast<const f4*>(&lds[buf][1][wn + 16 * t + fq][4 * g]);
#pragma unroll
    for (int u = 0; u < TW; ++u) fb[u] = *reinterpret_cast<const f4*>(&lds[buf][0][wm + 16 * u + fq][4 * g]);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int u = 0; u < TW; ++u) acc[t][u] = EDTTS_MFMA(fa[t][s], fb[u][s], acc[t][u]);
    if (kt + 1 < nk) store(buf ^ 1);
    __syncthreads();
  }
  // epilogue: acc[t][u] lane (g, fq) holds Y[m = m0 + wm + 16 u + fq][n = n0 + wn + 16 t + 4 g + r]
  float* Y = a.Y + (size_t)b * a.ybs + (size_t)grp * a.N;
  const float* R = a.R ? a.R + (size_t)b * a.ybs + (size_t)grp * a.N : nullptr;
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
      stg4(Y + off, o);
    }
  }
}

// ---- per-utterance frame counts ----------------------------------------------------------------------------------------------
struct ConvGeo {
  int n, k[kMaxConv], s[kMaxConv];
};
EDTTS_DEV int conv_out(int n, int k, int s) {  // torch.div(n - k, s, rounding_mode="floor") + 1, at least 0
  const int d = n - k;
  const int q = d >= 0 ? d / s : -((-d + s - 1) / s);
  return q + 1 > 0 ? q + 1 : 0;
}
// lengths (samples) clamped into [n_min, T_audio] -> conv0 frames len0[b] and output frames flen[b]
__global__ void k_hub_lens(const int64_t* len, int B, int T_audio, int n_min, ConvGeo geo, int64_t* len0, int64_t* flen) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int64_t v = len[b];
  int n = v < n_min ? n_min : (v > T_audio ? T_audio : (int)v);
  for (int i = 0; i < geo.n; ++i) {
    n = conv_out(n, geo.k[i], geo.s[i]);
    if (i == 0) len0[b] = n;
  }
  flen[b] = n;
}

// ---- conv0 + GroupNorm -------------------------------------------------------------------------------------------------------
// Statistics in two passes with a fixed order.  k_hub_gn_part: one block per (64 channels, chunk of kGnChunk frames, utterance), lane
// = channel, wave w sums frames w, w + 4, ... of the chunk in fp64 and the four partials add in wave order.  k_hub_gn_final: per
// (utterance, channel) the chunks add in chunk order.  The order depends on the utterance's frame count only -- not on B, the
// padded length or the grid -- and there are no float atomics.
constexpr int kGnChunk = 256;
__global__ __launch_bounds__(256) void k_hub_gn_part(const float* wav, int T_audio, const float* w0, int C0, int k0, int s0,
                                                     const int64_t* len0, int T0, double* part) {
  __shared__ float wt[64][kMaxK0 + 1];
  __shared__ double red[4][64][2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ch = blockIdx.y, b = blockIdx.z, c = blockIdx.x * 64 + lane;
  for (int i = tid; i < 64 * k0; i += 256) {
    const int cc = blockIdx.x * 64 + i / k0;
    wt[i / k0][i % k0] = cc < C0 ? w0[(size_t)(i % k0) * C0 + cc] : 0.f;
  }
  __syncthreads();
  const int F = len0 ? (int)len0[b] : T0;
  const int t1 = min(F, (ch + 1) * kGnChunk);
  const float* x = wav + (size_t)b * T_audio;
  double s = 0.0, q = 0.0;
  for (int t = ch * kGnChunk + wv; t < t1; t += 4) {
    const float* xp = x + (size_t)t * s0;
    float y = 0.f;
    for (int j = 0; j < k0; ++j) y = fmaf(wt[lane][j], xp[j], y);
    s += (double)y;
    q += (double)y * (double)y;
  }
  red[wv][lane][0] = s;
  red[wv][lane][1] = q;
  __syncthreads();
  if (wv == 0 && c < C0) {
    double* pp = part + (((size_t)b * gridDim.y + ch) * C0 + c) * 2;
    pp[0] = red[0][lane][0] + red[1][lane][0] + red[2][lane][0] + red[3][lane][0];
    pp[1] = red[0][lane][1] + red[1][lane][1] + red[2][lane][1] + red[3][lane][1];
  }
}
// stats [B][2][C0]: scale = gamma rstd and shift = beta - mean scale, so that conv0's epilogue is one FMA per element
__global__ __launch_bounds__(256) void k_hub_gn_final(const double* part, int nch, int C0, const int64_t* len0, int T0, float eps,
                                                      const float* gamma, const float* beta, float* stats, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C0) return;
  const int b = i / C0, c = i - b * C0;
  const int F = len0 ? (int)len0[b] : T0, n = (F + kGnChunk - 1) / kGnChunk;
  double s = 0.0, q = 0.0;
  for (int ch = 0; ch < n; ++ch) {
    const double* pp = part + (((size_t)b * nch + ch) * C0 + c) * 2;
    s += pp[0];
    q += pp[1];
  }
  const double mean = s / F, var = fmax(q / F - mean * mean, 0.0);
  const double sc = (double)gamma[c] / sqrt(var + (double)eps);
  stats[(size_t)b * 2 * C0 + c] = (float)sc;
  stats[(size_t)b * 2 * C0 + C0 + c] = (float)((double)beta[c] - mean * sc);
}
// y[b][t][c] = GELU(conv0(x)[t][c] scale + shift), four channels per thread (the weights packed [k0][C0]: one 16-byte load per tap);
// frames past len0[b] are 0 (their samples are not read)
__global__ __launch_bounds__(256) void k_hub_conv0(const float* wav, int T_audio, const float* w0, int C0, int k0, int s0,
                                                   const int64_t* len0, int T0, const float* stats, float* y, int B) {
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
    stg4(y + (size_t)row * C0 + c, o);
  }
}

// ---- packing and the tail --------------------------------------------------------------------------------------------------------
// conv weight [co][ci][k] (state dict) -> [co][k][ci]
__global__ __launch_bounds__(256) void k_hub_pack_conv(const float* src, float* dst, int co, int ci, int k) {
  const size_t n = (size_t)co * ci * k;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % ci);
    const size_t r = i / ci;
    const int j = (int)(r % k);
    const size_t o = r / k;
    dst[i] = src[(o * ci + c) * k + j];
  }
}
__global__ __launch_bounds__(256) void k_hub_zero_past(float* y, const int64_t* flen, int B, int T, int H) {
  const int H4 = H / 4;
  const size_t n = (size_t)B * T * H4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / H4;
    const int b = (int)(row / T), t = (int)(row - (size_t)b * T);
    if (t >= (int)flen[b]) stg4(y + 4 * i, splat(0.f));
  }
}

}  // namespace edtts_hub
