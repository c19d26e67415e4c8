// edtts_hubert.h -- the HuBERT backbone forward: 16 kHz waveform -> hidden_states[num_layers] (included by edtts_kernels.hip).
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

// ---- host side: layouts ---------------------------------------------------------------------------------------------------------
struct HubLayout {
  int nc, C[kMaxConv], k[kMaxConv], s[kMaxConv];
  int H, heads, DH, I, L, pk, pg, Cg;
  float eps;
  size_t conv0, gn_w, gn_b, conv[kMaxConv], fp_w, fp_b, proj_w, proj_b, pos_w, pos_b, enc_w, enc_b;
  size_t qkv_w, qkv_b, o_w, o_b, ln1_w, ln1_b, ff1_w, ff1_b, ff2_w, ff2_b, ln2_w, ln2_b, layer;  // offsets inside layer 0; stride `layer`
  size_t total;  // floats
};
static size_t al64(size_t n) { return (n + 63) & ~(size_t)63; }  // 256-byte alignment of every tensor

static int hub_layout(const EdttsHubertDims* d, HubLayout& L) {
  if (!d) return fail(EDTTS_ERR_ARG, "hubert dims is NULL");
  L = HubLayout{};
  if (d->n_conv < 1 || d->n_conv > kMaxConv) return fail(EDTTS_ERR_UNSUPPORTED, "conv_dim: %d layers, need 1..%d", d->n_conv, kMaxConv);
  L.nc = d->n_conv;
  for (int i = 0; i < L.nc; ++i) {
    L.C[i] = d->conv_dim[i]; L.k[i] = d->conv_kernel[i]; L.s[i] = d->conv_stride[i];
    if (L.C[i] < 4 || L.C[i] % 4 || L.C[i] > 8192) return fail(EDTTS_ERR_UNSUPPORTED, "conv_dim[%d]=%d: need a multiple of 4 in [4, 8192]", i, L.C[i]);
    if (L.k[i] < 1 || L.k[i] > (i ? 1024 : kMaxK0)) return fail(EDTTS_ERR_UNSUPPORTED, "conv_kernel[%d]=%d out of [1, %d]", i, L.k[i], i ? 1024 : kMaxK0);
    if (L.s[i] < 1 || L.s[i] > 1024) return fail(EDTTS_ERR_UNSUPPORTED, "conv_stride[%d]=%d out of [1, 1024]", i, L.s[i]);
  }
  L.H = d->hidden; L.heads = d->heads; L.I = d->intermediate; L.L = d->num_layers; L.pk = d->pos_kernel; L.pg = d->pos_groups;
  L.eps = d->layer_norm_eps;
  if (L.H < 4 || L.H % 4 || L.H > 8192) return fail(EDTTS_ERR_UNSUPPORTED, "hidden_size=%d: need a multiple of 4 in [4, 8192]", L.H);
  if (L.heads < 1 || L.H % L.heads) return fail(EDTTS_ERR_UNSUPPORTED, "num_attention_heads=%d does not divide hidden_size=%d", L.heads, L.H);
  L.DH = L.H / L.heads;
  if (L.DH > 128) return fail(EDTTS_ERR_UNSUPPORTED, "head_dim=%d > 128 (hidden_size=%d, num_attention_heads=%d)", L.DH, L.H, L.heads);
  if (L.I < 4 || L.I % 4 || L.I > 65536) return fail(EDTTS_ERR_UNSUPPORTED, "intermediate_size=%d: need a multiple of 4 in [4, 65536]", L.I);
  if (L.L < 0 || L.L > 256) return fail(EDTTS_ERR_UNSUPPORTED, "num_layers=%d out of [0, 256]", L.L);
  if (L.pg < 1 || L.H % L.pg || (L.H / L.pg) % 4)
    return fail(EDTTS_ERR_UNSUPPORTED, "num_conv_pos_embedding_groups=%d: need hidden_size / groups a multiple of 4", L.pg);
  if (L.pk < 1 || L.pk > 1024) return fail(EDTTS_ERR_UNSUPPORTED, "num_conv_pos_embeddings=%d out of [1, 1024]", L.pk);
  if (!(L.eps > 0.f)) return fail(EDTTS_ERR_UNSUPPORTED, "layer_norm_eps=%g: need > 0", (double)L.eps);
  L.Cg = L.H / L.pg;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += al64(n); return at; };
  L.conv0 = take((size_t)L.C[0] * L.k[0]);
  L.gn_w = take(L.C[0]);
  L.gn_b = take(L.C[0]);
  for (int i = 1; i < L.nc; ++i) L.conv[i] = take((size_t)L.C[i] * L.k[i] * L.C[i - 1]);
  const int CL = L.C[L.nc - 1];
  L.fp_w = take(CL); L.fp_b = take(CL);
  L.proj_w = take((size_t)L.H * CL); L.proj_b = take(L.H);
  L.pos_w = take((size_t)L.H * L.pk * L.Cg); L.pos_b = take(L.H);
  L.enc_w = take(L.H); L.enc_b = take(L.H);
  const size_t l0 = o;
  L.qkv_w = take((size_t)3 * L.H * L.H) - l0; L.qkv_b = take(3 * L.H) - l0;
  L.o_w = take((size_t)L.H * L.H) - l0; L.o_b = take(L.H) - l0;
  L.ln1_w = take(L.H) - l0; L.ln1_b = take(L.H) - l0;
  L.ff1_w = take((size_t)L.I * L.H) - l0; L.ff1_b = take(L.I) - l0;
  L.ff2_w = take((size_t)L.H * L.I) - l0; L.ff2_b = take(L.H) - l0;
  L.ln2_w = take(L.H) - l0; L.ln2_b = take(L.H) - l0;
  L.layer = o - l0;
  L.qkv_w += l0; L.qkv_b += l0; L.o_w += l0; L.o_b += l0; L.ln1_w += l0; L.ln1_b += l0;
  L.ff1_w += l0; L.ff1_b += l0; L.ff2_w += l0; L.ff2_b += l0; L.ln2_w += l0; L.ln2_b += l0;
  L.total = l0 + (size_t)L.L * L.layer;
  return EDTTS_OK;
}
static int hub_frames(const HubLayout& L, long long n) {
  for (int i = 0; i < L.nc; ++i) {
    const long long d = n - L.k[i];
    const long long q = d >= 0 ? d / L.s[i] : -((-d + L.s[i] - 1) / L.s[i]);
    n = q + 1 > 0 ? q + 1 : 0;
  }
  return (int)n;
}
static int hub_min_samples(const HubLayout& L) {  // the shortest input with one output frame
  long long r = 1;
  for (int i = L.nc - 1; i >= 0; --i) r = (r - 1) * L.s[i] + L.k[i];
  return (int)(r > 0x7fffffff ? 0x7fffffff : r);
}

struct HubWs {
  int T[kMaxConv];
  int nch;
  size_t lens, stats, part, buf0, buf1, h, att, big, total;  // bytes
};
static size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }
static int hub_ws(const HubLayout& L, int B, int T_audio, HubWs& W) {
  W = HubWs{};
  long long n = T_audio;
  for (int i = 0; i < L.nc; ++i) {
    const long long d = n - L.k[i];
    n = d < 0 ? 0 : d / L.s[i] + 1;
    W.T[i] = (int)n;
  }
  const int T = W.T[L.nc - 1];
  if (T < 1) return fail(EDTTS_ERR_ARG, "T_audio=%d gives no output frame (need at least %d samples)", T_audio, hub_min_samples(L));
  if ((long long)B * W.T[0] * L.C[0] >= 0x7fffffffLL) return fail(EDTTS_ERR_ARG, "B=%d x T_audio=%d: conv0 output too large", B, T_audio);
  size_t s0 = 0, s1 = 0;
  for (int i = 0; i < L.nc; ++i) {
    const size_t sz = (size_t)B * W.T[i] * L.C[i] * 4;
    if (i % 2 == 0) s0 = sz > s0 ? sz : s0;
    else s1 = sz > s1 ? sz : s1;
  }
  const size_t fp = (size_t)B * T * L.C[L.nc - 1] * 4;  // the feature projection's LayerNorm output: in the buffer the last conv did not write
  if (L.nc % 2 == 1) s1 = fp > s1 ? fp : s1;
  else s0 = fp > s0 ? fp : s0;
  const size_t M = (size_t)B * T, wide = (size_t)(3 * L.H > L.I ? 3 * L.H : L.I);
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += al256(n); return at; };
  W.lens = take((size_t)2 * B * 8);
  W.stats = take((size_t)B * L.C[0] * 2 * 4);
  W.nch = (W.T[0] + kGnChunk - 1) / kGnChunk;
  W.part = take((size_t)B * W.nch * L.C[0] * 2 * 8);
  W.buf0 = take(s0);
  W.buf1 = take(s1);
  W.h = take(M * L.H * 4);
  W.att = take(M * L.H * 4);
  W.big = take(M * wide * 4);
  W.total = o;
  return EDTTS_OK;
}

static bool hub_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static unsigned hub_grid(size_t n) { const size_t nb = (n + 255) / 256; return (unsigned)(nb > 8192 ? 8192 : (nb < 1 ? 1 : nb)); }

// Where a forward stops (edtts_hubert_forward_until): after the last launch of site `site` (EDTTS_HUB_*, include/edtts.h) with index
// `index`; site < 0: never.  tile: 0 = hub_gemm's own rule, 2 | 4 = that TW for every GEMM launch of the call.
struct HubStop {
  int site = -1, index = 0, tile = 0;
};
static bool hub_wide_tile(int M, int N, int G, int B, int tile) {
  const int n_sm = 256;  // MI355X compute units: below two 128-tiles per CU the 64-wide tile (4x the blocks) is used
  const long long big = (long long)((M + 127) / 128) * ((N + 127) / 128) * G * B;
  if (tile) return tile == 4;
  return big >= 2 * n_sm && N > 64;  // (N <= 64, the positional conv's groups: a 128-wide tile would be half empty)
}

template <int EPI>
static int hub_gemm(hipStream_t st, HGemmArgs a, int B, int G, int tile = 0) {
  if (hub_wide_tile(a.M, a.N, G, B, tile)) {
    a.ntn = (a.N + 127) / 128;
    hipLaunchKernelGGL((k_hub_gemm<EPI, 4>), dim3((a.M + 127) / 128, a.ntn * G, B), dim3(256), 0, st, a);
  } else {
    a.ntn = (a.N + 63) / 64;
    hipLaunchKernelGGL((k_hub_gemm<EPI, 2>), dim3((a.M + 63) / 64, a.ntn * G, B), dim3(256), 0, st, a);
  }
  LAUNCH_CHECK("k_hub_gemm");
  return EDTTS_OK;
}
// a plain row-major GEMM: Y[M][ldy] = epi(X[M][K] W[N][K]^T)
template <int EPI>
static int hub_dense(hipStream_t st, const float* X, const float* W, const float* bias, float* Y, const float* R, int M, int N, int K,
                     int tile = 0) {
  HGemmArgs a{};
  a.X = X; a.ldrow = K; a.Cin = K; a.stride = 1; a.Tin = M;
  a.W = W; a.K = K; a.bias = bias; a.Y = Y; a.R = R; a.ldy = N; a.M = M; a.N = N;
  return hub_gemm<EPI>(st, a, 1, 1, tile);
}
static int hub_norm(hipStream_t st, const float* x, float* y, int rows, int W, const float* g, const float* b, float eps) {
  edtts_gen::NormArgs a{x, y, g, b, nullptr, rows, W, W, 1, 0, eps};
  hipLaunchKernelGGL(edtts_gen::k_gen_norm<edtts_gen::NORM_LAYER>, dim3((rows + 3) / 4), dim3(256), 0, st, a);
  LAUNCH_CHECK("k_gen_norm");
  return EDTTS_OK;
}

static const char* const kHubSiteNames[EDTTS_HUB_COUNT] = {"LENS", "GNSTAT", "CONV0", "CONV", "FPNORM", "FPROJ", "POS", "ENCNORM", "QKV",
                                                           "VT", "ATTN", "OPROJ", "LN1", "FF1", "FF2", "LN2", "ZERO"};
// a stop that names a site the call does not have is refused (the forward would otherwise run to its end unnoticed)
static int hub_stop_check(const HubLayout& L, bool bf16, bool with_lengths, const HubStop& s) {
  const char* fn = "edtts_hubert_forward_until";
  if (s.tile != 0 && s.tile != 2 && s.tile != 4) return fail(EDTTS_ERR_ARG, "%s: tile=%d: expected 0 (the launcher's rule), 2 or 4", fn, s.tile);
  if (s.site < 0 || s.site >= EDTTS_HUB_COUNT)
    return fail(EDTTS_ERR_ARG, "%s: stop_site=%d: expected an EDTTS_HUB_* site in [0, %d)", fn, s.site, (int)EDTTS_HUB_COUNT);
  const char* nm = kHubSiteNames[s.site];
  if ((s.site == EDTTS_HUB_LENS || s.site == EDTTS_HUB_ZERO) && !with_lengths)
    return fail(EDTTS_ERR_ARG, "%s: site EDTTS_HUB_%s exists only with lengths", fn, nm);
  if (s.site == EDTTS_HUB_VT && !bf16) return fail(EDTTS_ERR_ARG, "%s: site EDTTS_HUB_VT exists only under EDTTS_HUBERT_BF16", fn);
  if (s.site == EDTTS_HUB_CONV) {
    if (s.index < 1 || s.index >= L.nc)
      return fail(EDTTS_ERR_ARG, "%s: site EDTTS_HUB_CONV: stop_index=%d: expected a conv layer in [1, %d)", fn, s.index, L.nc);
  } else if (s.site >= EDTTS_HUB_QKV && s.site <= EDTTS_HUB_LN2) {
    if (s.index < 0 || s.index >= L.L)
      return fail(EDTTS_ERR_ARG, "%s: site EDTTS_HUB_%s: stop_index=%d: expected an encoder layer in [0, %d)", fn, nm, s.index, L.L);
  } else if (s.index != 0) {
    return fail(EDTTS_ERR_ARG, "%s: site EDTTS_HUB_%s has no index: stop_index=%d, expected 0", fn, nm, s.index);
  }
  return EDTTS_OK;
}
#define EDTTS_HUB_STOP_AFTER(site_, index_) \
  if (stop.site == (site_) && stop.index == (index_)) return EDTTS_OK

static int hub_forward32(const HubLayout& L, const void* packed, const float* wav, int B, int T_audio, const int64_t* lengths, float* out,
                         void* workspace, hipStream_t st, const HubStop stop);

}  // namespace edtts_hub

extern "C" {

int edtts_hubert_packed_bytes(const EdttsHubertDims* dims, size_t* out_bytes) {
  edtts_hub::HubLayout L;
  TRY_G(edtts_hub::hub_layout(dims, L));
  if (!out_bytes) return fail(EDTTS_ERR_ARG, "out_bytes is NULL");
  *out_bytes = L.total * sizeof(float);
  return EDTTS_OK;
}

int edtts_hubert_frames(const EdttsHubertDims* dims, int64_t n_samples, int64_t* out_frames) {
  edtts_hub::HubLayout L;
  TRY_G(edtts_hub::hub_layout(dims, L));
  if (!out_frames) return fail(EDTTS_ERR_ARG, "out_frames is NULL");
  if (n_samples < 0 || n_samples > 0x7fffffffLL) return fail(EDTTS_ERR_ARG, "n_samples=%lld out of range", (long long)n_samples);
  *out_frames = edtts_hub::hub_frames(L, n_samples);
  return EDTTS_OK;
}

int edtts_hubert_workspace_bytes(const EdttsHubertDims* dims, int B, int T_audio, size_t* out_bytes) {
  edtts_hub::HubLayout L;
  TRY_G(edtts_hub::hub_layout(dims, L));
  if (!out_bytes) return fail(EDTTS_ERR_ARG, "out_bytes is NULL");
  if (B < 1 || T_audio < 1) return fail(EDTTS_ERR_ARG, "B=%d T_audio=%d: need >= 1", B, T_audio);
  edtts_hub::HubWs W;
  TRY_G(edtts_hub::hub_ws(L, B, T_audio, W));
  *out_bytes = W.total;
  return EDTTS_OK;
}

int edtts_hubert_pack(const EdttsHubertDims* dims, const void* const* slots, int n_slots, void* packed, void* stream) {
  using namespace edtts_hub;
  HubLayout L;
  TRY_G(hub_layout(dims, L));
  const int want = 3 + (L.nc - 1) + 8 + 16 * L.L;
  if (!slots || !packed) return fail(EDTTS_ERR_ARG, "slots/packed is NULL");
  if (n_slots != want) return fail(EDTTS_ERR_ARG, "expected %d weight slots, got %d", want, n_slots);
  for (int i = 0; i < n_slots; ++i)
    if (!slots[i]) return fail(EDTTS_ERR_ARG, "weight slot %d is NULL", i);
  hipStream_t st = (hipStream_t)stream;
  float* P = (float*)packed;
  const float* const* s = (const float* const*)slots;
  int i = 0;
  auto copy = [&](size_t off, size_t n) -> int {
    HIP_TRY(hipMemcpyAsync(P + off, s[i++], n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return EDTTS_OK;
  };
  auto conv = [&](size_t off, int co, int ci, int k) -> int {
    hipLaunchKernelGGL(k_hub_pack_conv, dim3(hub_grid((size_t)co * ci * k)), dim3(256), 0, st, s[i++], P + off, co, ci, k);
    LAUNCH_CHECK("k_hub_pack_conv");
    return EDTTS_OK;
  };
  const int H = L.H, CL = L.C[L.nc - 1];
  TRY_G(conv(L.conv0, 1, L.C[0], L.k[0]));  // [C0][1][k0] -> [k0][C0]
  TRY_G(copy(L.gn_w, L.C[0]));
  TRY_G(copy(L.gn_b, L.C[0]));
  for (int c = 1; c < L.nc; ++c) TRY_G(conv(L.conv[c], L.C[c], L.C[c - 1], L.k[c]));
  TRY_G(copy(L.fp_w, CL));
  TRY_G(copy(L.fp_b, CL));
  TRY_G(copy(L.proj_w, (size_t)H * CL));
  TRY_G(copy(L.proj_b, H));
  TRY_G(conv(L.pos_w, H, L.Cg, L.pk));
  TRY_G(copy(L.pos_b, H));
  TRY_G(copy(L.enc_w, H));
  TRY_G(copy(L.enc_b, H));
  for (int l = 0; l < L.L; ++l) {
    const size_t b0 = (size_t)l * L.layer;
    for (int p = 0; p < 3; ++p) {  // q, k, v -> one [3H][H] matrix and a [3H] bias
      TRY_G(copy(b0 + L.qkv_w + (size_t)p * H * H, (size_t)H * H));
      TRY_G(copy(b0 + L.qkv_b + (size_t)p * H, H));
    }
    TRY_G(copy(b0 + L.o_w, (size_t)H * H));
    TRY_G(copy(b0 + L.o_b, H));
    TRY_G(copy(b0 + L.ln1_w, H));
    TRY_G(copy(b0 + L.ln1_b, H));
    TRY_G(copy(b0 + L.ff1_w, (size_t)L.I * H));
    TRY_G(copy(b0 + L.ff1_b, L.I));
    TRY_G(copy(b0 + L.ff2_w, (size_t)H * L.I));
    TRY_G(copy(b0 + L.ff2_b, H));
    TRY_G(copy(b0 + L.ln2_w, H));
    TRY_G(copy(b0 + L.ln2_b, H));
  }
  return EDTTS_OK;
}

int edtts_hubert_forward(const EdttsHubertDims* dims, const void* packed, const float* wav, int B, int T_audio, const int64_t* lengths,
                         float* out, void* workspace, void* stream) {
  using namespace edtts_hub;
  HubLayout L;
  TRY_G(hub_layout(dims, L));
  if (!packed || !wav || !out || !workspace) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (B < 1 || T_audio < 1) return fail(EDTTS_ERR_ARG, "B=%d T_audio=%d: need >= 1", B, T_audio);
  if (!hub_al16(packed) || !hub_al16(out) || !hub_al16(workspace)) return fail(EDTTS_ERR_ARG, "packed, out and workspace must be 16-byte aligned");
  return hub_forward32(L, packed, wav, B, T_audio, lengths, out, workspace, (hipStream_t)stream, HubStop{});
}

}  // extern "C"

namespace edtts_hub {

// The fp32 forward's launch list.  The sites of edtts_hubert_forward_until (EDTTS_HUB_*, include/edtts.h): one line below each; `stop`
// never matches in the plain entry point (site -1), whose launch list is the whole of it.
static int hub_forward32(const HubLayout& L, const void* packed, const float* wav, int B, int T_audio, const int64_t* lengths, float* out,
                         void* workspace, hipStream_t st, const HubStop stop) {
  HubWs ws;
  TRY_G(hub_ws(L, B, T_audio, ws));
  const int tile = stop.tile;
  const float* P = (const float*)packed;
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
  float* buf[2] = {(float*)(wb + ws.buf0), (float*)(wb + ws.buf1)};
  float *h = (float*)(wb + ws.h), *att = (float*)(wb + ws.att), *big = (float*)(wb + ws.big);
  // conv0 + GroupNorm + GELU -> buf[0]
  double* part = (double*)(wb + ws.part);
  hipLaunchKernelGGL(k_hub_gn_part, dim3((L.C[0] + 63) / 64, ws.nch, B), dim3(256), 0, st, wav, T_audio, P + L.conv0, L.C[0], L.k[0],
                     L.s[0], len0, ws.T[0], part);
  LAUNCH_CHECK("k_hub_gn_part");
  hipLaunchKernelGGL(k_hub_gn_final, dim3((B * L.C[0] + 255) / 256), dim3(256), 0, st, part, ws.nch, L.C[0], len0, ws.T[0], 1e-5f,
                     P + L.gn_w, P + L.gn_b, stats, B);
  LAUNCH_CHECK("k_hub_gn_final");
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_GNSTAT, 0);
  hipLaunchKernelGGL(k_hub_conv0, dim3(hub_grid((size_t)B * ws.T[0] * L.C[0] / 4)), dim3(256), 0, st, wav, T_audio, P + L.conv0,
                     L.C[0], L.k[0], L.s[0], len0, ws.T[0], stats, buf[0], B);
  LAUNCH_CHECK("k_hub_conv0");
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_CONV0, 0);
  // conv1.. as implicit GEMMs + GELU, ping-ponging between the two buffers
  for (int c = 1; c < L.nc; ++c) {
    HGemmArgs a{};
    a.X = buf[(c - 1) & 1]; a.xbs = (long long)ws.T[c - 1] * L.C[c - 1]; a.ldrow = L.C[c - 1]; a.Cin = L.C[c - 1]; a.stride = L.s[c];
    a.Tin = ws.T[c - 1];
    a.W = P + L.conv[c]; a.K = L.k[c] * L.C[c - 1];
    a.Y = buf[c & 1]; a.ybs = (long long)ws.T[c] * L.C[c]; a.ldy = L.C[c]; a.M = ws.T[c]; a.N = L.C[c];
    TRY_G(hub_gemm<HEPI_GELU>(st, a, B, 1, tile));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_CONV, c);
  }
  // feature projection: LayerNorm -> Linear (+ bias) -> h
  const int CL = L.C[L.nc - 1];
  float* feat = buf[(L.nc - 1) & 1];
  float* fn = buf[L.nc & 1];
  TRY_G(hub_norm(st, feat, fn, M, CL, P + L.fp_w, P + L.fp_b, L.eps));
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_FPNORM, 0);
  TRY_G(hub_dense<HEPI_BIAS>(st, fn, P + L.proj_w, P + L.proj_b, h, nullptr, M, H, CL, tile));
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_FPROJ, 0);
  // att = h + GELU(pos_conv(h) + bias), one GEMM per group; zero rows outside [0, frames_b)
  {
    HGemmArgs a{};
    a.X = h; a.xbs = (long long)T * H; a.ldrow = H; a.Cin = L.Cg; a.stride = 1; a.pad = L.pk / 2; a.xg = L.Cg;
    a.nvalid = flen; a.Tin = T;
    a.W = P + L.pos_w; a.K = L.pk * L.Cg; a.bias = P + L.pos_b;
    a.Y = att; a.R = h; a.ybs = (long long)T * H; a.ldy = H; a.M = T; a.N = L.Cg;
    TRY_G(hub_gemm<HEPI_GELU_RESID>(st, a, B, L.pg, tile));
  }
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_POS, 0);
  TRY_G(hub_norm(st, att, L.L ? h : out, M, H, P + L.enc_w, P + L.enc_b, L.eps));
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_ENCNORM, 0);
  for (int l = 0; l < L.L; ++l) {
    const float* Y = P + (size_t)l * L.layer;
    TRY_G(hub_dense<HEPI_BIAS>(st, h, Y + L.qkv_w, Y + L.qkv_b, big, nullptr, M, 3 * H, H, tile));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_QKV, l);
    TRY_G(GenericLauncher::attn(st, AttnShape(H, L.heads, L.DH), B, big, 3 * H, big + H, big + 2 * H, 3 * H, att, T, T, -1, flen, flen, false,
                                false));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_ATTN, l);
    TRY_G(hub_dense<HEPI_RESID>(st, att, Y + L.o_w, Y + L.o_b, h, h, M, H, H, tile));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_OPROJ, l);
    TRY_G(hub_norm(st, h, h, M, H, Y + L.ln1_w, Y + L.ln1_b, L.eps));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_LN1, l);
    TRY_G(hub_dense<HEPI_GELU>(st, h, Y + L.ff1_w, Y + L.ff1_b, big, nullptr, M, L.I, H, tile));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_FF1, l);
    TRY_G(hub_dense<HEPI_RESID>(st, big, Y + L.ff2_w, Y + L.ff2_b, h, h, M, H, L.I, tile));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_FF2, l);
    TRY_G(hub_norm(st, h, l + 1 < L.L ? h : out, M, H, Y + L.ln2_w, Y + L.ln2_b, L.eps));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_LN2, l);
  }
  if (flen) {
    hipLaunchKernelGGL(k_hub_zero_past, dim3(hub_grid((size_t)M * H / 4)), dim3(256), 0, st, out, flen, B, T, H);
    LAUNCH_CHECK("k_hub_zero_past");
  }
  return EDTTS_OK;
}

}  // namespace edtts_hub
