// edtts_generic_bwd.h -- training on the generic fp32 decoder path: a forward that keeps a tape, and its backward (included by
// edtts_kernels.hip).
//
// The generic forward (edtts_generic.h) is a chain of plain row-major steps; this header differentiates it step by step.  Every
// contraction runs on v_mfma_f32_16x16x4_f32, every reduction has a fixed order (no float atomics): a sum over rows is cut into
// slabs whose partial results are added in slab order, and a scatter-add has one owner per destination row.
//
//   k_bwd_gemm<ACC>       C[M,N] (+)= sum_k A(m,k) B(n,k), both operands with run-time strides, through LDS tiles like k_gen_gemm:
//                         dX = dY W (A = dY, B = W read column-wise) and dW = dY^T X (A = dY^T, B = X^T; grid.z cuts the row
//                         sum into slabs of dw_slab_rows(M) rows, one partial [N][K] each)
//   k_bwd_slabsum         out[j] (+)= sum_s part[s][j], s ascending: the second half of every cut reduction
//   k_bwd_colsum          bias gradients: column sums of dY per slab of kColRows rows
//   k_bwd_norm_rows<MODE> dx of RMSNorm x gain (x AdaLN modulation) / LayerNorm, one wave per row; leaves rstd (and the mean)
//   k_bwd_norm_cols<MODE> per chunk of kNormChunk rows of one utterance: partial gain, (dscale | dshift) or LayerNorm-bias sums
//   k_bwd_swiglu          value / gate pre-activations -> their gradients, in place
//   k_bwd_attn_delta      delta = rowsum(dO o O) per (utterance, head, query)
//   k_bwd_attn_dq<DT>     owns 16 queries of one head: recomputes P from the tape's log-sum-exp, dQ = scale dS K
//   k_bwd_attn_dkv<DT>    owns 16 keys of one head: dV = P^T dO, dK = scale dS^T Q over the query tiles that meet the band
//   k_bwd_scatter_rows    embedding gradients: one block owns a table row and adds its positions in position order
//   k_bwd_time_emb, k_bwd_gelu, k_bwd_gelu_grad   the time MLP's elementwise pieces (its contractions reuse k_bwd_gemm)
// Dropout: k_gen_attn<DT, true> / k_gen_gemm<EPI, true> in the forward; k_bwd_attn_dq<DT, true> and
// k_bwd_attn_dkv<DT, true> regenerate the attention masks, k_bwd_swiglu_drop and k_bwd_drop_rows the feed-forward ones.
// k_drop_mask writes a mask out.
// Behind the kernels: the tape and scratch layouts, TrainLauncher, and the C ABI of training (edtts_train_*,
// edtts_decoder_forward_train*, edtts_decoder_backward*, edtts_dropout_mask).
namespace edtts_bwd {
using edtts_gen::wave_allsum;

constexpr int kDwSlabRows = 256;  // smallest slab of the dW row sum
constexpr int kColRows = 256;     // rows per partial of a bias gradient
constexpr int kNormChunk = 64;    // rows per partial of a norm's column sums (chunks never straddle two utterances)
// rows per dW slab: at most 32 slabs however long the batch
static int dw_slab_rows(int M) {
  const int r = ((M + 31) / 32 + 63) / 64 * 64;
  return r > kDwSlabRows ? r : kDwSlabRows;
}

// Per-utterance lengths in the backward.  Rows are laid out [utterance][rpb rows]; utterance b has
// utt_len(len, b, rpb) live rows and the rest is padding that is never loaded.
// (len is non-null in all of these; utt_len_of directly, as elsewhere: a further caller of utt_len_lane changes k_gen_embed's code)
EDTTS_DEV int row_count(const int64_t* len, int b, int rpb) { return utt_len_of(len[b], rpb, false); }
// row r is live (r below the row count)
EDTTS_DEV bool row_live(const int64_t* len, int rpb, int r) {
  const int b = r / rpb;
  return r - b * rpb < row_count(len, b, rpb);
}
// some row of [r0, r1) is live (r0 < r1 <= row count): the first utterance's live rows reach r0, or the next utterance begins
// before r1 (every utterance has a live row 0)
EDTTS_DEV bool rows_any_live(const int64_t* len, int rpb, int r0, int r1) {
  const int b = r0 / rpb;
  return r0 - b * rpb < row_count(len, b, rpb) || (b + 1) * rpb < r1;
}
// bit i: row r + i is live (rows at or past `total` are not)
EDTTS_DEV unsigned rows_live4(const int64_t* len, int rpb, int r, int total) {
  if (r >= total) return 0u;
  int b = r / rpb, pos = r - b * rpb, n = row_count(len, b, rpb);
  unsigned m = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (r + i >= total) break;
    if (pos >= rpb) {
      pos = 0;
      n = row_count(len, ++b, rpb);
    }
    if (pos < n) m |= 1u << i;
    ++pos;
  }
  return m;
}

enum { LEN_ROWS = 1, LEN_K = 2 };
struct BGemmArgs {
  const float *A, *B;
  float* C;
  int M, N, K;             // C[m][n] = sum_k A[m sam + k sak] B[n sbn + k sbk]
  long sam, sak, sbn, sbk;
  int ldc, kslab;          // block z contracts k in [z kslab, (z + 1) kslab) into C + z cslab   (kslab % 16 == 0)
  size_t cslab;
  int va, vb, vc;          // 16-byte loads along k (unit k stride, aligned rows, K % 4 == 0) / 16-byte stores
  // k_bwd_gemm<ACC, true>: per-utterance lengths of rpb rows each.  LEN_ROWS: m is the row (dX) -- dead rows of A load as 0, so
  // dead rows of C get 0 (ACC: stay as they are), and a tile of 64 dead rows contracts nothing; LEN_K: k is the row (dW) -- dead
  // k load as 0 in both operands and a k-step of 16 dead rows is skipped.  Every test that skips is the same for the whole block.
  const int64_t* len;
  int rpb, lmode;
};
template <int ACC, bool LEN = false>
__global__ __launch_bounds__(256) void k_bwd_gemm(BGemmArgs a) {
  using namespace edtts_gen;
  __shared__ float xs[kGBM][kGLd];
  __shared__ float ws[kGBN][kGLd];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fq = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * kGBM, n0 = blockIdx.y * kGBN;
  const int kbeg = blockIdx.z * a.kslab;
  int kend = kbeg + a.kslab < a.K ? kbeg + a.kslab : a.K;
  // loaders: an operand with unit k stride is read four k per thread (row = tid / 4); one with unit row stride one row per lane
  // (row = tid % 64), so that neighbouring threads read neighbouring addresses either way
  const int alr = a.sak == 1 ? tid >> 2 : tid & 63, alk = a.sak == 1 ? 4 * (tid & 3) : 4 * (tid >> 6);
  const int blr = a.sbk == 1 ? tid >> 2 : tid & 63, blk = a.sbk == 1 ? 4 * (tid & 3) : 4 * (tid >> 6);
  bool aok = m0 + alr < a.M;
  const bool bok = n0 + blr < a.N;
  if (LEN && a.lmode == LEN_ROWS) {
    if (!rows_any_live(a.len, a.rpb, m0, m0 + kGBM < a.M ? m0 + kGBM : a.M)) kend = kbeg;  // (block-uniform: no k-step, zeros stored)
    aok = aok && row_live(a.len, a.rpb, m0 + alr);
  }
  const float* ap = a.A + (size_t)(aok ? m0 + alr : 0) * a.sam;
  const float* bp = a.B + (size_t)(bok ? n0 + blr : 0) * a.sbn;
  const int wn0 = 32 * (w & 1), wn1 = wn0 + 16, wm = 32 * (w >> 1);
  f4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = splat(0.f);
  for (int k0 = kbeg; k0 < kend; k0 += kGBK) {
    f4 xv = splat(0.f), wv = splat(0.f);
    const int ka = k0 + alk, kb = k0 + blk;
    if (LEN && a.lmode == LEN_K) {  // (never with 16-byte loads along k: the rows are strided there)
      if (!rows_any_live(a.len, a.rpb, k0, k0 + kGBK < kend ? k0 + kGBK : kend)) continue;  // (block-uniform, ahead of the barriers)
      const unsigned la = rows_live4(a.len, a.rpb, ka, kend), lb = rows_live4(a.len, a.rpb, kb, kend);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        xv[r] = (aok && (la >> r & 1u)) ? ap[(size_t)(ka + r) * a.sak] : 0.f;
        wv[r] = (bok && (lb >> r & 1u)) ? bp[(size_t)(kb + r) * a.sbk] : 0.f;
      }
    } else {
      if (a.va) {
        if (aok && ka < kend) xv = ldg4(ap + ka);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) xv[r] = (aok && ka + r < kend) ? ap[(size_t)(ka + r) * a.sak] : 0.f;
      }
      if (a.vb) {
        if (bok && kb < kend) wv = ldg4(bp + kb);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) wv[r] = (bok && kb + r < kend) ? bp[(size_t)(kb + r) * a.sbk] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      xs[alr][alk + r] = xv[r];
      ws[blr][blk + r] = wv[r];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kGBK / 4; ++s) {
      const int kk = 4 * s + g;
      const float a0 = ws[wn0 + fq][kk], a1 = ws[wn1 + fq][kk];
      const float b0 = xs[wm + fq][kk], b1 = xs[wm + 16 + fq][kk];
      acc[0][0] = EDTTS_MFMA(a0, b0, acc[0][0]);
      acc[0][1] = EDTTS_MFMA(a0, b1, acc[0][1]);
      acc[1][0] = EDTTS_MFMA(a1, b0, acc[1][0]);
      acc[1][1] = EDTTS_MFMA(a1, b1, acc[1][1]);
    }
  }
  // acc[t][u] lane (g, fq) holds C[m = m0 + wm + 16u + fq][n = n0 + (wn0 | wn1) + 4g + r]
  float* cb = a.C + (size_t)blockIdx.z * a.cslab;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int n = n0 + (t ? wn1 : wn0) + 4 * g;
    if (n >= a.N) continue;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int m = m0 + wm + 16 * u + fq;
      if (m >= a.M) continue;
      float* cp = cb + (size_t)m * a.ldc + n;
      if (a.vc && n + 3 < a.N) {
        stg4(cp, ACC ? ldg4(cp) + acc[t][u] : acc[t][u]);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < a.N) cp[r] = ACC ? cp[r] + acc[t][u][r] : acc[t][u][r];
      }
    }
  }
}

// the same product with both operands rounded to bf16 on their way into LDS (edtts_generic16.h)
// (TB = __bf16: B holds bf16 elements, Layout::TAPE16 -- dW_down's X is the tape's SwiGLU output; sbn / sbk count elements)
template <int ACC, bool LEN = false, typename TB = float>
__global__ __launch_bounds__(256) void k_bwd_gemm16(BGemmArgs a);

// out[y ostride + j] (+)= sum_{s < ns} part[(y ns + s) pstride + j], s ascending
__global__ __launch_bounds__(256) void k_bwd_slabsum(const float* part, float* out, size_t n, int ns, size_t pstride, size_t ostride, int acc) {
  const int y = blockIdx.y;
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x) {
    const float* p = part + (size_t)y * ns * pstride + j;
    float s = p[0];
    for (int i = 1; i < ns; ++i) s += p[(size_t)i * pstride];
    float* o = out + (size_t)y * ostride + j;
    *o = acc ? *o + s : s;
  }
}

// part[slab][N]: column sums of rows [slab kColRows, ...) of Y[M][ld]
// (len non-null: rows past their utterance's count, rpb rows each, are not loaded)
__global__ __launch_bounds__(256) void k_bwd_colsum(const float* Y, int ld, int M, int N, float* part, const int64_t* len, int rpb) {
  __shared__ float sm[4][64];
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6, col = blockIdx.x * 64 + c;
  const int r0 = blockIdx.y * kColRows, r1 = r0 + kColRows < M ? r0 + kColRows : M;
  float s = 0.f;
  if (col < N) {
    if (len == nullptr) {
      for (int r = r0 + rg; r < r1; r += 4) s += Y[(size_t)r * ld + col];
    } else {
      for (int r = r0 + rg; r < r1; r += 4)
        if (row_live(len, rpb, r)) s += Y[(size_t)r * ld + col];
    }
  }
  sm[rg][c] = s;
  __syncthreads();
  if (rg == 0 && col < N) part[(size_t)blockIdx.y * N + col] = ((sm[0][c] + sm[1][c]) + sm[2][c]) + sm[3][c];
}

// ---- row norms ---------------------------------------------------------------------------------------------------------------
struct NormBwdArgs {
  const float *x, *dy;
  float* dx;
  const float* w;
  const float* mod;  // AdaLN rows (1 + scale | shift) per utterance, or null
  float* stat;       // [rows] rstd (RMSNorm) / [rows][2] mean, rstd (LayerNorm)
  float* part;       // k_bwd_norm_cols: [chunk][3][W]
  int rows, W, rows_per_b, mod_bstride, acc;
  float eps;
  const int64_t* len;  // per-utterance live rows of rows_per_b, or null
};
template <int MODE>
__global__ __launch_bounds__(256) void k_bwd_norm_rows(NormBwdArgs a) {
  using namespace edtts_gen;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;  // (no block-level synchronisation in this kernel: a wave may leave)
  const float* x = a.x + (size_t)row * a.W;
  const float* dy = a.dy + (size_t)row * a.W;
  float* dx = a.dx + (size_t)row * a.W;
  if (a.len != nullptr && !row_live(a.len, a.rows_per_b, row)) {  // a padding row: x, dy and stat are not touched, dx is 0
    if (!a.acc)
      for (int j = lane; j < a.W; j += 64) dx[j] = 0.f;
    return;
  }
  if (MODE == NORM_LAYER) {  // y = (x - mu) rs w + b
    float s = 0.f;
    for (int j = lane; j < a.W; j += 64) s += x[j];
    const float mu = wave_allsum(s) / (float)a.W;
    float q = 0.f;
    for (int j = lane; j < a.W; j += 64) {
      const float d = x[j] - mu;
      q += d * d;
    }
    const float rs = rsqrtf(wave_allsum(q) / (float)a.W + a.eps);
    float s1 = 0.f, s2 = 0.f;
    for (int j = lane; j < a.W; j += 64) {
      const float gx = dy[j] * a.w[j];
      s1 += gx;
      s2 += gx * ((x[j] - mu) * rs);
    }
    const float m1 = wave_allsum(s1) / (float)a.W, m2 = wave_allsum(s2) / (float)a.W;
    for (int j = lane; j < a.W; j += 64) {
      const float v = rs * (dy[j] * a.w[j] - m1 - (x[j] - mu) * rs * m2);
      dx[j] = a.acc ? dx[j] + v : v;
    }
    if (lane == 0) {
      a.stat[2 * (size_t)row] = mu;
      a.stat[2 * (size_t)row + 1] = rs;
    }
  } else {  // y = x rs w (1 + scale) + shift
    float q = 0.f;
    for (int j = lane; j < a.W; j += 64) q += x[j] * x[j];
    const float rs = rsqrtf(wave_allsum(q) / (float)a.W + a.eps);
    const float* md = a.mod ? a.mod + (size_t)(row / a.rows_per_b) * a.mod_bstride : nullptr;
    float c = 0.f;
    for (int j = lane; j < a.W; j += 64) {
      const float gn = dy[j] * a.w[j] * (md ? md[j] : 1.0f);
      c += gn * (x[j] * rs);
    }
    const float mean = wave_allsum(c) / (float)a.W;
    for (int j = lane; j < a.W; j += 64) {
      const float gn = dy[j] * a.w[j] * (md ? md[j] : 1.0f);
      const float v = rs * (gn - x[j] * rs * mean);
      dx[j] = a.acc ? dx[j] + v : v;
    }
    if (lane == 0) a.stat[row] = rs;
  }
}
// grid (ceil(W / 64), B * chunks per utterance); partial 0: gain gradient, 1: dscale (LayerNorm: bias gradient), 2: dshift
template <int MODE>
__global__ __launch_bounds__(256) void k_bwd_norm_cols(NormBwdArgs a) {
  using namespace edtts_gen;
  __shared__ float sm[3][4][64];
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6, col = blockIdx.x * 64 + c;
  const int cpb = (a.rows_per_b + kNormChunk - 1) / kNormChunk;
  const int b = blockIdx.y / cpb, ch = blockIdx.y - b * cpb;
  const int r0 = b * a.rows_per_b + ch * kNormChunk;
  const int e = b * a.rows_per_b + utt_len(a.len, b, a.rows_per_b), r1 = r0 + kNormChunk < e ? r0 + kNormChunk : e;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;  // (a chunk wholly past the utterance's count sums nothing and stores zeros)
  if (col < a.W) {
    const float wj = a.w[col];
    const float* md = a.mod ? a.mod + (size_t)b * a.mod_bstride : nullptr;
    const float sc = md ? md[col] : 1.0f;
    for (int r = r0 + rg; r < r1; r += 4) {
      const float xv = a.x[(size_t)r * a.W + col], d = a.dy[(size_t)r * a.W + col];
      if (MODE == NORM_LAYER) {
        s0 += d * ((xv - a.stat[2 * (size_t)r]) * a.stat[2 * (size_t)r + 1]);
        s1 += d;
      } else {
        const float n = xv * a.stat[r];
        s0 += d * sc * n;
        s1 += d * (n * wj);
        s2 += d;
      }
    }
  }
  sm[0][rg][c] = s0; sm[1][rg][c] = s1; sm[2][rg][c] = s2;
  __syncthreads();
  if (rg == 0 && col < a.W) {
    float* p = a.part + (size_t)blockIdx.y * 3 * a.W + col;
#pragma unroll
    for (int i = 0; i < 3; ++i) p[(size_t)i * a.W] = ((sm[i][0][c] + sm[i][1][c]) + sm[i][2][c]) + sm[i][3][c];
  }
}

// ---- SwiGLU ------------------------------------------------------------------------------------------------------------------
// u [M][2 FH] holds value | gate pre-activations and receives their gradients; da [M][FH] is the gradient of value * silu(gate)
__global__ __launch_bounds__(256) void k_bwd_swiglu(float* u, const float* da, size_t M, int FH) {
  const size_t n = M * FH;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / FH;
    const int c = (int)(i - row * FH);
    float* ur = u + row * 2 * FH;
    const float v = ur[c], gt = ur[FH + c], d = da[i];
    const float sg = 1.0f / (1.0f + expf(-gt));
    ur[c] = d * (gt * sg);
    ur[FH + c] = d * v * (sg * (1.0f + gt * (1.0f - sg)));
  }
}

// ... with dropout behind value * silu(gate): da is multiplied by that mask (site 2) first.  One thread per four columns.
__global__ __launch_bounds__(256) void k_bwd_swiglu_drop(float* u, const float* da, size_t M, int FH, DropArgs dr_in) {
  const DropArgs dr = drop_live(dr_in);
  const int ng = (FH + 3) / 4;
  const size_t n = M * ng;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / ng;
    const int c0 = 4 * (int)(i - row * ng);
    const f4 dm = drop_row4(dr, (int)row, c0);
    float* ur = u + row * 2 * FH;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + r;
      if (c >= FH) break;
      const float v = ur[c], gt = ur[FH + c], d = da[row * FH + c] * dm[r];
      const float sg = 1.0f / (1.0f + expf(-gt));
      ur[c] = d * (gt * sg);
      ur[FH + c] = d * v * (sg * (1.0f + gt * (1.0f - sg)));
    }
  }
}
// y[M][W] = x[M][W] o mask: the residual gradient entering the dropped down projection (site 3)
__global__ __launch_bounds__(256) void k_bwd_drop_rows(const float* x, float* y, size_t M, int W, DropArgs dr_in) {
  const DropArgs dr = drop_live(dr_in);
  const int ng = (W + 3) / 4;
  const size_t n = M * ng;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / ng;
    const int c0 = 4 * (int)(i - row * ng);
    const f4 dm = drop_row4(dr, (int)row, c0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (c0 + r < W) y[row * W + c0 + r] = x[row * W + c0 + r] * dm[r];
  }
}
// edtts_dropout_mask: keep bytes of one site through the functions the kernels call.  Attention sites: rows = B heads Tq rows of
// W = Tk keys (row = bh Tq + q); feed-forward sites: rows = B T rows of W columns.
__global__ __launch_bounds__(256) void k_drop_mask(uint8_t* keep, size_t rows, int W, int Tq, int attn, DropArgs dr_in) {
  const DropArgs dr = drop_live(dr_in);
  const int ng = (W + 3) / 4;
  const size_t n = rows * ng;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / ng;
    const int c0 = 4 * (int)(i - row * ng);
    const f4 dm = attn ? drop_attn_keys4(dr, (unsigned)(row / Tq), (int)(row % Tq), c0, true) : drop_row4(dr, (int)row, c0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (c0 + r < W) keep[row * W + c0 + r] = dm[r] != 0.f ? 1 : 0;
  }
}

// ---- attention ---------------------------------------------------------------------------------------------------------------
// delta[(b HEADS + hd) Tq + i] = sum_d dO[row][hd DH + d] O[row][hd DH + d]   (row = b Tq + i), d ascending
// (q_len non-null: a query past its utterance's count gets 0 without a load)
__global__ __launch_bounds__(256) void k_bwd_attn_delta(const float* o, const float* dO, float* delta, int B, int Tq, int HEADS, int DH, int ld,
                                                        const int64_t* q_len) {
  const size_t n = (size_t)B * HEADS * Tq;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t bh = i / Tq;
    const int q = (int)(i - bh * Tq), hd = (int)(bh % HEADS);
    if (q_len != nullptr && q >= row_count(q_len, (int)(bh / HEADS), Tq)) {
      delta[i] = 0.f;
      continue;
    }
    const size_t row = (bh / HEADS) * Tq + q;
    const float* op = o + row * ld + (size_t)hd * DH;
    const float* dp = dO + row * ld + (size_t)hd * DH;
    float s = 0.f;
    for (int d = 0; d < DH; ++d) s += op[d] * dp[d];
    delta[i] = s;
  }
}
struct AttnBwdArgs {
  const float *q, *k, *v, *dO;  // rows b Tq + i (q, dO) / b Tk + j (k, v), feature head * DH + d
  const float *lse, *delta;     // [(b HEADS + head) Tq + i]; lse in the exp2 domain
  float *dq, *dk, *dv;
  int ldq, ldkv, ldo, lddq, lddkv, Tq, Tk, DH, window;
  float scale, scale_nat;       // log2(e) / sqrt(head_dim) (scores as the forward forms them), 1 / sqrt(head_dim)
  DropArgs dr;                  // the <DT, true> instantiations only: the forward's mask of the probabilities
  const int64_t *q_len, *k_len; // per-utterance query / key counts [B], or null: Tq / Tk for all (as AttnArgs)
};
// One wave = 16 queries of one (utterance, head), laid out as k_gen_attn: S^T = K Q^T and dP^T = V dO^T tiles hold (key 4g + r,
// query fq) on lane (g, fq); dS^T is then the B operand of dQ^T += K^T dS^T as P^T is of O^T += V^T P^T in the forward.
// DROP: O = (P o D) V with D = keep * scale regenerated here; dS = P o (D o dP - delta) (delta = rowsum(dO o O) as without dropout).
template <int DT, bool DROP = false>
__global__ __launch_bounds__(64) void k_bwd_attn_dq(AttnBwdArgs a) {
  const int lane = threadIdx.x, fq = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, hd = blockIdx.y, b = blockIdx.z;
  const int qi = q0 + fq;
  // Per-utterance lengths: queries and keys are bounded by the utterance's counts, with the forward's lo / hi sequence; nothing past
  // them is loaded.  The dq rows of padding queries are stored as zeros (the destination is reused scratch that the next dX / dW
  // reads); a block wholly past the count does only that (one wave per block: leaving early is safe).
  const int Tqb = utt_len(a.q_len, b, a.Tq), Tkb = utt_len(a.k_len, b, a.Tk);
  if (q0 >= Tqb) {
    if (qi < a.Tq) {
      float* zrow = a.dq + ((size_t)b * a.Tq + qi) * a.lddq + hd * a.DH;
      for (int d = g; d < a.DH; d += 4) zrow[d] = 0.f;
    }
    return;
  }
  const bool qok = qi < Tqb;
  const size_t qr = (size_t)b * a.Tq + (qok ? qi : 0);
  const float* qrow = a.q + qr * a.ldq + hd * a.DH;
  const float* drow = a.dO + qr * a.ldo + hd * a.DH;
  float qv[4 * DT], dov[4 * DT];
#pragma unroll
  for (int s = 0; s < 4 * DT; ++s) {
    const int d = 4 * s + g;
    const bool ok = qok && d < a.DH;
    qv[s] = ok ? qrow[d] * a.scale : 0.f;
    dov[s] = ok ? drow[d] : 0.f;
  }
  const size_t si = ((size_t)b * gridDim.y + hd) * a.Tq + (qok ? qi : 0);
  const float ls = a.lse[si], dl = a.delta[si];
  f4 acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) acc[t] = splat(0.f);
  int lo = 0, hi = Tkb;
  if (a.window >= 0) {
    lo = q0 - a.window > 0 ? q0 - a.window : 0;
    const int e = q0 + 16 + a.window;
    hi = e < Tkb ? e : Tkb;
  }
  const float* kb = a.k + (size_t)b * a.Tk * a.ldkv + hd * a.DH;
  const float* vb = a.v + (size_t)b * a.Tk * a.ldkv + hd * a.DH;
  const DropArgs dr = DROP ? drop_live(a.dr) : DropArgs{};
  for (int j0 = lo; j0 < hi; j0 += 16) {
    const int kj = j0 + fq;
    const bool kok = kj < hi;
    const float* krow = kb + (size_t)(kok ? kj : 0) * a.ldkv;
    const float* vrow = vb + (size_t)(kok ? kj : 0) * a.ldkv;
    f4 sc = splat(0.f), dp = splat(0.f);
#pragma unroll
    for (int s = 0; s < 4 * DT; ++s) {
      const int d = 4 * s + g;
      const bool ok = kok && d < a.DH;
      sc = EDTTS_MFMA(ok ? krow[d] : 0.f, qv[s], sc);
      dp = EDTTS_MFMA(ok ? vrow[d] : 0.f, dov[s], dp);
    }
    if (DROP) {
      const f4 dm = drop_attn_keys4(dr, (unsigned)(b * gridDim.y + hd), qi, j0 + 4 * g, (lo & 3) == 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) dp[r] *= dm[r];
    }
    f4 ds;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = j0 + 4 * g + r;
      const bool ok = qok && key < hi && (a.window < 0 || (key - qi <= a.window && qi - key <= a.window));
      const float p = ok ? exp2f(sc[r] - ls) : 0.f;
      ds[r] = p * (dp[r] - dl);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int key = j0 + 4 * g + s;
      const float* kr2 = kb + (size_t)(key < hi ? key : 0) * a.ldkv;
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        const int d = 16 * t + fq;
        acc[t] = EDTTS_MFMA((key < hi && d < a.DH) ? kr2[d] : 0.f, ds[s], acc[t]);
      }
    }
  }
  if (qi >= a.Tq) return;
  float* orow = a.dq + ((size_t)b * a.Tq + qi) * a.lddq + hd * a.DH;
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int d = 16 * t + 4 * g + r;  // acc[t] lane (g, i) holds dQ^T[d][i]
      if (d < a.DH) orow[d] = qok ? acc[t][r] * a.scale_nat : 0.f;
    }
}
// One wave = 16 keys of one (utterance, head).  S = Q K^T and dP = dO V^T tiles hold (query 4g + r, key fq) on lane (g, fq): P and
// dS are the B operands of dV^T += dO^T P and dK^T += Q^T dS.  Only the query tiles that meet the band are visited.
// DROP: dV^T += dO^T (P o D), dS as in k_bwd_attn_dq.
template <int DT, bool DROP = false>
__global__ __launch_bounds__(64) void k_bwd_attn_dkv(AttnBwdArgs a) {
  const int lane = threadIdx.x, fq = lane & 15, g = lane >> 4;
  const int k0 = blockIdx.x * 16, hd = blockIdx.y, b = blockIdx.z;
  const int kj = k0 + fq;
  // Per-utterance lengths: as in k_bwd_attn_dq -- the query walk ends at the utterance's query count, the dk / dv rows of padding
  // keys are stored as zeros, and a block wholly past the key count does only that.
  const int Tqb = utt_len(a.q_len, b, a.Tq), Tkb = utt_len(a.k_len, b, a.Tk);
  if (k0 >= Tkb) {
    if (kj < a.Tk) {
      float* zk = a.dk + ((size_t)b * a.Tk + kj) * a.lddkv + hd * a.DH;
      float* zv = a.dv + ((size_t)b * a.Tk + kj) * a.lddkv + hd * a.DH;
      for (int d = g; d < a.DH; d += 4) zk[d] = zv[d] = 0.f;
    }
    return;
  }
  const bool kok = kj < Tkb;
  const size_t kr = (size_t)b * a.Tk + (kok ? kj : 0);
  const float* krow = a.k + kr * a.ldkv + hd * a.DH;
  const float* vrow = a.v + kr * a.ldkv + hd * a.DH;
  float kv[4 * DT], vv[4 * DT];
#pragma unroll
  for (int s = 0; s < 4 * DT; ++s) {
    const int d = 4 * s + g;
    const bool ok = kok && d < a.DH;
    kv[s] = ok ? krow[d] * a.scale : 0.f;
    vv[s] = ok ? vrow[d] : 0.f;
  }
  f4 ak[DT], av[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) ak[t] = av[t] = splat(0.f);
  int lo = 0, hi = Tqb;
  if (a.window >= 0) {
    lo = k0 - a.window > 0 ? k0 - a.window : 0;
    const int e = k0 + 16 + a.window;
    hi = e < Tqb ? e : Tqb;
  }
  const float* qb = a.q + (size_t)b * a.Tq * a.ldq + hd * a.DH;
  const float* db = a.dO + (size_t)b * a.Tq * a.ldo + hd * a.DH;
  const float* lb = a.lse + ((size_t)b * gridDim.y + hd) * a.Tq;
  const float* eb = a.delta + ((size_t)b * gridDim.y + hd) * a.Tq;
  const DropArgs dr = DROP ? drop_live(a.dr) : DropArgs{};
  for (int i0 = lo; i0 < hi; i0 += 16) {
    const int qi = i0 + fq;
    const bool qok = qi < hi;
    const float* qrow = qb + (size_t)(qok ? qi : 0) * a.ldq;
    const float* drow = db + (size_t)(qok ? qi : 0) * a.ldo;
    f4 sc = splat(0.f), dp = splat(0.f);
#pragma unroll
    for (int s = 0; s < 4 * DT; ++s) {
      const int d = 4 * s + g;
      const bool ok = qok && d < a.DH;
      sc = EDTTS_MFMA(ok ? qrow[d] : 0.f, kv[s], sc);
      dp = EDTTS_MFMA(ok ? drow[d] : 0.f, vv[s], dp);
    }
    f4 dm;
    if (DROP) {  // (query tiles start at lo + 16 n: odd for every tile or for none)
      dm = drop_attn_queries4(dr, (unsigned)(b * gridDim.y + hd), i0 + 4 * g, kj, (lo & 1) != 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) dp[r] *= dm[r];
    }
    f4 p, ds;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qq = i0 + 4 * g + r;
      const bool ok = kok && qq < hi && (a.window < 0 || (kj - qq <= a.window && qq - kj <= a.window));
      const int qs = qq < hi ? qq : 0;
      p[r] = ok ? exp2f(sc[r] - lb[qs]) : 0.f;
      ds[r] = p[r] * (dp[r] - eb[qs]);
    }
    if (DROP) {
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] *= dm[r];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int qq = i0 + 4 * g + s;
      const bool ok = qq < hi;
      const float* qr2 = qb + (size_t)(ok ? qq : 0) * a.ldq;
      const float* dr2 = db + (size_t)(ok ? qq : 0) * a.ldo;
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        const int d = 16 * t + fq;
        const bool okd = ok && d < a.DH;
        av[t] = EDTTS_MFMA(okd ? dr2[d] : 0.f, p[s], av[t]);
        ak[t] = EDTTS_MFMA(okd ? qr2[d] : 0.f, ds[s], ak[t]);
      }
    }
  }
  if (kj >= a.Tk) return;
  float* okp = a.dk + ((size_t)b * a.Tk + kj) * a.lddkv + hd * a.DH;
  float* ovp = a.dv + ((size_t)b * a.Tk + kj) * a.lddkv + hd * a.DH;
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int d = 16 * t + 4 * g + r;  // lane (g, j) holds dK^T[d][j], dV^T[d][j]
      if (d < a.DH) {
        okp[d] = kok ? ak[t][r] * a.scale_nat : 0.f;
        ovp[d] = kok ? av[t][r] : 0.f;
      }
    }
}
// the same two kernels with every contraction on bf16 MFMAs, four query / key tiles per block (edtts_generic_attn16.h)
// (TQ = __bf16: q, k and v hold bf16 elements, Layout::TAPE16; dO, the log-sum-exp, delta and every gradient stay fp32)
template <int DT, bool DROP = false, typename TQ = float>
__global__ __launch_bounds__(256) void k_bwd_attn_dq16(AttnBwdArgs a);
template <int DT, bool DROP = false, typename TQ = float>
__global__ __launch_bounds__(256) void k_bwd_attn_dkv16(AttnBwdArgs a);

// ---- embeddings ----------------------------------------------------------------------------------------------------------------
// out[row][c] = sum over positions p (ascending) whose index, clamped as the forward clamps it, is row, of src[p][c]: block = row.
// The block walks the positions 256 at a time; the ones that hit its row are compacted IN POSITION ORDER into LDS (ballot + prefix
// count) and every column thread adds them in that order, so a chunk without a hit costs one index load per thread.
// len non-null: positions come rpb per utterance and the ones at or past the utterance's count are not scanned (the forward gave them
// id 0 without reading idx, and their src rows are zero).
__global__ __launch_bounds__(256) void k_bwd_scatter_rows(const int64_t* idx, int n_pos, int n_rows, const float* src, int H, float* out,
                                                          const int64_t* len, int rpb) {
  __shared__ int list[256];
  __shared__ int wcnt[4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int cg = 0; cg < H; cg += 1024) {  // four columns per thread and pass (one pass up to hidden 1024)
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < n_pos; c0 += 256) {
      const int p = c0 + tid;
      bool hit = false;
      if (p < n_pos && (len == nullptr || row_live(len, rpb, p))) {
        long tk = (long)idx[p];
        tk = tk < 0 ? 0 : (tk >= n_rows ? n_rows - 1 : tk);
        hit = tk == row;
      }
      const unsigned long long bal = __ballot(hit);
      if (lane == 0) wcnt[w] = __popcll(bal);
      __syncthreads();
      const int n0 = wcnt[0], n1 = wcnt[1], n2 = wcnt[2], total = n0 + n1 + n2 + wcnt[3];
      if (total) {  // (the same for every thread of the block)
        if (hit) list[(w > 0 ? n0 : 0) + (w > 1 ? n1 : 0) + (w > 2 ? n2 : 0) + __popcll(bal & ((1ull << lane) - 1ull))] = p;
        __syncthreads();
        for (int i = 0; i < total; ++i) {
          const float* sp = src + (size_t)list[i] * H;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = cg + tid + 256 * j;
            if (c < H) acc[j] += sp[c];
          }
        }
      }
      __syncthreads();  // list and wcnt are rewritten by the next chunk
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cg + tid + 256 * j;
      if (c < H) out[(size_t)row * H + c] = acc[j];
    }
  }
}

// ---- time MLP ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bwd_time_emb(const int64_t* t, const float* freqs, int rows, int H, float* e) {
  const int half = H / 2;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows * H; i += gridDim.x * blockDim.x) {
    const int row = i / H, j = i - row * H;
    const float arg = (float)t[row] * freqs[j < half ? j : j - half];  // as k_cond_mlp
    e[i] = j < half ? sinf(arg) : cosf(arg);
  }
}
// a1 [rows][H] += bias (the pre-activation, kept); u = GELU(a1)
__global__ __launch_bounds__(256) void k_bwd_gelu(float* a1, const float* bias, int rows, int H, float* u) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows * H; i += gridDim.x * blockDim.x) {
    const float x = a1[i] + bias[i % H];
    a1[i] = x;
    u[i] = 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
  }
}
// du <- du * GELU'(a1)
__global__ __launch_bounds__(256) void k_bwd_gelu_grad(float* du, const float* a1, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float x = a1[i];
    du[i] *= 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * 0.3989422804014327f * expf(-0.5f * x * x);
  }
}

}  // namespace edtts_bwd

// =========================================================================================================
// the tape and the backward's scratch (offsets in floats)
// =========================================================================================================
// Layout::TAPE16 (EDTTS_TAPE_BF16): the Narrowed members hold __bf16 -- n elements take (n + 1) / 2 floats of the
// tape; their offsets still count floats (every region starts on a multiple of 64 floats = 256 bytes), their pitches elements.
struct Narrowed {
  size_t off;
  bool h;  // this tape's elements are bf16
};
static Act operator+(const float* tp, const Narrowed& r) { return Act(tp + r.off, r.h); }
struct TapeLayer {
  size_t crp;                 // kv_down rows before kv_norm [B S][R]
  Narrowed kv;                // K|V rows [B S][2H]
  size_t h0, h1, h2;          // the residual stream entering norm1 / norm2 / norm3
  Narrowed qkv;               // self-attention: q|k|v rows ...
  size_t att1, lse1;          // ... attention output, log-sum-exp [B][HEADS][T]
  Narrowed qc;                // cross-attention: query rows ...
  size_t att2, lse2;          // ... attention output, log-sum-exp
  Narrowed act;               // value * silu(gate) [B T][FM H]
};
struct TrainTape {
  size_t cond, tcond;  // AdaLN rows [B][L][2][2H] and, right behind them, t_cond [B][H]
  size_t ctx;          // context rows [B S][H]
  TapeLayer layer[kMaxLayers];
  size_t hL;           // the residual stream entering final_norm
  size_t total;
};
// The tape's regions, stated once: f(which, layer, member, n) for each of them in tape order -- `which` its EDTTS_TAPE_* name, `layer`
// its layer (-1: a whole-model member), `member` its place in *t, n its element count.  make_tape lays the tape out from it,
// edtts_train_tape_region answers from it; the forward and the backward reach the regions through the members it filled.
template <class Tape, class F>
static void tape_regions(const Layout& lo, int B, int T, int S, Tape& t, F&& f) {
  const size_t H = lo.H, M = (size_t)B * T, CS = (size_t)B * S;
  f(EDTTS_TAPE_COND, -1, t.cond, (size_t)B * lo.L * 4 * H);
  f(EDTTS_TAPE_TCOND, -1, t.tcond, (size_t)B * H);
  f(EDTTS_TAPE_CTX, -1, t.ctx, CS * H);
  for (int l = 0; l < lo.L; ++l) {
    auto& y = t.layer[l];
    f(EDTTS_TAPE_CRP, l, y.crp, CS * lo.R);
    f(EDTTS_TAPE_KV, l, y.kv, CS * 2 * H);
    f(EDTTS_TAPE_H0, l, y.h0, M * H);
    f(EDTTS_TAPE_H1, l, y.h1, M * H);
    f(EDTTS_TAPE_H2, l, y.h2, M * H);
    f(EDTTS_TAPE_QKV, l, y.qkv, M * 3 * H);
    f(EDTTS_TAPE_ATT1, l, y.att1, M * H);
    f(EDTTS_TAPE_LSE1, l, y.lse1, M * lo.HEADS);
    f(EDTTS_TAPE_QC, l, y.qc, M * H);
    f(EDTTS_TAPE_ATT2, l, y.att2, M * H);
    f(EDTTS_TAPE_LSE2, l, y.lse2, M * lo.HEADS);
    f(EDTTS_TAPE_ACT, l, y.act, M * lo.FM * H);
  }
  f(EDTTS_TAPE_HL, -1, t.hL, M * H);
}
// a member at float offset o: the floats its n elements take
static size_t tape_place(size_t& m, size_t o, size_t n, bool) { m = o; return n; }
static size_t tape_place(Narrowed& m, size_t o, size_t n, bool t16) { m = Narrowed{o, t16}; return t16 ? (n + 1) / 2 : n; }
// ... and back: its offset and the bytes of one element
struct TapePlace {
  size_t off;
  int elem_bytes;
};
static TapePlace tape_place_of(size_t m) { return TapePlace{m, 4}; }
static TapePlace tape_place_of(const Narrowed& m) { return TapePlace{m.off, m.h ? 2 : 4}; }
static void make_tape(const Layout& lo, int B, int T, int S, TrainTape* t) {
  size_t o = 0;
  tape_regions(lo, B, T, S, *t, [&](int which, int, auto& m, size_t n) {
    if (which != EDTTS_TAPE_TCOND) o = align64(o);  // (t_cond lies right behind the AdaLN rows)
    o += tape_place(m, o, n, lo.TAPE16 != 0);
  });
  t->total = align64(o);
}
struct TrainScratch {
  size_t dh, xn, ga, gq, big, da, stat, delta, dkv, crn, dcr, dcp, dctx;
  size_t dmod, dtc, e, a1, u1, du1;  // conditioning path, [B] rows
  size_t part;
  size_t total;
};
// The scratch's members, stated once: f(which, member, n) for each of them in scratch order -- `which` its EDTTS_SCRATCH_* name,
// `member` its place in *s, n its float count.  make_train_scratch lays the scratch out from it, edtts_train_scratch_region answers
// from it; the backward reaches the members through the offsets it filled.
template <class Scratch, class F>
static void scratch_regions(const Layout& lo, int B, int T, int S, Scratch& s, F&& f) {
  const size_t H = lo.H, M = (size_t)B * T, CS = (size_t)B * S, FH = (size_t)lo.FM * H, R = lo.R;
  auto mx = [](size_t a, size_t b) { return a > b ? a : b; };
  f(EDTTS_SCRATCH_DH, s.dh, M * H); f(EDTTS_SCRATCH_XN, s.xn, M * H); f(EDTTS_SCRATCH_GA, s.ga, M * H); f(EDTTS_SCRATCH_GQ, s.gq, M * H);
  f(EDTTS_SCRATCH_BIG, s.big, M * mx(2 * FH, 3 * H)); f(EDTTS_SCRATCH_DA, s.da, M * FH);
  f(EDTTS_SCRATCH_STAT, s.stat, 2 * mx(M, CS)); f(EDTTS_SCRATCH_DELTA, s.delta, M * lo.HEADS);
  f(EDTTS_SCRATCH_DKV, s.dkv, CS * 2 * H); f(EDTTS_SCRATCH_CRN, s.crn, CS * R); f(EDTTS_SCRATCH_DCR, s.dcr, CS * R);
  f(EDTTS_SCRATCH_DCP, s.dcp, CS * R); f(EDTTS_SCRATCH_DCTX, s.dctx, CS * H);
  f(EDTTS_SCRATCH_DMOD, s.dmod, (size_t)B * lo.L * 4 * H); f(EDTTS_SCRATCH_DTC, s.dtc, (size_t)B * H); f(EDTTS_SCRATCH_E, s.e, (size_t)B * H);
  f(EDTTS_SCRATCH_A1, s.a1, (size_t)B * H); f(EDTTS_SCRATCH_U1, s.u1, (size_t)B * H); f(EDTTS_SCRATCH_DU1, s.du1, (size_t)B * H);
  // partial slabs: the largest of the dW partials (slab count of its row sum x [N][K]), the bias partials and the norm partials
  size_t part = 0;
  auto dwp = [&](size_t rows, size_t n, size_t k) {
    const size_t r = edtts_bwd::dw_slab_rows((int)rows), ns = (rows + r - 1) / r;
    if (ns > 1) part = mx(part, ns * n * k);
  };
  dwp(M, lo.MEL, H); dwp(M, H, FH); dwp(M, 2 * FH, H); dwp(M, H, H); dwp(M, 3 * H, H); dwp(M, H, lo.MEL);   // decoder rows
  dwp(CS, 2 * H, R); dwp(CS, R, H); dwp(CS, H, lo.SD);                                                     // context rows
  dwp(B, 2 * H, H); dwp(B, H, H);                                                                          // conditioning rows
  const size_t cr = edtts_bwd::kColRows;
  part = mx(part, (M + cr - 1) / cr * mx(2 * FH, (size_t)lo.MEL));  // bias partials: [slabs][N], N <= 2 FH (or n_mels)
  part = mx(part, (CS + cr - 1) / cr * H);
  const size_t cpb = ((size_t)mx(T, S) + edtts_bwd::kNormChunk - 1) / edtts_bwd::kNormChunk;
  part = mx(part, (size_t)B * cpb * 3 * H);                        // norm partials: [chunk][3][W]
  f(EDTTS_SCRATCH_PART, s.part, part);
}
static void make_train_scratch(const Layout& lo, int B, int T, int S, TrainScratch* s) {
  size_t o = 0;
  scratch_regions(lo, B, T, S, *s, [&](int, size_t& m, size_t n) { m = o; o = align64(o + n); });
  s->total = o;
}

// Where the backward stops (edtts_decoder_backward_until): after the last launch of site `site` of layer `layer`.  site < 0: never.
struct BwdStop {
  int layer = -1, site = -1;
};

// =========================================================================================================
// TrainLauncher: forward with a tape, backward from it
// =========================================================================================================
// A row set with per-utterance lengths: rpb rows per utterance of which len[b] are live (len null: all of them)
struct RowLens {
  const int64_t* len = nullptr;
  int rpb = 0;
};
struct TrainLauncher {
  using G = GenericLauncher;
  // The generic forward with its intermediates in the tape: what the backward needs is written there directly, or copied there
  // (the residual stream); kv_norm's output stays in the workspace.  The AdaLN rows are already in the tape (launch_cond).
  // Per-utterance lengths (c.ln) enter where they enter there: the embedding's padding ids, both attentions' key counts and query
  // skip, and eps zeroed past T_b -- so eps is bitwise edtts_decoder_forward_len's.  Tape rows past the lengths hold whatever the
  // row-local steps made of the padding (or nothing at all: skipped query blocks); the backward never loads them.
  // drop non-null: the tape's attention outputs and SwiGLU output are the dropped ones.
  static int forward(const CallCtx& c, float* tp, const TrainTape& tt, const float* x, const int64_t* sem_idx, const float* sem_feat, float* eps,
                     const DropState* drop = nullptr) {
    FwdBufs fb;
    fb.ctx = tp + tt.ctx;
    fb.hL = tp + tt.hL;
    for (int l = 0; l < c.lo.L; ++l) {
      const TapeLayer& z = tt.layer[l];
      FwdLayerBufs& f = fb.layer[l];
      f.crp = tp + z.crp; f.crn = c.wsb + c.ws.g_cr; f.kv = tp + z.kv;
      f.qkv = tp + z.qkv; f.att1 = tp + z.att1; f.lse1 = tp + z.lse1;
      f.qc = tp + z.qc; f.att2 = tp + z.att2; f.lse2 = tp + z.lse2;
      f.act = tp + z.act;
      f.h0 = tp + z.h0; f.h1 = tp + z.h1; f.h2 = tp + z.h2;
    }
    StepTail tail;
    tail.eps = eps;
    TRY_G(G::ctx(c, fb, sem_idx, sem_feat));
    return G::forward(c, fb, x, tp + tt.cond, c.lo.L * 4 * c.lo.H, tail, drop);
  }

  // ---- backward helpers ----
  static bool al16(const void* p) { return G::al16(p); }
  // The instances of the backward's product that exist, over (bf16 products, accumulating, row lengths, bf16 operand B): B holds bf16
  // elements in one call only -- dW_down's X with Layout::TAPE16 -- which k_bwd_gemm16 serves, not accumulating
  template <bool MM16, int ACC, class TB>
  static constexpr bool bgemm_instance() { return std::is_same<TB, float>::value || (MM16 && !ACC); }
  template <bool MM16, int ACC, bool LEN, class TB>
  static constexpr auto bgemm_kernel() {
    if constexpr (MM16) return &edtts_bwd::k_bwd_gemm16<ACC, LEN, TB>;
    else return &edtts_bwd::k_bwd_gemm<ACC, LEN>;
  }
  static int bgemm(MmStream st, edtts_bwd::BGemmArgs a, int slabs, bool acc, bool b16 = false) {
    const dim3 grid((a.M + 63) / 64, (a.N + 63) / 64, slabs);
    return with_flag(st.bf16, [&](auto mm) { return with_flag(acc, [&](auto accum) {
      return with_flag(a.len != nullptr, [&](auto lens) { return with_elem(b16, [&](auto eb) -> int {
        using TB = typename decltype(eb)::type;
        constexpr bool MM16 = decltype(mm)::value;
        constexpr int ACC = decltype(accum)::value;
        if constexpr (bgemm_instance<MM16, ACC, TB>()) {
          hipLaunchKernelGGL((bgemm_kernel<MM16, ACC, decltype(lens)::value, TB>()), grid, dim3(256), 0, st.st, a);
          LAUNCH_CHECK("k_bwd_gemm");
          return EDTTS_OK;
        } else {
          return fail(EDTTS_ERR_UNSUPPORTED, "generic kernels: a bf16 operand needs the bf16 products, not accumulating");
        }
      }); });
    }); });
  }
  static int slabsum(hipStream_t st, const float* part, float* out, size_t n, int ns, size_t pstride, int ny = 1, size_t ostride = 0, bool acc = false) {
    hipLaunchKernelGGL(edtts_bwd::k_bwd_slabsum, dim3(G::grid_1d(n), ny), dim3(256), 0, st, part, out, n, ns, pstride, ostride, (int)acc);
    LAUNCH_CHECK("k_bwd_slabsum");
    return EDTTS_OK;
  }
  // dX[M][K] (+)= dY[M][N] W[N][K]   (wT: the blob keeps W transposed, [K][N])
  // (rl: the M rows' lengths -- dead rows of dY are not loaded, dead rows of dX are 0)
  static int dx(MmStream st, const float* dY, long ldy, const float* W, int M, int N, int K, float* dX, int ldx, bool acc, bool wT = false,
                RowLens rl = RowLens{}) {
    edtts_bwd::BGemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = dY; a.B = W; a.C = dX; a.M = M; a.N = K; a.K = N;
    a.sam = ldy; a.sak = 1; a.sbn = wT ? N : 1; a.sbk = wT ? 1 : K;
    a.ldc = ldx; a.kslab = (N + 15) / 16 * 16; a.cslab = 0;
    a.va = (N % 4 == 0) && (ldy % 4 == 0) && al16(dY);
    a.vb = wT && (N % 4 == 0) && al16(W);
    a.vc = (ldx % 4 == 0) && al16(dX);
    a.len = rl.len; a.rpb = rl.rpb; a.lmode = edtts_bwd::LEN_ROWS;
    return bgemm(st, a, 1, acc);
  }
  // dW[N][K] = dY[M][N]^T X[M][K]: slabs of dw_slab_rows(M) rows, summed in slab order
  // (rl: the M rows' lengths -- dead rows of dY and X are not loaded)
  // (X: fp32 rows, or the tape's bf16 SwiGLU output)
  static int dw(MmStream st, const float* dY, long ldy, Act X, long ldx, int M, int N, int K, float* dW, float* part,
                RowLens rl = RowLens{}) {
    if (!dW) return EDTTS_OK;
    const int rows = edtts_bwd::dw_slab_rows(M), ns = (M + rows - 1) / rows;
    edtts_bwd::BGemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = dY; a.B = X.p; a.C = ns == 1 ? dW : part; a.M = N; a.N = K; a.K = M;
    a.sam = 1; a.sak = ldy; a.sbn = 1; a.sbk = ldx;
    a.ldc = K; a.kslab = rows; a.cslab = (size_t)N * K;
    a.vc = (K % 4 == 0) && al16(a.C);
    a.len = rl.len; a.rpb = rl.rpb; a.lmode = edtts_bwd::LEN_K;
    TRY_G(bgemm(st, a, ns, false, X.h));
    if (ns > 1) TRY_G(slabsum(st, part, dW, (size_t)N * K, ns, (size_t)N * K));
    return EDTTS_OK;
  }
  static int colsum(hipStream_t st, const float* Y, int ld, int M, int N, float* out, float* part, RowLens rl = RowLens{}) {
    if (!out) return EDTTS_OK;
    const int ns = (M + edtts_bwd::kColRows - 1) / edtts_bwd::kColRows;
    hipLaunchKernelGGL(edtts_bwd::k_bwd_colsum, dim3((N + 63) / 64, ns), dim3(256), 0, st, Y, ld, M, N, part, rl.len, rl.rpb);
    LAUNCH_CHECK("k_bwd_colsum");
    return slabsum(st, part, out, (size_t)N, ns, (size_t)N);
  }
  // The gradients of one `linear` site Y[M][N] = X[M][K] W[N][K]^T + b from dY (pitch ldy; X, dW and dX are dense): the bias column
  // sum -> db, dW = dY^T X and dX (+)= dY W, launched in that order; a null destination skips its launch.
  static int linear_bwd(MmStream st, const float* dY, int ldy, Act X, const float* W, int M, int N, int K, float* db, float* dW, float* dX,
                        float* part, RowLens rl = RowLens{}, bool acc = false, bool wT = false) {
    TRY_G(colsum(st, dY, ldy, M, N, db, part, rl));
    TRY_G(dw(st, dY, ldy, X, K, M, N, K, dW, part, rl));
    return dX ? dx(st, dY, ldy, W, M, N, K, dX, K, acc, wT, rl) : EDTTS_OK;
  }
  // RMSNorm / LayerNorm backward: dx (+)= ..., gain gradient -> dgain (null: skipped), LayerNorm bias gradient -> dbias,
  // AdaLN (dscale | dshift) -> dmod[b dmod_bstride ...] (null: skipped)
  template <int MODE>
  static int norm_bwd(hipStream_t st, const float* x, const float* dy, float* dxp, bool acc, int rows, int W, int rows_per_b, const float* w,
                      float eps, const float* mod, int mod_bstride, float* stat, float* part, float* dgain, float* dbias, float* dmod,
                      int dmod_bstride, const int64_t* len = nullptr) {
    edtts_bwd::NormBwdArgs a{x, dy, dxp, w, mod, stat, part, rows, W, rows_per_b, mod_bstride, (int)acc, eps, len};
    hipLaunchKernelGGL(edtts_bwd::k_bwd_norm_rows<MODE>, dim3((rows + 3) / 4), dim3(256), 0, st, a);
    LAUNCH_CHECK("k_bwd_norm_rows");
    if (!dgain && !dbias && !dmod) return EDTTS_OK;
    const int cpb = (rows_per_b + edtts_bwd::kNormChunk - 1) / edtts_bwd::kNormChunk, nb = rows / rows_per_b;
    hipLaunchKernelGGL(edtts_bwd::k_bwd_norm_cols<MODE>, dim3((W + 63) / 64, nb * cpb), dim3(256), 0, st, a);
    LAUNCH_CHECK("k_bwd_norm_cols");
    if (dgain) TRY_G(slabsum(st, part, dgain, (size_t)W, nb * cpb, (size_t)3 * W));
    if (dbias) TRY_G(slabsum(st, part + W, dbias, (size_t)W, nb * cpb, (size_t)3 * W));
    if (dmod) TRY_G(slabsum(st, part + W, dmod, (size_t)2 * W, cpb, (size_t)3 * W, nb, (size_t)dmod_bstride));
    return EDTTS_OK;
  }
  // k_bwd_attn_dq / _dkv (a wave = 16 queries / keys) or, for the bf16 attention, their 64-row twins, which alone read bf16 rows
  template <int DT, bool ATT16, bool DROP, class TQ>
  static constexpr auto attn_dq_kernel() {
    if constexpr (ATT16) return &edtts_bwd::k_bwd_attn_dq16<DT, DROP, TQ>;
    else return &edtts_bwd::k_bwd_attn_dq<DT, DROP>;
  }
  template <int DT, bool ATT16, bool DROP, class TQ>
  static constexpr auto attn_dkv_kernel() {
    if constexpr (ATT16) return &edtts_bwd::k_bwd_attn_dkv16<DT, DROP, TQ>;
    else return &edtts_bwd::k_bwd_attn_dkv<DT, DROP>;
  }
  // gradients of one attention call: dq, dk, dv from q, k, v, the output o, its gradient dO and the tape's log-sum-exp
  // (q, k, v of one element type, as GenericLauncher::attn)
  static int attn_bwd(hipStream_t st, const AttnShape& as, int B, Act q, int ldq, Act k, Act v, int ldkv, const float* o,
                      const float* dO, const float* lse, float* delta, float* dq, int lddq, float* dk, float* dv, int lddkv, int Tq, int Tk,
                      int window, const DropArgs* dr = nullptr, const int64_t* q_len = nullptr, const int64_t* k_len = nullptr) {
    if (q.h != k.h || q.h != v.h || (q.h && !as.att16))
      return fail(EDTTS_ERR_UNSUPPORTED, "generic kernels: bf16 q, k, v rows need the bf16 attention (EDTTS_ATTN_BF16), all three of them");
    const size_t n = (size_t)B * as.HEADS * Tq;
    hipLaunchKernelGGL(edtts_bwd::k_bwd_attn_delta, dim3(G::grid_1d(n)), dim3(256), 0, st, o, dO, delta, B, Tq, as.HEADS, as.DH, as.H, q_len);
    LAUNCH_CHECK("k_bwd_attn_delta");
    const float sn = 1.0f / sqrtf((float)as.DH);
    edtts_bwd::AttnBwdArgs a{q.p, k.p, v.p, dO, lse, delta, dq, dk, dv, ldq, ldkv, as.H, lddq, lddkv, Tq, Tk, as.DH, window,
                             1.4426950408889634f / sqrtf((float)as.DH), sn, dr ? *dr : DropArgs{}, q_len, k_len};
    const int rpb = as.att16 ? 64 : 16;  // queries / keys per block: one wave each 16 of them
    const dim3 gq((Tq + rpb - 1) / rpb, as.HEADS, B), gk((Tk + rpb - 1) / rpb, as.HEADS, B), block(4 * rpb);
    return with_head_tiles<8>(as.DH, [&](auto dt) { return with_flag(as.att16, [&](auto a16) {
      return with_flag(dr != nullptr, [&](auto dropping) { return with_elem(q.h, [&](auto eq) -> int {
        using TQ = typename decltype(eq)::type;
        constexpr int DT = decltype(dt)::value;
        constexpr bool ATT16 = decltype(a16)::value, DROP = decltype(dropping)::value;
        if constexpr (ATT16 || std::is_same<TQ, float>::value) {  // (bf16 rows without the bf16 attention: refused above)
          hipLaunchKernelGGL((attn_dq_kernel<DT, ATT16, DROP, TQ>()), gq, block, 0, st, a);
          hipLaunchKernelGGL((attn_dkv_kernel<DT, ATT16, DROP, TQ>()), gk, block, 0, st, a);
          LAUNCH_CHECK("k_bwd_attn");
        }
        return EDTTS_OK;
      }); });
    }); });
  }

  // The backward.  Reads the tape, the blob and its arguments; every buffer it writes is in `sc` (its own scratch) or a gradient.
  // gs: gradient destinations in edtts_pack_weights slot order (null: not wanted).
  static int backward(const Layout& lo, const float* blob, const float* tp, const TrainTape& tt, float* sc, const TrainScratch& ss, int B, int T,
                      int S, int window, const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx, const float* sem_feat,
                      const float* d_eps, float* const* gs, float* d_x, float* d_sem, hipStream_t stream, const DropState* drop = nullptr,
                      const Lens& ln = Lens{}, const BwdStop stop = BwdStop{}) {
    using namespace edtts_gen;
    // The sites of edtts_decoder_backward_until (EDTTS_BWD_*, include/edtts.h): one line of the launch list below each.  The head's and
    // the tail's sites carry layer 0; `stop` never matches in the plain entry points (site -1), whose launch list is the whole of it.
#define EDTTS_STOP_AFTER(layer_, site_) \
  if (stop.site == (site_) && stop.layer == (layer_)) return EDTTS_OK
    const MmStream st{stream, lo.MM16 != 0};  // every dx / dw / recomputation below follows the layout's matmul_dtype
    // Per-utterance lengths: tr / sr mask every contraction over decoder / context rows and zero the dead
    // rows of every dX; the elementwise steps in between run on all rows (what they make of a dead row is never loaded again).
    const RowLens tr{ln.t, T}, sr{ln.s, S};
    const int M = B * T, CS = B * S, H = lo.H, R = lo.R, FH = lo.FM * lo.H, MEL = lo.MEL, L = lo.L;
    float *dh = sc + ss.dh, *xn = sc + ss.xn, *ga = sc + ss.ga, *gq = sc + ss.gq, *big = sc + ss.big, *da = sc + ss.da;
    float *stat = sc + ss.stat, *delta = sc + ss.delta, *dkv = sc + ss.dkv, *crn = sc + ss.crn, *dcr = sc + ss.dcr, *dcp = sc + ss.dcp;
    float *dctx = sc + ss.dctx, *dmod = sc + ss.dmod, *part = sc + ss.part;
    const float* cond_row = tp + tt.cond;
    const int cb = L * 4 * H;
    const size_t row = (size_t)4 * H;
    auto GG = [&](int i) { return gs[i]; };
    HIP_TRY(hipMemsetAsync(dctx, 0, (size_t)CS * H * sizeof(float), st));
    // out_proj and final_norm
    TRY_G(colsum(st, d_eps, MEL, M, MEL, GG(G_OUT_B), part, tr));
    TRY_G(G::norm<NORM_LAYER>(st, tp + tt.hL, xn, M, H, blob + lo.fnw, blob + lo.fnb, 1e-5f));
    TRY_G(linear_bwd(st, d_eps, MEL, xn, blob + lo.s_outp, M, MEL, H, nullptr, GG(G_OUT_W), ga, part, tr));  // (its bias: summed above)
    EDTTS_STOP_AFTER(0, EDTTS_BWD_OUT);
    TRY_G(norm_bwd<NORM_LAYER>(st, tp + tt.hL, ga, dh, false, M, H, T, blob + lo.fnw, 1e-5f, nullptr, 0, stat, part, GG(G_FN_W), GG(G_FN_B),
                               nullptr, 0, ln.t));
    EDTTS_STOP_AFTER(0, EDTTS_BWD_FNORM);
    for (int l = L - 1; l >= 0; --l) {
      const LayerLayout& y = lo.layer[l];
      const TapeLayer& z = tt.layer[l];
      auto W = [&](int i) { return gs[G_COUNT + l * L_COUNT + i]; };
      DropArgs dra[4];
      for (int i = 0; i < 4; ++i) dra[i] = drop ? drop->site(l, i) : DropArgs{};
      auto D = [&](int i) -> const DropArgs* { return drop ? &dra[i] : nullptr; };
      // feed-forward branch: h3 = h2 + down(value * silu(gate)) + b
      // (dropout: h3 = h2 + mask3 o (down(act) + b) with act = mask2 o (value * silu(gate)) on the tape: the residual gradient is
      // masked once into gq, free until the cross-attention branch, and that copy feeds the bias sum, dW_down and dX)
      const float* dd = dh;
      if (drop) {
        hipLaunchKernelGGL(edtts_bwd::k_bwd_drop_rows, dim3(G::grid_1d(((size_t)M * H + 3) / 4)), dim3(256), 0, st, dh, gq, (size_t)M, H, dra[DROP_DOWN]);
        LAUNCH_CHECK("k_bwd_drop_rows");
        dd = gq;
      }
      EDTTS_STOP_AFTER(l, EDTTS_BWD_DROPDOWN);
      TRY_G(linear_bwd(st, dd, H, tp + z.act, blob + y.g_down, M, H, FH, W(L_DOWN_B), W(L_DOWN_W), da, part, tr));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_DOWN);
      TRY_G(G::norm<NORM_RMS>(st, tp + z.h2, xn, M, H, blob + y.n3w, nullptr, 1e-6f, cond_row + l * row + 2 * H, T, cb));
      TRY_G(G::gemm<EPI_BIAS>(st, xn, H, blob + y.g_up, blob + y.up_b, big, 2 * FH, M, 2 * FH, H));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_UPRE);
      if (drop)
        hipLaunchKernelGGL(edtts_bwd::k_bwd_swiglu_drop, dim3(G::grid_1d(((size_t)M * FH + 3) / 4)), dim3(256), 0, st, big, da, (size_t)M, FH,
                           dra[DROP_ACT]);
      else
        hipLaunchKernelGGL(edtts_bwd::k_bwd_swiglu, dim3(G::grid_1d((size_t)M * FH)), dim3(256), 0, st, big, da, (size_t)M, FH);
      LAUNCH_CHECK("k_bwd_swiglu");
      EDTTS_STOP_AFTER(l, EDTTS_BWD_SWIGLU);
      TRY_G(linear_bwd(st, big, 2 * FH, xn, blob + y.g_up, M, 2 * FH, H, W(L_UP_B), W(L_UP_W), ga, part, tr));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_UP);
      TRY_G(norm_bwd<NORM_RMS>(st, tp + z.h2, ga, dh, true, M, H, T, blob + y.n3w, 1e-6f, cond_row + l * row + 2 * H, cb, stat, part, W(L_N3_W),
                               nullptr, dmod + l * row + 2 * H, cb, ln.t));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_N3);
      // cross-attention branch: h2 = h1 + att2 Wop^T
      TRY_G(linear_bwd(st, dh, H, tp + z.att2, blob + y.g_op, M, H, H, nullptr, W(L_OP_W), ga, part, tr));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_OP);
      TRY_G(attn_bwd(st, lo, B, tp + z.qc, H, tp + z.kv, (tp + z.kv) + H, 2 * H, tp + z.att2, ga, tp + z.lse2, delta, gq, H, dkv, dkv + H, 2 * H, T,
                     S, -1, D(DROP_CROSS), ln.t, ln.s));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_CROSS);
      TRY_G(G::norm<NORM_RMS>(st, tp + z.h1, xn, M, H, blob + y.n2w, nullptr, 1e-6f));
      TRY_G(linear_bwd(st, gq, H, xn, blob + y.g_qp, M, H, H, nullptr, W(L_QP_W), ga, part, tr));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_QP);
      TRY_G(norm_bwd<NORM_RMS>(st, tp + z.h1, ga, dh, true, M, H, T, blob + y.n2w, 1e-6f, nullptr, 0, stat, part, W(L_N2_W), nullptr, nullptr, 0, ln.t));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_N2);
      // ... and its context chain: context -> kv_down -> kv_norm -> kv_up -> K|V
      TRY_G(G::norm<NORM_RMS>(st, tp + z.crp, crn, CS, R, blob + y.kvn, nullptr, 1e-6f));
      TRY_G(linear_bwd(st, dkv, 2 * H, crn, blob + y.kvu, CS, 2 * H, R, nullptr, W(L_KVU_W), dcr, part, sr));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_KVU);
      TRY_G(norm_bwd<NORM_RMS>(st, tp + z.crp, dcr, dcp, false, CS, R, S, blob + y.kvn, 1e-6f, nullptr, 0, stat, part, W(L_KVN_W), nullptr,
                               nullptr, 0, ln.s));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_KVN);
      TRY_G(linear_bwd(st, dcp, R, tp + tt.ctx, blob + y.kvd, CS, R, H, nullptr, W(L_KVD_W), dctx, part, sr, true));  // (dctx: summed over layers)
      EDTTS_STOP_AFTER(l, EDTTS_BWD_KVD);
      // self-attention branch: h1 = h0 + att1 Wproj^T + b
      TRY_G(linear_bwd(st, dh, H, tp + z.att1, blob + y.g_proj, M, H, H, W(L_PROJ_B), W(L_PROJ_W), ga, part, tr));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_PROJ);
      const Act qkv = tp + z.qkv;
      TRY_G(attn_bwd(st, lo, B, qkv, 3 * H, qkv + H, qkv + 2 * H, 3 * H, tp + z.att1, ga, tp + z.lse1, delta, big, 3 * H, big + H, big + 2 * H,
                     3 * H, T, T, window, D(DROP_ATTN), ln.t, ln.t));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_SELF);
      TRY_G(G::norm<NORM_RMS>(st, tp + z.h0, xn, M, H, blob + y.n1w, nullptr, 1e-6f, cond_row + l * row, T, cb));
      TRY_G(linear_bwd(st, big, 3 * H, xn, blob + y.s_qkv, M, 3 * H, H, nullptr, W(L_QKV_W), ga, part, tr));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_QKV);
      TRY_G(norm_bwd<NORM_RMS>(st, tp + z.h0, ga, dh, true, M, H, T, blob + y.n1w, 1e-6f, cond_row + l * row, cb, stat, part, W(L_N1_W), nullptr,
                               dmod + l * row, cb, ln.t));
      EDTTS_STOP_AFTER(l, EDTTS_BWD_N1);
    }
    // in_proj
    TRY_G(linear_bwd(st, dh, H, x, blob + lo.inp, M, H, MEL, GG(G_INP_B), GG(G_INP_W), d_x, part, tr));
    EDTTS_STOP_AFTER(0, EDTTS_BWD_INP);
    // context sources
    if (sem_feat) {
      TRY_G(linear_bwd(st, dctx, H, sem_feat, blob + lo.semp, CS, H, lo.SD, GG(G_SEMP_B), GG(G_SEMP_W), d_sem, part, sr));
      if (GG(G_TOK)) HIP_TRY(hipMemsetAsync(GG(G_TOK), 0, (size_t)lo.NTOK * H * sizeof(float), st));  // (does not enter the output)
    } else {
      if (GG(G_SEMP_W)) HIP_TRY(hipMemsetAsync(GG(G_SEMP_W), 0, (size_t)H * lo.SD * sizeof(float), st));
      if (GG(G_SEMP_B)) HIP_TRY(hipMemsetAsync(GG(G_SEMP_B), 0, (size_t)H * sizeof(float), st));
    }
    if (!sem_feat && GG(G_TOK)) {
      hipLaunchKernelGGL(edtts_bwd::k_bwd_scatter_rows, dim3(lo.NTOK), dim3(256), 0, st, sem_idx, CS, lo.NTOK, dctx, H, GG(G_TOK), ln.s, S);
      LAUNCH_CHECK("k_bwd_scatter_rows");
    }
    if (GG(G_STEP) && !step_idx) HIP_TRY(hipMemsetAsync(GG(G_STEP), 0, (size_t)lo.NSTEP * H * sizeof(float), st));  // (likewise)
    EDTTS_STOP_AFTER(0, EDTTS_BWD_SEM);
    // conditioning path: AdaLN projections, then the time MLP and step_emb
    bool any_proj = false;
    for (int l = 0; l < L; ++l)
      any_proj = any_proj || gs[G_COUNT + l * L_COUNT + L_N1P_W] || gs[G_COUNT + l * L_COUNT + L_N1P_B] ||
                 gs[G_COUNT + l * L_COUNT + L_N3P_W] || gs[G_COUNT + l * L_COUNT + L_N3P_B];
    const bool any_time = GG(G_T1_W) || GG(G_T1_B) || GG(G_T3_W) || GG(G_T3_B) || GG(G_STEP);
    if (!any_proj && !any_time) return EDTTS_OK;
    const float* tcond = tp + tt.tcond;
    float *dtc = sc + ss.dtc, *e = sc + ss.e, *a1 = sc + ss.a1, *u1 = sc + ss.u1, *du1 = sc + ss.du1;
    HIP_TRY(hipMemsetAsync(dtc, 0, (size_t)B * H * sizeof(float), st));
    for (int l = 0; l < L; ++l) {
      const LayerLayout& y = lo.layer[l];
      for (int which = 0; which < 2; ++which) {
        const float* dm = dmod + l * row + which * 2 * H;
        float* gw = gs[G_COUNT + l * L_COUNT + (which ? L_N3P_W : L_N1P_W)];
        float* gb = gs[G_COUNT + l * L_COUNT + (which ? L_N3P_B : L_N1P_B)];
        TRY_G(linear_bwd(st, dm, cb, tcond, blob + (which ? y.ada3T : y.ada1T), B, 2 * H, H, gb, gw, dtc, part, RowLens{}, true, true));
      }
    }
    EDTTS_STOP_AFTER(0, EDTTS_BWD_ADA);
    if (!any_time) return EDTTS_OK;
    if (GG(G_STEP) && step_idx) {
      hipLaunchKernelGGL(edtts_bwd::k_bwd_scatter_rows, dim3(lo.NSTEP), dim3(256), 0, st, step_idx, B, lo.NSTEP, dtc, H, GG(G_STEP),
                         (const int64_t*)nullptr, 0);
      LAUNCH_CHECK("k_bwd_scatter_rows");
    }
    EDTTS_STOP_AFTER(0, EDTTS_BWD_STEP);
    // t_cond = W3 GELU(W1 e + b1) + b3: recompute e, the pre-activation and the hidden row
    hipLaunchKernelGGL(edtts_bwd::k_bwd_time_emb, dim3(G::grid_1d((size_t)B * H)), dim3(256), 0, st, t, blob + lo.freqs, B, H, e);
    LAUNCH_CHECK("k_bwd_time_emb");
    {
      edtts_bwd::BGemmArgs a;  // a1 = e W1^T (the blob keeps W1 transposed)
      memset(&a, 0, sizeof(a));
      a.A = e; a.B = blob + lo.t1T; a.C = a1; a.M = B; a.N = H; a.K = H; a.sam = H; a.sak = 1; a.sbn = 1; a.sbk = H; a.ldc = H;
      a.kslab = (H + 15) / 16 * 16;
      TRY_G(bgemm(st, a, 1, false));
    }
    hipLaunchKernelGGL(edtts_bwd::k_bwd_gelu, dim3(G::grid_1d((size_t)B * H)), dim3(256), 0, st, a1, blob + lo.t1b, B, H, u1);
    LAUNCH_CHECK("k_bwd_gelu");
    TRY_G(linear_bwd(st, dtc, H, u1, blob + lo.t3T, B, H, H, GG(G_T3_B), GG(G_T3_W), du1, part, RowLens{}, false, true));
    hipLaunchKernelGGL(edtts_bwd::k_bwd_gelu_grad, dim3(G::grid_1d((size_t)B * H)), dim3(256), 0, st, du1, a1, B * H);
    LAUNCH_CHECK("k_bwd_gelu_grad");
    return linear_bwd(st, du1, H, e, nullptr, B, H, H, GG(G_T1_B), GG(G_T1_W), nullptr, part);  // (EDTTS_BWD_TIME: the call's end)
#undef EDTTS_STOP_AFTER
  }
  // Which of the tail's optional sites a call with these gradient slots has (the launch list above skips the others)
  static bool has_site(const Layout& lo, float* const* gs, const int64_t* step_idx, bool dropping, int site) {
    using namespace edtts_gen;
    bool any_proj = false;
    for (int l = 0; l < lo.L; ++l)
      any_proj = any_proj || gs[G_COUNT + l * L_COUNT + L_N1P_W] || gs[G_COUNT + l * L_COUNT + L_N1P_B] ||
                 gs[G_COUNT + l * L_COUNT + L_N3P_W] || gs[G_COUNT + l * L_COUNT + L_N3P_B];
    const bool any_time = gs[G_T1_W] || gs[G_T1_B] || gs[G_T3_W] || gs[G_T3_B] || gs[G_STEP];
    switch (site) {
      case EDTTS_BWD_DROPDOWN: return dropping;
      case EDTTS_BWD_ADA: return any_proj || any_time;
      case EDTTS_BWD_STEP: return any_time && gs[G_STEP] && step_idx;
      case EDTTS_BWD_TIME: return any_time;
      default: return site >= 0 && site < EDTTS_BWD_COUNT;
    }
  }
};

// =========================================================================================================
// the C ABI of training: a forward that keeps a tape, the backward from it, the dropout masks
// =========================================================================================================
// EdttsDropout -> DropState.  *on = false for NULL or p == 0 (the call then makes exactly the launches of its plain twin).
// key: the seed in device memory (the *_dev entry points; drop->seed is then not read), or nullptr.
static int drop_state(const EdttsDropout* drop, const char* who, DropState* ds, bool* on, const uint64_t* key = nullptr) {
  *on = false;
  if (!drop || drop->p == 0.0f) return EDTTS_OK;
  const float p = drop->p;
  const double thr = nearbyint((double)p * 65536.0);  // (ties to even, as round() of the tests' restatement)
  if (!(p >= 0.0f && p < 1.0f) || thr > 65535.0)
    return fail(EDTTS_ERR_ARG, "%s: dropout p=%g is outside [0, 1) (needs round(p * 65536) <= 65535)", who, (double)p);
  ds->k0 = (unsigned)drop->seed;
  ds->k1 = (unsigned)(drop->seed >> 32);
  ds->key = reinterpret_cast<const unsigned*>(key);
  ds->thr = (unsigned)thr;
  ds->scale = 65536.0f / (float)(65536u - ds->thr);
  *on = true;
  return EDTTS_OK;
}

// EdttsDropoutDev -> the EdttsDropout (seed 0) and the device key that drop_state takes
static int drop_dev(const EdttsDropoutDev* dev, const char* who, EdttsDropout* host, const uint64_t** key) {
  *host = EdttsDropout{dev ? dev->p : 0.0f, 0};
  *key = dev ? dev->key : nullptr;
  if (dev && !dev->key) return fail(EDTTS_ERR_ARG, "%s: drop->key is NULL", who);
  if (dev && ((size_t)dev->key & 7)) return fail(EDTTS_ERR_ARG, "%s: drop->key is not 8-byte aligned", who);
  return EDTTS_OK;
}

static int decoder_forward_train_impl(const EdttsDims* dims, const void* packed, void* workspace, void* tape, int B, int T, int S,
                                      const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                                      const float* sem_features, float* eps, const EdttsDropout* drop, const uint64_t* key,
                                      const int64_t* t_len, const int64_t* s_len, void* stream);
static int decoder_backward_impl(const EdttsDims* dims, const void* packed, void* workspace, const void* tape, int B, int T, int S,
                                 const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx, const float* sem_features,
                                 const float* d_eps, void* const* grad_slots, int n_slots, float* d_x, float* d_sem_features, void* scratch,
                                 const EdttsDropout* drop, const uint64_t* key, const int64_t* t_len, const int64_t* s_len, void* stream,
                                 BwdStop stop = BwdStop{});
static int dropout_mask_impl(const EdttsDims* dims, int site, int layer, int B, int T, int S, const EdttsDropout* drop, const uint64_t* key,
                             uint8_t* keep, void* stream);

extern "C" {

int edtts_train_dw_slab_rows(int rows) { return edtts_bwd::dw_slab_rows(rows); }

int edtts_train_tape_bytes(const EdttsDims* dims, int B, int T, int S, size_t* out_bytes) {
  Layout lo;
  TRY_G(train_layout(dims, "edtts_train_tape_bytes", &lo));
  if (!out_bytes) return fail(EDTTS_ERR_ARG, "out_bytes is NULL");
  TRY_G(check_shapes(lo, B, T, S));
  TrainTape tt;
  make_tape(lo, B, T, S, &tt);
  *out_bytes = tt.total * sizeof(float);
  return EDTTS_OK;
}

int edtts_train_tape_region(const EdttsDims* dims, int B, int T, int S, int layer, int which, size_t* offset_bytes, size_t* bytes,
                            int* elem_bytes) {
  Layout lo;
  TRY_G(train_layout(dims, "edtts_train_tape_region", &lo));
  if (!offset_bytes || !bytes || !elem_bytes) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  TRY_G(check_shapes(lo, B, T, S));
  if (layer < 0 || layer >= lo.L) return fail(EDTTS_ERR_ARG, "edtts_train_tape_region: layer %d outside [0, %d)", layer, lo.L);
  TrainTape tt;
  make_tape(lo, B, T, S, &tt);
  TapePlace at{0, 0};
  size_t n = 0;
  const TrainTape& ct = tt;
  tape_regions(lo, B, T, S, ct, [&](int w, int l, const auto& m, size_t count) {  // (the whole-model members: the same answer for every layer)
    if (w == which && (l < 0 || l == layer)) { at = tape_place_of(m); n = count; }
  });
  if (!at.elem_bytes) return fail(EDTTS_ERR_ARG, "edtts_train_tape_region: which=%d is not one of EDTTS_TAPE_CRP .. EDTTS_TAPE_HL", which);
  *elem_bytes = at.elem_bytes;
  *offset_bytes = at.off * sizeof(float);
  *bytes = n * (size_t)at.elem_bytes;
  return EDTTS_OK;
}

int edtts_train_scratch_bytes(const EdttsDims* dims, int B, int T, int S, size_t* out_bytes) {
  Layout lo;
  TRY_G(train_layout(dims, "edtts_train_scratch_bytes", &lo));
  if (!out_bytes) return fail(EDTTS_ERR_ARG, "out_bytes is NULL");
  TRY_G(check_shapes(lo, B, T, S));
  TrainScratch ss;
  make_train_scratch(lo, B, T, S, &ss);
  *out_bytes = ss.total * sizeof(float);
  return EDTTS_OK;
}

int edtts_train_scratch_region(const EdttsDims* dims, int B, int T, int S, int which, size_t* offset_bytes, size_t* bytes) {
  Layout lo;
  TRY_G(train_layout(dims, "edtts_train_scratch_region", &lo));
  if (!offset_bytes || !bytes) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  TRY_G(check_shapes(lo, B, T, S));
  TrainScratch ss;
  make_train_scratch(lo, B, T, S, &ss);
  bool found = false;
  const TrainScratch& cs = ss;
  scratch_regions(lo, B, T, S, cs, [&](int w, const size_t& m, size_t n) {
    if (w == which) { *offset_bytes = m * sizeof(float); *bytes = n * sizeof(float); found = true; }
  });
  if (!found) return fail(EDTTS_ERR_ARG, "edtts_train_scratch_region: which=%d is not one of EDTTS_SCRATCH_DH .. EDTTS_SCRATCH_PART", which);
  return EDTTS_OK;
}

int edtts_decoder_forward_train(const EdttsDims* dims, const void* packed, void* workspace, void* tape, int B, int T, int S, const float* x,
                                const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx, const float* sem_features, float* eps,
                                void* stream) {
  return edtts_decoder_forward_train_drop(dims, packed, workspace, tape, B, T, S, x, t, step_idx, sem_idx, sem_features, eps, nullptr, stream);
}

int edtts_decoder_forward_train_drop(const EdttsDims* dims, const void* packed, void* workspace, void* tape, int B, int T, int S,
                                     const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                                     const float* sem_features, float* eps, const EdttsDropout* drop, void* stream) {
  return edtts_decoder_forward_train_len(dims, packed, workspace, tape, B, T, S, x, t, step_idx, sem_idx, sem_features, eps, drop, nullptr,
                                         nullptr, stream);
}

int edtts_decoder_forward_train_len(const EdttsDims* dims, const void* packed, void* workspace, void* tape, int B, int T, int S,
                                    const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                                    const float* sem_features, float* eps, const EdttsDropout* drop, const int64_t* t_len,
                                    const int64_t* s_len, void* stream) {
  return decoder_forward_train_impl(dims, packed, workspace, tape, B, T, S, x, t, step_idx, sem_idx, sem_features, eps, drop, nullptr, t_len,
                                    s_len, stream);
}

int edtts_decoder_forward_train_dev(const EdttsDims* dims, const void* packed, void* workspace, void* tape, int B, int T, int S,
                                    const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                                    const float* sem_features, float* eps, const EdttsDropoutDev* drop, const int64_t* t_len,
                                    const int64_t* s_len, void* stream) {
  EdttsDropout host;
  const uint64_t* key;
  TRY_G(drop_dev(drop, "edtts_decoder_forward_train_dev", &host, &key));
  return decoder_forward_train_impl(dims, packed, workspace, tape, B, T, S, x, t, step_idx, sem_idx, sem_features, eps, drop ? &host : nullptr,
                                    key, t_len, s_len, stream);
}

}  // extern "C"

static int decoder_forward_train_impl(const EdttsDims* dims, const void* packed, void* workspace, void* tape, int B, int T, int S,
                                      const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx,
                                      const float* sem_features, float* eps, const EdttsDropout* drop, const uint64_t* key,
                                      const int64_t* t_len, const int64_t* s_len, void* stream) {
  const SettingsScope settings;
  Layout lo;
  TRY_G(train_layout(dims, "edtts_decoder_forward_train", &lo));
  DropState ds;
  bool dropping;
  TRY_G(drop_state(drop, "edtts_decoder_forward_train_drop", &ds, &dropping, key));
  if (!sem_idx && !sem_features) return fail(EDTTS_ERR_ARG, "Either sem_idx or sem_features must be provided");
  if (!packed || !workspace || !tape || !x || !t || !eps) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  TRY_G(check_shapes(lo, B, T, S));
  hipStream_t st = (hipStream_t)stream;
  const float* blob = (const float*)packed;
  float* wsb = (float*)workspace;
  float* tp = (float*)tape;
  Workspace ws;
  make_workspace(lo, B, T, S, B, &ws);
  TrainTape tt;
  make_tape(lo, B, T, S, &tt);
  TRY_G(launch_len_check(t_len, s_len, B, T, S, wsb, st));
  TRY_G(launch_cond(lo, blob, t, step_idx, nullptr, B, tp + tt.cond, wsb, st));  // the AdaLN rows and t_cond go straight to the tape
  const CallCtx c{lo, blob, ws, wsb, B, T, S, dims->window, Lens{t_len, s_len}, st};
  return TrainLauncher::forward(c, tp, tt, x, sem_features ? nullptr : sem_idx, sem_features, eps, dropping ? &ds : nullptr);
}

extern "C" {

int edtts_decoder_backward(const EdttsDims* dims, const void* packed, void* workspace, const void* tape, int B, int T, int S, const float* x,
                           const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx, const float* sem_features, const float* d_eps,
                           void* const* grad_slots, int n_slots, float* d_x, float* d_sem_features, void* scratch, void* stream) {
  return edtts_decoder_backward_drop(dims, packed, workspace, tape, B, T, S, x, t, step_idx, sem_idx, sem_features, d_eps, grad_slots, n_slots,
                                     d_x, d_sem_features, scratch, nullptr, stream);
}

int edtts_decoder_backward_drop(const EdttsDims* dims, const void* packed, void* workspace, const void* tape, int B, int T, int S,
                                const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx, const float* sem_features,
                                const float* d_eps, void* const* grad_slots, int n_slots, float* d_x, float* d_sem_features, void* scratch,
                                const EdttsDropout* drop, void* stream) {
  return edtts_decoder_backward_len(dims, packed, workspace, tape, B, T, S, x, t, step_idx, sem_idx, sem_features, d_eps, grad_slots, n_slots,
                                    d_x, d_sem_features, scratch, drop, nullptr, nullptr, stream);
}

int edtts_decoder_backward_len(const EdttsDims* dims, const void* packed, void* workspace, const void* tape, int B, int T, int S,
                               const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx, const float* sem_features,
                               const float* d_eps, void* const* grad_slots, int n_slots, float* d_x, float* d_sem_features, void* scratch,
                               const EdttsDropout* drop, const int64_t* t_len, const int64_t* s_len, void* stream) {
  return decoder_backward_impl(dims, packed, workspace, tape, B, T, S, x, t, step_idx, sem_idx, sem_features, d_eps, grad_slots, n_slots, d_x,
                               d_sem_features, scratch, drop, nullptr, t_len, s_len, stream);
}

int edtts_decoder_backward_until(const EdttsDims* dims, const void* packed, void* workspace, const void* tape, int B, int T, int S,
                                 const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx, const float* sem_features,
                                 const float* d_eps, void* const* grad_slots, int n_slots, float* d_x, float* d_sem_features, void* scratch,
                                 const EdttsDropout* drop, const int64_t* t_len, const int64_t* s_len, int stop_layer, int stop_site,
                                 void* stream) {
  if (stop_site < 0) return fail(EDTTS_ERR_ARG, "edtts_decoder_backward_until: stop_site %d is not one of EDTTS_BWD_*", stop_site);
  return decoder_backward_impl(dims, packed, workspace, tape, B, T, S, x, t, step_idx, sem_idx, sem_features, d_eps, grad_slots, n_slots, d_x,
                               d_sem_features, scratch, drop, nullptr, t_len, s_len, stream, BwdStop{stop_layer, stop_site});
}

int edtts_decoder_backward_dev(const EdttsDims* dims, const void* packed, void* workspace, const void* tape, int B, int T, int S,
                               const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx, const float* sem_features,
                               const float* d_eps, void* const* grad_slots, int n_slots, float* d_x, float* d_sem_features, void* scratch,
                               const EdttsDropoutDev* drop, const int64_t* t_len, const int64_t* s_len, void* stream) {
  EdttsDropout host;
  const uint64_t* key;
  TRY_G(drop_dev(drop, "edtts_decoder_backward_dev", &host, &key));
  return decoder_backward_impl(dims, packed, workspace, tape, B, T, S, x, t, step_idx, sem_idx, sem_features, d_eps, grad_slots, n_slots, d_x,
                               d_sem_features, scratch, drop ? &host : nullptr, key, t_len, s_len, stream);
}

int edtts_dropout_mask(const EdttsDims* dims, int site, int layer, int B, int T, int S, const EdttsDropout* drop, uint8_t* keep, void* stream) {
  return dropout_mask_impl(dims, site, layer, B, T, S, drop, nullptr, keep, stream);
}

int edtts_dropout_mask_dev(const EdttsDims* dims, int site, int layer, int B, int T, int S, const EdttsDropoutDev* drop, uint8_t* keep,
                           void* stream) {
  EdttsDropout host;
  const uint64_t* key;
  TRY_G(drop_dev(drop, "edtts_dropout_mask_dev", &host, &key));
  return dropout_mask_impl(dims, site, layer, B, T, S, drop ? &host : nullptr, key, keep, stream);
}

}  // extern "C"

static int decoder_backward_impl(const EdttsDims* dims, const void* packed, void* workspace, const void* tape, int B, int T, int S,
                                 const float* x, const int64_t* t, const int64_t* step_idx, const int64_t* sem_idx, const float* sem_features,
                                 const float* d_eps, void* const* grad_slots, int n_slots, float* d_x, float* d_sem_features, void* scratch,
                                 const EdttsDropout* drop, const uint64_t* key, const int64_t* t_len, const int64_t* s_len, void* stream,
                                 BwdStop stop) {
  Layout lo;
  TRY_G(train_layout(dims, "edtts_decoder_backward", &lo));
  DropState ds;
  bool dropping;
  TRY_G(drop_state(drop, "edtts_decoder_backward_drop", &ds, &dropping, key));
  if (!sem_idx && !sem_features) return fail(EDTTS_ERR_ARG, "Either sem_idx or sem_features must be provided");
  if (!packed || !workspace || !tape || !x || !t || !d_eps || !grad_slots || !scratch) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (n_slots != G_COUNT + lo.L * L_COUNT) return fail(EDTTS_ERR_ARG, "expected %d gradient slots, got %d", G_COUNT + lo.L * L_COUNT, n_slots);
  TRY_G(check_shapes(lo, B, T, S));
  if (stop.site >= 0) {  // (edtts_decoder_backward_until; every other entry point passes "never")
    if (stop.layer < 0 || stop.layer >= lo.L)
      return fail(EDTTS_ERR_ARG, "edtts_decoder_backward_until: stop_layer %d outside [0, %d)", stop.layer, lo.L);
    if (stop.site >= EDTTS_BWD_COUNT) return fail(EDTTS_ERR_ARG, "edtts_decoder_backward_until: stop_site %d is not one of EDTTS_BWD_*", stop.site);
    const bool per_layer = stop.site >= EDTTS_BWD_DROPDOWN && stop.site <= EDTTS_BWD_N1;
    if (!per_layer && stop.layer != 0)
      return fail(EDTTS_ERR_ARG, "edtts_decoder_backward_until: stop_site %d belongs to no layer, stop_layer must be 0", stop.site);
    if (!TrainLauncher::has_site(lo, reinterpret_cast<float* const*>(grad_slots), step_idx, dropping, stop.site))
      return fail(EDTTS_ERR_ARG, "edtts_decoder_backward_until: this call has no site %d (dropout, step_idx or the gradient slots it needs are absent)",
                  stop.site);
  }
  TrainTape tt;
  make_tape(lo, B, T, S, &tt);
  TrainScratch ss;
  make_train_scratch(lo, B, T, S, &ss);
  TRY_G(launch_len_check(t_len, s_len, B, T, S, (float*)workspace, (hipStream_t)stream));  // (the index-error word: the only use of `workspace`)
  return TrainLauncher::backward(lo, (const float*)packed, (const float*)tape, tt, (float*)scratch, ss, B, T, S, dims->window, x, t, step_idx,
                                 sem_features ? nullptr : sem_idx, sem_features, d_eps, reinterpret_cast<float* const*>(grad_slots), d_x,
                                 d_sem_features, (hipStream_t)stream, dropping ? &ds : nullptr, Lens{t_len, s_len}, stop);
}

static int dropout_mask_impl(const EdttsDims* dims, int site, int layer, int B, int T, int S, const EdttsDropout* drop, const uint64_t* key,
                             uint8_t* keep, void* stream) {
  Layout lo;
  TRY_G(train_layout(dims, "edtts_dropout_mask", &lo));
  if (!drop) return fail(EDTTS_ERR_ARG, "edtts_dropout_mask: drop is NULL");
  DropState ds{(unsigned)drop->seed, (unsigned)(drop->seed >> 32), 0u, 1.0f, reinterpret_cast<const unsigned*>(key)};  // (p == 0: threshold 0, everything kept)
  bool dropping;
  TRY_G(drop_state(drop, "edtts_dropout_mask", &ds, &dropping, key));
  if (site < DROP_ATTN || site > DROP_DOWN) return fail(EDTTS_ERR_ARG, "edtts_dropout_mask: site %d is not one of 0 .. 3", site);
  if (layer < 0 || layer >= lo.L) return fail(EDTTS_ERR_ARG, "edtts_dropout_mask: layer %d outside [0, %d)", layer, lo.L);
  if (!keep) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  TRY_G(check_shapes(lo, B, T, S));
  const bool attn = site == DROP_ATTN || site == DROP_CROSS;
  const size_t rows = attn ? (size_t)B * lo.HEADS * T : (size_t)B * T;
  const int W = site == DROP_ATTN ? T : site == DROP_CROSS ? S : site == DROP_ACT ? lo.FM * lo.H : lo.H;
  hipLaunchKernelGGL(edtts_bwd::k_drop_mask, dim3(GenericLauncher::grid_1d(rows * ((W + 3) / 4))), dim3(256), 0, (hipStream_t)stream, keep, rows,
                     W, T, (int)attn, ds.site(layer, site));
  LAUNCH_CHECK("k_drop_mask");
  return EDTTS_OK;
}
