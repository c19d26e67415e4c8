// edtts_semantic_bwd.h -- training the semantic head: proj and FSQEncoder / VectorQuantizer under autograd (included by
// edtts_kernels.hip behind edtts_semantic.h; DESIGN.md sections 21, 23 and 37).
//
// The training forward is k_sem_encode<true> (edtts_semantic.h): the inference chain, which also writes the tape (M = B T_feat rows)
//   FSQ: y1 = proj.0(h) before GELU [M][S] | z [M][S] (both only with a proj) | zb = tanh(proj_down(z)) [M][16]
//   VQ:  y1 | z (both only with a proj) | r = c - z [M][S] | sq [M] = sum_s r^2 per frame
// (r, not c: the EMA update overwrites the codebook before the backward runs, and both gradients are functions of r alone)
// and multiplies the LayerNorm output by the head's dropout mask (stream word 0x40000, positions as drop_row4 maps them).
//
//   k_sem_bwd_frames   the frame-local part of the backward in the forward's layout (64 frames per block, frame = lane & 15, the
//                      TRANSPOSED weights as the A operand, streamed through LDS by stream_rt):  G = d z_q ->
//                      d zq_low = Wu^T G -> du = d zq_low o (1 - zb^2) (the straight-through line passes the gradient to zb
//                      unchanged) -> dz = Wd^T du -> da = W3^T dz -> x dropout multiplier (regenerated) -> LayerNorm backward
//                      (statistics recomputed from y1 in fp64; the per-frame sums cross the four lane groups with __shfl_xor) ->
//                      erf-GELU derivative -> dy1.  It leaves du, zq_low, dz, the post-dropout LayerNorm output a, the masked da, x^ and dy1
//                      for the sums over frames, zero for frames at or past lengths[b].
//                      <true>, the VQ head: dz = G - coef[0] r, then the proj backward of the FSQ instantiation
//   k_sem_pack_fragT   the transposed matrices in fragment order (the training blob)
//   k_sem_vq_loss     sq -> vq_loss = L + commit L, L = sum sq / (N S): one block, fixed order, fp64 accumulation, rounded once
//   k_sem_codesum     out[K][S] = sum_m [idx[m] = k] X[m][:] as a one-hot GEMM on v_mfma_f32_16x16x4_f32: the one-hot A operand is
//                     made in registers from idx (a product by 1.0 or 0.0 is exact), a block owns one tile of 16 codes and one
//                     slab of dw_slab_rows(M) rows, which its four waves walk 64 rows at a time; a 4-row k-step in which no id
//                     falls into the tile is skipped (one ballot per 64 rows).  Waves are added in wave order, slabs in ascending
//                     order by k_bwd_slabsum: no float atomics.
//                     X = z for ema_w, X = r for the codebook gradient.
//   k_sem_vq_ema      counts and the code sums of z -> ema_cluster_size, ema_w, codebook.weight (one wave per code)
//   k_sem_vq_coef     N from the lengths and g = d vq_loss -> coef[0] = g commit 2 / (N S), coef[1] = g 2 / (N S)
//   k_sem_vq_dcb      d codebook = coef[1] x the code sums of r (rows of unused codes: exactly 0)
// The sums over frames reuse section 19's kernels (TrainLauncher::dw / colsum, k_bwd_norm_cols): fixed orders, no float atomics.
//
// The host side is written once for both quantizers: L.vq decides which members a layout has and which kernel instance runs.
namespace edtts_sem {

// Training blob (floats), each matrix rt-major in fragment order: FSQ Wu^T [16][S] | Wd^T [S][16], then with a proj W3^T [S][S]
// (a VQ head without a proj has nothing to pack).
struct SemTrainLayout {
  size_t wuT, wdT, w3T, total;
};
static SemTrainLayout sem_train_layout(const SemLayout& L) {
  SemTrainLayout R{};
  auto take = [&](size_t floats) { size_t r = R.total; R.total += (floats + 3) & ~(size_t)3; return r; };
  if (!L.vq) {
    R.wuT = take((size_t)L.nt * 64 * 4);
    R.wdT = take((size_t)L.nt * 64 * 4);
  }
  if (L.in_dim) R.w3T = take((size_t)L.nt * L.nt * 64 * 4);
  return R;
}

// The tape and the backward's scratch, each stated once (as tape_regions / scratch_regions state the decoder's, edtts_generic_bwd.h):
// f(which, member, n) for every member the head has, in memory order -- `which` its EDTTS_SEM_TAPE_* / EDTTS_SEM_SCRATCH_* name,
// `member` its place in the struct, n its float count.  sem_tape / sem_scratch lay the memory out from the walk,
// edtts_sem_train_region answers from it, the launchers reach the members through the offsets it filled.  The members of the other
// quantizer, and those of a proj the head does not have, stay 0.
struct SemTape {
  size_t y1, z, zb, r, sq, total;
};
template <class Tape, class F>
static void sem_tape_regions(const SemLayout& L, size_t M, Tape& t, F&& f) {
  const size_t MS = M * L.S;
  if (L.in_dim) { f(EDTTS_SEM_TAPE_Y1, t.y1, MS); f(EDTTS_SEM_TAPE_Z, t.z, MS); }  // (without a proj z is the caller's input)
  if (L.vq) { f(EDTTS_SEM_TAPE_R, t.r, MS); f(EDTTS_SEM_TAPE_SQ, t.sq, M); }
  else f(EDTTS_SEM_TAPE_ZB, t.zb, 16 * M);
}
// (the members follow each other directly: all but sq, the last one, are multiples of 16 floats)
static SemTape sem_tape(const SemLayout& L, size_t M) {
  SemTape t{};
  sem_tape_regions(L, M, t, [&](int, size_t& m, size_t n) { m = t.total; t.total += n; });
  return t;
}
// Scratch of the backward (and of the VQ head's EMA update): FSQ du | zq_low [M][16], dz | gm [M][S]; VQ coef [4] | csum [K][S] (the
// summed slabs of a code sum) and, with a proj, dz; with a proj a | dam | xh | dy1 [M][S] and stat [M][2]; then the partial sums of
// the reductions.  Every member starts on a multiple of 4 floats.
struct SemScratch {
  size_t du, zql, coef, csum, dz, gm, a, dam, xh, dy1, stat, part, total;
};
template <class Scratch, class F>
static void sem_scratch_regions(const SemLayout& L, int B, int T, Scratch& s, F&& f) {
  const size_t M = (size_t)B * T, S = L.S, MS = M * S;
  auto mx = [](size_t a, size_t b) { return a > b ? a : b; };
  if (L.vq) { f(EDTTS_SEM_SCRATCH_COEF, s.coef, 4); f(EDTTS_SEM_SCRATCH_CSUM, s.csum, (size_t)L.K * S); }
  else { f(EDTTS_SEM_SCRATCH_DU, s.du, 16 * M); f(EDTTS_SEM_SCRATCH_ZQL, s.zql, 16 * M); }
  if (!L.vq || L.in_dim) f(EDTTS_SEM_SCRATCH_DZ, s.dz, MS);  // (a VQ head without a proj: dz is the caller's d_z and nothing else)
  if (!L.vq) f(EDTTS_SEM_SCRATCH_GM, s.gm, MS);
  if (L.in_dim) {
    f(EDTTS_SEM_SCRATCH_A, s.a, MS); f(EDTTS_SEM_SCRATCH_DAM, s.dam, MS); f(EDTTS_SEM_SCRATCH_XH, s.xh, MS);
    f(EDTTS_SEM_SCRATCH_DY1, s.dy1, MS); f(EDTTS_SEM_SCRATCH_STAT, s.stat, 2 * M);
  }
  // partial sums: the largest of the slab partials [slabs][N][K] of a cut sum over frames, the bias partials and the LayerNorm partials
  const size_t r = edtts_bwd::dw_slab_rows((int)M), ns = (M + r - 1) / r;
  size_t part = 0;
  if (ns > 1) {
    part = ns * S * (L.vq ? (size_t)L.K : 16);                         // VQ: code-sum slabs; FSQ: proj_down / proj_up dW slabs
    if (L.in_dim) part = mx(part, ns * S * mx(S, (size_t)L.in_dim));  // proj's dW slabs
  }
  if (!L.vq || L.in_dim) part = mx(part, (M + edtts_bwd::kColRows - 1) / edtts_bwd::kColRows * S);                     // bias partials
  if (L.in_dim) part = mx(part, (size_t)B * (((size_t)T + edtts_bwd::kNormChunk - 1) / edtts_bwd::kNormChunk) * 3 * S);  // LayerNorm partials
  f(EDTTS_SEM_SCRATCH_PART, s.part, part);
}
static SemScratch sem_scratch(const SemLayout& L, int B, int T) {
  SemScratch s{};
  sem_scratch_regions(L, B, T, s, [&](int, size_t& m, size_t n) { m = s.total; s.total += (n + 3) & ~(size_t)3; });
  return s;
}

// dst (fragment order, rt-major) <- M^T for M [K][R] row-major: the packed matrix has R rows and K columns
__global__ void k_sem_pack_fragT(const float* __restrict__ M, int R, int K, int nrt, int nkb, float* __restrict__ dst) {
  const long long n = (long long)nrt * nkb * 256;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(e & 3), lane = (int)((e >> 2) & 63);
    const long long t = e >> 8;
    const int rt = (int)(t / nkb), kb = (int)(t % nkb);
    const int r = 16 * rt + (lane & 15), k = 16 * kb + 4 * (lane >> 4) + j;
    dst[e] = (r < R && k < K) ? M[(size_t)k * R + r] : 0.f;
  }
}

struct SemBwdArgs {
  const float* p;           // the inference blob: LayerNorm gain and bias, FSQ tables
  const float* pt;          // the training blob
  const float* g;           // d z_q [N][S]
  const long long* len;     // [B] or null
  const float *t_y1, *t_zb; // tape
  float *du, *zql, *dz, *gm, *a, *dam, *xh, *dy1, *stat;  // dz null: not wanted (in_dim 0); gm null: no lengths
  int N, T, in_dim, S, nt, D;
  size_t lng, lnb, half, lev, wuT, wdT, w3T;
  DropArgs dr;
  int dropping;
  const float* t_r;         // k_sem_bwd_frames<true>: the VQ tape's r = c - z [N][S]
  const float* coef;        // ... and coef[0] = g commit 2 / (N S) on the device (g: the incoming gradient of vq_loss)
};

// group_sum in fp64
EDTTS_DEV double group_sum_d(double v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// VQ: the head of the chain is dz = G - coef r (G = d z_q through the straight-through line, null: 0; the commitment loss's share
// from the tape's r), and everything from dz onward is the FSQ instantiation's.
template <bool VQ>
__global__ __launch_bounds__(256) void k_sem_bwd_frames(SemBwdArgs a) {
  __shared__ f4 buf[2][kChunk];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, grp = lane >> 4;
  const int frame = blockIdx.x * kFrames + 16 * w + (lane & 15);
  const bool in = frame < a.N;
  bool ok = in;
  if (ok && a.len) {
    const int b = frame / a.T, t = frame - b * a.T;
    long long n = a.len[b];
    n = n < 1 ? 1 : (n > a.T ? a.T : n);
    ok = t < n;
  }
  const float* p = a.p;
  const float* pt = a.pt;
  const int S = a.S, nt = a.nt;
  const size_t rd = (size_t)(ok ? frame : 0);           // the row this lane reads (frames that are not ok read nothing of their own)
  const size_t orow = (size_t)frame * S + 4 * grp;      // ... and writes (only when `in`)
  const size_t drow = (size_t)frame * 16 + 4 * grp;
  f4 X[kMaxNT], dz[kMaxNT];
  if constexpr (VQ) {
    const float coef = a.coef[0];
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t) {
      const f4 G = (ok && a.g && t < nt) ? ldg4(a.g + rd * S + 4 * grp + 16 * t) : splat(0.f);
      const f4 r = (ok && t < nt) ? ldg4(a.t_r + rd * S + 4 * grp + 16 * t) : splat(0.f);
      dz[t] = G - coef * r;
      X[t] = splat(0.f);
    }
  } else {
  // ---- G = d z_q as B fragments
#pragma unroll
  for (int t = 0; t < kMaxNT; ++t) X[t] = (ok && t < nt) ? ldg4(a.g + rd * S + 4 * grp + 16 * t) : splat(0.f);
  if (a.gm && in) {
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t)
      if (t < nt) stg4(a.gm + orow + 16 * t, X[t]);
  }
  // ---- d zq_low = Wu^T G (one 16-row tile); du = d zq_low o (1 - zb^2); zq_low recomputed from zb as the forward computes it
  f4 dzl = splat(0.f);
  stream_rt(reinterpret_cast<const f4*>(pt + a.wuT), 1, nt, nullptr, 0, X, buf, [&](int, f4 acc) { dzl = acc; });
  {
    const f4 zb = ok ? ldg4(a.t_zb + rd * 16 + 4 * grp) : splat(0.f);
    const int* lev = reinterpret_cast<const int*>(p + a.lev);
    f4 du = splat(0.f), zq = splat(0.f);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int d = 4 * grp + r;
      if (ok && d < a.D) {
        const float half = p[a.half + d];
        float q = rintf((zb[r] + 1.0f) * half);
        q = fminf(fmaxf(q, 0.0f), (float)(lev[d] - 1));
        q = q / half - 1.0f;
        zq[r] = zb[r] + (q - zb[r]);
        du[r] = dzl[r] * (1.0f - zb[r] * zb[r]);
      }
    }
    if (in) {
      stg4(a.du + drow, du);
      stg4(a.zql + drow, zq);
    }
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t) X[t] = splat(0.f);
    X[0] = du;
  }
  // ---- dz = Wd^T du
#pragma unroll
  for (int t = 0; t < kMaxNT; ++t) dz[t] = splat(0.f);
  stream_rt(reinterpret_cast<const f4*>(pt + a.wdT), nt, 1, nullptr, 0, X, buf, [&](int rt, f4 acc) {
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t)
      if (t == rt) dz[t] = acc;
  });
  }
  if (a.dz && in) {
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t)
      if (t < nt) stg4(a.dz + orow + 16 * t, dz[t]);
  }
  if (!a.in_dim) return;  // the quantizer alone: dz is the input gradient
  // ---- da = W3^T dz
#pragma unroll
  for (int t = 0; t < kMaxNT; ++t) X[t] = splat(0.f);
  stream_rt(reinterpret_cast<const f4*>(pt + a.w3T), nt, nt, nullptr, 0, dz, buf, [&](int rt, f4 acc) {
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t)
      if (t == rt) X[t] = acc;
  });
  // ---- LayerNorm statistics from y1.  The gain gradient sums da o x^ over frames and x^ = (g - mean) rstd multiplies every rounding
  // of g = GELU(y1) by rstd (several units when a frame's activations lie close together), so GELU, its derivative, the statistics
  // and the two per-frame sums of the LayerNorm backward are evaluated in fp64 here and rounded once: y1 then holds GELU'(y1).
  f4 y1[kMaxNT], xh[kMaxNT];
  double s = 0.0;
#pragma unroll
  for (int t = 0; t < kMaxNT; ++t) {
    y1[t] = (ok && t < nt) ? ldg4(a.t_y1 + rd * S + 4 * grp + 16 * t) : splat(0.f);
    xh[t] = splat(0.f);
    if (t < nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double yv = (double)y1[t][r];
        const double cdf = 0.5 * (1.0 + erf(yv * 0.70710678118654752440));
        xh[t][r] = (float)(yv * cdf);
        y1[t][r] = (float)(cdf + yv * 0.39894228040143267794 * exp(-0.5 * yv * yv));
        s += (double)xh[t][r];
      }
    }
  }
  const double mean = group_sum_d(s) / (double)S;
  double v = 0.0;
#pragma unroll
  for (int t = 0; t < kMaxNT; ++t)
    if (t < nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double d = (double)xh[t][r] - mean;
        v = fma(d, d, v);
      }
    }
  const double rstd_d = 1.0 / sqrt(group_sum_d(v) / (double)S + 1e-5);
  const float rstd = (float)rstd_d;
  // ---- x dropout multiplier; a = (x^ gain + bias) o mask; gx = da o gain and its two per-frame sums
  double s1 = 0.0, s2 = 0.0;
  const DropArgs dr = a.dropping ? drop_live(a.dr) : DropArgs{};
#pragma unroll
  for (int t = 0; t < kMaxNT; ++t) {
    if (t < nt) {
      const f4 dm = a.dropping ? drop_row4(dr, frame, 16 * t + 4 * grp) : splat(1.0f);
      f4 av, dam;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * t + 4 * grp + r;
        const float xv = (float)(((double)xh[t][r] - mean) * rstd_d);
        xh[t][r] = ok ? xv : 0.f;
        av[r] = ok ? (xv * p[a.lng + f] + p[a.lnb + f]) * dm[r] : 0.f;
        dam[r] = X[t][r] * dm[r];  // (zero for frames that are not ok: G is)
        X[t][r] = dam[r] * p[a.lng + f];
        s1 += (double)X[t][r];
        s2 += (double)X[t][r] * (double)xh[t][r];
      }
      if (in) {
        stg4(a.a + orow + 16 * t, av);
        stg4(a.dam + orow + 16 * t, dam);
        stg4(a.xh + orow + 16 * t, xh[t]);
      }
    }
  }
  const float m1 = (float)(group_sum_d(s1) / (double)S), m2 = (float)(group_sum_d(s2) / (double)S);
  // ---- LayerNorm backward, then the GELU derivative
  if (in) {
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t)
      if (t < nt) {
        f4 dy;
#pragma unroll
        for (int r = 0; r < 4; ++r) dy[r] = rstd * (X[t][r] - m1 - xh[t][r] * m2) * y1[t][r];
        stg4(a.dy1 + orow + 16 * t, dy);
      }
    if (grp == 0) {  // k_bwd_norm_cols reads (x - mean) rstd: x^ is stored, so its statistics are (0, 1)
      a.stat[2 * (size_t)frame] = 0.f;
      a.stat[2 * (size_t)frame + 1] = 1.0f;
    }
  }
}

// the number of valid frames: sum of the clamped lengths (len null: B T), every thread of the block gets it
EDTTS_DEV long long vq_valid_frames(const long long* len, int B, int T, long long* sl) {
  const int tid = threadIdx.x;
  long long n = 0;
  if (len) {
    for (int b = tid; b < B; b += 256) {
      const long long v = len[b];
      n += v < 1 ? 1 : (v > T ? T : v);
    }
  }
  sl[tid] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sl[tid] += sl[tid + o];
    __syncthreads();
  }
  const long long tot = len ? sl[0] : (long long)B * T;
  __syncthreads();
  return tot;
}

// loss[0] = L + commit L with L = (sum_m sq[m]) / (N S) (training == 0: 0).  sq of a frame past its length is 0.
__global__ __launch_bounds__(256) void k_sem_vq_loss(const float* __restrict__ sq, int M, const long long* __restrict__ len, int B, int T, int S,
                                                     float commit, int training, float* __restrict__ loss) {
  __shared__ double sd[256];
  __shared__ long long sl[256];
  const int tid = threadIdx.x;
  const long long N = vq_valid_frames(len, B, T, sl);
  double s = 0.0;
  for (int m = tid; m < M; m += 256) s += (double)sq[m];
  sd[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sd[tid] += sd[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const float L = N > 0 ? (float)(sd[0] / ((double)N * (double)S)) : 0.f;
    *loss = training ? L + commit * L : 0.f;
  }
}

// coef[0] = g commit 2 / (N S), coef[1] = g 2 / (N S); g = *d_loss (null: 0)
__global__ __launch_bounds__(256) void k_sem_vq_coef(const float* __restrict__ d_loss, const long long* __restrict__ len, int B, int T, int S,
                                                     float commit, float* __restrict__ coef) {
  __shared__ long long sl[256];
  const long long N = vq_valid_frames(len, B, T, sl);
  if (threadIdx.x == 0) {
    const double g = d_loss ? (double)*d_loss : 0.0;
    const double c = N > 0 ? g * 2.0 / ((double)N * (double)S) : 0.0;
    coef[0] = (float)(c * (double)commit);
    coef[1] = (float)c;
  }
}

struct CodeSumArgs {
  const long long* idx;   // [M]
  const float* X;         // [M][S]
  const long long* len;   // [B] or null
  float* out;             // [slab][K][S]
  int M, T, S, nt, K, nrt_codes, slab_rows;
};
// grid (nrt_codes, slabs): block (x, y) owns code tile x of slab y.  Its four waves take the slab's 64-row chunks in turn (wave w:
// chunks w, w + 4, ...), rows ascending through the MFMA's fixed k order, and the four partial tiles are added through LDS in wave
// order ((w0 + w1) + w2) + w3: the result is a function of the inputs alone.
__global__ __launch_bounds__(256) void k_sem_codesum(CodeSumArgs a) {
  __shared__ float red[3][kMaxNT * 4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, fq = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x;
  const int r0 = blockIdx.y * a.slab_rows, r1 = r0 + a.slab_rows < a.M ? r0 + a.slab_rows : a.M;
  const int S = a.S, nt = a.nt;
  f4 acc[kMaxNT];
#pragma unroll
  for (int t = 0; t < kMaxNT; ++t) acc[t] = splat(0.f);
  for (int base = r0 + 64 * w; base < r1; base += 256) {
    // lane l: the id of row base + l, -1 when the row is past the slab or past its utterance's length
    const int m = base + lane;
    int id = -1;
    if (m < r1) {
      bool live = true;
      if (a.len) {
        const int b = m / a.T, t = m - b * a.T;
        long long n = a.len[b];
        n = n < 1 ? 1 : (n > a.T ? a.T : n);
        live = t < n;
      }
      if (live) id = (int)a.idx[m];
    }
    const unsigned long long hits = __ballot(id >= 0 && (id >> 4) == tile);
    if (hits == 0ull) continue;
#pragma unroll 1
    for (int q = 0; q < 16; ++q) {
      const int rid = __shfl(id, 4 * q + g);  // the id of this lane's row of the k-step (every lane takes part)
      if (((hits >> (4 * q)) & 0xfull) == 0ull) continue;  // (wave-uniform)
      const float one = rid == 16 * tile + fq ? 1.0f : 0.0f;
      const float* xp = a.X + (size_t)(base + 4 * q + g) * S + fq;
#pragma unroll
      for (int t = 0; t < kMaxNT; ++t)
        if (t < nt) acc[t] = EDTTS_MFMA(one, rid >= 0 ? xp[16 * t] : 0.f, acc[t]);
    }
  }
  if (w > 0) {
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t)
      if (t < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w - 1][4 * t + r][lane] = acc[t][r];
      }
  }
  __syncthreads();
  if (w > 0) return;
  // acc[t][r] = out[code 16 tile + 4 g + r][feature 16 t + fq]
  float* o = a.out + (size_t)blockIdx.y * a.K * S;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = 16 * tile + 4 * g + r;
    if (c < a.K) {
#pragma unroll
      for (int t = 0; t < kMaxNT; ++t)
        if (t < nt) o[(size_t)c * S + 16 * t + fq] = ((acc[t][r] + red[0][4 * t + r][lane]) + red[1][4 * t + r][lane]) + red[2][4 * t + r][lane];
    }
  }
}

// One wave per code k: n' = ema_cluster_size[k] decay + (1 - decay) counts[k]; ema_w[k] = ema_w[k] decay + (1 - decay) csum[k];
// codebook[k] = ema_w[k] / max(n', epsilon).  Every lane reads the old n before lane 0 stores the new one (one load instruction).
__global__ __launch_bounds__(256) void k_sem_vq_ema(const int* __restrict__ counts, const float* __restrict__ csum, int K, int S, float decay,
                                                    float alpha, float epsilon, float* __restrict__ ecs, float* __restrict__ ema_w,
                                                    float* __restrict__ codebook) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= K) return;
  const float n_new = fmaf(alpha, (float)counts[k], ecs[k] * decay);
  const float den = fmaxf(n_new, epsilon);
  for (int s = lane; s < S; s += 64) {
    const size_t e = (size_t)k * S + s;
    const float wv = fmaf(alpha, csum[e], ema_w[e] * decay);
    ema_w[e] = wv;
    codebook[e] = wv / den;
  }
  if (lane == 0) ecs[k] = n_new;
}

// out[e] = coef[1] csum[e]
__global__ void k_sem_vq_dcb(const float* __restrict__ csum, const float* __restrict__ coef, size_t n, float* __restrict__ out) {
  const float c = coef[1];
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) out[e] = c * csum[e];
}

// csum[K][S] = sum over the live rows m of [idx[m] = k] X[m][:]
static int vq_codesum(hipStream_t st, const SemLayout& L, const long long* idx, const float* X, const long long* len, int M, int T, float* csum,
                      float* part) {
  const int rows = edtts_bwd::dw_slab_rows(M), ns = (M + rows - 1) / rows;
  CodeSumArgs a{idx, X, len, ns == 1 ? csum : part, M, T, L.S, L.nt, L.K, L.nrt_codes, rows};
  hipLaunchKernelGGL(k_sem_codesum, dim3(L.nrt_codes, ns), dim3(256), 0, st, a);
  LAUNCH_CHECK("k_sem_codesum");
  if (ns > 1) TRY_G(TrainLauncher::slabsum(st, part, csum, (size_t)L.K * L.S, ns, (size_t)L.K * L.S));
  return EDTTS_OK;
}

}  // namespace edtts_sem

// =========================================================================================================
// launchers and the C ABI
// =========================================================================================================
// dims -> layout of a trainable head of the quantizer the entry point serves (vq: an edtts_sem_vq_* call)
static int sem_train_open(const EdttsSemDims* dims, const char* who, bool vq, edtts_sem::SemLayout& L) {
  TRY_G(edtts_sem::sem_layout(dims, L));
  if (L.vq && !vq)
    return fail(EDTTS_ERR_UNSUPPORTED, "%s: training covers the FSQ quantizer only (a VQ head trains through edtts_sem_vq_*)", who);
  if (!L.vq && vq)
    return fail(EDTTS_ERR_UNSUPPORTED, "%s: the VQ quantizer only (an FSQ head trains through edtts_sem_encode_train / edtts_sem_backward)", who);
  return EDTTS_OK;
}
// the head's one dropout site: stream word 0x40000 (include/edtts.h, "Philox stream ids")
static int sem_drop(const edtts_sem::SemLayout& L, const EdttsDropout* drop, const char* who, DropArgs* dr, bool* on,
                    const uint64_t* key = nullptr) {
  DropState ds{};
  TRY_G(drop_state(drop, who, &ds, on, key));
  if (*on && !L.in_dim) return fail(EDTTS_ERR_ARG, "%s: dropout p=%g given, but a head without proj (in_dim 0) has no dropout site", who, (double)drop->p);
  *dr = DropArgs{ds.k0, ds.k1, 0x40000u, ds.thr, ds.scale, ds.key};
  return EDTTS_OK;
}
static int sem_shape(int B, int T) {
  if (B < 0 || T < 0 || (long long)B * T > 0x7fffffffLL - edtts_sem::kFrames) return fail(EDTTS_ERR_ARG, "B=%d T=%d out of range", B, T);
  return EDTTS_OK;
}
// state-dict slots: proj's six (only with a proj), then the quantizer's own
static int sem_n_slots(const edtts_sem::SemLayout& L) { return (L.in_dim ? 6 : 0) + (L.vq ? 1 : 4); }

// What a training forward or backward starts with, in this order: the dims, a VQ call's commit, the dropout, the shape.
struct SemCall {
  edtts_sem::SemLayout L;
  DropArgs dr{};
  bool dropping;
};
static int sem_call_open(const EdttsSemDims* dims, const char* who, bool vq, double commit, const EdttsDropout* drop, const uint64_t* key, int B,
                         int T, SemCall& c) {
  TRY_G(sem_train_open(dims, who, vq, c.L));
  if (vq && (!(commit >= 0.0) || !(commit <= 1e6))) return fail(EDTTS_ERR_ARG, "%s: commit=%g outside [0, 1e6]", who, commit);
  TRY_G(sem_drop(c.L, drop, who, &c.dr, &c.dropping, key));
  return sem_shape(B, T);
}
// ... and a backward: then its slot count and d_z
static int sem_bwd_open(const EdttsSemDims* dims, const char* who, bool vq, double commit, const EdttsDropout* drop, const uint64_t* key, int B,
                        int T, int n_slots, const float* d_z, SemCall& c) {
  TRY_G(sem_call_open(dims, who, vq, commit, drop, key, B, T, c));
  if (n_slots != sem_n_slots(c.L)) return fail(EDTTS_ERR_ARG, "expected %d gradient slots, got %d", sem_n_slots(c.L), n_slots);
  if (c.L.in_dim && d_z) return fail(EDTTS_ERR_ARG, "%s: d_z is the input gradient of a head without proj (in_dim 0)", who);
  return EDTTS_OK;
}

// The six byte-count queries: the training blob, or the tape / the scratch of B x T frames.
enum SemSized { SEM_BLOB, SEM_TAPE, SEM_SCRATCH };
static int sem_train_bytes(const EdttsSemDims* dims, const char* who, bool vq, SemSized what, int B, int T, size_t* out_bytes) {
  using namespace edtts_sem;
  SemLayout L;
  TRY_G(sem_train_open(dims, who, vq, L));
  if (!out_bytes) return fail(EDTTS_ERR_ARG, "out_bytes is NULL");
  if (what != SEM_BLOB) TRY_G(sem_shape(B, T));
  const size_t n = what == SEM_BLOB ? sem_train_layout(L).total : what == SEM_TAPE ? sem_tape(L, (size_t)B * T).total : sem_scratch(L, B, T).total;
  *out_bytes = n * sizeof(float);
  return EDTTS_OK;
}

// The training blob of either head from its (checked) slots: every slot non-NULL, then one k_sem_pack_fragT per matrix.
static int sem_pack_train(const edtts_sem::SemLayout& L, const void* const* slots, int n_slots, void* packed_train, void* stream) {
  using namespace edtts_sem;
  for (int i = 0; i < n_slots; ++i)
    if (!slots[i]) return fail(EDTTS_ERR_ARG, "weight slot %d is NULL", i);
  const SemTrainLayout R = sem_train_layout(L);
  hipStream_t st = (hipStream_t)stream;
  float* P = (float*)packed_train;
  const float* const* s = (const float* const*)slots;
  const int q = L.in_dim ? 6 : 0;
  auto fragT = [&](const float* M, int Rr, int K, int nrt, int nkb, size_t off) -> int {
    const long long n = (long long)nrt * nkb * 256;
    hipLaunchKernelGGL(k_sem_pack_fragT, dim3((unsigned)min((n + 255) / 256, 4096LL)), dim3(256), 0, st, M, Rr, K, nrt, nkb, P + off);
    LAUNCH_CHECK("k_sem_pack_fragT");
    return EDTTS_OK;
  };
  if (!L.vq) {
    TRY_G(fragT(s[q + 2], L.D, L.S, 1, L.nt, R.wuT));  // proj_up.weight [S][D]   -> Wu^T [D][S]
    TRY_G(fragT(s[q], L.S, L.D, L.nt, 1, R.wdT));      // proj_down.weight [D][S] -> Wd^T [S][D]
  }
  if (L.in_dim) TRY_G(fragT(s[4], L.S, L.S, L.nt, L.nt, R.w3T));  // final Linear weight [S][S] -> W3^T
  return EDTTS_OK;
}

// The training forward of either head behind its checks: enc_begin, the tape's pointers, k_sem_encode<true>.  *blocks == 0: no
// frames, nothing launched.  tt: the tape's layout, for what the caller launches behind it.
static int sem_encode_train_run(const SemCall& c, const void* packed, const float* h, int B, int T, const int64_t* lengths, int64_t* idx,
                                float* z_q, int32_t* counts, void* tape, hipStream_t st, edtts_sem::SemTape& tt, unsigned* blocks) {
  using namespace edtts_sem;
  const SemLayout& L = c.L;
  tt = sem_tape(L, (size_t)B * T);
  float* tp = (float*)tape;  // (null only when a VQ call has no frames: every offset is then 0, and nothing is launched)
  EncTrainArgs a{};
  TRY_G(enc_begin(L, packed, h, B, T, lengths, idx, L.in_dim ? tp + tt.z : nullptr, z_q, counts, st, a, blocks));
  if (*blocks == 0) return EDTTS_OK;
  a.t_y1 = tp + tt.y1;
  if (L.vq) {
    a.t_r = tp + tt.r;
    a.t_sq = tp + tt.sq;
  } else {
    a.t_zb = tp + tt.zb;
  }
  a.dr = c.dr;
  a.dropping = c.dropping;
  hipLaunchKernelGGL(k_sem_encode<true>, dim3(*blocks), dim3(256), 0, st, a);
  LAUNCH_CHECK(L.vq ? "k_sem_encode<train, vq>" : "k_sem_encode<train>");
  return EDTTS_OK;
}

// k_sem_bwd_frames' arguments from the layouts and the call's pointers; what the other instantiation reads stays null / 0.
static edtts_sem::SemBwdArgs sem_bwd_args(const SemCall& c, const edtts_sem::SemTape& tt, const edtts_sem::SemScratch& ss, const void* packed,
                                          const void* packed_train, const void* tape, void* scratch, const int64_t* lengths, const float* d_zq,
                                          float* d_z, int M, int T) {
  using namespace edtts_sem;
  const SemLayout& L = c.L;
  const SemTrainLayout R = sem_train_layout(L);
  const float* tp = (const float*)tape;
  float* sc = (float*)scratch;
  SemBwdArgs a{};
  a.p = (const float*)packed;
  a.pt = (const float*)packed_train;
  a.g = d_zq;
  a.len = (const long long*)lengths;
  a.t_y1 = tp + tt.y1;
  if (L.vq) {
    a.t_r = tp + tt.r;
    a.coef = sc + ss.coef;
  } else {
    a.t_zb = tp + tt.zb;
    a.du = sc + ss.du; a.zql = sc + ss.zql;
    a.gm = lengths ? sc + ss.gm : nullptr;
  }
  a.dz = L.in_dim ? sc + ss.dz : d_z;
  a.a = sc + ss.a; a.dam = sc + ss.dam; a.xh = sc + ss.xh; a.dy1 = sc + ss.dy1; a.stat = sc + ss.stat;
  a.N = M; a.T = T; a.in_dim = L.in_dim; a.S = L.S; a.nt = L.nt; a.D = L.D;
  a.lng = L.lng; a.lnb = L.lnb; a.half = L.half; a.lev = L.lev;
  a.wuT = R.wuT; a.wdT = R.wdT; a.w3T = R.w3T;
  a.dr = c.dr;
  a.dropping = c.dropping;
  return a;
}

// No frames: every sum over frames is empty.  gs holds proj's six slots (only with a proj), then the quantizer's own, of `quant` floats.
static int sem_zero_grads(hipStream_t st, const edtts_sem::SemLayout& L, float* const* gs, std::initializer_list<size_t> quant) {
  const size_t S = L.S;
  int i = 0;
  auto zero = [&](size_t n) -> int {
    if (gs[i]) HIP_TRY(hipMemsetAsync(gs[i], 0, n * sizeof(float), st));
    ++i;
    return EDTTS_OK;
  };
  if (L.in_dim)
    for (size_t n : {S * L.in_dim, S, S, S, S * S, S}) TRY_G(zero(n));
  for (size_t n : quant) TRY_G(zero(n));
  return EDTTS_OK;
}
// proj's gradient sums over the M = B T frames that k_sem_bwd_frames left in `a`, in state-dict slot order (gs[0 .. 5])
static int sem_proj_sums(hipStream_t st, const edtts_sem::SemLayout& L, const edtts_sem::SemBwdArgs& a, const float* h, int B, int T,
                         float* const* gs, float* part) {
  using TL = TrainLauncher;
  const int S = L.S, M = B * T;
  TRY_G(TL::dw(st, a.dy1, S, h, L.in_dim, M, S, L.in_dim, gs[0], part));  // proj.0.weight = dy1^T h
  TRY_G(TL::colsum(st, a.dy1, S, M, S, gs[1], part));
  if (gs[2] || gs[3]) {                                                  // LayerNorm gain = sum dam o x^, bias = sum dam
    const int cpb = (T + edtts_bwd::kNormChunk - 1) / edtts_bwd::kNormChunk;
    edtts_bwd::NormBwdArgs na{a.xh, a.dam, nullptr, a.p + L.lng, nullptr, a.stat, part, M, S, T, 0, 0, 1e-5f};
    hipLaunchKernelGGL(edtts_bwd::k_bwd_norm_cols<edtts_gen::NORM_LAYER>, dim3((S + 63) / 64, B * cpb), dim3(256), 0, st, na);
    LAUNCH_CHECK("k_bwd_norm_cols");
    if (gs[2]) TRY_G(TL::slabsum(st, part, gs[2], (size_t)S, B * cpb, (size_t)3 * S));
    if (gs[3]) TRY_G(TL::slabsum(st, part + S, gs[3], (size_t)S, B * cpb, (size_t)3 * S));
  }
  TRY_G(TL::dw(st, a.dz, S, a.a, S, M, S, S, gs[4], part));               // final Linear weight = dz^T a
  return TL::colsum(st, a.dz, S, M, S, gs[5], part);
}

// The bodies of the three FSQ entry points that draw masks: `key` is the seed in device memory (the *_dev twins) or nullptr.
static int sem_encode_train_impl(const EdttsSemDims* dims, const void* packed, const float* h, int B, int T, const int64_t* lengths, int64_t* idx,
                                 float* z_q, int32_t* counts, void* tape, const EdttsDropout* drop, const uint64_t* key, void* stream) {
  SemCall c;
  TRY_G(sem_call_open(dims, "edtts_sem_encode_train", false, 0.0, drop, key, B, T, c));
  if (!packed || !h || !idx || !tape) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  edtts_sem::SemTape tt;
  unsigned blocks;
  return sem_encode_train_run(c, packed, h, B, T, lengths, idx, z_q, counts, tape, (hipStream_t)stream, tt, &blocks);
}

static int sem_backward_impl(const EdttsSemDims* dims, const void* packed, const void* packed_train, const void* tape, const float* h, int B,
                             int T, const int64_t* lengths, const float* d_zq, void* const* grad_slots, int n_slots, float* d_z, void* scratch,
                             const EdttsDropout* drop, const uint64_t* key, void* stream) {
  using namespace edtts_sem;
  using TL = TrainLauncher;
  SemCall c;
  TRY_G(sem_bwd_open(dims, "edtts_sem_backward", false, 0.0, drop, key, B, T, n_slots, d_z, c));
  if (!packed || !packed_train || !tape || !h || !d_zq || !grad_slots || !scratch) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  const SemLayout& L = c.L;
  hipStream_t st = (hipStream_t)stream;
  float* const* gs = reinterpret_cast<float* const*>(grad_slots);
  const int S = L.S, D = L.D, M = B * T, q = L.in_dim ? 6 : 0;
  if (M == 0) return sem_zero_grads(st, L, gs, {(size_t)D * S, (size_t)D, (size_t)S * D, (size_t)S});
  const SemTape tt = sem_tape(L, (size_t)M);
  const SemScratch ss = sem_scratch(L, B, T);
  const SemBwdArgs a = sem_bwd_args(c, tt, ss, packed, packed_train, tape, scratch, lengths, d_zq, d_z, M, T);
  hipLaunchKernelGGL(k_sem_bwd_frames<false>, dim3((M + kFrames - 1) / kFrames), dim3(256), 0, st, a);
  LAUNCH_CHECK("k_sem_bwd_frames");
  // the sums over frames, in state-dict slot order
  float* part = (float*)scratch + ss.part;
  const float* G = lengths ? a.gm : d_zq;
  const float* z = L.in_dim ? (const float*)tape + tt.z : h;
  if (L.in_dim) TRY_G(sem_proj_sums(st, L, a, h, B, T, gs, part));
  TRY_G(TL::dw(st, a.du, 16, z, S, M, D, S, gs[q], part));                  // proj_down.weight = du^T z
  TRY_G(TL::colsum(st, a.du, 16, M, D, gs[q + 1], part));
  TRY_G(TL::dw(st, G, S, a.zql, 16, M, S, D, gs[q + 2], part));             // proj_up.weight = G^T zq_low
  TRY_G(TL::colsum(st, G, S, M, S, gs[q + 3], part));
  return EDTTS_OK;
}

static int sem_dropout_mask_impl(const EdttsSemDims* dims, int B, int T, const EdttsDropout* drop, const uint64_t* key, uint8_t* keep,
                                 void* stream) {
  edtts_sem::SemLayout L;
  TRY_G(sem_train_open(dims, "edtts_sem_dropout_mask", false, L));
  if (!drop) return fail(EDTTS_ERR_ARG, "edtts_sem_dropout_mask: drop is NULL");
  if (!L.in_dim) return fail(EDTTS_ERR_ARG, "edtts_sem_dropout_mask: a head without proj (in_dim 0) has no dropout site");
  DropArgs dr{};
  bool dropping;
  TRY_G(sem_drop(L, drop, "edtts_sem_dropout_mask", &dr, &dropping, key));
  if (!dropping) dr = DropArgs{(unsigned)drop->seed, (unsigned)(drop->seed >> 32), 0x40000u, 0u, 1.0f};  // p == 0: everything kept
  TRY_G(sem_shape(B, T));
  if (!keep) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  const size_t rows = (size_t)B * T;
  if (rows == 0) return EDTTS_OK;
  hipLaunchKernelGGL(edtts_bwd::k_drop_mask, dim3(GenericLauncher::grid_1d(rows * (L.S / 4))), dim3(256), 0, (hipStream_t)stream, keep, rows, L.S,
                     T, 0, dr);
  LAUNCH_CHECK("k_drop_mask");
  return EDTTS_OK;
}

extern "C" {

int edtts_sem_train_packed_bytes(const EdttsSemDims* dims, size_t* out_bytes) {
  return sem_train_bytes(dims, "edtts_sem_train_packed_bytes", false, SEM_BLOB, 0, 0, out_bytes);
}
int edtts_sem_train_tape_bytes(const EdttsSemDims* dims, int B, int T, size_t* out_bytes) {
  return sem_train_bytes(dims, "edtts_sem_train_tape_bytes", false, SEM_TAPE, B, T, out_bytes);
}
int edtts_sem_train_scratch_bytes(const EdttsSemDims* dims, int B, int T, size_t* out_bytes) {
  return sem_train_bytes(dims, "edtts_sem_train_scratch_bytes", false, SEM_SCRATCH, B, T, out_bytes);
}
int edtts_sem_vq_train_packed_bytes(const EdttsSemDims* dims, size_t* out_bytes) {
  return sem_train_bytes(dims, "edtts_sem_vq_train_packed_bytes", true, SEM_BLOB, 0, 0, out_bytes);
}
int edtts_sem_vq_tape_bytes(const EdttsSemDims* dims, int B, int T, size_t* out_bytes) {
  return sem_train_bytes(dims, "edtts_sem_vq_tape_bytes", true, SEM_TAPE, B, T, out_bytes);
}
int edtts_sem_vq_scratch_bytes(const EdttsSemDims* dims, int B, int T, size_t* out_bytes) {
  return sem_train_bytes(dims, "edtts_sem_vq_scratch_bytes", true, SEM_SCRATCH, B, T, out_bytes);
}

int edtts_sem_train_region(const EdttsSemDims* dims, int B, int T, int which, size_t* offset_bytes, size_t* bytes) {
  using namespace edtts_sem;
  SemLayout L;
  TRY_G(sem_layout(dims, L));
  if (!offset_bytes || !bytes) return fail(EDTTS_ERR_ARG, "offset_bytes/bytes is NULL");
  TRY_G(sem_shape(B, T));
  static const char* const names[EDTTS_SEM_REGION_COUNT] = {"TAPE_Y1",     "TAPE_Z",      "TAPE_ZB",    "TAPE_R",      "TAPE_SQ",     "SCRATCH_DU",
                                                            "SCRATCH_ZQL", "SCRATCH_DZ",  "SCRATCH_GM", "SCRATCH_A",   "SCRATCH_DAM", "SCRATCH_XH",
                                                            "SCRATCH_DY1", "SCRATCH_STAT", "SCRATCH_PART", "SCRATCH_COEF", "SCRATCH_CSUM"};
  if (which < 0 || which >= EDTTS_SEM_REGION_COUNT)
    return fail(EDTTS_ERR_ARG, "edtts_sem_train_region: which=%d: expected an EDTTS_SEM_TAPE_* / EDTTS_SEM_SCRATCH_* member in [0, %d)", which,
                EDTTS_SEM_REGION_COUNT);
  bool found = false;
  auto pick = [&](int w, const size_t& m, size_t n) {
    if (w == which) { *offset_bytes = m * sizeof(float); *bytes = n * sizeof(float); found = true; }
  };
  const SemTape tt = sem_tape(L, (size_t)B * T);
  sem_tape_regions(L, (size_t)B * T, tt, pick);
  const SemScratch ss = sem_scratch(L, B, T);
  sem_scratch_regions(L, B, T, ss, pick);
  if (!found)
    return fail(EDTTS_ERR_ARG, "edtts_sem_train_region: EDTTS_SEM_%s is not a member of this head's layout (%s %s a proj)", names[which],
                L.vq ? "EDTTS_SEM_VQ" : "EDTTS_SEM_FSQ", L.in_dim ? "with" : "without");
  return EDTTS_OK;
}

int edtts_sem_train_pack(const EdttsSemDims* dims, const void* const* slots, int n_slots, void* packed_train, void* stream) {
  edtts_sem::SemLayout L;
  TRY_G(sem_train_open(dims, "edtts_sem_train_pack", false, L));
  if (!slots || !packed_train) return fail(EDTTS_ERR_ARG, "slots/packed_train is NULL");
  if (n_slots != sem_n_slots(L)) return fail(EDTTS_ERR_ARG, "expected %d weight slots, got %d", sem_n_slots(L), n_slots);
  return sem_pack_train(L, slots, n_slots, packed_train, stream);
}

int edtts_sem_vq_train_pack(const EdttsSemDims* dims, const void* const* slots, int n_slots, void* packed_train, void* stream) {
  edtts_sem::SemLayout L;
  TRY_G(sem_train_open(dims, "edtts_sem_vq_train_pack", true, L));
  if (n_slots != sem_n_slots(L)) return fail(EDTTS_ERR_ARG, "expected %d weight slots, got %d", sem_n_slots(L), n_slots);
  if (!L.in_dim) return EDTTS_OK;  // nothing to pack
  if (!slots || !packed_train) return fail(EDTTS_ERR_ARG, "slots/packed_train is NULL");
  return sem_pack_train(L, slots, n_slots, packed_train, stream);
}

int edtts_sem_encode_train(const EdttsSemDims* dims, const void* packed, const float* h, int B, int T, const int64_t* lengths, int64_t* idx,
                           float* z_q, int32_t* counts, void* tape, const EdttsDropout* drop, void* stream) {
  return sem_encode_train_impl(dims, packed, h, B, T, lengths, idx, z_q, counts, tape, drop, nullptr, stream);
}

int edtts_sem_encode_train_dev(const EdttsSemDims* dims, const void* packed, const float* h, int B, int T, const int64_t* lengths, int64_t* idx,
                               float* z_q, int32_t* counts, void* tape, const EdttsDropoutDev* drop, void* stream) {
  EdttsDropout host;
  const uint64_t* key;
  TRY_G(drop_dev(drop, "edtts_sem_encode_train_dev", &host, &key));
  return sem_encode_train_impl(dims, packed, h, B, T, lengths, idx, z_q, counts, tape, drop ? &host : nullptr, key, stream);
}

int edtts_sem_backward(const EdttsSemDims* dims, const void* packed, const void* packed_train, const void* tape, const float* h, int B, int T,
                       const int64_t* lengths, const float* d_zq, void* const* grad_slots, int n_slots, float* d_z, void* scratch,
                       const EdttsDropout* drop, void* stream) {
  return sem_backward_impl(dims, packed, packed_train, tape, h, B, T, lengths, d_zq, grad_slots, n_slots, d_z, scratch, drop, nullptr, stream);
}

int edtts_sem_backward_dev(const EdttsSemDims* dims, const void* packed, const void* packed_train, const void* tape, const float* h, int B, int T,
                           const int64_t* lengths, const float* d_zq, void* const* grad_slots, int n_slots, float* d_z, void* scratch,
                           const EdttsDropoutDev* drop, void* stream) {
  EdttsDropout host;
  const uint64_t* key;
  TRY_G(drop_dev(drop, "edtts_sem_backward_dev", &host, &key));
  return sem_backward_impl(dims, packed, packed_train, tape, h, B, T, lengths, d_zq, grad_slots, n_slots, d_z, scratch, drop ? &host : nullptr,
                           key, stream);
}

int edtts_sem_dropout_mask(const EdttsSemDims* dims, int B, int T, const EdttsDropout* drop, uint8_t* keep, void* stream) {
  return sem_dropout_mask_impl(dims, B, T, drop, nullptr, keep, stream);
}

int edtts_sem_dropout_mask_dev(const EdttsSemDims* dims, int B, int T, const EdttsDropoutDev* drop, uint8_t* keep, void* stream) {
  EdttsDropout host;
  const uint64_t* key;
  TRY_G(drop_dev(drop, "edtts_sem_dropout_mask_dev", &host, &key));
  return sem_dropout_mask_impl(dims, B, T, drop ? &host : nullptr, key, keep, stream);
}

// ---- the VQ head
int edtts_sem_vq_encode_train(const EdttsSemDims* dims, const void* packed, const float* h, int B, int T, const int64_t* lengths, int64_t* idx,
                              float* z_q, int32_t* counts, float* loss, void* tape, int training, double commit, const EdttsDropout* drop,
                              void* stream) {
  using namespace edtts_sem;
  SemCall c;
  TRY_G(sem_call_open(dims, "edtts_sem_vq_encode_train", true, commit, drop, nullptr, B, T, c));
  const int N = B * T;
  if (!packed || !loss || (N > 0 && (!h || !idx || !z_q || !tape))) return fail(EDTTS_ERR_ARG, "NULL pointer argument");  // (no frames: nothing to point at)
  hipStream_t st = (hipStream_t)stream;
  SemTape tt;
  unsigned blocks;
  TRY_G(sem_encode_train_run(c, packed, h, B, T, lengths, idx, z_q, counts, tape, st, tt, &blocks));
  if (blocks == 0) {
    HIP_TRY(hipMemsetAsync(loss, 0, sizeof(float), st));
    return EDTTS_OK;
  }
  hipLaunchKernelGGL(k_sem_vq_loss, dim3(1), dim3(256), 0, st, (const float*)tape + tt.sq, N, (const long long*)lengths, B, T, c.L.S, (float)commit,
                     training, loss);
  LAUNCH_CHECK("k_sem_vq_loss");
  return EDTTS_OK;
}

int edtts_sem_vq_ema_update(const EdttsSemDims* dims, const int64_t* idx, const float* z, int B, int T, const int64_t* lengths,
                            const int32_t* counts, double decay, double epsilon, float* ema_cluster_size, float* ema_w, float* codebook,
                            void* scratch, void* stream) {
  using namespace edtts_sem;
  SemLayout L;
  TRY_G(sem_train_open(dims, "edtts_sem_vq_ema_update", true, L));
  if (!(decay > 0.0) || !(decay <= 1.0)) return fail(EDTTS_ERR_ARG, "edtts_sem_vq_ema_update: decay=%g outside (0, 1]", decay);
  if (!(epsilon >= 0.0)) return fail(EDTTS_ERR_ARG, "edtts_sem_vq_ema_update: epsilon=%g < 0", epsilon);
  TRY_G(sem_shape(B, T));
  if (!counts || !ema_cluster_size || !ema_w || !codebook || !scratch) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  const int M = B * T;
  if (M > 0 && (!idx || !z)) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const SemScratch ss = sem_scratch(L, B, T);
  float* sc = (float*)scratch;
  if (M == 0) HIP_TRY(hipMemsetAsync(sc + ss.csum, 0, (size_t)L.K * L.S * sizeof(float), st));
  else TRY_G(vq_codesum(st, L, (const long long*)idx, z, (const long long*)lengths, M, T, sc + ss.csum, sc + ss.part));
  hipLaunchKernelGGL(k_sem_vq_ema, dim3((L.K + 3) / 4), dim3(256), 0, st, counts, sc + ss.csum, L.K, L.S, (float)decay, (float)(1.0 - decay),
                     (float)epsilon, ema_cluster_size, ema_w, codebook);
  LAUNCH_CHECK("k_sem_vq_ema");
  return EDTTS_OK;
}

int edtts_sem_vq_backward(const EdttsSemDims* dims, const void* packed, const void* packed_train, const void* tape, const float* h,
                          const int64_t* idx, int B, int T, const int64_t* lengths, const float* d_zq, const float* d_loss, double commit,
                          void* const* grad_slots, int n_slots, float* d_z, void* scratch, const EdttsDropout* drop, void* stream) {
  using namespace edtts_sem;
  SemCall c;
  TRY_G(sem_bwd_open(dims, "edtts_sem_vq_backward", true, commit, drop, nullptr, B, T, n_slots, d_z, c));
  const SemLayout& L = c.L;
  const int S = L.S, M = B * T, q = L.in_dim ? 6 : 0;
  if (!grad_slots || (M > 0 && (!tape || !h || !idx || !scratch || (L.in_dim && (!packed || !packed_train)))))
    return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  hipStream_t st = (hipStream_t)stream;
  float* const* gs = reinterpret_cast<float* const*>(grad_slots);
  if (M == 0) return sem_zero_grads(st, L, gs, {(size_t)L.K * S});
  const SemTape tt = sem_tape(L, (size_t)M);
  const SemScratch ss = sem_scratch(L, B, T);
  float* sc = (float*)scratch;
  hipLaunchKernelGGL(k_sem_vq_coef, dim3(1), dim3(256), 0, st, d_loss, (const long long*)lengths, B, T, S, (float)commit, sc + ss.coef);
  LAUNCH_CHECK("k_sem_vq_coef");
  if (L.in_dim || d_z) {
    const SemBwdArgs a = sem_bwd_args(c, tt, ss, packed, packed_train, tape, scratch, lengths, d_zq, d_z, M, T);
    hipLaunchKernelGGL(k_sem_bwd_frames<true>, dim3((M + kFrames - 1) / kFrames), dim3(256), 0, st, a);
    LAUNCH_CHECK("k_sem_bwd_frames<vq>");
    if (L.in_dim) TRY_G(sem_proj_sums(st, L, a, h, B, T, gs, sc + ss.part));
  }
  if (gs[q]) {  // d codebook = coef[1] sum_{m: idx[m] = k} r_m: the decoder's gradient never reaches the codebook
    const size_t n = (size_t)L.K * S;
    if (!d_loss) {
      HIP_TRY(hipMemsetAsync(gs[q], 0, n * sizeof(float), st));
    } else {
      TRY_G(vq_codesum(st, L, (const long long*)idx, (const float*)tape + tt.r, (const long long*)lengths, M, T, sc + ss.csum, sc + ss.part));
      hipLaunchKernelGGL(k_sem_vq_dcb, dim3(GenericLauncher::grid_1d(n)), dim3(256), 0, st, sc + ss.csum, sc + ss.coef, n, gs[q]);
      LAUNCH_CHECK("k_sem_vq_dcb");
    }
  }
  return EDTTS_OK;
}

}  // extern "C"
