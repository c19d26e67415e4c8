// edtts_generic.h -- the generic fp32 decoder path: every shape a run-time value (included by edtts_kernels.hip).
//
// The fused kernels of edtts_kernels.hip are compiled per decoder shape (hidden, heads, n_mels).  The kernels here take the shape
// as arguments; they are templated on epilogue, tail and a padded head-dim tile count only, so the build grows by a fixed set of
// kernels however many shapes run on them.  Selected per decoder with EDTTS_KERNELS_GENERIC / EDTTS_KERNELS_AUTO (include/edtts.h).
//
//   k_gen_gemm<EPI>    Y[M,N] = X[M,K] W[N,K]^T on v_mfma_f32_16x16x4_f32, both operands through LDS tiles (zero-filled past K / N),
//                      masked stores; epilogues: + bias, + bias + positional row (in_proj / context), residual h += acc + bias,
//                      SwiGLU (a block computes value column j and gate column j together: value * silu(gate) is stored)
//   k_gen_norm<MODE>   one wave per row, run-time width: RMSNorm x gain (optionally AdaLN (1+scale) y + shift), LayerNorm
//   k_gen_attn<DT>     flash-style attention for 16 queries x one head per wave: S^T = K Q^T and O^T = V^T P^T on MFMA, fp32 online
//                      softmax (exp2 domain), head_dim padded to DT 16-wide tiles; self-attention visits only the band |j - i| <= window
//   k_gen_embed        context = token_emb[sem_idx] + context_pos_emb (clamped indices set EDTTS_IDX_SEM)
//                      (the training forward, edtts_generic_bwd.h, also has it store each query's log-sum-exp)
//   k_gen_tail<TAIL>   the sampler updates of the fused tails, elementwise: tail_apply (vector path) or the same helpers per element
//
// Activations are plain row-major [rows][features] fp32 in the workspace; weights are the state-dict's own [N][K] matrices.
namespace edtts_gen {

enum { EPI_BIAS = 0, EPI_PE = 1, EPI_RESID = 2, EPI_SWIGLU = 3 };

struct GemmArgs {
  const float* X;     // [M][ldx]
  const float* W;     // [N(x2 for SwiGLU)][K], K contiguous
  const float* bias;  // [N] (SwiGLU: [2N], value half then gate half) or null
  float* Y;           // [M][ldy]
  const float* pe;    // EPI_PE: positional table [*][N], row = m % T
  int M, N, K, ldx, ldy, T;
  int vec_x, vec_w, vec_y;  // 16-byte loads / stores allowed (K % 4 == 0 and aligned rows; N, ldy % 4 == 0)
  DropArgs dr;              // k_gen_gemm<EPI, true> only: the mask of its epilogue
};
constexpr int kGBM = 64, kGBN = 64, kGBK = 16, kGLd = kGBK + 1;

// (DROP: the training forward's dropout, EPI_SWIGLU / EPI_RESID only -- the epilogue multiplies its four columns by drop_row4)
template <int EPI, bool DROP = false>
__global__ __launch_bounds__(256) void k_gen_gemm(GemmArgs a) {
  __shared__ float xs[kGBM][kGLd];
  __shared__ float ws[kGBN][kGLd];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fq = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * kGBM;
  const int n0 = blockIdx.y * (EPI == EPI_SWIGLU ? kGBN / 2 : kGBN);
  // loader: LDS row lr, k offsets lk .. lk + 3 of the current k-tile
  const int lr = tid >> 2, lk = 4 * (tid & 3);
  int wrow;
  bool wok;
  if (EPI == EPI_SWIGLU) {  // LDS rows 0..31: value rows n0.., rows 32..63: the matching gate rows N + n0..
    const int j = n0 + (lr & 31);
    wrow = (lr < 32 ? 0 : a.N) + j;
    wok = j < a.N;
  } else {
    wrow = n0 + lr;
    wok = wrow < a.N;
  }
  const int xrow = m0 + lr;
  const bool xok = xrow < a.M;
  const float* xp = a.X + (size_t)(xok ? xrow : 0) * a.ldx;
  const float* wp = a.W + (size_t)(wok ? wrow : 0) * a.K;
  // this wave's two weight sub-tiles (LDS rows) and its 32 activation rows
  const int wn0 = EPI == EPI_SWIGLU ? 16 * (w & 1) : 32 * (w & 1);
  const int wn1 = EPI == EPI_SWIGLU ? wn0 + 32 : wn0 + 16;
  const int wm = 32 * (w >> 1);
  f4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = splat(0.f);
  for (int k0 = 0; k0 < a.K; k0 += kGBK) {
    const int k = k0 + lk;
    f4 xv = splat(0.f), wv = splat(0.f);
    if (a.vec_x) {
      if (xok && k < a.K) xv = ldg4(xp + k);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) xv[r] = (xok && k + r < a.K) ? xp[k + r] : 0.f;
    }
    if (a.vec_w) {
      if (wok && k < a.K) wv = ldg4(wp + k);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) wv[r] = (wok && k + r < a.K) ? wp[k + r] : 0.f;
    }
    __syncthreads();  // the previous k-tile has been consumed by every wave
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      xs[lr][lk + r] = xv[r];
      ws[lr][lk + r] = wv[r];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kGBK / 4; ++s) {
      const int kk = 4 * s + g;  // A[n = fq][k = g], B[k = g][m = fq]
      const float a0 = ws[wn0 + fq][kk], a1 = ws[wn1 + fq][kk];
      const float b0 = xs[wm + fq][kk], b1 = xs[wm + 16 + fq][kk];
      acc[0][0] = EDTTS_MFMA(a0, b0, acc[0][0]);
      acc[0][1] = EDTTS_MFMA(a0, b1, acc[0][1]);
      acc[1][0] = EDTTS_MFMA(a1, b0, acc[1][0]);
      acc[1][1] = EDTTS_MFMA(a1, b1, acc[1][1]);
    }
  }
  // epilogue: acc[t][u] lane (g, fq) holds Y[m = m0 + wm + 16u + fq][n = 4g + r of weight sub-tile t]
  const DropArgs dr = DROP ? drop_live(a.dr) : DropArgs{};
  if (EPI == EPI_SWIGLU) {
    const int n = n0 + wn0 + 4 * g;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int m = m0 + wm + 16 * u + fq;
      if (m >= a.M) continue;
      f4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = n + r < a.N;
        const float v = acc[0][u][r] + (a.bias && ok ? a.bias[n + r] : 0.f);
        const float gt = acc[1][u][r] + (a.bias && ok ? a.bias[a.N + n + r] : 0.f);
        o[r] = v * silu(gt);
      }
      if (DROP) {
        const f4 dm = drop_row4(dr, m, n);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] *= dm[r];
      }
      float* yp = a.Y + (size_t)m * a.ldy + n;
      if (a.vec_y && n + 3 < a.N) {
        stg4(yp, o);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < a.N) yp[r] = o[r];
      }
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int n = n0 + (t ? wn1 : wn0) + 4 * g;
    if (n >= a.N) continue;
    f4 bv = splat(0.f);
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = (a.bias && n + r < a.N) ? a.bias[n + r] : 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int m = m0 + wm + 16 * u + fq;
      if (m >= a.M) continue;
      f4 o = acc[t][u] + bv;
      float* yp = a.Y + (size_t)m * a.ldy + n;
      const bool full = a.vec_y && n + 3 < a.N;
      if (EPI == EPI_PE) {
        const float* pp = a.pe + (size_t)(m % a.T) * a.N + n;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < a.N) o[r] += pp[r];
      }
      if (DROP) {  // h = h + dropout(x W^T + b)
        const f4 dm = drop_row4(dr, m, n);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] *= dm[r];
      }
      if (EPI == EPI_RESID) {  // h = h + (x W^T + b): the reference's residual order
        if (full) {
          stg4(yp, ldg4(yp) + o);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n + r < a.N) yp[r] = yp[r] + o[r];
        }
      } else if (full) {
        stg4(yp, o);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < a.N) yp[r] = o[r];
      }
    }
  }
}
// the same product with both operands rounded to bf16 on their way into LDS (edtts_generic16.h); TX / TY = __bf16: X holds / Y gets
// bf16 elements (Layout::TAPE16) -- GemmArgs' pointers then name buffers of __bf16, ldx / ldy still count elements
template <int EPI, bool DROP = false, typename TX = float, typename TY = float>
__global__ __launch_bounds__(256) void k_gen_gemm16(GemmArgs a);


// ---- row norms -------------------------------------------------------------------------------------------------------------
enum { NORM_RMS = 0, NORM_LAYER = 1 };
struct NormArgs {
  const float* x;
  float* y;
  const float *w, *b;  // gain; LayerNorm bias
  const float* mod;    // AdaLN: [2W] per batch row = (1 + scale | shift), or null
  int rows, W, ld, rows_per_b, mod_bstride;
  float eps;
};
EDTTS_DEV float wave_allsum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <int MODE>
__global__ __launch_bounds__(256) void k_gen_norm(NormArgs a) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;  // (no block-level synchronisation in this kernel)
  const float* x = a.x + (size_t)row * a.ld;
  float* y = a.y + (size_t)row * a.ld;
  if (MODE == NORM_LAYER) {
    float s = 0.f;
    for (int j = lane; j < a.W; j += 64) s += x[j];
    const float mu = wave_allsum(s) / (float)a.W;
    float q = 0.f;
    for (int j = lane; j < a.W; j += 64) {
      const float d = x[j] - mu;
      q += d * d;
    }
    const float rs = rsqrtf(wave_allsum(q) / (float)a.W + a.eps);
    for (int j = lane; j < a.W; j += 64) y[j] = (x[j] - mu) * rs * a.w[j] + a.b[j];
  } else {
    float q = 0.f;
    for (int j = lane; j < a.W; j += 64) q += x[j] * x[j];
    const float rs = rsqrtf(wave_allsum(q) / (float)a.W + a.eps);
    const float* md = a.mod ? a.mod + (size_t)(row / a.rows_per_b) * a.mod_bstride : nullptr;
    for (int j = lane; j < a.W; j += 64) {
      float v = x[j] * rs * a.w[j];
      if (md) v = v * md[j] + md[a.W + j];
      y[j] = v;
    }
  }
}

// ---- attention -------------------------------------------------------------------------------------------------------------
struct AttnArgs {
  const float* q;   // row b * Tq + i, feature head * DH + d
  const float *k, *v;  // row b * Tk + j
  float* o;         // like q
  int ldq, ldkv, ldo, Tq, Tk, DH, window;  // window < 0: every key
  float scale;      // log2(e) / sqrt(head_dim): scores in the exp2 domain
  const int64_t *q_len, *k_len;  // per-utterance query / key counts [B] (edtts_*_len), or null: Tq / Tk for all
  int q_dbl, k_dbl;              // ... given as token counts of which they are twice (see utt_len)
  float* lse;                    // training forward: log-sum-exp (exp2 domain) per [utterance][head][query], or null
  DropArgs dr;                   // k_gen_attn<DT, true> only: the mask of the probabilities
};
// One wave = 16 queries of one (utterance, head).  S^T tile (16 keys x 16 queries) = K Q^T: lane (g, i) holds the scores of query i
// against keys 4g + r.  P^T then is the B operand of O^T += V^T P^T as it stands when MFMA step s contracts keys {4g + s}: the V^T
// operand of lane (g, d) reads V[key 4g + s][d].  Query statistics live on lane & 15; the four lane groups combine with two xor shuffles.
// DROP (the training forward's dropout): l and the log-sum-exp come from the undropped probabilities; the B operand of
// O^T += V^T P^T is p * keep * scale.
template <int DT, bool DROP = false>
__global__ __launch_bounds__(64) void k_gen_attn(AttnArgs a) {
  const int lane = threadIdx.x, fq = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, hd = blockIdx.y, b = blockIdx.z;
  // Per-utterance lengths: keys past the utterance's count are never read (as in its solo call, whose Tk it is); a block of queries
  // wholly past its count has no solo counterpart and stores nothing -- those rows are read by no other row (every other step is
  // row-local), and the output's rows past the count are zeroed at the end of the forward.
  const int Tk = utt_len(a.k_len, b, a.Tk, a.k_dbl);
  if (q0 >= utt_len(a.q_len, b, a.Tq, a.q_dbl)) return;
  const int qi = q0 + fq;
  const bool qok = qi < a.Tq;
  const float* qrow = a.q + (size_t)(b * a.Tq + (qok ? qi : 0)) * a.ldq + hd * a.DH;
  float qv[4 * DT];
#pragma unroll
  for (int s = 0; s < 4 * DT; ++s) {
    const int d = 4 * s + g;
    qv[s] = (qok && d < a.DH) ? qrow[d] * a.scale : 0.f;
  }
  f4 acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) acc[t] = splat(0.f);
  float m = -1e30f, l = 0.f;
  int lo = 0, hi = Tk;
  if (a.window >= 0) {
    lo = q0 - a.window > 0 ? q0 - a.window : 0;
    const int e = q0 + 16 + a.window;
    hi = e < Tk ? e : Tk;
  }
  const float* kb = a.k + (size_t)b * a.Tk * a.ldkv + hd * a.DH;
  const float* vb = a.v + (size_t)b * a.Tk * a.ldkv + hd * a.DH;
  const DropArgs dr = DROP ? drop_live(a.dr) : DropArgs{};
  for (int j0 = lo; j0 < hi; j0 += 16) {
    const int kj = j0 + fq;
    const bool kok = kj < hi;
    const float* krow = kb + (size_t)(kok ? kj : 0) * a.ldkv;
    f4 sc = splat(0.f);
#pragma unroll
    for (int s = 0; s < 4 * DT; ++s) {
      const int d = 4 * s + g;
      const float ka = (kok && d < a.DH) ? krow[d] : 0.f;
      sc = EDTTS_MFMA(ka, qv[s], sc);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = j0 + 4 * g + r;
      const bool ok = key < hi && (a.window < 0 || (key - qi <= a.window && qi - key <= a.window));
      sc[r] = ok ? sc[r] : -INFINITY;
      mx = fmaxf(mx, sc[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);
    const float alpha = exp2f(m - mn);
    f4 p;
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[r] = exp2f(sc[r] - mn);
      ps += p[r];
    }
    ps += __shfl_xor(ps, 16);
    ps += __shfl_xor(ps, 32);
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int t = 0; t < DT; ++t) acc[t] *= alpha;
    if (DROP) {  // (key tiles start at lo + 16 n: aligned for every tile or for none)
      const f4 dm = drop_attn_keys4(dr, (unsigned)(b * gridDim.y + hd), qi, j0 + 4 * g, (lo & 3) == 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] *= dm[r];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int key = j0 + 4 * g + s;
      const float* vrow = vb + (size_t)(key < hi ? key : 0) * a.ldkv;
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        const int d = 16 * t + fq;
        const float va = (key < hi && d < a.DH) ? vrow[d] : 0.f;
        acc[t] = EDTTS_MFMA(va, p[s], acc[t]);
      }
    }
  }
  if (!qok) return;
  if (a.lse != nullptr && g == 0) a.lse[((size_t)b * gridDim.y + hd) * a.Tq + qi] = m + log2f(l);
  const float inv = 1.0f / l;
  float* orow = a.o + (size_t)(b * a.Tq + qi) * a.ldo + hd * a.DH;
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int d = 16 * t + 4 * g + r;  // acc[t] lane (g, i) holds O^T[d][i]
      if (d < a.DH) orow[d] = acc[t][r] * inv;
    }
}
// the same attention with both contractions on bf16 MFMAs, four query tiles per block (edtts_generic_attn16.h)
// (TQ = __bf16: q, k and v hold bf16 elements, Layout::TAPE16; AttnArgs' pointers name the buffers, ldq / ldkv count elements)
template <int DT, bool DROP = false, typename TQ = float>
__global__ __launch_bounds__(256) void k_gen_attn16(AttnArgs a);

// ---- context embedding (token ids) ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gen_embed(const int64_t* sem_idx, const float* tok, const float* cpe, float* ctx, int rows, int S,
                                                   int H, int n_tok, unsigned* err, const int64_t* s_len) {
  const size_t n = (size_t)rows * H;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / H;
    const int c = (int)(i - row * H);
    // (a token past the utterance's length is padding: never read, no index check; its row is never a key)
    long tk = (s_len && (int)(row % S) >= utt_len_lane(s_len, (int)(row / S), S)) ? 0 : (long)sem_idx[row];
    if (tk < 0 || tk >= n_tok) {  // nn.Embedding would raise IndexError: clamp (never fault) and leave a mark for the host
      if (c == 0) atomicOr(err, (unsigned)EDTTS_IDX_SEM);
      tk = tk < 0 ? 0 : n_tok - 1;
    }
    ctx[i] = tok[(size_t)tk * H + c] + cpe[(size_t)(row % S) * H + c];
  }
}

// ---- sampler tails ---------------------------------------------------------------------------------------------------------------
// The fused kernels' tail_apply (edtts_kernels.hip) on a stored eps: bitwise the same update.  vec: n % 4 == 0 and 16-byte aligned
// tensors; otherwise one element per thread through the same per-element helpers (Philox: element e is lane e & 3 of draw e >> 2).
template <int TAIL>
EDTTS_DEV void tail_elem(const KArgs& a, size_t idx, float e) {
  if (TAIL == TAIL_LMS) {
    const float hn = a.lms.mode >= 2 ? a.h_new[idx] : 0.f, ho = a.lms.mode >= 3 ? a.h_old[idx] : 0.f;
    float v0, vn;
    lms_elem(a.x[idx], e, hn, ho, a.lms, v0, vn);
    a.x0_hist[idx] = v0;
    if (a.x0_all) a.x0_all[idx] = v0;
    a.x_prev[idx] = vn;
  } else if (TAIL == TAIL_VLMS) {
    const float v = a.v_uncond ? cfg_combine(e, a.v_uncond[idx], a.vp.cfg) : e;
    const float hn = a.lms.mode >= 2 ? a.h_new[idx] : 0.f, ho = a.lms.mode >= 3 ? a.h_old[idx] : 0.f;
    float v0, vn;
    lms_elem(a.x[idx], v, hn, ho, a.lms, v0, vn);
    a.x0_hist[idx] = v0;
    if (a.x0_all) a.x0_all[idx] = v0;
    if (a.known != nullptr) {  // the next step's q_sample of the known frames (vlms_blend, one element: k_inpaint_inject1's values)
      const size_t row = (size_t)a.T * a.inj_mel, b = idx / row, r = idx - b * row, per = (size_t)a.inj_frames * a.inj_mel;
      if (r < per) {  // (the caller has checked the frame against the utterance's length)
        const size_t ki = b * per + r;
        vn = a.known[ki];
        if (a.p_coef2 != 0.f) {
          const float nz = a.noise ? a.noise[ki]
                                   : (a.seeds ? philox_normal4(a.seeds[b], a.step, r >> 2)[(int)(r & 3)] : philox_normal4(a.seed, a.step, ki >> 2)[(int)(ki & 3)]);
          vn = qsample_elem(vn, a.p_coef1, nz, a.p_coef2);
        }
      }
    }
    a.x_prev[idx] = vn;
  } else if (TAIL == TAIL_VPRED) {
    const float v = a.v_uncond ? cfg_combine(e, a.v_uncond[idx], a.vp.cfg) : e;
    a.x_prev[idx] = vpred_elem(a.x[idx], v, a.vp);
  } else if (TAIL == TAIL_DDPM) {
    const unsigned long long ge = a.philox_base + idx;
    const float nz = a.noise ? a.noise[idx] : philox_normal4(a.seed, a.step, ge >> 2)[(int)(ge & 3)];
    const DdpmCoef cf{a.p_coef1, a.p_coef2, a.p_sd};
    a.x_prev[idx] = ddpm_elem(a.x[idx], e, nz, cf);
  } else {
    float v0, vp;
    ddim_elem(a.x[idx], e, a.c_s1m, a.c_sab, a.c_sabp, a.c_dir, v0, vp);
    a.x0[idx] = v0;
    a.x_prev[idx] = vp;
  }
}
template <int TAIL>
EDTTS_DEV void tail_zero_elem(const KArgs& a, size_t idx) {
  if (TAIL == TAIL_LMS || TAIL == TAIL_VLMS) {
    a.x0_hist[idx] = 0.f;
    if (a.x0_all) a.x0_all[idx] = 0.f;
  } else if (TAIL == TAIL_DDIM) {
    a.x0[idx] = 0.f;
  }
  a.x_prev[idx] = 0.f;
}
// element idx of [B][T][MEL] lies past its utterance's frame count (per-utterance lengths; no lengths: never)
EDTTS_DEV bool past_len(const int64_t* t_len, bool dbl, size_t idx, int T, int MEL) {
  if (t_len == nullptr) return false;
  const size_t row = idx / MEL;
  return (int)(row % T) >= utt_len_lane(t_len, (int)(row / T), T, dbl);
}
// (with lengths, vec also needs MEL % 4 == 0: a float4 then never straddles two frames)
template <int TAIL>
__global__ __launch_bounds__(256) void k_gen_tail(KArgs a, const float* eps, size_t n, int vec, int MEL) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  if (vec) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += stride) {
      if constexpr (TAIL == TAIL_VLMS) {  // (its blend needs the frame: vec then also means MEL % 4 == 0)
        const size_t row = 4 * i / MEL;
        const int f = (int)(row % a.T);
        // (utt_len_lane called from here changed k_gen_embed's code, as from k_inpaint_inject)
        const int Tb = a.t_len ? utt_len_of(a.t_len[row / a.T], a.T, a.t_dbl) : a.T;
        tail_store<TAIL>(a, f, Tb, 4 * i, ldg4(eps + 4 * i));
        continue;
      }
      if (past_len(a.t_len, a.t_dbl, 4 * i, a.T, MEL)) tail_zero<TAIL>(a, 4 * i);
      else tail_apply<TAIL>(a, 4 * i, ldg4(eps + 4 * i));
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      if (past_len(a.t_len, a.t_dbl, i, a.T, MEL)) tail_zero_elem<TAIL>(a, i);
      else tail_elem<TAIL>(a, i, eps[i]);
    }
  }
}
// eps rows past each utterance's frame count -> 0 (the forward's own output, TAIL_EPS)
__global__ __launch_bounds__(256) void k_gen_zero_past(float* y, const int64_t* t_len, int dbl, size_t n, int T, int MEL) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    if (past_len(t_len, dbl, i, T, MEL)) y[i] = 0.f;
}

}  // namespace edtts_gen

// A validated EdttsDropout (include/edtts.h, "Dropout masks"): the key words, the threshold and the scale of the kept values.
enum { DROP_ATTN = 0, DROP_CROSS = 1, DROP_ACT = 2, DROP_DOWN = 3 };
struct DropState {
  unsigned k0, k1, thr;
  float scale;
  const unsigned* key = nullptr;  // EdttsDropoutDev: the key in device memory instead of (k0, k1)
  DropArgs site(int layer, int site_id) const { return DropArgs{k0, k1, 0x30000u + 4u * (unsigned)layer + (unsigned)site_id, thr, scale, key}; }
};

// Where one forward's intermediates go.  Inference reuses a few workspace buffers for all of them; the training forward
// (edtts_generic_bwd.h) points them into its tape and also asks for the snapshots and the log-sum-exps.
// An activation buffer together with its element type: fp32, or -- the four buffers that Layout::TAPE16 narrows (EDTTS_TAPE_BF16,
// DESIGN.md section 28) -- bf16.  `+` and every ld / pitch that goes with it count ELEMENTS, so the launch lists read the same for
// both; gemm / attn / attn_bwd / dw pick the instantiation from `h`.  A plain float pointer converts to an fp32 one.
struct Act {
  const float* p;  // the buffer (h: its bytes hold __bf16)
  bool h;
  Act(const float* q = nullptr, bool half = false) : p(q), h(half) {}
  Act operator+(size_t n) const { return h ? Act(reinterpret_cast<const float*>(reinterpret_cast<const __bf16*>(p) + n), true) : Act(p + n); }
  float* w() const { return const_cast<float*>(p); }  // (as an output: every Act a launch list writes was made from a float*)
};
struct FwdLayerBufs {
  float *crp, *crn;          // kv_down rows [B S][R] before / after kv_norm
  Act kv;                    // K|V rows [B S][2H]
  Act qkv;                   // self-attention: q|k|v rows
  float *att1, *lse1;        // ... attention output, log-sum-exp [B][HEADS][T] or null
  Act qc;                    // cross-attention: query rows
  float *att2, *lse2;        // ... attention output, log-sum-exp or null
  Act act;                   // value * silu(gate) [B T][FM H]
  float *h0, *h1, *h2;       // or null: copies of the residual stream entering norm1 / norm2 / norm3
};
struct FwdBufs {
  float* ctx;  // context rows [B S][H]
  FwdLayerBufs layer[kMaxLayers];
  float* hL;   // or null: a copy of the residual stream entering final_norm
  FwdBufs() = default;
  // the workspace's buffers: kv_norm in place, one buffer for q|k|v, the cross queries and the SwiGLU output, one for both
  // attention outputs; no snapshot, no log-sum-exp  (TAPE16: the same offsets, of which the bf16 rows fill the first half)
  explicit FwdBufs(const CallCtx& c) : ctx(c.wsb + c.ws.g_ctx), hL(nullptr) {
    const bool t16 = c.lo.TAPE16 != 0;
    float *cr = c.wsb + c.ws.g_cr, *big = c.wsb + c.ws.g_big, *att = c.wsb + c.ws.g_att;
    for (int l = 0; l < c.lo.L; ++l) {
      FwdLayerBufs& z = layer[l];
      z.crp = z.crn = cr;
      z.kv = Act(c.wsb + c.ws.g_kv + (size_t)l * c.B * c.S * 2 * c.lo.H, t16);
      z.qkv = z.qc = z.act = Act(big, t16);
      z.att1 = z.att2 = att;
      z.lse1 = z.lse2 = z.h0 = z.h1 = z.h2 = nullptr;
    }
  }
};

// =========================================================================================================
// GenericLauncher: the static interface of Launcher / Launcher16 on the run-time-shape kernels
// =========================================================================================================
// The stream of a `linear` site together with the arithmetic of its product: fp32 MFMAs (k_gen_gemm, k_bwd_gemm) or, for a layout
// with EDTTS_MATMUL_BF16, the bf16 ones of edtts_generic16.h.  The decoder's launch lists build one from their layout and hand it to
// every gemm / dx / dw; a plain hipStream_t (the semantic head's calls) means fp32.
struct MmStream {
  hipStream_t st;
  bool bf16;
  MmStream(hipStream_t s, bool b = false) : st(s), bf16(b) {}
  operator hipStream_t() const { return st; }
};
// The shape of an attention call: row width (all heads), heads, head_dim, and whether the bf16 attention (EDTTS_ATTN_BF16) runs it.
// The decoder's is its layout's; HuBERT's fp32 forward brings its own.
struct AttnShape {
  int H, HEADS, DH;
  bool att16;
  AttnShape(int h, int heads, int dh, bool a16 = false) : H(h), HEADS(heads), DH(dh), att16(a16) {}
  AttnShape(const Layout& lo) : H(lo.H), HEADS(lo.HEADS), DH(lo.DH), att16(lo.ATT16 != 0) {}
};

struct GenericLauncher {
  static int set_attrs() { return EDTTS_OK; }  // (no kernel here needs more than 64 KiB of LDS)

  static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
  static unsigned grid_1d(size_t n) { const size_t nb = (n + 255) / 256; return (unsigned)(nb > 4096 ? 4096 : (nb < 1 ? 1 : nb)); }
  // The instances of a `linear` site's product that exist, over (bf16 products, dropout, bf16 loads, bf16 stores) -- gemm instantiates
  // no other and refuses what falls outside: the dropout epilogue belongs to EPI_SWIGLU and EPI_RESID; bf16 rows (Layout::TAPE16) are
  // k_gen_gemm16's alone, stored by EPI_BIAS and EPI_SWIGLU and loaded by EPI_RESID -- exactly the sites that the narrowed buffers have
  static constexpr bool drop_epi(int epi) { return epi == edtts_gen::EPI_SWIGLU || epi == edtts_gen::EPI_RESID; }
  template <int EPI, bool MM16, bool DROP, class TX, class TY>
  static constexpr bool gemm_instance() {
    constexpr bool xh = std::is_same<TX, __bf16>::value, yh = std::is_same<TY, __bf16>::value;
    return (!DROP || drop_epi(EPI)) && (!xh || (MM16 && EPI == edtts_gen::EPI_RESID)) &&
           (!yh || (MM16 && (EPI == edtts_gen::EPI_BIAS || EPI == edtts_gen::EPI_SWIGLU)));
  }
  template <int EPI, bool MM16, bool DROP, class TX, class TY>
  static constexpr auto gemm_kernel() {
    if constexpr (MM16) return &edtts_gen::k_gen_gemm16<EPI, DROP, TX, TY>;
    else return &edtts_gen::k_gen_gemm<EPI, DROP>;
  }
  // dr non-null (EPI_SWIGLU / EPI_RESID): the dropout instantiation, its epilogue masked with *dr
  // X.h / Y.h (Layout::TAPE16): the bf16-load / bf16-store instantiation; one that gemm_instance lacks is an error, never a conversion
  template <int EPI>
  static int gemm(MmStream st, Act X, int ldx, const float* W, const float* bias, Act Y, int ldy, int M, int N, int K,
                  const float* pe = nullptr, int T = 1, const edtts::DropArgs* dr = nullptr) {
    using namespace edtts_gen;
    GemmArgs a;
    a.X = X.p; a.W = W; a.bias = bias; a.Y = Y.w(); a.pe = pe; a.M = M; a.N = N; a.K = K; a.ldx = ldx; a.ldy = ldy; a.T = T;
    // 16-byte loads: four fp32 or eight bf16; stores of four columns: 16 bytes of fp32 or 8 bytes of bf16
    a.vec_x = X.h ? (K % 8 == 0) && (ldx % 8 == 0) && al16(X.p) : (K % 4 == 0) && (ldx % 4 == 0) && al16(X.p);
    a.vec_w = (K % 4 == 0) && al16(W);
    a.vec_y = Y.h ? (ldy % 4 == 0) && ((uintptr_t)Y.p & 7) == 0 : (ldy % 4 == 0) && al16(Y.p);
    const int nb = EPI == EPI_SWIGLU ? kGBN / 2 : kGBN;
    a.dr = dr ? *dr : edtts::DropArgs{};
    const dim3 grid((M + kGBM - 1) / kGBM, (N + nb - 1) / nb);
    if ((X.h || Y.h) && !st.bf16)
      return fail(EDTTS_ERR_UNSUPPORTED, "generic kernels: a bf16 activation buffer needs the bf16 products (EDTTS_MATMUL_BF16)");
    return with_flag(st.bf16, [&](auto mm) { return with_flag(dr && drop_epi(EPI), [&](auto dropping) {
      return with_elem(X.h, [&](auto ex) { return with_elem(Y.h, [&](auto ey) -> int {
        using TX = typename decltype(ex)::type;
        using TY = typename decltype(ey)::type;
        constexpr bool MM16 = decltype(mm)::value, DROP = decltype(dropping)::value;
        if constexpr (gemm_instance<EPI, MM16, DROP, TX, TY>()) {
          hipLaunchKernelGGL((gemm_kernel<EPI, MM16, DROP, TX, TY>()), grid, dim3(256), 0, st.st, a);
          LAUNCH_CHECK("k_gen_gemm");
          return EDTTS_OK;
        } else {
          return fail(EDTTS_ERR_UNSUPPORTED, "generic kernels: no product with epilogue %d reads bf16=%d and stores bf16=%d", EPI, (int)X.h, (int)Y.h);
        }
      }); });
    }); });
  }
  template <int MODE>
  static int norm(hipStream_t st, const float* x, float* y, int rows, int W, const float* w, const float* b, float eps,
                  const float* mod = nullptr, int rows_per_b = 1, int mod_bstride = 0) {
    edtts_gen::NormArgs a{x, y, w, b, mod, rows, W, W, rows_per_b, mod_bstride, eps};
    hipLaunchKernelGGL(edtts_gen::k_gen_norm<MODE>, dim3((rows + 3) / 4), dim3(256), 0, st, a);
    LAUNCH_CHECK("k_gen_norm");
    return EDTTS_OK;
  }
  // k_gen_attn (a wave = 16 queries) or, for the bf16 attention, k_gen_attn16 (four waves = 64 queries), which alone reads bf16 rows
  template <int DT, bool ATT16, bool DROP, class TQ>
  static constexpr auto attn_kernel() {
    if constexpr (ATT16) return &edtts_gen::k_gen_attn16<DT, DROP, TQ>;
    else return &edtts_gen::k_gen_attn<DT, DROP>;
  }
  // (q, k, v of one element type: fp32, or bf16 with Layout::TAPE16, which only the bf16 attention reads)
  static int attn(hipStream_t st, const AttnShape& as, int B, Act q, int ldq, Act k, Act v, int ldkv, float* o,
                  int Tq, int Tk, int window, const int64_t* q_len, const int64_t* k_len, bool q_dbl, bool k_dbl, float* lse = nullptr,
                  const edtts::DropArgs* dr = nullptr) {
    if (q.h != k.h || q.h != v.h || (q.h && !as.att16))
      return fail(EDTTS_ERR_UNSUPPORTED, "generic kernels: bf16 q, k, v rows need the bf16 attention (EDTTS_ATTN_BF16), all three of them");
    edtts_gen::AttnArgs a{q.p, k.p, v.p, o, ldq, ldkv, as.H, Tq, Tk, as.DH, window, 1.4426950408889634f / sqrtf((float)as.DH), q_len, k_len,
                          (int)q_dbl, (int)k_dbl, lse, dr ? *dr : edtts::DropArgs{}};
    const int qpb = as.att16 ? 64 : 16;  // queries per block: one wave each 16 of them
    const dim3 grid((Tq + qpb - 1) / qpb, as.HEADS, B), block(4 * qpb);
    return with_head_tiles<8>(as.DH, [&](auto dt) { return with_flag(as.att16, [&](auto a16) {
      return with_flag(dr != nullptr, [&](auto dropping) { return with_elem(q.h, [&](auto eq) -> int {
        using TQ = typename decltype(eq)::type;
        constexpr bool ATT16 = decltype(a16)::value;
        if constexpr (ATT16 || std::is_same<TQ, float>::value) {  // (bf16 rows without the bf16 attention: refused above)
          hipLaunchKernelGGL((attn_kernel<decltype(dt)::value, ATT16, decltype(dropping)::value, TQ>()), grid, block, 0, st, a);
          LAUNCH_CHECK("k_gen_attn");
        }
        return EDTTS_OK;
      }); });
    }); });
  }

  static int copy(hipStream_t st, float* dst, const float* src, size_t n) {
    HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return EDTTS_OK;
  }

  // context rows (token_emb gather or sem_proj) + context PE, then per layer kv_down -> kv_norm -> kv_up into the K|V rows
  // (per-utterance lengths: context rows past S_b are built from whatever the padding holds and are never read -- the attention reads
  // keys < S_b only, and every other step is row-local)
  static int ctx(const CallCtx& cc, const int64_t* sem_idx, const float* sem_feat) { return ctx(cc, FwdBufs(cc), sem_idx, sem_feat); }
  static int ctx(const CallCtx& cc, const FwdBufs& fb, const int64_t* sem_idx, const float* sem_feat) {
    using namespace edtts_gen;
    const Layout& lo = cc.lo;
    const Workspace& ws = cc.ws;
    const float* blob = cc.blob;
    float* wsb = cc.wsb;
    const MmStream st{cc.st, lo.MM16 != 0};
    const int S = cc.S, rows = cc.B * S, H = lo.H, R = lo.R;
    float* c = fb.ctx;
    if (sem_feat) {
      TRY_G(gemm<EPI_PE>(st, sem_feat, lo.SD, blob + lo.semp, blob + lo.semp_b, c, H, rows, H, lo.SD, blob + lo.cpe, S));
    } else {
      unsigned* err = ws.errp ? ws.errp : reinterpret_cast<unsigned*>(wsb + ws.err);
      size_t nb = ((size_t)rows * H + 255) / 256;
      if (nb > 4096) nb = 4096;
      hipLaunchKernelGGL(k_gen_embed, dim3((unsigned)nb), dim3(256), 0, st, sem_idx, blob + lo.tok, blob + lo.cpe, c, rows, S, H, lo.NTOK, err, cc.ln.s);
      LAUNCH_CHECK("k_gen_embed");
    }
    for (int l = 0; l < lo.L; ++l) {
      const LayerLayout& y = lo.layer[l];
      const FwdLayerBufs& z = fb.layer[l];
      TRY_G(gemm<EPI_BIAS>(st, c, H, blob + y.kvd, nullptr, z.crp, R, rows, R, H));
      TRY_G(norm<NORM_RMS>(st, z.crp, z.crn, rows, R, blob + y.kvn, nullptr, 1e-6f));
      TRY_G(gemm<EPI_BIAS>(st, z.crn, R, blob + y.kvu, nullptr, z.kv, 2 * H, rows, 2 * H, R));
    }
    return EDTTS_OK;
  }

  static int forward(const CallCtx& c, const float* x, const float* cond_row, int cond_bstride, const StepTail& tail) {
    return forward(c, FwdBufs(c), x, cond_row, cond_bstride, tail);
  }
  // drop non-null: the four dropout sites of every block run their masked instantiations (the attention outputs and the SwiGLU
  // output in fb are then the dropped ones)
  static int forward(const CallCtx& c, const FwdBufs& fb, const float* x, const float* cond_row, int cond_bstride, const StepTail& tail,
                     const DropState* drop = nullptr) {
    using namespace edtts_gen;
    const Layout& lo = c.lo;
    const Workspace& ws = c.ws;
    const float* blob = c.blob;
    float* wsb = c.wsb;
    const MmStream st{c.st, lo.MM16 != 0};
    const Lens& ln = c.ln;
    const int B = c.B, T = c.T, S = c.S;
    const int M = B * T, H = lo.H, FH = lo.FM * lo.H, MEL = lo.MEL;
    float *h = wsb + ws.h, *xn = wsb + ws.g_xn;
    const size_t row = (size_t)2 * 2 * H;  // one layer's (norm1 | norm3) AdaLN rows
    auto snap = [&](float* dst) { return dst ? copy(st, dst, h, (size_t)M * H) : EDTTS_OK; };  // the residual stream as it stands
    TRY_G(gemm<EPI_PE>(st, x, MEL, blob + lo.inp, blob + lo.inp_b, h, H, M, H, MEL, blob + lo.pe, T));
    for (int l = 0; l < lo.L; ++l) {
      const LayerLayout& y = lo.layer[l];
      const FwdLayerBufs& z = fb.layer[l];
      DropArgs dra[4];
      for (int i = 0; i < 4; ++i) dra[i] = drop ? drop->site(l, i) : DropArgs{};
      auto D = [&](int i) -> const DropArgs* { return drop ? &dra[i] : nullptr; };
      // self-attention branch
      TRY_G(snap(z.h0));
      TRY_G(norm<NORM_RMS>(st, h, xn, M, H, blob + y.n1w, nullptr, 1e-6f, cond_row + l * row, T, cond_bstride));
      TRY_G(gemm<EPI_BIAS>(st, xn, H, blob + y.s_qkv, nullptr, z.qkv, 3 * H, M, 3 * H, H));  // (z.qkv, z.qc, z.kv, z.act: fp32 or bf16 rows)
      TRY_G(attn(st, lo, B, z.qkv, 3 * H, z.qkv + H, z.qkv + 2 * H, 3 * H, z.att1, T, T, c.window, ln.t, ln.t, ln.t_dbl, ln.t_dbl, z.lse1,
                 D(DROP_ATTN)));
      TRY_G(gemm<EPI_RESID>(st, z.att1, H, blob + y.g_proj, blob + y.proj_b, h, H, M, H, H));
      // cross-attention branch
      TRY_G(snap(z.h1));
      TRY_G(norm<NORM_RMS>(st, h, xn, M, H, blob + y.n2w, nullptr, 1e-6f));
      TRY_G(gemm<EPI_BIAS>(st, xn, H, blob + y.g_qp, nullptr, z.qc, H, M, H, H));
      TRY_G(attn(st, lo, B, z.qc, H, z.kv, z.kv + H, 2 * H, z.att2, T, S, -1, ln.t, ln.s, ln.t_dbl, false, z.lse2, D(DROP_CROSS)));
      TRY_G(gemm<EPI_RESID>(st, z.att2, H, blob + y.g_op, nullptr, h, H, M, H, H));
      // feed-forward branch
      TRY_G(snap(z.h2));
      TRY_G(norm<NORM_RMS>(st, h, xn, M, H, blob + y.n3w, nullptr, 1e-6f, cond_row + l * row + 2 * H, T, cond_bstride));
      TRY_G(gemm<EPI_SWIGLU>(st, xn, H, blob + y.g_up, blob + y.up_b, z.act, FH, M, FH, H, nullptr, 1, D(DROP_ACT)));
      TRY_G(gemm<EPI_RESID>(st, z.act, FH, blob + y.g_down, blob + y.down_b, h, H, M, H, FH, nullptr, 1, D(DROP_DOWN)));
    }
    TRY_G(snap(fb.hL));
    TRY_G(norm<NORM_LAYER>(st, h, xn, M, H, blob + lo.fnw, blob + lo.fnb, 1e-5f));
    float* e = tail.kind == TAIL_EPS ? tail.eps : wsb + ws.g_eps;
    TRY_G(gemm<EPI_BIAS>(st, xn, H, blob + lo.s_outp, blob + lo.outp_b, e, MEL, M, MEL, H));
    if (tail.kind == TAIL_EPS) {
      if (ln.t) {
        hipLaunchKernelGGL(k_gen_zero_past, dim3(grid_1d((size_t)M * MEL)), dim3(256), 0, st, e, ln.t, (int)ln.t_dbl, (size_t)M * MEL, T, MEL);
        LAUNCH_CHECK("k_gen_zero_past");
      }
      return EDTTS_OK;
    }
    KArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x;
    a.T = T; a.t_len = ln.t; a.t_dbl = ln.t_dbl;
    set_tail_args(tail, &a);
    bool vec = al16(x) && al16(a.x_prev) && al16(e) && (ln.t == nullptr || MEL % 4 == 0);
    if (tail.kind == TAIL_LMS) {
      vec = vec && al16(a.h_new) && al16(a.h_old) && al16(a.x0_hist) && al16(a.x0_all);
    } else if (tail.kind == TAIL_VLMS) {
      vec = vec && al16(a.v_uncond) && al16(a.h_new) && al16(a.h_old) && al16(a.x0_hist) && al16(a.x0_all) && al16(a.known) &&
            al16(a.noise) && (a.known == nullptr || MEL % 4 == 0);
    } else if (tail.kind == TAIL_VPRED) {
      vec = vec && al16(a.v_uncond);
    } else if (tail.kind == TAIL_DDPM) {
      vec = vec && al16(a.noise) && (a.philox_base & 3) == 0;
    } else {
      vec = vec && al16(a.x0);
    }
    const size_t n = (size_t)M * MEL;
    vec = vec && n % 4 == 0;
    size_t nb = ((vec ? n / 4 : n) + 255) / 256;
    if (nb > 4096) nb = 4096;
    if (nb < 1) nb = 1;
    return with_tail(tail.kind, [&](auto t) -> int {
      constexpr int TL = decltype(t)::value;
      if constexpr (TL != TAIL_QKV && TL != TAIL_EPS) {  // (TAIL_EPS has returned above; TAIL_QKV is never a forward's tail)
        hipLaunchKernelGGL(k_gen_tail<TL>, dim3((unsigned)nb), dim3(256), 0, st, a, e, n, (int)vec, MEL);
        LAUNCH_CHECK("k_gen_tail");
      }
      return EDTTS_OK;
    });
  }
};
