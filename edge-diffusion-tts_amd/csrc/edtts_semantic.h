// edtts_semantic.h -- the semantic head: HuBERT features -> FSQ / VQ tokens (included by edtts_kernels.hip).
//
// The trained head that sits after the frozen HuBERT backbone (reference models/encoder.py:40-57, models/fsq.py, models/vq.py):
//   z   = W3 LN(GELU(W1 h + b1)) + b3                      proj (Linear, GELU, LayerNorm, [Dropout = identity], Linear)
//   FSQ: u = Wd z + bd, zb = tanh(u), q = clamp(rint((zb + 1) half), 0, L - 1) / half - 1, zq_low = zb + (q - zb),
//        idx = sum rint((zq_low + 1) half) basis, z_q = Wu zq_low + bu
//   VQ:  dist = (|z|^2 - 2 z.c) + |c|^2, idx = first argmin, z_q = z + (c - z)
//
//   k_sem_encode   64 frames per block, 16 per wave.  Every contraction is W . X^T on v_mfma_f32_16x16x4_f32 with the weight as the
//                  A operand (rows = output features / codes) and the frames as the B operand (the frame on lane & 15): an output
//                  tile then holds features 4 (lane >> 4) + r of frame lane & 15 in register r, which is exactly the B fragment of
//                  the next contraction if the k order inside a 16-wide k-block is taken as 4 (lane >> 4) + j.  The packed weights
//                  use that order (k_sem_pack), so the whole chain stays in registers.  Weights stream through a double-buffered
//                  16 KiB LDS chunk that the block's four waves share (W1 is 384 KiB at the defaults); each feature row is read
//                  from HBM once, by the one wave whose frames it holds.  Usage counts: one integer atomicAdd per valid frame.
//                  k_sem_encode<true> is the training forward (edtts_semantic_bwd.h): the same chain, which also
//                  writes the backward's tape and multiplies the LayerNorm output by the head's dropout mask.
//   k_sem_decode   idx -> z_q, one thread per output element (FSQEncoder.decode / VectorQuantizer.decode; ids clamped)
//   k_sem_stats    counts -> (perplexity, used) in one block, fixed order, fp64 accumulation
//   k_sem_pack     state-dict matrices -> fragment order (zero-padded to 16 x 16 tiles), vectors padded, |c|^2 per code
namespace edtts_sem {

constexpr int kFrames = 64;      // frames per block (4 waves x 16)
constexpr int kChunk = 1024;     // f4 per LDS chunk (16 KiB); two chunks double-buffer the weight stream
constexpr int kMaxNT = 8;        // semantic_dim / 16 <= 8
constexpr int kMaxLevels = 16;   // FSQ dims (one 16-row tile)

// Packed blob (offsets in floats, every matrix 16-byte aligned).  Fragment order of a matrix M [R][K] as the A operand:
// f4 (kb, rt, lane) = M[16 rt + (lane & 15)][16 kb + 4 (lane >> 4) + j], j = 0..3 (zero outside R x K).
struct SemLayout {
  int in_dim, S, nt, kb1, vq, D, K, nrt_codes;
  long long n_codes;
  size_t w1, b1, lng, lnb, w3, b3;     // proj (w1 k-block major, w3 row-tile major)
  size_t wd, bd, wu, bu, half, lev, basis;  // FSQ
  size_t cb, cc, cbraw;                // VQ
  size_t total;                        // floats
};

static int sem_layout(const EdttsSemDims* d, SemLayout& L) {
  if (!d) return fail(EDTTS_ERR_ARG, "semantic dims is NULL");
  L = SemLayout{};
  L.in_dim = d->in_dim;
  L.S = d->semantic_dim;
  L.vq = d->quantizer == EDTTS_SEM_VQ;
  if (d->quantizer != EDTTS_SEM_FSQ && d->quantizer != EDTTS_SEM_VQ)
    return fail(EDTTS_ERR_UNSUPPORTED, "quantizer=%d (0 = FSQ, 1 = VQ)", d->quantizer);
  if (L.S < 16 || L.S > 16 * kMaxNT || L.S % 16)
    return fail(EDTTS_ERR_UNSUPPORTED, "semantic_dim=%d: need a multiple of 16 in [16, %d]", L.S, 16 * kMaxNT);
  if (L.in_dim != 0 && (L.in_dim < 16 || L.in_dim > 4096 || L.in_dim % 16))
    return fail(EDTTS_ERR_UNSUPPORTED, "in_dim=%d: need 0 (quantizer only) or a multiple of 16 in [16, 4096]", L.in_dim);
  L.nt = L.S / 16;
  L.kb1 = L.in_dim / 16;
  if (L.vq) {
    if (d->codebook_size < 1 || d->codebook_size > 65536)
      return fail(EDTTS_ERR_UNSUPPORTED, "codebook_size=%d outside [1, 65536]", d->codebook_size);
    L.K = d->codebook_size;
    L.nrt_codes = (L.K + 15) / 16;
    L.n_codes = L.K;
  } else {
    if (d->n_levels < 1 || d->n_levels > kMaxLevels) return fail(EDTTS_ERR_UNSUPPORTED, "n_levels=%d outside [1, %d]", d->n_levels, kMaxLevels);
    L.D = d->n_levels;
    L.n_codes = 1;
    for (int i = 0; i < L.D; ++i) {
      if (d->levels[i] < 2 || d->levels[i] > 256) return fail(EDTTS_ERR_UNSUPPORTED, "levels[%d]=%d outside [2, 256]", i, d->levels[i]);
      L.n_codes *= d->levels[i];
      if (L.n_codes > (1 << 24)) return fail(EDTTS_ERR_UNSUPPORTED, "FSQ levels give more than 2^24 codes");
    }
  }
  size_t o = 0;
  auto take = [&](size_t floats) { size_t r = o; o += (floats + 3) & ~(size_t)3; return r; };
  if (L.in_dim) {
    L.w1 = take((size_t)L.kb1 * L.nt * 64 * 4);
    L.b1 = take(L.S); L.lng = take(L.S); L.lnb = take(L.S);
    L.w3 = take((size_t)L.nt * L.nt * 64 * 4);
    L.b3 = take(L.S);
  }
  if (L.vq) {
    L.cb = take((size_t)L.nrt_codes * L.nt * 64 * 4);
    L.cc = take(L.K);
    L.cbraw = take((size_t)L.K * L.S);
  } else {
    L.wd = take((size_t)L.nt * 64 * 4);
    L.bd = take(16);
    L.wu = take((size_t)L.nt * 64 * 4);
    L.bu = take(L.S);
    L.half = take(16);
    L.lev = take(16);
    L.basis = take(32);  // int64 [16]
  }
  L.total = o;
  return EDTTS_OK;
}

// ------------------------------------------------------------------------------------------------ packing
// dst (fragment order, kb-major when kmajor else rt-major) <- M [R][K] row-major fp32
__global__ void k_sem_pack_frag(const float* __restrict__ M, int R, int K, int nrt, int nkb, int kmajor, float* __restrict__ dst) {
  const long long n = (long long)nrt * nkb * 256;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(e & 3), lane = (int)((e >> 2) & 63);
    const long long t = e >> 8;
    const int rt = kmajor ? (int)(t % nrt) : (int)(t / nkb);
    const int kb = kmajor ? (int)(t / nrt) : (int)(t % nkb);
    const int r = 16 * rt + (lane & 15), k = 16 * kb + 4 * (lane >> 4) + j;
    dst[e] = (r < R && k < K) ? M[(size_t)r * K + k] : 0.f;
  }
}

// dst[i] = i < n ? src[i] : 0 for i < n_pad
__global__ void k_sem_pack_vec(const float* __restrict__ src, int n, int n_pad, float* __restrict__ dst) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += gridDim.x * blockDim.x)
    dst[i] = i < n ? src[i] : 0.f;
}

// |c|^2 of each code (fp32, sequential over the features) and the raw codebook copy the gather reads
__global__ void k_sem_pack_codes(const float* __restrict__ cbk, int K, int S, float* __restrict__ cc, float* __restrict__ raw) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < K; c += gridDim.x * blockDim.x) {
    const float* row = cbk + (size_t)c * S;
    float s = 0.f;
    for (int k = 0; k < S; ++k) {
      const float v = row[k];
      s = fmaf(v, v, s);
      raw[(size_t)c * S + k] = v;
    }
    cc[c] = s;
  }
}

struct SemTables {
  float half[kMaxLevels];
  int lev[kMaxLevels];
  long long basis[kMaxLevels];
};
__global__ void k_sem_pack_tables(SemTables t, float* half, int* lev, long long* basis) {
  const int d = threadIdx.x;
  if (d < kMaxLevels) {
    half[d] = t.half[d];
    lev[d] = t.lev[d];
    basis[d] = t.basis[d];
  }
}

// ------------------------------------------------------------------------------------------------ encode
struct EncArgs {
  const float* p;          // packed blob
  const float* h;          // [N][in_dim] (in_dim 0: z [N][S])
  const long long* len;    // [B] or null
  long long* idx;          // [N]
  float* z;                // [N][S] or null
  float* zq;               // [N][S] or null
  int* counts;             // [n_codes] or null
  int N, T, in_dim, S, nt, kb1, vq, D, K, nrt_codes;
  long long n_codes;
  size_t w1, b1, lng, lnb, w3, b3, wd, bd, wu, bu, half, lev, basis, cb, cc, cbraw;
};

// ... plus what the training forward writes and its dropout site (k_sem_encode<true> only: the inference kernel's arguments stay as
// they are)
struct EncTrainArgs : EncArgs {
  float* t_y1;   // tape: proj.0 output before GELU [N][S] (in_dim > 0)
  float* t_zb;   // tape: tanh(proj_down(z)) [N][16]
  DropArgs dr;   // the mask between LayerNorm and the last Linear
  int dropping;
  float* t_r;    // VQ tape: r = c - z [N][S]
  float* t_sq;   // VQ tape: sum_s r^2 per frame [N]
};
template <bool TRAIN>
struct EncArgsOf { using type = EncArgs; };
template <>
struct EncArgsOf<true> { using type = EncTrainArgs; };

// Copy `n` f4 (n <= kChunk) of a packed stream into registers: thread tid holds elements tid + 256 i.
EDTTS_DEV void chunk_load(const f4* __restrict__ src, int n, f4 (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = threadIdx.x + 256 * i;
    r[i] = e < n ? src[e] : splat(0.f);
  }
}
EDTTS_DEV void chunk_store(f4* dst, int n, const f4 (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = threadIdx.x + 256 * i;
    if (e < n) dst[e] = r[i];
  }
}

// Y = M . X^T for n_rt row tiles of a rt-major packed matrix with nkb k-blocks (<= kMaxNT), X in registers as B fragments (X[kb]
// element j = X[frame lane & 15][16 kb + 4 (lane >> 4) + j]).  Accumulators start at bias (rows >= n_rows: 0).  epi(rt, acc) sees each
// finished row tile.  Every wave of the block calls this with the same arguments (it synchronises the block).
template <class Epi>
EDTTS_DEV void stream_rt(const f4* __restrict__ M, int n_rt, int nkb, const float* __restrict__ bias, int n_rows, const f4 (&X)[kMaxNT],
                         f4 (*buf)[kChunk], Epi&& epi) {
  const int lane = threadIdx.x & 63;
  const int per = nkb * 64, G = kChunk / per, n_chunks = (n_rt + G - 1) / G;
  f4 pre[4];
  __syncthreads();  // the buffers' previous readers are done
  chunk_load(M, min(G, n_rt) * per, pre);
  chunk_store(buf[0], min(G, n_rt) * per, pre);
  __syncthreads();
  for (int c = 0; c < n_chunks; ++c) {
    const int nxt = min(G, n_rt - (c + 1) * G) * per;  // f4 of the next chunk (<= 0: none)
    if (nxt > 0) chunk_load(M + (size_t)(c + 1) * G * per, nxt, pre);
    const f4* cur = buf[c & 1];
    for (int g = 0; g < G; ++g) {
      const int rt = c * G + g;
      if (rt >= n_rt) break;
      f4 acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * rt + 4 * (lane >> 4) + r;
        acc[r] = (bias && row < n_rows) ? bias[row] : 0.f;
      }
      const f4* a = cur + g * per + lane;
#pragma unroll
      for (int kb = 0; kb < kMaxNT; ++kb) {
        if (kb < nkb) {
          const f4 w = a[kb * 64];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc = EDTTS_MFMA(w[j], X[kb][j], acc);
        }
      }
      epi(rt, acc);
    }
    if (nxt > 0) chunk_store(buf[(c + 1) & 1], nxt, pre);
    __syncthreads();
  }
}

// Y[t] = W1 . H^T for t < nt with W1 kb-major, H from global memory (each lane reads f4 (frame, 16 kb + 4 (lane >> 4)) once)
EDTTS_DEV void stream_w1(const f4* __restrict__ W, int kb1, int nt, const float* __restrict__ hrow, bool ok, f4 (&acc)[kMaxNT],
                         f4 (*buf)[kChunk]) {
  const int lane = threadIdx.x & 63;
  const int per = nt * 64;
  const int CK = min(4, kChunk / per), n_chunks = (kb1 + CK - 1) / CK;
  const float* hp = hrow + 4 * (lane >> 4);
  f4 pre[4], hx[4], hn[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) hx[q] = (ok && q < CK && q < kb1) ? ldg4(hp + 16 * q) : splat(0.f);
  __syncthreads();
  chunk_load(W, min(CK, kb1) * per, pre);
  chunk_store(buf[0], min(CK, kb1) * per, pre);
  __syncthreads();
  for (int c = 0; c < n_chunks; ++c) {
    const int kb0n = (c + 1) * CK;
    const int nxt = min(CK, kb1 - kb0n) * per;
    if (nxt > 0) chunk_load(W + (size_t)kb0n * per, nxt, pre);
#pragma unroll
    for (int q = 0; q < 4; ++q) hn[q] = (ok && q < CK && kb0n + q < kb1) ? ldg4(hp + 16 * (kb0n + q)) : splat(0.f);
    const f4* cur = buf[c & 1] + lane;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < CK && c * CK + q < kb1) {
#pragma unroll
        for (int t = 0; t < kMaxNT; ++t) {
          if (t < nt) {
            const f4 w = cur[(q * nt + t) * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[t] = EDTTS_MFMA(w[j], hx[q][j], acc[t]);
          }
        }
      }
    }
    if (nxt > 0) chunk_store(buf[(c + 1) & 1], nxt, pre);
#pragma unroll
    for (int q = 0; q < 4; ++q) hx[q] = hn[q];
    __syncthreads();
  }
}

EDTTS_DEV float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

// sum over the four lane groups that hold one frame's features (lanes l, l ^ 16, l ^ 32, l ^ 48)
EDTTS_DEV float group_sum(float v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

template <bool TRAIN>
__global__ __launch_bounds__(256) void k_sem_encode(typename EncArgsOf<TRAIN>::type a) {
  __shared__ f4 buf[2][kChunk];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, grp = lane >> 4;
  const int frame = blockIdx.x * kFrames + 16 * w + (lane & 15);
  bool ok = frame < a.N;
  if (ok && a.len) {
    const int b = frame / a.T, t = frame - b * a.T;
    long long n = a.len[b];
    n = n < 1 ? 1 : (n > a.T ? a.T : n);  // the decoder's clamp of a device length (edtts_*_len)
    ok = t < n;
  }
  const float* p = a.p;
  const int S = a.S, nt = a.nt;
  f4 z[kMaxNT];
  if (a.in_dim) {
    // ---- proj: y = W1 h + b1 -> GELU -> LayerNorm -> z = W3 y + b3
    f4 y[kMaxNT];
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) y[t][r] = t < nt ? p[a.b1 + 16 * t + 4 * grp + r] : 0.f;
    const float* hrow = a.h + (size_t)(ok ? frame : 0) * a.in_dim;
    stream_w1(reinterpret_cast<const f4*>(p + a.w1), a.kb1, nt, hrow, ok, y, buf);
    if constexpr (TRAIN) {
      if (frame < a.N) {
#pragma unroll
        for (int t = 0; t < kMaxNT; ++t)
          if (t < nt) stg4(a.t_y1 + (size_t)frame * S + 4 * grp + 16 * t, ok ? y[t] : splat(0.f));
      }
    }
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t)
      if (t < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          y[t][r] = gelu_erf(y[t][r]);
          s += y[t][r];
        }
      }
    const float mean = group_sum(s) / (float)S;
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t)
      if (t < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float d = y[t][r] - mean;
          v = fmaf(d, d, v);
        }
      }
    const float rstd = 1.0f / sqrtf(group_sum(v) / (float)S + 1e-5f);
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * t + 4 * grp + r;
        y[t][r] = t < nt ? (y[t][r] - mean) * rstd * p[a.lng + f] + p[a.lnb + f] : 0.f;
      }
    if constexpr (TRAIN) {
      if (a.dropping) {
        const DropArgs dr = drop_live(a.dr);
#pragma unroll
        for (int t = 0; t < kMaxNT; ++t)
          if (t < nt) y[t] = y[t] * drop_row4(dr, frame, 16 * t + 4 * grp);
      }
    }
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t) z[t] = splat(0.f);
    stream_rt(reinterpret_cast<const f4*>(p + a.w3), nt, nt, p + a.b3, S, y, buf, [&](int rt, f4 acc) {
#pragma unroll
      for (int t = 0; t < kMaxNT; ++t)
        if (t == rt) z[t] = acc;
    });
  } else {
    // quantizer only: z is the input
    const float* zrow = a.h + (size_t)(ok ? frame : 0) * S + 4 * grp;
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t) z[t] = (ok && t < nt) ? ldg4(zrow + 16 * t) : splat(0.f);
  }
  const size_t orow = (size_t)frame * S + 4 * grp;
  if (a.z && frame < a.N) {
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t)
      if (t < nt) stg4(a.z + orow + 16 * t, ok ? z[t] : splat(0.f));
  }

  long long code = 0;
  if (!a.vq) {
    // ---- FSQ: u = Wd z + bd (one 16-row tile), bound, quantise, index; z_q = Wu zq_low + bu
    f4 zl[kMaxNT];
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t) zl[t] = splat(0.f);
    int part = 0;
    stream_rt(reinterpret_cast<const f4*>(p + a.wd), 1, nt, p + a.bd, a.D, z, buf, [&](int, f4 u) {
      const int* lev = reinterpret_cast<const int*>(p + a.lev);
      const long long* basis = reinterpret_cast<const long long*>(p + a.basis);
      [[maybe_unused]] f4 zbv = splat(0.f);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = 4 * grp + r;
        if (d < a.D) {
          const float half = p[a.half + d];
          const float zb = tanhf(u[r]);
          if constexpr (TRAIN) zbv[r] = zb;
          float q = rintf((zb + 1.0f) * half);                       // torch.round: half to even
          q = fminf(fmaxf(q, 0.0f), (float)(lev[d] - 1));
          q = q / half - 1.0f;
          const float zq = zb + (q - zb);                            // the straight-through line, as computed
          zl[0][r] = zq;
          part += (int)rintf((zq + 1.0f) * half) * (int)basis[d];    // codes_to_indices, recomputed from zq_low
        }
      }
      if constexpr (TRAIN) {
        if (frame < a.N) stg4(a.t_zb + (size_t)frame * 16 + 4 * grp, ok ? zbv : splat(0.f));
      }
    });
    part += __shfl_xor(part, 16);
    part += __shfl_xor(part, 32);
    code = part < 0 ? 0 : (part >= a.n_codes ? a.n_codes - 1 : part);  // (only a NaN feature can leave the range)
    stream_rt(reinterpret_cast<const f4*>(p + a.wu), nt, 1, p + a.bu, S, zl, buf, [&](int rt, f4 acc) {
      if (a.zq && frame < a.N) stg4(a.zq + orow + 16 * rt, ok ? acc : splat(0.f));
    });
  } else {
    // ---- VQ: nearest code by (|z|^2 - 2 z.c) + |c|^2, first minimum; z_q = z + (c - z)
    float zz = 0.f;
#pragma unroll
    for (int t = 0; t < kMaxNT; ++t)
      if (t < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) zz = fmaf(z[t][r], z[t][r], zz);
      }
    zz = group_sum(zz);
    float best = INFINITY;
    int bi = 0x7fffffff;
    const float* cc = p + a.cc;
    stream_rt(reinterpret_cast<const f4*>(p + a.cb), a.nrt_codes, nt, nullptr, 0, z, buf, [&](int rt, f4 dot) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * rt + 4 * grp + r;
        if (c < a.K) {
          const float d = (zz - 2.0f * dot[r]) + cc[c];
          if (d < best) { best = d; bi = c; }
        }
      }
    });
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (bi == 0x7fffffff) bi = 0;  // every distance NaN
    code = bi;
    if constexpr (TRAIN) {
      // the training forward (edtts_semantic_bwd.h): next to the gather, the residual r = c - z and its
      // per-frame sum of squares go to the tape (the loss and both gradients are functions of r alone)
      float q = 0.f;
      if (frame < a.N) {
        const float* crow = p + a.cbraw + (size_t)bi * S + 4 * grp;
#pragma unroll
        for (int t = 0; t < kMaxNT; ++t)
          if (t < nt) {
            const f4 c = ldg4(crow + 16 * t);
            const f4 r = c - z[t];
            stg4(a.zq + orow + 16 * t, ok ? z[t] + r : splat(0.f));
            stg4(a.t_r + orow + 16 * t, ok ? r : splat(0.f));
            if (ok) {
#pragma unroll
              for (int j = 0; j < 4; ++j) q = fmaf(r[j], r[j], q);
            }
          }
      }
      q = group_sum(q);  // every lane group of a frame then holds the same value: one store
      if (grp == 0 && frame < a.N) a.t_sq[frame] = q;
    } else {
      if (a.zq && frame < a.N) {
        const float* crow = p + a.cbraw + (size_t)bi * S + 4 * grp;
#pragma unroll
        for (int t = 0; t < kMaxNT; ++t)
          if (t < nt) {
            const f4 c = ldg4(crow + 16 * t);
            stg4(a.zq + orow + 16 * t, ok ? z[t] + (c - z[t]) : splat(0.f));
          }
      }
    }
  }
  if (grp == 0 && frame < a.N) {
    a.idx[frame] = ok ? code : 0;
    if (ok && a.counts) atomicAdd(a.counts + code, 1);
  }
}

// ------------------------------------------------------------------------------------------------ decode / stats
__global__ void k_sem_decode(const float* __restrict__ p, const long long* __restrict__ idx, long long n, int S, int vq, int D,
                             long long n_codes, size_t wu, size_t bu, size_t half, size_t lev, size_t cbraw, float* __restrict__ out) {
  const long long total = n * S;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long i = e / S;
    const int s = (int)(e - i * S);
    long long id = idx[i];
    id = id < 0 ? 0 : (id >= n_codes ? n_codes - 1 : id);  // the decoder's token-id policy: clamp (the host checks in debug mode)
    if (vq) {
      out[e] = p[cbraw + (size_t)id * S + s];
      continue;
    }
    // FSQ.indices_to_codes as the reference writes it: the LAST dimension is the least significant digit
    const int* L = reinterpret_cast<const int*>(p + lev);
    float zl[kMaxLevels];
    int rem = (int)id;
#pragma unroll
    for (int d = kMaxLevels - 1; d >= 0; --d) {
      if (d < D) {
        zl[d] = (float)(rem % L[d]) / p[half + d] - 1.0f;
        rem /= L[d];
      } else {
        zl[d] = 0.f;
      }
    }
    // Wu from its fragment-packed form: element (row s, k d) sits at f4 (rt = s / 16, lane = s % 16 + 16 (d / 4)), component d % 4
    const float* wrow = p + wu + ((size_t)(s >> 4) * 64 + (s & 15)) * 4;
    float acc = p[bu + s];
#pragma unroll
    for (int d = 0; d < kMaxLevels; ++d)
      if (d < D) acc = fmaf(wrow[(d >> 2) * 64 + (d & 3)], zl[d], acc);
    out[e] = acc;
  }
}

// probs = counts / max(sum, 1); perplexity = exp(-sum p log(max(p, 1e-12))); used = #(counts > 0)   (fsq.py:189-193, vq.py:101-105)
__global__ __launch_bounds__(256) void k_sem_stats(const int* __restrict__ counts, long long n, float* perplexity, long long* used) {
  __shared__ double sd[256];
  __shared__ long long sl[256];
  const int tid = threadIdx.x;
  long long tot = 0, u = 0;
  for (long long i = tid; i < n; i += 256) {
    tot += counts[i];
    u += counts[i] > 0;
  }
  sl[tid] = tot;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sl[tid] += sl[tid + o];
    __syncthreads();
  }
  const double total = sl[0] < 1 ? 1.0 : (double)(float)sl[0];
  __syncthreads();
  double h = 0.0;
  for (long long i = tid; i < n; i += 256) {
    const double pr = (double)((float)counts[i] / (float)total);
    if (pr > 0.0) h += pr * log(pr < 1e-12 ? 1e-12 : pr);
  }
  sd[tid] = h;
  sl[tid] = u;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      sd[tid] += sd[tid + o];
      sl[tid] += sl[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    *perplexity = (float)exp(-sd[0]);
    *used = sl[0];
  }
}

// The start of an encode call, inference or training: `counts` zeroed, the kernel's arguments from the layout and the call's
// pointers, and *blocks = its grid (0: no frames, nothing to launch).  The layout holds zeros in the other quantizer's fields
// (sem_layout starts from SemLayout{}): an FSQ head gets vq = K = nrt_codes = 0 and no codebook offsets, a VQ head D = 0.
static int enc_begin(const SemLayout& L, const void* packed, const float* h, int B, int T, const int64_t* lengths, int64_t* idx, float* z,
                     float* z_q, int32_t* counts, hipStream_t st, EncArgs& a, unsigned* blocks) {
  if (counts) HIP_TRY(hipMemsetAsync(counts, 0, (size_t)L.n_codes * sizeof(int32_t), st));
  const int N = B * T;
  *blocks = (unsigned)((N + kFrames - 1) / kFrames);
  a.p = (const float*)packed;
  a.h = h;
  a.len = (const long long*)lengths;
  a.idx = (long long*)idx;
  a.z = z;
  a.zq = z_q;
  a.counts = counts;
  a.N = N; a.T = T; a.in_dim = L.in_dim; a.S = L.S; a.nt = L.nt; a.kb1 = L.kb1; a.vq = L.vq; a.D = L.D; a.K = L.K;
  a.nrt_codes = L.nrt_codes;
  a.n_codes = L.n_codes;
  a.w1 = L.w1; a.b1 = L.b1; a.lng = L.lng; a.lnb = L.lnb; a.w3 = L.w3; a.b3 = L.b3;
  a.wd = L.wd; a.bd = L.bd; a.wu = L.wu; a.bu = L.bu; a.half = L.half; a.lev = L.lev; a.basis = L.basis;
  a.cb = L.cb; a.cc = L.cc; a.cbraw = L.cbraw;
  return EDTTS_OK;
}

}  // namespace edtts_sem

extern "C" {

int edtts_sem_packed_bytes(const EdttsSemDims* dims, size_t* out_bytes) {
  edtts_sem::SemLayout L;
  TRY_G(edtts_sem::sem_layout(dims, L));
  if (!out_bytes) return fail(EDTTS_ERR_ARG, "out_bytes is NULL");
  *out_bytes = L.total * sizeof(float);
  return EDTTS_OK;
}

int edtts_sem_num_codes(const EdttsSemDims* dims, int64_t* out_codes) {
  edtts_sem::SemLayout L;
  TRY_G(edtts_sem::sem_layout(dims, L));
  if (!out_codes) return fail(EDTTS_ERR_ARG, "out_codes is NULL");
  *out_codes = L.n_codes;
  return EDTTS_OK;
}

int edtts_sem_pack(const EdttsSemDims* dims, const void* const* slots, int n_slots, void* packed, void* stream) {
  using namespace edtts_sem;
  SemLayout L;
  TRY_G(sem_layout(dims, L));
  const int want = (L.in_dim ? 6 : 0) + (L.vq ? 1 : 4);
  if (!slots || !packed) return fail(EDTTS_ERR_ARG, "slots/packed is NULL");
  if (n_slots != want) return fail(EDTTS_ERR_ARG, "expected %d weight slots, got %d", want, n_slots);
  for (int i = 0; i < n_slots; ++i)
    if (!slots[i]) return fail(EDTTS_ERR_ARG, "weight slot %d is NULL", i);
  hipStream_t st = (hipStream_t)stream;
  float* P = (float*)packed;
  const float* const* s = (const float* const*)slots;
  const int S = L.S;
  int i = 0;
  auto frag = [&](const float* M, int R, int K, int nrt, int nkb, int kmajor, size_t off) -> int {
    const long long n = (long long)nrt * nkb * 256;
    hipLaunchKernelGGL(k_sem_pack_frag, dim3((unsigned)min((n + 255) / 256, 4096LL)), dim3(256), 0, st, M, R, K, nrt, nkb, kmajor, P + off);
    LAUNCH_CHECK("k_sem_pack_frag");
    return EDTTS_OK;
  };
  auto vec = [&](const float* v, int n, int n_pad, size_t off) -> int {
    hipLaunchKernelGGL(k_sem_pack_vec, dim3((n_pad + 255) / 256), dim3(256), 0, st, v, n, n_pad, P + off);
    LAUNCH_CHECK("k_sem_pack_vec");
    return EDTTS_OK;
  };
  if (L.in_dim) {
    TRY_G(frag(s[0], S, L.in_dim, L.nt, L.kb1, 1, L.w1));
    TRY_G(vec(s[1], S, S, L.b1));
    TRY_G(vec(s[2], S, S, L.lng));
    TRY_G(vec(s[3], S, S, L.lnb));
    TRY_G(frag(s[4], S, S, L.nt, L.nt, 0, L.w3));
    TRY_G(vec(s[5], S, S, L.b3));
    i = 6;
  }
  if (L.vq) {
    TRY_G(frag(s[i], L.K, S, L.nrt_codes, L.nt, 0, L.cb));
    hipLaunchKernelGGL(k_sem_pack_codes, dim3((L.K + 255) / 256), dim3(256), 0, st, s[i], L.K, S, P + L.cc, P + L.cbraw);
    LAUNCH_CHECK("k_sem_pack_codes");
  } else {
    TRY_G(frag(s[i], L.D, S, 1, L.nt, 0, L.wd));        // proj_down.weight [D][S]
    TRY_G(vec(s[i + 1], L.D, 16, L.bd));
    TRY_G(frag(s[i + 2], S, L.D, L.nt, 1, 0, L.wu));    // proj_up.weight [S][D]
    TRY_G(vec(s[i + 3], S, S, L.bu));
    // per-dimension tables from the dims (kernel arguments: no host copy, capturable)
    SemTables tb{};
    long long b = 1;
    for (int d = 0; d < L.D; ++d) {
      tb.half[d] = ((float)dims->levels[d] - 1.0f) / 2.0f;  // (levels.float() - 1) / 2
      tb.lev[d] = dims->levels[d];
      tb.basis[d] = b;                                     // cumprod([1] + levels[:-1])
      b *= dims->levels[d];
    }
    hipLaunchKernelGGL(k_sem_pack_tables, dim3(1), dim3(16), 0, st, tb, P + L.half, reinterpret_cast<int*>(P + L.lev),
                       reinterpret_cast<long long*>(P + L.basis));
    LAUNCH_CHECK("k_sem_pack_tables");
  }
  return EDTTS_OK;
}

int edtts_sem_encode(const EdttsSemDims* dims, const void* packed, const float* h, int B, int T, const int64_t* lengths, int64_t* idx,
                     float* z, float* z_q, int32_t* counts, void* stream) {
  using namespace edtts_sem;
  SemLayout L;
  TRY_G(sem_layout(dims, L));
  if (!packed || !h || !idx) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (B < 0 || T < 0 || (long long)B * T > 0x7fffffffLL - kFrames) return fail(EDTTS_ERR_ARG, "B=%d T=%d out of range", B, T);
  hipStream_t st = (hipStream_t)stream;
  EncArgs a{};
  unsigned blocks;
  TRY_G(enc_begin(L, packed, h, B, T, lengths, idx, z, z_q, counts, st, a, &blocks));
  if (blocks == 0) return EDTTS_OK;
  hipLaunchKernelGGL(k_sem_encode<false>, dim3(blocks), dim3(256), 0, st, a);
  LAUNCH_CHECK("k_sem_encode");
  return EDTTS_OK;
}

int edtts_sem_decode(const EdttsSemDims* dims, const void* packed, const int64_t* idx, int64_t n, float* z_q, void* stream) {
  using namespace edtts_sem;
  SemLayout L;
  TRY_G(sem_layout(dims, L));
  if (!packed || (n > 0 && (!idx || !z_q))) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (n < 0) return fail(EDTTS_ERR_ARG, "n=%lld < 0", (long long)n);
  if (n == 0) return EDTTS_OK;
  const long long total = n * L.S;
  hipLaunchKernelGGL(k_sem_decode, dim3((unsigned)min((total + 255) / 256, 65536LL)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)packed, (const long long*)idx, (long long)n, L.S, L.vq, L.D, L.n_codes, L.wu, L.bu, L.half, L.lev,
                     L.cbraw, z_q);
  LAUNCH_CHECK("k_sem_decode");
  return EDTTS_OK;
}

int edtts_sem_stats(const int32_t* counts, int64_t n_codes, float* perplexity, int64_t* used, void* stream) {
  if (!counts || !perplexity || !used) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (n_codes < 1) return fail(EDTTS_ERR_ARG, "n_codes=%lld < 1", (long long)n_codes);
  hipLaunchKernelGGL(edtts_sem::k_sem_stats, dim3(1), dim3(256), 0, (hipStream_t)stream, counts, (long long)n_codes, perplexity,
                     (long long*)used);
  LAUNCH_CHECK("k_sem_stats");
  return EDTTS_OK;
}

}  // extern "C"
