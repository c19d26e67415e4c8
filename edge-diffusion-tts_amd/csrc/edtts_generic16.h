// edtts_generic16.h -- bf16 MFMA products for the generic decoder path (included by edtts_kernels.hip after edtts_generic.h and
// edtts_generic_bwd.h).  Selected per decoder with EDTTS_MATMUL_BF16 (Layout::MM16): the launch lists of
// GenericLauncher / TrainLauncher stay single and hand an MmStream to every `linear` site, which picks the kernel.
//
// What is rounded: the two operands of a product, fp32 in global memory, to bf16 (round to nearest even, v_cvt_pk_bf16_f32) in
// registers on their way into LDS.  Products on v_mfma_f32_16x16x32_bf16, accumulators fp32, epilogues and stores those of the fp32
// kernels (gemm_epilogue / bgemm_store restate them).  Nothing is stored as bf16 in global memory -- unless the decoder also carries
// EDTTS_TAPE_BF16 (Layout::TAPE16): the four activation buffers that only these loaders and the attention's read
// (q|k|v, the cross queries, the cross K|V, the SwiGLU output) then hold bf16(x), which is the operand the loaders form from x.  The
// kernels take the element type of such an operand as a template parameter that defaults to float: an instantiation with float is
// the kernel of before, statement for statement.  TX = __bf16 loads X without converting; TY = __bf16 rounds the epilogue's four
// columns with the loaders' conversion and stores them as 8 bytes (or 2-byte elements where the pitch or the edge forbids it).
//
//   k_gen_gemm16<EPI, DROP, TX, TY>  k_gen_gemm's product: same GemmArgs, grid, 64 x 64 block tile and wave tiles, K tiles of 32
//   k_bwd_gemm16<ACC, LEN, TB>       k_bwd_gemm's product: same BGemmArgs, grid and slabs, run-time strides on both operands
//   launch_cond16            the conditioning rows (time MLP, AdaLN projections) as k_bwd_gemm16 products
//
// LDS: two buffers of [X | W][64 rows][32 k] bf16; lane (fq, g) reads k = 8g .. 8g + 7 of row fq as one ds_read_b128 (the operand
// layout of edtts_hubert16.h).  The row pitch is 48 elements = 96 bytes = 6 sixteen-byte slots, not that header's 80: a ds_read_b128
// is served in four groups of 16 lanes that are NOT contiguous -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 -- so a
// group holds rows {0-3, 12-15} of chunk g and rows 4-11 of chunk g + 1.  At slot (6 row + chunk) mod 16 the first set lands on the
// eight even slots and the second on the eight odd ones (or the reverse): each group touches all 64 banks once.  At 80 bytes rows
// 1-3 of one chunk meet rows 4-6 of the next (2-way).  One barrier per K tile; the next tile's global loads are in flight during the
// MFMAs.
//
// Loaders.  Every thread stages 8 consecutive k of ONE row per operand and tile, converts them in registers and writes them as one
// 16-byte LDS store, whatever the operand's strides; two-byte LDS writes, which would serialise on banks, never happen.  A
// ds_write_b128 is served in groups of 8 contiguous lanes over 32 banks = 8 slots, so 8 neighbouring threads take 4 rows x 2 chunks:
// slots (6 row + chunk) mod 8 = {0,1}, {6,7}, {4,5}, {2,3} -- conflict-free (8 rows of one chunk, or 2 rows x 4 chunks, are 2-way).
// What differs between the two kinds of operand is which 4 rows x 2 chunks:
//   k contiguous (X, W of the forward; dY of dX)   ld_k_row / ld_k_chunk: a wave covers 16 rows x 4 chunks, i.e. 128 contiguous bytes
//                                                  of each row; two 16-byte loads per thread where alignment and K % 4 allow, else
//                                                  8 guarded scalar loads
//   rows contiguous (W of dX; dY^T and X^T of dW)  ld_r_row / ld_r_chunk: a wave covers 32 rows x 2 chunks; 8 strided scalar loads
//                                                  per thread, each of them two runs of 32 consecutive rows (128 bytes) across the
//                                                  wave.  The transposition happens in registers: the gather IS the transpose.
// Everything past M, N, K (or the slab's end) and every dead row of a ragged batch is staged as zero.
//
// Every output element is one k-ordered chain of MFMA steps whatever its tile, M or the batch: no atomics, no split accumulation
// other than the dW slabs (k_bwd_slabsum, fp32, slab order), no scratch.
namespace edtts_gen {

constexpr int kG16K = 32;           // K tile: one MFMA k-step
constexpr int kG16Ld = kG16K + 16;  // LDS row pitch in bf16 (96 bytes, see above)
// the loaders' thread -> (LDS row, first k of its 8) maps (see above); both are bijections of 256 threads onto 64 rows x 4 chunks
EDTTS_DEV int ld_k_row(int tid) { return ((tid >> 1) & 3) + 4 * (tid >> 4); }
EDTTS_DEV int ld_k_chunk(int tid) { return 8 * ((tid & 1) + 2 * ((tid >> 3) & 1)); }
EDTTS_DEV int ld_r_row(int tid) { return 32 * ((tid >> 6) & 1) + ((tid & 63) >> 1); }
EDTTS_DEV int ld_r_chunk(int tid) { return 8 * (2 * (tid >> 7) + (tid & 1)); }

// k .. k + 7 of a row whose k is contiguous -> 8 bf16; k at or past kend (and a row that is not ok) reads as zero
// (vec: kend % 4 == 0 and 16-byte aligned rows, so a float4 lies wholly inside or wholly outside)
EDTTS_DEV bf8 load8_row(const float* p, int k, int kend, bool ok, int vec) {
  f4 lo = splat(0.f), hi = splat(0.f);
  if (vec) {
    if (ok && k < kend) lo = ldg4(p + k);
    if (ok && k + 4 < kend) hi = ldg4(p + k + 4);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      lo[r] = (ok && k + r < kend) ? p[k + r] : 0.f;
      hi[r] = (ok && k + 4 + r < kend) ? p[k + 4 + r] : 0.f;
    }
  }
  return edtts16::pack8(lo, hi);
}
// Elements that are bf16 already.  A 2-byte load goes into a register of its own and the eight are paired afterwards, as the fp32
// loaders convert afterwards: inserting each into a packed vector as it arrives makes every load wait for the one before it (measured:
// dW_down 245 -> 672 us per step at B = 64 x 512).
EDTTS_DEV unsigned ld_bf16(const __bf16* p, bool ok) { return ok ? (unsigned)*reinterpret_cast<const unsigned short*>(p) : 0u; }
EDTTS_DEV bf8 pair8(const unsigned (&e)[8]) {
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  return __builtin_bit_cast(bf8, u4v{e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16, e[6] | e[7] << 16});
}
// ... of a row that holds bf16 already (vec: kend % 8 == 0 and 16-byte aligned rows, so the eight lie wholly inside or outside)
EDTTS_DEV bf8 load8_row(const __bf16* p, int k, int kend, bool ok, int vec) {
  if (vec) {
    bf8 v = edtts16::as_bf8(splat(0.f));
    if (ok && k < kend) v = *reinterpret_cast<const bf8*>(p + k);
    return v;
  }
  unsigned e[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) e[r] = ld_bf16(p + k + r, ok && k + r < kend);
  return pair8(e);
}
// ... of a row whose k has stride sk; bit i of live: k + i is loaded
EDTTS_DEV bf8 gather8(const float* p, long sk, int k, int kend, bool ok, unsigned live) {
  f4 lo, hi;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lo[r] = (ok && k + r < kend && (live >> r & 1u)) ? p[(size_t)(k + r) * sk] : 0.f;
    hi[r] = (ok && k + 4 + r < kend && (live >> (r + 4) & 1u)) ? p[(size_t)(k + 4 + r) * sk] : 0.f;
  }
  return edtts16::pack8(lo, hi);
}
EDTTS_DEV bf8 gather8(const __bf16* p, long sk, int k, int kend, bool ok, unsigned live) {
  unsigned e[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) e[r] = ld_bf16(p + (size_t)(k + r) * sk, ok && k + r < kend && (live >> r & 1u));
  return pair8(e);
}
// four consecutive n of an output row: fp32 as they are; bf16 rounded as the loaders round (pack4 is pack8's conversion), one 8-byte
// store where `full` (8-byte aligned, all four inside N), else the first `left` of them as 2-byte elements
EDTTS_DEV void store_row4(float* yp, f4 o, bool full, int left) {
  if (full) {
    stg4(yp, o);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < left) yp[r] = o[r];
  }
}
EDTTS_DEV void store_row4(__bf16* yp, f4 o, bool full, int left) {
  typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
  const edtts16::f2s pk = edtts16::pack4(o);
  if (full) {
    *reinterpret_cast<edtts16::f2s*>(yp) = pk;
  } else {
    const bf4 b = __builtin_bit_cast(bf4, pk);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < left) yp[r] = b[r];
  }
}
// one K tile of the block's 64 x 64 product from LDS buffer [X | W][64][kG16Ld]: the wave tiles of k_gen_gemm
EDTTS_DEV void mfma_tile16(const __bf16 (*t)[kGBM][kG16Ld], f4 (&acc)[2][2], int wm, int wn0, int wn1, int fq, int g) {
  const bf8 a0 = *reinterpret_cast<const bf8*>(&t[1][wn0 + fq][8 * g]), a1 = *reinterpret_cast<const bf8*>(&t[1][wn1 + fq][8 * g]);
  const bf8 b0 = *reinterpret_cast<const bf8*>(&t[0][wm + fq][8 * g]), b1 = *reinterpret_cast<const bf8*>(&t[0][wm + 16 + fq][8 * g]);
  acc[0][0] = EDTTS_MFMA16(a0, b0, acc[0][0]);
  acc[0][1] = EDTTS_MFMA16(a0, b1, acc[0][1]);
  acc[1][0] = EDTTS_MFMA16(a1, b0, acc[1][0]);
  acc[1][1] = EDTTS_MFMA16(a1, b1, acc[1][1]);
}

// k_gen_gemm's epilogue, statement for statement (that kernel keeps its own copy so that its code does not move): the accumulators
// have its layout -- acc[t][u] lane (g, fq) holds Y[m = m0 + wm + 16u + fq][n = 4g + r of weight sub-tile t] (LDS rows wn0 / wn1)
// (TY = __bf16: the stores go through store_row4; the float instantiation keeps its statements)
template <int EPI, bool DROP, typename TY = float>
EDTTS_DEV void gemm_epilogue(const GemmArgs& a, const f4 (&acc)[2][2], int m0, int n0, int wm, int wn0, int wn1, int fq, int g) {
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
      if constexpr (sizeof(TY) == 2) {
        store_row4(reinterpret_cast<__bf16*>(a.Y) + (size_t)m * a.ldy + n, o, a.vec_y && n + 3 < a.N, a.N - n);
        continue;
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
      if constexpr (sizeof(TY) == 2) {
        static_assert((EPI == EPI_BIAS && !DROP) || EPI == EPI_SWIGLU /* (returned above) */, "bf16 stores: the q|k|v, cross query, K|V and SwiGLU rows only");
        store_row4(reinterpret_cast<__bf16*>(a.Y) + (size_t)m * a.ldy + n, o, full, a.N - n);
        continue;
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

template <int EPI, bool DROP, typename TX, typename TY>
__global__ __launch_bounds__(256) void k_gen_gemm16(GemmArgs a) {
  __shared__ __attribute__((aligned(16))) __bf16 lds[2][2][kGBM][kG16Ld];  // [buffer][X | W][row][k]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fq = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * kGBM;
  const int n0 = blockIdx.y * (EPI == EPI_SWIGLU ? kGBN / 2 : kGBN);
  // loader: LDS row lr, k offsets lk .. lk + 7 of the current K tile
  const int lr = ld_k_row(tid), lk = ld_k_chunk(tid);
  int wrow;
  bool wok;
  if (EPI == EPI_SWIGLU) {  // LDS rows 0..31: value rows n0.., rows 32..63: the matching gate rows N + n0..  (as k_gen_gemm)
    const int j = n0 + (lr & 31);
    wrow = (lr < 32 ? 0 : a.N) + j;
    wok = j < a.N;
  } else {
    wrow = n0 + lr;
    wok = wrow < a.N;
  }
  const int xrow = m0 + lr;
  const bool xok = xrow < a.M;
  const TX* xp = reinterpret_cast<const TX*>(a.X) + (size_t)(xok ? xrow : 0) * a.ldx;  // (GemmArgs names the buffer; TX its elements)
  const float* wp = a.W + (size_t)(wok ? wrow : 0) * a.K;
  const int wn0 = EPI == EPI_SWIGLU ? 16 * (w & 1) : 32 * (w & 1);
  const int wn1 = EPI == EPI_SWIGLU ? wn0 + 32 : wn0 + 16;
  const int wm = 32 * (w >> 1);
  f4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = splat(0.f);
  bf8 xv, wv;
  auto load = [&](int k0) {
    xv = load8_row(xp, k0 + lk, a.K, xok, a.vec_x);
    wv = load8_row(wp, k0 + lk, a.K, wok, a.vec_w);
  };
  auto store = [&](int buf) {
    *reinterpret_cast<bf8*>(&lds[buf][0][lr][lk]) = xv;
    *reinterpret_cast<bf8*>(&lds[buf][1][lr][lk]) = wv;
  };
  load(0);
  store(0);
  __syncthreads();
  for (int k0 = 0, buf = 0; k0 < a.K; k0 += kG16K, buf ^= 1) {
    const bool more = k0 + kG16K < a.K;
    if (more) load(k0 + kG16K);
    mfma_tile16(lds[buf], acc, wm, wn0, wn1, fq, g);
    if (more) store(buf ^ 1);  // (read last by the previous tile's MFMAs, which every wave left at the barrier below)
    __syncthreads();
  }
  gemm_epilogue<EPI, DROP, TY>(a, acc, m0, n0, wm, wn0, wn1, fq, g);
}

}  // namespace edtts_gen

namespace edtts_bwd {

// k_bwd_gemm's store, statement for statement (as gemm_epilogue above)
template <int ACC>
EDTTS_DEV void bgemm_store(const BGemmArgs& a, const f4 (&acc)[2][2], int m0, int n0, int wm, int wn0, int wn1, int fq, int g) {
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

template <int ACC, bool LEN, typename TB>
__global__ __launch_bounds__(256) void k_bwd_gemm16(BGemmArgs a) {
  using namespace edtts_gen;
  __shared__ __attribute__((aligned(16))) __bf16 lds[2][2][kGBM][kG16Ld];  // [buffer][A | B][row][k]: A in X's place, B in W's
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fq = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * kGBM, n0 = blockIdx.y * kGBN;
  const int kbeg = blockIdx.z * a.kslab;
  int kend = kbeg + a.kslab < a.K ? kbeg + a.kslab : a.K;
  // loaders (see the file comment): 8 k of one row per thread, the row chosen so that neighbouring threads read neighbouring addresses
  const int alr = a.sak == 1 ? ld_k_row(tid) : ld_r_row(tid), alk = a.sak == 1 ? ld_k_chunk(tid) : ld_r_chunk(tid);
  const int blr = a.sbk == 1 ? ld_k_row(tid) : ld_r_row(tid), blk = a.sbk == 1 ? ld_k_chunk(tid) : ld_r_chunk(tid);
  bool aok = m0 + alr < a.M;
  const bool bok = n0 + blr < a.N;
  const bool len_k = LEN && a.lmode == LEN_K;
  if (LEN && a.lmode == LEN_ROWS) {
    if (!rows_any_live(a.len, a.rpb, m0, m0 + kGBM < a.M ? m0 + kGBM : a.M)) kend = kbeg;  // (block-uniform: no k-step, zeros stored)
    aok = aok && row_live(a.len, a.rpb, m0 + alr);
  }
  const float* ap = a.A + (size_t)(aok ? m0 + alr : 0) * a.sam;
  const TB* bp = reinterpret_cast<const TB*>(a.B) + (size_t)(bok ? n0 + blr : 0) * a.sbn;  // (TB = __bf16: dW_down's X^T, the tape's act)
  const int wn0 = 32 * (w & 1), wn1 = wn0 + 16, wm = 32 * (w >> 1);
  f4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = splat(0.f);
  // LEN_K: the first k-step at or behind k0 with a live row (block-uniform); a skipped step holds zero products only
  auto live_step = [&](int k0) {
    if (len_k)
      while (k0 < kend && !rows_any_live(a.len, a.rpb, k0, k0 + kG16K < kend ? k0 + kG16K : kend)) k0 += kG16K;
    return k0;
  };
  bf8 av, bv;
  auto load = [&](int k0) {
    const int ka = k0 + alk, kb = k0 + blk;
    if (len_k) {  // (never with 16-byte loads along k: the rows are strided there)
      av = gather8(ap, a.sak, ka, kend, aok, rows_live4(a.len, a.rpb, ka, kend) | rows_live4(a.len, a.rpb, ka + 4, kend) << 4);
      bv = gather8(bp, a.sbk, kb, kend, bok, rows_live4(a.len, a.rpb, kb, kend) | rows_live4(a.len, a.rpb, kb + 4, kend) << 4);
    } else {
      av = a.va ? load8_row(ap, ka, kend, aok, 1) : gather8(ap, a.sak, ka, kend, aok, 0xffu);
      bv = a.vb ? load8_row(bp, kb, kend, bok, 1) : gather8(bp, a.sbk, kb, kend, bok, 0xffu);
    }
  };
  auto store = [&](int buf) {
    *reinterpret_cast<bf8*>(&lds[buf][0][alr][alk]) = av;
    *reinterpret_cast<bf8*>(&lds[buf][1][blr][blk]) = bv;
  };
  int k0 = live_step(kbeg);
  if (k0 < kend) {
    load(k0);
    store(0);
  }
  __syncthreads();
  for (int buf = 0; k0 < kend; buf ^= 1) {
    const int kn = live_step(k0 + kG16K);
    if (kn < kend) load(kn);
    mfma_tile16(lds[buf], acc, wm, wn0, wn1, fq, g);
    if (kn < kend) store(buf ^ 1);
    __syncthreads();
    k0 = kn;
  }
  bgemm_store<ACC>(a, acc, m0, n0, wm, wn0, wn1, fq, g);
}

}  // namespace edtts_bwd

// ---- conditioning rows ---------------------------------------------------------------------------------------------------------
// launch_cond on the same switch: t_cond = W3 GELU(W1 e + b1) + b3 + step_emb and the AdaLN rows (1 + scale | shift) = proj(t_cond),
// the four kinds of product as k_bwd_gemm16 calls on the blob's transposed matrices (as the backward recomputes them), the rest
// elementwise.  e, the pre-activation and the hidden row are staged in the first 3H floats of each row's AdaLN area (L 4H floats),
// which the projections overwrite last; t_cond goes where k_cond_mlp puts it.
__global__ __launch_bounds__(256) void k_cond16_emb(CondArgs a, int rows, int ld) {
  const int H = a.H, half = H / 2;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows * H; i += gridDim.x * blockDim.x) {
    const int row = i / H, j = i - row * H;
    const float tf = a.use_host ? (float)a.t_host[row] : (float)a.t[row];
    const float arg = tf * a.freqs[j < half ? j : j - half];  // as k_cond_mlp
    a.cond[(size_t)row * ld + j] = j < half ? sinf(arg) : cosf(arg);
  }
}
// u = GELU(a1 + b1) with a1 at cond + H and u at cond + 2H of every row
__global__ __launch_bounds__(256) void k_cond16_gelu(CondArgs a, int rows, int ld) {
  const int H = a.H;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows * H; i += gridDim.x * blockDim.x) {
    const int row = i / H, j = i - row * H;
    float* p = a.cond + (size_t)row * ld + H + j;
    const float x = p[0] + a.t1b[j];
    p[0] = x;
    p[H] = 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
  }
}
// t_cond += b3 + step_emb[step_idx] (indices clamped and marked as k_cond_mlp does)
__global__ __launch_bounds__(256) void k_cond16_tcond(CondArgs a, int rows) {
  const int H = a.H;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows * H; i += gridDim.x * blockDim.x) {
    const int row = i / H, n = i - row * H;
    float acc = a.tcond[i] + a.t3b[n];
    if (a.use_host ? a.host_has_step : (a.step_idx != nullptr)) {
      long sidx = a.use_host ? (long)a.step_host[row] : (long)a.step_idx[row];
      if (sidx < 0 || sidx >= a.n_step) {
        if (n == 0) atomicOr(a.err, (unsigned)EDTTS_IDX_STEP);
        sidx = sidx < 0 ? 0 : a.n_step - 1;
      }
      acc += a.step[(size_t)sidx * H + n];
    }
    a.tcond[i] = acc;
  }
}
// the AdaLN rows' biases and the 1 + of the scale half
__global__ __launch_bounds__(256) void k_cond16_ada(CondArgs a, int rows) {
  const int H = a.H, per = a.L * 4 * H;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows * per; i += gridDim.x * blockDim.x) {
    const int c = i % per, lw = c / (2 * H), n = c - lw * 2 * H, l = lw >> 1;
    const float v = a.cond[i] + a.blob[(lw & 1 ? a.ada3b[l] : a.ada1b[l]) + n];
    a.cond[i] = n < H ? 1.0f + v : v;
  }
}
static int launch_cond16(const Layout& lo, const CondArgs& a, int rows, hipStream_t stream) {
  using TL = TrainLauncher;
  const MmStream st{stream, true};
  const int H = lo.H, cb = lo.L * 4 * H;
  const dim3 grid(GenericLauncher::grid_1d((size_t)rows * H));
  // C[rows][N] = A[rows][H] (row stride lda) WT[H][N]
  auto mm = [&](const float* A, int lda, const float* WT, int N, float* C, int ldc) {
    edtts_bwd::BGemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.B = WT; g.C = C; g.M = rows; g.N = N; g.K = H; g.sam = lda; g.sak = 1; g.sbn = 1; g.sbk = N; g.ldc = ldc;
    g.kslab = (H + 31) / 32 * 32;
    return TL::bgemm(st, g, 1, false);
  };
  hipLaunchKernelGGL(k_cond16_emb, grid, dim3(256), 0, stream, a, rows, cb);
  LAUNCH_CHECK("k_cond16_emb");
  TRY_G(mm(a.cond, cb, a.t1T, H, a.cond + H, cb));
  hipLaunchKernelGGL(k_cond16_gelu, grid, dim3(256), 0, stream, a, rows, cb);
  LAUNCH_CHECK("k_cond16_gelu");
  TRY_G(mm(a.cond + 2 * H, cb, a.t3T, H, a.tcond, H));
  hipLaunchKernelGGL(k_cond16_tcond, grid, dim3(256), 0, stream, a, rows);
  LAUNCH_CHECK("k_cond16_tcond");
  for (int l = 0; l < lo.L; ++l)
    for (int which = 0; which < 2; ++which)
      TRY_G(mm(a.tcond, H, a.blob + (which ? a.ada3T[l] : a.ada1T[l]), 2 * H, a.cond + (size_t)(2 * l + which) * 2 * H, cb));
  hipLaunchKernelGGL(k_cond16_ada, dim3(GenericLauncher::grid_1d((size_t)rows * cb)), dim3(256), 0, stream, a, rows);
  LAUNCH_CHECK("k_cond16_ada");
  return EDTTS_OK;
}
