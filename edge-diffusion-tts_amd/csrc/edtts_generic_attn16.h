// edtts_generic_attn16.h -- the generic path's attention, forward and backward, on bf16 MFMAs (included by edtts_kernels.hip after
// edtts_generic.h, edtts_generic_bwd.h, edtts_bf16.h and edtts_generic16.h).  Selected per decoder with
// EDTTS_ATTN_BF16 (Layout::ATT16): GenericLauncher::attn and TrainLauncher::attn_bwd pick these kernels or the fp32 ones, the launch
// lists stay single.  AttnArgs / AttnBwdArgs are the fp32 kernels'; nothing is stored as bf16 in global memory by these kernels.
// With EDTTS_TAPE_BF16 (Layout::TAPE16) q, k and v ARRIVE as bf16: TQ = __bf16, the loaders of those three copy
// instead of converting (bf16(bf16(x)) = bf16(x): the operand is the one formed from fp32 rows, bit for bit); dO, the log-sum-exp,
// delta and every store stay fp32, and LDS images, the walk, barriers, dropout counters and MFMAs are the same statements.
//
//   k_gen_attn16<DT, DROP, TQ>      k_gen_attn's attention: a block = four waves = 64 adjacent queries of one (utterance, head)
//   k_bwd_attn_dq16<DT, DROP, TQ>   k_bwd_attn_dq's dQ: the same block
//   k_bwd_attn_dkv16<DT, DROP, TQ>  k_bwd_attn_dkv's dK / dV: a block = 64 adjacent keys
//
// Rounding contract (include/edtts.h, EDTTS_ATTN_BF16): only MFMA operands are rounded (nearest even, v_cvt_pk_bf16_f32).
//   S = bf16(q) bf16(k)^T, * log2(e) / sqrt(d) in fp32 -- the operands are the stored values, so all three kernels form the same S up to
//   summation order (a bf16 x bf16 product is exact in fp32); mask, running maximum, exp2, l and the log-sum-exp in fp32 from the unrounded
//   probabilities; O = bf16(P~) bf16(v) / l; dP = bf16(dO) bf16(v)^T; dV = bf16(P o D)^T bf16(dO); dS = P o (D o dP - delta) in fp32;
//   dQ = bf16(dS) bf16(k) / sqrt(d); dK = bf16(dS)^T bf16(q) / sqrt(d).
//
// Walk.  The block walks 32 rows of the other side per step (keys; dK/dV: queries) over the union of its waves' bands, on a grid
// aligned to 32: step j0 runs from (first row of the block - window, clamped at 0, rounded down to 32) to the band's end or the
// utterance's count.  It depends on position, window and that utterance's counts only.  A wave skips the MFMAs of a step wholly
// outside its own band (it still stages and meets the barriers).  32 rows are one k-step of the second contraction: the two 16 x 16
// score tiles of a step leave rows {4g + r} and {16 + 4g + r} on lane (g, i), which packed pairwise are the B operand of
// v_mfma_f32_16x16x32_bf16 with k-slot 8g + 4t + r <-> row 16t + 4g + r; the A operand is staged in that slot order.
//
// LDS.  Each step's rows are loaded from global memory once per block, converted in registers and written with 16-byte stores as
//   row-major images   R[32 rows][32 KS + 16]   (KS = k-steps of head_dim): the A operand of the score-type products; lane (fq, g)
//                                                reads d = 32 ks + 8g .. + 7 of row 16t + fq as one ds_read_b128
//   transposed images  T[32 KS d][32 + 16]      row d holds the step's 32 rows in slot order: the A operand of the second contraction
// Both pitches are 2 (mod 4) sixteen-byte slots (6, 10, 14, 18; 6): the groups of lanes that a ds_read_b128 is served in -- rows
// {0-3, 12-15} of chunk g with rows 4-11 of chunk g + 1, section 26 -- land on eight distinct even and eight distinct odd slots (mod
// 16) for every such pitch, since 8 rows that differ mod 8 times 2m (m odd) differ mod 16.  The loaders' thread maps are section
// 26's: 8 neighbouring threads write 4 rows x 2 chunks.  The transposed images are gathered with scalar loads (the gather is the
// transpose; a wave's load covers 2 rows x 32 consecutive d); the row-major ones with two 16-byte loads where ld, head_dim and the
// base allow, else 8 guarded scalar loads.  Rows at or past the utterance's count and d >= head_dim are never loaded: staged as zero.
// One buffer, two barriers per step; the next step's global loads are issued before the MFMAs and land during them.
//
// Every output element is one fixed-order chain of MFMA steps: no atomics, no scratch, no split accumulation.
namespace edtts_gen {

constexpr int kA16Q = 64;     // rows a block owns: four 16-row wave tiles
constexpr int kA16TP = 48;    // pitch of a transposed image in bf16 (96 bytes)
template <int DT>
struct A16 {
  static constexpr int KS = (DT + 1) / 2;    // k-steps of 32 over head_dim (zero padded)
  static constexpr int RP = 32 * KS + 16;    // pitch of a row-major image in bf16
  static constexpr int NI = 128 * KS;        // 8-element items of one image of either kind: a multiple of the wave size
};
EDTTS_DEV bool a16_al(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// The dropout masks of a step.  Steps start at multiples of 32, so only the one-draw form of drop_attn_keys4 (key0 % 4 == 0) and the
// two-draw form of drop_attn_queries4 (q0 even) occur; these are those forms, from the same drop_attn_draw / drop_attn_field.  The
// field is extracted from the draw's words BY VALUE: drop_field selects among the members of a U4 reference, which hipcc turns into a
// dynamically indexed private copy of the draw (scratch) in these kernels.
EDTTS_DEV float a16_drop_mul(const DropArgs& d, unsigned x, unsigned y, unsigned z, unsigned w, int j) {
  const unsigned v = (j & 4) ? ((j & 2) ? w : z) : ((j & 2) ? y : x);
  return ((j & 1) ? v >> 16 : v & 0xffffu) >= d.thr ? d.scale : 0.f;
}
EDTTS_DEV f4 a16_drop_keys4(const DropArgs& d, unsigned bh, int q, int key0) {
  const U4 w = drop_attn_draw(d, bh, q, key0);
  f4 m;
#pragma unroll
  for (int r = 0; r < 4; ++r) m[r] = a16_drop_mul(d, w.x, w.y, w.z, w.w, drop_attn_field(q, key0 + r));
  return m;
}
EDTTS_DEV f4 a16_drop_queries4(const DropArgs& d, unsigned bh, int q0, int key) {
  const U4 w0 = drop_attn_draw(d, bh, q0, key), w1 = drop_attn_draw(d, bh, q0 + 2, key);
  f4 m;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    m[r] = r < 2 ? a16_drop_mul(d, w0.x, w0.y, w0.z, w0.w, drop_attn_field(q0 + r, key))
                 : a16_drop_mul(d, w1.x, w1.y, w1.z, w1.w, drop_attn_field(q0 + r, key));
  return m;
}
// item i of a row-major image -> row, first d of its 8
template <int KS>
EDTTS_DEV void a16_rm(int i, int& row, int& d0) {
  const int hi = i >> 3;
  row = ((i >> 1) & 3) + 4 * (hi / (2 * KS));
  d0 = 8 * ((i & 1) + 2 * (hi % (2 * KS)));
}
// item i of a transposed image -> d, slot group gs (slots 8 gs .. 8 gs + 7 = rows 4 gs + r and 16 + 4 gs + r)
EDTTS_DEV void a16_tr(int i, int& d, int& gs) {
  const int hi = i >> 6;
  d = 32 * (hi >> 1) + ((i & 63) >> 1);
  gs = (i & 1) + 2 * (hi & 1);
}
// rows r0 + {4 gs + r, 16 + 4 gs + r} of column d (base points at row 0, column 0 of the head) -> the 8 slots of group gs
EDTTS_DEV bf8 a16_gather(const float* base, int ld, int r0, int rend, int d, int DH, int gs) {
  f4 lo, hi;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ra = r0 + 4 * gs + r, rb = ra + 16;
    lo[r] = (d < DH && ra < rend) ? base[(size_t)ra * ld + d] : 0.f;
    hi[r] = (d < DH && rb < rend) ? base[(size_t)rb * ld + d] : 0.f;
  }
  return edtts16::pack8(lo, hi);
}
EDTTS_DEV bf8 a16_row(const float* base, int ld, int row, int rend, int d0, int DH, int vec) {
  const bool ok = row < rend;
  return load8_row(base + (size_t)(ok ? row : 0) * ld, d0, DH, ok, vec);
}
// The same two loaders for q, k, v rows that hold bf16 already (TQ = __bf16, Layout::TAPE16): the stored value IS the operand, so
// nothing is converted.  vec: ld % 8 == 0, head_dim % 8 == 0 and a 16-byte aligned base -- one 16-byte load of eight elements.
EDTTS_DEV bf8 a16_gather(const __bf16* base, int ld, int r0, int rend, int d, int DH, int gs) {
  unsigned e[8];  // (each load into a register of its own, paired afterwards: ld_bf16 / pair8, edtts_generic16.h)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ra = r0 + 4 * gs + r, rb = ra + 16;
    e[r] = ld_bf16(base + (size_t)ra * ld + d, d < DH && ra < rend);
    e[4 + r] = ld_bf16(base + (size_t)rb * ld + d, d < DH && rb < rend);
  }
  return pair8(e);
}
EDTTS_DEV bf8 a16_row(const __bf16* base, int ld, int row, int rend, int d0, int DH, int vec) {
  const bool ok = row < rend;
  return load8_row(base + (size_t)(ok ? row : 0) * ld, d0, DH, ok, vec);
}
// ld | head_dim must be a multiple of this + 1 for the 16-byte loads of a row of T
template <typename T>
constexpr int a16_vm() { return sizeof(T) == 2 ? 7 : 3; }

template <int DT, bool DROP, typename TQ>
__global__ __launch_bounds__(256) void k_gen_attn16(AttnArgs a) {
  constexpr int KS = A16<DT>::KS, RP = A16<DT>::RP, NI = A16<DT>::NI;
  __shared__ __attribute__((aligned(16))) __bf16 Ks[32][RP];          // K rows of the step
  __shared__ __attribute__((aligned(16))) __bf16 Vt[32 * KS][kA16TP];  // V^T of the step, keys in slot order
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fq = lane & 15, g = lane >> 4;
  const int Q0 = blockIdx.x * kA16Q, hd = blockIdx.y, b = blockIdx.z;
  // Per-utterance lengths, as k_gen_attn: keys past the count are never read, a tile of queries wholly past its count stores nothing.
  const int Tk = utt_len(a.k_len, b, a.Tk, a.k_dbl), Tqb = utt_len(a.q_len, b, a.Tq, a.q_dbl);
  if (Q0 >= Tqb) return;  // (the whole block: no barrier is left waiting)
  const int q0 = Q0 + 16 * w, qi = q0 + fq;
  const bool wlive = q0 < Tqb;  // wave-uniform
  const int vq = ((a.ldq | a.DH) & a16_vm<TQ>()) == 0 && a16_al(a.q), vkv = ((a.ldkv | a.DH) & a16_vm<TQ>()) == 0 && a16_al(a.k) && a16_al(a.v);
  const TQ* qrow = reinterpret_cast<const TQ*>(a.q) + (size_t)(b * a.Tq + (qi < Tqb ? qi : 0)) * a.ldq + hd * a.DH;
  bf8 qb[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qb[ks] = load8_row(qrow, 32 * ks + 8 * g, a.DH, qi < Tqb, vq);
  f4 acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) acc[t] = splat(0.f);
  float m = -1e30f, l = 0.f;
  int lo = 0, hi = Tk;
  if (a.window >= 0) {
    lo = (Q0 - a.window > 0 ? Q0 - a.window : 0) & ~31;
    const int e = Q0 + kA16Q + a.window;
    hi = e < Tk ? e : Tk;
  }
  const TQ* kb = reinterpret_cast<const TQ*>(a.k) + (size_t)b * a.Tk * a.ldkv + hd * a.DH;
  const TQ* vb = reinterpret_cast<const TQ*>(a.v) + (size_t)b * a.Tk * a.ldkv + hd * a.DH;
  bf8 st[KS];  // this thread's items of the next step: [0, NI) K row-major, [NI, 2 NI) V^T
  auto load = [&](int j0) {
#pragma unroll
    for (int it = 0; it < KS; ++it) {
      const int item = tid + 256 * it;
      if (item < NI) {
        int row, d0;
        a16_rm<KS>(item, row, d0);
        st[it] = a16_row(kb, a.ldkv, j0 + row, hi, d0, a.DH, vkv);
      } else {
        int d, gs;
        a16_tr(item - NI, d, gs);
        st[it] = a16_gather(vb, a.ldkv, j0, hi, d, a.DH, gs);
      }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int it = 0; it < KS; ++it) {
      const int item = tid + 256 * it;
      if (item < NI) {
        int row, d0;
        a16_rm<KS>(item, row, d0);
        *reinterpret_cast<bf8*>(&Ks[row][d0]) = st[it];
      } else {
        int d, gs;
        a16_tr(item - NI, d, gs);
        *reinterpret_cast<bf8*>(&Vt[d][8 * gs]) = st[it];
      }
    }
  };
  if (lo < hi) load(lo);
  const DropArgs dr = DROP ? drop_live(a.dr) : DropArgs{};
  for (int j0 = lo; j0 < hi; j0 += 32) {
    __syncthreads();  // every wave is done reading the previous step
    store();
    __syncthreads();
    if (j0 + 32 < hi) load(j0 + 32);
    // a step wholly outside this wave's band (or a wave of padding queries): no MFMA
    if (!wlive || (a.window >= 0 && (j0 > q0 + 15 + a.window || j0 + 31 < q0 - a.window))) continue;
    f4 sc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      sc[t] = splat(0.f);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) sc[t] = EDTTS_MFMA16(*reinterpret_cast<const bf8*>(&Ks[16 * t + fq][32 * ks + 8 * g]), qb[ks], sc[t]);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = j0 + 16 * t + 4 * g + r;
        const bool ok = key < hi && (a.window < 0 || (key - qi <= a.window && qi - key <= a.window));
        sc[t][r] = ok ? sc[t][r] * a.scale : -INFINITY;
        mx = fmaxf(mx, sc[t][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);
    const float alpha = exp2f(m - mn);
    f4 p[2];
    float ps = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[t][r] = exp2f(sc[t][r] - mn);
        ps += p[t][r];
      }
    ps += __shfl_xor(ps, 16);
    ps += __shfl_xor(ps, 32);
    l = l * alpha + ps;  // (from the unrounded probabilities, as the backward recomputes them)
    m = mn;
#pragma unroll
    for (int t = 0; t < DT; ++t) acc[t] *= alpha;
    if (DROP) {  // (steps start at multiples of 32: one draw per four keys)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const f4 dm = a16_drop_keys4(dr, (unsigned)(b * gridDim.y + hd), qi, j0 + 16 * t + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) p[t][r] *= dm[r];
      }
    }
    const bf8 pb = edtts16::pack8(p[0], p[1]);
#pragma unroll
    for (int t = 0; t < DT; ++t) acc[t] = EDTTS_MFMA16(*reinterpret_cast<const bf8*>(&Vt[16 * t + fq][8 * g]), pb, acc[t]);
  }
  if (!wlive || qi >= a.Tq) return;
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

}  // namespace edtts_gen

namespace edtts_bwd {
using edtts_gen::A16;
using edtts_gen::a16_al;
using edtts_gen::a16_drop_keys4;
using edtts_gen::a16_drop_queries4;
using edtts_gen::a16_gather;
using edtts_gen::a16_rm;
using edtts_gen::a16_row;
using edtts_gen::a16_tr;
using edtts_gen::a16_vm;
using edtts_gen::kA16Q;
using edtts_gen::kA16TP;
using edtts_gen::load8_row;

// The block of k_gen_attn16: S^T = K Q^T and dP^T = V dO^T tiles hold (key 16t + 4g + r, query fq) on lane (g, fq); the packed dS^T
// is the B operand of dQ^T += K^T dS^T.  Staged per step: K and V row-major, K^T in slot order.
template <int DT, bool DROP, typename TQ>
__global__ __launch_bounds__(256) void k_bwd_attn_dq16(AttnBwdArgs a) {
  constexpr int KS = A16<DT>::KS, RP = A16<DT>::RP, NI = A16<DT>::NI, NIT = (3 * NI + 255) / 256;
  __shared__ __attribute__((aligned(16))) __bf16 Ks[32][RP];
  __shared__ __attribute__((aligned(16))) __bf16 Vs[32][RP];
  __shared__ __attribute__((aligned(16))) __bf16 Kt[32 * KS][kA16TP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fq = lane & 15, g = lane >> 4;
  const int Q0 = blockIdx.x * kA16Q, hd = blockIdx.y, b = blockIdx.z;
  const int q0 = Q0 + 16 * w, qi = q0 + fq;
  // Per-utterance lengths, as k_bwd_attn_dq: nothing past the counts is loaded, the dq rows of padding queries are stored as zeros,
  // and a block wholly past the count does only that.
  const int Tqb = utt_len(a.q_len, b, a.Tq), Tkb = utt_len(a.k_len, b, a.Tk);
  if (Q0 >= Tqb) {
    if (qi < a.Tq) {
      float* zrow = a.dq + ((size_t)b * a.Tq + qi) * a.lddq + hd * a.DH;
      for (int d = g; d < a.DH; d += 4) zrow[d] = 0.f;
    }
    return;
  }
  const bool wlive = q0 < Tqb, qok = qi < Tqb;
  const int vq = ((a.ldq | a.DH) & a16_vm<TQ>()) == 0 && a16_al(a.q), vo = ((a.ldo | a.DH) & 3) == 0 && a16_al(a.dO);
  const int vkv = ((a.ldkv | a.DH) & a16_vm<TQ>()) == 0 && a16_al(a.k) && a16_al(a.v);
  const size_t qr = (size_t)b * a.Tq + (qok ? qi : 0);
  const TQ* qrow = reinterpret_cast<const TQ*>(a.q) + qr * a.ldq + hd * a.DH;
  const float* drow = a.dO + qr * a.ldo + hd * a.DH;
  bf8 qb[KS], dob[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qb[ks] = load8_row(qrow, 32 * ks + 8 * g, a.DH, qok, vq);
    dob[ks] = load8_row(drow, 32 * ks + 8 * g, a.DH, qok, vo);
  }
  const size_t si = ((size_t)b * gridDim.y + hd) * a.Tq + (qok ? qi : 0);
  const float ls = a.lse[si], dl = a.delta[si];
  f4 acc[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) acc[t] = splat(0.f);
  int lo = 0, hi = Tkb;
  if (a.window >= 0) {
    lo = (Q0 - a.window > 0 ? Q0 - a.window : 0) & ~31;
    const int e = Q0 + kA16Q + a.window;
    hi = e < Tkb ? e : Tkb;
  }
  const TQ* kb = reinterpret_cast<const TQ*>(a.k) + (size_t)b * a.Tk * a.ldkv + hd * a.DH;
  const TQ* vb = reinterpret_cast<const TQ*>(a.v) + (size_t)b * a.Tk * a.ldkv + hd * a.DH;
  bf8 st[NIT];  // items [0, NI) K, [NI, 2 NI) V, [2 NI, 3 NI) K^T
  auto load = [&](int j0) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int item = tid + 256 * it;
      if (item < 2 * NI) {
        int row, d0;
        a16_rm<KS>(item < NI ? item : item - NI, row, d0);
        st[it] = a16_row(item < NI ? kb : vb, a.ldkv, j0 + row, hi, d0, a.DH, vkv);
      } else if (item < 3 * NI) {
        int d, gs;
        a16_tr(item - 2 * NI, d, gs);
        st[it] = a16_gather(kb, a.ldkv, j0, hi, d, a.DH, gs);
      }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int item = tid + 256 * it;
      if (item < 2 * NI) {
        int row, d0;
        a16_rm<KS>(item < NI ? item : item - NI, row, d0);
        *reinterpret_cast<bf8*>(item < NI ? &Ks[row][d0] : &Vs[row][d0]) = st[it];
      } else if (item < 3 * NI) {
        int d, gs;
        a16_tr(item - 2 * NI, d, gs);
        *reinterpret_cast<bf8*>(&Kt[d][8 * gs]) = st[it];
      }
    }
  };
  if (lo < hi) load(lo);
  const DropArgs dr = DROP ? drop_live(a.dr) : DropArgs{};
  for (int j0 = lo; j0 < hi; j0 += 32) {
    __syncthreads();
    store();
    __syncthreads();
    if (j0 + 32 < hi) load(j0 + 32);
    if (!wlive || (a.window >= 0 && (j0 > q0 + 15 + a.window || j0 + 31 < q0 - a.window))) continue;
    f4 sc[2], dp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      sc[t] = dp[t] = splat(0.f);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        sc[t] = EDTTS_MFMA16(*reinterpret_cast<const bf8*>(&Ks[16 * t + fq][32 * ks + 8 * g]), qb[ks], sc[t]);
        dp[t] = EDTTS_MFMA16(*reinterpret_cast<const bf8*>(&Vs[16 * t + fq][32 * ks + 8 * g]), dob[ks], dp[t]);
      }
    }
    f4 ds[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (DROP) {
        const f4 dm = a16_drop_keys4(dr, (unsigned)(b * gridDim.y + hd), qi, j0 + 16 * t + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) dp[t][r] *= dm[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = j0 + 16 * t + 4 * g + r;
        const bool ok = qok && key < hi && (a.window < 0 || (key - qi <= a.window && qi - key <= a.window));
        const float p = ok ? exp2f(sc[t][r] * a.scale - ls) : 0.f;
        ds[t][r] = p * (dp[t][r] - dl);
      }
    }
    const bf8 dsb = edtts16::pack8(ds[0], ds[1]);
#pragma unroll
    for (int t = 0; t < DT; ++t) acc[t] = EDTTS_MFMA16(*reinterpret_cast<const bf8*>(&Kt[16 * t + fq][8 * g]), dsb, acc[t]);
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

// A block = 64 adjacent keys of one (utterance, head), a wave = 16 of them.  S = Q K^T and dP = dO V^T tiles hold (query 16t + 4g + r,
// key fq) on lane (g, fq); the packed P o D and dS are the B operands of dV^T += dO^T (P o D) and dK^T += Q^T dS.  Staged per step of 32
// queries: Q and dO row-major, Q^T and dO^T in slot order, and the queries' log-sum-exp and delta.
template <int DT, bool DROP, typename TQ>
__global__ __launch_bounds__(256) void k_bwd_attn_dkv16(AttnBwdArgs a) {
  constexpr int KS = A16<DT>::KS, RP = A16<DT>::RP, NI = A16<DT>::NI, NIT = 2 * KS;  // 4 NI items over 256 threads
  __shared__ __attribute__((aligned(16))) __bf16 Qs[32][RP];
  __shared__ __attribute__((aligned(16))) __bf16 Ds[32][RP];
  __shared__ __attribute__((aligned(16))) __bf16 Qt[32 * KS][kA16TP];
  __shared__ __attribute__((aligned(16))) __bf16 Dt[32 * KS][kA16TP];
  __shared__ __attribute__((aligned(16))) float stat[2][32];  // log-sum-exp | delta of the step's queries
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fq = lane & 15, g = lane >> 4;
  const int K0 = blockIdx.x * kA16Q, hd = blockIdx.y, b = blockIdx.z;
  const int k0 = K0 + 16 * w, kj = k0 + fq;
  // Per-utterance lengths, as k_bwd_attn_dkv: the query walk ends at the utterance's query count, the dk / dv rows of padding keys
  // are stored as zeros, and a block wholly past the key count does only that.
  const int Tqb = utt_len(a.q_len, b, a.Tq), Tkb = utt_len(a.k_len, b, a.Tk);
  if (K0 >= Tkb) {
    if (kj < a.Tk) {
      float* zk = a.dk + ((size_t)b * a.Tk + kj) * a.lddkv + hd * a.DH;
      float* zv = a.dv + ((size_t)b * a.Tk + kj) * a.lddkv + hd * a.DH;
      for (int d = g; d < a.DH; d += 4) zk[d] = zv[d] = 0.f;
    }
    return;
  }
  const bool wlive = k0 < Tkb, kok = kj < Tkb;
  const int vq = ((a.ldq | a.DH) & a16_vm<TQ>()) == 0 && a16_al(a.q), vo = ((a.ldo | a.DH) & 3) == 0 && a16_al(a.dO);
  const int vkv = ((a.ldkv | a.DH) & a16_vm<TQ>()) == 0 && a16_al(a.k) && a16_al(a.v);
  const size_t kr = (size_t)b * a.Tk + (kok ? kj : 0);
  const TQ* krow = reinterpret_cast<const TQ*>(a.k) + kr * a.ldkv + hd * a.DH;
  const TQ* vrow = reinterpret_cast<const TQ*>(a.v) + kr * a.ldkv + hd * a.DH;
  bf8 kb[KS], vb[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kb[ks] = load8_row(krow, 32 * ks + 8 * g, a.DH, kok, vkv);
    vb[ks] = load8_row(vrow, 32 * ks + 8 * g, a.DH, kok, vkv);
  }
  f4 ak[DT], av[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) ak[t] = av[t] = splat(0.f);
  int lo = 0, hi = Tqb;
  if (a.window >= 0) {
    lo = (K0 - a.window > 0 ? K0 - a.window : 0) & ~31;
    const int e = K0 + kA16Q + a.window;
    hi = e < Tqb ? e : Tqb;
  }
  const TQ* qb = reinterpret_cast<const TQ*>(a.q) + (size_t)b * a.Tq * a.ldq + hd * a.DH;
  const float* db = a.dO + (size_t)b * a.Tq * a.ldo + hd * a.DH;
  const float* lb = a.lse + ((size_t)b * gridDim.y + hd) * a.Tq;
  const float* eb = a.delta + ((size_t)b * gridDim.y + hd) * a.Tq;
  bf8 st[NIT];  // items [0, NI) Q, [NI, 2 NI) dO, [2 NI, 3 NI) Q^T, [3 NI, 4 NI) dO^T
  float sv = 0.f;
  auto load = [&](int i0) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int item = tid + 256 * it;
      if (item < 2 * NI) {
        int row, d0;
        a16_rm<KS>(item < NI ? item : item - NI, row, d0);
        st[it] = item < NI ? a16_row(qb, a.ldq, i0 + row, hi, d0, a.DH, vq) : a16_row(db, a.ldo, i0 + row, hi, d0, a.DH, vo);
      } else {
        int d, gs;
        a16_tr(item < 3 * NI ? item - 2 * NI : item - 3 * NI, d, gs);
        st[it] = item < 3 * NI ? a16_gather(qb, a.ldq, i0, hi, d, a.DH, gs) : a16_gather(db, a.ldo, i0, hi, d, a.DH, gs);
      }
    }
    if (tid < 64) {
      const int qq = i0 + (tid & 31);
      sv = qq < hi ? (tid < 32 ? lb[qq] : eb[qq]) : 0.f;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int item = tid + 256 * it;
      if (item < 2 * NI) {
        int row, d0;
        a16_rm<KS>(item < NI ? item : item - NI, row, d0);
        *reinterpret_cast<bf8*>(item < NI ? &Qs[row][d0] : &Ds[row][d0]) = st[it];
      } else {
        int d, gs;
        a16_tr(item < 3 * NI ? item - 2 * NI : item - 3 * NI, d, gs);
        *reinterpret_cast<bf8*>(item < 3 * NI ? &Qt[d][8 * gs] : &Dt[d][8 * gs]) = st[it];
      }
    }
    if (tid < 64) stat[tid >> 5][tid & 31] = sv;
  };
  if (lo < hi) load(lo);
  const DropArgs dr = DROP ? drop_live(a.dr) : DropArgs{};
  for (int i0 = lo; i0 < hi; i0 += 32) {
    __syncthreads();
    store();
    __syncthreads();
    if (i0 + 32 < hi) load(i0 + 32);
    if (!wlive || (a.window >= 0 && (i0 > k0 + 15 + a.window || i0 + 31 < k0 - a.window))) continue;
    f4 sc[2], dp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      sc[t] = dp[t] = splat(0.f);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        sc[t] = EDTTS_MFMA16(*reinterpret_cast<const bf8*>(&Qs[16 * t + fq][32 * ks + 8 * g]), kb[ks], sc[t]);
        dp[t] = EDTTS_MFMA16(*reinterpret_cast<const bf8*>(&Ds[16 * t + fq][32 * ks + 8 * g]), vb[ks], dp[t]);
      }
    }
    f4 p[2], ds[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f4 dm;
      if (DROP) {  // (steps start at multiples of 32: even)
        dm = a16_drop_queries4(dr, (unsigned)(b * gridDim.y + hd), i0 + 16 * t + 4 * g, kj);
#pragma unroll
        for (int r = 0; r < 4; ++r) dp[t][r] *= dm[r];
      }
      const f4 lsv = *reinterpret_cast<const f4*>(&stat[0][16 * t + 4 * g]), dlv = *reinterpret_cast<const f4*>(&stat[1][16 * t + 4 * g]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qq = i0 + 16 * t + 4 * g + r;
        const bool ok = kok && qq < hi && (a.window < 0 || (kj - qq <= a.window && qq - kj <= a.window));
        p[t][r] = ok ? exp2f(sc[t][r] * a.scale - lsv[r]) : 0.f;
        ds[t][r] = p[t][r] * (dp[t][r] - dlv[r]);
      }
      if (DROP) {
#pragma unroll
        for (int r = 0; r < 4; ++r) p[t][r] *= dm[r];
      }
    }
    const bf8 pb = edtts16::pack8(p[0], p[1]), dsb = edtts16::pack8(ds[0], ds[1]);
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      av[t] = EDTTS_MFMA16(*reinterpret_cast<const bf8*>(&Dt[16 * t + fq][8 * g]), pb, av[t]);
      ak[t] = EDTTS_MFMA16(*reinterpret_cast<const bf8*>(&Qt[16 * t + fq][8 * g]), dsb, ak[t]);
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

}  // namespace edtts_bwd
