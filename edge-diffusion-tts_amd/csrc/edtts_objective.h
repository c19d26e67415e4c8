// edtts_objective.h -- the training objective between the decoder's prediction and the optimiser (included by edtts_kernels.hip;
// DESIGN.md section 25): normalize_mel, q_sample on Philox noise, the v / eps targets, F.mse_loss and its gradient, the distillation
// and consistency losses (training/consistency.py:60-122) and the logging metrics of train_v2.py:149-154.
//
// A row of [T][M] is walked as quads of 4 consecutive elements; a block of kObjThreads threads owns one chunk of kObjChunk elements
// of one row, thread i the quads i, i + kObjThreads, ...  The float4 path (every pointer 16-byte aligned, every row stride a multiple
// of 4) loads and stores a wholly live quad as one vector; the per-element path walks the same quads element by element.  Both go
// through the same per-element helpers in the same order, so they give the same bits, sums included.
//
//   k_obj_stats    one block per (row, 64 mel bins): mean and unbiased std over the row's live frames.  fp64, two passes; wave w
//                  sums frames w, w + 16, ... in ascending order, the sixteen waves are added in wave order through LDS
//   k_obj_prepare  mel -> x_t (and mel_n, noise, target where asked for); 0 past a row's length
//   k_obj_loss     regenerates mel_n, noise, x_t and the target through the device functions k_obj_prepare uses, reads the
//                  prediction(s), writes the unit gradient (d loss / d pred for an upstream gradient of 1; exactly 0 past the
//                  lengths) and kObjSums partial sums per (row, chunk): per thread in fp32 in quad order, then fp64: lanes by
//                  __shfl_xor, the four waves in wave order through LDS
//   k_obj_finish   one block: per row the chunks in ascending order, then the rows in ascending order, in fp64 -> loss, terms,
//                  x0_mse, x0_cos
//   k_obj_scale    d_pred = unit * grad_out[0] (grad_out read on the device)
// No float atomics, no inline assembly, no scratch memory.  Nothing past a row's length is ever loaded.
namespace edtts_obj {

constexpr int kObjThreads = 256;
constexpr int kObjPer = 4;                             // quads per thread and chunk
constexpr int kObjChunk = kObjThreads * kObjPer * 4;   // elements per (row, chunk) block
constexpr int kObjSums = 8;                            // doubles per (row, chunk): 3 loss terms, x0 mse, x0.mel_n, |x0|^2, |mel_n|^2, 0
constexpr unsigned kObjNoiseStream = 0x54;             // include/edtts.h, "Philox stream ids": training q_sample noise

struct ObjArgs {  // the prepared batch: what k_obj_prepare and k_obj_loss rebuild mel_n, noise and x_t from
  const float* mel;    // [B][T][M]
  int B, T, M;
  const int64_t* lengths;  // [B] or NULL
  const int64_t* t;        // [B]
  const float* tables;     // [4][n_table]: sqrt_alpha_bar | sqrt_one_minus_alpha_bar | sqrt_recip_alpha_bar | sqrt_recip_alpha_bar_minus_one
  int n_table;
  const float* mean;   // [B][M] or NULL (mel is already normalised)
  const float* stdv;
  const unsigned long long* seeds;  // [B] or NULL
  const float* noise;               // [B][T][M] or NULL (then seeds)
};

struct ObjCoef {
  float sab, s1m, sra, srm1;
};
struct ObjRow {
  const float* mel;
  const float* noise;
  const float* mean;
  const float* stdv;
  unsigned long long seed;
  ObjCoef k;
  int n_live;  // live elements of the row
  int M;
  bool vec;
};
struct ObjQuad {
  f4 mel_n, noise, x_t;
};

EDTTS_DEV int obj_frames(const ObjArgs& a, int b, int cap) {  // live frames of row b: lengths[b] clamped into [1, T], at most cap
  long long v = a.lengths ? a.lengths[b] : a.T;
  v = v < 1 ? 1 : (v > a.T ? a.T : v);
  return v < cap ? (int)v : cap;
}
EDTTS_DEV ObjCoef obj_coef(const ObjArgs& a, const int64_t* t, int b) {
  long long i = t[b];
  i = i < 0 ? 0 : (i >= a.n_table ? a.n_table - 1 : i);
  return ObjCoef{a.tables[i], a.tables[a.n_table + i], a.tables[2 * (size_t)a.n_table + i], a.tables[3 * (size_t)a.n_table + i]};
}
EDTTS_DEV ObjRow obj_row(const ObjArgs& a, int b, int cap, bool vec) {
  ObjRow r;
  const size_t base = (size_t)b * a.T * a.M;
  r.mel = a.mel + base;
  r.noise = a.noise ? a.noise + base : nullptr;
  r.mean = a.mean ? a.mean + (size_t)b * a.M : nullptr;
  r.stdv = a.mean ? a.stdv + (size_t)b * a.M : nullptr;
  r.seed = a.noise ? 0ull : a.seeds[b];
  r.k = obj_coef(a, a.t, b);
  r.n_live = obj_frames(a, b, cap) * a.M;
  r.M = a.M;
  r.vec = vec;
  return r;
}

// elements e0 .. e0 + 3 of a row with n_live live elements; a dead element is not loaded and reads as 0
EDTTS_DEV f4 obj_load4(const float* row, int e0, int n_live, bool vec) {
  if (vec && e0 + 4 <= n_live) return ldg4(row + e0);
  f4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (e0 + k < n_live) v[k] = row[e0 + k];
  return v;
}
// ... and of a row of n_row elements in all (e0 < n_row)
EDTTS_DEV void obj_store4(float* row, int e0, int n_row, bool vec, f4 v) {
  if (vec) {
    stg4(row + e0, v);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (e0 + k < n_row) row[e0 + k] = v[k];
}

// the reference's expressions, one rounding per operation (no fma contraction)
EDTTS_DEV float obj_norm(float x, float mu, float sd) {  // normalize_mel: (mel - mean) / std
#pragma clang fp contract(off)
  float d = x - mu;
  return d / sd;
}
EDTTS_DEV float obj_vtarget(float x0, float nz, float sab, float s1m) {  // get_v_target: sab * noise - s1m * x0
#pragma clang fp contract(off)
  float a = sab * nz;
  float b = s1m * x0;
  return a - b;
}
EDTTS_DEV float obj_x0(float xt, float p, float c0, float c1) {  // predict_x0_from_v (sab, s1m) / predict_x0_from_eps (sra, srm1)
#pragma clang fp contract(off)
  float a = c0 * xt;
  float b = c1 * p;
  return a - b;
}

// mel_n, noise and x_t of quad e0 (a multiple of 4, e0 < n_live); dead elements are 0
EDTTS_DEV ObjQuad obj_quad(const ObjRow& r, int e0) {
  ObjQuad q;
  const f4 x = obj_load4(r.mel, e0, r.n_live, r.vec);
  const f4 nz = r.noise ? obj_load4(r.noise, e0, r.n_live, r.vec) : philox_normal4(r.seed, kObjNoiseStream, (unsigned long long)(e0 >> 2));
  int m = e0 % r.M;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool live = e0 + k < r.n_live;
    float xn = 0.f, z = 0.f, xt = 0.f;
    if (live) {
      xn = r.mean ? obj_norm(x[k], r.mean[m], r.stdv[m]) : x[k];
      z = nz[k];
      xt = qsample_elem(xn, r.k.sab, z, r.k.s1m);
    }
    q.mel_n[k] = xn;
    q.noise[k] = z;
    q.x_t[k] = xt;
    m = m + 1 == r.M ? 0 : m + 1;
  }
  return q;
}

constexpr int kObjStatWaves = 16;  // (128 frames a wave at 4 waves left B x 2 blocks waiting on latency: 46 us at 64 x 512 x 80)
__global__ __launch_bounds__(64 * kObjStatWaves) void k_obj_stats(ObjArgs a, float* __restrict__ mean, float* __restrict__ stdv) {
  __shared__ double part[kObjStatWaves][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y;
  const int m = blockIdx.x * 64 + lane;
  const int n = obj_frames(a, b, a.T);
  const float* row = a.mel + (size_t)b * a.T * a.M;
  const bool on = m < a.M;
  double s = 0.0;
  if (on) {
#pragma unroll 4
    for (int f = w; f < n; f += kObjStatWaves) s += (double)row[(size_t)f * a.M + m];
  }
  part[w][lane] = s;
  __syncthreads();
  double mu = part[0][lane];
  for (int k = 1; k < kObjStatWaves; ++k) mu += part[k][lane];
  mu /= (double)n;
  __syncthreads();
  double q = 0.0;
  if (on) {
#pragma unroll 4
    for (int f = w; f < n; f += kObjStatWaves) {
      const double d = (double)row[(size_t)f * a.M + m] - mu;
      q += d * d;
    }
  }
  part[w][lane] = q;
  __syncthreads();
  if (w != 0 || !on) return;
  double m2 = part[0][lane];
  for (int k = 1; k < kObjStatWaves; ++k) m2 += part[k][lane];
  float sd = __builtin_nanf("");  // torch.std of one value: 0 / 0
  if (n >= 2) sd = fmaxf((float)sqrt(m2 / (double)(n - 1)), 1e-5f);
  mean[(size_t)b * a.M + m] = (float)mu;
  stdv[(size_t)b * a.M + m] = sd;
}

__global__ __launch_bounds__(kObjThreads) void k_obj_prepare(ObjArgs a, int kind, int vec, float* __restrict__ x_t, float* __restrict__ mel_n,
                                                             float* __restrict__ noise_out, float* __restrict__ target) {
  const int b = blockIdx.y, n_row = a.T * a.M;
  const ObjRow r = obj_row(a, b, a.T, vec != 0);
  const size_t base = (size_t)b * n_row;
#pragma unroll
  for (int j = 0; j < kObjPer; ++j) {
    const int e0 = blockIdx.x * kObjChunk + 4 * ((int)threadIdx.x + j * kObjThreads);
    if (e0 >= n_row) break;
    ObjQuad q;
    q.mel_n = q.noise = q.x_t = f4{0.f, 0.f, 0.f, 0.f};
    if (e0 < r.n_live) q = obj_quad(r, e0);
    obj_store4(x_t + base, e0, n_row, r.vec, q.x_t);
    if (mel_n) obj_store4(mel_n + base, e0, n_row, r.vec, q.mel_n);
    if (noise_out) obj_store4(noise_out + base, e0, n_row, r.vec, q.noise);
    if (target) {
      f4 tg = q.noise;  // EDTTS_OBJ_EPS
      if (kind != EDTTS_OBJ_EPS) {
#pragma unroll
        for (int k = 0; k < 4; ++k) tg[k] = obj_vtarget(q.mel_n[k], q.noise[k], r.k.sab, r.k.s1m);  // (a dead element: 0 - 0)
      }
      obj_store4(target + base, e0, n_row, r.vec, tg);
    }
  }
}

struct ObjLossArgs {
  ObjArgs a;
  int kind;
  const float* pred;   // [B][T_pred][M]
  int T_pred;
  const float* pred2;  // the teacher's prediction (DISTILL) or the second prediction (CONSISTENCY) [B][T_pred2][M], else NULL
  int T_pred2;
  const int64_t* t2;   // CONSISTENCY: the second prediction's timesteps [B]
  float* unit;         // [B][T_pred][M] or NULL
  float* unit2;        // CONSISTENCY: [B][T_pred2][M] or NULL
  double* partial;     // [B][chunks][kObjSums]
  int vec;
};

EDTTS_DEV int obj_tm(const ObjLossArgs& L) {  // the reference's "align sequence lengths"
  int tm = L.a.T < L.T_pred ? L.a.T : L.T_pred;
  if (L.pred2 && L.T_pred2 < tm) tm = L.T_pred2;
  return tm;
}

__global__ __launch_bounds__(kObjThreads) void k_obj_loss(ObjLossArgs L) {
  __shared__ double wsum[kObjThreads / 64][kObjSums];
  __shared__ float s_norm;
  const ObjArgs& a = L.a;
  const int tid = threadIdx.x, b = blockIdx.y, c = blockIdx.x;
  const int tm = obj_tm(L);
  if (tid < 64) {  // live frames of the batch (integers: any order)
    int n = 0;
    if (a.lengths) {
      for (int i = tid; i < a.B; i += 64) n += obj_frames(a, i, tm);
      for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o);
    } else {
      n = a.B * tm;
    }
    if (tid == 0) s_norm = (float)(2.0 / ((double)n * (double)a.M));  // mse_loss's backward: 2 / numel, rounded to fp32
  }
  __syncthreads();
  const float norm = s_norm, half_norm = 0.5f * s_norm;
  const bool vec = L.vec != 0;
  const ObjRow r = obj_row(a, b, tm, vec);
  ObjCoef k2 = r.k;
  if (L.kind == EDTTS_OBJ_CONSISTENCY) k2 = obj_coef(a, L.t2, b);
  const int n_row1 = L.T_pred * a.M, n_row2 = L.T_pred2 * a.M;
  const float* p1 = L.pred + (size_t)b * n_row1;
  const float* p2 = L.pred2 ? L.pred2 + (size_t)b * n_row2 : nullptr;
  float* u1 = L.unit ? L.unit + (size_t)b * n_row1 : nullptr;
  float* u2 = L.unit2 ? L.unit2 + (size_t)b * n_row2 : nullptr;
  float s[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < kObjPer; ++j) {
    const int e0 = c * kObjChunk + 4 * (tid + j * kObjThreads);
    f4 g1 = {0.f, 0.f, 0.f, 0.f}, g2 = {0.f, 0.f, 0.f, 0.f};
    if (e0 < r.n_live) {
      const ObjQuad q = obj_quad(r, e0);
      const f4 v1 = obj_load4(p1, e0, r.n_live, vec);
      f4 v2 = {0.f, 0.f, 0.f, 0.f};
      if (p2) v2 = obj_load4(p2, e0, r.n_live, vec);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (e0 + k >= r.n_live) continue;
        const float xn = q.mel_n[k], nz = q.noise[k], xt = q.x_t[k];
        float x0;
        if (L.kind == EDTTS_OBJ_V || L.kind == EDTTS_OBJ_EPS) {
          const bool v = L.kind == EDTTS_OBJ_V;
          const float d = v1[k] - (v ? obj_vtarget(xn, nz, r.k.sab, r.k.s1m) : nz);
          s[0] += d * d;
          g1[k] = norm * d;
          x0 = v ? obj_x0(xt, v1[k], r.k.sab, r.k.s1m) : obj_x0(xt, v1[k], r.k.sra, r.k.srm1);
        } else if (L.kind == EDTTS_OBJ_DISTILL) {
          x0 = obj_x0(xt, v1[k], r.k.sab, r.k.s1m);
          const float d = x0 - obj_x0(xt, v2[k], r.k.sab, r.k.s1m);
          s[0] += d * d;
          g1[k] = -r.k.s1m * (norm * d);
        } else {
          x0 = obj_x0(xt, v1[k], r.k.sab, r.k.s1m);
          const float x02 = obj_x0(qsample_elem(xn, k2.sab, nz, k2.s1m), v2[k], k2.sab, k2.s1m);
          const float d0 = x0 - x02, d1 = x0 - xn, d2 = x02 - xn;
          s[0] += d0 * d0;
          s[1] += d1 * d1;
          s[2] += d2 * d2;
          g1[k] = -r.k.s1m * (norm * d0 + half_norm * d1);
          g2[k] = -k2.s1m * (half_norm * d2);
        }
        const float dm = x0 - xn;
        s[3] += dm * dm;
        s[4] += x0 * xn;
        s[5] += x0 * x0;
        s[6] += xn * xn;
      }
    }
    if (u1 && e0 < n_row1) obj_store4(u1, e0, n_row1, vec, g1);
    if (u2 && e0 < n_row2) obj_store4(u2, e0, n_row2, vec, g2);
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    double d = (double)s[i];
    for (int o = 32; o >= 1; o >>= 1) d += __shfl_xor(d, o);
    if ((tid & 63) == 0) wsum[tid >> 6][i] = d;
  }
  __syncthreads();
  if (tid < kObjSums) {
    double t = 0.0;
    if (tid < 7) {
      t = wsum[0][tid];
      for (int w = 1; w < kObjThreads / 64; ++w) t += wsum[w][tid];
    }
    L.partial[((size_t)b * gridDim.x + c) * kObjSums + tid] = t;
  }
}

// out[8]: loss | the loss's terms as means (3; unused ones 0) | x0_mse | x0_cos | 0 | 0
__global__ __launch_bounds__(kObjThreads) void k_obj_finish(ObjLossArgs L, int chunks, float* __restrict__ out) {
  __shared__ double rows[kObjThreads][6];  // per row: 3 terms, x0 mse, cosine, live frames
  const ObjArgs& a = L.a;
  const int tid = threadIdx.x, tm = obj_tm(L);
  double tot[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int base = 0; base < a.B; base += kObjThreads) {
    const int b = base + tid;
    if (b < a.B) {
      double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      const double* p = L.partial + (size_t)b * chunks * kObjSums;
      for (int c = 0; c < chunks; ++c)
        for (int i = 0; i < 7; ++i) v[i] += p[(size_t)c * kObjSums + i];
      for (int i = 0; i < 4; ++i) rows[tid][i] = v[i];
      // F.cosine_similarity: sum((x / max(|x|, eps)) (y / max(|y|, eps))), eps = 1e-8
      rows[tid][4] = v[4] / (fmax(sqrt(v[5]), 1e-8) * fmax(sqrt(v[6]), 1e-8));
      rows[tid][5] = (double)obj_frames(a, b, tm);
    }
    __syncthreads();
    if (tid == 0) {
      const int n = a.B - base < kObjThreads ? a.B - base : kObjThreads;
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < 6; ++i) tot[i] += rows[j][i];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double N = tot[5] * (double)a.M;
  const float m0 = (float)(tot[0] / N), m1 = (float)(tot[1] / N), m2 = (float)(tot[2] / N);
  out[0] = L.kind == EDTTS_OBJ_CONSISTENCY ? m0 + 0.5f * (m1 + m2) : m0;
  out[1] = m0;
  out[2] = m1;
  out[3] = m2;
  out[4] = (float)(tot[3] / N);
  out[5] = (float)(tot[4] / (double)a.B);
  out[6] = 0.f;
  out[7] = 0.f;
}

__global__ __launch_bounds__(256) void k_obj_scale(const float* __restrict__ unit, const float* __restrict__ grad_out, size_t n, int vec,
                                                   float* __restrict__ d) {
  const float g = grad_out[0];
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n4 = vec ? n >> 2 : 0;
  for (size_t i = i0; i < n4; i += stride) stg4(d + 4 * i, ldg4(unit + 4 * i) * g);
  for (size_t i = 4 * n4 + i0; i < n; i += stride) d[i] = unit[i] * g;
}

static int obj_chunks(long long row_elems) { return (int)((row_elems + kObjChunk - 1) / kObjChunk); }
static bool obj_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace edtts_obj

extern "C" {

int edtts_objective_scratch_bytes(int B, int T, int n_mels, size_t* out_bytes) {
  using namespace edtts_obj;
  if (!out_bytes) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (B < 1 || T < 1 || n_mels < 1 || (long long)T * n_mels >= (1ll << 30)) return fail(EDTTS_ERR_ARG, "bad sizes: B=%d T=%d n_mels=%d", B, T, n_mels);
  *out_bytes = (size_t)B * obj_chunks((long long)T * n_mels) * kObjSums * sizeof(double);
  return EDTTS_OK;
}

static int obj_check(const float* mel, int B, int T, int M, const int64_t* t, const float* tables, int n_table, const float* mean,
                     const float* stdv, const uint64_t* seeds, const float* noise) {
  if (!mel || !t || !tables) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (B < 1 || B > 65535 || T < 1 || M < 1 || n_table < 1 || (long long)T * M >= (1ll << 30))
    return fail(EDTTS_ERR_ARG, "bad sizes: B=%d T=%d n_mels=%d n_table=%d", B, T, M, n_table);
  if ((mean == nullptr) != (stdv == nullptr)) return fail(EDTTS_ERR_ARG, "mean and stdv come together (both NULL: mel is already normalised)");
  if (!seeds && !noise) return fail(EDTTS_ERR_ARG, "either seeds or noise must be given");
  return EDTTS_OK;
}

int edtts_objective_stats(const float* mel, int B, int T, int n_mels, const int64_t* lengths, float* mean, float* stdv, void* stream) {
  using namespace edtts_obj;
  if (!mel || !mean || !stdv) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (B < 1 || B > 65535 || T < 1 || n_mels < 1 || (long long)T * n_mels >= (1ll << 30))
    return fail(EDTTS_ERR_ARG, "bad sizes: B=%d T=%d n_mels=%d", B, T, n_mels);
  ObjArgs a{};
  a.mel = mel; a.B = B; a.T = T; a.M = n_mels; a.lengths = lengths;
  hipLaunchKernelGGL(k_obj_stats, dim3((n_mels + 63) / 64, B), dim3(64 * kObjStatWaves), 0, (hipStream_t)stream, a, mean, stdv);
  LAUNCH_CHECK("k_obj_stats");
  return EDTTS_OK;
}

int edtts_objective_prepare(const float* mel, int B, int T, int n_mels, const int64_t* lengths, const int64_t* t, const float* tables,
                            int n_table, const float* mean, const float* stdv, const uint64_t* seeds, const float* noise, int kind,
                            float* x_t, float* mel_n, float* noise_out, float* target, void* stream) {
  using namespace edtts_obj;
  if (int rc = obj_check(mel, B, T, n_mels, t, tables, n_table, mean, stdv, seeds, noise)) return rc;
  if (!x_t) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (kind != EDTTS_OBJ_V && kind != EDTTS_OBJ_EPS) return fail(EDTTS_ERR_ARG, "kind=%d: the target is EDTTS_OBJ_V's or EDTTS_OBJ_EPS's", kind);
  ObjArgs a{mel, B, T, n_mels, lengths, t, tables, n_table, mean, stdv, reinterpret_cast<const unsigned long long*>(seeds), noise};
  const long long n_row = (long long)T * n_mels;
  const int vec = (n_row % 4 == 0) && obj_al16(mel) && obj_al16(noise) && obj_al16(x_t) && obj_al16(mel_n) && obj_al16(noise_out) && obj_al16(target);
  hipLaunchKernelGGL(k_obj_prepare, dim3(obj_chunks(n_row), B), dim3(kObjThreads), 0, (hipStream_t)stream, a, kind, vec, x_t, mel_n,
                     noise_out, target);
  LAUNCH_CHECK("k_obj_prepare");
  return EDTTS_OK;
}

int edtts_objective_loss(int kind, const float* mel, int B, int T, int n_mels, const int64_t* lengths, const int64_t* t,
                         const float* tables, int n_table, const float* mean, const float* stdv, const uint64_t* seeds,
                         const float* noise, const float* pred, int T_pred, const float* pred2, int T_pred2, const int64_t* t2,
                         float* unit, float* unit2, void* scratch, size_t scratch_bytes, float* out, void* stream) {
  using namespace edtts_obj;
  if (int rc = obj_check(mel, B, T, n_mels, t, tables, n_table, mean, stdv, seeds, noise)) return rc;
  if (!pred || !scratch || !out) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (kind < EDTTS_OBJ_V || kind > EDTTS_OBJ_CONSISTENCY) return fail(EDTTS_ERR_ARG, "kind=%d", kind);
  const bool two = kind == EDTTS_OBJ_DISTILL || kind == EDTTS_OBJ_CONSISTENCY;
  if (two != (pred2 != nullptr)) return fail(EDTTS_ERR_ARG, "kind=%d: pred2 is %s", kind, two ? "required" : "not taken");
  if (kind == EDTTS_OBJ_CONSISTENCY && !t2) return fail(EDTTS_ERR_ARG, "EDTTS_OBJ_CONSISTENCY needs the second prediction's timesteps");
  if (unit2 && kind != EDTTS_OBJ_CONSISTENCY) return fail(EDTTS_ERR_ARG, "kind=%d has no second gradient", kind);
  if (!two) T_pred2 = T_pred;
  if (T_pred < 1 || T_pred2 < 1 || (long long)T_pred * n_mels >= (1ll << 30) || (long long)T_pred2 * n_mels >= (1ll << 30))
    return fail(EDTTS_ERR_ARG, "bad sizes: T_pred=%d T_pred2=%d", T_pred, T_pred2);
  const int t_max = T_pred > T_pred2 ? T_pred : T_pred2;
  const int chunks = obj_chunks((long long)t_max * n_mels);
  const size_t need = (size_t)B * chunks * kObjSums * sizeof(double);
  if (scratch_bytes < need) return fail(EDTTS_ERR_ARG, "scratch of %zu bytes, need %zu (edtts_objective_scratch_bytes at the longer prediction)", scratch_bytes, need);
  if ((uintptr_t)scratch & 7) return fail(EDTTS_ERR_ARG, "scratch must be 8-byte aligned");
  ObjLossArgs L{};
  L.a = ObjArgs{mel, B, T, n_mels, lengths, t, tables, n_table, mean, stdv, reinterpret_cast<const unsigned long long*>(seeds), noise};
  L.kind = kind; L.pred = pred; L.T_pred = T_pred; L.pred2 = pred2; L.T_pred2 = T_pred2; L.t2 = t2; L.unit = unit; L.unit2 = unit2;
  L.partial = static_cast<double*>(scratch);
  L.vec = ((long long)T * n_mels % 4 == 0) && ((long long)T_pred * n_mels % 4 == 0) && ((long long)T_pred2 * n_mels % 4 == 0) && obj_al16(mel) &&
          obj_al16(noise) && obj_al16(pred) && obj_al16(pred2) && obj_al16(unit) && obj_al16(unit2);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_obj_loss, dim3(chunks, B), dim3(kObjThreads), 0, st, L);
  LAUNCH_CHECK("k_obj_loss");
  hipLaunchKernelGGL(k_obj_finish, dim3(1), dim3(kObjThreads), 0, st, L, chunks, out);
  LAUNCH_CHECK("k_obj_finish");
  return EDTTS_OK;
}

int edtts_objective_scale(const float* unit, const float* grad_out, size_t n, float* d_pred, void* stream) {
  using namespace edtts_obj;
  if (n == 0) return EDTTS_OK;
  if (!unit || !grad_out || !d_pred) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  const int vec = obj_al16(unit) && obj_al16(d_pred);
  size_t bx = ((vec ? n / 4 : n) + 255) / 256;
  bx = bx < 1 ? 1 : (bx > 4096 ? 4096 : bx);
  hipLaunchKernelGGL(k_obj_scale, dim3((unsigned)bx), dim3(256), 0, (hipStream_t)stream, unit, grad_out, n, vec, d_pred);
  LAUNCH_CHECK("k_obj_scale");
  return EDTTS_OK;
}

}  // extern "C"
