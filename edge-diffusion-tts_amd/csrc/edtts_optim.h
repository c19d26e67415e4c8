// edtts_optim.h -- the optimiser step of the training loop as multi-tensor-apply kernels (included by edtts_kernels.hip;
// DESIGN.md section 24): gradient clipping (torch.nn.utils.clip_grad_norm_), AdamW (torch.optim.AdamW, single-tensor form), the
// consistency stage's EMA teacher (training/consistency.py:45-50, lerp_) and the refresh of the generic decoder's packed blob, in
// one pass over the parameters.
//
// The host cuts the list of tensors into chunks (tensor, offset, count) of at most kOptChunk elements -- chunk starts inside a
// tensor are multiples of kOptChunk, hence of 4 -- and uploads one table per step (group hyper-parameters | tensors | chunks).
//
//   k_opt_sqsum    one block per chunk: fp32 sum of g^2 in a fixed order (per-thread strided sum, lanes by __shfl_xor, the four
//                  waves through LDS in wave order) -> one partial per chunk
//   k_opt_finish   one block: partials in ascending chunk order in fp64 -> total_norm, clip_coef; the step counter; 1 - beta1^step
//                  and sqrt(1 - beta2^step) per group in fp64; or, with skip_nonfinite and a non-finite norm, the skip flag
//   k_opt_adamw    one block per chunk: the update (float4 when every pointer of the tensor is 16-byte aligned, scalar otherwise
//                  and for the tail), the EMA target, the mirrors (plain or transposed), the zeroing of g.  Nothing when the skip
//                  flag is up.
// No float atomics, no inline assembly, no scratch memory.  The C ABI (edtts_optim_*) is at the end of this file.
namespace edtts_opt {

constexpr int kOptChunk = 8192;   // elements per chunk (exported: edtts_optim_chunk_size)
constexpr int kOptThreads = 256;

struct OptBias {  // per parameter group, written by k_opt_finish
  double bc1, bc2_sqrt;
};
struct OptTensor {  // device form of EdttsOptimTensor
  float *p, *g, *m, *v, *ema, *mirror, *ema_mirror;
  int group, rows, cols;  // rows > 0: p is [rows][cols] and the mirrors hold its transpose [cols][rows]
  float ema_w;            // 1 - ema_decay
};
struct OptChunk {
  long long offset;
  int tensor, count;
};
struct OptArgs {
  EdttsOptimState* state;
  OptBias* bias;
  float* partial;
  EdttsOptimGroup* groups;  // (k_opt_finish of a resident step writes lr)
  const OptTensor* tensors;
  const OptChunk* chunks;
  int n_chunks, n_groups, flags;
  float max_norm;
};

// Scratch (bytes): EdttsOptimState | OptBias[n_groups] | partial[n_chunks] | the uploaded table: groups | tensors | chunks
struct OptScratch {
  size_t bias, partial, groups, tensors, chunks, total;
};
static size_t opt_align(size_t v) { return (v + 15) & ~(size_t)15; }
static void opt_scratch(size_t n_chunks, size_t n_groups, OptScratch* s) {
  size_t o = opt_align(sizeof(EdttsOptimState));
  s->bias = o; o = opt_align(o + n_groups * sizeof(OptBias));
  s->partial = o; o = opt_align(o + n_chunks * sizeof(float));
  s->groups = o; o = opt_align(o + n_groups * sizeof(EdttsOptimGroup));
  s->tensors = o; o = opt_align(o + n_chunks * sizeof(OptTensor));  // (a tensor has at least one chunk)
  s->chunks = o; o = opt_align(o + n_chunks * sizeof(OptChunk));
  s->total = o;
}

__global__ __launch_bounds__(kOptThreads) void k_opt_sqsum(OptArgs a) {
  __shared__ float wsum[kOptThreads / 64];
  const OptChunk ch = a.chunks[blockIdx.x];
  const float* g = a.tensors[ch.tensor].g + ch.offset;
  const int tid = threadIdx.x;
  float s = 0.f;
  if (((size_t)g & 15) == 0) {
    const int n4 = ch.count >> 2;
    constexpr int kPer = kOptChunk / 4 / kOptThreads;  // 16-byte loads per thread: all issued before the first is consumed
    f4 x[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int i = tid + j * kOptThreads;
      x[j] = i < n4 ? *reinterpret_cast<const f4*>(g + 4 * (size_t)i) : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {  // (an absent element adds +0: the order is the strided one either way)
      s += x[j][0] * x[j][0];
      s += x[j][1] * x[j][1];
      s += x[j][2] * x[j][2];
      s += x[j][3] * x[j][3];
    }
    const int i = 4 * n4 + tid;
    if (i < ch.count) s += g[i] * g[i];
  } else {
    for (int i = tid; i < ch.count; i += kOptThreads) s += g[i] * g[i];
  }
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) wsum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    float t = wsum[0];
    for (int w = 1; w < kOptThreads / 64; ++w) t += wsum[w];
    a.partial[blockIdx.x] = t;
  }
}

// b^n for an integer n >= 0 by squaring, in fp64 (about log2(n) roundings: far inside what the fp32 update can see)
EDTTS_DEV double opt_ipow(double b, long long n) {
  double r = 1.0;
  while (n > 0) {
    if (n & 1) r *= b;
    b *= b;
    n >>= 1;
  }
  return r;
}

// train_v2.cosine_lr_schedule at step n in fp64, in Python's order of operations (no contraction into fused multiply-adds)
EDTTS_DEV double opt_sched_lr(const EdttsOptimSchedule& s, long long n) {
#pragma clang fp contract(off)
  if (n < s.warmup_steps) {
    const long long w = s.warmup_steps > 1 ? s.warmup_steps : 1;
    return s.base_lr * (double)n / (double)w;
  }
  const long long span = s.total_steps - s.warmup_steps > 1 ? s.total_steps - s.warmup_steps : 1;
  const double progress = (double)(n - s.warmup_steps) / (double)span;
  return s.min_lr + 0.5 * (s.base_lr - s.min_lr) * (1.0 + cos(3.141592653589793 * progress));
}

// lr_dev (fp64 [n_groups], device) or sched.kind != EDTTS_SCHED_NONE: the resident step's learning rate, stored into the groups
// of the scratch before the step sizes are formed from it (edtts_optim_step passes neither: the uploaded lr holds).
__global__ __launch_bounds__(kOptThreads) void k_opt_finish(OptArgs a, int have_norm, const double* lr_dev, EdttsOptimSchedule sched) {
  __shared__ float buf[1024];
  const int tid = threadIdx.x;
  double acc = 0.0;
  if (have_norm) {
    for (int base = 0; base < a.n_chunks; base += 1024) {
      const int n = a.n_chunks - base < 1024 ? a.n_chunks - base : 1024;
      for (int j = tid; j < n; j += kOptThreads) buf[j] = a.partial[base + j];
      __syncthreads();
      if (tid == 0)
        for (int j = 0; j < n; ++j) acc += (double)buf[j];  // ascending chunk order
      __syncthreads();
    }
  }
  if (tid != 0) return;
  EdttsOptimState* st = a.state;
  const float tn = (float)sqrt(acc);
  float coef = 1.f;
  if (a.flags & EDTTS_OPT_CLIP) {
    coef = a.max_norm / (tn + 1e-6f);  // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0) -- a NaN stays a NaN
    if (coef > 1.f) coef = 1.f;
  }
  const bool bad = (a.flags & EDTTS_OPT_SKIP_NONFINITE) && !(fabsf(tn) <= 3.402823466e38f);
  if (lr_dev || sched.kind != EDTTS_SCHED_NONE) {  // (a skipped step has its lr too: the schedule's position is step + skipped)
    const double lr_s = sched.kind != EDTTS_SCHED_NONE ? opt_sched_lr(sched, st->step + st->skipped) : 0.0;
    for (int i = 0; i < a.n_groups; ++i) a.groups[i].lr = lr_dev ? lr_dev[i] : lr_s;
  }
  st->total_norm = tn;
  st->clip_coef = coef;
  st->skip = bad ? 1 : 0;
  if (bad) {
    st->skipped += 1;
    return;
  }
  const long long step = st->step + 1;
  st->step = step;
  for (int i = 0; i < a.n_groups; ++i) {
    a.bias[i].bc1 = 1.0 - opt_ipow(a.groups[i].beta1, step);
    a.bias[i].bc2_sqrt = sqrt(1.0 - opt_ipow(a.groups[i].beta2, step));
  }
}

struct OptCoef {
  float clip, decay, w1, b2, w2, step_size, bc2s, eps;
};
// torch/optim/adamw.py, _single_tensor_adamw (the host scalars are Python doubles, rounded to fp32 where they meet a tensor)
EDTTS_DEV void opt_update(const OptCoef& c, float& p, float g, float& m, float& v) {
  g *= c.clip;
  p *= c.decay;
  m = m + c.w1 * (g - m);
  v = v * c.b2 + c.w2 * g * g;
  const float denom = sqrtf(v) / c.bc2s + c.eps;
  p = p - c.step_size * (m / denom);
}

__global__ __launch_bounds__(kOptThreads) void k_opt_adamw(OptArgs a) {
  const bool ema_only = a.flags & EDTTS_OPT_EMA_ONLY;
  if (!ema_only && a.state->skip) return;
  const OptChunk ch = a.chunks[blockIdx.x];
  const OptTensor t = a.tensors[ch.tensor];
  const int tid = threadIdx.x;
  OptCoef c{};
  if (!ema_only) {
    const EdttsOptimGroup gr = a.groups[t.group];
    const OptBias bs = a.bias[t.group];
    c.clip = (a.flags & EDTTS_OPT_CLIP) ? a.state->clip_coef : 1.f;
    c.decay = (float)(1.0 - gr.lr * gr.weight_decay);
    c.w1 = (float)(1.0 - gr.beta1);
    c.b2 = (float)gr.beta2;
    c.w2 = (float)(1.0 - gr.beta2);
    c.step_size = (float)(gr.lr / bs.bc1);
    c.bc2s = (float)bs.bc2_sqrt;
    c.eps = (float)gr.eps;
  }
  const bool zero_g = !ema_only && (a.flags & EDTTS_OPT_ZERO_GRADS);
  const size_t off = (size_t)ch.offset;
  float* p = t.p + off;
  float* g = ema_only ? nullptr : t.g + off;
  float* m = ema_only ? nullptr : t.m + off;
  float* v = ema_only ? nullptr : t.v + off;
  float* e = t.ema ? t.ema + off : nullptr;
  const bool tr = t.rows > 0;
  // element i of the tensor -> its place in a mirror: i itself, or (i % cols) * rows + i / cols in the transpose
  auto mirror1 = [&](size_t i, float pn, float en) {
    size_t d = i;
    if (tr) d = (i % (size_t)t.cols) * (size_t)t.rows + i / (size_t)t.cols;
    if (t.mirror) t.mirror[d] = pn;
    if (t.ema_mirror) t.ema_mirror[d] = en;
  };
  auto scalar1 = [&](int i) {
    float pn = p[i], en = 0.f;
    if (!ema_only) {
      float mm = m[i], vv = v[i];
      opt_update(c, pn, g[i], mm, vv);
      p[i] = pn;
      m[i] = mm;
      v[i] = vv;
      if (zero_g) g[i] = 0.f;
    }
    if (e) {
      en = e[i];
      en = en + (pn - en) * t.ema_w;
      e[i] = en;
    }
    if (t.mirror || t.ema_mirror) mirror1(off + i, pn, en);
  };
  size_t al = (size_t)t.p | (size_t)t.g | (size_t)t.m | (size_t)t.v | (size_t)t.ema;
  if (!tr) al |= (size_t)t.mirror | (size_t)t.ema_mirror;
  if (al & 15) {
    for (int i = tid; i < ch.count; i += kOptThreads) scalar1(i);
    return;
  }
  const int n4 = ch.count >> 2;
  for (int i4 = tid; i4 < n4; i4 += kOptThreads) {
    const size_t i = 4 * (size_t)i4;
    f4 pn = *reinterpret_cast<const f4*>(p + i), en = {0.f, 0.f, 0.f, 0.f};
    if (!ema_only) {
      const f4 gg = *reinterpret_cast<const f4*>(g + i);
      f4 mm = *reinterpret_cast<const f4*>(m + i), vv = *reinterpret_cast<const f4*>(v + i);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pr = pn[r], mr = mm[r], vr = vv[r];
        opt_update(c, pr, gg[r], mr, vr);
        pn[r] = pr; mm[r] = mr; vv[r] = vr;
      }
      *reinterpret_cast<f4*>(p + i) = pn;
      *reinterpret_cast<f4*>(m + i) = mm;
      *reinterpret_cast<f4*>(v + i) = vv;
      if (zero_g) *reinterpret_cast<f4*>(g + i) = f4{0.f, 0.f, 0.f, 0.f};
    }
    if (e) {
      en = *reinterpret_cast<const f4*>(e + i);
#pragma unroll
      for (int r = 0; r < 4; ++r) en[r] = en[r] + (pn[r] - en[r]) * t.ema_w;
      *reinterpret_cast<f4*>(e + i) = en;
    }
    if (tr) {
#pragma unroll
      for (int r = 0; r < 4; ++r) mirror1(off + i + r, pn[r], en[r]);
    } else {
      if (t.mirror) *reinterpret_cast<f4*>(t.mirror + off + i) = pn;
      if (t.ema_mirror) *reinterpret_cast<f4*>(t.ema_mirror + off + i) = en;
    }
  }
  const int i = 4 * n4 + tid;
  if (i < ch.count) scalar1(i);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// Chunks of one tensor: starts 0, kOptChunk, 2 kOptChunk, ... (multiples of 4); a tensor without elements has none.
static long long opt_chunks_of(long long numel) { return numel <= 0 ? 0 : (numel + kOptChunk - 1) / kOptChunk; }

// Pinned staging ring for the per-step table.  A step takes the next slot, fills it and enqueues the copy into the scratch's table
// and the kernels behind it; the event recorded behind the copy says when the slot may be written again.  So a step issued
// while earlier ones have not run is safe; only with more than kOptRing steps outstanding does the host wait for the oldest copy.
constexpr int kOptRing = 8;
struct OptSlot {
  void* host = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  bool pending = false;
};
static std::mutex g_opt_mu;
static OptSlot g_opt_ring[kOptRing];
static int g_opt_next = 0;

}  // namespace edtts_opt

// =========================================================================================================
// the C ABI
// =========================================================================================================
extern "C" {

int edtts_optim_chunk_size(void) { return edtts_opt::kOptChunk; }

int edtts_optim_chunk_table(const int64_t* numels, int n_tensors, int cap, int32_t* tensor, int64_t* offset, int32_t* count, int* n_chunks) {
  if (!numels || !n_chunks || n_tensors < 0) return fail(EDTTS_ERR_ARG, "edtts_optim_chunk_table: NULL pointer argument or n_tensors < 0");
  long long n = 0;
  for (int i = 0; i < n_tensors; ++i) {
    if (numels[i] < 0) return fail(EDTTS_ERR_ARG, "edtts_optim_chunk_table: numels[%d] = %lld < 0", i, (long long)numels[i]);
    for (long long o = 0; o < numels[i]; o += edtts_opt::kOptChunk, ++n) {
      if (n >= cap) continue;  // (counted, not written)
      if (!tensor || !offset || !count) return fail(EDTTS_ERR_ARG, "edtts_optim_chunk_table: cap > 0 needs the three output arrays");
      const long long left = numels[i] - o;
      tensor[n] = i;
      offset[n] = o;
      count[n] = (int32_t)(left < edtts_opt::kOptChunk ? left : edtts_opt::kOptChunk);
    }
  }
  if (n > 0x7fffffff) return fail(EDTTS_ERR_UNSUPPORTED, "edtts_optim_chunk_table: %lld chunks", n);
  *n_chunks = (int)n;
  return EDTTS_OK;
}

int edtts_optim_scratch_bytes(int n_chunks, int n_groups, size_t* out_bytes) {
  if (!out_bytes || n_chunks < 0 || n_groups < 1) return fail(EDTTS_ERR_ARG, "edtts_optim_scratch_bytes: n_chunks=%d n_groups=%d", n_chunks, n_groups);
  edtts_opt::OptScratch s;
  edtts_opt::opt_scratch((size_t)n_chunks, (size_t)n_groups, &s);
  *out_bytes = s.total;
  return EDTTS_OK;
}

// The checks of a step's arguments and the count of its chunks (`who` names the entry point in messages).
static int opt_validate(const char* who, const EdttsOptimTensor* tensors, int n_tensors, const EdttsOptimGroup* groups, int n_groups,
                        double max_norm, int flags, const void* scratch, long long* n_chunks_out) {
  using namespace edtts_opt;
  if (n_tensors < 0 || n_groups < 1 || (n_tensors && !tensors) || !groups || !scratch)
    return fail(EDTTS_ERR_ARG, "%s: NULL pointer argument, n_tensors=%d or n_groups=%d", who, n_tensors, n_groups);
  if (flags & ~(EDTTS_OPT_CLIP | EDTTS_OPT_SKIP_NONFINITE | EDTTS_OPT_ZERO_GRADS | EDTTS_OPT_EMA_ONLY))
    return fail(EDTTS_ERR_ARG, "%s: unknown flag bits 0x%x", who, flags);
  const bool ema_only = flags & EDTTS_OPT_EMA_ONLY;
  if (ema_only && (flags & ~EDTTS_OPT_EMA_ONLY)) return fail(EDTTS_ERR_ARG, "%s: EDTTS_OPT_EMA_ONLY excludes the other flags", who);
  if ((flags & EDTTS_OPT_CLIP) && !(max_norm >= 0.0)) return fail(EDTTS_ERR_ARG, "%s: max_norm=%g", who, max_norm);
  long long n_chunks = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const EdttsOptimTensor& t = tensors[i];
    if (t.numel < 0) return fail(EDTTS_ERR_ARG, "%s: tensor %d has numel %lld", who, i, (long long)t.numel);
    if (t.numel == 0) continue;
    if (!t.p || (!ema_only && (!t.g || !t.m || !t.v)) || (ema_only && !t.ema))
      return fail(EDTTS_ERR_ARG, "%s: tensor %d has a NULL p, g, m, v or (EDTTS_OPT_EMA_ONLY) ema", who, i);
    if (((size_t)t.p | (size_t)t.g | (size_t)t.m | (size_t)t.v | (size_t)t.ema | (size_t)t.mirror | (size_t)t.ema_mirror) & 3)
      return fail(EDTTS_ERR_ARG, "%s: tensor %d has a pointer that is not 4-byte aligned", who, i);
    if (t.group < 0 || t.group >= n_groups) return fail(EDTTS_ERR_ARG, "%s: tensor %d names group %d of %d", who, i, t.group, n_groups);
    if (t.rows < 0 || t.cols < 0 || (t.rows > 0 && (int64_t)t.rows * t.cols != t.numel))
      return fail(EDTTS_ERR_ARG, "%s: tensor %d: rows=%d cols=%d do not make numel=%lld", who, i, t.rows, t.cols, (long long)t.numel);
    if (t.ema_mirror && !t.ema) return fail(EDTTS_ERR_ARG, "%s: tensor %d has an ema_mirror without an ema", who, i);
    if (t.ema && !(t.ema_decay >= 0.f && t.ema_decay <= 1.f)) return fail(EDTTS_ERR_ARG, "%s: tensor %d: ema_decay=%g", who, i, (double)t.ema_decay);
    n_chunks += opt_chunks_of(t.numel);
  }
  if (n_chunks > 0x7fffffff) return fail(EDTTS_ERR_UNSUPPORTED, "%s: %lld chunks", who, n_chunks);
  *n_chunks_out = n_chunks;
  return EDTTS_OK;
}

// The table (groups | tensors | chunks) of validated arguments into the scratch, through the pinned ring, behind `st`'s work.
static int opt_upload_table(const EdttsOptimTensor* tensors, int n_tensors, const EdttsOptimGroup* groups, int n_groups,
                            const edtts_opt::OptScratch& ls, char* sc, hipStream_t st) {
  using namespace edtts_opt;
  const size_t up_bytes = ls.total - ls.groups;  // groups | tensors | chunks, as they lie in the scratch
  std::lock_guard<std::mutex> lock(g_opt_mu);
  OptSlot& slot = g_opt_ring[g_opt_next];
  g_opt_next = (g_opt_next + 1) % kOptRing;
  if (slot.pending) {
    HIP_TRY(hipEventSynchronize(slot.ev));  // (returns at once unless kOptRing steps are outstanding)
    slot.pending = false;
  }
  if (slot.cap < up_bytes) {
    if (slot.host) HIP_TRY(hipHostFree(slot.host));
    slot.host = nullptr;
    slot.cap = 0;
    HIP_TRY(hipHostMalloc(&slot.host, up_bytes + up_bytes / 2, hipHostMallocDefault));
    slot.cap = up_bytes + up_bytes / 2;
  }
  if (slot.ev) (void)hipEventDestroy(slot.ev);  // (an event belongs to the device that was current when it was made: a new one per step)
  slot.ev = nullptr;
  HIP_TRY(hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming));
  char* up = (char*)slot.host;
  memset(up, 0, up_bytes);
  memcpy(up, groups, (size_t)n_groups * sizeof(EdttsOptimGroup));
  OptTensor* ht = (OptTensor*)(up + (ls.tensors - ls.groups));
  OptChunk* hc = (OptChunk*)(up + (ls.chunks - ls.groups));
  int ti = 0;
  long long ci = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const EdttsOptimTensor& t = tensors[i];
    if (t.numel == 0) continue;
    ht[ti] = OptTensor{t.p, t.g, t.m, t.v, t.ema, t.mirror, t.ema_mirror, t.group, t.rows, t.cols, (float)(1.0 - (double)t.ema_decay)};
    for (long long o = 0; o < t.numel; o += kOptChunk, ++ci) {
      const long long left = t.numel - o;
      hc[ci] = OptChunk{o, ti, (int)(left < kOptChunk ? left : kOptChunk)};
    }
    ++ti;
  }
  HIP_TRY(hipMemcpyAsync(sc + ls.groups, up, up_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(slot.ev, st));
  slot.pending = true;
  return EDTTS_OK;
}

// The two or three launches of a step on the table that lies in the scratch.
static int opt_launch(long long n_chunks, int n_groups, double max_norm, int flags, const edtts_opt::OptScratch& ls, char* sc,
                      const double* lr_dev, const EdttsOptimSchedule& sched, hipStream_t st) {
  using namespace edtts_opt;
  OptArgs a{(EdttsOptimState*)sc, (OptBias*)(sc + ls.bias), (float*)(sc + ls.partial), (EdttsOptimGroup*)(sc + ls.groups),
            (const OptTensor*)(sc + ls.tensors), (const OptChunk*)(sc + ls.chunks), (int)n_chunks, n_groups, flags, (float)max_norm};
  if (!(flags & EDTTS_OPT_EMA_ONLY)) {
    const int have_norm = (flags & (EDTTS_OPT_CLIP | EDTTS_OPT_SKIP_NONFINITE)) ? 1 : 0;
    if (have_norm) {
      hipLaunchKernelGGL(k_opt_sqsum, dim3((unsigned)n_chunks), dim3(kOptThreads), 0, st, a);
      LAUNCH_CHECK("k_opt_sqsum");
    }
    hipLaunchKernelGGL(k_opt_finish, dim3(1), dim3(kOptThreads), 0, st, a, have_norm, lr_dev, sched);
    LAUNCH_CHECK("k_opt_finish");
  }
  hipLaunchKernelGGL(k_opt_adamw, dim3((unsigned)n_chunks), dim3(kOptThreads), 0, st, a);
  LAUNCH_CHECK("k_opt_adamw");
  return EDTTS_OK;
}

int edtts_optim_step(const EdttsOptimTensor* tensors, int n_tensors, const EdttsOptimGroup* groups, int n_groups, double max_norm, int flags,
                     void* scratch, size_t scratch_bytes, void* stream) {
  using namespace edtts_opt;
  long long n_chunks = 0;
  TRY_G(opt_validate("edtts_optim_step", tensors, n_tensors, groups, n_groups, max_norm, flags, scratch, &n_chunks));
  if (n_chunks == 0) return EDTTS_OK;  // nothing to step: as torch, no state changes (the step counter included)
  OptScratch ls;
  opt_scratch((size_t)n_chunks, (size_t)n_groups, &ls);
  if (ls.total > scratch_bytes)
    return fail(EDTTS_ERR_ARG, "edtts_optim_step: %lld chunks in %d groups need %zu bytes of scratch, got %zu", n_chunks, n_groups, ls.total, scratch_bytes);
  TRY_G(opt_upload_table(tensors, n_tensors, groups, n_groups, ls, (char*)scratch, (hipStream_t)stream));
  return opt_launch(n_chunks, n_groups, max_norm, flags, ls, (char*)scratch, nullptr, EdttsOptimSchedule{}, (hipStream_t)stream);
}

int edtts_optim_upload(const EdttsOptimTensor* tensors, int n_tensors, const EdttsOptimGroup* groups, int n_groups, int flags, void* scratch,
                       size_t scratch_bytes, int* n_chunks_out, size_t* groups_offset, void* stream) {
  using namespace edtts_opt;
  if (!n_chunks_out || !groups_offset) return fail(EDTTS_ERR_ARG, "edtts_optim_upload: NULL n_chunks or groups_offset");
  if (flags & EDTTS_OPT_EMA_ONLY) return fail(EDTTS_ERR_ARG, "edtts_optim_upload: EDTTS_OPT_EMA_ONLY has no resident form");
  long long n_chunks = 0;
  TRY_G(opt_validate("edtts_optim_upload", tensors, n_tensors, groups, n_groups, 0.0, flags, scratch, &n_chunks));
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing((hipStream_t)stream, &cap));
  if (cap != hipStreamCaptureStatusNone) return fail(EDTTS_ERR_ARG, "edtts_optim_upload: the stream is capturing (upload outside the capture)");
  OptScratch ls;
  opt_scratch((size_t)n_chunks, (size_t)n_groups, &ls);
  if (ls.total > scratch_bytes)
    return fail(EDTTS_ERR_ARG, "edtts_optim_upload: %lld chunks in %d groups need %zu bytes of scratch, got %zu", n_chunks, n_groups, ls.total, scratch_bytes);
  if (n_chunks) TRY_G(opt_upload_table(tensors, n_tensors, groups, n_groups, ls, (char*)scratch, (hipStream_t)stream));
  *n_chunks_out = (int)n_chunks;
  *groups_offset = ls.groups;
  return EDTTS_OK;
}

int edtts_optim_step_resident(int n_chunks, int n_groups, double max_norm, int flags, void* scratch, size_t scratch_bytes, const double* lr_dev,
                              const EdttsOptimSchedule* sched, void* stream) {
  using namespace edtts_opt;
  if (n_chunks < 0 || n_groups < 1 || !scratch) return fail(EDTTS_ERR_ARG, "edtts_optim_step_resident: NULL scratch, n_chunks=%d or n_groups=%d", n_chunks, n_groups);
  if (flags & ~(EDTTS_OPT_CLIP | EDTTS_OPT_SKIP_NONFINITE | EDTTS_OPT_ZERO_GRADS))
    return fail(EDTTS_ERR_ARG, "edtts_optim_step_resident: flag bits 0x%x (EDTTS_OPT_EMA_ONLY has no resident form)", flags);
  if ((flags & EDTTS_OPT_CLIP) && !(max_norm >= 0.0)) return fail(EDTTS_ERR_ARG, "edtts_optim_step_resident: max_norm=%g", max_norm);
  if ((size_t)lr_dev & 7) return fail(EDTTS_ERR_ARG, "edtts_optim_step_resident: lr_dev is not 8-byte aligned");
  EdttsOptimSchedule sc{};
  if (sched) {
    sc = *sched;
    if (sc.kind != EDTTS_SCHED_NONE && sc.kind != EDTTS_SCHED_COSINE) return fail(EDTTS_ERR_ARG, "edtts_optim_step_resident: schedule kind %d", sc.kind);
    if (sc.kind == EDTTS_SCHED_COSINE && (!(sc.base_lr >= 0.0) || !(sc.min_lr >= 0.0) || sc.warmup_steps < 0 || sc.total_steps < 0))
      return fail(EDTTS_ERR_ARG, "edtts_optim_step_resident: cosine schedule with base_lr=%g min_lr=%g warmup_steps=%lld total_steps=%lld", sc.base_lr,
                  sc.min_lr, (long long)sc.warmup_steps, (long long)sc.total_steps);
  }
  if (n_chunks == 0) return EDTTS_OK;
  OptScratch ls;
  opt_scratch((size_t)n_chunks, (size_t)n_groups, &ls);
  if (ls.total > scratch_bytes)
    return fail(EDTTS_ERR_ARG, "edtts_optim_step_resident: %d chunks in %d groups need %zu bytes of scratch, got %zu", n_chunks, n_groups, ls.total, scratch_bytes);
  return opt_launch(n_chunks, n_groups, max_norm, flags, ls, (char*)scratch, lr_dev, sc, (hipStream_t)stream);
}

}  // extern "C"
