// edtts_samplers.h -- the samplers (included by edtts_kernels.hip behind the launchers, launch_cond, the length and shape checks and
// EDTTS_DISPATCH, which it needs).  A sampler step's update runs in the tail of the last layer's kernel (tail_apply; edtts_generic.h:
// k_gen_tail), so the kernels here are what is left over:
//
//   k_ddim / k_ddpm            stand-alone elementwise updates (HBM-bound)                         schedule.py:157-238
//   k_inpaint_inject(1)        q_sample of the known frames of an in-painting call                 inference_pipeline.py:117-123
//   k_inpaint_inject_mask(1)   ... of the frames a per-frame mask names (known frames anywhere, not a prefix)
//   k_randn / k_randn_rows     standard normals from the library's Philox streams
//   run_sampler                the sub-batched step loop of edtts_generate / edtts_sample_multistep / edtts_sample_ddpm
//   run_inpaint                the step loop of the in-painting samplers, on the caller's stream alone
// C ABI: edtts_generate(_len), edtts_sample_multistep(_len), edtts_sample_ddpm(_len), edtts_sample_inpaint(_len),
// edtts_sample_inpaint_multistep_len, edtts_sample_inpaint_mask_len, edtts_sample_inpaint_multistep_mask_len, edtts_ddim_step,
// edtts_ddpm_step, edtts_randn, edtts_randn_rows.

// =========================================================================================================
// standalone DDIM / DDPM updates (HBM-bound: read x, eps ; write x_prev, x0 = 16 B/element)
// =========================================================================================================
struct StepArgs {
  const float *alphas, *alpha_bar, *betas, *post_var;
  int n_table;
  const float *x, *eps, *noise;
  const int64_t *t, *t_prev;
  size_t n_per_batch;
  float eta;
  float *x_prev, *x0;
  int vec4;  // 1: n_per_batch % 4 == 0 and every tensor 16-byte aligned -> float4 accesses; 0: scalar path
};
// the float4 path of the stand-alone update kernels needs every batch row base 16-byte aligned
static int step_vec4(size_t n_per_batch, std::initializer_list<const void*> ptrs) {
  uintptr_t m = 0;
  for (const void* p : ptrs) m |= (uintptr_t)p;
  return (n_per_batch & 3) == 0 && (m & 15) == 0;
}
EDTTS_DEV long clamp_idx(long v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

__global__ __launch_bounds__(256) void k_ddim(StepArgs a) {
  const int b = blockIdx.y;
  // per-batch scalars, evaluated with the reference's operation sequence (schedule.py:179-196)
  const float ab = a.alpha_bar[clamp_idx((long)a.t[b], a.n_table)];
  const long tp = (long)a.t_prev[b];
  const float abp = tp >= 0 ? a.alpha_bar[clamp_idx(tp, a.n_table)] : 1.0f;
  const DdimCoef cf = ddim_coef(ab, abp, a.eta);
  const float s1m = cf.s1m, sab = cf.sab, sabp = cf.sabp, cdir = cf.cdir, sigma = cf.sigma;
  const size_t base = (size_t)b * a.n_per_batch;
  const size_t n4 = a.vec4 ? a.n_per_batch >> 2 : 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t o = base + 4 * i;
    const f4 xv = ldg4(a.x + o), e = ldg4(a.eps + o);
    f4 nz = splat(0.f);
    if (a.noise) nz = ldg4(a.noise + o);
    f4 x0, xp;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v, p;
      ddim_elem(xv[r], e[r], s1m, sab, sabp, cdir, v, p);
      if (a.noise) p = add_mul_rn(p, sigma, nz[r]);
      x0[r] = v;
      xp[r] = p;
    }
    stg4(a.x0 + o, x0);
    stg4(a.x_prev + o, xp);
  }
  // scalar path: everything when n_per_batch % 4 != 0 or a tensor is not 16-byte aligned (never on the sampler's own tensors)
  for (size_t i = (n4 << 2) + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_per_batch; i += (size_t)gridDim.x * blockDim.x) {
    const size_t o = base + i;
    float v, p;
    ddim_elem(a.x[o], a.eps[o], s1m, sab, sabp, cdir, v, p);
    if (a.noise) p = add_mul_rn(p, sigma, a.noise[o]);
    a.x0[o] = v;
    a.x_prev[o] = p;
  }
}

__global__ __launch_bounds__(256) void k_ddpm(StepArgs a) {
  const int b = blockIdx.y;
  const long tt = clamp_idx((long)a.t[b], a.n_table);
  const float al = a.alphas[tt], ab = a.alpha_bar[tt], be = a.betas[tt];
  const DdpmCoef cf = ddpm_coef(al, ab, be, a.post_var[tt], (long)a.t[b] > 0);
  const size_t base = (size_t)b * a.n_per_batch;
  const size_t n4 = a.vec4 ? a.n_per_batch >> 2 : 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t o = base + 4 * i;
    const f4 xv = ldg4(a.x + o), e = ldg4(a.eps + o), nz = ldg4(a.noise + o);
    f4 xp;
#pragma unroll
    for (int r = 0; r < 4; ++r) xp[r] = ddpm_elem(xv[r], e[r], nz[r], cf);
    stg4(a.x_prev + o, xp);
  }
  for (size_t i = (n4 << 2) + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_per_batch; i += (size_t)gridDim.x * blockDim.x) {
    const size_t o = base + i;  // scalar path (see k_ddim)
    a.x_prev[o] = ddpm_elem(a.x[o], a.eps[o], a.noise[o], cf);
  }
}

// The next six kernels have C linkage: their symbols in the code object are the plain names (k_inpaint_inject, k_randn, ...), as
// they were when the kernels stood inside edtts_kernels.hip's extern "C" block.  Outside such a block the names would be mangled.
extern "C" {

// x[b][f < overlap][:] = c_known * known[b][f][:] + c_noise * noise   (noise: injected [B, overlap, MEL] or Philox keyed by
// (seed, step, global element of the [B, overlap, MEL] tensor)); c_noise = 0 -> exact copy of the known frames.
// Per-row seeds (device uint64 [B], or null): row b draws with seeds[b] at its ROW-LOCAL element index -- the draws of the same call
// made on row b alone.  Per-row frame counts t_len (or null): row b injects its first min(overlap, T_b) frames only.
__global__ __launch_bounds__(256) void k_inpaint_inject(float* x, const float* known, const float* noise, int B, int T, int ov, int MEL,
                                                        float c_known, float c_noise, unsigned long long seed, unsigned step,
                                                        const unsigned long long* seeds, const int64_t* t_len) {
  const size_t per = (size_t)ov * MEL / 4, n4 = (size_t)B * per;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / per, r = i - b * per;
    const int Tb = t_len ? utt_len_of(t_len[b], T, false) : T;  // (utt_len_lane called from here changed k_gen_embed's code)
    const size_t live = Tb < ov ? (size_t)Tb * MEL : 4 * per;  // elements of this row's injected frames
    if (4 * r >= live) continue;
    const f4 kv = ldg4(known + 4 * i);
    f4 o = kv;
    if (c_noise != 0.f) {
      const f4 nz = noise ? ldg4(noise + 4 * i) : (seeds ? philox_normal4(seeds[b], step, r) : philox_normal4(seed, step, i));
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = qsample_elem(kv[e], c_known, nz[e], c_noise);
    }
    if (4 * r + 4 <= live) {
      stg4(x + (b * T) * MEL + 4 * r, o);
    } else {  // (a row shorter than the overlap whose last frame ends inside this quad: n_mels % 4 != 0)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * r + e < live) x[(b * T) * MEL + 4 * r + e] = o[e];
    }
  }
}

// ... one element per thread, for shapes whose rows are not float4-aligned (generic path, n_mels % 4 != 0): the same values (element e
// of the [B, overlap, MEL] noise tensor is lane e & 3 of Philox draw e >> 2; with per-row seeds e counts from the row's start)
__global__ __launch_bounds__(256) void k_inpaint_inject1(float* x, const float* known, const float* noise, int B, int T, int ov, int MEL,
                                                         float c_known, float c_noise, unsigned long long seed, unsigned step,
                                                         const unsigned long long* seeds, const int64_t* t_len) {
  const size_t per = (size_t)ov * MEL, n = (size_t)B * per;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / per, r = i - b * per;
    const int Tb = t_len ? utt_len_of(t_len[b], T, false) : T;
    if (Tb < ov && r >= (size_t)Tb * MEL) continue;
    float o = known[i];
    if (c_noise != 0.f) {
      const float nz = noise ? noise[i] : (seeds ? philox_normal4(seeds[b], step, r >> 2)[(int)(r & 3)] : philox_normal4(seed, step, i >> 2)[(int)(i & 3)]);
      o = qsample_elem(o, c_known, nz, c_noise);
    }
    x[(b * T) * MEL + r] = o;
  }
}

// The same q_sample at the frames a mask names: x[b][f][:] = c_known * known[b][f][:] + c_noise * noise wherever keep[b][f] != 0 and
// f < T_b; known, noise and x are [B, T, MEL], keep is [B, T].  The keep byte is read first: at a frame that is not kept, or past the
// row's length, neither known nor noise is loaded.  Philox keys: with per-row seeds (seeds[b], step, row-local element f * MEL + m) --
// the word k_inpaint_inject draws for the same (b, f, m) --, else (seed, step, global element b * T * MEL + f * MEL + m).
// MEL % 4 == 0 (a quad lies in one frame; every row of the three tensors starts on a float4).
__global__ __launch_bounds__(256) void k_inpaint_inject_mask(float* x, const float* known, const float* noise, const unsigned char* keep,
                                                             int B, int T, int MEL, float c_known, float c_noise, unsigned long long seed,
                                                             unsigned step, const unsigned long long* seeds, const int64_t* t_len) {
  const size_t q = (size_t)MEL / 4, per = (size_t)T * q, n4 = (size_t)B * per;  // quads per frame, per row, in all
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t fr = i / q;  // frame b * T + f
    if (!keep[fr]) continue;
    const size_t b = fr / T;
    const int Tb = t_len ? utt_len_of(t_len[b], T, false) : T;
    if (fr - b * T >= (size_t)Tb) continue;
    const f4 kv = ldg4(known + 4 * i);
    f4 o = kv;
    if (c_noise != 0.f) {
      const f4 nz = noise ? ldg4(noise + 4 * i) : (seeds ? philox_normal4(seeds[b], step, i - b * per) : philox_normal4(seed, step, i));
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = qsample_elem(kv[e], c_known, nz[e], c_noise);
    }
    stg4(x + 4 * i, o);
  }
}

// ... one element per thread, for n_mels % 4 != 0 (generic path: a quad of the row straddles frames): the same values (element e is
// lane e & 3 of Philox draw e >> 2; with per-row seeds e counts from the row's start)
__global__ __launch_bounds__(256) void k_inpaint_inject_mask1(float* x, const float* known, const float* noise, const unsigned char* keep,
                                                              int B, int T, int MEL, float c_known, float c_noise, unsigned long long seed,
                                                              unsigned step, const unsigned long long* seeds, const int64_t* t_len) {
  const size_t per = (size_t)T * MEL, n = (size_t)B * per;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t fr = i / MEL;
    if (!keep[fr]) continue;
    const size_t b = fr / T, r = i - b * per;
    const int Tb = t_len ? utt_len_of(t_len[b], T, false) : T;
    if (fr - b * T >= (size_t)Tb) continue;
    float o = known[i];
    if (c_noise != 0.f) {
      const float nz = noise ? noise[i] : (seeds ? philox_normal4(seeds[b], step, r >> 2)[(int)(r & 3)] : philox_normal4(seed, step, i >> 2)[(int)(i & 3)]);
      o = qsample_elem(o, c_known, nz, c_noise);
    }
    x[i] = o;
  }
}

// standard normals from the Philox stream of (seed, stream_id), element i of the GLOBAL tensor at out[i - elem_offset]
__global__ __launch_bounds__(256) void k_randn(float* out, size_t n, unsigned long long seed, unsigned stream_id,
                                               unsigned long long elem_offset, float scale) {
  const size_t n4 = n >> 2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f4 v = philox_normal4(seed, stream_id, (elem_offset >> 2) + i);
    stg4(out + 4 * i, v * scale);
  }
}

// row b of [B, n] = the first n draws of the Philox stream (seeds[b], stream_id): element e is lane e & 3 of draw e >> 2, as in k_randn
__global__ __launch_bounds__(256) void k_randn_rows(float* out, int B, size_t n, const unsigned long long* seeds, unsigned stream_id,
                                                    float scale) {
  const size_t q = (n + 3) >> 2, nq = (size_t)B * q;  // quads per row, all quads
  const bool vec = (n & 3) == 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / q, r = i - b * q;
    const f4 v = philox_normal4(seeds[b], stream_id, r) * scale;
    float* o = out + b * n + 4 * r;
    if (vec) {
      stg4(o, v);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * r + e < n) o[e] = v[e];
    }
  }
}

}  // extern "C"

// =========================================================================================================
// host side: the samplers' step loops
// =========================================================================================================
// What a sampler call runs on besides its per-step tails
struct SamplerInputs {
  const int64_t* t_dev = nullptr;   // conditioning: device timesteps of every step (edtts_sample_ddpm) ...
  const int64_t* t_host = nullptr;  // ... or host ones, row i = (timesteps[i], step index i)
  const int64_t* sem_idx = nullptr;
  const float* sem_features = nullptr;
  Lens ln;                // per-utterance lengths of the whole batch (token counts in ln.t are checked through ln.s)
  const float* x_T = nullptr;  // step 0 reads it ...
  const float* x = nullptr;    // ... every later step the sample the previous one wrote
};
// The sub-batched step loop of the samplers, after the entry point's own argument checks: conditioning rows of every step, the
// context cache per sub-batch, then step-major over the sub-batches.  tail_of(i, off, o) builds the tail of step i for the sub-batch
// that starts at utterance off (element o = off * T * n_mels of a [B, T, n_mels] tensor).
template <class TailOf>
static int run_sampler(const EdttsDims* dims, const Layout& lo, const void* packed, void* workspace, int B, int T, int S, int num_steps,
                       const SamplerInputs& in, void* stream, TailOf&& tail_of) {
  hipStream_t st = (hipStream_t)stream;
  const float* blob = (const float*)packed;
  float* wsb = (float*)workspace;
  SubBatches sb;
  plan_call(lo, B, T, S, num_steps, wsb, &sb);
  TRY_G(launch_len_check(in.ln.t_dbl ? nullptr : in.ln.t, in.ln.s, B, T, S, wsb, st));
  TRY_G(launch_cond(lo, blob, in.t_dev, nullptr, in.t_host, num_steps, wsb + sb.cond, wsb, st));
  const size_t row = (size_t)lo.L * 2 * 2 * lo.H;
  const size_t per_utt = (size_t)T * lo.MEL;
  ForkJoin fj;
  TRY_G(fj.init(sb, st));
  auto call = [&](int j) { return CallCtx{lo, blob, sb.ws[j], wsb + sb.base[j], sb.B[j], T, S, dims->window, in.ln.at(sb.off[j]), fj.st[j]}; };
  EDTTS_DISPATCH(lo, {
    TRY_G(set_attrs_once<LN>());
    for (int j = 0; j < sb.n; ++j) {
      const size_t off = sb.off[j];
      TRY_G(LN::ctx(call(j), (in.sem_features || !in.sem_idx) ? nullptr : in.sem_idx + off * S,
                  in.sem_features ? in.sem_features + off * S * lo.SD : nullptr));
    }
    for (int i = 0; i < num_steps; ++i)
      for (int j = 0; j < sb.n; ++j) {
        const size_t o = (size_t)sb.off[j] * per_utt;
#ifdef EDTTS_WAVELOG
        g_wavelog_base = sb.off[j] * (sb.ws[j].Tp / 32);
#endif
        TRY_G(LN::forward(call(j), (i == 0 ? in.x_T : in.x) + o, wsb + sb.cond + i * row, 0, tail_of(i, sb.off[j], o)));
      }
  });
  return EDTTS_OK;
}

// The multistep samplers' rows of coef_host: {mode, p0, p1, c0, c1, rinv, cB, cC}; a step cannot look further back than the steps before it
static int check_lms_modes(const float* coef_host, int num_steps) {
  for (int i = 0; i < num_steps; ++i) {
    const int mode = (int)coef_host[8 * i];
    if (mode < 1 || mode > 3 || mode > i + 1) return fail(EDTTS_ERR_ARG, "step %d: bad solver mode %d", i, mode);
  }
  return EDTTS_OK;
}
// LmsStepArgs of step i from its coefficient row c.  hist is a ring of two slots of `per` floats: step i writes slot i%2; newest
// previous = slot (i-1)%2, the one before = slot i%2.  o: element offset of the (sub-)batch in a [B, T, n_mels] tensor.
static LmsStepArgs lms_step_args(const float* c, float* hist, float* x0_all, size_t per, int i, size_t o) {
  LmsStepArgs ls;
  ls.k = LmsCoef{(int)c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]};
  ls.x0_hist = hist + (size_t)(i & 1) * per + o;
  ls.h_new = hist + (size_t)((i + 1) & 1) * per + o;
  ls.h_old = hist + (size_t)(i & 1) * per + o;
  ls.x0_all = x0_all ? x0_all + (size_t)i * per + o : nullptr;
  return ls;
}

// What the in-painting entry points share: the arguments of edtts_sample_inpaint_len, in its order (include/edtts.h)
struct InpaintArgs {
  const EdttsDims* dims; const void* packed; void *workspace, *workspace_uncond; int B, T, S;
  const float *sem_features, *zero_features; float* x; int num_steps; const int64_t *t_all, *step_all;
  const float *coef_host, *known_mel; int overlap_len; const float* noise_k; uint64_t seed; float cfg_scale; float* v_uncond;
  const int64_t *t_len, *s_len; const uint64_t* seeds; void* stream;
  const uint8_t* keep = nullptr;  // the *_mask_len entry points: [B, T], known_mel and noise_k are whole [B, T, n_mels] tensors, overlap_len unused
};
// The step loop of the in-painting samplers, in one piece on the caller's stream (no sub-batches: a captured call stays one chain):
// the shared argument checks (own_ptrs: the entry point's further pointers are there; own_checks(): its further checks, made last),
// the conditioning rows of every step, the context cache (guided: a second one in workspace_uncond) and per step the unconditional
// forward into v_uncond (guided), then the conditional one with tail_of(i), whose vp.v_uncond is set here.  With a known tail,
// inject_before(i) runs ahead of step i and inject_after() behind the last one.
template <class Checks, class InjectBefore, class TailOf, class InjectAfter>
static int run_inpaint(const InpaintArgs& a, const Layout& lo, bool own_ptrs, Checks&& own_checks, InjectBefore&& inject_before,
                       TailOf&& tail_of, InjectAfter&& inject_after) {
  if (!a.packed || !a.workspace || !a.sem_features || !a.x || !a.t_all || !a.step_all || !a.coef_host || !own_ptrs) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (a.num_steps < 1) return fail(EDTTS_ERR_ARG, "num_steps=%d < 1", a.num_steps);
  const bool guided = a.cfg_scale != 1.0f;
  if (guided && (!a.workspace_uncond || !a.zero_features || !a.v_uncond)) return fail(EDTTS_ERR_ARG, "cfg_scale != 1 needs workspace_uncond, zero_features and v_uncond");
  const bool prefix = a.known_mel && !a.keep;  // the known frames are the first overlap_len of every row
  if (prefix && (a.overlap_len < 1 || a.overlap_len > a.T)) return fail(EDTTS_ERR_ARG, "overlap_len=%d outside [1,%d]", a.overlap_len, a.T);
  TRY_G(check_shapes(lo, a.B, a.T, a.S));
  TRY_G(own_checks());
  hipStream_t st = (hipStream_t)a.stream;
  const float* blob = (const float*)a.packed;
  float* wsb = (float*)a.workspace;
  Workspace ws;
  make_workspace(lo, a.B, a.T, a.S, a.num_steps, &ws);
  TRY_G(launch_len_check(a.t_len, a.s_len, a.B, a.T, a.S, wsb, st, prefix ? a.overlap_len : 1));
  TRY_G(launch_cond(lo, blob, a.t_all, a.step_all, nullptr, a.num_steps, wsb + ws.cond, wsb, st));
  const size_t row = (size_t)lo.L * 2 * 2 * lo.H;
  const CallCtx c{lo, blob, ws, wsb, a.B, a.T, a.S, a.dims->window, Lens{a.t_len, a.s_len}, st};
  CallCtx cu = c;  // the unconditional pass: its own context cache and activations (workspace_uncond)
  cu.wsb = (float*)a.workspace_uncond;
  EDTTS_DISPATCH(lo, {
    TRY_G(set_attrs_once<LN>());
    TRY_G(LN::ctx(c, nullptr, a.sem_features));
    if (guided) TRY_G(LN::ctx(cu, nullptr, a.zero_features));  // (the solo call's zero context has S_b rows)
    for (int i = 0; i < a.num_steps; ++i) {
      if (a.known_mel) TRY_G(inject_before(i));
      StepTail tail = tail_of(i);
      if (guided) {
        // the unconditional pass shares nothing with the conditional one but x and the conditioning rows
        StepTail eps_tail;
        eps_tail.eps = a.v_uncond;
        TRY_G(LN::forward(cu, a.x, wsb + ws.cond + i * row, 0, eps_tail));
        tail.vp.v_uncond = a.v_uncond;
      }
      TRY_G(LN::forward(c, a.x, wsb + ws.cond + i * row, 0, tail));
    }
    if (a.known_mel) TRY_G(inject_after());
  });
  return EDTTS_OK;
}

// One launch of k_inpaint_inject (whole float4s) or, for a known block that is not made of them (generic path, n_mels % 4 != 0),
// k_inpaint_inject1: q_sample of the known frames with step `step`'s noise (injected: block `step` of noise_k) and stream id.
static void launch_inject(const InpaintArgs& a, int mel, float c_known, float c_noise, int step) {
  const size_t per_k = (size_t)a.B * a.overlap_len * mel;
  const bool vec = ((size_t)a.overlap_len * mel) % 4 == 0 && ((size_t)a.T * mel) % 4 == 0;
  const size_t bx = (per_k / (vec ? 4 : 1) + 255) / 256;
  hipLaunchKernelGGL(vec ? k_inpaint_inject : k_inpaint_inject1, dim3(bx > 2048 ? 2048u : (unsigned)bx), dim3(256), 0, (hipStream_t)a.stream, a.x, a.known_mel,
                     a.noise_k ? a.noise_k + (size_t)step * per_k : nullptr, a.B, a.T, a.overlap_len, mel, c_known, c_noise,
                     (unsigned long long)a.seed, kStreamInpaintStep + (unsigned)step, reinterpret_cast<const unsigned long long*>(a.seeds),
                     a.t_len);
}

// ... of k_inpaint_inject_mask (n_mels % 4 == 0) or k_inpaint_inject_mask1: the same for the frames a.keep names, over the whole
// [B, T, n_mels] tensors (block `step` of an injected noise_k is that large)
static void launch_inject_mask(const InpaintArgs& a, int mel, float c_known, float c_noise, int step) {
  const size_t per = (size_t)a.B * a.T * mel;
  const bool vec = step_vec4((size_t)mel, {a.x, a.known_mel, a.noise_k});
  const size_t bx = (per / (vec ? 4 : 1) + 255) / 256;
  hipLaunchKernelGGL(vec ? k_inpaint_inject_mask : k_inpaint_inject_mask1, dim3(bx > 2048 ? 2048u : (unsigned)bx), dim3(256), 0, (hipStream_t)a.stream, a.x,
                     a.known_mel, a.noise_k ? a.noise_k + (size_t)step * per : nullptr, a.keep, a.B, a.T, mel, c_known, c_noise,
                     (unsigned long long)a.seed, kStreamInpaintStep + (unsigned)step, reinterpret_cast<const unsigned long long*>(a.seeds),
                     a.t_len);
}
// known_mel and keep come together or not at all (neither: the plain sampler)
static int check_mask_args(const float* known_mel, const uint8_t* keep) {
  if ((known_mel == nullptr) != (keep == nullptr)) return fail(EDTTS_ERR_ARG, "known_mel and keep must both be given or both be NULL");
  return EDTTS_OK;
}

static unsigned step_blocks(const StepArgs& a) {  // blocks per utterance of k_ddim / k_ddpm
  const size_t bx = ((a.vec4 ? a.n_per_batch / 4 : a.n_per_batch) + 255) / 256;
  return bx > 2048 ? 2048u : (bx < 1 ? 1u : (unsigned)bx);
}

extern "C" {

int edtts_generate(const EdttsDims* dims, const void* packed, void* workspace, int B, int S, const int64_t* sem_idx,
                   const float* x_T, int num_steps, const int64_t* timesteps_host, const float* coef_host, float* x_work,
                   float* x0_out, void* stream) {
  return edtts_generate_len(dims, packed, workspace, B, S, sem_idx, nullptr, x_T, num_steps, timesteps_host, coef_host, x_work, x0_out,
                            stream);
}

int edtts_generate_len(const EdttsDims* dims, const void* packed, void* workspace, int B, int S, const int64_t* sem_idx,
                       const int64_t* s_len, const float* x_T, int num_steps, const int64_t* timesteps_host, const float* coef_host,
                       float* x_work, float* x0_out, void* stream) {
  const SettingsScope settings;
  Layout lo;
  TRY_G(make_layout(dims, &lo));
  if (!packed || !workspace || !sem_idx || !x_T || !timesteps_host || !coef_host || !x_work || !x0_out)
    return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (num_steps < 1 || num_steps > lo.NSTEP)
    return fail(EDTTS_ERR_ARG, "num_steps=%d outside [1,%d] (step_emb rows; the reference raises IndexError)", num_steps, lo.NSTEP);
  const int T = 2 * S;  // inference.py:31
  TRY_G(check_shapes(lo, B, T, S));
  SamplerInputs in;
  in.t_host = timesteps_host; in.sem_idx = sem_idx;
  in.ln = Lens{s_len, s_len, true};  // frames = 2 x tokens (inference.py:31)
  in.x_T = x_T; in.x = x_work;
  return run_sampler(dims, lo, packed, workspace, B, T, S, num_steps, in, stream, [&](int i, int, size_t o) {
    StepTail tail;
    tail.kind = TAIL_DDIM; tail.x_prev = x_work + o; tail.x0 = x0_out + o; tail.coef = coef_host + 4 * i;
    return tail;
  });
}

int edtts_sample_multistep(const EdttsDims* dims, const void* packed, void* workspace, int B, int T, int S, const int64_t* sem_idx,
                           const float* sem_features, const float* x_T, int num_steps, const int64_t* timesteps_host,
                           const float* coef_host, float* hist, float* x0_all, float* x_out, void* stream) {
  return edtts_sample_multistep_len(dims, packed, workspace, B, T, S, sem_idx, sem_features, nullptr, nullptr, x_T, num_steps,
                                    timesteps_host, coef_host, hist, x0_all, x_out, stream);
}

int edtts_sample_multistep_len(const EdttsDims* dims, const void* packed, void* workspace, int B, int T, int S, const int64_t* sem_idx,
                               const float* sem_features, const int64_t* t_len, const int64_t* s_len, const float* x_T, int num_steps,
                               const int64_t* timesteps_host, const float* coef_host, float* hist, float* x0_all, float* x_out,
                               void* stream) {
  const SettingsScope settings;
  Layout lo;
  TRY_G(make_layout(dims, &lo));
  if (!sem_idx && !sem_features) return fail(EDTTS_ERR_ARG, "Either sem_idx or sem_features must be provided");
  if (!packed || !workspace || !x_T || !timesteps_host || !coef_host || !hist || !x_out) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (num_steps < 1 || num_steps > lo.NSTEP)
    return fail(EDTTS_ERR_ARG, "num_steps=%d outside [1,%d] (step_emb rows; the reference raises IndexError)", num_steps, lo.NSTEP);
  TRY_G(check_shapes(lo, B, T, S));
  TRY_G(check_lms_modes(coef_host, num_steps));
  SamplerInputs in;
  in.t_host = timesteps_host; in.sem_idx = sem_idx; in.sem_features = sem_features;
  in.ln = Lens{t_len, s_len};
  in.x_T = x_T; in.x = x_out;
  const size_t per = (size_t)B * T * lo.MEL;
  return run_sampler(dims, lo, packed, workspace, B, T, S, num_steps, in, stream, [&](int i, int, size_t o) {
    StepTail tail;
    tail.kind = TAIL_LMS; tail.x_prev = x_out + o;
    tail.lms = lms_step_args(coef_host + 8 * i, hist, x0_all, per, i, o);
    return tail;
  });
}

int edtts_sample_ddpm(const EdttsDims* dims, const void* packed, void* workspace, int B, int S, const int64_t* sem_idx,
                      const float* x_T, int num_steps, const int64_t* t_all, const float* coef_host, const float* noise_all,
                      uint64_t seed, int64_t batch_offset, float* x_out, void* stream) {
  return edtts_sample_ddpm_len(dims, packed, workspace, B, S, sem_idx, nullptr, x_T, num_steps, t_all, coef_host, noise_all, seed,
                               batch_offset, x_out, stream);
}

int edtts_sample_ddpm_len(const EdttsDims* dims, const void* packed, void* workspace, int B, int S, const int64_t* sem_idx,
                          const int64_t* s_len, const float* x_T, int num_steps, const int64_t* t_all, const float* coef_host,
                          const float* noise_all, uint64_t seed, int64_t batch_offset, float* x_out, void* stream) {
  const SettingsScope settings;
  Layout lo;
  TRY_G(make_layout(dims, &lo));
  if (!packed || !workspace || !sem_idx || !x_T || !t_all || !coef_host || !x_out) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (num_steps < 1) return fail(EDTTS_ERR_ARG, "num_steps=%d < 1", num_steps);
  if (batch_offset < 0) return fail(EDTTS_ERR_ARG, "batch_offset=%lld < 0", (long long)batch_offset);
  const int T = 2 * S;
  TRY_G(check_shapes(lo, B, T, S));
  SamplerInputs in;
  in.t_dev = t_all; in.sem_idx = sem_idx;  // step_idx = None (train.py:155 usage)
  in.ln = Lens{s_len, s_len, true};  // frames = 2 x tokens
  in.x_T = x_T; in.x = x_out;
  const size_t per_step = (size_t)B * T * lo.MEL;
  return run_sampler(dims, lo, packed, workspace, B, T, S, num_steps, in, stream, [&](int i, int off, size_t o) {
    StepTail tail;
    tail.kind = TAIL_DDPM; tail.x_prev = x_out + o; tail.coef = coef_host + 3 * i;
    tail.ddpm = DdpmStepArgs{noise_all ? noise_all + (size_t)i * per_step + o : nullptr, (unsigned long long)seed,
                             ((unsigned long long)batch_offset + (unsigned long long)off) * T * lo.MEL, kStreamDdpmStep + (unsigned)i};
    return tail;
  });
}

int edtts_sample_inpaint(const EdttsDims* dims, const void* packed, void* workspace, void* workspace_uncond, int B, int T, int S,
                         const float* sem_features, const float* zero_features, float* x, int num_steps,
                         const int64_t* t_all, const int64_t* step_all, const float* coef_host, const float* known_mel, int overlap_len,
                         const float* noise_k, uint64_t seed, float cfg_scale, float* v_uncond, void* stream) {
  return edtts_sample_inpaint_len(dims, packed, workspace, workspace_uncond, B, T, S, sem_features, zero_features, x, num_steps, t_all,
                                  step_all, coef_host, known_mel, overlap_len, noise_k, seed, cfg_scale, v_uncond, nullptr, nullptr, nullptr,
                                  stream);
}

int edtts_sample_inpaint_len(const EdttsDims* dims, const void* packed, void* workspace, void* workspace_uncond, int B, int T, int S,
                             const float* sem_features, const float* zero_features, float* x, int num_steps,
                             const int64_t* t_all, const int64_t* step_all, const float* coef_host, const float* known_mel,
                             int overlap_len, const float* noise_k, uint64_t seed, float cfg_scale, float* v_uncond,
                             const int64_t* t_len, const int64_t* s_len, const uint64_t* seeds, void* stream) {
  const SettingsScope settings;
  Layout lo;
  TRY_G(make_layout(dims, &lo));
  const InpaintArgs a{dims, packed, workspace, workspace_uncond, B, T, S, sem_features, zero_features, x, num_steps, t_all, step_all,
                      coef_host, known_mel, overlap_len, noise_k, seed, cfg_scale, v_uncond, t_len, s_len, seeds, stream};
  // coef_host rows: {sqrt_ab[t], sqrt_1mab[t], sqrt(ab[t_next]), sqrt(1 - ab[t_next])}
  return run_inpaint(
      a, lo, true, [] { return EDTTS_OK; },
      [&](int i) -> int {  // q_sample(known_mel, t) into the first overlap_len frames (inference_pipeline.py:117-123)
        launch_inject(a, lo.MEL, coef_host[4 * i], coef_host[4 * i + 1], i);
        LAUNCH_CHECK("k_inpaint_inject");
        return EDTTS_OK;
      },
      [&](int i) {
        const float* k = coef_host + 4 * i;
        StepTail tail;
        tail.kind = TAIL_VPRED; tail.x_prev = x;
        tail.vp = VpredStepArgs{{k[0], k[1], k[2], k[3], cfg_scale}, nullptr};
        return tail;
      },
      [&]() -> int {  // final force (inference_pipeline.py:135-136)
        launch_inject(a, lo.MEL, 1.0f, 0.0f, 0);
        LAUNCH_CHECK("k_inpaint_inject");
        return EDTTS_OK;
      });
}

int edtts_sample_inpaint_multistep_len(const EdttsDims* dims, const void* packed, void* workspace, void* workspace_uncond, int B, int T,
                                       int S, const float* sem_features, const float* zero_features, float* x, int num_steps,
                                       const int64_t* t_all, const int64_t* step_all, const float* coef_host, const float* known_mel,
                                       int overlap_len, const float* noise_k, uint64_t seed, float cfg_scale, float* v_uncond,
                                       const int64_t* t_len, const int64_t* s_len, const uint64_t* seeds, float* hist, float* x0_all,
                                       void* stream) {
  const SettingsScope settings;
  Layout lo;
  TRY_G(make_layout(dims, &lo));
  const InpaintArgs a{dims, packed, workspace, workspace_uncond, B, T, S, sem_features, zero_features, x, num_steps, t_all, step_all,
                      coef_host, known_mel, overlap_len, noise_k, seed, cfg_scale, v_uncond, t_len, s_len, seeds, stream};
  const size_t per = (size_t)B * T * lo.MEL, per_k = (size_t)B * overlap_len * lo.MEL;
  // q_sample's scalars of step i are in its coefficient row: p0 = sqrt_ab[t_i], p1 = -sqrt_1mab[t_i] (v-prediction rows)
  auto c_known = [&](int i) { return coef_host[8 * i + 1]; };
  auto c_noise = [&](int i) { return -coef_host[8 * i + 2]; };
  return run_inpaint(
      a, lo, hist != nullptr, [&] { return check_lms_modes(coef_host, num_steps); },
      [&](int i) -> int {  // step 0's q_sample of the known frames; every later one is written by the tail of the step before it
        if (i > 0) return EDTTS_OK;
        launch_inject(a, lo.MEL, c_known(0), c_noise(0), 0);
        LAUNCH_CHECK("k_inpaint_inject");
        return EDTTS_OK;
      },
      [&](int i) {
        StepTail tail;
        tail.kind = TAIL_VLMS; tail.x_prev = x;
        tail.lms = lms_step_args(coef_host + 8 * i, hist, x0_all, per, i, 0);
        tail.vp.k.cfg = cfg_scale;
        if (known_mel) {  // (whole float4s; a known block that is not made of them goes through the generic path's per-element tail)
          const bool last = i + 1 == num_steps;  // after the last step: the known frames themselves (inference_pipeline.py:135-136)
          tail.blend = BlendStepArgs{known_mel, (noise_k && !last) ? noise_k + (size_t)(i + 1) * per_k : nullptr, overlap_len, lo.MEL,
                                     last ? 1.0f : c_known(i + 1), last ? 0.0f : c_noise(i + 1),
                                     (unsigned long long)seed, reinterpret_cast<const unsigned long long*>(seeds),
                                     kStreamInpaintStep + (unsigned)(last ? 0 : i + 1)};
        }
        return tail;
      },
      [] { return EDTTS_OK; });
}

int edtts_sample_inpaint_mask_len(const EdttsDims* dims, const void* packed, void* workspace, void* workspace_uncond, int B, int T, int S,
                                  const float* sem_features, const float* zero_features, float* x, int num_steps,
                                  const int64_t* t_all, const int64_t* step_all, const float* coef_host, const float* known_mel,
                                  const uint8_t* keep, const float* noise_k, uint64_t seed, float cfg_scale, float* v_uncond,
                                  const int64_t* t_len, const int64_t* s_len, const uint64_t* seeds, void* stream) {
  const SettingsScope settings;
  Layout lo;
  TRY_G(make_layout(dims, &lo));
  TRY_G(check_mask_args(known_mel, keep));
  const InpaintArgs a{dims, packed, workspace, workspace_uncond, B, T, S, sem_features, zero_features, x, num_steps, t_all, step_all,
                      coef_host, known_mel, 0, noise_k, seed, cfg_scale, v_uncond, t_len, s_len, seeds, stream, keep};
  return run_inpaint(
      a, lo, true, [] { return EDTTS_OK; },
      [&](int i) -> int {  // q_sample(known_mel, t) into the kept frames
        launch_inject_mask(a, lo.MEL, coef_host[4 * i], coef_host[4 * i + 1], i);
        LAUNCH_CHECK("k_inpaint_inject_mask");
        return EDTTS_OK;
      },
      [&](int i) {
        const float* k = coef_host + 4 * i;
        StepTail tail;
        tail.kind = TAIL_VPRED; tail.x_prev = x;
        tail.vp = VpredStepArgs{{k[0], k[1], k[2], k[3], cfg_scale}, nullptr};
        return tail;
      },
      [&]() -> int {  // final force
        launch_inject_mask(a, lo.MEL, 1.0f, 0.0f, 0);
        LAUNCH_CHECK("k_inpaint_inject_mask");
        return EDTTS_OK;
      });
}

int edtts_sample_inpaint_multistep_mask_len(const EdttsDims* dims, const void* packed, void* workspace, void* workspace_uncond, int B,
                                            int T, int S, const float* sem_features, const float* zero_features, float* x, int num_steps,
                                            const int64_t* t_all, const int64_t* step_all, const float* coef_host, const float* known_mel,
                                            const uint8_t* keep, const float* noise_k, uint64_t seed, float cfg_scale, float* v_uncond,
                                            const int64_t* t_len, const int64_t* s_len, const uint64_t* seeds, float* hist, float* x0_all,
                                            void* stream) {
  const SettingsScope settings;
  Layout lo;
  TRY_G(make_layout(dims, &lo));
  TRY_G(check_mask_args(known_mel, keep));
  const InpaintArgs a{dims, packed, workspace, workspace_uncond, B, T, S, sem_features, zero_features, x, num_steps, t_all, step_all,
                      coef_host, known_mel, 0, noise_k, seed, cfg_scale, v_uncond, t_len, s_len, seeds, stream, keep};
  const size_t per = (size_t)B * T * lo.MEL;
  return run_inpaint(
      a, lo, hist != nullptr, [&] { return check_lms_modes(coef_host, num_steps); },
      [&](int i) -> int {  // every step's q_sample is a launch of its own: the tails carry no blend (their kernels know prefixes only)
        launch_inject_mask(a, lo.MEL, coef_host[8 * i + 1], -coef_host[8 * i + 2], i);
        LAUNCH_CHECK("k_inpaint_inject_mask");
        return EDTTS_OK;
      },
      [&](int i) {
        StepTail tail;
        tail.kind = TAIL_VLMS; tail.x_prev = x;
        tail.lms = lms_step_args(coef_host + 8 * i, hist, x0_all, per, i, 0);
        tail.vp.k.cfg = cfg_scale;
        return tail;
      },
      [&]() -> int {  // final force
        launch_inject_mask(a, lo.MEL, 1.0f, 0.0f, 0);
        LAUNCH_CHECK("k_inpaint_inject_mask");
        return EDTTS_OK;
      });
}

int edtts_ddim_step(const float* alpha_bar, int n_table, const float* x, const float* eps, const int64_t* t,
                    const int64_t* t_prev, int B, size_t n_per_batch, float eta, const float* noise, float* x_prev, float* x0,
                    void* stream) {
  if (!alpha_bar || !x || !eps || !t || !t_prev || !x_prev || !x0) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (eta > 0.f && !noise) return fail(EDTTS_ERR_ARG, "eta > 0 needs a noise tensor");
  if (B < 1 || n_per_batch < 1 || n_table < 1) return fail(EDTTS_ERR_ARG, "bad sizes");
  StepArgs a;
  memset(&a, 0, sizeof(a));
  a.alpha_bar = alpha_bar; a.n_table = n_table; a.x = x; a.eps = eps; a.t = t; a.t_prev = t_prev;
  a.n_per_batch = n_per_batch; a.eta = eta; a.noise = eta > 0.f ? noise : nullptr; a.x_prev = x_prev; a.x0 = x0;
  a.vec4 = step_vec4(n_per_batch, {x, eps, a.noise, x_prev, x0});
  hipLaunchKernelGGL(k_ddim, dim3(step_blocks(a), B), dim3(256), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK("k_ddim");
  return EDTTS_OK;
}

int edtts_ddpm_step(const float* alphas, const float* alpha_bar, const float* betas, const float* post_var, int n_table,
                    const float* x, const float* eps, const int64_t* t, int B, size_t n_per_batch, const float* noise,
                    float* x_prev, void* stream) {
  if (!alphas || !alpha_bar || !betas || !post_var || !x || !eps || !t || !noise || !x_prev) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (B < 1 || n_per_batch < 1 || n_table < 1) return fail(EDTTS_ERR_ARG, "bad sizes");
  StepArgs a;
  memset(&a, 0, sizeof(a));
  a.alphas = alphas; a.alpha_bar = alpha_bar; a.betas = betas; a.post_var = post_var; a.n_table = n_table;
  a.x = x; a.eps = eps; a.t = t; a.n_per_batch = n_per_batch; a.noise = noise; a.x_prev = x_prev;
  a.vec4 = step_vec4(n_per_batch, {x, eps, noise, x_prev});
  hipLaunchKernelGGL(k_ddpm, dim3(step_blocks(a), B), dim3(256), 0, (hipStream_t)stream, a);
  LAUNCH_CHECK("k_ddpm");
  return EDTTS_OK;
}

int edtts_randn(float* out, size_t n, uint64_t seed, uint32_t stream_id, uint64_t elem_offset, float scale, void* stream) {
  if ((n & 3) || (elem_offset & 3)) return fail(EDTTS_ERR_ARG, "n=%zu and elem_offset=%llu must be multiples of 4", n, (unsigned long long)elem_offset);
  if (stream_id >= kStreamDdpmStep) return fail(EDTTS_ERR_ARG, "stream_id %u is reserved for the samplers' per-step draws (>= 0x10000)", stream_id);
  if (n == 0) return EDTTS_OK;  // an empty shard (fewer utterances than ranks): its zero-element tensor has a NULL data pointer
  if (!out) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if ((uintptr_t)out & 15) return fail(EDTTS_ERR_ARG, "out must be 16-byte aligned");
  size_t bx = (n / 4 + 255) / 256;
  if (bx > 4096) bx = 4096;
  hipLaunchKernelGGL(k_randn, dim3((unsigned)bx), dim3(256), 0, (hipStream_t)stream, out, n, (unsigned long long)seed, (unsigned)stream_id,
                     (unsigned long long)elem_offset, scale);
  LAUNCH_CHECK("k_randn");
  return EDTTS_OK;
}

int edtts_randn_rows(float* out, int B, size_t n_per_row, const uint64_t* seeds, uint32_t stream_id, float scale, void* stream) {
  if (B < 0) return fail(EDTTS_ERR_ARG, "B=%d < 0", B);
  if (stream_id >= kStreamDdpmStep) return fail(EDTTS_ERR_ARG, "stream_id %u is reserved for the samplers' per-step draws (>= 0x10000)", stream_id);
  if (B == 0 || n_per_row == 0) return EDTTS_OK;
  if (!out || !seeds) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if ((n_per_row & 3) == 0 && ((uintptr_t)out & 15)) return fail(EDTTS_ERR_ARG, "out must be 16-byte aligned");
  const size_t nq = (size_t)B * ((n_per_row + 3) / 4);
  size_t bx = (nq + 255) / 256;
  if (bx > 4096) bx = 4096;
  hipLaunchKernelGGL(k_randn_rows, dim3((unsigned)bx), dim3(256), 0, (hipStream_t)stream, out, B, n_per_row,
                     reinterpret_cast<const unsigned long long*>(seeds), (unsigned)stream_id, scale);
  LAUNCH_CHECK("k_randn_rows");
  return EDTTS_OK;
}

}  // extern "C"
