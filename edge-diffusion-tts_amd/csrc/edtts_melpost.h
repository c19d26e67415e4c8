// edtts_melpost.h -- mel post-processing kernels: the step right after the sampler in the
// reference's scripts (generate_sample.py:115-145, inference_pipeline.py:382-396): denormalize_mel (utils/audio.py:17-19) -> exp
// -> torchaudio InverseMelScale (minimum-norm least squares = multiplication by the pseudo-inverse of the mel filter bank, relu)
// -> torchaudio GriffinLim (n_iter x [istft -> stft -> momentum phase update], final istft).  Included by edtts_kernels.hip, behind
// launch_len_check, which the launchers and the C ABI at the end of this file (edtts_mel_to_spec*, edtts_griffin_lim*) call.
//
// Bounds: the inverse-mel product is a small GEMM ([513 x 80] per frame: 82 kFLOP/frame, HBM traffic 320 B in / 2 KB out per
// frame); Griffin-Lim is FFT-bound: per iteration and frame one 1024-point inverse and one forward complex FFT (2 x 51 kFLOP, in
// fp64: see cplxd below) in LDS plus 4 KB (frame buffer) + 8 KB (phase state) + 4 KB (spectrum) of HBM traffic -> ~25 FLOP/B: HBM-bound on MI355X
// (ridge 20 FLOP/B for fp32 vector math); the iteration state is laid out frame-major so that every access is a contiguous row.
//
// Ragged batches (edtts_mel_to_spec_len, edtts_griffin_lim_len): rows padded to a common T carry their own frame
// count T_b = t_len[b] (clamped into [1, T]; nullptr = T for every row, today's behaviour).  A block of a frame t >= T_b leaves before
// its first barrier (the whole block takes that branch), the overlap-add and the reflect padding end at the row's own last frame, and
// the library-drawn phases hash the row's solo element index f T_b + t with the row's own seed, so row b is bitwise the call on
// spec[b, :, :T_b] alone.  Strides stay those of the padded batch; the state of padded frames is neither written nor read.
// k_mel_to_spec_smooth is k_mel_to_spec for linear-mel input behind a kh x kw box filter (the reference's long-form tail,
// inference_pipeline.py:376-399: F.avg_pool2d(lin_mel, (5, 3), stride=1, padding=(2, 1)), count_include_pad), the row's own end
// being the filter's edge.
namespace melpost {
using namespace edtts;

constexpr int kNfft = 1024, kBins = kNfft / 2 + 1, kThreads = 256;

struct cplx {
  float re, im;
};
// The two transforms of Griffin-Lim run in fp64 between their fp32 operands and their fp32 results: the phase
// update divides by |a|, so a bin of the rebuilt spectrum far below its row's level turns the transforms' own rounding into a phase
// error 1 / |a| times as large.  In fp64 what is left is the rounding of the stored operands.
struct cplxd {
  double re, im;
};
EDTTS_DEV cplxd cmul(cplxd a, cplxd b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

// tw[q] = exp(-2 pi i q / 1024), q < 512, in fp64 in the block's LDS (the fp32 host table would put an fp32 rounding back into every
// butterfly): thread tid evaluates q = tid and derives q + 256 = q turned by -i.  Visible after fft1024's first barrier.
EDTTS_DEV void twiddle64(cplxd* tw, int tid) {
  double s, c;
  sincospi(-(double)tid * (1.0 / (kNfft / 2)), &s, &c);
  tw[tid] = {c, s};
  tw[tid + kThreads] = {s, -c};
}

// 1024-point complex FFT in LDS, radix-2 Stockham autosort (natural order in and out), 256 threads x 2 butterflies per stage.
// tw: twiddle64's table; INV conjugates it (no 1/N scaling here).
// x holds the input; returns the buffer (x or y) that holds the result.  Callers synchronise before reading.
template <bool INV>
EDTTS_DEV cplxd* fft1024(cplxd* x, cplxd* y, const cplxd* tw, int tid) {
  constexpr int N = kNfft, T = N / 2;
#pragma unroll 1
  for (int p = 1; p < N; p <<= 1) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = tid + u * kThreads;      // butterfly index in [0, 512)
      const int k = i & (p - 1);
      const int j = ((i - k) << 1) + k;
      cplxd w = tw[k * (T / p)];             // exp(-i pi k / p)
      if (INV) w.im = -w.im;
      const cplxd u0 = x[i], u1 = cmul(w, x[i + T]);
      y[j] = {u0.re + u1.re, u0.im + u1.im};
      y[j + p] = {u0.re - u1.re, u0.im - u1.im};
    }
    cplxd* t = x; x = y; y = t;
  }
  __syncthreads();
  return x;
}

constexpr int kSmoothMax = 9, kSmoothMaxMels = 256;  // box filter sides (odd) and mel bins of k_mel_to_spec_smooth (LDS: 40 x n_mels floats)

// The inverse-mel product of one 16-frame tile staged in LDS (lin [16][M]): thread -> (frequency f, 16 frames), the 16 outputs of a
// frequency being contiguous in the [.., f, t] layout
EDTTS_DEV void mel_pinv_tile(const float* lin, const float* __restrict__ pinv, int b, int t0, int T, int M, int NFQ, float* __restrict__ spec) {
  for (int f = threadIdx.x; f < NFQ; f += kThreads) {
    float acc[16];
#pragma unroll
    for (int tl = 0; tl < 16; ++tl) acc[tl] = 0.f;
    const float* pr = pinv + (size_t)f * M;
    for (int m = 0; m < M; ++m) {
      const float w = pr[m];
#pragma unroll
      for (int tl = 0; tl < 16; ++tl) acc[tl] = fmaf(w, lin[tl * M + m], acc[tl]);
    }
    float* o = spec + ((size_t)b * NFQ + f) * T + t0;
#pragma unroll
    for (int tl = 0; tl < 16; ++tl)
      if (t0 + tl < T) o[tl] = fmaxf(acc[tl], 0.f);
  }
}

// spec[b][f][t] = relu(sum_m pinv[f][m] * lin[b][t][m]),  lin = exp(mel_n * std + mean) or the input itself   (torch layout [B, n_freqs, T])
// t_len: frames t >= t_len[b] are staged as 0 and so written as 0 (their input is never read)
__global__ __launch_bounds__(kThreads) void k_mel_to_spec(const float* __restrict__ mel, const float* __restrict__ mean, const float* __restrict__ stdv,
                                                          const float* __restrict__ pinv, int T, int M, int NFQ, const int64_t* __restrict__ t_len,
                                                          float* __restrict__ spec) {
  extern __shared__ float lin[];  // [16 frames][M]
  const int b = blockIdx.y, t0 = blockIdx.x * 16;
  const int Tb = utt_len(t_len, b, T);
  for (int i = threadIdx.x; i < 16 * M; i += kThreads) {
    const int tl = i / M, m = i % M, t = t0 + tl;
    float v = 0.f;
    if (t < Tb) {
      v = mel[((size_t)b * T + t) * M + m];
      // normalised log-mel in (mean / std given): denormalise (utils/audio.py:19) and leave the log domain (generate_sample.py:119);
      // otherwise the input already is the linear mel spectrogram (plain torchaudio InverseMelScale semantics)
      if (stdv) v = expf(v * stdv[(size_t)b * M + m] + mean[(size_t)b * M + m]);
    }
    lin[i] = v;
  }
  __syncthreads();
  mel_pinv_tile(lin, pinv, b, t0, T, M, NFQ, spec);
}

// ... of the box-filtered linear mel: sm[t][m] = (1 / (kh kw)) sum_{|dm| <= kh/2, |dt| <= kw/2} lin[t + dt][m + dm], zeros outside
// 0 <= m < M, 0 <= t < T_b (avg_pool2d, stride 1, padding (kh/2, kw/2), count_include_pad); kh, kw odd, <= kSmoothMax.  The tile is
// staged with its frame halo; the sum runs dm-major, dt-minor in ascending order (one fixed chain per element).
__global__ __launch_bounds__(kThreads) void k_mel_to_spec_smooth(const float* __restrict__ mel, const float* __restrict__ pinv, int T, int M, int NFQ,
                                                                 const int64_t* __restrict__ t_len, int kh, int kw, float* __restrict__ spec) {
  extern __shared__ float lin[];  // [16 frames][M] smoothed | [16 + kw - 1 frames][M] raw
  float* raw = lin + 16 * M;
  const int b = blockIdx.y, t0 = blockIdx.x * 16, hh = kh >> 1, hw = kw >> 1;
  const int Tb = utt_len(t_len, b, T);
  for (int i = threadIdx.x; i < (16 + 2 * hw) * M; i += kThreads) {
    const int t = t0 - hw + i / M;
    raw[i] = t >= 0 && t < Tb ? mel[((size_t)b * T + t) * M + i % M] : 0.f;
  }
  __syncthreads();
  const float scale = 1.0f / (float)(kh * kw);
  for (int i = threadIdx.x; i < 16 * M; i += kThreads) {
    const int tl = i / M, m = i % M;
    float s = 0.f;
    if (t0 + tl < Tb) {
      const int m_lo = m - hh < 0 ? 0 : m - hh, m_hi = m + hh > M - 1 ? M - 1 : m + hh;
      for (int mm = m_lo; mm <= m_hi; ++mm)
        for (int dt = 0; dt <= 2 * hw; ++dt) s += raw[(tl + dt) * M + mm];
      s *= scale;
    }
    lin[i] = s;
  }
  __syncthreads();
  mel_pinv_tile(lin, pinv, b, t0, T, M, NFQ, spec);
}

// mag[b][t][f] = spec[b][f][t] ^ (1 / power); angles[b][t][f] = angles0 (torch layout [B, n_freqs, T] complex) or uniform draws
// t_len: the draws of row b are keyed by (seeds[b], f T_b + t), the element index of the row's solo call (B = 1, T = T_b)
__global__ __launch_bounds__(kThreads) void k_gl_init(const float* __restrict__ spec, const float* __restrict__ angles0, int T, float inv_power,
                                                      unsigned long long seed, const int64_t* __restrict__ t_len,
                                                      const unsigned long long* __restrict__ seeds, float* __restrict__ mag, cplx* __restrict__ ang,
                                                      cplx* __restrict__ tprev) {
  const int b = blockIdx.y, t = blockIdx.x;
  const int Tb = utt_len(t_len, b, T);
  if (t >= Tb) return;
  for (int f = threadIdx.x; f < kBins; f += kThreads) {
    const size_t src = ((size_t)b * kBins + f) * T + t, dst = ((size_t)b * T + t) * kBins + f;
    const float s = spec[src];
    mag[dst] = inv_power == 0.5f ? sqrtf(s) : powf(s, inv_power);
    cplx a;
    if (angles0) a = {angles0[2 * src], angles0[2 * src + 1]};
    else {  // torch.rand(complex): real and imaginary parts uniform in [0, 1)
      // counter hash (splitmix64 of (seed, element)) -> two 24-bit uniforms; the reference's draw comes from torch's global RNG
      const unsigned long long sd = t_len ? seeds[b] : seed, el = t_len ? (unsigned long long)f * Tb + t : (unsigned long long)src;
      unsigned long long z = (sd ^ 0x9E3779B97F4A7C15ull) + el * 0xBF58476D1CE4E5B9ull;
      z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
      a = {(float)(unsigned)(z >> 40) * (1.0f / 16777216.0f), (float)(unsigned)((z >> 16) & 0xFFFFFF) * (1.0f / 16777216.0f)};
    }
    ang[dst] = a;
    tprev[dst] = {0.f, 0.f};
  }
}

// frames[b][t][n] = window[n] * irfft(mag * angles)[n]      (torch.istft: per-frame inverse real FFT, "backward" normalisation)
__global__ __launch_bounds__(kThreads) void k_gl_istft(const float* __restrict__ mag, const cplx* __restrict__ ang, const float* __restrict__ window,
                                                       int T, const int64_t* __restrict__ t_len, float* __restrict__ frames) {
  __shared__ cplxd bufa[kNfft], bufb[kNfft], tw[kNfft / 2];  // 40 KB
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  if (t >= utt_len(t_len, b, T)) return;  // a padded frame: the whole block leaves before the first barrier
  twiddle64(tw, tid);
  const size_t row = ((size_t)b * T + t) * kBins;
  for (int f = tid; f < kBins; f += kThreads) {
    const double m = mag[row + f];
    cplxd v = {m * ang[row + f].re, m * ang[row + f].im};  // exact: products of two fp32 values
    if (f == 0 || f == kNfft / 2) v.im = 0.0;  // a real signal's DC / Nyquist bins (irfft ignores their imaginary parts)
    bufa[f] = v;
    if (f > 0 && f < kNfft / 2) bufa[kNfft - f] = {v.re, -v.im};  // Hermitian extension
  }
  cplxd* r = fft1024<true>(bufa, bufb, tw, tid);
  float* out = frames + ((size_t)b * T + t) * kNfft;
  for (int n = tid; n < kNfft; n += kThreads) out[n] = (float)(r[n].re * (1.0 / kNfft) * window[n]);
}

// wave[b][p] = sum_t frames[b][t][p - t hop] / sum_t window^2[p - t hop]   over the frames that cover padded position p
// (torch.istft overlap-add and window-envelope normalisation; ascending t: deterministic)
// t_len: row b's padded signal is Lp_b = n_fft + hop (T_b - 1) long (row stride Lp); positions past it are left alone
__global__ __launch_bounds__(kThreads) void k_gl_ola(const float* __restrict__ frames, const float* __restrict__ window, int T, int hop, int Lp,
                                                     const int64_t* __restrict__ t_len, float* __restrict__ wave) {
  const int b = blockIdx.y;
  const int Tb = utt_len(t_len, b, T), Lpb = kNfft + hop * (Tb - 1);
  for (int p = blockIdx.x * kThreads + threadIdx.x; p < Lpb; p += gridDim.x * kThreads) {
    int t_lo = (p - (kNfft - 1) + hop - 1) / hop;
    if (p - (kNfft - 1) < 0) t_lo = 0;
    int t_hi = p / hop;
    if (t_hi > Tb - 1) t_hi = Tb - 1;
    float s = 0.f, e = 0.f;
    for (int t = t_lo; t <= t_hi; ++t) {
      const int n = p - t * hop;
      s += frames[((size_t)b * T + t) * kNfft + n];
      const float w = window[n];
      e = fmaf(w, w, e);
    }
    wave[(size_t)b * Lp + p] = e > 1e-11f ? s / e : 0.f;
  }
}

// rebuilt = stft(x, center=True, reflect), x = wave[n_fft/2 : n_fft/2 + Lx];  then the momentum phase update
//   a = rebuilt - mom * tprev;  angles = a / (|a| + 1e-16);  tprev = rebuilt          (torchaudio.functional.griffinlim)
__global__ __launch_bounds__(kThreads) void k_gl_stft(const float* __restrict__ wave, const float* __restrict__ window, int T, int hop, int Lp,
                                                      float mom, const int64_t* __restrict__ t_len, cplx* __restrict__ ang,
                                                      cplx* __restrict__ tprev) {
  __shared__ cplxd bufa[kNfft], bufb[kNfft], tw[kNfft / 2];  // 40 KB
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int Tb = utt_len(t_len, b, T);
  if (t >= Tb) return;  // a padded frame: the whole block leaves before the first barrier
  twiddle64(tw, tid);
  const int Lx = hop * (Tb - 1);  // the row's own signal: the reflection is at its own end
  const float* x = wave + (size_t)b * Lp + kNfft / 2;
  for (int n = tid; n < kNfft; n += kThreads) {
    int idx = t * hop + n - kNfft / 2;
    if (idx < 0) idx = -idx;
    if (idx >= Lx) idx = 2 * (Lx - 1) - idx;
    idx = idx < 0 ? 0 : idx;  // (signals shorter than the pad are not supported by torch either)
    bufa[n] = {(double)x[idx] * window[n], 0.0};  // exact
  }
  cplxd* r = fft1024<false>(bufa, bufb, tw, tid);
  const size_t row = ((size_t)b * T + t) * kBins;
  for (int f = tid; f < kBins; f += kThreads) {
    const cplx rb = {(float)r[f].re, (float)r[f].im}, tp = tprev[row + f];  // the update reads what tprev will hold
    const cplx a = {rb.re - mom * tp.re, rb.im - mom * tp.im};
    const float inv = 1.0f / (sqrtf(a.re * a.re + a.im * a.im) + 1e-16f);
    ang[row + f] = {a.re * inv, a.im * inv};
    tprev[row + f] = rb;
  }
}

// wave_out[b][i] = wave[b][n_fft / 2 + i] for i < hop (T_b - 1), 0 behind it (torch.istft's trim of the centre padding, per row)
__global__ __launch_bounds__(kThreads) void k_gl_trim(const float* __restrict__ wave, int T, int hop, int Lp, const int64_t* __restrict__ t_len,
                                                      float* __restrict__ wave_out) {
  const int b = blockIdx.y, Lo = hop * (T - 1);
  const int Lxb = hop * (utt_len(t_len, b, T) - 1);
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < Lo; i += gridDim.x * kThreads)
    wave_out[(size_t)b * Lo + i] = i < Lxb ? wave[(size_t)b * Lp + kNfft / 2 + i] : 0.f;
}

}  // namespace melpost

// =========================================================================================================
// launchers and the C ABI
// =========================================================================================================
// The index-error word of the mel post-processing *_len entry points: one device uint32 the caller owns (read and cleared by
// edtts_index_errors, like Workspace::err); rows whose frame count is outside [t_min, T] set EDTTS_IDX_LEN in it.
static int melpost_len_check(const int64_t* t_len, int B, int T, int t_min, void* idx_err, hipStream_t st) {
  if (!t_len || !idx_err) return EDTTS_OK;
  return launch_len_check(t_len, nullptr, B, T, 0, reinterpret_cast<float*>(idx_err), st, t_min);
}

// Both Griffin-Lim entry points.  t_len == nullptr: every row has T frames, the draws are keyed by (seed, element of the batch).
// twiddle (the fp32 table exp(-2 pi i q / n_fft), q < n_fft / 2) stays in the ABI and is checked, but is no longer read: the
// transforms run in fp64 and build their table themselves (twiddle64).
static int griffin_lim_run(const float* spec, int B, int T, int n_fft, int hop, const float* window, const float* twiddle, int n_iter,
                           float momentum, float power, const float* angles0, uint64_t seed, const int64_t* t_len, const uint64_t* seeds,
                           void* idx_err, float* scratch, float* wave_out, void* stream) {
  if (!spec || !window || !twiddle || !scratch || !wave_out) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (B < 1 || T < 2 || hop < 1 || hop > n_fft || n_iter < 0 || power <= 0.f) return fail(EDTTS_ERR_ARG, "bad sizes");
  if (n_fft != melpost::kNfft) return fail(EDTTS_ERR_UNSUPPORTED, "n_fft=%d (compiled: %d, win_length = n_fft)", n_fft, melpost::kNfft);
  if (hop * (T - 1) <= n_fft / 2) return fail(EDTTS_ERR_ARG, "signal of %d samples is shorter than the reflect padding (torch.stft raises too)", hop * (T - 1));
  using namespace melpost;
  hipStream_t st = (hipStream_t)stream;
  // the shortest row the solo call accepts: hop (T_b - 1) > n_fft / 2; shorter device-side lengths are flagged (and only clamped into [1, T])
  TRY_G(melpost_len_check(t_len, B, T, (n_fft / 2) / hop + 2, idx_err, st));
  const size_t bt = (size_t)B * T;
  const int Lp = n_fft + hop * (T - 1);
  float* mag = scratch;
  cplx* ang = reinterpret_cast<cplx*>(mag + bt * kBins);
  cplx* tprev = ang + bt * kBins;
  float* frames = reinterpret_cast<float*>(tprev + bt * kBins);
  float* wave = frames + bt * n_fft;
  const float mom = momentum / (1.0f + momentum);
  hipLaunchKernelGGL(k_gl_init, dim3(T, B), dim3(kThreads), 0, st, spec, angles0, T, 1.0f / power, (unsigned long long)seed, t_len,
                     reinterpret_cast<const unsigned long long*>(seeds), mag, ang, tprev);
  LAUNCH_CHECK("k_gl_init");
  int gx = (Lp + kThreads - 1) / kThreads;
  for (int it = 0; it <= n_iter; ++it) {
    hipLaunchKernelGGL(k_gl_istft, dim3(T, B), dim3(kThreads), 0, st, mag, ang, window, T, t_len, frames);
    hipLaunchKernelGGL(k_gl_ola, dim3(gx, B), dim3(kThreads), 0, st, frames, window, T, hop, Lp, t_len, wave);
    if (it < n_iter) hipLaunchKernelGGL(k_gl_stft, dim3(T, B), dim3(kThreads), 0, st, wave, window, T, hop, Lp, mom, t_len, ang, tprev);
  }
  LAUNCH_CHECK("griffin-lim kernels");
  // torch.istft trims the centre padding: n_fft / 2 at the start, and (length = None) as much at the end
  if (t_len) {
    hipLaunchKernelGGL(k_gl_trim, dim3((hop * (T - 1) + kThreads - 1) / kThreads, B), dim3(kThreads), 0, st, wave, T, hop, Lp, t_len, wave_out);
    LAUNCH_CHECK("k_gl_trim");
    return EDTTS_OK;
  }
  HIP_TRY(hipMemcpy2DAsync(wave_out, (size_t)hop * (T - 1) * sizeof(float), wave + n_fft / 2, (size_t)Lp * sizeof(float),
                           (size_t)hop * (T - 1) * sizeof(float), B, hipMemcpyDeviceToDevice, st));
  return EDTTS_OK;
}

extern "C" {

int edtts_mel_to_spec(const float* mel_n, const float* mean, const float* stdv, const float* pinv, int B, int T, int n_mels, int n_freqs,
                      float* spec, void* stream) {
  return edtts_mel_to_spec_len(mel_n, mean, stdv, pinv, B, T, n_mels, n_freqs, nullptr, 0, 0, nullptr, spec, stream);
}

int edtts_mel_to_spec_len(const float* mel_n, const float* mean, const float* stdv, const float* pinv, int B, int T, int n_mels, int n_freqs,
                          const int64_t* t_len, int smooth_h, int smooth_w, void* idx_err, float* spec, void* stream) {
  if (!mel_n || !pinv || !spec || (!mean != !stdv)) return fail(EDTTS_ERR_ARG, "NULL pointer argument (mean and std come together)");
  if (B < 1 || T < 1 || n_mels < 1 || n_freqs < 1 || n_mels > 512) return fail(EDTTS_ERR_ARG, "bad sizes");
  const bool smooth = smooth_h != 0 || smooth_w != 0;
  if (smooth) {
    if (smooth_h < 1 || smooth_w < 1 || !(smooth_h & 1) || !(smooth_w & 1) || smooth_h > melpost::kSmoothMax || smooth_w > melpost::kSmoothMax)
      return fail(EDTTS_ERR_ARG, "smooth %d x %d: the box filter's sides are odd and in [1, %d] (0 x 0: none)", smooth_h, smooth_w,
                  melpost::kSmoothMax);
    if (mean) return fail(EDTTS_ERR_ARG, "smoothing takes the linear mel spectrogram (mean and std NULL)");
    if (n_mels > melpost::kSmoothMaxMels) return fail(EDTTS_ERR_ARG, "smoothing is built for n_mels <= %d, got %d", melpost::kSmoothMaxMels, n_mels);
  }
  hipStream_t st = (hipStream_t)stream;
  TRY_G(melpost_len_check(t_len, B, T, 1, idx_err, st));
  const dim3 grid((T + 15) / 16, B);
  if (smooth) {
    hipLaunchKernelGGL(melpost::k_mel_to_spec_smooth, grid, dim3(melpost::kThreads), (size_t)(32 + smooth_w - 1) * n_mels * sizeof(float), st, mel_n,
                       pinv, T, n_mels, n_freqs, t_len, smooth_h, smooth_w, spec);
    LAUNCH_CHECK("k_mel_to_spec_smooth");
  } else {
    hipLaunchKernelGGL(melpost::k_mel_to_spec, grid, dim3(melpost::kThreads), 16 * n_mels * sizeof(float), st, mel_n, mean, stdv, pinv, T, n_mels,
                       n_freqs, t_len, spec);
    LAUNCH_CHECK("k_mel_to_spec");
  }
  return EDTTS_OK;
}

int edtts_griffin_lim_scratch_floats(int B, int T, int n_fft, int hop, size_t* out_floats) {
  if (!out_floats || B < 1 || T < 2 || hop < 1) return fail(EDTTS_ERR_ARG, "bad sizes");
  if (n_fft != melpost::kNfft) return fail(EDTTS_ERR_UNSUPPORTED, "n_fft=%d (compiled: %d)", n_fft, melpost::kNfft);
  const size_t bt = (size_t)B * T, Lp = (size_t)n_fft + (size_t)hop * (T - 1);
  *out_floats = bt * melpost::kBins * 5 + bt * n_fft + (size_t)B * Lp;  // mag | angles | tprev | frames | padded signal
  return EDTTS_OK;
}

int edtts_griffin_lim(const float* spec, int B, int T, int n_fft, int hop, const float* window, const float* twiddle, int n_iter,
                      float momentum, float power, const float* angles0, uint64_t seed, float* scratch, float* wave_out, void* stream) {
  return griffin_lim_run(spec, B, T, n_fft, hop, window, twiddle, n_iter, momentum, power, angles0, seed, nullptr, nullptr, nullptr, scratch,
                         wave_out, stream);
}

int edtts_griffin_lim_len(const float* spec, int B, int T, int n_fft, int hop, const float* window, const float* twiddle, int n_iter,
                          float momentum, float power, const float* angles0, const int64_t* t_len, const uint64_t* seeds, void* idx_err,
                          float* scratch, float* wave_out, void* stream) {
  if (!t_len) return fail(EDTTS_ERR_ARG, "t_len is NULL (edtts_griffin_lim is the call without lengths)");
  if (!angles0 && !seeds) return fail(EDTTS_ERR_ARG, "seeds is NULL: without angles0, t_len and seeds come together");
  return griffin_lim_run(spec, B, T, n_fft, hop, window, twiddle, n_iter, momentum, power, angles0, 0, t_len, seeds, idx_err, scratch, wave_out,
                         stream);
}

}  // extern "C"
