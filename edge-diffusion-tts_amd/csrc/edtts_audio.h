// edtts_audio.h -- the analysis side of the mel and the resampler in front of it (included by edtts_kernels.hip): what the reference
// takes from torchaudio at every entry point (generate_sample.py:75-116, data/collate.py:34-60, inference_pipeline.py:206-207, 354-355).
//
//   k_mel_frames        MelSpectrogram(n_fft = 1024, center, reflect, periodic Hann, HTK bank, norm None) per frame, one wave per
//                       frame: the power (or magnitude) mel [B][n_mels][T], or log(max(mel, 1e-5)) frame-major [B][T][n_mels]
//   k_mel_segstats<1>   normalize_mel's (mean, unbiased std) of the log-mel of wav[b, s:e] ALONE (reflect padding at the segment's own
//                       ends), one block per segment, nothing but the statistics written
//   k_mel_segstats<0>   the same statistics from a log-mel k_mel_frames wrote (the whole-utterance case, one frame per wave over the
//                       whole grid first): per frame and per reduction step the same operations in the same order as <1>
//   k_resample          torchaudio.functional.resample (sinc_interp_hann): a polyphase GEMM out[m][p] = sum_j xpad[m orig + j] h[p][j]
//                       on v_mfma_f32_16x16x4_f32, A fragments built from a contiguous sample span staged in LDS
//
// The FFT.  The 1024 real samples of a frame are packed as 512 complex values z[n] = x[2n] + i x[2n+1]; the 512-point DFT is three
// radix-8 passes in registers (8 values per lane, n = l + 64 j -> k = q + 8 c + 64 d) with two LDS transposes, then the real-FFT split
// X[k] = (Z[k] + Z*[512-k]) / 2 - i W^k (Z[k] - Z*[512-k]) / 2, k = 0 .. 512.  LDS per frame: 3 x 4 KB written and read (the two
// transposes and the natural-order spectrum) + 2 KB of power spectrum: ~20 KB of traffic, against ~160 KB for melpost::fft1024.
// The 513-bin spectrum lives in the wave's LDS only.  The mel projection is sparse: each filter is a contiguous bin range (host table
// (lo, count, offset) + packed weights), summed in ascending bin order by the lane that owns the filter.
//
// Determinism.  Every output is one fixed-order chain: a frame's values depend on its samples only; a segment's statistics are a
// Welford chain per wave over the frames t = w, w + W, ... (W = kStatWaves) followed by Chan's combination of the W partials in wave
// order -- independent of B, of the grid and of the other segments.  The frame math is compiled with fp contraction off, so the
// fused <1> and the two-kernel path produce the same bits.  No float atomics.
namespace edtts_audio {
using melpost::cplx;

constexpr int kNfft = 1024, kHalf = kNfft / 2, kBins = kHalf + 1, kFrameWaves = 4, kStatWaves = 8, kMaxMels = 128;

EDTTS_DEV void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// W_1024^r for any r >= 0 from the Griffin-Lim table tw[q] = exp(-2 pi i q / 1024), q < 512 (W^(r + 512) = -W^r)
EDTTS_DEV cplx tw1024(const cplx* __restrict__ tw, int r) {
  cplx w = tw[r & 511];
  if (r & 512) { w.re = -w.re; w.im = -w.im; }
  return w;
}

EDTTS_DEV cplx cmul_nc(cplx a, cplx b) {
#pragma clang fp contract(off)
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}

// in-place 8-point forward DFT, X[k] = sum_j a[j] exp(-2 pi i j k / 8)
EDTTS_DEV void dft8(cplx* a) {
#pragma clang fp contract(off)
  constexpr float r2 = 0.70710678118654752f;
  const cplx b0 = {a[0].re + a[4].re, a[0].im + a[4].im}, b1 = {a[0].re - a[4].re, a[0].im - a[4].im};
  const cplx b2 = {a[2].re + a[6].re, a[2].im + a[6].im}, b3 = {a[2].im - a[6].im, a[6].re - a[2].re};  // (a2 - a6) * -i
  const cplx c0 = {a[1].re + a[5].re, a[1].im + a[5].im}, c1 = {a[1].re - a[5].re, a[1].im - a[5].im};
  const cplx c2 = {a[3].re + a[7].re, a[3].im + a[7].im}, c3 = {a[3].im - a[7].im, a[7].re - a[3].re};  // (a3 - a7) * -i
  const cplx e0 = {b0.re + b2.re, b0.im + b2.im}, e2 = {b0.re - b2.re, b0.im - b2.im};
  const cplx e1 = {b1.re + b3.re, b1.im + b3.im}, e3 = {b1.re - b3.re, b1.im - b3.im};
  const cplx o0 = {c0.re + c2.re, c0.im + c2.im}, o2 = {c0.re - c2.re, c0.im - c2.im};
  const cplx o1 = {c1.re + c3.re, c1.im + c3.im}, o3 = {c1.re - c3.re, c1.im - c3.im};
  const cplx w1 = {(o1.re + o1.im) * r2, (o1.im - o1.re) * r2};   // W8^1 o1
  const cplx w2 = {o2.im, -o2.re};                                // W8^2 o2 = -i o2
  const cplx w3 = {(o3.im - o3.re) * r2, -(o3.re + o3.im) * r2};  // W8^3 o3
  a[0] = {e0.re + o0.re, e0.im + o0.im}; a[4] = {e0.re - o0.re, e0.im - o0.im};
  a[1] = {e1.re + w1.re, e1.im + w1.im}; a[5] = {e1.re - w1.re, e1.im - w1.im};
  a[2] = {e2.re + w2.re, e2.im + w2.im}; a[6] = {e2.re - w2.re, e2.im - w2.im};
  a[3] = {e3.re + w3.re, e3.im + w3.im}; a[7] = {e3.re - w3.re, e3.im - w3.im};
}

// reflect index into [0, n) (torch.nn.functional.pad mode "reflect"; n > n_fft / 2 so one reflection suffices)
EDTTS_DEV int reflect(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i;
}

// One frame t of the signal x[0 .. n) (centred: samples t hop - 512 .. t hop + 511, reflected at x's ends), by one wave.
// buf: the wave's 512 complex values of LDS, pw: its 513 floats.  Returns the mel of filters lane and lane + 64 (0 past n_mels).
EDTTS_DEV void mel_frame(const float* __restrict__ x, int n, int t, int hop, const float* __restrict__ win, const cplx* __restrict__ tw,
                         const int* __restrict__ fbd, const float* __restrict__ fbw, int M, bool magnitude, cplx* buf, float* pw,
                         int lane, float& mel0, float& mel1) {
#pragma clang fp contract(off)
  cplx a[8];
  const int base = t * hop - kHalf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int s = 2 * (lane + 64 * j);
    a[j] = {x[reflect(base + s, n)] * win[s], x[reflect(base + s + 1, n)] * win[s + 1]};
  }
  // pass 1: DFT over j (n = l + 64 j), twiddle W_512^(l q)
  dft8(a);
#pragma unroll
  for (int q = 1; q < 8; ++q) a[q] = cmul_nc(a[q], tw1024(tw, 2 * lane * q));
  wave_sync();  // the previous frame's readers of buf / pw are done
#pragma unroll
  for (int q = 0; q < 8; ++q) buf[q * 64 + lane] = a[q];
  wave_sync();
  // pass 2: lane = 8 q + a; DFT over b (l = a + 8 b), twiddle W_64^(a c)
  const int q = lane >> 3, r = lane & 7;
#pragma unroll
  for (int b = 0; b < 8; ++b) a[b] = buf[q * 64 + r + 8 * b];
  dft8(a);
#pragma unroll
  for (int c = 1; c < 8; ++c) a[c] = cmul_nc(a[c], tw1024(tw, 16 * r * c));
  wave_sync();
#pragma unroll
  for (int c = 0; c < 8; ++c) buf[q * 64 + c * 8 + r] = a[c];
  wave_sync();
  // pass 3: lane = 8 q + c; DFT over a -> Z[q + 8 c + 64 d]
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = buf[q * 64 + r * 8 + i];
  dft8(a);
  wave_sync();
#pragma unroll
  for (int d = 0; d < 8; ++d) buf[q + 8 * r + 64 * d] = a[d];
  wave_sync();
  // real-FFT split and |X|^2 (or |X|)
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const int k = lane + 64 * i;
    if (i == 8 && lane > 0) break;
    const cplx zk = buf[k & 511], zm = buf[(kHalf - k) & 511];
    const float fer = 0.5f * (zk.re + zm.re), fei = 0.5f * (zk.im - zm.im);
    const float for_ = 0.5f * (zk.im + zm.im), foi = -0.5f * (zk.re - zm.re);  // -i (Z[k] - Z*[512-k]) / 2
    const cplx w = tw1024(tw, k);
    const float xr = fer + (w.re * for_ - w.im * foi), xi = fei + (w.re * foi + w.im * for_);
    const float p = xr * xr + xi * xi;
    pw[k] = magnitude ? sqrtf(p) : p;
  }
  wave_sync();
  float out[2] = {0.f, 0.f};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int m = lane + 64 * h;
    if (m < M) {
      const int lo = fbd[3 * m], cnt = fbd[3 * m + 1], off = fbd[3 * m + 2];
      float acc = 0.f;
      for (int i = 0; i < cnt; ++i) acc = fmaf(fbw[off + i], pw[lo + i], acc);
      out[h] = acc;
    }
  }
  mel0 = out[0];
  mel1 = out[1];
}

EDTTS_DEV float log_clamp(float v) { return logf(fmaxf(v, 1e-5f)); }

// the mel-analysis lengths: [n_fft / 2 + 1, L]
EDTTS_DEV int mel_len(const int64_t* lengths, int b, int L) {
  if (!lengths) return L;
  const int64_t v = lengths[b];
  return v < kBins ? kBins : (v > L ? L : (int)v);
}

// grid (ceil(T / 4), B), 4 waves: wave w -> frame 4 blockIdx.x + w of row b.  mode 0: out [B][M][T] (power / magnitude mel);
// mode 1: out [B][T][M] log-mel.  Frames past the row's own count len_b // hop + 1 are written as 0.
__global__ __launch_bounds__(64 * kFrameWaves) void k_mel_frames(const float* __restrict__ wav, int L, const int64_t* __restrict__ lengths,
                                                                 int T, int hop, const float* __restrict__ win, const cplx* __restrict__ tw,
                                                                 const int* __restrict__ fbd, const float* __restrict__ fbw, int M,
                                                                 int magnitude, int mode, float* __restrict__ out) {
  __shared__ cplx sbuf[kFrameWaves][kHalf];
  __shared__ float spw[kFrameWaves][kBins + 3];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y, t = blockIdx.x * kFrameWaves + w;
  if (t >= T) return;
  const int n = mel_len(lengths, b, L);
  float v0 = 0.f, v1 = 0.f;
  if (t <= n / hop) {
    mel_frame(wav + (size_t)b * L, n, t, hop, win, tw, fbd, fbw, M, magnitude != 0, sbuf[w], spw[w], lane, v0, v1);
    if (mode == 1) { v0 = log_clamp(v0); v1 = log_clamp(v1); }
  }
  if (mode == 1) {
    float* o = out + ((size_t)b * T + t) * M;
    if (lane < M) o[lane] = v0;
    if (lane + 64 < M) o[lane + 64] = v1;
  } else {
    float* o = out + (size_t)b * M * T + t;
    if (lane < M) o[(size_t)lane * T] = v0;
    if (lane + 64 < M) o[(size_t)(lane + 64) * T] = v1;
  }
}

struct Welford {
  float n, mean, m2;
};
EDTTS_DEV void welford_add(Welford& s, float v) {
#pragma clang fp contract(off)
  s.n += 1.f;
  const float d = v - s.mean;
  s.mean = s.mean + d / s.n;
  s.m2 = s.m2 + d * (v - s.mean);
}
EDTTS_DEV Welford chan(Welford a, Welford b) {  // Chan et al.: combine two partials (an empty one is the identity)
#pragma clang fp contract(off)
  if (b.n == 0.f) return a;
  if (a.n == 0.f) return b;
  const float n = a.n + b.n, d = b.mean - a.mean;
  return {n, a.mean + d * (b.n / n), a.m2 + b.m2 + d * d * (a.n * b.n / n)};
}

// One block of kStatWaves waves per segment i = (row, start, end): mean and unbiased std (clamped at 1e-5; NaN for one frame, as
// torch) of the log-mel of wav[row, start : min(end, len_row)] alone, per mel -> mean / std [n_seg][M].  FUSED: the frames are
// computed here (nothing else written); otherwise they are read from logmel [B][T_lm][M] (segments (b, 0, len_b) only).
// A segment of fewer than n_fft / 2 + 1 samples (possible only through device-side lengths) gives NaN.
template <bool FUSED>
__global__ __launch_bounds__(64 * kStatWaves) void k_mel_segstats(const float* __restrict__ wav, int B, int L, const int64_t* __restrict__ lengths,
                                                                  const int64_t* __restrict__ seg, int hop, const float* __restrict__ win,
                                                                  const cplx* __restrict__ tw, const int* __restrict__ fbd,
                                                                  const float* __restrict__ fbw, int M, const float* __restrict__ logmel,
                                                                  int T_lm, float* __restrict__ mean, float* __restrict__ stdv) {
  __shared__ cplx sbuf[FUSED ? kStatWaves : 1][kHalf];
  __shared__ float spw[FUSED ? kStatWaves : 1][kBins + 3];
  __shared__ Welford part[kStatWaves][kMaxMels];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = blockIdx.x;
  int64_t b = FUSED ? seg[3 * i] : i;
  b = b < 0 ? 0 : (b >= B ? B - 1 : b);
  const int len = mel_len(lengths, (int)b, L);
  int64_t s = FUSED ? seg[3 * i + 1] : 0, e = FUSED ? seg[3 * i + 2] : len;
  s = s < 0 ? 0 : (s > len ? len : s);
  e = e < s ? s : (e > len ? len : e);
  const int n = (int)(e - s), T = n / hop + 1;
  Welford a0 = {0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f};
  if (n >= kBins) {
    for (int t = w; t < T; t += kStatWaves) {
      float v0, v1;
      if (FUSED) {
        mel_frame(wav + (size_t)b * L + s, n, t, hop, win, tw, fbd, fbw, M, false, sbuf[w], spw[w], lane, v0, v1);
        v0 = log_clamp(v0);
        v1 = log_clamp(v1);
      } else {
        const float* r = logmel + ((size_t)b * T_lm + t) * M;
        v0 = lane < M ? r[lane] : 0.f;
        v1 = lane + 64 < M ? r[lane + 64] : 0.f;
      }
      welford_add(a0, v0);
      welford_add(a1, v1);
    }
  }
  if (lane < M) part[w][lane] = a0;
  if (lane + 64 < M) part[w][lane + 64] = a1;
  __syncthreads();
  for (int m = threadIdx.x; m < M; m += 64 * kStatWaves) {
    Welford acc = part[0][m];
    for (int k = 1; k < kStatWaves; ++k) acc = chan(acc, part[k][m]);
    float sd;
    if (n < kBins) sd = __builtin_nanf("");
    else if (acc.n < 2.f) sd = __builtin_nanf("");  // torch.std of one value: 0 / 0
    else sd = fmaxf(sqrtf(acc.m2 / (acc.n - 1.f)), 1e-5f);
    mean[(size_t)i * M + m] = n < kBins ? __builtin_nanf("") : acc.mean;
    stdv[(size_t)i * M + m] = sd;
  }
}

// ---- resampler -----------------------------------------------------------------------------------------------------------------
// y[b][m new + p] = sum_{j < Kp} h[p][j] xpad[m orig + j], xpad = (width zeros, x[b, :len_b], zeros); outputs past ceil(new len_b / orig)
// are 0.  hB [Kp / 4][Np][4]: h[p][4 ks + kg] at ((ks Np + p) 4 + kg), zero for p >= new and j >= K -- the B fragment of k-step ks and
// p-tile pt is 64 contiguous floats.  Block: 4 waves over the same 16 MB output blocks m; wave w takes p-tiles (4 blockIdx.y + w) PT ..
// + PT - 1.  LDS: the block's sample span xpad[m0 orig .. (m0 + 16 MB) orig + Kp), each A fragment one ds_read_b32 per lane.
constexpr int kRsMB = 2;
template <int PT>
__global__ __launch_bounds__(256) void k_resample(const float* __restrict__ x, int L, const int64_t* __restrict__ lengths, int orig, int nw,
                                                  int width, int Kp, const float* __restrict__ hB, int Np, int n_groups, int64_t Lout,
                                                  float* __restrict__ y) {
  extern __shared__ float xs[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.z;
  const int64_t m0 = (int64_t)blockIdx.x * 16 * kRsMB;
  int64_t len = L;
  if (lengths) {
    const int64_t v = lengths[b];
    len = v < 1 ? 1 : (v > L ? L : v);
  }
  const int64_t nout = (len * nw + orig - 1) / orig;
  const int span = 16 * kRsMB * orig + Kp;
  const float* xr = x + (size_t)b * L;
  for (int i = threadIdx.x; i < span; i += 256) {
    const int64_t s = m0 * orig + i - width;
    xs[i] = (s >= 0 && s < len) ? xr[s] : 0.f;
  }
  __syncthreads();
  const int g = blockIdx.y * 4 + w;
  if (g >= n_groups) return;
  f4 acc[kRsMB][PT];
#pragma unroll
  for (int mb = 0; mb < kRsMB; ++mb)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) acc[mb][pt] = f4{0.f, 0.f, 0.f, 0.f};
  const int i = lane & 15, kg = lane >> 4;
  const float* hb = hB + ((size_t)g * PT * 16 + i) * 4 + kg;
  const float* xa = xs + i * orig + kg;
  const int nks = Kp >> 2;
#pragma unroll 2
  for (int ks = 0; ks < nks; ++ks) {
    float bv[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) bv[pt] = hb[((size_t)ks * Np + pt * 16) * 4];
#pragma unroll
    for (int mb = 0; mb < kRsMB; ++mb) {
      const float av = xa[mb * 16 * orig + 4 * ks];
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) acc[mb][pt] = EDTTS_MFMA(av, bv[pt], acc[mb][pt]);
    }
  }
  float* yr = y + (size_t)b * Lout;
#pragma unroll
  for (int mb = 0; mb < kRsMB; ++mb)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const int p = (g * PT + pt) * 16 + i;
      if (p >= nw) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + mb * 16 + kg * 4 + r, o = m * nw + p;
        if (o < Lout) yr[o] = o < nout ? acc[mb][pt][r] : 0.f;
      }
    }
}

}  // namespace edtts_audio

extern "C" {

int edtts_melspec(const float* wav, int B, int L, const int64_t* lengths, int n_fft, int hop, const float* window, const float* twiddle,
                  const int32_t* fb_desc, const float* fb_weights, int n_mels, int power, int mode, float* out, void* stream) {
  using namespace edtts_audio;
  if (!wav || !window || !twiddle || !fb_desc || !fb_weights || !out) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (n_fft != kNfft) return fail(EDTTS_ERR_UNSUPPORTED, "n_fft=%d (compiled: %d, win_length = n_fft)", n_fft, kNfft);
  if (n_mels < 1 || n_mels > kMaxMels) return fail(EDTTS_ERR_UNSUPPORTED, "n_mels=%d (built: 1 .. %d)", n_mels, kMaxMels);
  if (power != 1 && power != 2) return fail(EDTTS_ERR_UNSUPPORTED, "power=%d (built: 1, 2)", power);
  if (mode != EDTTS_MEL_POWER && mode != EDTTS_MEL_LOG) return fail(EDTTS_ERR_ARG, "mode=%d", mode);
  if (B < 1 || hop < 1 || hop > n_fft) return fail(EDTTS_ERR_ARG, "bad sizes: B=%d hop=%d", B, hop);
  if (L <= n_fft / 2) return fail(EDTTS_ERR_ARG, "signal of %d samples is not longer than the reflect padding %d (torch.stft raises too)", L, n_fft / 2);
  const int T = L / hop + 1;
  hipLaunchKernelGGL(k_mel_frames, dim3((T + kFrameWaves - 1) / kFrameWaves, B), dim3(64 * kFrameWaves), 0, (hipStream_t)stream, wav, L,
                     lengths, T, hop, window, reinterpret_cast<const cplx*>(twiddle), fb_desc, fb_weights, n_mels, power == 1 ? 1 : 0,
                     mode, out);
  LAUNCH_CHECK("k_mel_frames");
  return EDTTS_OK;
}

int edtts_mel_segment_stats(const float* wav, int B, int L, const int64_t* lengths, const int64_t* segments, int n_seg, int n_fft, int hop,
                            const float* window, const float* twiddle, const int32_t* fb_desc, const float* fb_weights, int n_mels,
                            float* mean, float* stdv, void* stream) {
  using namespace edtts_audio;
  if (!wav || !segments || !window || !twiddle || !fb_desc || !fb_weights || !mean || !stdv) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (n_fft != kNfft) return fail(EDTTS_ERR_UNSUPPORTED, "n_fft=%d (compiled: %d, win_length = n_fft)", n_fft, kNfft);
  if (n_mels < 1 || n_mels > kMaxMels) return fail(EDTTS_ERR_UNSUPPORTED, "n_mels=%d (built: 1 .. %d)", n_mels, kMaxMels);
  if (B < 1 || n_seg < 1 || hop < 1 || hop > n_fft) return fail(EDTTS_ERR_ARG, "bad sizes: B=%d n_seg=%d hop=%d", B, n_seg, hop);
  if (L <= n_fft / 2) return fail(EDTTS_ERR_ARG, "signal of %d samples is not longer than the reflect padding %d (torch.stft raises too)", L, n_fft / 2);
  hipLaunchKernelGGL(k_mel_segstats<true>, dim3(n_seg), dim3(64 * kStatWaves), 0, (hipStream_t)stream, wav, B, L, lengths, segments, hop,
                     window, reinterpret_cast<const cplx*>(twiddle), fb_desc, fb_weights, n_mels, nullptr, 0, mean, stdv);
  LAUNCH_CHECK("k_mel_segstats");
  return EDTTS_OK;
}

int edtts_logmel_stats(const float* logmel, int B, int T, int n_mels, int L, const int64_t* lengths, int hop, float* mean, float* stdv,
                       void* stream) {
  using namespace edtts_audio;
  if (!logmel || !mean || !stdv) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (n_mels < 1 || n_mels > kMaxMels) return fail(EDTTS_ERR_UNSUPPORTED, "n_mels=%d (built: 1 .. %d)", n_mels, kMaxMels);
  if (B < 1 || hop < 1 || L <= kHalf || T != L / hop + 1) return fail(EDTTS_ERR_ARG, "bad sizes: B=%d T=%d L=%d hop=%d", B, T, L, hop);
  hipLaunchKernelGGL(k_mel_segstats<false>, dim3(B), dim3(64 * kStatWaves), 0, (hipStream_t)stream, nullptr, B, L, lengths, nullptr, hop,
                     nullptr, nullptr, nullptr, nullptr, n_mels, logmel, T, mean, stdv);
  LAUNCH_CHECK("k_mel_segstats");
  return EDTTS_OK;
}

int edtts_resample(const float* x, int B, int L, const int64_t* lengths, int orig, int new_freq, int width, int taps, const float* table,
                   int64_t L_out, float* y, void* stream) {
  using namespace edtts_audio;
  if (!x || !table || !y) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  if (B < 1 || B > 65535 || L < 1 || orig < 1 || new_freq < 1 || width < 0 || taps != 2 * width + orig)
    return fail(EDTTS_ERR_ARG, "bad sizes: B=%d L=%d orig=%d new=%d width=%d taps=%d (need taps = 2 width + orig)", B, L, orig, new_freq, width, taps);
  if (L_out != ((int64_t)L * new_freq + orig - 1) / orig) return fail(EDTTS_ERR_ARG, "L_out=%lld: need ceil(new L / orig)", (long long)L_out);
  const int Kp = (taps + 3) & ~3, Np = (new_freq + 15) & ~15;
  const size_t lds = (size_t)(16 * kRsMB * orig + Kp) * sizeof(float);
  if (lds > 64 * 1024) return fail(EDTTS_ERR_UNSUPPORTED, "orig=%d after the gcd: the %d-block sample span needs %zu B of LDS (limit 64 KiB)", orig, 16 * kRsMB, lds);
  const int tiles = Np / 16, PT = tiles % 5 == 0 ? 5 : 1, n_groups = tiles / PT;
  const int64_t blocks = (L_out + new_freq - 1) / new_freq;
  const dim3 grid((unsigned)((blocks + 16 * kRsMB - 1) / (16 * kRsMB)), (unsigned)((n_groups + 3) / 4), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (PT == 5) hipLaunchKernelGGL(k_resample<5>, grid, dim3(256), lds, st, x, L, lengths, orig, new_freq, width, Kp, table, Np, n_groups, L_out, y);
  else hipLaunchKernelGGL(k_resample<1>, grid, dim3(256), lds, st, x, L, lengths, orig, new_freq, width, Kp, table, Np, n_groups, L_out, y);
  LAUNCH_CHECK("k_resample");
  return EDTTS_OK;
}

}  // extern "C"
