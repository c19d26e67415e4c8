// edtts_hubert_host.h -- the host side of the HuBERT backbone, once for both compute dtypes (included by edtts_kernels.hip after the
// two kernel sets, edtts_hubert.h and edtts_hubert16.h): the packed blob's layout, the workspace, the packing, the forward's launch
// list and the edtts_hubert_* entry points.  `bf16` (compute_dtype == EDTTS_HUBERT_BF16) decides four things and nothing else:
//   - a matrix that feeds an MFMA is packed as bf16 (half the floats of its slot) by k_hub_pack16;
//   - an intermediate that only a GEMM or the attention reads is stored as bf16 (conv stages before the last, q | k | v, the
//     attention output, the FFN intermediate), and the workspace has the V^T member;
//   - a GEMM is k_hub_gemm16<EPI, TW, XBF, YBF> instead of k_hub_gemm<EPI, TW> (hub_gemm below: XBF / YBF name the bf16 path's
//     storage of X and Y at that site and are chosen at compile time, so only the instances the launch list names exist);
//   - the attention is k_hub_vt + k_hub_attn16 instead of GenericLauncher::attn.
namespace edtts_hub {

// ---- layouts ----------------------------------------------------------------------------------------------------------------------
struct HubLayout {
  int nc, C[kMaxConv], k[kMaxConv], s[kMaxConv];
  int H, heads, DH, I, L, pk, pg, Cg;
  float eps;
  size_t conv0, gn_w, gn_b, conv[kMaxConv], fp_w, fp_b, proj_w, proj_b, pos_w, pos_b, enc_w, enc_b;
  size_t qkv_w, qkv_b, o_w, o_b, ln1_w, ln1_b, ff1_w, ff1_b, ff2_w, ff2_b, ln2_w, ln2_b, layer;  // layer 0's offsets; stride `layer`
  size_t total;  // floats
};
static size_t al64(size_t n) { return (n + 63) & ~(size_t)63; }  // 256-byte alignment of every tensor

// The blob: offsets in floats for both dtypes; under bf16 a matrix that feeds an MFMA is bf16 (half the floats), conv0 / GroupNorm /
// biases / norm parameters stay fp32.
static int hub_layout(const EdttsHubertDims* d, bool bf16, HubLayout& L) {
  if (!d) return fail(EDTTS_ERR_ARG, "hubert dims is NULL");
  L = HubLayout{};
  if (d->n_conv < 1 || d->n_conv > kMaxConv) return fail(EDTTS_ERR_UNSUPPORTED, "conv_dim: %d layers, need 1..%d", d->n_conv, kMaxConv);
  L.nc = d->n_conv;
  for (int i = 0; i < L.nc; ++i) {
    L.C[i] = d->conv_dim[i]; L.k[i] = d->conv_kernel[i]; L.s[i] = d->conv_stride[i];
    if (L.C[i] < 4 || L.C[i] % 4 || L.C[i] > 8192) return fail(EDTTS_ERR_UNSUPPORTED, "conv_dim[%d]=%d: need a multiple of 4 in [4, 8192]", i, L.C[i]);
    if (L.k[i] < 1 || L.k[i] > (i ? 1024 : kMaxK0)) return fail(EDTTS_ERR_UNSUPPORTED, "conv_kernel[%d]=%d out of [1, %d]", i, L.k[i], i ? 1024 : kMaxK0);
    if (L.s[i] < 1 || L.s[i] > 1024) return fail(EDTTS_ERR_UNSUPPORTED, "conv_stride[%d]=%d out of [1, 1024]", i, L.s[i]);
  }
  L.H = d->hidden; L.heads = d->heads; L.I = d->intermediate; L.L = d->num_layers; L.pk = d->pos_kernel; L.pg = d->pos_groups;
  L.eps = d->layer_norm_eps;
  if (L.H < 4 || L.H % 4 || L.H > 8192) return fail(EDTTS_ERR_UNSUPPORTED, "hidden_size=%d: need a multiple of 4 in [4, 8192]", L.H);
  if (L.heads < 1 || L.H % L.heads) return fail(EDTTS_ERR_UNSUPPORTED, "num_attention_heads=%d does not divide hidden_size=%d", L.heads, L.H);
  L.DH = L.H / L.heads;
  if (L.DH > 128) return fail(EDTTS_ERR_UNSUPPORTED, "head_dim=%d > 128 (hidden_size=%d, num_attention_heads=%d)", L.DH, L.H, L.heads);
  if (L.I < 4 || L.I % 4 || L.I > 65536) return fail(EDTTS_ERR_UNSUPPORTED, "intermediate_size=%d: need a multiple of 4 in [4, 65536]", L.I);
  if (L.L < 0 || L.L > 256) return fail(EDTTS_ERR_UNSUPPORTED, "num_layers=%d out of [0, 256]", L.L);
  if (L.pg < 1 || L.H % L.pg || (L.H / L.pg) % 4)
    return fail(EDTTS_ERR_UNSUPPORTED, "num_conv_pos_embedding_groups=%d: need hidden_size / groups a multiple of 4", L.pg);
  if (L.pk < 1 || L.pk > 1024) return fail(EDTTS_ERR_UNSUPPORTED, "num_conv_pos_embeddings=%d out of [1, 1024]", L.pk);
  if (!(L.eps > 0.f)) return fail(EDTTS_ERR_UNSUPPORTED, "layer_norm_eps=%g: need > 0", (double)L.eps);
  L.Cg = L.H / L.pg;
  if (bf16) {  // 16-byte chunks of 8 k in k_hub_gemm16 (no chunk straddles two taps); one 32-wide MFMA k-tile per 32 of head_dim
    for (int i = 0; i < L.nc; ++i)
      if (L.C[i] % 8) return fail(EDTTS_ERR_UNSUPPORTED, "conv_dim[%d]=%d: compute_dtype bf16 needs a multiple of 8", i, L.C[i]);
    if (L.H % 8) return fail(EDTTS_ERR_UNSUPPORTED, "hidden_size=%d: compute_dtype bf16 needs a multiple of 8", L.H);
    if (L.DH % 32)
      return fail(EDTTS_ERR_UNSUPPORTED, "head_dim=%d (hidden_size=%d / num_attention_heads=%d): compute_dtype bf16 needs a multiple of 32",
                  L.DH, L.H, L.heads);
    if (L.I % 8) return fail(EDTTS_ERR_UNSUPPORTED, "intermediate_size=%d: compute_dtype bf16 needs a multiple of 8", L.I);
    if (L.Cg % 8)
      return fail(EDTTS_ERR_UNSUPPORTED, "num_conv_pos_embedding_groups=%d: compute_dtype bf16 needs hidden_size / groups a multiple of 8", L.pg);
  }
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += al64(n); return at; };
  auto mat = [&](size_t n) { return take(bf16 ? (n + 1) / 2 : n); };  // a matrix that feeds an MFMA
  L.conv0 = take((size_t)L.C[0] * L.k[0]);
  L.gn_w = take(L.C[0]);
  L.gn_b = take(L.C[0]);
  for (int i = 1; i < L.nc; ++i) L.conv[i] = mat((size_t)L.C[i] * L.k[i] * L.C[i - 1]);
  const int CL = L.C[L.nc - 1];
  L.fp_w = take(CL); L.fp_b = take(CL);
  L.proj_w = mat((size_t)L.H * CL); L.proj_b = take(L.H);
  L.pos_w = mat((size_t)L.H * L.pk * L.Cg); L.pos_b = take(L.H);
  L.enc_w = take(L.H); L.enc_b = take(L.H);
  const size_t l0 = o;
  L.qkv_w = mat((size_t)3 * L.H * L.H); L.qkv_b = take(3 * L.H);
  L.o_w = mat((size_t)L.H * L.H); L.o_b = take(L.H);
  L.ln1_w = take(L.H); L.ln1_b = take(L.H);
  L.ff1_w = mat((size_t)L.I * L.H); L.ff1_b = take(L.I);
  L.ff2_w = mat((size_t)L.H * L.I); L.ff2_b = take(L.H);
  L.ln2_w = take(L.H); L.ln2_b = take(L.H);
  L.layer = o - l0;
  L.total = l0 + (size_t)L.L * L.layer;
  return EDTTS_OK;
}
static int hub_conv_out(long long n, int k, int s) {  // conv_out (edtts_hubert.h) on the host: floor((n - k) / s) + 1, at least 0
  const long long d = n - k;
  const long long q = d >= 0 ? d / s : -((-d + s - 1) / s);
  return (int)(q + 1 > 0 ? q + 1 : 0);
}
static int hub_frames(const HubLayout& L, long long n, int* stage = nullptr) {  // frames after the conv stack (and after every stage)
  for (int i = 0; i < L.nc; ++i) {
    n = hub_conv_out(n, L.k[i], L.s[i]);
    if (stage) stage[i] = (int)n;
  }
  return (int)n;
}
static int hub_min_samples(const HubLayout& L) {  // the shortest input with one output frame
  long long r = 1;
  for (int i = L.nc - 1; i >= 0; --i) r = (r - 1) * L.s[i] + L.k[i];
  return (int)(r > 0x7fffffff ? 0x7fffffff : r);
}

struct HubWs {
  int T[kMaxConv];
  int nch, Tp;  // GroupNorm chunks of conv0's frames; T rounded up to 32 (V^T's row pitch)
  size_t lens, stats, part, buf0, buf1, h, att, big, vt, total;  // bytes; vt: 0 bytes under fp32
};
static size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }
// element size of conv stage i's output: bf16 when the next conv reads it, fp32 when the feature projection's LayerNorm does
static size_t hub_esz(const HubLayout& L, bool bf16, int i) { return bf16 && i + 1 < L.nc ? 2 : 4; }
static int hub_ws(const HubLayout& L, bool bf16, int B, int T_audio, HubWs& W) {
  W = HubWs{};
  const int T = hub_frames(L, T_audio, W.T);
  if (T < 1) return fail(EDTTS_ERR_ARG, "T_audio=%d gives no output frame (need at least %d samples)", T_audio, hub_min_samples(L));
  if ((long long)B * W.T[0] * L.C[0] >= 0x7fffffffLL) return fail(EDTTS_ERR_ARG, "B=%d x T_audio=%d: conv0 output too large", B, T_audio);
  W.Tp = (T + 31) & ~31;
  size_t s0 = 0, s1 = 0;
  for (int i = 0; i < L.nc; ++i) {
    const size_t sz = (size_t)B * W.T[i] * L.C[i] * hub_esz(L, bf16, i);
    if (i % 2 == 0) s0 = sz > s0 ? sz : s0;
    else s1 = sz > s1 ? sz : s1;
  }
  const size_t fp = (size_t)B * T * L.C[L.nc - 1] * 4;  // the feature projection's LayerNorm output: in the buffer the last conv did not write
  if (L.nc % 2 == 1) s1 = fp > s1 ? fp : s1;
  else s0 = fp > s0 ? fp : s0;
  const size_t M = (size_t)B * T, wide = (size_t)(3 * L.H > L.I ? 3 * L.H : L.I);
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += al256(n); return at; };
  W.lens = take((size_t)2 * B * 8);
  W.stats = take((size_t)B * L.C[0] * 2 * 4);
  W.nch = (W.T[0] + kGnChunk - 1) / kGnChunk;
  W.part = take((size_t)B * W.nch * L.C[0] * 2 * 8);
  W.buf0 = take(s0);
  W.buf1 = take(s1);
  W.h = take(M * L.H * 4);
  W.att = take(M * L.H * 4);               // the positional conv's output (fp32), then every layer's attention output (fp32 | bf16)
  W.big = take(M * wide * (bf16 ? 2 : 4));  // q | k | v rows, then the FFN intermediate
  W.vt = take(bf16 ? (size_t)B * L.H * W.Tp * 2 : 0);
  W.total = o;
  return EDTTS_OK;
}

static bool hub_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static unsigned hub_grid(size_t n) { const size_t nb = (n + 255) / 256; return (unsigned)(nb > 8192 ? 8192 : (nb < 1 ? 1 : nb)); }

// ---- packing ----------------------------------------------------------------------------------------------------------------------
static int hub_pack(const HubLayout& L, bool bf16, const float* const* s, float* P, hipStream_t st) {
  int i = 0;
  auto copy = [&](size_t off, size_t n) -> int {
    HIP_TRY(hipMemcpyAsync(P + off, s[i++], n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return EDTTS_OK;
  };
  auto conv32 = [&](size_t off, int co, int ci, int k) -> int {  // fp32 [co][ci][k] -> fp32 [co][k][ci]
    hipLaunchKernelGGL(k_hub_pack_conv, dim3(hub_grid((size_t)co * ci * k)), dim3(256), 0, st, s[i++], P + off, co, ci, k);
    LAUNCH_CHECK("k_hub_pack_conv");
    return EDTTS_OK;
  };
  auto pack16 = [&](size_t off, size_t at, int co, int ci, int k) -> int {  // ... -> bf16 [co][k][ci], `at` elements into the tensor
    hipLaunchKernelGGL(k_hub_pack16, dim3(hub_grid((size_t)co * ci * k)), dim3(256), 0, st, s[i++], (__bf16*)(P + off) + at, co, ci, k);
    LAUNCH_CHECK("k_hub_pack16");
    return EDTTS_OK;
  };
  // the matrices that feed an MFMA: a conv's weight, and a plain [co][ci] matrix (fp32: copied as it is)
  auto conv = [&](size_t off, int co, int ci, int k) -> int { return bf16 ? pack16(off, 0, co, ci, k) : conv32(off, co, ci, k); };
  auto mat = [&](size_t off, int co, int ci, size_t at = 0) -> int {
    return bf16 ? pack16(off, at, co, ci, 1) : copy(off + at, (size_t)co * ci);
  };
  const int H = L.H, CL = L.C[L.nc - 1];
  TRY_G(conv32(L.conv0, 1, L.C[0], L.k[0]));  // [C0][1][k0] -> [k0][C0], fp32 in both
  TRY_G(copy(L.gn_w, L.C[0]));
  TRY_G(copy(L.gn_b, L.C[0]));
  for (int c = 1; c < L.nc; ++c) TRY_G(conv(L.conv[c], L.C[c], L.C[c - 1], L.k[c]));
  TRY_G(copy(L.fp_w, CL));
  TRY_G(copy(L.fp_b, CL));
  TRY_G(mat(L.proj_w, H, CL));
  TRY_G(copy(L.proj_b, H));
  TRY_G(conv(L.pos_w, H, L.Cg, L.pk));
  TRY_G(copy(L.pos_b, H));
  TRY_G(copy(L.enc_w, H));
  TRY_G(copy(L.enc_b, H));
  for (int l = 0; l < L.L; ++l) {
    const size_t b0 = (size_t)l * L.layer;
    for (int p = 0; p < 3; ++p) {  // q, k, v -> one [3H][H] matrix and a [3H] bias
      TRY_G(mat(b0 + L.qkv_w, H, H, (size_t)p * H * H));
      TRY_G(copy(b0 + L.qkv_b + (size_t)p * H, H));
    }
    TRY_G(mat(b0 + L.o_w, H, H));
    TRY_G(copy(b0 + L.o_b, H));
    TRY_G(copy(b0 + L.ln1_w, H));
    TRY_G(copy(b0 + L.ln1_b, H));
    TRY_G(mat(b0 + L.ff1_w, L.I, H));
    TRY_G(copy(b0 + L.ff1_b, L.I));
    TRY_G(mat(b0 + L.ff2_w, H, L.I));
    TRY_G(copy(b0 + L.ff2_b, H));
    TRY_G(copy(b0 + L.ln2_w, H));
    TRY_G(copy(b0 + L.ln2_b, H));
  }
  return EDTTS_OK;
}

// ---- launches ---------------------------------------------------------------------------------------------------------------------
// Where a forward stops (edtts_hubert_forward_until): after the last launch of site `site` (EDTTS_HUB_*, include/edtts.h) with index
// `index`; site < 0: never.  tile: 0 = hub_gemm's own rule, 2 | 4 = that TW for every GEMM launch of the call.
struct HubStop {
  int site = -1, index = 0, tile = 0;
};
static bool hub_wide_tile(int M, int N, int G, int B, int tile) {
  const int n_sm = 256;  // MI355X compute units: below two 128-tiles per CU the 64-wide tile (4x the blocks) is used
  const long long big = (long long)((M + 127) / 128) * ((N + 127) / 128) * G * B;
  if (tile) return tile == 4;
  return big >= 2 * n_sm && N > 64;  // (N <= 64, the positional conv's groups: a 128-wide tile would be half empty)
}

// One GEMM launch as the host describes it, for either kernel: HGemmArgs / HGemm16Args (edtts_hubert.h, edtts_hubert16.h: the fields'
// meanings) without the element types.  W points at the matrix's float offset in the blob, whatever it holds.
struct HubGemm {
  const void* X;
  long long xbs;
  int ldrow, Cin, stride, pad, xg;
  const int64_t* nvalid;
  int Tin;
  const float* W;
  int K;
  const float* bias;
  void* Y;
  const float* R;
  long long ybs;
  int ldy, M, N;
};
template <class Args>
static Args hub_gemm_args(const HubGemm& g, int ntn) {
  Args a{};
  a.X = static_cast<decltype(a.X)>(g.X); a.xbs = g.xbs; a.ldrow = g.ldrow; a.Cin = g.Cin; a.stride = g.stride; a.pad = g.pad; a.xg = g.xg;
  a.nvalid = g.nvalid; a.Tin = g.Tin;
  a.W = reinterpret_cast<decltype(a.W)>(g.W); a.K = g.K; a.bias = g.bias;
  a.Y = static_cast<decltype(a.Y)>(g.Y); a.R = g.R; a.ybs = g.ybs; a.ldy = g.ldy; a.M = g.M; a.N = g.N; a.ntn = ntn;
  return a;
}
// Y = epi(X W^T) over B utterances and G groups.  XBF / YBF: X is read / Y is stored as bf16 under bf16 (the fp32 path has no use
// for them).  Both kernels share the tile rule and the grid.
template <int EPI, bool XBF, bool YBF>
static int hub_gemm(hipStream_t st, bool bf16, const HubGemm& g, int B, int G, int tile) {
  const bool wide = hub_wide_tile(g.M, g.N, G, B, tile);
  const int bt = wide ? 128 : 64, ntn = (g.N + bt - 1) / bt;
  const dim3 grid((g.M + bt - 1) / bt, ntn * G, B);
  if (bf16) {
    HGemm16Args a = hub_gemm_args<HGemm16Args>(g, ntn);
    if (wide) hipLaunchKernelGGL((k_hub_gemm16<EPI, 4, XBF, YBF>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_hub_gemm16<EPI, 2, XBF, YBF>), grid, dim3(256), 0, st, a);
    LAUNCH_CHECK("k_hub_gemm16");
  } else {
    HGemmArgs a = hub_gemm_args<HGemmArgs>(g, ntn);
    if (wide) hipLaunchKernelGGL((k_hub_gemm<EPI, 4>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_hub_gemm<EPI, 2>), grid, dim3(256), 0, st, a);
    LAUNCH_CHECK("k_hub_gemm");
  }
  return EDTTS_OK;
}
// a plain row-major GEMM: Y[M][N] = epi(X[M][K] W[N][K]^T)
template <int EPI, bool XBF, bool YBF>
static int hub_dense(hipStream_t st, bool bf16, const void* X, const float* W, const float* bias, void* Y, const float* R, int M, int N,
                     int K, int tile) {
  HubGemm g{};
  g.X = X; g.ldrow = K; g.Cin = K; g.stride = 1; g.Tin = M;
  g.W = W; g.K = K; g.bias = bias; g.Y = Y; g.R = R; g.ldy = N; g.M = M; g.N = N;
  return hub_gemm<EPI, XBF, YBF>(st, bf16, g, 1, 1, tile);
}
static int hub_norm(hipStream_t st, const float* x, float* y, int rows, int W, const float* g, const float* b, float eps) {
  edtts_gen::NormArgs a{x, y, g, b, nullptr, rows, W, W, 1, 0, eps};
  hipLaunchKernelGGL(edtts_gen::k_gen_norm<edtts_gen::NORM_LAYER>, dim3((rows + 3) / 4), dim3(256), 0, st, a);
  LAUNCH_CHECK("k_gen_norm");
  return EDTTS_OK;
}

static const char* const kHubSiteNames[EDTTS_HUB_COUNT] = {"LENS", "GNSTAT", "CONV0", "CONV", "FPNORM", "FPROJ", "POS", "ENCNORM", "QKV",
                                                           "VT", "ATTN", "OPROJ", "LN1", "FF1", "FF2", "LN2", "ZERO"};
// a stop that names a site the call does not have is refused (the forward would otherwise run to its end unnoticed)
static int hub_stop_check(const HubLayout& L, bool bf16, bool with_lengths, const HubStop& s) {
  const char* fn = "edtts_hubert_forward_until";
  if (s.tile != 0 && s.tile != 2 && s.tile != 4) return fail(EDTTS_ERR_ARG, "%s: tile=%d: expected 0 (the launcher's rule), 2 or 4", fn, s.tile);
  if (s.site < 0 || s.site >= EDTTS_HUB_COUNT)
    return fail(EDTTS_ERR_ARG, "%s: stop_site=%d: expected an EDTTS_HUB_* site in [0, %d)", fn, s.site, (int)EDTTS_HUB_COUNT);
  const char* nm = kHubSiteNames[s.site];
  if ((s.site == EDTTS_HUB_LENS || s.site == EDTTS_HUB_ZERO) && !with_lengths)
    return fail(EDTTS_ERR_ARG, "%s: site EDTTS_HUB_%s exists only with lengths", fn, nm);
  if (s.site == EDTTS_HUB_VT && !bf16) return fail(EDTTS_ERR_ARG, "%s: site EDTTS_HUB_VT exists only under EDTTS_HUBERT_BF16", fn);
  if (s.site == EDTTS_HUB_CONV) {
    if (s.index < 1 || s.index >= L.nc)
      return fail(EDTTS_ERR_ARG, "%s: site EDTTS_HUB_CONV: stop_index=%d: expected a conv layer in [1, %d)", fn, s.index, L.nc);
  } else if (s.site >= EDTTS_HUB_QKV && s.site <= EDTTS_HUB_LN2) {
    if (s.index < 0 || s.index >= L.L)
      return fail(EDTTS_ERR_ARG, "%s: site EDTTS_HUB_%s: stop_index=%d: expected an encoder layer in [0, %d)", fn, nm, s.index, L.L);
  } else if (s.index != 0) {
    return fail(EDTTS_ERR_ARG, "%s: site EDTTS_HUB_%s has no index: stop_index=%d, expected 0", fn, nm, s.index);
  }
  return EDTTS_OK;
}
#define EDTTS_HUB_STOP_AFTER(site_, index_) \
  if (stop.site == (site_) && stop.index == (index_)) return EDTTS_OK

// The forward's launch list.  The sites of edtts_hubert_forward_until (EDTTS_HUB_*, include/edtts.h): one line below each; `stop`
// never matches in the plain entry points (site -1), whose launch list is the whole of it.
static int hub_forward(const HubLayout& L, bool bf16, const void* packed, const float* wav, int B, int T_audio, const int64_t* lengths,
                       float* out, void* workspace, hipStream_t st, const HubStop stop) {
  HubWs ws;
  TRY_G(hub_ws(L, bf16, B, T_audio, ws));
  const int tile = stop.tile;
  const float* P = (const float*)packed;
  char* wb = (char*)workspace;
  const int T = ws.T[L.nc - 1], H = L.H, M = B * T;
  int64_t *len0 = nullptr, *flen = nullptr;
  if (lengths) {
    len0 = (int64_t*)(wb + ws.lens);
    flen = len0 + B;
    ConvGeo geo{};
    geo.n = L.nc;
    for (int i = 0; i < L.nc; ++i) { geo.k[i] = L.k[i]; geo.s[i] = L.s[i]; }
    hipLaunchKernelGGL(k_hub_lens, dim3((B + 63) / 64), dim3(64), 0, st, lengths, B, T_audio, hub_min_samples(L), geo, len0, flen);
    LAUNCH_CHECK("k_hub_lens");
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_LENS, 0);
  }
  float* stats = (float*)(wb + ws.stats);
  void* buf[2] = {wb + ws.buf0, wb + ws.buf1};
  float *h = (float*)(wb + ws.h), *att = (float*)(wb + ws.att);  // att: fp32 after the positional conv; the attention's output
  void* big = wb + ws.big;                                       // ... and big (q | k | v, the FFN intermediate): fp32 | bf16
  // conv0 + GroupNorm + GELU -> buf[0] (bf16 when a conv reads it)
  double* part = (double*)(wb + ws.part);
  hipLaunchKernelGGL(k_hub_gn_part, dim3((L.C[0] + 63) / 64, ws.nch, B), dim3(256), 0, st, wav, T_audio, P + L.conv0, L.C[0], L.k[0],
                     L.s[0], len0, ws.T[0], part);
  LAUNCH_CHECK("k_hub_gn_part");
  hipLaunchKernelGGL(k_hub_gn_final, dim3((B * L.C[0] + 255) / 256), dim3(256), 0, st, part, ws.nch, L.C[0], len0, ws.T[0], 1e-5f,
                     P + L.gn_w, P + L.gn_b, stats, B);
  LAUNCH_CHECK("k_hub_gn_final");
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_GNSTAT, 0);
  const dim3 g0(hub_grid((size_t)B * ws.T[0] * L.C[0] / 4));
  if (bf16 && L.nc > 1) {
    hipLaunchKernelGGL(k_hub_conv0_16, g0, dim3(256), 0, st, wav, T_audio, P + L.conv0, L.C[0], L.k[0], L.s[0], len0, ws.T[0], stats,
                       (__bf16*)buf[0], B);
    LAUNCH_CHECK("k_hub_conv0_16");
  } else {
    hipLaunchKernelGGL(k_hub_conv0, g0, dim3(256), 0, st, wav, T_audio, P + L.conv0, L.C[0], L.k[0], L.s[0], len0, ws.T[0], stats,
                       (float*)buf[0], B);
    LAUNCH_CHECK("k_hub_conv0");
  }
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_CONV0, 0);
  // conv1.. as implicit GEMMs + GELU, ping-ponging between the two buffers
  for (int c = 1; c < L.nc; ++c) {
    HubGemm g{};
    g.X = buf[(c - 1) & 1]; g.xbs = (long long)ws.T[c - 1] * L.C[c - 1]; g.ldrow = L.C[c - 1]; g.Cin = L.C[c - 1]; g.stride = L.s[c];
    g.Tin = ws.T[c - 1];
    g.W = P + L.conv[c]; g.K = L.k[c] * L.C[c - 1];
    g.Y = buf[c & 1]; g.ybs = (long long)ws.T[c] * L.C[c]; g.ldy = L.C[c]; g.M = ws.T[c]; g.N = L.C[c];
    if (c + 1 < L.nc) TRY_G((hub_gemm<HEPI_GELU, true, true>(st, bf16, g, B, 1, tile)));
    else TRY_G((hub_gemm<HEPI_GELU, true, false>(st, bf16, g, B, 1, tile)));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_CONV, c);
  }
  // feature projection: LayerNorm (fp32) -> Linear (+ bias) -> h
  const int CL = L.C[L.nc - 1];
  float* feat = (float*)buf[(L.nc - 1) & 1];
  float* fn = (float*)buf[L.nc & 1];
  TRY_G(hub_norm(st, feat, fn, M, CL, P + L.fp_w, P + L.fp_b, L.eps));
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_FPNORM, 0);
  TRY_G((hub_dense<HEPI_BIAS, false, false>(st, bf16, fn, P + L.proj_w, P + L.proj_b, h, nullptr, M, H, CL, tile)));
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_FPROJ, 0);
  // att = h + GELU(pos_conv(h) + bias), one GEMM per group; zero rows outside [0, frames_b)
  {
    HubGemm g{};
    g.X = h; g.xbs = (long long)T * H; g.ldrow = H; g.Cin = L.Cg; g.stride = 1; g.pad = L.pk / 2; g.xg = L.Cg;
    g.nvalid = flen; g.Tin = T;
    g.W = P + L.pos_w; g.K = L.pk * L.Cg; g.bias = P + L.pos_b;
    g.Y = att; g.R = h; g.ybs = (long long)T * H; g.ldy = H; g.M = T; g.N = L.Cg;
    TRY_G((hub_gemm<HEPI_GELU_RESID, false, false>(st, bf16, g, B, L.pg, tile)));
  }
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_POS, 0);
  TRY_G(hub_norm(st, att, L.L ? h : out, M, H, P + L.enc_w, P + L.enc_b, L.eps));
  EDTTS_HUB_STOP_AFTER(EDTTS_HUB_ENCNORM, 0);
  const HAttn16Args aa{(const __bf16*)big, (__bf16*)(wb + ws.vt), (__bf16*)att, flen, H, L.heads, L.DH, T, ws.Tp,
                       1.4426950408889634f / sqrtf((float)L.DH)};  // (bf16 only)
  for (int l = 0; l < L.L; ++l) {
    const float* Y = P + (size_t)l * L.layer;
    TRY_G((hub_dense<HEPI_BIAS, false, true>(st, bf16, h, Y + L.qkv_w, Y + L.qkv_b, big, nullptr, M, 3 * H, H, tile)));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_QKV, l);
    if (bf16) {
      hipLaunchKernelGGL(k_hub_vt, dim3(ws.Tp / 32, L.heads, B), dim3(256), 0, st, aa);
      LAUNCH_CHECK("k_hub_vt");
      EDTTS_HUB_STOP_AFTER(EDTTS_HUB_VT, l);
      const dim3 grid((T + 63) / 64, L.heads, B);
      TRY_G(with_head_tiles<8>(L.DH, [&](auto dt) -> int {  // head_dim = 32 KT: an even count of 16-wide tiles (hub_layout)
        constexpr int DT = decltype(dt)::value;
        if constexpr (DT % 2 == 0) {
          hipLaunchKernelGGL(k_hub_attn16<DT / 2>, grid, dim3(256), 0, st, aa);
          LAUNCH_CHECK("k_hub_attn16");
          return EDTTS_OK;
        } else {
          return fail(EDTTS_ERR_UNSUPPORTED, "head_dim=%d: compute_dtype bf16 needs a multiple of 32 up to 128", L.DH);
        }
      }));
    } else {
      const float* qkv = (const float*)big;
      TRY_G(GenericLauncher::attn(st, AttnShape(H, L.heads, L.DH), B, qkv, 3 * H, qkv + H, qkv + 2 * H, 3 * H, att, T, T, -1, flen, flen, false,
                                  false));
    }
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_ATTN, l);
    TRY_G((hub_dense<HEPI_RESID, true, false>(st, bf16, att, Y + L.o_w, Y + L.o_b, h, h, M, H, H, tile)));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_OPROJ, l);
    TRY_G(hub_norm(st, h, h, M, H, Y + L.ln1_w, Y + L.ln1_b, L.eps));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_LN1, l);
    TRY_G((hub_dense<HEPI_GELU, false, true>(st, bf16, h, Y + L.ff1_w, Y + L.ff1_b, big, nullptr, M, L.I, H, tile)));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_FF1, l);
    TRY_G((hub_dense<HEPI_RESID, true, false>(st, bf16, big, Y + L.ff2_w, Y + L.ff2_b, h, h, M, H, L.I, tile)));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_FF2, l);
    TRY_G(hub_norm(st, h, l + 1 < L.L ? h : out, M, H, Y + L.ln2_w, Y + L.ln2_b, L.eps));
    EDTTS_HUB_STOP_AFTER(EDTTS_HUB_LN2, l);
  }
  if (flen) {
    hipLaunchKernelGGL(k_hub_zero_past, dim3(hub_grid((size_t)M * H / 4)), dim3(256), 0, st, out, flen, B, T, H);
    LAUNCH_CHECK("k_hub_zero_past");
  }
  return EDTTS_OK;
}

// ---- the entry points' argument checks, once ----------------------------------------------------------------------------------------
static int hub_open(const EdttsHubertDims* dims, int compute_dtype, HubLayout& L, bool& bf16) {
  if (compute_dtype != EDTTS_HUBERT_FP32 && compute_dtype != EDTTS_HUBERT_BF16)
    return fail(EDTTS_ERR_ARG, "compute_dtype=%d: expected EDTTS_HUBERT_FP32 (0) or EDTTS_HUBERT_BF16 (1)", compute_dtype);
  bf16 = compute_dtype == EDTTS_HUBERT_BF16;
  return hub_layout(dims, bf16, L);
}
static int hub_shape_check(int B, int T_audio) {
  if (B < 1 || T_audio < 1) return fail(EDTTS_ERR_ARG, "B=%d T_audio=%d: need >= 1", B, T_audio);
  return EDTTS_OK;
}
// edtts_hubert_forward_dt (until null) and edtts_hubert_forward_until
static int hub_run(const EdttsHubertDims* dims, int compute_dtype, const void* packed, const float* wav, int B, int T_audio,
                   const int64_t* lengths, float* out, void* workspace, const HubStop* until, void* stream) {
  HubLayout L;
  bool bf16;
  TRY_G(hub_open(dims, compute_dtype, L, bf16));
  if (!packed || !wav || !out || !workspace) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  TRY_G(hub_shape_check(B, T_audio));
  if (!hub_al16(packed) || !hub_al16(out) || !hub_al16(workspace)) return fail(EDTTS_ERR_ARG, "packed, out and workspace must be 16-byte aligned");
  if (until) TRY_G(hub_stop_check(L, bf16, lengths != nullptr, *until));
  return hub_forward(L, bf16, packed, wav, B, T_audio, lengths, out, workspace, (hipStream_t)stream, until ? *until : HubStop{});
}

}  // namespace edtts_hub

extern "C" {

int edtts_hubert_frames(const EdttsHubertDims* dims, int64_t n_samples, int64_t* out_frames) {
  edtts_hub::HubLayout L;
  TRY_G(edtts_hub::hub_layout(dims, false, L));
  if (!out_frames) return fail(EDTTS_ERR_ARG, "out_frames is NULL");
  if (n_samples < 0 || n_samples > 0x7fffffffLL) return fail(EDTTS_ERR_ARG, "n_samples=%lld out of range", (long long)n_samples);
  *out_frames = edtts_hub::hub_frames(L, n_samples);
  return EDTTS_OK;
}

int edtts_hubert_packed_bytes_dt(const EdttsHubertDims* dims, int compute_dtype, size_t* out_bytes) {
  edtts_hub::HubLayout L;
  bool bf16;
  TRY_G(edtts_hub::hub_open(dims, compute_dtype, L, bf16));
  if (!out_bytes) return fail(EDTTS_ERR_ARG, "out_bytes is NULL");
  *out_bytes = L.total * sizeof(float);
  return EDTTS_OK;
}

int edtts_hubert_workspace_bytes_dt(const EdttsHubertDims* dims, int compute_dtype, int B, int T_audio, size_t* out_bytes) {
  using namespace edtts_hub;
  HubLayout L;
  bool bf16;
  TRY_G(hub_open(dims, compute_dtype, L, bf16));
  if (!out_bytes) return fail(EDTTS_ERR_ARG, "out_bytes is NULL");
  TRY_G(hub_shape_check(B, T_audio));
  HubWs W;
  TRY_G(hub_ws(L, bf16, B, T_audio, W));
  *out_bytes = W.total;
  return EDTTS_OK;
}

int edtts_hubert_pack_dt(const EdttsHubertDims* dims, int compute_dtype, const void* const* slots, int n_slots, void* packed, void* stream) {
  using namespace edtts_hub;
  HubLayout L;
  bool bf16;
  TRY_G(hub_open(dims, compute_dtype, L, bf16));
  const int want = 3 + (L.nc - 1) + 8 + 16 * L.L;
  if (!slots || !packed) return fail(EDTTS_ERR_ARG, "slots/packed is NULL");
  if (n_slots != want) return fail(EDTTS_ERR_ARG, "expected %d weight slots, got %d", want, n_slots);
  for (int i = 0; i < n_slots; ++i)
    if (!slots[i]) return fail(EDTTS_ERR_ARG, "weight slot %d is NULL", i);
  if (!hub_al16(packed)) return fail(EDTTS_ERR_ARG, "packed must be 16-byte aligned");  // (the forward refuses any other blob)
  return hub_pack(L, bf16, (const float* const*)slots, (float*)packed, (hipStream_t)stream);
}

int edtts_hubert_forward_dt(const EdttsHubertDims* dims, int compute_dtype, const void* packed, const float* wav, int B, int T_audio,
                            const int64_t* lengths, float* out, void* workspace, void* stream) {
  return edtts_hub::hub_run(dims, compute_dtype, packed, wav, B, T_audio, lengths, out, workspace, nullptr, stream);
}

int edtts_hubert_forward_until(const EdttsHubertDims* dims, int compute_dtype, const void* packed, const float* wav, int B, int T_audio,
                               const int64_t* lengths, float* out, void* workspace, int stop_site, int stop_index, int tile, void* stream) {
  edtts_hub::HubStop stop;
  stop.site = stop_site; stop.index = stop_index; stop.tile = tile;
  return edtts_hub::hub_run(dims, compute_dtype, packed, wav, B, T_audio, lengths, out, workspace, &stop, stream);
}

int edtts_hubert_workspace_region(const EdttsHubertDims* dims, int compute_dtype, int B, int T_audio, int which, size_t* offset_bytes,
                                  size_t* bytes) {
  using namespace edtts_hub;
  HubLayout L;
  bool bf16;
  TRY_G(hub_open(dims, compute_dtype, L, bf16));
  if (!offset_bytes || !bytes) return fail(EDTTS_ERR_ARG, "offset_bytes/bytes is NULL");
  TRY_G(hub_shape_check(B, T_audio));
  HubWs W;
  TRY_G(hub_ws(L, bf16, B, T_audio, W));
  // the members' offsets in layout order, closed by the total: a member reaches up to the next one's offset
  const size_t at[EDTTS_HUB_WS_COUNT + 1] = {W.lens, W.stats, W.part, W.buf0, W.buf1, W.h, W.att, W.big, W.vt, W.total};
  const int n = bf16 ? EDTTS_HUB_WS_COUNT : EDTTS_HUB_WS_VT;
  if (which < 0 || which >= n)
    return fail(EDTTS_ERR_ARG, "edtts_hubert_workspace_region: which=%d: expected an EDTTS_HUB_WS_* member in [0, %d)%s", which, n,
                bf16 ? "" : " (EDTTS_HUB_WS_VT exists only under EDTTS_HUBERT_BF16)");
  *offset_bytes = at[which];
  *bytes = at[which + 1] - at[which];
  return EDTTS_OK;
}

// the fp32 entry points of before compute_dtype
int edtts_hubert_packed_bytes(const EdttsHubertDims* dims, size_t* out_bytes) {
  return edtts_hubert_packed_bytes_dt(dims, EDTTS_HUBERT_FP32, out_bytes);
}
int edtts_hubert_workspace_bytes(const EdttsHubertDims* dims, int B, int T_audio, size_t* out_bytes) {
  return edtts_hubert_workspace_bytes_dt(dims, EDTTS_HUBERT_FP32, B, T_audio, out_bytes);
}
int edtts_hubert_pack(const EdttsHubertDims* dims, const void* const* slots, int n_slots, void* packed, void* stream) {
  return edtts_hubert_pack_dt(dims, EDTTS_HUBERT_FP32, slots, n_slots, packed, stream);
}
int edtts_hubert_forward(const EdttsHubertDims* dims, const void* packed, const float* wav, int B, int T_audio, const int64_t* lengths,
                         float* out, void* workspace, void* stream) {
  return edtts_hubert_forward_dt(dims, EDTTS_HUBERT_FP32, packed, wav, B, T_audio, lengths, out, workspace, stream);
}

}  // extern "C"
