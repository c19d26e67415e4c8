// edtts_keys.h -- the key stream of a captured training step (included by edtts_kernels.hip): a device array
// of 64-bit Philox keys that one launch regenerates from a device-resident (base seed, call counter).  The keys feed the dropout
// masks of the step's forwards (EdttsDropoutDev) and the objective's per-row noise seeds, so a replayed graph draws new masks and
// new noise without any host work.  The C ABI (edtts_keys_*) is at the end of this file.
namespace edtts_keys {

constexpr unsigned kStreamKeys = 0x50000u;  // include/edtts.h, "Philox stream ids"
constexpr int kKeyThreads = 256;

// K(base, c, i): words 0 and 1 of philox4x32_10(key = base, counter = (i, c lo, kStreamKeys, c hi)), bit 63 cleared
__host__ EDTTS_DEV unsigned long long key_of(unsigned long long base, unsigned long long c, unsigned i) {
  const U4 w = philox4x32_10((unsigned)base, (unsigned)(base >> 32), i, (unsigned)c, kStreamKeys, (unsigned)(c >> 32));
  return ((unsigned long long)w.x | ((unsigned long long)w.y << 32)) & 0x7fffffffffffffffull;
}

// One block.  Every thread reads the counter, the barrier stands between the last of those reads and the store of c + 1.
__global__ __launch_bounds__(kKeyThreads) void k_keys_advance(unsigned long long* keys, int n, unsigned long long* state) {
  const unsigned long long base = state[0], c = state[1];
  for (int i = threadIdx.x; i < n; i += kKeyThreads) keys[i] = key_of(base, c, (unsigned)i);
  __syncthreads();
  if (threadIdx.x == 0) state[1] = c + 1;
}

}  // namespace edtts_keys

extern "C" {

int edtts_keys_advance(uint64_t* keys, int n, uint64_t* state, void* stream) {
  if (n < 0 || (n && !keys) || !state) return fail(EDTTS_ERR_ARG, "edtts_keys_advance: NULL pointer argument or n=%d", n);
  if (((size_t)keys | (size_t)state) & 7) return fail(EDTTS_ERR_ARG, "edtts_keys_advance: keys and state must be 8-byte aligned");
  hipLaunchKernelGGL(edtts_keys::k_keys_advance, dim3(1), dim3(edtts_keys::kKeyThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<unsigned long long*>(keys), n, reinterpret_cast<unsigned long long*>(state));
  LAUNCH_CHECK("k_keys_advance");
  return EDTTS_OK;
}

int edtts_keys_host(uint64_t base, uint64_t counter, int64_t first, int n, uint64_t* out) {
  if (n < 0 || first < 0 || (n && !out) || first + (int64_t)n > 0x100000000ll)
    return fail(EDTTS_ERR_ARG, "edtts_keys_host: NULL out, n=%d or first=%lld outside [0, 2^32 - n]", n, (long long)first);
  for (int i = 0; i < n; ++i) out[i] = edtts_keys::key_of(base, counter, (unsigned)(first + i));
  return EDTTS_OK;
}

}  // extern "C"
