// edtts_debug.h -- diagnostics (included by edtts_kernels.hip behind the launchers): the per-launch timing of the layer kernels that
// bench.py's roofline leg reads (Profiler / PROF_LAUNCH head edtts_kernels.hip, the launchers use them), and the exports that exist
// in diagnostic builds only (-DEDTTS_STAMPS, -DEDTTS_WAVELOG: they set the globals that ForwardArgs hands to the layer kernels).
extern "C" {

int edtts_profile_enable(int max_records) {
  std::lock_guard<std::mutex> lock(g_prof.mu);
  g_prof.on.store(false);
  for (hipEvent_t e : g_prof.start) (void)hipEventDestroy(e);
  for (hipEvent_t e : g_prof.stop) (void)hipEventDestroy(e);
  g_prof.start.clear(); g_prof.stop.clear(); g_prof.used = 0;
  if (max_records < 0) return fail(EDTTS_ERR_ARG, "max_records < 0");
  for (int i = 0; i < max_records; ++i) {
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    g_prof.start.push_back(a); g_prof.stop.push_back(b);
  }
  g_prof.on.store(max_records > 0);
  return EDTTS_OK;
}

int edtts_profile_collect(double* ms_by_kind, int* launches_by_kind) {
  if (!ms_by_kind || !launches_by_kind) return fail(EDTTS_ERR_ARG, "NULL pointer argument");
  std::lock_guard<std::mutex> lock(g_prof.mu);
  ms_by_kind[0] = ms_by_kind[1] = 0.0;
  launches_by_kind[0] = launches_by_kind[1] = 0;
  for (int i = 0; i < g_prof.used; ++i) {
    HIP_TRY(hipEventSynchronize(g_prof.stop[i]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, g_prof.start[i], g_prof.stop[i]));
    ms_by_kind[0] += ms;  // (slot 1, the FFN half of a two-launch layer, stays 0: every layer is one launch)
    launches_by_kind[0] += 1;
  }
  g_prof.used = 0;
  return EDTTS_OK;
}

#ifdef EDTTS_STAMPS
// Diagnostic builds only (-DEDTTS_STAMPS; scratch/stamps_bf16.py): where block 0 / wave 0 of the bf16 layer kernel spends its cycles.
int edtts_debug_set_stamps(void* device_buffer) {
  g_stamps_fwd = (unsigned long long*)device_buffer;
  return EDTTS_OK;
}
#endif

#ifdef EDTTS_WAVELOG
int edtts_debug_set_wavelog(void* device_buffer) {
  g_wavelog = (unsigned long long*)device_buffer;
  return EDTTS_OK;
}
#endif

}  // extern "C"
