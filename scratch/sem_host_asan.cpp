// Host-sanitizer walk over the semantic head's training host side: the six byte-count queries, every
// edtts_sem_train_region member and the entry points' refusals, over the suite's heads (tests/sem_train_util.py H1-H5,
// tests/vq_train_util.py V1-V5) at their own shapes and at the slab edges.  No call reaches HIP: CPU only.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude \
//         edge-diffusion-tts_amd/csrc/edtts_kernels.hip scratch/sem_host_asan.cpp -o /tmp/sem_host_asan && /tmp/sem_host_asan
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "edtts.h"

static int g_bad = 0, g_calls = 0, g_refused = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_bad; } \
  } while (0)

static int refused(int rc, const char* text) {  // the call was refused, and the message says `text`
  ++g_calls;
  const bool ok = rc < 0 && std::strstr(edtts_last_error(), text);
  if (!ok) { std::printf("expected a refusal with \"%s\", got %d \"%s\"\n", text, rc, edtts_last_error()); ++g_bad; }
  g_refused += ok;
  return rc;
}

struct Head {
  const char* name;
  EdttsSemDims d;
  int B, T;
};
static Head fsq(const char* name, int in_dim, int S, std::initializer_list<int> lv, int B, int T) {
  Head h{name, {}, B, T};
  h.d.in_dim = in_dim; h.d.semantic_dim = S; h.d.quantizer = EDTTS_SEM_FSQ; h.d.n_levels = (int)lv.size();
  int i = 0;
  for (int v : lv) h.d.levels[i++] = v;
  return h;
}
static Head vq(const char* name, int in_dim, int S, int K, int B, int T) {
  Head h{name, {}, B, T};
  h.d.in_dim = in_dim; h.d.semantic_dim = S; h.d.quantizer = EDTTS_SEM_VQ; h.d.codebook_size = K;
  return h;
}

int main() {
  const std::vector<Head> heads = {
      fsq("H1", 768, 128, {4, 4, 3, 3, 2, 2, 2, 2}, 2, 37), fsq("H2", 256, 64, {7, 5, 3}, 3, 50), fsq("H3", 48, 16, {8, 6, 5, 5, 5}, 1, 5),
      fsq("H4", 0, 32, {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2}, 2, 33), fsq("H5", 128, 64, {7, 5, 3}, 4, 175),
      vq("V1", 768, 128, 512, 2, 37), vq("V2", 256, 64, 1000, 3, 50), vq("V3", 0, 32, 24, 2, 33), vq("V4", 128, 64, 64, 4, 175),
      vq("V5", 48, 16, 5, 1, 5)};
  void* const fake = (void*)0x1000;  // non-NULL, never looked at: the refusal comes first
  for (const Head& h : heads) {
    const bool q = h.d.quantizer == EDTTS_SEM_VQ;
    const int shapes[6][2] = {{h.B, h.T}, {0, 5}, {1, 1}, {1, 256}, {1, 257}, {16, 1500}};
    size_t blob = 0;
    CHECK((q ? edtts_sem_vq_train_packed_bytes(&h.d, &blob) : edtts_sem_train_packed_bytes(&h.d, &blob)) == EDTTS_OK);
    ++g_calls;
    for (const auto& s : shapes) {
      const int B = s[0], T = s[1];
      size_t tape = 0, scratch = 0;
      CHECK((q ? edtts_sem_vq_tape_bytes(&h.d, B, T, &tape) : edtts_sem_train_tape_bytes(&h.d, B, T, &tape)) == EDTTS_OK);
      CHECK((q ? edtts_sem_vq_scratch_bytes(&h.d, B, T, &scratch) : edtts_sem_train_scratch_bytes(&h.d, B, T, &scratch)) == EDTTS_OK);
      g_calls += 2;
      // the members the head has tile the tape (0 .. 4) and the scratch (5 ..) without overlap; the others are refused by name
      std::vector<std::pair<size_t, size_t>> at[2];
      int present = 0;
      for (int which = 0; which < EDTTS_SEM_REGION_COUNT; ++which) {
        size_t off = 0, n = 0;
        ++g_calls;
        if (edtts_sem_train_region(&h.d, B, T, which, &off, &n) != EDTTS_OK) {
          CHECK(std::strstr(edtts_last_error(), "is not a member of this head's layout"));
          ++g_refused;
          continue;
        }
        at[which >= EDTTS_SEM_SCRATCH_DU].push_back({off, n});
        ++present;
      }
      for (int k = 0; k < 2; ++k) {
        std::sort(at[k].begin(), at[k].end());
        size_t end = 0;
        for (const auto& m : at[k]) {
          CHECK(m.first == end);
          end = k ? (m.first + m.second + 15) / 16 * 16 : m.first + m.second;
        }
        CHECK(end == (k ? scratch : tape));
      }
      std::printf("%s %dx%d: blob %zu tape %zu scratch %zu, %d members\n", h.name, B, T, blob, tape, scratch, present);
    }
    // refusals, every pointer NULL unless the refusal needs one
    const Head& o = heads[q ? 0 : 5];  // a head of the other quantizer
    size_t out = 0, off = 0, n = 0;
    EdttsDropout bad_p{1.0f, 1}, half{0.5f, 1};
    const int want = (h.d.in_dim ? 6 : 0) + (q ? 1 : 4);
    std::vector<const void*> slots(want + 1, fake);
    refused(edtts_sem_train_region(&h.d, 1, 1, -1, &off, &n), "which=-1");
    refused(edtts_sem_train_region(&h.d, 1, 1, EDTTS_SEM_REGION_COUNT, &off, &n), "which=17");
    refused(edtts_sem_train_region(&h.d, 1, 1, 0, nullptr, &n), "offset_bytes/bytes is NULL");
    refused(edtts_sem_train_region(&h.d, -1, 1, 0, &off, &n), "out of range");
    refused(edtts_sem_train_region(nullptr, 1, 1, 0, &off, &n), "semantic dims is NULL");
    if (!q) {
      refused(edtts_sem_train_packed_bytes(&o.d, &out), "FSQ quantizer only");
      refused(edtts_sem_train_packed_bytes(&h.d, nullptr), "out_bytes is NULL");
      refused(edtts_sem_train_tape_bytes(&h.d, 1, 1, nullptr), "out_bytes is NULL");
      refused(edtts_sem_train_tape_bytes(&h.d, -1, 1, &out), "out of range");
      refused(edtts_sem_train_scratch_bytes(&o.d, 1, 1, &out), "FSQ quantizer only");
      refused(edtts_sem_train_scratch_bytes(&h.d, 1 << 16, 1 << 16, &out), "out of range");
      refused(edtts_sem_train_pack(&h.d, nullptr, want, fake, nullptr), "slots/packed_train is NULL");
      refused(edtts_sem_train_pack(&h.d, slots.data(), want + 1, fake, nullptr), "weight slots");
      slots[want - 1] = nullptr;
      refused(edtts_sem_train_pack(&h.d, slots.data(), want, fake, nullptr), "is NULL");
      refused(edtts_sem_encode_train(&o.d, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "FSQ quantizer only");
      refused(edtts_sem_encode_train(&h.d, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, &bad_p, nullptr), "dropout p=");
      refused(edtts_sem_encode_train(&h.d, nullptr, nullptr, -1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "out of range");
      refused(edtts_sem_encode_train(&h.d, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "NULL pointer");
      refused(edtts_sem_encode_train_dev(&h.d, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "NULL pointer");
      refused(edtts_sem_backward(&h.d, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, want + 1, nullptr, nullptr, nullptr, nullptr),
              "gradient slots");
      refused(edtts_sem_backward(&h.d, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, want, nullptr, nullptr, nullptr, nullptr),
              "NULL pointer");
      refused(edtts_sem_backward_dev(&h.d, nullptr, nullptr, nullptr, nullptr, 1, -1, nullptr, nullptr, nullptr, want, nullptr, nullptr, nullptr, nullptr),
              "out of range");
      refused(edtts_sem_backward(&h.d, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, want, (float*)fake, nullptr, &half, nullptr),
              h.d.in_dim ? "d_z is the input gradient" : "no dropout site");
      refused(edtts_sem_dropout_mask(&h.d, 1, 1, nullptr, nullptr, nullptr), "drop is NULL");
      refused(edtts_sem_dropout_mask(&h.d, 1, 1, &half, nullptr, nullptr), h.d.in_dim ? "NULL pointer" : "no dropout site");
      refused(edtts_sem_dropout_mask_dev(&o.d, 1, 1, nullptr, nullptr, nullptr), "FSQ quantizer only");
    } else {
      refused(edtts_sem_vq_train_packed_bytes(&o.d, &out), "VQ quantizer only");
      refused(edtts_sem_vq_train_packed_bytes(&h.d, nullptr), "out_bytes is NULL");
      refused(edtts_sem_vq_tape_bytes(&h.d, 1, 1, nullptr), "out_bytes is NULL");
      refused(edtts_sem_vq_tape_bytes(&h.d, 1, -1, &out), "out of range");
      refused(edtts_sem_vq_scratch_bytes(&o.d, 1, 1, &out), "VQ quantizer only");
      refused(edtts_sem_vq_scratch_bytes(&h.d, 1 << 16, 1 << 16, &out), "out of range");
      refused(edtts_sem_vq_train_pack(&h.d, nullptr, want + 1, nullptr, nullptr), "weight slots");
      if (h.d.in_dim) {
        refused(edtts_sem_vq_train_pack(&h.d, nullptr, want, fake, nullptr), "slots/packed_train is NULL");
        slots[0] = nullptr;
        refused(edtts_sem_vq_train_pack(&h.d, slots.data(), want, fake, nullptr), "weight slot 0 is NULL");
      } else {
        CHECK(edtts_sem_vq_train_pack(&h.d, nullptr, want, nullptr, nullptr) == EDTTS_OK);  // nothing to pack
      }
      refused(edtts_sem_vq_encode_train(&o.d, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0.25, nullptr, nullptr),
              "VQ quantizer only");
      refused(edtts_sem_vq_encode_train(&h.d, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, -1.0, &bad_p, nullptr),
              "commit=");
      refused(edtts_sem_vq_encode_train(&h.d, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0.25, &bad_p, nullptr),
              "dropout p=");
      refused(edtts_sem_vq_encode_train(&h.d, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0.25, nullptr, nullptr),
              "NULL pointer");
      refused(edtts_sem_vq_ema_update(&h.d, nullptr, nullptr, 1, 1, nullptr, nullptr, 0.0, 1e-5, nullptr, nullptr, nullptr, nullptr, nullptr), "decay=");
      refused(edtts_sem_vq_ema_update(&h.d, nullptr, nullptr, 1, 1, nullptr, nullptr, 0.99, -1.0, nullptr, nullptr, nullptr, nullptr, nullptr), "epsilon=");
      refused(edtts_sem_vq_ema_update(&h.d, nullptr, nullptr, 1, 1, nullptr, nullptr, 0.99, 1e-5, nullptr, nullptr, nullptr, nullptr, nullptr),
              "NULL pointer");
      refused(edtts_sem_vq_backward(&h.d, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, 2e6, nullptr, want, nullptr,
                                    nullptr, nullptr, nullptr),
              "commit=");
      refused(edtts_sem_vq_backward(&h.d, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, 0.25, nullptr, want + 1, nullptr,
                                    nullptr, nullptr, nullptr),
              "gradient slots");
      refused(edtts_sem_vq_backward(&h.d, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, 0.25, nullptr, want, (float*)fake,
                                    nullptr, &half, nullptr),
              h.d.in_dim ? "d_z is the input gradient" : "no dropout site");
      refused(edtts_sem_vq_backward(&h.d, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, 0.25, nullptr, want, nullptr,
                                    nullptr, nullptr, nullptr),
              "NULL pointer");
    }
  }
  std::printf("%d calls, %d refusals as expected, %d failures\n", g_calls, g_refused, g_bad);
  return g_bad ? 1 : 0;
}
