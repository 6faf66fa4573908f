// Stand-alone check of image storage mode 1 (mvn_set_image_storage, include/mvn_engine_api.h) on the host emulation:
// mvn_deconvolve_described with uint16 images kept as uint16 against the same call in mode 0, bit for bit, on the
// shapes where the uint16 paths index differently - an odd last extent (scalar epilogue, RP = d2 + 1), an even extent
// whose row pitch is no multiple of 8 (4-byte stores of the uint16 -> uint16 ingest pass), and uint16 images as
// unaligned windows that END where their allocation ends, embedded under the "zero" policy and in "device" memory
// (the emulation takes any pointer as device memory).  Every stack is an exactly-sized heap allocation, so that the
// sanitizer sees an access past it.  Built with -fsanitize=address,undefined against the emulation built the same way
// (csrc/Makefile, target image-storage-asan); exits non-zero on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "multiviewnative.h"
#include "mvn_engine_api.h"

struct Case {
  int d[3];
  const char* pad;
  int window;    // uint16 elements in front of every row of the image's allocation (0: dense)
  int location;  // of the images
};

static int run(const Case& c) {
  const int V = 2, iters = 2;
  const long n = (long)c.d[0] * c.d[1] * c.d[2];
  int dims[3] = {c.d[0], c.d[1], c.d[2]};
  int kd[3] = {3, 3, 3};
  std::mt19937 rng(11u + (unsigned)c.d[2]);
  std::uniform_int_distribution<int> px(1, 4000);
  std::vector<float> kernel(27);
  float ks = 0.f;
  for (int i = 0; i < 27; ++i) ks += kernel[(size_t)i] = 1.f + (float)(i % 5);
  for (float& k : kernel) k /= ks;
  const long pitch = c.d[2] + c.window;  // the window is the END of every row: the last row ends the allocation
  std::vector<std::vector<uint16_t>> img((size_t)V);
  std::vector<std::vector<float>> wts((size_t)V);
  for (int v = 0; v < V; ++v) {
    img[(size_t)v].assign((size_t)((long)c.d[0] * c.d[1] * pitch), 9);
    for (long r = 0; r < (long)c.d[0] * c.d[1]; ++r)
      for (int x = 0; x < c.d[2]; ++x) img[(size_t)v][(size_t)(r * pitch + c.window + x)] = (uint16_t)px(rng);
    wts[(size_t)v].assign((size_t)n, 1.f / V);
  }
  std::vector<view_data> views((size_t)V);
  std::vector<mvn_stack_desc> idesc((size_t)V);
  for (int v = 0; v < V; ++v) {
    view_data& d = views[(size_t)v];
    d.image_ = (imageType*)(void*)(img[(size_t)v].data() + c.window);
    d.weights_ = wts[(size_t)v].data();
    d.kernel1_ = d.kernel2_ = kernel.data();
    d.image_dims_ = d.weights_dims_ = dims;
    d.kernel1_dims_ = d.kernel2_dims_ = kd;
    idesc[(size_t)v].dtype = MVN_U16;
    idesc[(size_t)v].location = c.location;
    idesc[(size_t)v].stride[0] = (long long)c.d[1] * pitch;
    idesc[(size_t)v].stride[1] = pitch;
    idesc[(size_t)v].stride[2] = 1;
  }
  workspace ws;
  std::memset(&ws, 0, sizeof(ws));
  ws.data_ = views.data();
  ws.num_views_ = (unsigned short)V;
  ws.lambda_ = 0.006;
  ws.minValue_ = 1e-4f;
  ws.num_iterations_ = iters;
  mvn_call_desc call;
  std::memset(&call, 0, sizeof(call));
  call.psi.dtype = MVN_F32, call.psi.location = MVN_HOST;
  call.psi.stride[0] = (long long)c.d[1] * c.d[2], call.psi.stride[1] = c.d[2], call.psi.stride[2] = 1;
  call.image = idesc.data();
  call.weights = nullptr;
  std::vector<float> psi[2];
  long long cnt[2][2];
  if (mvn_set_pad_mode(c.pad) < 0) return 1;
  for (int mode = 0; mode < 2; ++mode) {
    psi[mode].assign((size_t)n, 100.f);
    long long before[2], after[2];
    mvn_image_storage_counters(before);
    if (mvn_set_image_storage(mode) < 0 || mvn_deconvolve_described(psi[mode].data(), ws, &call, 0) < 0) {
      std::printf("call failed: %s\n", mvn_last_error());
      return 1;
    }
    mvn_image_storage_counters(after);
    cnt[mode][0] = after[0] - before[0], cnt[mode][1] = after[1] - before[1];
    mvn_release_cached_engines();
  }
  mvn_set_image_storage(0);
  int bad = std::memcmp(psi[0].data(), psi[1].data(), (size_t)n * sizeof(float)) != 0;
  if (psi[0][0] == 100.f) ++bad;                         // (the loop ran)
  if (cnt[0][0] != 0 || cnt[0][1] != 0) ++bad;           // mode 0 never touches a uint16 volume
  if (cnt[1][0] != (long long)V * iters) ++bad;          // one divide pass per (view, iteration)
  const bool placed_by_copy = c.location == MVN_HOST && std::strcmp(c.pad, "none") == 0;
  if (cnt[1][1] != (placed_by_copy ? 0 : V)) ++bad;      // the uint16 -> uint16 ingest pass, once per view
  std::printf("(%d, %d, %d) pad %s window %d location %d: divides %lld, ingests %lld, %s\n", c.d[0], c.d[1], c.d[2], c.pad,
              c.window, c.location, cnt[1][0], cnt[1][1], bad ? "MISMATCH" : "equal");
  return bad;
}

int main() {
  const Case cases[] = {
      {{6, 7, 19}, "none", 0, MVN_HOST},     // odd last extent: scalar epilogue, the padded column of RP = 20
      {{6, 7, 19}, "none", 3, MVN_DEVICE},   // ... through the ingest pass, unaligned rows
      {{5, 6, 20}, "none", 0, MVN_DEVICE},   // RP = 20: no multiple of 8, pair stores to the end of the row
      {{5, 6, 20}, "none", 5, MVN_HOST},     // rows placed by 2-D copies with 2-byte pitches
      {{6, 7, 19}, "zero", 3, MVN_HOST},     // embedded: through the scratch, then uint16 -> uint16
      {{5, 6, 20}, "zero", 3, MVN_DEVICE},   // embedded, read where it lies
      {{4, 16, 64}, "none", 1, MVN_DEVICE},  // 64 rows, whole tiles: the fixed-length divide; 16-byte stores, source rows 2 bytes off
      {{4, 16, 96}, "none", 0, MVN_HOST},    // a walking fixed-length form (H = 48)
      {{4, 16, 512}, "zero", 0, MVN_HOST},   // d2 = 512 under "none" would be the wave-row form; embedded: the padded extent's
      {{4, 16, 512}, "none", 3, MVN_DEVICE}, // the wave-row form
  };
  int bad = 0;
  for (const Case& c : cases) bad += run(c);
  mvn_set_pad_mode(nullptr);
  std::printf(bad ? "MISMATCH\n" : "ok\n");
  return bad ? 1 : 0;
}
