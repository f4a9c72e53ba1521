// The host half of the libpcnn internals (poisson_cnn_amd/csrc/pcnn_host.h) without a GPU and without a HIP library: the four runtime calls the
// header makes are defined here over malloc, count their calls and can be told to fail.  Built plain and under ASan + UBSan by tests/test_pcnn_host.py.
#include "../../poisson_cnn_amd/csrc/pcnn_host.h"
#include <stdlib.h>
#include <string.h>
#include <set>

static int n_malloc, n_free, n_sync, fail_next_malloc;
static size_t last_malloc_bytes;
static hipError_t pending = hipSuccess;       // HIP's sticky last error
static std::set<void*> live;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
  } while (0)

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
  ++n_malloc;
  last_malloc_bytes = bytes;
  if (fail_next_malloc) { --fail_next_malloc; *p = nullptr; return pending = hipErrorOutOfMemory; }
  *p = malloc(bytes ? bytes : 1);
  live.insert(*p);
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  if (!p) return hipSuccess;
  ++n_free;
  CHECK(live.erase(p) == 1);                  // unknown or already freed block
  free(p);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { ++n_sync; return hipSuccess; }
hipError_t hipGetLastError(void) { const hipError_t e = pending; pending = hipSuccess; return e; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory"; }
}

static int check_launch(pcnn_handle_s* h) { PCNN_CHECK_LAUNCH(h, "launch"); return 0; }

// what pcnn_destroy does with the handle's buffers
static void sweep(pcnn_handle_s* h) {
  for (pcnn_buffer* b : {&h->scratch, &h->spec_ws, &h->aux_ws}) (void)hipFree(b->p);
  for (void* p : h->retired) (void)hipFree(p);
}

static void test_reserve() {
  const size_t MB = (size_t)1 << 20;
  pcnn_handle_s h{};
  bool grew = true;
  // first use: the floor
  CHECK(pcnn_reserve(&h, h.scratch, 1000, 4 * MB, "a", &grew) == 0);
  CHECK(grew && n_malloc == 1 && last_malloc_bytes == 4 * MB && h.scratch.bytes == 4 * MB && h.scratch.p);
  CHECK(n_sync == 0 && n_free == 0);          // nothing to release yet
  // large enough: nothing happens, the block stays where it is
  void* first = h.scratch.p;
  CHECK(pcnn_reserve(&h, h.scratch, 4 * MB, 4 * MB, "a", &grew) == 0);
  CHECK(!grew && n_malloc == 1 && h.scratch.p == first && h.scratch.bytes == 4 * MB);
  CHECK(pcnn_reserve(&h, h.scratch, 1, 0, "a") == 0 && n_malloc == 1 && h.scratch.p == first);
  // a need above the floor is allocated in full (the narrow convolution's case), the old block is freed after ONE stream synchronise
  CHECK(pcnn_reserve(&h, h.scratch, 4 * MB + 1, 4 * MB, "a", &grew) == 0);
  CHECK(grew && n_malloc == 2 && last_malloc_bytes == 4 * MB + 1 && h.scratch.bytes == 4 * MB + 1);
  CHECK(n_sync == 1 && n_free == 1 && live.count(first) == 0 && live.count(h.scratch.p) == 1);
  // the exact need where there is no floor
  CHECK(pcnn_reserve(&h, h.aux_ws, 12345, 0, "b", &grew) == 0);
  CHECK(grew && last_malloc_bytes == 12345 && h.aux_ws.bytes == 12345 && n_sync == 1 && n_free == 1);
  // retain: the outgrown block is parked - no synchronise, no free
  h.retain = 1;
  void* parked = h.aux_ws.p;
  CHECK(pcnn_reserve(&h, h.aux_ws, 20000, 0, "b", &grew) == 0);
  CHECK(grew && n_sync == 1 && n_free == 1 && h.retired.size() == 1 && h.retired[0] == parked && live.count(parked) == 1 && h.aux_ws.p != parked);
  h.retain = 0;
  // a failed allocation: 1, an empty buffer, the caller's name in the text, no stale error left for the next launch check
  fail_next_malloc = 1;
  const int frees = n_free;
  CHECK(pcnn_reserve(&h, h.aux_ws, 30000, 0, "pcnn_some_entry", &grew) == 1);
  CHECK(!grew && h.aux_ws.p == nullptr && h.aux_ws.bytes == 0 && n_free == frees + 1);
  CHECK(strstr(h.err.c_str(), "pcnn_some_entry: cannot allocate 30000 B") == h.err.c_str());
  CHECK(pending == hipSuccess && check_launch(&h) == 0);
  // ... and the next call with a working allocator succeeds
  CHECK(pcnn_reserve(&h, h.aux_ws, 30000, MB, "pcnn_some_entry", &grew) == 0);
  CHECK(grew && h.aux_ws.p && h.aux_ws.bytes == MB);
  // a failure without `grew`
  fail_next_malloc = 1;
  CHECK(pcnn_reserve(&h, h.spec_ws, 64, 0, "c") == 1 && h.spec_ws.p == nullptr && h.spec_ws.bytes == 0 && pending == hipSuccess);
  CHECK(pcnn_reserve(&h, h.spec_ws, 64, 0, "c") == 0 && h.spec_ws.bytes == 64);
  // pcnn_drop (pcnn_set_workspace_limit), then the sweep of pcnn_destroy: every block is freed exactly once (hipFree above refuses a second time,
  // the leak check of the sanitizer build a missing one)
  const int syncs = n_sync;
  pcnn_drop(&h, h.spec_ws);
  CHECK(h.spec_ws.p == nullptr && h.spec_ws.bytes == 0 && n_sync == syncs + 1);
  pcnn_drop(&h, h.spec_ws);                   // an empty buffer: nothing to do
  CHECK(n_sync == syncs + 1);
  sweep(&h);
  CHECK(live.empty() && n_free == n_malloc - 2);   // two of the allocations failed
}

struct Case { const char* what; pcnn_conv_desc d; int max_cin, max_cout, max_taps; const char* problem; };

static pcnn_conv_desc desc(int H, int W, int Cin, int Cout, int kh, int kw, int pt, int pl, int mode) {
  pcnn_conv_desc d{};
  d.N = 2; d.H = H; d.W = W; d.Cin = Cin; d.ldx = Cin; d.Ho = H; d.Wo = W; d.Cout = Cout; d.ldy = Cout;
  d.kh = kh; d.kw = kw; d.pad_top = pt; d.pad_left = pl; d.pad_mode = mode;
  return d;
}
// an H x W image with `top` / `bottom` / `left` / `right` rows and columns of padding around it, filter 3 x 3: Ho = H + top + bottom - 2
static pcnn_conv_desc padded(int H, int W, int top, int bottom, int left, int right, int mode) {
  pcnn_conv_desc d = desc(H, W, 4, 4, 3, 3, top, left, mode);
  d.Ho = H + top + bottom - 2; d.Wo = W + left + right - 2;
  return d;
}
template <typename F>
static pcnn_conv_desc with(pcnn_conv_desc d, F f) { f(d); return d; }

static void test_desc() {
  const int C = PCNN_PAD_CONSTANT, S = PCNN_PAD_SYMMETRIC, R = PCNN_PAD_REFLECT;
  const char *ok = nullptr, *empty = "empty tensor", *cin = "Cin", *cout = "Cout", *taps = "filter size", *ld = "channel stride", *mode = "pad_mode", *pad = "padding exceeds";
  const pcnn_conv_desc base = desc(8, 9, 4, 4, 3, 3, 1, 1, C);
  const Case cases[] = {
      {"plain", base, 64, 64, 31, ok},
      {"N = 0", with(base, [](pcnn_conv_desc& d) { d.N = 0; }), 64, 64, 31, empty},
      {"H = 0", with(base, [](pcnn_conv_desc& d) { d.H = 0; }), 64, 64, 31, empty},
      {"W = 0", with(base, [](pcnn_conv_desc& d) { d.W = 0; }), 64, 64, 31, empty},
      {"Ho = 0", with(base, [](pcnn_conv_desc& d) { d.Ho = 0; }), 64, 64, 31, empty},
      {"Wo = 0", with(base, [](pcnn_conv_desc& d) { d.Wo = 0; }), 64, 64, 31, empty},
      {"Cin = 1", desc(8, 9, 1, 4, 3, 3, 1, 1, C), 64, 64, 31, ok},
      {"Cin = 0", with(base, [](pcnn_conv_desc& d) { d.Cin = 0; }), 64, 64, 31, cin},
      {"Cin = max", desc(8, 9, 128, 4, 3, 3, 1, 1, C), 128, 64, 31, ok},
      {"Cin = max + 1", desc(8, 9, 129, 4, 3, 3, 1, 1, C), 128, 64, 31, cin},
      {"Cin, no limit", desc(8, 9, 100000, 4, 3, 3, 1, 1, C), PCNN_ANY, 64, 31, ok},
      {"Cout = 1", desc(8, 9, 4, 1, 3, 3, 1, 1, C), 64, 64, 31, ok},
      {"Cout = 0", with(base, [](pcnn_conv_desc& d) { d.Cout = 0; }), 64, 64, 31, cout},
      {"Cout = max", desc(8, 9, 4, 64, 3, 3, 1, 1, C), 64, 64, 31, ok},
      {"Cout = max + 1", desc(8, 9, 4, 65, 3, 3, 1, 1, C), 64, 64, 31, cout},
      {"Cout = 33 of 32", desc(8, 9, 4, 33, 3, 3, 1, 1, C), 64, 32, 31, cout},
      {"taps 1 x 1", desc(8, 9, 4, 4, 1, 1, 0, 0, C), 64, 64, 31, ok},
      {"kh = 0", desc(8, 9, 4, 4, 0, 3, 0, 1, C), 64, 64, 31, taps},
      {"kw = 0", desc(8, 9, 4, 4, 3, 0, 1, 0, C), 64, 64, 31, taps},
      {"taps 31 x 31", desc(8, 9, 4, 4, 31, 31, 15, 15, C), 64, 64, 31, ok},
      {"kh = 32", desc(8, 9, 4, 4, 32, 31, 15, 15, C), 64, 64, 31, taps},
      {"kw = 32", desc(8, 9, 4, 4, 31, 32, 15, 15, C), 64, 64, 31, taps},
      {"taps, no limit", desc(8, 9, 4, 4, 99, 99, 49, 49, C), 64, 64, PCNN_ANY, ok},
      {"ldx = Cin - 1", with(base, [](pcnn_conv_desc& d) { d.ldx = d.Cin - 1; }), 64, 64, 31, ld},
      {"ldy = Cout - 1", with(base, [](pcnn_conv_desc& d) { d.ldy = d.Cout - 1; }), 64, 64, 31, ld},
      {"wider strides", with(base, [](pcnn_conv_desc& d) { d.ldx = 64; d.ldy = 7; }), 64, 64, 31, ok},
      {"pad_mode -1", with(base, [](pcnn_conv_desc& d) { d.pad_mode = -1; }), 64, 64, 31, mode},
      {"pad_mode 3", with(base, [](pcnn_conv_desc& d) { d.pad_mode = 3; }), 64, 64, 31, mode},
      {"pad_mode 2", with(base, [](pcnn_conv_desc& d) { d.pad_mode = 2; }), 64, 64, 31, ok},
      // tf.pad: SYMMETRIC reaches H rows (W columns), REFLECT H - 1 (W - 1); each side on its own (the other three sides at 1)
      {"SYMMETRIC top = H", padded(8, 9, 8, 1, 1, 1, S), 64, 64, 31, ok},
      {"SYMMETRIC top = H + 1", padded(8, 9, 9, 1, 1, 1, S), 64, 64, 31, pad},
      {"SYMMETRIC bottom = H", padded(8, 9, 1, 8, 1, 1, S), 64, 64, 31, ok},
      {"SYMMETRIC bottom = H + 1", padded(8, 9, 1, 9, 1, 1, S), 64, 64, 31, pad},
      {"SYMMETRIC left = W", padded(8, 9, 1, 1, 9, 1, S), 64, 64, 31, ok},
      {"SYMMETRIC left = W + 1", padded(8, 9, 1, 1, 10, 1, S), 64, 64, 31, pad},
      {"SYMMETRIC right = W", padded(8, 9, 1, 1, 1, 9, S), 64, 64, 31, ok},
      {"SYMMETRIC right = W + 1", padded(8, 9, 1, 1, 1, 10, S), 64, 64, 31, pad},
      {"REFLECT top = H - 1", padded(8, 9, 7, 1, 1, 1, R), 64, 64, 31, ok},
      {"REFLECT top = H", padded(8, 9, 8, 1, 1, 1, R), 64, 64, 31, pad},
      {"REFLECT bottom = H - 1", padded(8, 9, 1, 7, 1, 1, R), 64, 64, 31, ok},
      {"REFLECT bottom = H", padded(8, 9, 1, 8, 1, 1, R), 64, 64, 31, pad},
      {"REFLECT left = W - 1", padded(8, 9, 1, 1, 8, 1, R), 64, 64, 31, ok},
      {"REFLECT left = W", padded(8, 9, 1, 1, 9, 1, R), 64, 64, 31, pad},
      {"REFLECT right = W - 1", padded(8, 9, 1, 1, 1, 8, R), 64, 64, 31, ok},
      {"REFLECT right = W", padded(8, 9, 1, 1, 1, 9, R), 64, 64, 31, pad},
      {"REFLECT of one row, no padding", with(padded(1, 9, 0, 2, 1, 1, R), [](pcnn_conv_desc& d) { d.kh = 1; d.Ho = 1; }), 64, 64, 31, ok},
      {"CONSTANT with any reach", padded(8, 9, 100, 200, 300, 400, C), 64, 64, 31, ok},
  };
  for (const Case& c : cases) {
    const char* got = pcnn_conv_desc_problem(&c.d, c.max_cin, c.max_cout, c.max_taps);
    const bool match = c.problem ? (got && strstr(got, c.problem)) : got == nullptr;
    if (!match) { printf("descriptor case '%s': expected %s, got %s\n", c.what, c.problem ? c.problem : "no problem", got ? got : "no problem"); exit(1); }
  }
  // the launchers' wrapper: entry point and numbers in the handle's error text, nothing on success
  pcnn_handle_s h{};
  CHECK(pcnn_check_conv_desc(&h, "pcnn_entry", &base, 64, 64, 31) == 0 && h.err.empty());
  const pcnn_conv_desc bad = desc(8, 9, 4, 80, 3, 3, 1, 1, C);
  CHECK(pcnn_check_conv_desc(&h, "pcnn_entry", &bad, 64, 64, 31) == 1);
  CHECK(strstr(h.err.c_str(), "pcnn_entry: Cout") == h.err.c_str() && strstr(h.err.c_str(), "80"));
  printf("%d descriptor cases\n", (int)(sizeof(cases) / sizeof(cases[0])));
}

static void test_small_helpers() {
  alignas(16) static float buf[8];
  CHECK(pcnn_quads_ok(buf, 4) && pcnn_quads_ok(buf, 0) && pcnn_quads_ok(buf + 4, 8));
  CHECK(!pcnn_quads_ok(buf + 1, 4) && !pcnn_quads_ok(buf, 6) && !pcnn_quads_ok(buf + 2, 4));
  CHECK(pcnn_cdiv(7, 4) == 2 && pcnn_cdiv(8, 4) == 2 && pcnn_cdiv64((int64_t)1 << 40, 3) == (((int64_t)1 << 40) + 2) / 3);
}

int main() {
  test_reserve();
  test_desc();
  test_small_helpers();
  printf("pcnn_host: all checks passed\n");
  return 0;
}
