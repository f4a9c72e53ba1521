// Host half of the libpcnn internals: the handle, the error macros, the handle-owned buffers and the argument checks the launchers share.
// No device code and no hip_runtime.h: a plain C++17 compiler takes this header (tests/host/test_pcnn_host.cpp runs it without a GPU).
#pragma once
#include <hip/hip_runtime_api.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../../include/pcnn.h"

// A device buffer the handle owns and grows on demand (pcnn_reserve); never shrunk except by pcnn_drop / pcnn_destroy.
struct pcnn_buffer { void* p = nullptr; size_t bytes = 0; };

struct pcnn_handle_s {
  int device;
  hipStream_t stream;
  std::string err;
  pcnn_buffer scratch;            // packed filters of the convolution / deconvolution launchers, partial sums of pcnn_loss_partials
  int math_mode = 0;              // PCNN_MATH_FP32 (exact fp32 MFMA) or PCNN_MATH_SPLIT_F16 (3 x fp16 split, fp32 accumulate)
  float* y_absmax = nullptr;      // set by pcnn_conv2d_fwd_absmax for the duration of one forward launch: receives max|y|
  pcnn_buffer spec_ws;            // spectral-convolution workspace (tables, filter spectrum, tile spectra)
  size_t spec_ws_limit = 0;       // caller's cap on the spectral workspace in bytes (0: none), pcnn_set_workspace_limit
  pcnn_buffer aux_ws;             // intermediates and partial sums of the two-pass resize, pcnn_sweep_chain (sweep_common.h: the fused Jacobi sweeps of stencil.hip and varcoef_train.hip), pcnn_sample_scale_bwd, pcnn_conv2d_dgrad_post, pcnn_grouped_deconv_bwd_filter, pcnn_varcoef_pi_loss_partials, pcnn_varcoef_bc_jacobi_bwd_inputs (the recomputed iterates)
  int spectral_mode = -1;         // PCNN_SPECTRAL_AUTO (cost model) / _OFF / _FORCE, see pcnn_set_spectral_mode
  int spectral_tile = 0;          // 0: per layer (pick_tile), 32 / 64: that tile size wherever the layer allows it, see pcnn_set_spectral_tile
  int spectral_xform = 1;         // transform kernels of the spectral route: 1 = in-register FFT on the vector ALUs (default since round 5), 0 = DFT as a GEMM on the matrix cores (pcnn_set_spectral_transform)
  int retain = 0;                 // pcnn_set_workspace_retain: outgrown handle-owned buffers are kept (a captured hipGraph may still replay into them)
  std::vector<void*> retired;     // ... here, until pcnn_destroy
  unsigned long long filter_version = 0;   // pcnn_set_filter_version: 0 = filter spectra are recomputed by every call; else the caller's weights version
  void* filter_cache = nullptr;   // ... and the spectra kept per (filter pointer, shape, tile size), spectral_conv.hip
  long long fc_hits = 0, fc_fills = 0, fc_refreshes = 0;   // cumulative over the handle's life (pcnn_filter_cache_clear empties the cache, not these)
  void* comm = nullptr;           // RCCL communicator (ncclComm_t) of pcnn_comm_init, see collective.hip
  int comm_rank = 0, comm_size = 0;
};

#define PCNN_FAIL(h, ...)                                   \
  do {                                                      \
    char _b[512];                                           \
    snprintf(_b, sizeof(_b), __VA_ARGS__);                  \
    if (h) (h)->err = _b;                                   \
    return 1;                                               \
  } while (0)

#define PCNN_REQUIRE(h, cond, ...) \
  do {                             \
    if (!(cond)) PCNN_FAIL(h, __VA_ARGS__); \
  } while (0)

#define PCNN_CHECK_LAUNCH(h, name)                                               \
  do {                                                                           \
    hipError_t _e = hipGetLastError();                                           \
    if (_e != hipSuccess) PCNN_FAIL(h, "%s: %s", name, hipGetErrorString(_e));   \
  } while (0)

static inline int pcnn_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int64_t pcnn_cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// A handle-owned buffer is being outgrown (or capped): free it once the stream has drained - unless the caller declared that recorded work
// (a hipGraph captured on this handle's stream) may still use it; then it is parked until pcnn_destroy.
static inline void pcnn_release(pcnn_handle_s* h, void* p) {
  if (!p) return;
  if (h->retain) { h->retired.push_back(p); return; }
  (void)hipStreamSynchronize(h->stream);
  (void)hipFree(p);
}

static inline void pcnn_drop(pcnn_handle_s* h, pcnn_buffer& b) {
  pcnn_release(h, b.p);
  b = pcnn_buffer();
}

// Makes b hold at least `need` bytes.  A buffer that is large enough stays as it is (old contents and address included); otherwise the old block goes
// through pcnn_release and max(need, min_bytes) bytes are allocated - the old contents are gone, *grew (if given) says so.  Stream-ordered reuse by several
// entry points is safe because a handle has one stream and every user fills the buffer before it reads it.  On failure: b is empty, HIP's sticky
// last error is consumed (the next PCNN_CHECK_LAUNCH must not report it as a launch failure), h->err = "<who>: cannot allocate ...", returns 1.
static inline int pcnn_reserve(pcnn_handle_s* h, pcnn_buffer& b, size_t need, size_t min_bytes, const char* who, bool* grew = nullptr) {
  if (grew) *grew = false;
  if (b.bytes >= need) return 0;
  pcnn_drop(h, b);
  const size_t cap = need < min_bytes ? min_bytes : need;
  if (hipMalloc(&b.p, cap) != hipSuccess) {
    (void)hipGetLastError();
    b = pcnn_buffer();
    PCNN_FAIL(h, "%s: cannot allocate %zu B of scratch", who, cap);
  }
  b.bytes = cap;
  if (grew) *grew = true;
  return 0;
}
constexpr size_t PCNN_SCRATCH_FLOOR = (size_t)4 << 20;   // what the convolution launchers take at once, so that a model's layers do not grow the scratch one by one

// dynamic LDS beyond 64 KB has to be allowed per kernel before its first launch
template <typename K>
void set_lds(K kernel, size_t bytes) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); }

// whole 16-byte pieces of a channel vector may be loaded / stored: base aligned, pixel stride a multiple of 4 floats
static inline bool pcnn_quads_ok(const void* p, int ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }

// What is wrong with a convolution descriptor (nullptr: nothing), for a launcher that takes up to max_cin / max_cout channels and max_taps filter
// taps per axis (PCNN_ANY: no limit of its own).  Everything the kernels assume without looking: non-empty tensors, channel strides that cover the
// channels, a known pad_mode, and - for SYMMETRIC / REFLECT - that every read resolves inside the image: the farthest tap of the first and of the
// last output must be within tf.pad's reach (H | H - 1 rows), else pcnn_pad_index would clamp where TensorFlow refuses.
constexpr int PCNN_ANY = INT_MAX;
static inline const char* pcnn_conv_desc_problem(const pcnn_conv_desc* d, int max_cin, int max_cout, int max_taps) {
  if (!(d->N > 0 && d->H > 0 && d->W > 0 && d->Ho > 0 && d->Wo > 0)) return "empty tensor";
  if (!(d->Cin >= 1 && d->Cin <= max_cin)) return "Cin unsupported";
  if (!(d->Cout >= 1 && d->Cout <= max_cout)) return "Cout unsupported";
  if (!(d->kh >= 1 && d->kw >= 1 && d->kh <= max_taps && d->kw <= max_taps)) return "filter size unsupported";
  if (!(d->ldx >= d->Cin && d->ldy >= d->Cout)) return "channel stride smaller than channel count";
  if (!(d->pad_mode >= 0 && d->pad_mode <= 2)) return "bad pad_mode";
  if (d->pad_mode != PCNN_PAD_CONSTANT) {
    const int lim_y = d->pad_mode == PCNN_PAD_SYMMETRIC ? d->H : d->H - 1, lim_x = d->pad_mode == PCNN_PAD_SYMMETRIC ? d->W : d->W - 1;
    const int pb = d->Ho - 1 - d->pad_top + d->kh - 1 - (d->H - 1), pr = d->Wo - 1 - d->pad_left + d->kw - 1 - (d->W - 1);
    if (!(d->pad_top <= lim_y && pb <= lim_y && d->pad_left <= lim_x && pr <= lim_x)) return "padding exceeds what tf.pad allows";
  }
  return nullptr;
}
// ... as a launcher's first check after its null-pointer test: sets the handle's error text (with the numbers) and returns 1
static inline int pcnn_check_conv_desc(pcnn_handle_s* h, const char* who, const pcnn_conv_desc* d, int max_cin, int max_cout, int max_taps) {
  if (const char* why = pcnn_conv_desc_problem(d, max_cin, max_cout, max_taps))
    PCNN_FAIL(h, "%s: %s (%d x %d x %d x %d, stride %d -> %d x %d x %d, stride %d; %d x %d taps, pad %d | %d, pad_mode %d)", who, why,
              d->N, d->H, d->W, d->Cin, d->ldx, d->Ho, d->Wo, d->Cout, d->ldy, d->kh, d->kw, d->pad_top, d->pad_left, d->pad_mode);
  return 0;
}
