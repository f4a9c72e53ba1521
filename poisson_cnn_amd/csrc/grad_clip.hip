// Gradient clipping on the flat gradient bucket (tf.keras OptimizerV2 `clipnorm` / `global_clipnorm` / `clipvalue`, TF 2.4; the formulas are in
// include/pcnn.h).  A bucket is cut into ITEMS by a host-side plan: (variable id, start, length <= PCNN_GRAD_CLIP_CHUNK), no item crosses a
// variable boundary.  Three streaming passes over memory the optimizer already owns:
//   grad_sqnorm_partials_kernel   one workgroup per item: fp32 sum of (grad_scale g)^2 in a FIXED order -> partial[item]
//   grad_var_sums_kernel          per variable: its partials added in plan order (double), the bucket total (double)
//   grad_clip_scales_kernel       per-variable or global scale from those sums (several buckets: their totals added in order)
//   grad_clip_apply_kernel        one workgroup per item: g <- clamp((grad_scale g) scale, -c, c) in place; items with scale == 1 are left alone
// No float atomics anywhere: every sum has one order, fixed by the plan, so a result depends on (gradient, plan) and on nothing else.
#include "pcnn_internal.h"
#include <math.h>

#define GC_THREADS 256
#define GC_WAVES (GC_THREADS / 64)

static_assert(PCNN_GRAD_CLIP_CHUNK % (4 * GC_THREADS) == 0, "a full item is a whole number of float4 rounds of the workgroup");

// An item's floats as [head | body of float4 | tail]: head = the 0..3 floats in front of the first 16-byte boundary (variable offsets are arbitrary:
// a 1-element bias sits between two kernels), tail = the 0..3 floats after the last whole float4.  Both are read with scalar loads.
struct gc_split { int head, nvec, tail; };

__device__ __forceinline__ gc_split gc_split_item(const float* p, int len) {
  gc_split s;
  const int mis = (int)(((uintptr_t)p >> 2) & 3);        // p is 4-byte aligned (a float of the bucket)
  s.head = mis ? min(4 - mis, len) : 0;
  s.nvec = (len - s.head) >> 2;
  s.tail = len - s.head - 4 * s.nvec;
  return s;
}

// Order of the sum (the error bound of tests/grad_clip_twin.py counts its depth): lane t adds its head float, then its float4s t, t+256, ... component
// by component, then its tail float - at most CHUNK/256 + 2 terms one after the other; a 6-level butterfly joins the 64 lanes of a wave; thread 0 adds
// the 4 wave sums from LDS as (w0 + w1) + (w2 + w3).
__global__ __launch_bounds__(GC_THREADS) void grad_sqnorm_partials_kernel(const float* __restrict__ g, const int64_t* __restrict__ item_start,
                                                                           const int* __restrict__ item_len, float gscale,
                                                                           float* __restrict__ partial) {
  __shared__ float wsum[GC_WAVES];
  const int item = blockIdx.x, t = threadIdx.x;
  const float* p = g + item_start[item];
  const int len = item_len[item];
  const gc_split s = gc_split_item(p, len);
  float acc = 0.f;
  if (t < s.head) { const float x = gscale * p[t]; acc += x * x; }
  const f32x4* pv = reinterpret_cast<const f32x4*>(p + s.head);
  for (int i = t; i < s.nvec; i += GC_THREADS) {
    const f32x4 v = pv[i];
    const float x0 = gscale * v[0], x1 = gscale * v[1], x2 = gscale * v[2], x3 = gscale * v[3];
    acc += x0 * x0; acc += x1 * x1; acc += x2 * x2; acc += x3 * x3;
  }
  if (t < s.tail) { const float x = gscale * p[s.head + 4 * s.nvec + t]; acc += x * x; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((t & 63) == 0) wsum[t >> 6] = acc;
  __syncthreads();
  if (t == 0) partial[item] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// One workgroup.  Thread t owns variables t, t+256, ...: the variable's partials in plan order into a double.  Thread 0 then adds the variables in
// order: a few hundred doubles.
__global__ __launch_bounds__(GC_THREADS) void grad_var_sums_kernel(int n_vars, const int* __restrict__ var_first_item, const float* __restrict__ partial,
                                                                    double* __restrict__ var_sq, float* __restrict__ sqnorm, double* __restrict__ total) {
  for (int v = threadIdx.x; v < n_vars; v += GC_THREADS) {
    double a = 0.0;
    for (int i = var_first_item[v]; i < var_first_item[v + 1]; ++i) a += (double)partial[i];
    var_sq[v] = a;
    if (sqnorm) sqnorm[v] = (float)a;
  }
  if (!total) return;
  __syncthreads();                       // one workgroup: var_sq of every variable is written (global writes of a block are visible to it after the barrier)
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int v = 0; v < n_vars; ++v) a += var_sq[v];
    *total = a;
  }
}

__device__ __forceinline__ float gc_scale_from_sq(double sq, float c, bool nan_if_not_finite) {
  const double nrm = sqrt(sq);
  if (nan_if_not_finite && !(nrm <= 1.7976931348623157e308)) return __builtin_nanf("");     // inf or NaN norm: tf.clip_by_global_norm yields NaN
  return nrm <= (double)c ? 1.0f : (float)((double)c / nrm);                                 // a NaN norm compares false: c / NaN = NaN
}

// One workgroup.  PER_VARIABLE: scale[v] from var_sq[v].  GLOBAL: scale[0] from the totals of every participating bucket, added in order.
// global_norm (optional): sqrt of that sum, as fp32.
__global__ __launch_bounds__(GC_THREADS) void grad_clip_scales_kernel(int mode, float c, int n_vars, const double* __restrict__ var_sq, int n_totals,
                                                                       const double* __restrict__ totals, float* __restrict__ scale,
                                                                       float* __restrict__ global_norm) {
  if (mode == PCNN_GRAD_CLIP_PER_VARIABLE)
    for (int v = threadIdx.x; v < n_vars; v += GC_THREADS) scale[v] = gc_scale_from_sq(var_sq[v], c, false);
  if (threadIdx.x == 0 && (mode == PCNN_GRAD_CLIP_GLOBAL || global_norm)) {
    double a = 0.0;
    for (int k = 0; k < n_totals; ++k) a += totals[k];
    if (mode == PCNN_GRAD_CLIP_GLOBAL) scale[0] = gc_scale_from_sq(a, c, true);
    if (global_norm) *global_norm = (float)sqrt(a);
  }
}

__device__ __forceinline__ float gc_clip1(float g, float gscale, float sc, bool clamp, float cv) {
  float x = (gscale * g) * sc;
  if (clamp) x = x < -cv ? -cv : (x > cv ? cv : x);      // comparisons, not fminf / fmaxf: a NaN stays a NaN (tf.clip_by_value)
  return x;
}

__global__ __launch_bounds__(GC_THREADS) void grad_clip_apply_kernel(float* __restrict__ g, const int* __restrict__ item_var,
                                                                      const int64_t* __restrict__ item_start, const int* __restrict__ item_len, int mode,
                                                                      const float* __restrict__ scale, float gscale, int clamp, float cv) {
  const int item = blockIdx.x, t = threadIdx.x;
  // the scale's address depends on the block index only: one value for the whole workgroup
  const float sc = mode == PCNN_GRAD_CLIP_GLOBAL ? scale[0] : mode == PCNN_GRAD_CLIP_PER_VARIABLE ? scale[item_var[item]] : 1.0f;
  if (sc == 1.0f && !clamp && gscale == 1.0f) return;    // nothing to do: the item keeps its bits
  float* p = g + item_start[item];
  const int len = item_len[item];
  const gc_split s = gc_split_item(p, len);
  if (t < s.head) p[t] = gc_clip1(p[t], gscale, sc, clamp, cv);
  f32x4* pv = reinterpret_cast<f32x4*>(p + s.head);
  for (int i = t; i < s.nvec; i += GC_THREADS) {
    f32x4 v = pv[i];
    v[0] = gc_clip1(v[0], gscale, sc, clamp, cv); v[1] = gc_clip1(v[1], gscale, sc, clamp, cv);
    v[2] = gc_clip1(v[2], gscale, sc, clamp, cv); v[3] = gc_clip1(v[3], gscale, sc, clamp, cv);
    pv[i] = v;
  }
  if (t < s.tail) { float* q = p + s.head + 4 * s.nvec + t; *q = gc_clip1(*q, gscale, sc, clamp, cv); }
}

// ------------------------------------------------------------------------------------------------------------------ host: the plan
extern "C" int64_t pcnn_grad_clip_plan_items(int n_vars, const int64_t* sizes) {
  if (n_vars < 0 || (n_vars > 0 && !sizes)) return -1;
  int64_t n = 0;
  for (int v = 0; v < n_vars; ++v) {
    if (sizes[v] < 0) return -1;
    n += pcnn_cdiv64(sizes[v], PCNN_GRAD_CLIP_CHUNK);
  }
  return n;
}

extern "C" int pcnn_grad_clip_plan(int n_vars, const int64_t* sizes, int32_t* item_var, int64_t* item_start, int32_t* item_len, int32_t* var_first_item) {
  const int64_t n_items = pcnn_grad_clip_plan_items(n_vars, sizes);
  if (n_items < 0 || n_items > INT32_MAX || !var_first_item || (n_items > 0 && !(item_var && item_start && item_len))) return 1;
  int64_t off = 0;
  int32_t k = 0;
  for (int v = 0; v < n_vars; ++v) {
    var_first_item[v] = k;
    for (int64_t done = 0; done < sizes[v]; done += PCNN_GRAD_CLIP_CHUNK, ++k) {
      item_var[k] = v;
      item_start[k] = off + done;
      item_len[k] = (int32_t)(sizes[v] - done < PCNN_GRAD_CLIP_CHUNK ? sizes[v] - done : PCNN_GRAD_CLIP_CHUNK);
    }
    off += sizes[v];
  }
  var_first_item[n_vars] = k;
  return 0;
}

static inline size_t gc_partials_bytes(int64_t n_items) { return ((size_t)n_items * sizeof(float) + 7) & ~(size_t)7; }

extern "C" size_t pcnn_grad_clip_workspace(int64_t n_items, int n_vars) {
  if (n_items < 0 || n_vars < 0) return 0;
  return gc_partials_bytes(n_items) + (size_t)n_vars * sizeof(double);
}

// ------------------------------------------------------------------------------------------------------------------ device entry points
extern "C" int pcnn_grad_clip_norms(pcnn_handle h, const float* g, int64_t n_items, const int64_t* item_start, const int32_t* item_len, int n_vars,
                                    const int32_t* var_first_item, float grad_scale, void* workspace, float* sqnorm, double* total) {
  PCNN_REQUIRE(h, h && n_items >= 0 && n_items <= INT32_MAX && n_vars >= 0, "pcnn_grad_clip_norms: bad argument");
  PCNN_REQUIRE(h, workspace && var_first_item && ((uintptr_t)workspace & 7) == 0, "pcnn_grad_clip_norms: the workspace must be 8-byte aligned");
  PCNN_REQUIRE(h, n_items == 0 || (g && item_start && item_len), "pcnn_grad_clip_norms: null argument");
  float* partial = (float*)workspace;
  double* var_sq = (double*)((char*)workspace + gc_partials_bytes(n_items));
  if (n_items > 0) {
    hipLaunchKernelGGL(grad_sqnorm_partials_kernel, dim3((unsigned)n_items), dim3(GC_THREADS), 0, h->stream, g, item_start, item_len, grad_scale, partial);
    PCNN_CHECK_LAUNCH(h, "pcnn_grad_clip_norms (partials)");
  }
  hipLaunchKernelGGL(grad_var_sums_kernel, dim3(1), dim3(GC_THREADS), 0, h->stream, n_vars, var_first_item, partial, var_sq, sqnorm, total);
  PCNN_CHECK_LAUNCH(h, "pcnn_grad_clip_norms (sums)");
  return 0;
}

extern "C" int pcnn_grad_clip_scales(pcnn_handle h, int mode, float c, int64_t n_items, int n_vars, const void* workspace, int n_totals,
                                     const double* totals, float* scale, float* global_norm) {
  PCNN_REQUIRE(h, h && (mode == PCNN_GRAD_CLIP_NONE || mode == PCNN_GRAD_CLIP_PER_VARIABLE || mode == PCNN_GRAD_CLIP_GLOBAL), "pcnn_grad_clip_scales: bad mode");
  PCNN_REQUIRE(h, mode == PCNN_GRAD_CLIP_NONE || (c >= 0.f && scale), "pcnn_grad_clip_scales: the clip norm must be >= 0 and `scale` given");
  PCNN_REQUIRE(h, mode != PCNN_GRAD_CLIP_PER_VARIABLE || (workspace && n_items >= 0 && n_vars >= 0), "pcnn_grad_clip_scales: per-variable mode needs the workspace of pcnn_grad_clip_norms");
  PCNN_REQUIRE(h, n_totals >= 0 && (n_totals == 0 || totals), "pcnn_grad_clip_scales: bad totals");
  PCNN_REQUIRE(h, (mode != PCNN_GRAD_CLIP_GLOBAL && !global_norm) || n_totals > 0, "pcnn_grad_clip_scales: a global norm needs the bucket totals");
  const double* var_sq = workspace ? (const double*)((const char*)workspace + gc_partials_bytes(n_items)) : nullptr;
  hipLaunchKernelGGL(grad_clip_scales_kernel, dim3(1), dim3(GC_THREADS), 0, h->stream, mode, c, n_vars, var_sq, n_totals, totals, scale, global_norm);
  PCNN_CHECK_LAUNCH(h, "pcnn_grad_clip_scales");
  return 0;
}

extern "C" int pcnn_grad_clip_apply(pcnn_handle h, float* g, int64_t n_items, const int32_t* item_var, const int64_t* item_start, const int32_t* item_len,
                                    int mode, const float* scale, float grad_scale, float clipvalue) {
  PCNN_REQUIRE(h, h && n_items >= 0 && n_items <= INT32_MAX, "pcnn_grad_clip_apply: bad argument");
  PCNN_REQUIRE(h, mode == PCNN_GRAD_CLIP_NONE || mode == PCNN_GRAD_CLIP_PER_VARIABLE || mode == PCNN_GRAD_CLIP_GLOBAL, "pcnn_grad_clip_apply: bad mode");
  PCNN_REQUIRE(h, mode == PCNN_GRAD_CLIP_NONE || scale, "pcnn_grad_clip_apply: a norm mode needs `scale`");
  if (n_items == 0) return 0;
  PCNN_REQUIRE(h, g && item_var && item_start && item_len, "pcnn_grad_clip_apply: null argument");
  const int clamp = clipvalue >= 0.f ? 1 : 0;            // a negative clipvalue means "none"
  hipLaunchKernelGGL(grad_clip_apply_kernel, dim3((unsigned)n_items), dim3(GC_THREADS), 0, h->stream, g, item_var, item_start, item_len, mode, scale, grad_scale,
                     clamp, clipvalue);
  PCNN_CHECK_LAUNCH(h, "pcnn_grad_clip_apply");
  return 0;
}
