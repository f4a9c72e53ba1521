// Internal helpers shared by the libpcnn translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include "pcnn_host.h"

void pcnn_comm_release(pcnn_handle_s* h);   // collective.hip
void pcnn_filter_cache_free(pcnn_handle_s* h);   // spectral_conv.hip

// The unknowns of a 5-point solve with per-edge Dirichlet / Neumann conditions: rows i0..i1 x columns j0..j1 of the H x W grid (mh x mw of them).
// types bit 0/1/2/3 = left / right / bottom / top is Neumann: that edge's nodes are unknowns, a Dirichlet edge's are given.
struct FdUnknowns { int i0, i1, j0, j1, mh, mw; };
__host__ __device__ inline FdUnknowns fd_unknowns(int H, int W, int types) {
  FdUnknowns u;
  u.i0 = (types & 1) ? 0 : 1; u.i1 = (types & 2) ? H - 1 : H - 2; u.j0 = (types & 4) ? 0 : 1; u.j1 = (types & 8) ? W - 1 : W - 2;
  u.mh = u.i1 - u.i0 + 1; u.mw = u.j1 - u.j0 + 1;
  return u;
}

// dataset.hip: the two steps of the FD Poisson pipeline that varcoef.hip runs too.
// dst = A_h src A_w per sample (A_h mh x mh and A_w mw x mw, shared by the batch) as two pcnn_batched_gemm_f64: mid = A_h src, dst = mid A_w; dst may be src
int pcnn_two_sided_gemm_f64(pcnn_handle h, int N, int mh, int mw, const double* A_h, const double* src, const double* A_w, double* mid, double* dst);
// soln (N,H,W) fp32 <- the unknowns U (fp64; rows / columns of a Neumann edge included, types bit 0/1/2/3 = left / right / bottom / top is Neumann) and
// the Dirichlet ring from the edge arrays; rows 0 / H-1 (left / right) win at the corners.  Launch only: the caller checks it.
void pcnn_fd_write_soln(pcnn_handle h, int N, int H, int W, int types, const double* U, const float* left, const float* right, const float* bottom,
                        const float* top, float* soln);

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float pcnn_act(float v, int act, float alpha) {
  switch (act) {
    case PCNN_ACT_LEAKY_RELU: return v > 0.f ? v : alpha * v;
    case PCNN_ACT_TANH: return tanhf(v);
    case PCNN_ACT_RELU: return v > 0.f ? v : 0.f;
    default: return v;
  }
}
// derivative of the activation expressed through its OUTPUT a = act(z)
__device__ __forceinline__ float pcnn_act_grad_from_out(float a, int act, float alpha) {
  switch (act) {
    case PCNN_ACT_LEAKY_RELU: return a > 0.f ? 1.f : alpha;
    case PCNN_ACT_TANH: return 1.f - a * a;
    case PCNN_ACT_RELU: return a > 0.f ? 1.f : 0.f;
    default: return 1.f;
  }
}

// red[0] <- op over red[0 .. THREADS) by the plain halving tree, a barrier per level; the caller's barrier after filling red comes first.
// Every thread of the block calls it with its index.  The order of the operations is fixed, so the same values give the same bits.
template <class T, int THREADS, class Op>
__device__ __forceinline__ void pcnn_block_reduce(T* red, int tid, Op op) {
#pragma unroll
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = op(red[tid], red[tid + s]);
    __syncthreads();
  }
}
struct pcnn_sum_op { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct pcnn_min_op { __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); } };
template <class T, int THREADS>
__device__ __forceinline__ void pcnn_block_sum(T* red, int tid) { pcnn_block_reduce<T, THREADS>(red, tid, pcnn_sum_op()); }

// a 1-D grid of `block`-thread blocks over `total` items, at most maxb of them (grid-stride kernels take the rest), at least one
static inline dim3 pcnn_grid1d(int64_t total, int block, int maxb) {
  int64_t b = pcnn_cdiv64(total, block);
  if (b > maxb) b = maxb;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

// tf.pad index map.  Returns the source index in [0,n) or -1 for "use the constant".
__device__ __forceinline__ int pcnn_pad_index(int i, int n, int mode) {
  if (i >= 0 && i < n) return i;
  if (mode == PCNN_PAD_CONSTANT) return -1;
  int r;
  if (mode == PCNN_PAD_SYMMETRIC) r = i < 0 ? -i - 1 : 2 * n - 1 - i;
  else r = i < 0 ? -i : 2 * n - 2 - i;
  return r < 0 ? 0 : (r >= n ? n - 1 : r);   // clamp: only reached by tile overhang that is never stored
}
