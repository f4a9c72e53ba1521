// The blocked-sweep scaffolding shared by the constant-coefficient smoother (stencil.hip) and the variable-density one (varcoef_train.hip):
// the workgroup walker, the clipped tile frame, the host chain of launches, and the launch checks.  DESIGN.md section 11.
// What a sweep computes at a point, the tile edge, the thread count and the halo cap stay with each file; nothing here fixes them.
#pragma once
#include "pcnn_internal.h"

// Walks the rectangle (y0, x0, h, w) with the workgroup's THREADS threads in row-major order, without a division per point.
template <int THREADS, class F>
__device__ __forceinline__ void pcnn_for_points(int tid, int y0, int x0, int h, int w, F body) {
  int q = tid / w, r = tid - q * w;
  const int dq = THREADS / w, dr = THREADS - dq * w;
  while (q < h) {
    body(y0 + q, x0 + r);
    q += dq; r += dr;
    if (r >= w) { r -= w; ++q; }
  }
}

// The workgroup's TILE x TILE tile of an H x W image (blockIdx.y / .x), and the rectangle held in LDS row-major from (ly0, lx0), LW floats per row.
template <int TILE>
struct pcnn_frame {
  int H, W, ty0, ty1, tx0, tx1, ly0, ly1, lx0, lx1, LW;
  __device__ __forceinline__ pcnn_frame(int H_, int W_) : H(H_), W(W_) {
    ty0 = blockIdx.y * TILE; tx0 = blockIdx.x * TILE;
    ty1 = min(ty0 + TILE, H); tx1 = min(tx0 + TILE, W);
  }
  // the tile grown by gy rows and gx columns, clipped to the image
  __device__ __forceinline__ void grow(int gy, int gx, int& y0, int& y1, int& x0, int& x1) const {
    y0 = max(ty0 - gy, 0); y1 = min(ty1 + gy, H);
    x0 = max(tx0 - gx, 0); x1 = min(tx1 + gx, W);
  }
  __device__ __forceinline__ void hold(int y0, int y1, int x0, int x1) { ly0 = y0; ly1 = y1; lx0 = x0; lx1 = x1; LW = x1 - x0; }
  __device__ __forceinline__ int at(int y, int x) const { return (y - ly0) * LW + (x - lx0); }
};

// n sweeps as ceil(n / kmax) launches of near-equal depth, launch(k, in, to) -> rc each.  Intermediate results alternate between `out` and one
// handle-owned scratch image so that the last launch writes `out` and no launch reads what it writes.
template <class L>
int pcnn_sweep_chain(pcnn_handle_s* h, const char* name, int N, int H, int W, int n_sweeps, int kmax, const float* u, float* out, L launch) {
  const int launches = pcnn_cdiv(n_sweeps, kmax);
  float* tmp = nullptr;
  if (launches > 1) {
    if (pcnn_reserve(h, h->aux_ws, (size_t)N * H * W * sizeof(float), 0, name)) return 1;
    tmp = static_cast<float*>(h->aux_ws.p);
  }
  const float* in = u;
  int left = n_sweeps;
  for (int l = 0; l < launches; ++l) {
    const int k = pcnn_cdiv(left, launches - l);
    float* to = ((launches - 1 - l) % 2 == 0) ? out : tmp;
    if (int rc = launch(k, in, to)) return rc;
    in = to;
    left -= k;
  }
  PCNN_CHECK_LAUNCH(h, name);
  return 0;
}

// The dynamic LDS of a launch against the 160 KB a workgroup can have (the message is the caller's), and the launch with that much allowed.
#define PCNN_REQUIRE_LDS(h, lds, ...) PCNN_REQUIRE(h, (lds) <= 160u * 1024u, __VA_ARGS__)
template <class K, class... A>
void pcnn_launch_lds(pcnn_handle_s* h, K kernel, dim3 grid, int threads, size_t lds, A... args) {
  set_lds(kernel, lds);
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, h->stream, args...);
}

// a batch of N images as grid.z
static inline bool pcnn_grid_ok(int N, int H, int W) { return N >= 1 && N <= 65535 && H >= 1 && W >= 1; }
