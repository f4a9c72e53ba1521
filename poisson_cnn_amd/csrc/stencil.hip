// Weighted-Jacobi sweeps of a cross-shaped FD stencil of any odd size 3..9 per axis (layers/JacobiIterationLayer.py:7-66), several sweeps per
// launch by temporal blocking in LDS, and the adjoint w.r.t. the guess blocked the same way.  DESIGN.md section 11.
//
// One sweep: new = dinv * (rhs - sum_taps tap * u) where ry <= y < H - ry and rx <= x < W - rx, new = u on the ring (:48-52).
// A workgroup owns one JAC_TILE x JAC_TILE output tile of one sample.  After k sweeps the tile depends on the guess within k*ry rows and
// k*rx columns of it, so that region - clipped to the image, where the frozen ring ends the dependence - is loaded into LDS once; sweep s of k
// then computes the tile grown by (k - s) radii (again clipped), ping-ponging between two LDS buffers, and the last sweep stores the tile itself
// to memory.  rhs is needed from the first sweep's region on: a halo of (k - 1) radii.  The arithmetic per point (the H taps top to bottom,
// then the W taps left to right, one fmaf each into one accumulator; then dinv * (rhs - acc)) does not depend on k or on where the tile lies,
// so any split of n sweeps into launches gives the same bits.
#include "pcnn_internal.h"

#define JAC_TILE 64        // output tile edge
#define JAC_HALO_MAX 8     // k * max(ry, rx) <= JAC_HALO_MAX: the LDS region is at most (64 + 16)^2 floats per buffer
#define JAC_THREADS 512

namespace {

// Walks the rectangle (y0, x0, h, w) with the workgroup's threads in row-major order, without a division per point.
template <class F>
__device__ __forceinline__ void for_points(int tid, int y0, int x0, int h, int w, F body) {
  int q = tid / w, r = tid - q * w;
  const int dq = JAC_THREADS / w, dr = JAC_THREADS - dq * w;
  while (q < h) {
    body(y0 + q, x0 + r);
    q += dq; r += dr;
    if (r >= w) { r -= w; ++q; }
  }
}

// BWD == false: u -> k sweeps -> out.   BWD == true: u is d(out), out is d(guess), rhs unused.
template <int RY, int RX, bool BWD>
__global__ __launch_bounds__(JAC_THREADS) void jacobi_fused_kernel(int H, int W, int k, const float* __restrict__ coef, const float* __restrict__ u,
                                                                   const float* __restrict__ rhs, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int SY = 2 * RY + 1, SX = 2 * RX + 1;
  const int n = blockIdx.z, tid = threadIdx.x;
  const int ty0 = blockIdx.y * JAC_TILE, tx0 = blockIdx.x * JAC_TILE;
  const int ty1 = min(ty0 + JAC_TILE, H), tx1 = min(tx0 + JAC_TILE, W);
  // the region held in LDS: the tile grown by k radii, clipped to the image
  const int ly0 = max(ty0 - k * RY, 0), ly1 = min(ty1 + k * RY, H);
  const int lx0 = max(tx0 - k * RX, 0), lx1 = min(tx1 + k * RX, W);
  const int LW = lx1 - lx0;
  const int S = (JAC_TILE + 2 * k * RY) * (JAC_TILE + 2 * k * RX);   // floats per buffer as the host sized them
  float* src = lds;
  float* dst = lds + S;
  float* rb = lds + 2 * S;                                            // forward only

  const float* cn = coef + (int64_t)n * (SY + SX + 1);
  float cy[SY], cx[SX];
#pragma unroll
  for (int i = 0; i < SY; ++i) cy[i] = cn[i];
#pragma unroll
  for (int j = 0; j < SX; ++j) cx[j] = cn[SY + j];
  const float dinv = cn[SY + SX];

  const int64_t img = (int64_t)n * H * W;
  for_points(tid, ly0, lx0, ly1 - ly0, LW, [&](int y, int x) { src[(y - ly0) * LW + (x - lx0)] = u[img + (int64_t)y * W + x]; });
  if (!BWD) {
    const int ry0 = max(ty0 - (k - 1) * RY, 0), ry1 = min(ty1 + (k - 1) * RY, H);
    const int rx0 = max(tx0 - (k - 1) * RX, 0), rx1 = min(tx1 + (k - 1) * RX, W);
    for_points(tid, ry0, rx0, ry1 - ry0, rx1 - rx0, [&](int y, int x) { rb[(y - ly0) * LW + (x - lx0)] = rhs[img + (int64_t)y * W + x]; });
  }
  __syncthreads();

  for (int s = 1; s <= k; ++s) {
    const int g = k - s;                                              // radii this sweep's region still extends past the tile
    const int y0 = max(ty0 - g * RY, 0), y1 = min(ty1 + g * RY, H);
    const int x0 = max(tx0 - g * RX, 0), x1 = min(tx1 + g * RX, W);
    for_points(tid, y0, x0, y1 - y0, x1 - x0, [&](int y, int x) {
      const int c = (y - ly0) * LW + (x - lx0);
      const bool in_x = x >= RX && x < W - RX, in_y = y >= RY && y < H - RY;
      float v;
      if (!BWD) {
        if (in_x && in_y) {
          float acc = 0.f;
#pragma unroll
          for (int i = 0; i < SY; ++i)
            if (i != RY) acc = fmaf(cy[i], src[c + (i - RY) * LW], acc);
#pragma unroll
          for (int j = 0; j < SX; ++j)
            if (j != RX) acc = fmaf(cx[j], src[c + (j - RX)], acc);
          v = dinv * (rb[c] - acc);
        } else {
          v = src[c];
        }
      } else {
        // adjoint: gather from the interior points q = p - t whose stencil reached p with tap t
        float acc = 0.f;
        if (in_x) {
#pragma unroll
          for (int i = 0; i < SY; ++i) {
            const int qy = y - (i - RY);
            if (i != RY && qy >= RY && qy < H - RY) acc = fmaf(cy[i], src[c - (i - RY) * LW], acc);
          }
        }
        if (in_y) {
#pragma unroll
          for (int j = 0; j < SX; ++j) {
            const int qx = x - (j - RX);
            if (j != RX && qx >= RX && qx < W - RX) acc = fmaf(cx[j], src[c - (j - RX)], acc);
          }
        }
        v = ((in_x && in_y) ? 0.f : src[c]) - dinv * acc;
      }
      if (s == k) out[img + (int64_t)y * W + x] = v;                 // the last sweep's region is the tile itself
      else dst[c] = v;
    });
    __syncthreads();
    float* t = src; src = dst; dst = t;
  }
}

template <bool BWD>
int jacobi_launch(pcnn_handle_s* h, int N, int H, int W, int sy, int sx, int k, const float* coef, const float* u, const float* rhs, float* out) {
  const int ry = sy / 2, rx = sx / 2;
  const dim3 grid((unsigned)pcnn_cdiv(W, JAC_TILE), (unsigned)pcnn_cdiv(H, JAC_TILE), (unsigned)N);
  const size_t lds = (size_t)(BWD ? 2 : 3) * (JAC_TILE + 2 * k * ry) * (JAC_TILE + 2 * k * rx) * sizeof(float);
  auto go = [&](auto kernel) {
    set_lds(kernel, lds);
    hipLaunchKernelGGL(kernel, grid, dim3(JAC_THREADS), lds, h->stream, H, W, k, coef, u, rhs, out);
  };
#define JAC_CASE(A, B) \
  case A * 8 + B: go(jacobi_fused_kernel<A, B, BWD>); break;
  switch (ry * 8 + rx) {
    JAC_CASE(1, 1) JAC_CASE(1, 2) JAC_CASE(1, 3) JAC_CASE(1, 4)
    JAC_CASE(2, 1) JAC_CASE(2, 2) JAC_CASE(2, 3) JAC_CASE(2, 4)
    JAC_CASE(3, 1) JAC_CASE(3, 2) JAC_CASE(3, 3) JAC_CASE(3, 4)
    JAC_CASE(4, 1) JAC_CASE(4, 2) JAC_CASE(4, 3) JAC_CASE(4, 4)
    default: PCNN_FAIL(h, "pcnn_jacobi_fused: no kernel for a %d x %d stencil", sy, sx);
  }
#undef JAC_CASE
  return 0;
}

// n sweeps as ceil(n / k_max) launches of near-equal depth.  Intermediate results alternate between `out` and one handle-owned scratch image so
// that the last launch writes `out` and no launch reads what it writes.
template <bool BWD>
int jacobi_chain(pcnn_handle_s* h, const char* name, int N, int H, int W, int sy, int sx, const float* coef, const float* u, const float* rhs,
                 int n_sweeps, float* out) {
  const int kmax = pcnn_jacobi_fused_max_sweeps(sy, sx);
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
    const int rc = jacobi_launch<BWD>(h, N, H, W, sy, sx, k, coef, in, rhs, to);
    if (rc) return rc;
    in = to;
    left -= k;
  }
  PCNN_CHECK_LAUNCH(h, name);
  return 0;
}

bool jacobi_shape_ok(int N, int H, int W, int sy, int sx, int n_sweeps) {
  return N >= 1 && N <= 65535 && sy % 2 == 1 && sx % 2 == 1 && sy >= 3 && sy <= 9 && sx >= 3 && sx <= 9 && H > 2 * (sy / 2) && W > 2 * (sx / 2) && n_sweeps >= 1;
}

}  // namespace

extern "C" int pcnn_jacobi_fused_tile(void) { return JAC_TILE; }

extern "C" int pcnn_jacobi_fused_max_sweeps(int sy, int sx) {
  const int r = (sy > sx ? sy : sx) / 2;
  return r < 1 ? 0 : (JAC_HALO_MAX / r < 1 ? 1 : JAC_HALO_MAX / r);
}

extern "C" int pcnn_jacobi_fused_fwd(pcnn_handle h, int N, int H, int W, int sy, int sx, const float* coef, const float* u, const float* rhs, int n_sweeps,
                                     float* out) {
  PCNN_REQUIRE(h, h && coef && u && rhs && out, "pcnn_jacobi_fused_fwd: null argument");
  PCNN_REQUIRE(h, jacobi_shape_ok(N, H, W, sy, sx, n_sweeps),
               "pcnn_jacobi_fused_fwd: needs odd stencil sizes in 3..9, H > 2*(sy/2), W > 2*(sx/2), n_sweeps >= 1 (got %d x %d stencil, %d x %d image, %d sweeps)", sy, sx,
               H, W, n_sweeps);
  PCNN_REQUIRE(h, out != u && out != rhs, "pcnn_jacobi_fused_fwd: out must not alias u or rhs");
  return jacobi_chain<false>(h, "pcnn_jacobi_fused_fwd", N, H, W, sy, sx, coef, u, rhs, n_sweeps, out);
}

extern "C" int pcnn_jacobi_fused_bwd(pcnn_handle h, int N, int H, int W, int sy, int sx, const float* coef, const float* dout, int n_sweeps, float* du) {
  PCNN_REQUIRE(h, h && coef && dout && du, "pcnn_jacobi_fused_bwd: null argument");
  PCNN_REQUIRE(h, jacobi_shape_ok(N, H, W, sy, sx, n_sweeps),
               "pcnn_jacobi_fused_bwd: needs odd stencil sizes in 3..9, H > 2*(sy/2), W > 2*(sx/2), n_sweeps >= 1 (got %d x %d stencil, %d x %d image, %d sweeps)", sy, sx,
               H, W, n_sweeps);
  PCNN_REQUIRE(h, du != dout, "pcnn_jacobi_fused_bwd: du must not alias dout");
  return jacobi_chain<true>(h, "pcnn_jacobi_fused_bwd", N, H, W, sy, sx, coef, dout, nullptr, n_sweeps, du);
}
