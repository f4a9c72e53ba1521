// Every Jacobi sweep of the constant-coefficient operator.  The one-sweep 3 x 3 pair (jacobi_kernel / jacobi_bwd_kernel: one launch per sweep, the
// model's default route), and weighted-Jacobi sweeps of a cross-shaped FD stencil of any odd size 3..9 per axis (layers/JacobiIterationLayer.py:7-66),
// several sweeps per launch by temporal blocking in LDS, with the adjoint w.r.t. the guess blocked the same way.  DESIGN.md section 11.
// The walker, the tile frame, the launch chain and the launch checks are sweep_common.h's, shared with varcoef_train.hip.
//
// One sweep: new = dinv * (rhs - sum_taps tap * u) where ry <= y < H - ry and rx <= x < W - rx, new = u on the ring (:48-52).
// A workgroup owns one JAC_TILE x JAC_TILE output tile of one sample.  After k sweeps the tile depends on the guess within k*ry rows and
// k*rx columns of it, so that region - clipped to the image, where the frozen ring ends the dependence - is loaded into LDS once; sweep s of k
// then computes the tile grown by (k - s) radii (again clipped), ping-ponging between two LDS buffers, and the last sweep stores the tile itself
// to memory.  rhs is needed from the first sweep's region on: a halo of (k - 1) radii.  The arithmetic per point (the H taps top to bottom,
// then the W taps left to right, one fmaf each into one accumulator; then dinv * (rhs - acc)) does not depend on k or on where the tile lies,
// so any split of n sweeps into launches gives the same bits.
//
// BC == true (pcnn_jacobi_fused_bc_*): one sweep is R_m o J.  R_m refreshes the frozen band where every edge that contains the point is Neumann
// (neumann_mask, include/pcnn.h): the point takes J(u) at its SYMMETRIC mirror image in the interior; a band point on a Dirichlet edge stays
// frozen.  A refreshed point depends on J(u) up to 2r - 1 points away, so the regions follow a recurrence (jac_range) instead of the plain
// (k - s) radii: each sweep's computed region includes the mirror sources of the band points it has to deliver, and the adjoint's includes the
// band points that mirror into it.  The refresh reads values other threads wrote in the same sweep and has a barrier of its own; a sweep whose
// region meets no Neumann band (workgroup-uniform) takes the BC == false path.  The BC == false instantiations are the code they were.
#include "sweep_common.h"

#define JAC_TILE 64        // output tile edge
#define JAC_HALO_MAX 8     // k * max(ry, rx) <= JAC_HALO_MAX: the LDS region is at most (64 + 16)^2 floats per buffer (BC adjoint: up to 2r - 1 more per axis)
#define JAC_THREADS 512

namespace {

// one weighted-Jacobi sweep of the 3x3 second-order Laplacian (layers/JacobiIterationLayer.py:43-54)
__global__ void jacobi_kernel(int N, int H, int W, const float* __restrict__ u, const float* __restrict__ rhs, const float* __restrict__ dx,
                              float* __restrict__ out) {
  const int64_t total = (int64_t)N * H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xx = i % W; const int yy = (i / W) % H; const int n = i / ((int64_t)H * W);
    if (yy == 0 || yy == H - 1 || xx == 0 || xx == W - 1) { out[i] = u[i]; continue; }
    const float ay = 1.0f / (dx[2 * n] * dx[2 * n]), ax = 1.0f / (dx[2 * n + 1] * dx[2 * n + 1]);
    const float cr = ay * (u[i - W] + u[i + W]) + ax * (u[i - 1] + u[i + 1]);
    const float dinv = 1.0f / (-2.0f * ay - 2.0f * ax);
    out[i] = dinv * (rhs[i] - cr);
  }
}

// adjoint of the sweep w.r.t. u
__global__ void jacobi_bwd_kernel(int N, int H, int W, const float* __restrict__ dout, const float* __restrict__ dx, float* __restrict__ du) {
  const int64_t total = (int64_t)N * H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xx = i % W; const int yy = (i / W) % H; const int n = i / ((int64_t)H * W);
    const float ay = 1.0f / (dx[2 * n] * dx[2 * n]), ax = 1.0f / (dx[2 * n + 1] * dx[2 * n + 1]);
    const float dinv = 1.0f / (-2.0f * ay - 2.0f * ax);
    auto interior = [&](int y, int x) { return y > 0 && y < H - 1 && x > 0 && x < W - 1; };
    float v = interior(yy, xx) ? 0.f : dout[i];
    if (yy - 1 >= 0 && interior(yy - 1, xx)) v -= dinv * ay * dout[i - W];
    if (yy + 1 < H && interior(yy + 1, xx)) v -= dinv * ay * dout[i + W];
    if (xx - 1 >= 0 && interior(yy, xx - 1)) v -= dinv * ax * dout[i - 1];
    if (xx + 1 < W && interior(yy, xx + 1)) v -= dinv * ax * dout[i + 1];
    du[i] = v;
  }
}

// One axis of the boundary-aware regions.  [t0, t1) is the tile, L the image extent, r the radius, lo / hi whether the low / high edge is Neumann.
// Forward: d = D_s, what sweep s has to deliver (D_k the tile, D_0 what is loaded); c = C_s, what sweep s computes: D_s and the mirror sources of
// its band points.  D_(s-1) is C_s grown by r.   Adjoint: d = D_s, what sweep s delivers; c = G_s, where R^T of its input is needed: D_s grown by
// r; D_(s-1) is G_s and the band points that mirror into it.  Everything is clipped to the image.  Called with s == 0 for the loaded region (c unused).
template <bool BWD>
__host__ __device__ __forceinline__ void jac_range(int t0, int t1, int L, int r, int k, int s, bool lo, bool hi, int& d0, int& d1, int& c0, int& c1) {
  d0 = t0; d1 = t1;
  for (int j = k;; --j) {
    if (!BWD) {
      c0 = d0; c1 = d1;
      if (lo && d0 < r && 2 * r - d0 > c1) c1 = 2 * r - d0;                      // sources 2r-1-y of the band points y in [d0, r)
      if (hi && d1 > L - r && 2 * (L - r) - d1 < c0) c0 = 2 * (L - r) - d1;      // sources 2(L-r)-1-y of y in [L-r, d1)
    } else {
      c0 = d0 - r < 0 ? 0 : d0 - r; c1 = d1 + r > L ? L : d1 + r;
    }
    if (j <= s) return;
    if (!BWD) {
      d0 = c0 - r < 0 ? 0 : c0 - r; d1 = c1 + r > L ? L : c1 + r;
    } else {
      d0 = c0; d1 = c1;
      if (lo && c0 < 2 * r && c1 > r) { const int e = c1 < 2 * r ? 2 * r - c1 : 0; if (e < d0) d0 = e; }             // band points 2r-1-y of y in [r, 2r)
      if (hi && c1 > L - 2 * r && c0 < L - r) { const int e = 2 * (L - r) - (c0 > L - 2 * r ? c0 : L - 2 * r); if (e > d1) d1 = e; }
    }
  }
}

// R_m at (y, x): false where the point keeps its own value (no band, or a band on a Dirichlet edge), else (my, mx) is the interior point it mirrors.
template <int RY, int RX>
__device__ __forceinline__ bool jac_refreshed(int y, int x, int H, int W, int mask, int& my, int& mx) {
  bool any = false, frozen = false;
  my = y; mx = x;
  if (y < RY) { any = true; if (mask & 1) my = 2 * RY - 1 - y; else frozen = true; }
  else if (y >= H - RY) { any = true; if (mask & 2) my = 2 * (H - RY) - 1 - y; else frozen = true; }
  if (x < RX) { any = true; if (mask & 4) mx = 2 * RX - 1 - x; else frozen = true; }
  else if (x >= W - RX) { any = true; if (mask & 8) mx = 2 * (W - RX) - 1 - x; else frozen = true; }
  return any && !frozen;
}

// BWD == false: u -> k sweeps -> out.   BWD == true: u is d(out), out is d(guess), rhs unused.
// BC == false: mask and S_bc are not read.   BC == true: S_bc is the floats per LDS buffer as the host sized them from jac_range.
template <int RY, int RX, bool BWD, bool BC>
__global__ __launch_bounds__(JAC_THREADS) void jacobi_fused_kernel(int H, int W, int k, const float* __restrict__ coef, const float* __restrict__ u,
                                                                   const float* __restrict__ rhs, float* __restrict__ out, int mask, int S_bc) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int SY = 2 * RY + 1, SX = 2 * RX + 1;
  const int n = blockIdx.z, tid = threadIdx.x;
  pcnn_frame<JAC_TILE> f(H, W);
  const int ty0 = f.ty0, ty1 = f.ty1, tx0 = f.tx0, tx1 = f.tx1;
  // the region held in LDS: the tile grown by k radii, clipped to the image (BC: D_0 of jac_range)
  int ly0, ly1, lx0, lx1;
  f.grow(k * RY, k * RX, ly0, ly1, lx0, lx1);
  int S = (JAC_TILE + 2 * k * RY) * (JAC_TILE + 2 * k * RX);         // floats per buffer as the host sized them
  if (BC) {
    int c0, c1;
    jac_range<BWD>(ty0, ty1, H, RY, k, 0, mask & 1, mask & 2, ly0, ly1, c0, c1);
    jac_range<BWD>(tx0, tx1, W, RX, k, 0, mask & 4, mask & 8, lx0, lx1, c0, c1);
    S = S_bc;
  }
  f.hold(ly0, ly1, lx0, lx1);
  const int LW = f.LW;
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
  pcnn_for_points<JAC_THREADS>(tid, ly0, lx0, ly1 - ly0, LW, [&](int y, int x) { src[f.at(y, x)] = u[img + (int64_t)y * W + x]; });
  if (!BWD) {
    int ry0, ry1, rx0, rx1;
    f.grow((k - 1) * RY, (k - 1) * RX, ry0, ry1, rx0, rx1);
    if (BC) {                                                         // the first sweep's computed region C_1; every later one lies inside it
      int d0, d1;
      jac_range<false>(ty0, ty1, H, RY, k, 1, mask & 1, mask & 2, d0, d1, ry0, ry1);
      jac_range<false>(tx0, tx1, W, RX, k, 1, mask & 4, mask & 8, d0, d1, rx0, rx1);
    }
    pcnn_for_points<JAC_THREADS>(tid, ry0, rx0, ry1 - ry0, rx1 - rx0, [&](int y, int x) { rb[f.at(y, x)] = rhs[img + (int64_t)y * W + x]; });
  }
  __syncthreads();

  // J (or J^T) at one point, read from `in`
  auto point = [&](const float* in, int c, int y, int x) -> float {
    const bool in_x = x >= RX && x < W - RX, in_y = y >= RY && y < H - RY;
    float v;
    if (!BWD) {
      if (in_x && in_y) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < SY; ++i)
          if (i != RY) acc = fmaf(cy[i], in[c + (i - RY) * LW], acc);
#pragma unroll
        for (int j = 0; j < SX; ++j)
          if (j != RX) acc = fmaf(cx[j], in[c + (j - RX)], acc);
        v = dinv * (rb[c] - acc);
      } else {
        v = in[c];
      }
    } else {
      // adjoint: gather from the interior points q = p - t whose stencil reached p with tap t
      float acc = 0.f;
      if (in_x) {
#pragma unroll
        for (int i = 0; i < SY; ++i) {
          const int qy = y - (i - RY);
          if (i != RY && qy >= RY && qy < H - RY) acc = fmaf(cy[i], in[c - (i - RY) * LW], acc);
        }
      }
      if (in_y) {
#pragma unroll
        for (int j = 0; j < SX; ++j) {
          const int qx = x - (j - RX);
          if (j != RX && qx >= RX && qx < W - RX) acc = fmaf(cx[j], in[c - (j - RX)], acc);
        }
      }
      v = ((in_x && in_y) ? 0.f : in[c]) - dinv * acc;
    }
    return v;
  };

  for (int s = 1; s <= k; ++s) {
    const int g = k - s;                                              // radii this sweep's region still extends past the tile
    int y0, y1, x0, x1;
    f.grow(g * RY, g * RX, y0, y1, x0, x1);
    if (BC) {
      int cy0, cy1, cx0, cx1;                                         // forward: C_s; adjoint: G_s
      jac_range<BWD>(ty0, ty1, H, RY, k, s, mask & 1, mask & 2, y0, y1, cy0, cy1);
      jac_range<BWD>(tx0, tx1, W, RX, k, s, mask & 4, mask & 8, x0, x1, cx0, cx1);
      if (!BWD) {
        // does what this sweep delivers meet a Neumann band?  (the same for every thread of the workgroup)
        const bool touch = ((mask & 1) && y0 < RY) || ((mask & 2) && y1 > H - RY) || ((mask & 4) && x0 < RX) || ((mask & 8) && x1 > W - RX);
        if (touch) {
          pcnn_for_points<JAC_THREADS>(tid, cy0, cx0, cy1 - cy0, cx1 - cx0, [&](int y, int x) {
            const int c = (y - ly0) * LW + (x - lx0);
            dst[c] = point(src, c, y, x);
          });
          __syncthreads();                                            // the refresh reads this sweep's J(u) as other threads wrote it
          pcnn_for_points<JAC_THREADS>(tid, y0, x0, y1 - y0, x1 - x0, [&](int y, int x) {
            const int c = (y - ly0) * LW + (x - lx0);
            int my, mx;
            const bool r = jac_refreshed<RY, RX>(y, x, H, W, mask, my, mx);   // sources are interior points: no refresh writes what another reads
            const int m = (my - ly0) * LW + (mx - lx0);
            if (s == k) out[img + (int64_t)y * W + x] = dst[r ? m : c];
            else if (r) dst[c] = dst[m];
          });
          __syncthreads();
          float* t = src; src = dst; dst = t;
          continue;
        }
      } else {
        // does R_m^T act on the region its output is gathered from?
        const bool touch = ((mask & 1) && cy0 < 2 * RY) || ((mask & 2) && cy1 > H - 2 * RY) || ((mask & 4) && cx0 < 2 * RX) || ((mask & 8) && cx1 > W - 2 * RX);
        if (touch) {
          // R_m^T as a gather: a point that kept its own value passes its gradient on, and an interior point collects those of the band points
          // that mirrored it - along y, along x, and across a Neumann/Neumann corner - in this fixed order
          pcnn_for_points<JAC_THREADS>(tid, cy0, cx0, cy1 - cy0, cx1 - cx0, [&](int y, int x) {
            const int c = (y - ly0) * LW + (x - lx0);
            int my, mx;
            float v = jac_refreshed<RY, RX>(y, x, H, W, mask, my, mx) ? 0.f : src[c];
            const bool in_x = x >= RX && x < W - RX, in_y = y >= RY && y < H - RY;
            const bool yl = (mask & 1) && y >= RY && y < 2 * RY, yh = (mask & 2) && y >= H - 2 * RY && y < H - RY;
            const bool xl = (mask & 4) && x >= RX && x < 2 * RX, xh = (mask & 8) && x >= W - 2 * RX && x < W - RX;
            const int oyl = (2 * RY - 1 - 2 * y) * LW, oyh = (2 * (H - RY) - 1 - 2 * y) * LW;
            const int oxl = 2 * RX - 1 - 2 * x, oxh = 2 * (W - RX) - 1 - 2 * x;
            if (in_x && yl) v += src[c + oyl];
            if (in_x && yh) v += src[c + oyh];
            if (in_y && xl) v += src[c + oxl];
            if (in_y && xh) v += src[c + oxh];
            if (yl && xl) v += src[c + oyl + oxl];
            if (yl && xh) v += src[c + oyl + oxh];
            if (yh && xl) v += src[c + oyh + oxl];
            if (yh && xh) v += src[c + oyh + oxh];
            dst[c] = v;
          });
          __syncthreads();
          pcnn_for_points<JAC_THREADS>(tid, y0, x0, y1 - y0, x1 - x0, [&](int y, int x) {
            const int c = (y - ly0) * LW + (x - lx0);
            const float v = point(dst, c, y, x);
            if (s == k) out[img + (int64_t)y * W + x] = v;
            else src[c] = v;                                          // all of src was read before the barrier: the result returns to it, no exchange
          });
          __syncthreads();
          continue;
        }
      }
    }
    pcnn_for_points<JAC_THREADS>(tid, y0, x0, y1 - y0, x1 - x0, [&](int y, int x) {
      const int c = f.at(y, x);
      const float v = point(src, c, y, x);
      if (s == k) out[img + (int64_t)y * W + x] = v;                 // the last sweep's region is the tile itself
      else dst[c] = v;
    });
    __syncthreads();
    float* t = src; src = dst; dst = t;
  }
}

// mask < 0: the frozen-band kernels.  mask >= 0: the boundary-aware ones (with mask 0 they compute the same bits - no sweep ever refreshes - but the
// entry points send mask 0 to the frozen-band kernels, which are faster).
template <bool BWD>
int jacobi_launch(pcnn_handle_s* h, int N, int H, int W, int sy, int sx, int k, const float* coef, const float* u, const float* rhs, float* out, int mask) {
  const int ry = sy / 2, rx = sx / 2;
  const dim3 grid((unsigned)pcnn_cdiv(W, JAC_TILE), (unsigned)pcnn_cdiv(H, JAC_TILE), (unsigned)N);
  size_t per = (size_t)(JAC_TILE + 2 * k * ry) * (JAC_TILE + 2 * k * rx);
  if (mask >= 0) {
    // the largest loaded region over the tiles of each axis, from the recurrence the kernel itself evaluates
    int mh = 0, mw = 0, d0, d1, c0, c1;
    for (int t = 0; t < H; t += JAC_TILE) {
      jac_range<BWD>(t, t + JAC_TILE < H ? t + JAC_TILE : H, H, ry, k, 0, mask & 1, mask & 2, d0, d1, c0, c1);
      mh = d1 - d0 > mh ? d1 - d0 : mh;
    }
    for (int t = 0; t < W; t += JAC_TILE) {
      jac_range<BWD>(t, t + JAC_TILE < W ? t + JAC_TILE : W, W, rx, k, 0, mask & 4, mask & 8, d0, d1, c0, c1);
      mw = d1 - d0 > mw ? d1 - d0 : mw;
    }
    per = (size_t)mh * mw;
  }
  const size_t lds = (size_t)(BWD ? 2 : 3) * per * sizeof(float);
  PCNN_REQUIRE_LDS(h, lds, "pcnn_jacobi_fused: %zu bytes of LDS for %d fused sweeps of a %d x %d stencil", lds, k, sy, sx);
  auto go = [&](auto kernel) { pcnn_launch_lds(h, kernel, grid, JAC_THREADS, lds, H, W, k, coef, u, rhs, out, mask, (int)per); };
#define JAC_CASE(A, B)                                        \
  case A * 8 + B:                                             \
    if (mask >= 0) go(jacobi_fused_kernel<A, B, BWD, true>);  \
    else go(jacobi_fused_kernel<A, B, BWD, false>);           \
    break;
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

bool jacobi_shape_ok(int N, int H, int W, int sy, int sx, int n_sweeps) {
  return pcnn_grid_ok(N, H, W) && sy % 2 == 1 && sx % 2 == 1 && sy >= 3 && sy <= 9 && sx >= 3 && sx <= 9 && H > 2 * (sy / 2) && W > 2 * (sx / 2) && n_sweeps >= 1;
}

// a Neumann edge's mirror sources must be interior points: three radii along every axis the mask touches
bool jacobi_mask_ok(int H, int W, int sy, int sx, int mask) {
  return mask >= 0 && mask < 16 && (!(mask & 3) || H >= 3 * (sy / 2)) && (!(mask & 12) || W >= 3 * (sx / 2));
}

// The checks and the launch chain of the four fused entry points.  bc: the entry point takes a neumann_mask.
template <bool BWD>
int jacobi_run(pcnn_handle_s* h, const char* name, int N, int H, int W, int sy, int sx, const float* coef, const float* u, const float* rhs, int n_sweeps,
               float* out, bool bc = false, int mask = 0) {
  PCNN_REQUIRE(h, h && coef && u && (BWD || rhs) && out, "%s: null argument", name);
  PCNN_REQUIRE(h, jacobi_shape_ok(N, H, W, sy, sx, n_sweeps),
               "%s: needs odd stencil sizes in 3..9, H > 2*(sy/2), W > 2*(sx/2), n_sweeps >= 1 (got %d x %d stencil, %d x %d image, %d sweeps)", name, sy, sx, H, W,
               n_sweeps);
  PCNN_REQUIRE(h, !bc || jacobi_mask_ok(H, W, sy, sx, mask),
               "%s: needs neumann_mask in 0..15, H >= 3*(sy/2) with a left or right Neumann edge, W >= 3*(sx/2) with a bottom or top one (got mask %d, "
               "%d x %d stencil, %d x %d image)", name, mask, sy, sx, H, W);
  if (BWD) PCNN_REQUIRE(h, out != u, "%s: du must not alias dout", name);
  else PCNN_REQUIRE(h, out != u && out != rhs, "%s: out must not alias u or rhs", name);
  // mask 0 runs the frozen-band kernels: the same bits, and measurably faster than the boundary-aware ones with nothing to refresh
  const int m = bc && mask ? mask : -1;
  return pcnn_sweep_chain(h, name, N, H, W, n_sweeps, pcnn_jacobi_fused_max_sweeps(sy, sx), u, out,
                          [&](int k, const float* in, float* to) { return jacobi_launch<BWD>(h, N, H, W, sy, sx, k, coef, in, rhs, to, m); });
}

}  // namespace

extern "C" int pcnn_jacobi_fused_tile(void) { return JAC_TILE; }

extern "C" int pcnn_jacobi_fused_max_sweeps(int sy, int sx) {
  const int r = (sy > sx ? sy : sx) / 2;
  return r < 1 ? 0 : (JAC_HALO_MAX / r < 1 ? 1 : JAC_HALO_MAX / r);
}

extern "C" int pcnn_jacobi_fused_fwd(pcnn_handle h, int N, int H, int W, int sy, int sx, const float* coef, const float* u, const float* rhs, int n_sweeps,
                                     float* out) {
  return jacobi_run<false>(h, "pcnn_jacobi_fused_fwd", N, H, W, sy, sx, coef, u, rhs, n_sweeps, out);
}

extern "C" int pcnn_jacobi_fused_bwd(pcnn_handle h, int N, int H, int W, int sy, int sx, const float* coef, const float* dout, int n_sweeps, float* du) {
  return jacobi_run<true>(h, "pcnn_jacobi_fused_bwd", N, H, W, sy, sx, coef, dout, nullptr, n_sweeps, du);
}

extern "C" int pcnn_jacobi_fused_bc_fwd(pcnn_handle h, int N, int H, int W, int sy, int sx, const float* coef, const float* u, const float* rhs, int n_sweeps,
                                        int neumann_mask, float* out) {
  return jacobi_run<false>(h, "pcnn_jacobi_fused_bc_fwd", N, H, W, sy, sx, coef, u, rhs, n_sweeps, out, true, neumann_mask);
}

extern "C" int pcnn_jacobi_fused_bc_bwd(pcnn_handle h, int N, int H, int W, int sy, int sx, const float* coef, const float* dout, int n_sweeps, int neumann_mask,
                                        float* du) {
  return jacobi_run<true>(h, "pcnn_jacobi_fused_bc_bwd", N, H, W, sy, sx, coef, dout, nullptr, n_sweeps, du, true, neumann_mask);
}

extern "C" int pcnn_jacobi_sweep(pcnn_handle h, int N, int H, int W, const float* u, const float* rhs, const float* dx, float* out) {
  PCNN_REQUIRE(h, h && u && rhs && dx && out && u != out, "pcnn_jacobi_sweep: bad argument");
  hipLaunchKernelGGL(jacobi_kernel, pcnn_grid1d((int64_t)N * H * W, 256, 8192), dim3(256), 0, h->stream, N, H, W, u, rhs, dx, out);
  PCNN_CHECK_LAUNCH(h, "pcnn_jacobi_sweep");
  return 0;
}

extern "C" int pcnn_jacobi_sweep_bwd(pcnn_handle h, int N, int H, int W, const float* dout, const float* dx, float* du) {
  PCNN_REQUIRE(h, h && dout && dx && du && dout != du, "pcnn_jacobi_sweep_bwd: bad argument");
  hipLaunchKernelGGL(jacobi_bwd_kernel, pcnn_grid1d((int64_t)N * H * W, 256, 8192), dim3(256), 0, h->stream, N, H, W, dout, dx, du);
  PCNN_CHECK_LAUNCH(h, "pcnn_jacobi_sweep_bwd");
  return 0;
}
