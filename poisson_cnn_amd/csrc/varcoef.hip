// Variable-density Poisson problem div((1/rho) grad u) = f on the dataset's vertex-centred grid (one spacing per sample, dy = dx), Dirichlet data on
// the four edges: the flux-form operator, and a conjugate-gradient solve preconditioned by the constant-coefficient DST solve.
//   beta_{i+1/2,j} = 2 / (rho[i,j] + rho[i+1,j])                                  (the first matrix of dataset/generators/variable_density)
//   (A u)[i,j] = ( beta_{i+1/2,j} (u[i,j] - u[i+1,j]) + beta_{i-1/2,j} (u[i,j] - u[i-1,j])
//                + beta_{i,j+1/2} (u[i,j] - u[i,j+1]) + beta_{i,j-1/2} (u[i,j] - u[i,j-1]) ) / dx^2       on the (H-2) x (W-2) interior nodes,
//   A u = b,  b = -f + (Dirichlet neighbours' values, each times its face coefficient / dx^2):  A is symmetric positive definite.
// Everything is fp64; rho, f, the boundary arrays and dx are read as fp32 and converted.  No atomics: every dot product is a per-block partial sum
// (fixed tree) reduced per sample by a second one-block stage in a fixed order, so results do not depend on the batch a sample is solved in.
// The face coefficients are built on the fly from an LDS tile of rho with a one-point halo: 20 B per point and product (p 8, rho 4, q 8) against
// 32 B with two fp64 face arrays built once per solve (p 8, faces 16, q 8).
// The face coefficient, the 16 x 64 tile and the LDS node loader are flux_form.h's, shared with varcoef_train.hip and error_stats.hip; the fp64
// operator sum (stencil_at) is this file's alone: its order ((a + b) + c) + d of pc - neighbour is not the fp32 residual's.
#include <math.h>
#include <type_traits>
#include "flux_form.h"

namespace {

constexpr int VT_LR = FLUX_ROWS + 2, VT_LC = FLUX_COLS + 2;                                               // the tile of interior points with its halo
constexpr int EW_THREADS = 256, EW_POINTS = 2048, EW_MAX_BLOCKS = 1024;                                   // element-wise kernels: blocks per SAMPLE
// per-sample scalars (doubles) of the solve
enum { VS_BB = 0, VS_RR = 1, VS_PQ = 2, VS_RZ0 = 3, VS_RZ1 = 4, VS_RHOMIN = 5, VS_STRIDE = 8 };

static inline int vc_tiles(int H, int W) { return pcnn_cdiv(H - 2, FLUX_ROWS) * pcnn_cdiv(W - 2, FLUX_COLS); }
static inline int vc_ew_blocks(int64_t per) {
  const int64_t b = pcnn_cdiv64(per, EW_POINTS);
  return (int)(b < 1 ? 1 : (b > EW_MAX_BLOCKS ? EW_MAX_BLOCKS : b));
}
static inline int vc_cap(int H, int W) {
  const int t = vc_tiles(H, W), e = vc_ew_blocks((int64_t)(H - 2) * (W - 2));
  return t > e ? t : e;
}
// workspace: x, r, p, q, z (N x (H-2) x (W-2) doubles each; q and z double as the two GEMM intermediates) and three partial-sum arrays of N x cap
struct VcWs { double *x, *r, *p, *q, *z, *part; int cap; };
static inline size_t vc_bytes(int N, int H, int W) { return (5 * (size_t)N * (H - 2) * (W - 2) + 3 * (size_t)N * vc_cap(H, W)) * sizeof(double); }
static inline VcWs vc_layout(void* ws, int N, int H, int W) {
  VcWs l;
  const size_t v = (size_t)N * (H - 2) * (W - 2);
  l.cap = vc_cap(H, W);
  l.x = static_cast<double*>(ws); l.r = l.x + v; l.p = l.r + v; l.q = l.p + v; l.z = l.q + v; l.part = l.z + v;
  return l;
}

// sum over the block's threads by the fixed tree of pcnn_block_reduce; every thread gets the total
template <int T>
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  pcnn_block_sum<double, T>(red, t);
  return red[0];
}

// rho on nodes (I0 .. I0+17) x (J0 .. J0+65): the tile's nodes I0+1.., J0+1.. and their halo.  Nodes beyond the grid read 1 (never used by a stored point).
__device__ __forceinline__ float load_rho_tile(float (*rs)[VT_LC], const float* __restrict__ rho_n, int H, int W, int I0, int J0) {
  float mn = INFINITY;
  for (int e = threadIdx.x; e < VT_LR * VT_LC; e += FLUX_THREADS) {
    const int r = e / VT_LC, c = e % VT_LC, i = I0 + r, j = J0 + c;
    float v = 1.f;
    if (i < H && j < W) {
      v = rho_n[(int64_t)i * W + j];
      mn = fminf(mn, v == v ? v : -INFINITY);      // fminf drops a NaN: it counts as -inf, so the rho > 0 refusal sees it
    }
    rs[r][c] = v;
  }
  return mn;
}

struct Faces { double lo_i, hi_i, lo_j, hi_j; };
// face coefficients of the interior point at tile offset (r, c): towards row i-1, i+1, column j-1, j+1
__device__ __forceinline__ Faces faces_at(const float (*rs)[VT_LC], int r, int c) {
  const double rc = (double)rs[r + 1][c + 1];
  Faces f;
  f.lo_i = pcnn_beta_face(rc, (double)rs[r][c + 1]);
  f.hi_i = pcnn_beta_face(rc, (double)rs[r + 2][c + 1]);
  f.lo_j = pcnn_beta_face(rc, (double)rs[r + 1][c]);
  f.hi_j = pcnn_beta_face(rc, (double)rs[r + 1][c + 2]);
  return f;
}
__device__ __forceinline__ double stencil_at(const Faces& f, const double (*ps)[VT_LC], int r, int c, double inv_h2) {
  const double pc = ps[r + 1][c + 1];
  return (f.lo_i * (pc - ps[r][c + 1]) + f.hi_i * (pc - ps[r + 2][c + 1]) + f.lo_j * (pc - ps[r + 1][c]) + f.hi_j * (pc - ps[r + 1][c + 2])) * inv_h2;
}

// q = A p and the tile's share of p.q.  grid (column tiles, row tiles, N); part[n][tile]
__global__ __launch_bounds__(FLUX_THREADS) void varcoef_apply_kernel(int H, int W, int cap, const float* __restrict__ rho, const float* __restrict__ dx,
                                                                     const double* __restrict__ p, double* __restrict__ q, double* __restrict__ part) {
  __shared__ float rs[VT_LR][VT_LC];
  __shared__ double ps[VT_LR][VT_LC];
  __shared__ double red[FLUX_THREADS];
  const int nh = H - 2, nw = W - 2, n = blockIdx.z, I0 = blockIdx.y * FLUX_ROWS, J0 = blockIdx.x * FLUX_COLS;
  const int64_t per = (int64_t)nh * nw;
  const double* pn = p + (int64_t)n * per;
  load_rho_tile(rs, rho + (int64_t)n * H * W, H, W, I0, J0);
  pcnn_load_nodes<VT_LR, VT_LC>(ps, pn, nh, nw, I0 - 1, J0 - 1, 0.0);               // interior indices; zero Dirichlet data outside
  __syncthreads();
  const double h = (double)dx[n], inv_h2 = 1.0 / (h * h);
  const int c = threadIdx.x % FLUX_COLS, r0 = (threadIdx.x / FLUX_COLS) * FLUX_RPT;
  double s = 0.0;
  if (J0 + c < nw) {
#pragma unroll
    for (int k = 0; k < FLUX_RPT; ++k) {
      const int r = r0 + k;
      if (I0 + r < nh) {
        const double v = stencil_at(faces_at(rs, r, c), ps, r, c, inv_h2);
        q[(int64_t)n * per + (int64_t)(I0 + r) * nw + J0 + c] = v;
        s += ps[r + 1][c + 1] * v;
      }
    }
  }
  const double tot = block_sum<FLUX_THREADS>(s, red);
  if (threadIdx.x == 0) part[(int64_t)n * cap + blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// Start of a solve: b from f, rho, the four boundary arrays and dx; x = x0 (interior of the optional initial guess, else 0); r = b - A x0; the tile's
// shares of b.b and r.r and its minimum of rho.  left/right (N,W): values on rows 0 / H-1; bottom/top (N,H): values on columns 0 / W-1.
__global__ __launch_bounds__(FLUX_THREADS) void varcoef_setup_kernel(int H, int W, int cap, int N, const float* __restrict__ rho, const float* __restrict__ f,
                                                                     const float* __restrict__ left, const float* __restrict__ right,
                                                                     const float* __restrict__ bottom, const float* __restrict__ top,
                                                                     const float* __restrict__ dx, const double* __restrict__ x0, double* __restrict__ x,
                                                                     double* __restrict__ rr_out, double* __restrict__ part) {
  __shared__ float rs[VT_LR][VT_LC];
  __shared__ double ps[VT_LR][VT_LC];
  __shared__ double red[FLUX_THREADS];
  const int nh = H - 2, nw = W - 2, n = blockIdx.z, I0 = blockIdx.y * FLUX_ROWS, J0 = blockIdx.x * FLUX_COLS;
  const int64_t per = (int64_t)nh * nw;
  const float mn = load_rho_tile(rs, rho + (int64_t)n * H * W, H, W, I0, J0);
  for (int e = threadIdx.x; e < VT_LR * VT_LC; e += FLUX_THREADS) {
    const int r = e / VT_LC, c = e % VT_LC, ii = I0 + r - 1, jj = J0 + c - 1;
    ps[r][c] = (x0 && ii >= 0 && ii < nh && jj >= 0 && jj < nw) ? x0[((int64_t)n * H + ii + 1) * W + jj + 1] : 0.0;
  }
  __syncthreads();
  const double h = (double)dx[n], inv_h2 = 1.0 / (h * h);
  const int c = threadIdx.x % FLUX_COLS, r0 = (threadIdx.x / FLUX_COLS) * FLUX_RPT;
  double sbb = 0.0, srr = 0.0;
  if (J0 + c < nw) {
#pragma unroll
    for (int k = 0; k < FLUX_RPT; ++k) {
      const int r = r0 + k, ii = I0 + r, jj = J0 + c;
      if (ii < nh) {
        const Faces fc = faces_at(rs, r, c);
        double b = -(double)f[((int64_t)n * H + ii + 1) * W + jj + 1];
        if (ii == 0) b += fc.lo_i * inv_h2 * (double)left[(int64_t)n * W + jj + 1];
        if (ii == nh - 1) b += fc.hi_i * inv_h2 * (double)right[(int64_t)n * W + jj + 1];
        if (jj == 0) b += fc.lo_j * inv_h2 * (double)bottom[(int64_t)n * H + ii + 1];
        if (jj == nw - 1) b += fc.hi_j * inv_h2 * (double)top[(int64_t)n * H + ii + 1];
        const double res = b - stencil_at(fc, ps, r, c, inv_h2);
        const int64_t o = (int64_t)n * per + (int64_t)ii * nw + jj;
        x[o] = ps[r + 1][c + 1];
        rr_out[o] = res;
        sbb += b * b;
        srr += res * res;
      }
    }
  }
  const int tile = blockIdx.y * gridDim.x + blockIdx.x;
  const double tbb = block_sum<FLUX_THREADS>(sbb, red);
  const double trr = block_sum<FLUX_THREADS>(srr, red);
  __syncthreads();
  red[threadIdx.x] = (double)mn;
  __syncthreads();
  pcnn_block_reduce<double, FLUX_THREADS>(red, threadIdx.x, pcnn_min_op());
  if (threadIdx.x == 0) {
    part[(int64_t)n * cap + tile] = tbb;
    part[((int64_t)N + n) * cap + tile] = trr;
    part[((int64_t)2 * N + n) * cap + tile] = red[0];
  }
}

// second stage of every reduction: one block per sample adds (OP 0) or takes the minimum (OP 1) of its `count` partials in a fixed order and stores
// the result with an ordinary store by one lane.  check: the result is r.r - raise the sample's flag when ||r|| <= tol ||b||.
template <int OP>
__global__ __launch_bounds__(EW_THREADS) void varcoef_reduce_kernel(int count, int cap, const double* __restrict__ part, double* __restrict__ out,
                                                                    int stride, int slot, int check, double tol2, int* __restrict__ flags) {
  __shared__ double red[EW_THREADS];
  const std::conditional_t<OP != 0, pcnn_min_op, pcnn_sum_op> op{};
  const int n = blockIdx.x, t = threadIdx.x;
  double v = OP ? (double)INFINITY : 0.0;
  for (int k = t; k < count; k += EW_THREADS) v = op(v, part[(int64_t)n * cap + k]);
  red[t] = v;
  __syncthreads();
  pcnn_block_reduce<double, EW_THREADS>(red, t, op);
  if (t == 0) {
    out[(int64_t)n * stride + slot] = red[0];
    if (check && red[0] <= tol2 * out[(int64_t)n * stride + VS_BB]) flags[n] = 1;
  }
}

// x += alpha p, r -= alpha q with alpha = (r.z) / (p.q) from the sample's scalars; the block's share of the new r.r.  alpha = 0 for a flagged
// sample: x and r are then neither changed nor written and p and q are not read, so nothing they hold can reach x.  grid (blocks per sample, N)
__global__ __launch_bounds__(EW_THREADS) void varcoef_update_xr_kernel(int64_t per, int cap, int cur, const double* __restrict__ scal, const int* __restrict__ flags,
                                                                       const double* __restrict__ p, const double* __restrict__ q, double* __restrict__ x,
                                                                       double* __restrict__ r, double* __restrict__ part) {
  __shared__ double red[EW_THREADS];
  const int n = blockIdx.y;
  const double pq = scal[n * VS_STRIDE + VS_PQ], rz = scal[n * VS_STRIDE + VS_RZ0 + cur];
  const double alpha = (flags[n] || !(pq > 0.0)) ? 0.0 : rz / pq;
  const int64_t base = (int64_t)n * per;
  double s = 0.0;
  for (int64_t k = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; k < per; k += (int64_t)gridDim.x * EW_THREADS) {
    double rn = r[base + k];
    if (alpha != 0.0) {                            // uniform over the block
      x[base + k] += alpha * p[base + k];
      rn -= alpha * q[base + k];
      r[base + k] = rn;
    }
    s += rn * rn;
  }
  const double tot = block_sum<EW_THREADS>(s, red);
  if (threadIdx.x == 0) part[(int64_t)n * cap + blockIdx.x] = tot;
}

// the eigenvalue division of the preconditioner, in place on the coefficients c = S_h r S_w: c / (lam_h + lam_w).  S is orthonormal and symmetric,
// so r.z = sum c^2 / (lam_h + lam_w): the block's share of r.z comes from this pass and needs no further read of r and z.
__global__ __launch_bounds__(EW_THREADS) void varcoef_divide_kernel(int nh, int nw, int cap, const double* __restrict__ lam_h, const double* __restrict__ lam_w,
                                                                    double* __restrict__ T, double* __restrict__ part) {
  __shared__ double red[EW_THREADS];
  const int n = blockIdx.y;
  double* Tn = T + (int64_t)n * nh * nw;
  double s = 0.0;
  for (int i = blockIdx.x; i < nh; i += gridDim.x) {           // a block takes whole rows: no index division per point
    const double li = lam_h[i];
    double* row = Tn + (int64_t)i * nw;
    for (int j = threadIdx.x; j < nw; j += EW_THREADS) {
      const double c = row[j], z = c / (li + lam_w[j]);
      row[j] = z;
      s += c * z;
    }
  }
  const double tot = block_sum<EW_THREADS>(s, red);
  if (threadIdx.x == 0) part[(int64_t)n * cap + blockIdx.x] = tot;
}

// p = z + beta p, beta = (r.z)_new / (r.z)_old from the sample's scalars; 0 for a flagged sample and for the first direction (first = 1).
// With beta = 0 the old p is not read: before the first direction it is memory nobody has written, and 0 * NaN is NaN.
__global__ __launch_bounds__(EW_THREADS) void varcoef_update_p_kernel(int64_t per, int cur, int first, const double* __restrict__ scal, const int* __restrict__ flags,
                                                                      const double* __restrict__ z, double* __restrict__ p) {
  const int n = blockIdx.y;
  const double rz_old = scal[n * VS_STRIDE + VS_RZ0 + cur], rz_new = scal[n * VS_STRIDE + VS_RZ0 + (cur ^ 1)];
  const double beta = (first || flags[n] || !(rz_old > 0.0)) ? 0.0 : rz_new / rz_old;
  const int64_t base = (int64_t)n * per;
  for (int64_t k = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; k < per; k += (int64_t)gridDim.x * EW_THREADS)
    p[base + k] = beta != 0.0 ? z[base + k] + beta * p[base + k] : z[base + k];
}

// g -> lo + (hi - lo) |g|: a density field from a smooth function already scaled to max|g| = 1
__global__ void varcoef_density_kernel(int64_t total, float lo, float hi, float* __restrict__ g) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) g[i] = lo + (hi - lo) * fminf(fabsf(g[i]), 1.f);
}

static int vc_check_shape(pcnn_handle h, const char* who, int N, int H, int W) {
  PCNN_REQUIRE(h, N >= 1 && N <= 65535, "%s: batch %d not in 1..65535", who, N);
  PCNN_REQUIRE(h, H >= 3 && W >= 3 && pcnn_cdiv(H - 2, FLUX_ROWS) <= 65535, "%s: grid %d x %d unsupported", who, H, W);
  return 0;
}
static dim3 vc_tile_grid(int N, int H, int W) { return dim3(pcnn_cdiv(W - 2, FLUX_COLS), pcnn_cdiv(H - 2, FLUX_ROWS), N); }

// z = M^-1 r, M the constant-coefficient 5-point operator with zero Dirichlet data (its 1/dx^2 left out: a positive factor of M does not change the
// iterates): z = S_h ((S_h r S_w) ./ (lam_h + lam_w)) S_w as four fp64 matrix-core products; q holds the half-transformed fields.  r.z -> scal slot.
static int vc_precondition(pcnn_handle h, int N, int H, int W, const VcWs& w, const double* S_h, const double* lam_h, const double* S_w, const double* lam_w,
                           double* scal, int slot) {
  const int nh = H - 2, nw = W - 2;
  const int64_t per = (int64_t)nh * nw;
  const int eb = vc_ew_blocks(per);
  if (int rc = pcnn_two_sided_gemm_f64(h, N, nh, nw, S_h, w.r, S_w, w.q, w.z)) return rc;
  hipLaunchKernelGGL(varcoef_divide_kernel, dim3(eb, N), dim3(EW_THREADS), 0, h->stream, nh, nw, w.cap, lam_h, lam_w, w.z, w.part);
  hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, eb, w.cap, w.part, scal, (int)VS_STRIDE, slot, 0, 0.0, (int*)nullptr);
  PCNN_CHECK_LAUNCH(h, "pcnn_varcoef_pcg(divide)");
  return pcnn_two_sided_gemm_f64(h, N, nh, nw, S_h, w.z, S_w, w.q, w.z);
}

}  // namespace

extern "C" int pcnn_varcoef_apply(pcnn_handle h, int N, int H, int W, const float* rho, const float* dx, const double* p, double* q, double* pq) {
  PCNN_REQUIRE(h, h && rho && dx && p && q && pq, "pcnn_varcoef_apply: null argument");
  if (int rc = vc_check_shape(h, "pcnn_varcoef_apply", N, H, W)) return rc;
  const int cap = vc_cap(H, W), tiles = vc_tiles(H, W);
  if (int rc = pcnn_reserve(h, h->aux_ws, (size_t)N * cap * sizeof(double), 0, "pcnn_varcoef_apply")) return rc;
  double* part = static_cast<double*>(h->aux_ws.p);
  hipLaunchKernelGGL(varcoef_apply_kernel, vc_tile_grid(N, H, W), dim3(FLUX_THREADS), 0, h->stream, H, W, cap, rho, dx, p, q, part);
  hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, tiles, cap, part, pq, 1, 0, 0, 0.0, (int*)nullptr);
  PCNN_CHECK_LAUNCH(h, "pcnn_varcoef_apply");
  return 0;
}

extern "C" size_t pcnn_varcoef_pcg_workspace(int N, int H, int W) {
  if (N < 1 || H < 3 || W < 3) return 0;
  return vc_bytes(N, H, W);
}

extern "C" int pcnn_varcoef_pcg_setup(pcnn_handle h, int N, int H, int W, const float* rho, const float* rhs, const float* left, const float* right,
                                      const float* bottom, const float* top, const float* dx, const double* x0, double tol, const double* S_h,
                                      const double* lam_h, const double* S_w, const double* lam_w, void* workspace, size_t workspace_bytes, double* scal,
                                      int* flags) {
  PCNN_REQUIRE(h, h && rho && rhs && left && right && bottom && top && dx && S_h && lam_h && S_w && lam_w && workspace && scal && flags,
               "pcnn_varcoef_pcg_setup: null argument");
  if (int rc = vc_check_shape(h, "pcnn_varcoef_pcg_setup", N, H, W)) return rc;
  PCNN_REQUIRE(h, tol > 0.0, "pcnn_varcoef_pcg_setup: tol must be positive");
  const VcWs w = vc_layout(workspace, N, H, W);
  PCNN_REQUIRE(h, workspace_bytes >= vc_bytes(N, H, W), "pcnn_varcoef_pcg_setup: workspace of %zu B, %zu B needed", workspace_bytes, vc_bytes(N, H, W));
  const int tiles = vc_tiles(H, W);
  const int64_t per = (int64_t)(H - 2) * (W - 2);
  if (hipMemsetAsync(flags, 0, (size_t)N * sizeof(int), h->stream) != hipSuccess || hipMemsetAsync(scal, 0, (size_t)N * VS_STRIDE * sizeof(double), h->stream) != hipSuccess)
    PCNN_FAIL(h, "pcnn_varcoef_pcg_setup: cannot clear the per-sample state");
  hipLaunchKernelGGL(varcoef_setup_kernel, vc_tile_grid(N, H, W), dim3(FLUX_THREADS), 0, h->stream, H, W, w.cap, N, rho, rhs, left, right, bottom, top, dx, x0, w.x,
                     w.r, w.part);
  hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, tiles, w.cap, w.part, scal, (int)VS_STRIDE, (int)VS_BB, 0, 0.0, (int*)nullptr);
  hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, tiles, w.cap, w.part + (size_t)N * w.cap, scal, (int)VS_STRIDE, (int)VS_RR, 1,
                     tol * tol, flags);
  hipLaunchKernelGGL(varcoef_reduce_kernel<1>, dim3(N), dim3(EW_THREADS), 0, h->stream, tiles, w.cap, w.part + (size_t)2 * N * w.cap, scal, (int)VS_STRIDE,
                     (int)VS_RHOMIN, 0, 0.0, (int*)nullptr);
  PCNN_CHECK_LAUNCH(h, "pcnn_varcoef_pcg_setup");
  if (int rc = vc_precondition(h, N, H, W, w, S_h, lam_h, S_w, lam_w, scal, VS_RZ0)) return rc;
  hipLaunchKernelGGL(varcoef_update_p_kernel, dim3(vc_ew_blocks(per), N), dim3(EW_THREADS), 0, h->stream, per, 1, 1, scal, flags, w.z, w.p);
  PCNN_CHECK_LAUNCH(h, "pcnn_varcoef_pcg_setup(direction)");
  return 0;
}

extern "C" int pcnn_varcoef_pcg_iterate(pcnn_handle h, int N, int H, int W, const float* rho, const float* dx, double tol, int first_iteration, int iterations,
                                        const double* S_h, const double* lam_h, const double* S_w, const double* lam_w, void* workspace, size_t workspace_bytes,
                                        double* scal, int* flags) {
  PCNN_REQUIRE(h, h && rho && dx && S_h && lam_h && S_w && lam_w && workspace && scal && flags, "pcnn_varcoef_pcg_iterate: null argument");
  if (int rc = vc_check_shape(h, "pcnn_varcoef_pcg_iterate", N, H, W)) return rc;
  PCNN_REQUIRE(h, tol > 0.0 && first_iteration >= 0 && iterations >= 1, "pcnn_varcoef_pcg_iterate: bad tol or iteration range");
  const VcWs w = vc_layout(workspace, N, H, W);
  PCNN_REQUIRE(h, workspace_bytes >= vc_bytes(N, H, W), "pcnn_varcoef_pcg_iterate: workspace of %zu B, %zu B needed", workspace_bytes, vc_bytes(N, H, W));
  const int tiles = vc_tiles(H, W);
  const int64_t per = (int64_t)(H - 2) * (W - 2);
  const int eb = vc_ew_blocks(per);
  for (int it = first_iteration; it < first_iteration + iterations; ++it) {
    const int cur = it & 1;                      // r.z of the current direction sits in slot VS_RZ0 + cur, the next one goes to the other slot
    hipLaunchKernelGGL(varcoef_apply_kernel, vc_tile_grid(N, H, W), dim3(FLUX_THREADS), 0, h->stream, H, W, w.cap, rho, dx, w.p, w.q, w.part);
    hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, tiles, w.cap, w.part, scal, (int)VS_STRIDE, (int)VS_PQ, 0, 0.0, (int*)nullptr);
    hipLaunchKernelGGL(varcoef_update_xr_kernel, dim3(eb, N), dim3(EW_THREADS), 0, h->stream, per, w.cap, cur, scal, flags, w.p, w.q, w.x, w.r, w.part);
    hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, eb, w.cap, w.part, scal, (int)VS_STRIDE, (int)VS_RR, 1, tol * tol, flags);
    PCNN_CHECK_LAUNCH(h, "pcnn_varcoef_pcg_iterate(update)");
    if (int rc = vc_precondition(h, N, H, W, w, S_h, lam_h, S_w, lam_w, scal, VS_RZ0 + (cur ^ 1))) return rc;
    hipLaunchKernelGGL(varcoef_update_p_kernel, dim3(eb, N), dim3(EW_THREADS), 0, h->stream, per, cur, 0, scal, flags, w.z, w.p);
    PCNN_CHECK_LAUNCH(h, "pcnn_varcoef_pcg_iterate(direction)");
  }
  return 0;
}

extern "C" int pcnn_varcoef_pcg_finish(pcnn_handle h, int N, int H, int W, const void* workspace, const float* left, const float* right, const float* bottom,
                                       const float* top, float* soln) {
  PCNN_REQUIRE(h, h && workspace && left && right && bottom && top && soln, "pcnn_varcoef_pcg_finish: null argument");
  if (int rc = vc_check_shape(h, "pcnn_varcoef_pcg_finish", N, H, W)) return rc;
  const VcWs w = vc_layout(const_cast<void*>(workspace), N, H, W);
  pcnn_fd_write_soln(h, N, H, W, 0, w.x, left, right, bottom, top, soln);     // interior from x, the ring as every FD solve here writes it
  PCNN_CHECK_LAUNCH(h, "pcnn_varcoef_pcg_finish");
  return 0;
}

extern "C" int pcnn_varcoef_density(pcnn_handle h, int64_t total, float lo, float hi, float* g) {
  PCNN_REQUIRE(h, h && g && total >= 1, "pcnn_varcoef_density: bad argument");
  PCNN_REQUIRE(h, lo > 0.f && hi >= lo, "pcnn_varcoef_density: need 0 < lo <= hi, got %g, %g", (double)lo, (double)hi);
  int64_t blocks = pcnn_cdiv64(total, 256);
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(varcoef_density_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, total, lo, hi, g);
  PCNN_CHECK_LAUNCH(h, "pcnn_varcoef_density");
  return 0;
}
