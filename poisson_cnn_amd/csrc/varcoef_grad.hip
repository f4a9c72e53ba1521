// Gradients of the variable-density problem div((1/rho) grad u) = f with respect to its DATA: rho, the right-hand side and the edge arrays (DESIGN.md
// section 24).  With (A u - b)_c = sum_k m_k beta_k (u_c - u_k) / h^2 + f_c - sum_e 2 g_e / (rho_c h) on the unknowns (flux_form.h: beta = 2 / (rho_a +
// rho_b), m = 2 on the inward face of a Neumann edge node) and lam the adjoint - A^T lam = d loss / d u on the unknowns, 0 on Dirichlet nodes - the
// implicit-function theorem gives d loss / d theta = -lam^T d(A u - b) / d theta, and d beta / d rho = -beta^2 / 2 at both nodes of a face:
//   d rho_p = sum over the faces (c, k) that touch p of 1/2 beta^2 m lam_c (u_c - u_k) / h^2  -  lam_p sum_e 2 g_e / (rho_p^2 h)     (coef_grad)
//   d f = -lam;   d (value of Dirichlet node d) = du_d + sum_c lam_c m beta / h^2;   d g_e at node c = lam_c 2 / (rho_c h)              (edge_grad)
// A face between two unknowns is counted from each side, and lam = 0 off the unknowns does the bookkeeping: a node with no neighbour on its other
// side (m = 2) has lam != 0 only on a Neumann edge.  The loss sum w r^2, r = L u - f = -(A u - b) with g = 0, has the same gradients with
// lam = 2 coef w r and no solve: pi_loss_bwd_inputs forms that lam in LDS from the shared residual code of flux_form.h and gathers from there.
// All three are gathers, one thread per output, no atomics: equal inputs give equal bits, and a sample's blocks read nothing of another sample.
// coef_grad differences a converged u, whose neighbour differences are O(h) small: it reads fp32, sums in fp64 and rounds once.
#include "flux_form.h"
#include "sweep_common.h"

namespace {

constexpr int EDGE_THREADS = 256;

bool vg_shape_ok(int N, int H, int W) { return pcnn_grid_ok(N, H, W) && H >= 3 && W >= 3 && pcnn_cdiv(H, FLUX_ROWS) <= 65535; }

// 2 where the node at index i of an n-long axis has no neighbour on the side away from `towards` (= i - 1 or i + 1), else 1
__device__ __forceinline__ int vg_m(int i, int towards, int n) {
  const int other = 2 * i - towards;
  return (other < 0 || other >= n) ? 2 : 1;
}

// beta^2 (m_pq lam_p - m_qp lam_q) (u_p - u_q) of the face between p and its neighbour q; 0 where q lies outside the field
template <class T>
__device__ __forceinline__ T vg_face(bool exists, T rp, T rq, T lp, T lq, T up, T uq, int mp, int mq) {
  if (!exists) return T(0);
  const T beta = pcnn_beta_face(rp, rq);
  return (beta * beta) * ((T(mp) * lp - T(mq) * lq) * (up - uq));
}

// the four faces of node (i, j), LDS entry (a, b) of ls and (a + o, b + o) of us / rs, summed (towards i-1 + i+1) + (j-1 + j+1)
template <class T, int LC, int EC>
__device__ __forceinline__ T vg_node_sum(const float (*us)[LC], const float (*rs)[LC], const float (*ls)[EC], int a, int b, int o, int i, int j, int H, int W) {
  const int A = a + o, B = b + o;
  const T up = us[A][B], rp = rs[A][B], lp = ls[a][b];
  const T f0 = vg_face<T>(i > 0, rp, rs[A - 1][B], lp, ls[a - 1][b], up, us[A - 1][B], vg_m(i, i - 1, H), vg_m(i - 1, i, H));
  const T f1 = vg_face<T>(i < H - 1, rp, rs[A + 1][B], lp, ls[a + 1][b], up, us[A + 1][B], vg_m(i, i + 1, H), vg_m(i + 1, i, H));
  const T f2 = vg_face<T>(j > 0, rp, rs[A][B - 1], lp, ls[a][b - 1], up, us[A][B - 1], vg_m(j, j - 1, W), vg_m(j - 1, j, W));
  const T f3 = vg_face<T>(j < W - 1, rp, rs[A][B + 1], lp, ls[a][b + 1], up, us[A][B + 1], vg_m(j, j + 1, W), vg_m(j + 1, j, W));
  return (f0 + f1) + (f2 + f3);
}

// grid (column tiles, row tiles, N) over all nodes
__global__ __launch_bounds__(FLUX_THREADS) void vg_coef_grad_kernel(int H, int W, int mask, const float* __restrict__ rho, const float* __restrict__ dx,
                                                                    const float* __restrict__ u, const float* __restrict__ lam,
                                                                    const float* __restrict__ left, const float* __restrict__ right,
                                                                    const float* __restrict__ bottom, const float* __restrict__ top,
                                                                    float* __restrict__ drho) {
  constexpr int LR = FLUX_ROWS + 2, LC = FLUX_COLS + 2;
  __shared__ float us[LR][LC];
  __shared__ float rs[LR][LC];
  __shared__ float ls[LR][LC];
  const int n = blockIdx.z, I0 = blockIdx.y * FLUX_ROWS, J0 = blockIdx.x * FLUX_COLS;     // LDS (r, c) is node (I0 - 1 + r, J0 - 1 + c)
  const int64_t img = (int64_t)n * H * W;
  pcnn_load_nodes<LR, LC>(us, u + img, H, W, I0 - 1, J0 - 1, 0.f);
  pcnn_load_nodes<LR, LC>(rs, rho + img, H, W, I0 - 1, J0 - 1, 1.f);
  pcnn_load_nodes<LR, LC>(ls, lam + img, H, W, I0 - 1, J0 - 1, 0.f);
  __syncthreads();
  const double h = (double)dx[n], inv_h2 = 1.0 / (h * h);
  const int c = threadIdx.x % FLUX_COLS, r0 = (threadIdx.x / FLUX_COLS) * FLUX_RPT;
  const int j = J0 + c;
  if (j >= W) return;
#pragma unroll
  for (int k = 0; k < FLUX_RPT; ++k) {
    const int r = r0 + k, i = I0 + r;
    if (i >= H) break;
    double g = 0.5 * inv_h2 * vg_node_sum<double, LC, LC>(us, rs, ls, r + 1, c + 1, 0, i, j, H, W);
    double gn = 0.0;                                   // the Neumann data of the edges the node lies on (lam is 0 where it is no unknown)
    if ((mask & 1) && i == 0 && left) gn += (double)left[(int64_t)n * W + j];
    if ((mask & 2) && i == H - 1 && right) gn += (double)right[(int64_t)n * W + j];
    if ((mask & 4) && j == 0 && bottom) gn += (double)bottom[(int64_t)n * H + i];
    if ((mask & 8) && j == W - 1 && top) gn += (double)top[(int64_t)n * H + i];
    const double rp = rs[r + 1][c + 1];
    g -= (double)ls[r + 1][c + 1] * (2.0 * gn / (rp * rp * h));
    drho[img + (int64_t)i * W + j] = (float)g;
  }
}

// The loss version, fp32: lam = 2 coef w r on the tile and a one-node halo (r needs pred and rho one node further out), then the same gather.
// grid (column tiles, row tiles, N) over all nodes
__global__ __launch_bounds__(FLUX_THREADS) void vg_pi_bwd_inputs_kernel(int H, int W, int mask, const float* __restrict__ pred, const float* __restrict__ rho,
                                                                        const float* __restrict__ rhs, const float* __restrict__ dx,
                                                                        const float* __restrict__ coef, float* __restrict__ drhs, float* __restrict__ drho) {
  constexpr int LR = FLUX_ROWS + 4, LC = FLUX_COLS + 4, ER = FLUX_ROWS + 2, EC = FLUX_COLS + 2;
  __shared__ float us[LR][LC];
  __shared__ float rs[LR][LC];
  __shared__ float ls[ER][EC];
  const FdUnknowns un = fd_unknowns(H, W, mask);
  const int n = blockIdx.z, I0 = blockIdx.y * FLUX_ROWS, J0 = blockIdx.x * FLUX_COLS;     // us / rs (r, c) is node (I0 - 2 + r, J0 - 2 + c); ls: (I0 - 1 + r, J0 - 1 + c)
  const int64_t img = (int64_t)n * H * W;
  pcnn_load_nodes_mirrored<LR, LC>(us, pred + img, H, W, I0 - 2, J0 - 2, mask, 0.f);
  pcnn_load_nodes_mirrored<LR, LC>(rs, rho + img, H, W, I0 - 2, J0 - 2, mask, 1.f);
  __syncthreads();
  const float h = dx[n], inv_h2 = 1.f / (h * h), scale = 2.f * coef[n];
  pcnn_flux_residual_halo<true, ER, EC, LC>(ls, us, rs, rhs + img, H, W, I0, J0, mask, un, inv_h2, [&](float v, int i, int j) {
    const int ii = i - un.i0, jj = j - un.j0;           // lam lives on the unknowns of the field itself: a mirror image beyond an edge holds none
    return (ii >= 0 && ii < un.mh && jj >= 0 && jj < un.mw) ? (scale * (float)vc_weight(ii, jj, un.mh, un.mw, mask)) * v : 0.f;
  });
  __syncthreads();
  const int c = threadIdx.x % FLUX_COLS, r0 = (threadIdx.x / FLUX_COLS) * FLUX_RPT;
  const int j = J0 + c;
  if (j >= W) return;
#pragma unroll
  for (int k = 0; k < FLUX_RPT; ++k) {
    const int r = r0 + k, i = I0 + r;
    if (i >= H) break;
    const int64_t at = img + (int64_t)i * W + j;
    if (drhs) drhs[at] = -ls[r + 1][c + 1];
    if (drho) drho[at] = (0.5f * inv_h2) * vg_node_sum<float, LC, EC>(us, rs, ls, r + 1, c + 1, 1, i, j, H, W);
  }
}

// One thread per edge-array entry: grid (pieces of the longer edge, 4 edges, N); edge 0/1/2/3 = left / right / bottom / top = row 0 / H-1, column 0 / W-1
__global__ __launch_bounds__(EDGE_THREADS) void vg_edge_grad_kernel(int H, int W, int mask, const float* __restrict__ rho, const float* __restrict__ dx,
                                                                    const float* __restrict__ lam, const float* __restrict__ du, float* __restrict__ dleft,
                                                                    float* __restrict__ dright, float* __restrict__ dbottom, float* __restrict__ dtop) {
  const int n = blockIdx.z, e = blockIdx.y, t = blockIdx.x * EDGE_THREADS + threadIdx.x;
  const int len = e < 2 ? W : H;
  float* out = e == 0 ? dleft : e == 1 ? dright : e == 2 ? dbottom : dtop;
  if (t >= len || !out) return;
  const int i = e == 0 ? 0 : e == 1 ? H - 1 : t, j = e == 2 ? 0 : e == 3 ? W - 1 : t;
  const int64_t img = (int64_t)n * H * W;
  const double h = (double)dx[n];
  const double rd = rho[img + (int64_t)i * W + j];
  double v;
  if (mask >> e & 1) {                                 // Neumann data g: b_c holds 2 g / (rho_c h)
    v = (double)lam[img + (int64_t)i * W + j] * (2.0 / (rd * h));
  } else if (e >= 2 && ((t == 0 && !(mask & 1)) || (t == H - 1 && !(mask & 2)))) {
    v = 0.0;                                           // the writer puts rows 0 / H-1 last: this entry of a column's array is never read
  } else {                                             // a Dirichlet value: every unknown neighbour c reads it with m beta / h^2
    auto nb = [&](int ci, int cj, bool exists, int m) -> double {
      if (!exists) return 0.0;
      const int64_t p = img + (int64_t)ci * W + cj;
      return (double)lam[p] * (double)m * pcnn_beta_face(rd, (double)rho[p]);
    };
    v = ((nb(i - 1, j, i > 0, vg_m(i - 1, i, H)) + nb(i + 1, j, i < H - 1, vg_m(i + 1, i, H))) +
         (nb(i, j - 1, j > 0, vg_m(j - 1, j, W)) + nb(i, j + 1, j < W - 1, vg_m(j + 1, j, W)))) / (h * h);
    if (du) v += (double)du[img + (int64_t)i * W + j];
  }
  out[(int64_t)n * len + t] = (float)v;
}

}  // namespace

extern "C" int pcnn_varcoef_bc_coef_grad(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, const float* u,
                                         const float* lam, const float* left, const float* right, const float* bottom, const float* top, float* drho) {
  const char* who = "pcnn_varcoef_bc_coef_grad";
  PCNN_REQUIRE(h, h && rho && dx && u && lam && drho, "%s: null argument", who);
  PCNN_REQUIRE(h, neumann_mask >= 0 && neumann_mask < 16, "%s: neumann_mask %d not in 0..15", who, neumann_mask);
  PCNN_REQUIRE(h, vg_shape_ok(N, H, W), "%s: batch %d of %d x %d grids unsupported", who, N, H, W);
  PCNN_REQUIRE(h, drho != rho && drho != u && drho != lam, "%s: drho must not alias an input", who);
  const dim3 grid(pcnn_cdiv(W, FLUX_COLS), pcnn_cdiv(H, FLUX_ROWS), N);
  hipLaunchKernelGGL(vg_coef_grad_kernel, grid, dim3(FLUX_THREADS), 0, h->stream, H, W, neumann_mask, rho, dx, u, lam, left, right, bottom, top, drho);
  PCNN_CHECK_LAUNCH(h, who);
  return 0;
}

extern "C" int pcnn_varcoef_bc_edge_grad(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, const float* lam,
                                         const float* du, float* dleft, float* dright, float* dbottom, float* dtop) {
  const char* who = "pcnn_varcoef_bc_edge_grad";
  PCNN_REQUIRE(h, h && rho && dx && lam, "%s: null argument", who);
  PCNN_REQUIRE(h, neumann_mask >= 0 && neumann_mask < 16, "%s: neumann_mask %d not in 0..15", who, neumann_mask);
  PCNN_REQUIRE(h, vg_shape_ok(N, H, W), "%s: batch %d of %d x %d grids unsupported", who, N, H, W);
  if (!dleft && !dright && !dbottom && !dtop) return 0;
  const dim3 grid(pcnn_cdiv(H > W ? H : W, EDGE_THREADS), 4, N);
  hipLaunchKernelGGL(vg_edge_grad_kernel, grid, dim3(EDGE_THREADS), 0, h->stream, H, W, neumann_mask, rho, dx, lam, du, dleft, dright, dbottom, dtop);
  PCNN_CHECK_LAUNCH(h, who);
  return 0;
}

extern "C" int pcnn_varcoef_bc_pi_loss_bwd_inputs(pcnn_handle h, int N, int H, int W, const float* pred, const float* rho, const float* rhs, const float* dx,
                                                  const float* coef, float* drhs, float* drho, int neumann_mask) {
  const char* who = "pcnn_varcoef_bc_pi_loss_bwd_inputs";
  PCNN_REQUIRE(h, h && pred && rho && rhs && dx && coef, "%s: null argument", who);
  PCNN_REQUIRE(h, neumann_mask >= 0 && neumann_mask < 16, "%s: neumann_mask %d not in 0..15", who, neumann_mask);
  PCNN_REQUIRE(h, vg_shape_ok(N, H, W), "%s: batch %d of %d x %d grids unsupported", who, N, H, W);
  if (!drhs && !drho) return 0;
  PCNN_REQUIRE(h, !drhs || (drhs != pred && drhs != rho && drhs != rhs), "%s: drhs must not alias an input", who);
  PCNN_REQUIRE(h, !drho || (drho != pred && drho != rho && drho != rhs && drho != drhs), "%s: drho must not alias an input or drhs", who);
  const dim3 grid(pcnn_cdiv(W, FLUX_COLS), pcnn_cdiv(H, FLUX_ROWS), N);
  hipLaunchKernelGGL(vg_pi_bwd_inputs_kernel, grid, dim3(FLUX_THREADS), 0, h->stream, H, W, neumann_mask, pred, rho, rhs, dx, coef, drhs, drho);
  PCNN_CHECK_LAUNCH(h, who);
  return 0;
}
