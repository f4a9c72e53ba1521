// The discretisation of the variable-density problem div((1/rho) grad u) = f, once: the face coefficient, the fp32 flux-form
// residual, the 16 x 64 tile with its LDS node loader, and the weight / mirrored index of the per-edge Neumann closure.  varcoef.hip (fp64 solve), varcoef_train.hip (loss, smoother) and error_stats.hip
// (statistics) all take them from here.  The fp64 operator of the solve (stencil_at in varcoef.hip) is NOT here on purpose: it sums
// ((a + b) + c) + d of pc - neighbour, the fp32 residual below (a + b) + (c + d) of neighbour - pc - two roundings, both pinned by goldens.
#pragma once
#include "pcnn_internal.h"

// the tile of the per-tile kernels: FLUX_ROWS x FLUX_COLS nodes by FLUX_THREADS threads, a column and FLUX_RPT consecutive rows per thread
constexpr int FLUX_ROWS = 16, FLUX_COLS = 64, FLUX_THREADS = 256, FLUX_RPT = FLUX_ROWS / (FLUX_THREADS / FLUX_COLS);

// the coefficient of the face between two nodes: the harmonic mean of their 1 / rho
template <class T>
__device__ __forceinline__ T pcnn_beta_face(T a, T b) { return T(2) / (a + b); }

// (L u - rhs) at an interior node: uc / rc the node's u / rho, (u?, r?) its four neighbours towards i-1, i+1, j-1, j+1.  Operation order, all fp32,
// no contraction:  b_k = 2 / (rc + r_k),  d_k = u_k - uc,  s = (b_0 d_0 + b_1 d_1) + (b_2 d_2 + b_3 d_3),  r = s * inv_h2 - f
__device__ __forceinline__ float pcnn_flux_residual(float uc, float rc, float u0, float r0, float u1, float r1, float u2, float r2, float u3, float r3,
                                                    float inv_h2, float f) {
  const float s = (pcnn_beta_face(rc, r0) * (u0 - uc) + pcnn_beta_face(rc, r1) * (u1 - uc)) +
                  (pcnn_beta_face(rc, r2) * (u2 - uc) + pcnn_beta_face(rc, r3) * (u3 - uc));
  return s * inv_h2 - f;
}

// Per-edge Neumann boundaries (DESIGN.md sections 19 and 20; neumann_mask bit 0/1/2/3 = left / right / bottom / top, unknowns fd_unknowns):
// the weight of unknown (ii, jj) of mh x mw in the W inner product: 1/2 per Neumann edge the node lies on (the first / last unknown row or column)
__device__ __forceinline__ double vc_weight(int ii, int jj, int mh, int mw, int mask) {
  const double wi = ((ii == 0 && (mask & 1)) || (ii == mh - 1 && (mask & 2))) ? 0.5 : 1.0;
  const double wj = ((jj == 0 && (mask & 4)) || (jj == mw - 1 && (mask & 8))) ? 0.5 : 1.0;
  return wi * wj;
}
// What the tile entry at index i of an n-long axis reads: i itself; beyond a Neumann end (lo / hi) the mirrored inward neighbour, which makes the
// inward face count twice; otherwise -1: zero Dirichlet data, or tile overhang no stored point uses.  n >= 2 whenever an end is Neumann.
__device__ __forceinline__ int vc_mirror(int i, int n, bool lo, bool hi) {
  if (i == -1 && lo) return 1;
  if (i == n && hi) return n - 2;
  return (i >= 0 && i < n) ? i : -1;
}

// pcnn_load_nodes over nodes, with node -1 / H (W) of an axis whose end is Neumann reading its mirror image (vc_mirror)
template <int LR, int LC, class T>
__device__ __forceinline__ void pcnn_load_nodes_mirrored(T (*t)[LC], const T* __restrict__ src, int H, int W, int I0, int J0, int mask, T fill) {
  for (int e = threadIdx.x; e < LR * LC; e += FLUX_THREADS) {
    const int r = e / LC, c = e % LC;
    const int i = vc_mirror(I0 + r, H, mask & 1, mask & 2), j = vc_mirror(J0 + c, W, mask & 4, mask & 8);
    t[r][c] = (i >= 0 && j >= 0) ? src[(int64_t)i * W + j] : fill;
  }
}

// nodes (I0 .. I0+LR-1) x (J0 .. J0+LC-1) of one sample's H x W field into LDS by the FLUX_THREADS threads; nodes outside the field read `fill`
template <int LR, int LC, class T>
__device__ __forceinline__ void pcnn_load_nodes(T (*t)[LC], const T* __restrict__ src, int H, int W, int I0, int J0, T fill) {
  for (int e = threadIdx.x; e < LR * LC; e += FLUX_THREADS) {
    const int r = e / LC, c = e % LC, i = I0 + r, j = J0 + c;
    t[r][c] = (i >= 0 && i < H && j >= 0 && j < W) ? src[(int64_t)i * W + j] : fill;
  }
}

// The residual on an output tile's nodes and a one-node halo, for the gathers that transpose L: es (r, c) is node (I0 - 1 + r, J0 - 1 + c), us / rs hold
// u / rho one node further out (LDS (a, b) is node (I0 - 2 + a, J0 - 2 + b), loaded by pcnn_load_nodes[_mirrored]).  An entry holds pcnn_flux_residual
// on an unknown of `un` and 0 on a Dirichlet node or outside the field; BC: beyond a Neumann edge it holds the residual of its mirror image, which
// lies within the two-node halo.  keep(v, i, j) -> what is stored for the entry of (unmirrored) node (i, j): the identity for the loss gradient,
// the weighted adjoint of varcoef_grad.hip.  All FLUX_THREADS threads call it between two barriers of their own.
template <bool BC, int ER, int EC, int LC, class Keep>
__device__ __forceinline__ void pcnn_flux_residual_halo(float (*es)[EC], const float (*us)[LC], const float (*rs)[LC], const float* __restrict__ rhs,
                                                        int H, int W, int I0, int J0, int mask, const FdUnknowns& un, float inv_h2, Keep keep) {
  for (int e = threadIdx.x; e < ER * EC; e += FLUX_THREADS) {
    const int r = e / EC, c = e % EC;
    int i = I0 - 1 + r, j = J0 - 1 + c;
    if (BC) {                        // the node whose residual this entry holds: beyond a Neumann edge the mirror image, within the tile's two-node halo
      i = vc_mirror(i, H, mask & 1, mask & 2);
      j = vc_mirror(j, W, mask & 4, mask & 8);
    }
    float v = 0.f;
    if (i >= un.i0 && i <= un.i1 && j >= un.j0 && j <= un.j1) {
      const int a = i - (I0 - 2), b = j - (J0 - 2);
      v = pcnn_flux_residual(us[a][b], rs[a][b], us[a - 1][b], rs[a - 1][b], us[a + 1][b], rs[a + 1][b], us[a][b - 1], rs[a][b - 1], us[a][b + 1],
                             rs[a][b + 1], inv_h2, rhs[(int64_t)i * W + j]);
    }
    es[r][c] = keep(v, I0 - 1 + r, J0 - 1 + c);
  }
}
