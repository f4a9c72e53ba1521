// Variable-density Poisson problem div((1/rho) grad u) = f on the dataset's vertex-centred grid (one spacing per sample, dy = dx), each edge with
// Dirichlet data or (the *_bc_* entry points) a Neumann condition du/dn = g: the flux-form operator, and a conjugate-gradient solve preconditioned by
// the constant-coefficient solve of the same edge types (DESIGN.md sections 16 and 19).
//   beta_{i+1/2,j} = 2 / (rho[i,j] + rho[i+1,j])                                  (the first matrix of dataset/generators/variable_density)
//   (A u)[i,j] = ( beta_{i+1/2,j} (u[i,j] - u[i+1,j]) + beta_{i-1/2,j} (u[i,j] - u[i-1,j])
//                + beta_{i,j+1/2} (u[i,j] - u[i,j+1]) + beta_{i,j-1/2} (u[i,j] - u[i,j-1]) ) / dx^2       on the unknowns,
//   A u = b,  b = -f + (Dirichlet neighbours' values, each times its face coefficient / dx^2).
// All four edges Dirichlet (BC = false): the unknowns are the (H-2) x (W-2) interior nodes and A is symmetric positive definite.
// With Neumann edges (BC = true; neumann_mask bit 0/1/2/3 = left / right / bottom / top) the unknowns are fd_unknowns(H, W, mask), a Neumann edge's
// nodes included.  Such a node has no outward neighbour: the inward face of that direction counts twice (the tiles load rho and p with the mirrored
// index, so the stencil code is the same), and b gains 2 g / (rho_c dx) - the coefficient 1 / rho_c of the boundary face of the node's half cell, NOT
// the mirrored face's beta (that closure is first order).  With w = w_i w_j, w_i = 1/2 on a Neumann edge's row, W A is symmetric: the loop is PCG in
// the W inner product, every dot product a sum of w (..).  For mask 0 every w is 1 and the BC = true kernels give the bits of the BC = false ones.
// All four Neumann (mask 15): W A is semi-definite with the constants as null space; setup projects b (b - sum w b / sum w), finish removes the
// w-mean of x.
// Everything is fp64; rho, f, the boundary arrays and dx are read as fp32 and converted.  No atomics: every dot product is a per-block partial sum
// (fixed tree) reduced per sample by a second one-block stage in a fixed order, so results do not depend on the batch a sample is solved in.
// The face coefficients are built on the fly from an LDS tile of rho with a one-point halo: 20 B per point and product (p 8, rho 4, q 8) against
// 32 B with two fp64 face arrays built once per solve (p 8, faces 16, q 8).
// The face coefficient, the 16 x 64 tile and the LDS node loader are flux_form.h's, shared with varcoef_train.hip and error_stats.hip; the fp64
// operator sum (stencil_at) is this file's alone: its order ((a + b) + c) + d of pc - neighbour is not the fp32 residual's.
// The *_scaled entry points (SC = true) precondition with s o M^-1 (s o r), s = d^-1/2 and d = diag(A) / diag(M) the mean of the
// node's four face coefficients (the inward one twice on a Neumann edge, as in A and in M): one more fp64 field s behind the partial sums, built by the
// setup launch; s o r goes to z - the buffer the transform then reads - from the pass that updates r, and p = s o z + beta p.  The SC = false
// instantiations are the code of the plain entry points, unchanged.
// The *_reaction entry points (RX = true) solve div((1/rho) grad u) - c u = f, i.e. (A + C) u = b with C = diag(c), c >= 0 an fp32
// field read on the unknowns: the operator and setup tiles load c for the thread's own points (no halo: 24 B per point against 20) and add c p inside
// the point's sum; setup also reduces the weighted means cbar of c and bbar of 1/rho over the unknowns and the minimum of c, and the division pass
// divides by bbar (lam_h + lam_w) / dx^2 + cbar - the preconditioner's scale matters now.  W (A + C) is definite for mask 15 once cbar > 0: no
// projection, no mean removal.  The RX = false instantiations are the code of the entry points without the suffix, unchanged.
#include <math.h>
#include <type_traits>
#include "flux_form.h"

namespace {

constexpr int VT_LR = FLUX_ROWS + 2, VT_LC = FLUX_COLS + 2;                                               // the tile of interior points with its halo
constexpr int EW_THREADS = 256, EW_POINTS = 2048, EW_MAX_BLOCKS = 1024;                                   // element-wise kernels: blocks per SAMPLE
// per-sample scalars (doubles) of the solve
// (mask 15 only: VS_WB = sum w b and VS_BBRAW = sum w b^2 of the b before its projection; 0 otherwise)
enum { VS_BB = 0, VS_RR = 1, VS_PQ = 2, VS_RZ0 = 3, VS_RZ1 = 4, VS_RHOMIN = 5, VS_WB = 6, VS_BBRAW = 7, VS_STRIDE = 8 };
// reaction family: N x VX_STRIDE more doubles BEHIND the N x VS_STRIDE table above (whose layout every kernel keeps): the weighted means of c and of
// 1/rho over the unknowns and the minimum of c there (a NaN or an infinity counting as -inf)
enum { VX_CBAR = 0, VX_BBAR = 1, VX_CMIN = 2, VX_STRIDE = 4 };
// what the RX = true kernels get on top: c (N,H,W) and 1 / sum w of the mask's unknowns
struct VcReaction { const float* c; double inv_sum_w; };

// Everything below is sized by the mh x mw unknowns: (H-2) x (W-2) when all four edges are Dirichlet
static inline int vc_tiles(int mh, int mw) { return pcnn_cdiv(mh, FLUX_ROWS) * pcnn_cdiv(mw, FLUX_COLS); }
static inline int vc_ew_blocks(int64_t per) {
  const int64_t b = pcnn_cdiv64(per, EW_POINTS);
  return (int)(b < 1 ? 1 : (b > EW_MAX_BLOCKS ? EW_MAX_BLOCKS : b));
}
static inline int vc_cap(int mh, int mw) {
  const int t = vc_tiles(mh, mw), e = vc_ew_blocks((int64_t)mh * mw);
  return t > e ? t : e;
}
// workspace: x, r, p, q, z (N x mh x mw doubles each; q and z double as the two GEMM intermediates) and three partial-sum arrays of N x cap
// scaled: the field s follows the partial sums, so x and part sit where the shared finish looks for them
// reaction (never scaled): three more partial-sum arrays of N x cap in that place - of sum w c, sum w / rho and min c
struct VcWs { double *x, *r, *p, *q, *z, *part, *s; int cap; };
static inline size_t vc_bytes(int N, int mh, int mw, bool scaled = false, bool reaction = false) {
  return ((scaled ? 6 : 5) * (size_t)N * mh * mw + (reaction ? 6 : 3) * (size_t)N * vc_cap(mh, mw)) * sizeof(double);
}
static inline VcWs vc_layout(void* ws, int N, int mh, int mw) {
  VcWs l;
  const size_t v = (size_t)N * mh * mw;
  l.cap = vc_cap(mh, mw);
  l.x = static_cast<double*>(ws); l.r = l.x + v; l.p = l.r + v; l.q = l.p + v; l.z = l.q + v; l.part = l.z + v;
  l.s = l.part + 3 * (size_t)N * l.cap;          // (only the scaled and the reaction workspaces reach that far)
  return l;
}

// (the weight vc_weight of an unknown in the W inner product and the mirrored tile index vc_mirror are flux_form.h's, shared with varcoef_train.hip)
// (row, column) of the flat index k = blockIdx.x * EW_THREADS + threadIdx.x + m * gridDim.x * EW_THREADS of the element-wise kernels, m = 0, 1, ..:
// one division at the start, none per point.  At most EW_MAX_BLOCKS * EW_THREADS = 2^18 per step: int is enough.
struct VcWalk {
  int ii, jj, di, dj, mw;
  __device__ __forceinline__ VcWalk(int mw_) : mw(mw_) {
    const int k0 = blockIdx.x * EW_THREADS + threadIdx.x, stride = gridDim.x * EW_THREADS;
    ii = k0 / mw; jj = k0 % mw; di = stride / mw; dj = stride % mw;
  }
  __device__ __forceinline__ void next() {
    ii += di; jj += dj;
    if (jj >= mw) { jj -= mw; ++ii; }
  }
};

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
// BC: I0 / J0 is -1 for the first tile of an axis whose low edge is Neumann; node -1 then reads node 1 and node H (W) reads node H-2 (W-2), the
// mirrored inward neighbour of an edge node (beyond a Dirichlet edge this is overhang).
template <bool BC>
__device__ __forceinline__ float load_rho_tile(float (*rs)[VT_LC], const float* __restrict__ rho_n, int H, int W, int I0, int J0) {
  float mn = INFINITY;
  for (int e = threadIdx.x; e < VT_LR * VT_LC; e += FLUX_THREADS) {
    const int r = e / VT_LC, c = e % VT_LC;
    int i = I0 + r, j = J0 + c;
    if (BC) {
      i = i < 0 ? 1 : (i == H ? H - 2 : i);
      j = j < 0 ? 1 : (j == W ? W - 2 : j);
    }
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

// q = A p and the tile's share of p.q (BC: of sum w p q).  grid (column tiles, row tiles, N) over the nh x nw unknowns; part[n][tile]
// RX: q = (A + C) p - c of the thread's own point joins the point's sum before p.q is formed.
template <bool BC, bool RX = false>
__global__ __launch_bounds__(FLUX_THREADS) void varcoef_apply_kernel(int H, int W, int cap, int mask, const float* __restrict__ rho, const float* __restrict__ dx,
                                                                     const double* __restrict__ p, double* __restrict__ q, double* __restrict__ part,
                                                                     const float* __restrict__ reaction) {
  __shared__ float rs[VT_LR][VT_LC];
  __shared__ double ps[VT_LR][VT_LC];
  __shared__ double red[FLUX_THREADS];
  const FdUnknowns u = fd_unknowns(H, W, BC ? mask : 0);
  const int nh = u.mh, nw = u.mw, n = blockIdx.z, I0 = blockIdx.y * FLUX_ROWS, J0 = blockIdx.x * FLUX_COLS;
  const int64_t per = (int64_t)nh * nw;
  const double* pn = p + (int64_t)n * per;
  load_rho_tile<BC>(rs, rho + (int64_t)n * H * W, H, W, u.i0 + I0 - 1, u.j0 + J0 - 1);
  if (BC) {
    for (int e = threadIdx.x; e < VT_LR * VT_LC; e += FLUX_THREADS) {
      const int r = e / VT_LC, c = e % VT_LC;
      const int ii = vc_mirror(I0 + r - 1, nh, mask & 1, mask & 2), jj = vc_mirror(J0 + c - 1, nw, mask & 4, mask & 8);
      ps[r][c] = (ii >= 0 && jj >= 0) ? pn[(int64_t)ii * nw + jj] : 0.0;
    }
  } else {
    pcnn_load_nodes<VT_LR, VT_LC>(ps, pn, nh, nw, I0 - 1, J0 - 1, 0.0);             // interior indices; zero Dirichlet data outside
  }
  __syncthreads();
  const double h = (double)dx[n], inv_h2 = 1.0 / (h * h);
  const int c = threadIdx.x % FLUX_COLS, r0 = (threadIdx.x / FLUX_COLS) * FLUX_RPT;
  double s = 0.0;
  if (J0 + c < nw) {
#pragma unroll
    for (int k = 0; k < FLUX_RPT; ++k) {
      const int r = r0 + k;
      if (I0 + r < nh) {
        double v = stencil_at(faces_at(rs, r, c), ps, r, c, inv_h2);
        if (RX) v += (double)reaction[((int64_t)n * H + u.i0 + I0 + r) * W + u.j0 + J0 + c] * ps[r + 1][c + 1];
        q[(int64_t)n * per + (int64_t)(I0 + r) * nw + J0 + c] = v;
        const double pv = ps[r + 1][c + 1] * v;
        s += BC ? vc_weight(I0 + r, J0 + c, nh, nw, mask) * pv : pv;
      }
    }
  }
  const double tot = block_sum<FLUX_THREADS>(s, red);
  if (threadIdx.x == 0) part[(int64_t)n * cap + blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// Start of a solve: b from f, rho, the four boundary arrays and dx; x = x0 (the unknowns of the optional initial guess, else 0); r = b - A x0; the
// tile's shares of b.b and r.r and its minimum of rho.  left/right (N,W): values on rows 0 / H-1; bottom/top (N,H): values on columns 0 / W-1 - or,
// on a Neumann edge (BC), du/dn there: such a node's b gains 2 g / (rho_c dx) per Neumann edge it lies on, and the sums are weighted.
// mask 15 (b_out != NULL): b is kept in b_out for the projection pass, and the second partial is the tile's share of sum w b - r.r is summed there.
// SC: s = (mean of the four face coefficients)^-1/2 -> s_out and s o r -> t_out (mask 15: the projection pass writes it, from the projected r).
// RX: r = b - (A + C) x0, and three more partials per tile behind the first three (part3): the tile's shares of the weighted means of c and of 1/rho
// over the unknowns and its minimum of c, a NaN or an infinity counting as -inf.
template <bool BC, bool SC, bool RX = false>
__global__ __launch_bounds__(FLUX_THREADS) void varcoef_setup_kernel(int H, int W, int cap, int N, int mask, const float* __restrict__ rho,
                                                                     const float* __restrict__ f, const float* __restrict__ left,
                                                                     const float* __restrict__ right, const float* __restrict__ bottom,
                                                                     const float* __restrict__ top, const float* __restrict__ dx,
                                                                     const double* __restrict__ x0, double* __restrict__ x, double* __restrict__ rr_out,
                                                                     double* __restrict__ b_out, double* __restrict__ part, double* __restrict__ s_out,
                                                                     double* __restrict__ t_out, VcReaction rx, double* __restrict__ part3) {
  __shared__ float rs[VT_LR][VT_LC];
  __shared__ double ps[VT_LR][VT_LC];
  __shared__ double red[FLUX_THREADS];
  const FdUnknowns u = fd_unknowns(H, W, BC ? mask : 0);
  const int nh = u.mh, nw = u.mw, n = blockIdx.z, I0 = blockIdx.y * FLUX_ROWS, J0 = blockIdx.x * FLUX_COLS;
  const int64_t per = (int64_t)nh * nw;
  const float mn = load_rho_tile<BC>(rs, rho + (int64_t)n * H * W, H, W, u.i0 + I0 - 1, u.j0 + J0 - 1);
  for (int e = threadIdx.x; e < VT_LR * VT_LC; e += FLUX_THREADS) {
    const int r = e / VT_LC, c = e % VT_LC;
    int ii = I0 + r - 1, jj = J0 + c - 1;
    if (BC) {
      ii = vc_mirror(ii, nh, mask & 1, mask & 2);
      jj = vc_mirror(jj, nw, mask & 4, mask & 8);
    }
    ps[r][c] = (x0 && ii >= 0 && ii < nh && jj >= 0 && jj < nw) ? x0[((int64_t)n * H + ii + u.i0) * W + jj + u.j0] : 0.0;
  }
  __syncthreads();
  const double h = (double)dx[n], inv_h2 = 1.0 / (h * h);
  const int c = threadIdx.x % FLUX_COLS, r0 = (threadIdx.x / FLUX_COLS) * FLUX_RPT;
  double sbb = 0.0, srr = 0.0, scc = 0.0, sib = 0.0;
  float cmn = INFINITY;
  if (J0 + c < nw) {
#pragma unroll
    for (int k = 0; k < FLUX_RPT; ++k) {
      const int r = r0 + k, ii = I0 + r, jj = J0 + c;
      if (ii < nh) {
        const int i = ii + u.i0, j = jj + u.j0;                                     // the node
        const Faces fc = faces_at(rs, r, c);
        const double gl = (double)left[(int64_t)n * W + j], gr = (double)right[(int64_t)n * W + j];
        const double gb = (double)bottom[(int64_t)n * H + i], gt = (double)top[(int64_t)n * H + i];
        const double gn = BC ? 2.0 / ((double)rs[r + 1][c + 1] * h) : 0.0;          // Neumann: 1 / rho_c of the half cell's boundary face
        double b = -(double)f[((int64_t)n * H + i) * W + j];
        if (BC && i == 0) b += gn * gl;                                              // (row 0 is an unknown only when left is Neumann)
        else if (i == 1 && !(BC && (mask & 1))) b += fc.lo_i * inv_h2 * gl;
        if (BC && i == H - 1) b += gn * gr;
        else if (i == H - 2 && !(BC && (mask & 2))) b += fc.hi_i * inv_h2 * gr;
        if (BC && j == 0) b += gn * gb;
        else if (j == 1 && !(BC && (mask & 4))) b += fc.lo_j * inv_h2 * gb;
        if (BC && j == W - 1) b += gn * gt;
        else if (j == W - 2 && !(BC && (mask & 8))) b += fc.hi_j * inv_h2 * gt;
        double ax = stencil_at(fc, ps, r, c, inv_h2);
        if (RX) {
          const float cv = rx.c[((int64_t)n * H + i) * W + j];
          const double w = BC ? vc_weight(ii, jj, nh, nw, mask) : 1.0;
          ax += (double)cv * ps[r + 1][c + 1];
          scc += w * (double)cv;
          sib += w / (double)rs[r + 1][c + 1];
          cmn = fminf(cmn, (cv == cv && fabsf(cv) != INFINITY) ? cv : -INFINITY);
        }
        const double res = b - ax;
        const int64_t o = (int64_t)n * per + (int64_t)ii * nw + jj;
        x[o] = ps[r + 1][c + 1];
        rr_out[o] = res;
        if (SC) {
          const double sc = 1.0 / sqrt(0.25 * (((fc.lo_i + fc.hi_i) + fc.lo_j) + fc.hi_j));
          s_out[o] = sc;
          if (!b_out) t_out[o] = sc * res;
        }
        if (BC) {
          const double w = vc_weight(ii, jj, nh, nw, mask);
          sbb += w * (b * b);
          if (b_out) {
            b_out[o] = b;
            srr += w * b;
          } else {
            srr += w * (res * res);
          }
        } else {
          sbb += b * b;
          srr += res * res;
        }
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
  if (RX) {
    const double tcc = block_sum<FLUX_THREADS>(scc, red);
    const double tib = block_sum<FLUX_THREADS>(sib, red);
    __syncthreads();
    red[threadIdx.x] = (double)cmn;
    __syncthreads();
    pcnn_block_reduce<double, FLUX_THREADS>(red, threadIdx.x, pcnn_min_op());
    if (threadIdx.x == 0) {
      part3[(int64_t)n * cap + tile] = tcc * rx.inv_sum_w;
      part3[((int64_t)N + n) * cap + tile] = tib * rx.inv_sum_w;
      part3[((int64_t)2 * N + n) * cap + tile] = red[0];
    }
  }
}

// mask 15, after the setup kernel: b and r lose m = sum w b / sum w (the compatibility projection: W A has the constants as null space, so a
// solvable b has sum w b = 0); the block's shares of sum w b^2 and sum w r^2 of the projected fields.  grid (blocks per sample, N)
// SC: t = s o (the projected r)
template <bool SC>
__global__ __launch_bounds__(EW_THREADS) void varcoef_project_kernel(int mh, int mw, int cap, int N, double sum_w, const double* __restrict__ scal,
                                                                     const double* __restrict__ b, double* __restrict__ r, double* __restrict__ part,
                                                                     const double* __restrict__ s, double* __restrict__ t) {
  __shared__ double red[EW_THREADS];
  const int n = blockIdx.y;
  const int64_t per = (int64_t)mh * mw, base = (int64_t)n * per;
  const double m = scal[n * VS_STRIDE + VS_WB] / sum_w;
  double sbb = 0.0, srr = 0.0;
  VcWalk at(mw);
  for (int64_t k = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; k < per; k += (int64_t)gridDim.x * EW_THREADS, at.next()) {
    const double w = vc_weight(at.ii, at.jj, mh, mw, 15), bp = b[base + k] - m, rp = r[base + k] - m;
    r[base + k] = rp;
    if (SC) t[base + k] = s[base + k] * rp;
    sbb += w * (bp * bp);
    srr += w * (rp * rp);
  }
  const double tbb = block_sum<EW_THREADS>(sbb, red);
  const double trr = block_sum<EW_THREADS>(srr, red);
  if (threadIdx.x == 0) {
    part[(int64_t)n * cap + blockIdx.x] = tbb;
    part[((int64_t)N + n) * cap + blockIdx.x] = trr;
  }
}

// mask 15, at the finish: the block's share of sum w x (mean == NULL), then x -= mean[n] / sum w: the solution whose trapezoidal integral vanishes
__global__ __launch_bounds__(EW_THREADS) void varcoef_mean_kernel(int mh, int mw, int cap, double sum_w, const double* __restrict__ mean, double* __restrict__ x,
                                                                  double* __restrict__ part) {
  __shared__ double red[EW_THREADS];
  const int n = blockIdx.y;
  const int64_t per = (int64_t)mh * mw, base = (int64_t)n * per;
  const double m = mean ? mean[n] / sum_w : 0.0;
  double s = 0.0;
  VcWalk at(mw);
  for (int64_t k = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; k < per; k += (int64_t)gridDim.x * EW_THREADS, at.next()) {
    if (mean) x[base + k] -= m;
    else s += vc_weight(at.ii, at.jj, mh, mw, 15) * x[base + k];
  }
  if (mean) return;                                  // uniform over the grid
  const double tot = block_sum<EW_THREADS>(s, red);
  if (threadIdx.x == 0) part[(int64_t)n * cap + blockIdx.x] = tot;
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
// BC: the share of sum w r^2 over the mh x mw unknowns (per = mh mw), in the same order: for mask 0 the same bits.
// SC: t = s o r, what the transform reads next, from the r this pass holds in a register.  It is written for a flagged sample too (t shares z's
// memory, which the back-transform has overwritten since): from r and s alone, and a flagged sample's alpha = 0 keeps it away from x.
template <bool BC, bool SC>
__global__ __launch_bounds__(EW_THREADS) void varcoef_update_xr_kernel(int64_t per, int mh, int mw, int mask, int cap, int cur, const double* __restrict__ scal,
                                                                       const int* __restrict__ flags,
                                                                       const double* __restrict__ p, const double* __restrict__ q, double* __restrict__ x,
                                                                       double* __restrict__ r, double* __restrict__ part, const double* __restrict__ s,
                                                                       double* __restrict__ t) {
  __shared__ double red[EW_THREADS];
  const int n = blockIdx.y;
  const double pq = scal[n * VS_STRIDE + VS_PQ], rz = scal[n * VS_STRIDE + VS_RZ0 + cur];
  const double alpha = (flags[n] || !(pq > 0.0)) ? 0.0 : rz / pq;
  const int64_t base = (int64_t)n * per;
  double sum = 0.0;
  VcWalk at(BC ? mw : 1);
  for (int64_t k = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; k < per; k += (int64_t)gridDim.x * EW_THREADS) {
    double rn = r[base + k];
    if (alpha != 0.0) {                            // uniform over the block
      x[base + k] += alpha * p[base + k];
      rn -= alpha * q[base + k];
      r[base + k] = rn;
    }
    if (SC) t[base + k] = s[base + k] * rn;
    if (BC) {
      sum += vc_weight(at.ii, at.jj, mh, mw, mask) * (rn * rn);
      at.next();
    } else {
      sum += rn * rn;
    }
  }
  const double tot = block_sum<EW_THREADS>(sum, red);
  if (threadIdx.x == 0) part[(int64_t)n * cap + blockIdx.x] = tot;
}

// the eigenvalue division of the preconditioner, in place on the coefficients c = S_h r S_w: c / (lam_h + lam_w).  S is orthonormal and symmetric,
// so r.z = sum c^2 / (lam_h + lam_w): the block's share of r.z comes from this pass and needs no further read of r and z.
// BC: c = Vinv_h r Vinv_w^T with V^T W V = I per axis, so Vinv = V^T W and sum w r z is the same sum c^2 / (lam_h + lam_w).  The null mode of the
// all-Neumann operator (lam_h + lam_w = 0) is dropped, as fd_divide_kernel drops it: z then has no constant part.
// RX: the divisor is bbar (lam_h + lam_w) / dx^2 + cbar with the sample's two means of extra (VX_*): the eigenvalues of bbar M + cbar I, M with its
// 1/dx^2 - the scale no longer cancels.  The lam = 0 mode is kept when cbar > 0 (its divisor is cbar) and dropped otherwise.
template <bool BC, bool RX = false>
__global__ __launch_bounds__(EW_THREADS) void varcoef_divide_kernel(int nh, int nw, int cap, const double* __restrict__ lam_h, const double* __restrict__ lam_w,
                                                                    double* __restrict__ T, double* __restrict__ part, const float* __restrict__ dx,
                                                                    const double* __restrict__ extra) {
  __shared__ double red[EW_THREADS];
  const int n = blockIdx.y;
  double* Tn = T + (int64_t)n * nh * nw;
  double s = 0.0;
  double kb = 1.0, cb = 0.0;
  if (RX) {
    const double h = (double)dx[n];
    kb = extra[n * VX_STRIDE + VX_BBAR] / (h * h);
    cb = extra[n * VX_STRIDE + VX_CBAR];
  }
  for (int i = blockIdx.x; i < nh; i += gridDim.x) {           // a block takes whole rows: no index division per point
    const double li = lam_h[i];
    double* row = Tn + (int64_t)i * nw;
    for (int j = threadIdx.x; j < nw; j += EW_THREADS) {
      const double c = row[j], l = li + lam_w[j];
      const double z = RX ? ((fabs(l) > 1e-13 || cb > 0.0) ? c / (kb * l + cb) : 0.0) : ((!BC || fabs(l) > 1e-13) ? c / l : 0.0);
      row[j] = z;
      s += c * z;
    }
  }
  const double tot = block_sum<EW_THREADS>(s, red);
  if (threadIdx.x == 0) part[(int64_t)n * cap + blockIdx.x] = tot;
}

// p = z + beta p, beta = (r.z)_new / (r.z)_old from the sample's scalars; 0 for a flagged sample and for the first direction (first = 1).
// With beta = 0 the old p is not read: before the first direction it is memory nobody has written, and 0 * NaN is NaN.
// SC: z arrives as M^-1 (s o r) and is multiplied by s here, where it is first consumed.
template <bool SC>
__global__ __launch_bounds__(EW_THREADS) void varcoef_update_p_kernel(int64_t per, int cur, int first, const double* __restrict__ scal, const int* __restrict__ flags,
                                                                      const double* __restrict__ z, double* __restrict__ p, const double* __restrict__ s) {
  const int n = blockIdx.y;
  const double rz_old = scal[n * VS_STRIDE + VS_RZ0 + cur], rz_new = scal[n * VS_STRIDE + VS_RZ0 + (cur ^ 1)];
  const double beta = (first || flags[n] || !(rz_old > 0.0)) ? 0.0 : rz_new / rz_old;
  const int64_t base = (int64_t)n * per;
  for (int64_t k = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; k < per; k += (int64_t)gridDim.x * EW_THREADS) {
    const double zk = SC ? s[base + k] * z[base + k] : z[base + k];
    p[base + k] = beta != 0.0 ? zk + beta * p[base + k] : zk;
  }
}

// g -> lo + (hi - lo) |g|: a density field from a smooth function already scaled to max|g| = 1
__global__ void varcoef_density_kernel(int64_t total, float lo, float hi, float* __restrict__ g) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) g[i] = lo + (hi - lo) * fminf(fabsf(g[i]), 1.f);
}

// The smooth profile, g -> lo + (hi - lo) (g - min g) / (max g - min g) per sample, in two launches of grid (blocks per sample, N).
// First the block's minimum and maximum of g[n] by the fixed tree -> mm[n][block][0 / 1] ...
constexpr int DS_MAX_BLOCKS = EW_THREADS;          // at most one partial per thread of the second launch
struct vc_fmin_op { __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); } };
struct vc_fmax_op { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };
__global__ __launch_bounds__(EW_THREADS) void varcoef_density_range_kernel(int64_t per, const float* __restrict__ g, float* __restrict__ mm) {
  __shared__ float lo_s[EW_THREADS], hi_s[EW_THREADS];
  const int n = blockIdx.y, t = threadIdx.x;
  const float* gn = g + (int64_t)n * per;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t k = (int64_t)blockIdx.x * EW_THREADS + t; k < per; k += (int64_t)gridDim.x * EW_THREADS) {
    const float v = gn[k];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  lo_s[t] = mn;
  hi_s[t] = mx;
  __syncthreads();
  pcnn_block_reduce<float, EW_THREADS>(lo_s, t, vc_fmin_op());
  pcnn_block_reduce<float, EW_THREADS>(hi_s, t, vc_fmax_op());
  if (t == 0) {
    mm[((int64_t)n * gridDim.x + blockIdx.x) * 2] = lo_s[0];
    mm[((int64_t)n * gridDim.x + blockIdx.x) * 2 + 1] = hi_s[0];
  }
}
// ... then every block reduces its sample's gridDim.x partials by the same tree (so all blocks of a sample hold the same two numbers) and maps its
// points.  A constant g gives lo.  min and max are exact in any order; the map is clamped to [lo, hi] against the rounding of its last addition.
__global__ __launch_bounds__(EW_THREADS) void varcoef_density_smooth_kernel(int64_t per, float lo, float hi, const float* __restrict__ mm, float* __restrict__ g) {
  __shared__ float lo_s[EW_THREADS], hi_s[EW_THREADS];
  const int n = blockIdx.y, t = threadIdx.x;
  lo_s[t] = t < (int)gridDim.x ? mm[((int64_t)n * gridDim.x + t) * 2] : INFINITY;
  hi_s[t] = t < (int)gridDim.x ? mm[((int64_t)n * gridDim.x + t) * 2 + 1] : -INFINITY;
  __syncthreads();
  pcnn_block_reduce<float, EW_THREADS>(lo_s, t, vc_fmin_op());
  pcnn_block_reduce<float, EW_THREADS>(hi_s, t, vc_fmax_op());
  const float mn = lo_s[0], span = hi_s[0] - mn, inv = span > 0.f ? 1.f / span : 0.f;
  float* gn = g + (int64_t)n * per;
  for (int64_t k = (int64_t)blockIdx.x * EW_THREADS + t; k < per; k += (int64_t)gridDim.x * EW_THREADS)
    gn[k] = fminf(fmaxf(lo + (hi - lo) * ((gn[k] - mn) * inv), lo), hi);
}

// A (solution, right-hand side) pair of the DISCRETE problem without a solve: u = sum_{A,B} c[A,B] phi_A(x_i) psi_B(y_j) in the
// homogeneous eigenfunction families of the mask's edge types, and f = L_h(rho) u = -(A u) by the operator above.  u is synthesised in fp64 where
// it is differenced - differencing an fp32-rounded u puts eps32 4 n^2 / (pi k)^2 of grid-scale noise into f - and only the two results are rounded.
// One block per FLUX_ROWS x FLUX_COLS tile of NODES of one sample, grid (column tiles, row tiles, N):
//   1. the trig tables of the tile and its one-node halo, each entry once: F[A][r] = phi_A(x), P[B][c] = psi_B(y); beyond a Neumann end the table
//      holds the mirrored node's value (the families are even about such an end), beyond the field 0 (no stored point uses it)
//   2. T[A][c] = sum_B c[A,B] P[B][c]
//   3. us[r][c] = sum_A F[A][r] T[A][c], an exact 0 on a node that is not an unknown (the sine factor leaves 1e-16 there)
//   4. a column and FLUX_RPT rows per thread: soln = (float) u on every node, rhs = (float) -stencil_at on the unknowns, 0 elsewhere.
// No thread leaves before the last barrier; rows >= H and columns >= W are computed and not stored; no atomics.
constexpr int VSER_MAXK = 16;
// mode k+1 of the family `kind` (bit 0: cosine, bit 1: quarter waves - dataset._axis_basis) at node idx of an n-point axis: sin / cos of
// (q / 2) idx pi / (n - 1), q = 2 (k + 1) - (quarter ? 1 : 0).  q idx is reduced modulo the period 4 (n - 1) in integers, so the argument is exact.
__device__ __forceinline__ double vser_basis(int kind, int k, int idx, int n) {
  const int64_t q = 2 * (k + 1) - ((kind & 2) ? 1 : 0), period = 4 * (int64_t)(n - 1);
  const double x = (double)((q * idx) % period) / (double)(2 * (int64_t)(n - 1));
  return (kind & 1) ? cospi(x) : sinpi(x);
}
__device__ __forceinline__ int vser_kind(bool lo, bool hi) { return (lo ? 1 : 0) | (lo != hi ? 2 : 0); }

__global__ __launch_bounds__(FLUX_THREADS) void varcoef_series_pair_kernel(int H, int W, int ka, int kb, int mask, const float* __restrict__ coef,
                                                                           const float* __restrict__ rho, const float* __restrict__ dx,
                                                                           float* __restrict__ soln, float* __restrict__ rhs) {
  __shared__ float rs[VT_LR][VT_LC];
  __shared__ double us[VT_LR][VT_LC];
  __shared__ double P[VSER_MAXK][VT_LC], T[VSER_MAXK][VT_LC];
  __shared__ double F[VSER_MAXK][VT_LR];
  __shared__ double cs[VSER_MAXK * VSER_MAXK];
  const FdUnknowns u = fd_unknowns(H, W, mask);
  const int n = blockIdx.z, I0 = blockIdx.y * FLUX_ROWS, J0 = blockIdx.x * FLUX_COLS, tid = threadIdx.x;
  const int kind_a = vser_kind(mask & 1, mask & 2), kind_b = vser_kind(mask & 4, mask & 8);
  load_rho_tile<true>(rs, rho + (int64_t)n * H * W, H, W, I0 - 1, J0 - 1);
  for (int e = tid; e < ka * kb; e += FLUX_THREADS) cs[e] = (double)coef[(int64_t)n * ka * kb + e];
  for (int e = tid; e < ka * VT_LR; e += FLUX_THREADS) {
    const int A = e / VT_LR, r = e % VT_LR, i = vc_mirror(I0 + r - 1, H, mask & 1, mask & 2);
    F[A][r] = i >= 0 ? vser_basis(kind_a, A, i, H) : 0.0;
  }
  for (int e = tid; e < kb * VT_LC; e += FLUX_THREADS) {
    const int B = e / VT_LC, c = e % VT_LC, j = vc_mirror(J0 + c - 1, W, mask & 4, mask & 8);
    P[B][c] = j >= 0 ? vser_basis(kind_b, B, j, W) : 0.0;
  }
  __syncthreads();
  for (int e = tid; e < ka * VT_LC; e += FLUX_THREADS) {
    const int A = e / VT_LC, c = e % VT_LC;
    double s = 0.0;
    for (int B = 0; B < kb; ++B) s += cs[A * kb + B] * P[B][c];
    T[A][c] = s;
  }
  __syncthreads();
  for (int e = tid; e < VT_LR * VT_LC; e += FLUX_THREADS) {
    const int r = e / VT_LC, c = e % VT_LC;
    const int i = vc_mirror(I0 + r - 1, H, mask & 1, mask & 2), j = vc_mirror(J0 + c - 1, W, mask & 4, mask & 8);
    double s = 0.0;
    for (int A = 0; A < ka; ++A) s += F[A][r] * T[A][c];
    us[r][c] = (i >= u.i0 && i <= u.i1 && j >= u.j0 && j <= u.j1) ? s : 0.0;
  }
  __syncthreads();
  const double h = (double)dx[n], inv_h2 = 1.0 / (h * h);
  const int c = tid % FLUX_COLS, r0 = (tid / FLUX_COLS) * FLUX_RPT, j = J0 + c;
  if (j < W) {
#pragma unroll
    for (int k = 0; k < FLUX_RPT; ++k) {
      const int r = r0 + k, i = I0 + r;
      if (i < H) {
        const bool unknown = i >= u.i0 && i <= u.i1 && j >= u.j0 && j <= u.j1;
        const int64_t o = ((int64_t)n * H + i) * W + j;
        soln[o] = (float)us[r + 1][c + 1];
        rhs[o] = unknown ? (float)-stencil_at(faces_at(rs, r, c), us, r, c, inv_h2) : 0.f;
      }
    }
  }
}

// the six arrays of a preconditioner: per axis the eigenbasis of the constant-coefficient 1-D operator on that axis' unknowns, the second axis'
// matrices transposed (applied from the right) - pcnn_fd_poisson_mixed's.  All-Dirichlet: the orthonormal DST-I matrix S for all four.
struct VcBasis { const double *Vinv_h, *V_h, *lam_h, *VinvT_w, *VT_w, *lam_w; };

// the shape checks of every entry point; u: the unknowns of the mask (0 for the all-Dirichlet entry points)
static int vc_check_shape(pcnn_handle h, const char* who, int N, int H, int W, int mask, FdUnknowns* u) {
  PCNN_REQUIRE(h, N >= 1 && N <= 65535, "%s: batch %d not in 1..65535", who, N);
  PCNN_REQUIRE(h, mask >= 0 && mask < 16, "%s: neumann_mask %d not in 0..15", who, mask);
  PCNN_REQUIRE(h, H >= 3 && W >= 3, "%s: grid %d x %d unsupported", who, H, W);
  *u = fd_unknowns(H, W, mask);
  PCNN_REQUIRE(h, pcnn_cdiv(u->mh, FLUX_ROWS) <= 65535, "%s: grid %d x %d unsupported", who, H, W);
  return 0;
}
static dim3 vc_tile_grid(int N, const FdUnknowns& u) { return dim3(pcnn_cdiv(u.mw, FLUX_COLS), pcnn_cdiv(u.mh, FLUX_ROWS), N); }

// z = M^-1 r, M the constant-coefficient 5-point operator of the same edge types with zero data (its 1/dx^2 left out: a positive factor of M does not
// change the iterates): z = V_h ((Vinv_h r VinvT_w) ./ (lam_h + lam_w)) VT_w as four fp64 matrix-core products; q holds the half-transformed fields.
// r.z (BC: sum w r z) -> scal slot.
// SC: the transform reads t = s o r, which the pass before left in z, and z comes out as M^-1 t: with c the coefficients of t the division pass' sum
// c^2 / (lam_h + lam_w) is (s o r).M^-1 (s o r) = r.(s o M^-1 (s o r)), the r.z of the scaled preconditioner (diag(s) commutes with the weights).
// RX: the division takes dx and the two means behind the scalar table.
template <bool BC, bool SC, bool RX = false>
static int vc_precondition(pcnn_handle h, int N, const FdUnknowns& u, const VcWs& w, const VcBasis& B, double* scal, int slot, const float* dx = nullptr) {
  const int64_t per = (int64_t)u.mh * u.mw;
  const int eb = vc_ew_blocks(per);
  if (int rc = pcnn_two_sided_gemm_f64(h, N, u.mh, u.mw, B.Vinv_h, SC ? w.z : w.r, B.VinvT_w, w.q, w.z)) return rc;
  hipLaunchKernelGGL((varcoef_divide_kernel<BC, RX>), dim3(eb, N), dim3(EW_THREADS), 0, h->stream, u.mh, u.mw, w.cap, B.lam_h, B.lam_w, w.z, w.part, dx,
                     (const double*)(RX ? scal + (size_t)N * VS_STRIDE : nullptr));
  hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, eb, w.cap, w.part, scal, (int)VS_STRIDE, slot, 0, 0.0, (int*)nullptr);
  PCNN_CHECK_LAUNCH(h, "pcnn_varcoef_pcg(divide)");
  return pcnn_two_sided_gemm_f64(h, N, u.mh, u.mw, B.V_h, w.z, B.VT_w, w.q, w.z);
}

// The bodies of the entry points: BC = false behind the all-Dirichlet names (mask 0, S for every basis matrix), BC = true behind the *_bc_* names.
template <bool BC, bool RX = false>
static int vc_apply(pcnn_handle h, const char* who, int N, int H, int W, int mask, const float* rho, const float* dx, const double* p, double* q, double* pq,
                    const float* reaction = nullptr) {
  PCNN_REQUIRE(h, h && rho && dx && p && q && pq && (!RX || reaction), "%s: null argument", who);
  FdUnknowns u;
  if (int rc = vc_check_shape(h, who, N, H, W, mask, &u)) return rc;
  const int cap = vc_cap(u.mh, u.mw), tiles = vc_tiles(u.mh, u.mw);
  if (int rc = pcnn_reserve(h, h->aux_ws, (size_t)N * cap * sizeof(double), 0, who)) return rc;
  double* part = static_cast<double*>(h->aux_ws.p);
  hipLaunchKernelGGL((varcoef_apply_kernel<BC, RX>), vc_tile_grid(N, u), dim3(FLUX_THREADS), 0, h->stream, H, W, cap, mask, rho, dx, p, q, part, reaction);
  hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, tiles, cap, part, pq, 1, 0, 0, 0.0, (int*)nullptr);
  PCNN_CHECK_LAUNCH(h, who);
  return 0;
}

template <bool BC, bool SC, bool RX = false>
static int vc_setup(pcnn_handle h, const char* who, int N, int H, int W, int mask, const float* rho, const float* rhs, const float* left, const float* right,
                    const float* bottom, const float* top, const float* dx, const double* x0, double tol, const VcBasis& B, void* workspace,
                    size_t workspace_bytes, double* scal, int* flags, const float* reaction = nullptr) {
  static_assert(!(RX && SC), "the scaled preconditioner has no reaction variant");
  PCNN_REQUIRE(h, h && rho && rhs && left && right && bottom && top && dx && B.Vinv_h && B.V_h && B.lam_h && B.VinvT_w && B.VT_w && B.lam_w && workspace && scal &&
                      flags && (!RX || reaction), "%s: null argument", who);
  FdUnknowns u;
  if (int rc = vc_check_shape(h, who, N, H, W, mask, &u)) return rc;
  PCNN_REQUIRE(h, tol > 0.0, "%s: tol must be positive", who);
  const VcWs w = vc_layout(workspace, N, u.mh, u.mw);
  PCNN_REQUIRE(h, workspace_bytes >= vc_bytes(N, u.mh, u.mw, SC, RX), "%s: workspace of %zu B, %zu B needed", who, workspace_bytes, vc_bytes(N, u.mh, u.mw, SC, RX));
  const int tiles = vc_tiles(u.mh, u.mw);
  const int64_t per = (int64_t)u.mh * u.mw;
  const int eb = vc_ew_blocks(per);
  const bool singular = BC && mask == 15 && !RX;             // (with a reaction term mask 15 is definite: no projection)
  double* part_rr = w.part + (size_t)N * w.cap;
  if (hipMemsetAsync(flags, 0, (size_t)N * sizeof(int), h->stream) != hipSuccess ||
      hipMemsetAsync(scal, 0, (size_t)N * (VS_STRIDE + (RX ? VX_STRIDE : 0)) * sizeof(double), h->stream) != hipSuccess)
    PCNN_FAIL(h, "%s: cannot clear the per-sample state", who);
  double* const sc = SC ? w.s : (double*)nullptr;
  double* const part3 = RX ? w.s : (double*)nullptr;
  const VcReaction rx = {reaction, 1.0 / (((double)u.mh - 0.5 * ((mask & 1) + ((mask >> 1) & 1))) * ((double)u.mw - 0.5 * (((mask >> 2) & 1) + ((mask >> 3) & 1))))};
  hipLaunchKernelGGL((varcoef_setup_kernel<BC, SC, RX>), vc_tile_grid(N, u), dim3(FLUX_THREADS), 0, h->stream, H, W, w.cap, N, mask, rho, rhs, left, right, bottom, top,
                     dx, x0, w.x, w.r, singular ? w.q : (double*)nullptr, w.part, sc, SC ? w.z : (double*)nullptr, rx, part3);
  if (RX) {
    double* extra = scal + (size_t)N * VS_STRIDE;
    hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, tiles, w.cap, part3, extra, (int)VX_STRIDE, (int)VX_CBAR, 0, 0.0, (int*)nullptr);
    hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, tiles, w.cap, part3 + (size_t)N * w.cap, extra, (int)VX_STRIDE, (int)VX_BBAR, 0,
                       0.0, (int*)nullptr);
    hipLaunchKernelGGL(varcoef_reduce_kernel<1>, dim3(N), dim3(EW_THREADS), 0, h->stream, tiles, w.cap, part3 + (size_t)2 * N * w.cap, extra, (int)VX_STRIDE, (int)VX_CMIN,
                       0, 0.0, (int*)nullptr);
  }
  int bb_count = tiles;
  if (singular) {            // sum w b^2 and sum w b of the b as given, then the projection: b.b and r.r are the projected fields'
    const double sum_w = (double)(H - 1) * (double)(W - 1);
    hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, tiles, w.cap, w.part, scal, (int)VS_STRIDE, (int)VS_BBRAW, 0, 0.0, (int*)nullptr);
    hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, tiles, w.cap, part_rr, scal, (int)VS_STRIDE, (int)VS_WB, 0, 0.0, (int*)nullptr);
    hipLaunchKernelGGL(varcoef_project_kernel<SC>, dim3(eb, N), dim3(EW_THREADS), 0, h->stream, u.mh, u.mw, w.cap, N, sum_w, scal, w.q, w.r, w.part, (const double*)sc,
                       SC ? w.z : (double*)nullptr);
    bb_count = eb;
  }
  hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, bb_count, w.cap, w.part, scal, (int)VS_STRIDE, (int)VS_BB, 0, 0.0, (int*)nullptr);
  hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, bb_count, w.cap, part_rr, scal, (int)VS_STRIDE, (int)VS_RR, 1, tol * tol, flags);
  hipLaunchKernelGGL(varcoef_reduce_kernel<1>, dim3(N), dim3(EW_THREADS), 0, h->stream, tiles, w.cap, w.part + (size_t)2 * N * w.cap, scal, (int)VS_STRIDE,
                     (int)VS_RHOMIN, 0, 0.0, (int*)nullptr);
  PCNN_CHECK_LAUNCH(h, who);
  if (int rc = vc_precondition<BC, SC, RX>(h, N, u, w, B, scal, VS_RZ0, dx)) return rc;
  hipLaunchKernelGGL(varcoef_update_p_kernel<SC>, dim3(eb, N), dim3(EW_THREADS), 0, h->stream, per, 1, 1, scal, flags, w.z, w.p, (const double*)sc);
  PCNN_CHECK_LAUNCH(h, who);
  return 0;
}

template <bool BC, bool SC, bool RX = false>
static int vc_iterate(pcnn_handle h, const char* who, int N, int H, int W, int mask, const float* rho, const float* dx, double tol, int first_iteration,
                      int iterations, const VcBasis& B, void* workspace, size_t workspace_bytes, double* scal, int* flags, const float* reaction = nullptr) {
  PCNN_REQUIRE(h, h && rho && dx && B.Vinv_h && B.V_h && B.lam_h && B.VinvT_w && B.VT_w && B.lam_w && workspace && scal && flags && (!RX || reaction),
               "%s: null argument", who);
  FdUnknowns u;
  if (int rc = vc_check_shape(h, who, N, H, W, mask, &u)) return rc;
  PCNN_REQUIRE(h, tol > 0.0 && first_iteration >= 0 && iterations >= 1, "%s: bad tol or iteration range", who);
  const VcWs w = vc_layout(workspace, N, u.mh, u.mw);
  PCNN_REQUIRE(h, workspace_bytes >= vc_bytes(N, u.mh, u.mw, SC, RX), "%s: workspace of %zu B, %zu B needed", who, workspace_bytes, vc_bytes(N, u.mh, u.mw, SC, RX));
  const int tiles = vc_tiles(u.mh, u.mw);
  const int64_t per = (int64_t)u.mh * u.mw;
  const int eb = vc_ew_blocks(per);
  double* const sc = SC ? w.s : (double*)nullptr;
  for (int it = first_iteration; it < first_iteration + iterations; ++it) {
    const int cur = it & 1;                      // r.z of the current direction sits in slot VS_RZ0 + cur, the next one goes to the other slot
    hipLaunchKernelGGL((varcoef_apply_kernel<BC, RX>), vc_tile_grid(N, u), dim3(FLUX_THREADS), 0, h->stream, H, W, w.cap, mask, rho, dx, w.p, w.q, w.part, reaction);
    hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, tiles, w.cap, w.part, scal, (int)VS_STRIDE, (int)VS_PQ, 0, 0.0, (int*)nullptr);
    hipLaunchKernelGGL((varcoef_update_xr_kernel<BC, SC>), dim3(eb, N), dim3(EW_THREADS), 0, h->stream, per, u.mh, u.mw, mask, w.cap, cur, scal, flags, w.p, w.q, w.x,
                       w.r, w.part, (const double*)sc, SC ? w.z : (double*)nullptr);
    hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, eb, w.cap, w.part, scal, (int)VS_STRIDE, (int)VS_RR, 1, tol * tol, flags);
    PCNN_CHECK_LAUNCH(h, who);
    if (int rc = vc_precondition<BC, SC, RX>(h, N, u, w, B, scal, VS_RZ0 + (cur ^ 1), dx)) return rc;
    hipLaunchKernelGGL(varcoef_update_p_kernel<SC>, dim3(eb, N), dim3(EW_THREADS), 0, h->stream, per, cur, 0, scal, flags, w.z, w.p, (const double*)sc);
    PCNN_CHECK_LAUNCH(h, who);
  }
  return 0;
}

// soln: the unknowns from x, the Dirichlet ring from the boundary arrays, as every FD solve here writes it.  mask 15: x first loses its w-mean
// (keep_mean: not so - the reaction family's mask 15 is nonsingular).
static int vc_finish(pcnn_handle h, const char* who, int N, int H, int W, int mask, void* workspace, const float* left, const float* right, const float* bottom,
                     const float* top, float* soln, bool keep_mean = false) {
  PCNN_REQUIRE(h, h && workspace && left && right && bottom && top && soln, "%s: null argument", who);
  FdUnknowns u;
  if (int rc = vc_check_shape(h, who, N, H, W, mask, &u)) return rc;
  const VcWs w = vc_layout(workspace, N, u.mh, u.mw);
  if (mask == 15 && !keep_mean) {
    const int eb = vc_ew_blocks((int64_t)u.mh * u.mw);
    const double sum_w = (double)(H - 1) * (double)(W - 1);
    double* mean = w.part + (size_t)N * w.cap;     // the second partial-sum array: N doubles are enough
    hipLaunchKernelGGL(varcoef_mean_kernel, dim3(eb, N), dim3(EW_THREADS), 0, h->stream, u.mh, u.mw, w.cap, sum_w, (const double*)nullptr, w.x, w.part);
    hipLaunchKernelGGL(varcoef_reduce_kernel<0>, dim3(N), dim3(EW_THREADS), 0, h->stream, eb, w.cap, w.part, mean, 1, 0, 0, 0.0, (int*)nullptr);
    hipLaunchKernelGGL(varcoef_mean_kernel, dim3(eb, N), dim3(EW_THREADS), 0, h->stream, u.mh, u.mw, w.cap, sum_w, (const double*)mean, w.x, w.part);
  }
  pcnn_fd_write_soln(h, N, H, W, mask, w.x, left, right, bottom, top, soln);
  PCNN_CHECK_LAUNCH(h, who);
  return 0;
}

}  // namespace

extern "C" int pcnn_varcoef_apply(pcnn_handle h, int N, int H, int W, const float* rho, const float* dx, const double* p, double* q, double* pq) {
  return vc_apply<false>(h, "pcnn_varcoef_apply", N, H, W, 0, rho, dx, p, q, pq);
}

extern "C" size_t pcnn_varcoef_pcg_workspace(int N, int H, int W) {
  if (N < 1 || H < 3 || W < 3) return 0;
  return vc_bytes(N, H - 2, W - 2);
}

extern "C" int pcnn_varcoef_pcg_setup(pcnn_handle h, int N, int H, int W, const float* rho, const float* rhs, const float* left, const float* right,
                                      const float* bottom, const float* top, const float* dx, const double* x0, double tol, const double* S_h,
                                      const double* lam_h, const double* S_w, const double* lam_w, void* workspace, size_t workspace_bytes, double* scal,
                                      int* flags) {
  return vc_setup<false, false>(h, "pcnn_varcoef_pcg_setup", N, H, W, 0, rho, rhs, left, right, bottom, top, dx, x0, tol, VcBasis{S_h, S_h, lam_h, S_w, S_w, lam_w}, workspace,
                         workspace_bytes, scal, flags);
}

extern "C" int pcnn_varcoef_pcg_iterate(pcnn_handle h, int N, int H, int W, const float* rho, const float* dx, double tol, int first_iteration, int iterations,
                                        const double* S_h, const double* lam_h, const double* S_w, const double* lam_w, void* workspace, size_t workspace_bytes,
                                        double* scal, int* flags) {
  return vc_iterate<false, false>(h, "pcnn_varcoef_pcg_iterate", N, H, W, 0, rho, dx, tol, first_iteration, iterations, VcBasis{S_h, S_h, lam_h, S_w, S_w, lam_w}, workspace,
                           workspace_bytes, scal, flags);
}

extern "C" int pcnn_varcoef_pcg_finish(pcnn_handle h, int N, int H, int W, const void* workspace, const float* left, const float* right, const float* bottom,
                                       const float* top, float* soln) {
  return vc_finish(h, "pcnn_varcoef_pcg_finish", N, H, W, 0, const_cast<void*>(workspace), left, right, bottom, top, soln);     // mask 0 only reads it
}

extern "C" int pcnn_varcoef_bc_apply(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, const double* p, double* q,
                                     double* pq) {
  return vc_apply<true>(h, "pcnn_varcoef_bc_apply", N, H, W, neumann_mask, rho, dx, p, q, pq);
}

extern "C" size_t pcnn_varcoef_bc_pcg_workspace(int N, int H, int W, int neumann_mask) {
  if (N < 1 || H < 3 || W < 3 || neumann_mask < 0 || neumann_mask > 15) return 0;
  const FdUnknowns u = fd_unknowns(H, W, neumann_mask);
  return vc_bytes(N, u.mh, u.mw);
}

extern "C" int pcnn_varcoef_bc_pcg_setup(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* rhs, const float* left,
                                         const float* right, const float* bottom, const float* top, const float* dx, const double* x0, double tol,
                                         const double* Vinv_h, const double* V_h, const double* lam_h, const double* VinvT_w, const double* VT_w,
                                         const double* lam_w, void* workspace, size_t workspace_bytes, double* scal, int* flags) {
  return vc_setup<true, false>(h, "pcnn_varcoef_bc_pcg_setup", N, H, W, neumann_mask, rho, rhs, left, right, bottom, top, dx, x0, tol,
                        VcBasis{Vinv_h, V_h, lam_h, VinvT_w, VT_w, lam_w}, workspace, workspace_bytes, scal, flags);
}

extern "C" int pcnn_varcoef_bc_pcg_iterate(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, double tol, int first_iteration,
                                           int iterations, const double* Vinv_h, const double* V_h, const double* lam_h, const double* VinvT_w,
                                           const double* VT_w, const double* lam_w, void* workspace, size_t workspace_bytes, double* scal, int* flags) {
  return vc_iterate<true, false>(h, "pcnn_varcoef_bc_pcg_iterate", N, H, W, neumann_mask, rho, dx, tol, first_iteration, iterations,
                          VcBasis{Vinv_h, V_h, lam_h, VinvT_w, VT_w, lam_w}, workspace, workspace_bytes, scal, flags);
}

extern "C" int pcnn_varcoef_bc_pcg_finish(pcnn_handle h, int N, int H, int W, int neumann_mask, void* workspace, const float* left, const float* right,
                                          const float* bottom, const float* top, float* soln) {
  return vc_finish(h, "pcnn_varcoef_bc_pcg_finish", N, H, W, neumann_mask, workspace, left, right, bottom, top, soln);
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

extern "C" int pcnn_varcoef_series_pair(pcnn_handle h, int N, int H, int W, int ka, int kb, const float* coef, int neumann_mask, const float* rho,
                                        const float* dx, float* soln, float* rhs) {
  const char* who = "pcnn_varcoef_series_pair";
  PCNN_REQUIRE(h, h && coef && rho && dx && soln && rhs, "%s: null argument", who);
  FdUnknowns u;
  if (int rc = vc_check_shape(h, who, N, H, W, neumann_mask, &u)) return rc;
  PCNN_REQUIRE(h, pcnn_cdiv(H, FLUX_ROWS) <= 65535, "%s: grid %d x %d unsupported", who, H, W);             // the tiles cover the nodes, not the unknowns
  PCNN_REQUIRE(h, ka >= 1 && kb >= 1 && ka <= VSER_MAXK && kb <= VSER_MAXK, "%s: %dx%d coefficients unsupported (<=%d)", who, ka, kb, VSER_MAXK);
  hipLaunchKernelGGL(varcoef_series_pair_kernel, dim3(pcnn_cdiv(W, FLUX_COLS), pcnn_cdiv(H, FLUX_ROWS), N), dim3(FLUX_THREADS), 0, h->stream, H, W, ka, kb,
                     neumann_mask, coef, rho, dx, soln, rhs);
  PCNN_CHECK_LAUNCH(h, who);
  return 0;
}

// ---- the diagonally scaled preconditioner: the SC = true instantiations; finish is the plain entry points'
extern "C" size_t pcnn_varcoef_pcg_workspace_scaled(int N, int H, int W) {
  if (N < 1 || H < 3 || W < 3) return 0;
  return vc_bytes(N, H - 2, W - 2, true);
}

extern "C" int pcnn_varcoef_pcg_setup_scaled(pcnn_handle h, int N, int H, int W, const float* rho, const float* rhs, const float* left, const float* right,
                                             const float* bottom, const float* top, const float* dx, const double* x0, double tol, const double* S_h,
                                             const double* lam_h, const double* S_w, const double* lam_w, void* workspace, size_t workspace_bytes, double* scal,
                                             int* flags) {
  return vc_setup<false, true>(h, "pcnn_varcoef_pcg_setup_scaled", N, H, W, 0, rho, rhs, left, right, bottom, top, dx, x0, tol, VcBasis{S_h, S_h, lam_h, S_w, S_w, lam_w},
                               workspace, workspace_bytes, scal, flags);
}

extern "C" int pcnn_varcoef_pcg_iterate_scaled(pcnn_handle h, int N, int H, int W, const float* rho, const float* dx, double tol, int first_iteration, int iterations,
                                               const double* S_h, const double* lam_h, const double* S_w, const double* lam_w, void* workspace,
                                               size_t workspace_bytes, double* scal, int* flags) {
  return vc_iterate<false, true>(h, "pcnn_varcoef_pcg_iterate_scaled", N, H, W, 0, rho, dx, tol, first_iteration, iterations, VcBasis{S_h, S_h, lam_h, S_w, S_w, lam_w},
                                 workspace, workspace_bytes, scal, flags);
}

extern "C" size_t pcnn_varcoef_bc_pcg_workspace_scaled(int N, int H, int W, int neumann_mask) {
  if (N < 1 || H < 3 || W < 3 || neumann_mask < 0 || neumann_mask > 15) return 0;
  const FdUnknowns u = fd_unknowns(H, W, neumann_mask);
  return vc_bytes(N, u.mh, u.mw, true);
}

extern "C" int pcnn_varcoef_bc_pcg_setup_scaled(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* rhs, const float* left,
                                                const float* right, const float* bottom, const float* top, const float* dx, const double* x0, double tol,
                                                const double* Vinv_h, const double* V_h, const double* lam_h, const double* VinvT_w, const double* VT_w,
                                                const double* lam_w, void* workspace, size_t workspace_bytes, double* scal, int* flags) {
  return vc_setup<true, true>(h, "pcnn_varcoef_bc_pcg_setup_scaled", N, H, W, neumann_mask, rho, rhs, left, right, bottom, top, dx, x0, tol,
                              VcBasis{Vinv_h, V_h, lam_h, VinvT_w, VT_w, lam_w}, workspace, workspace_bytes, scal, flags);
}

extern "C" int pcnn_varcoef_bc_pcg_iterate_scaled(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, double tol,
                                                  int first_iteration, int iterations, const double* Vinv_h, const double* V_h, const double* lam_h,
                                                  const double* VinvT_w, const double* VT_w, const double* lam_w, void* workspace, size_t workspace_bytes,
                                                  double* scal, int* flags) {
  return vc_iterate<true, true>(h, "pcnn_varcoef_bc_pcg_iterate_scaled", N, H, W, neumann_mask, rho, dx, tol, first_iteration, iterations,
                                VcBasis{Vinv_h, V_h, lam_h, VinvT_w, VT_w, lam_w}, workspace, workspace_bytes, scal, flags);
}

extern "C" int pcnn_varcoef_density_smooth(pcnn_handle h, int N, int64_t per, float lo, float hi, float* g) {
  PCNN_REQUIRE(h, h && g && N >= 1 && N <= 65535 && per >= 1, "pcnn_varcoef_density_smooth: bad argument");
  PCNN_REQUIRE(h, lo > 0.f && hi >= lo, "pcnn_varcoef_density_smooth: need 0 < lo <= hi, got %g, %g", (double)lo, (double)hi);
  int64_t blocks = pcnn_cdiv64(per, EW_POINTS);
  if (blocks > DS_MAX_BLOCKS) blocks = DS_MAX_BLOCKS;
  if (int rc = pcnn_reserve(h, h->aux_ws, (size_t)N * blocks * 2 * sizeof(float), 0, "pcnn_varcoef_density_smooth")) return rc;
  float* mm = static_cast<float*>(h->aux_ws.p);
  hipLaunchKernelGGL(varcoef_density_range_kernel, dim3((unsigned)blocks, N), dim3(EW_THREADS), 0, h->stream, per, (const float*)g, mm);
  hipLaunchKernelGGL(varcoef_density_smooth_kernel, dim3((unsigned)blocks, N), dim3(EW_THREADS), 0, h->stream, per, lo, hi, (const float*)mm, g);
  PCNN_CHECK_LAUNCH(h, "pcnn_varcoef_density_smooth");
  return 0;
}

// ---- the reaction term: the RX = true instantiations of the *_bc_* family
extern "C" int pcnn_varcoef_bc_apply_reaction(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, const double* p, double* q,
                                              double* pq, const float* reaction) {
  return vc_apply<true, true>(h, "pcnn_varcoef_bc_apply_reaction", N, H, W, neumann_mask, rho, dx, p, q, pq, reaction);
}

extern "C" size_t pcnn_varcoef_bc_pcg_workspace_reaction(int N, int H, int W, int neumann_mask) {
  if (N < 1 || H < 3 || W < 3 || neumann_mask < 0 || neumann_mask > 15) return 0;
  const FdUnknowns u = fd_unknowns(H, W, neumann_mask);
  return vc_bytes(N, u.mh, u.mw, false, true);
}

extern "C" int pcnn_varcoef_bc_pcg_setup_reaction(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* rhs, const float* left,
                                                  const float* right, const float* bottom, const float* top, const float* dx, const double* x0, double tol,
                                                  const double* Vinv_h, const double* V_h, const double* lam_h, const double* VinvT_w, const double* VT_w,
                                                  const double* lam_w, void* workspace, size_t workspace_bytes, double* scal, int* flags, const float* reaction) {
  return vc_setup<true, false, true>(h, "pcnn_varcoef_bc_pcg_setup_reaction", N, H, W, neumann_mask, rho, rhs, left, right, bottom, top, dx, x0, tol,
                                     VcBasis{Vinv_h, V_h, lam_h, VinvT_w, VT_w, lam_w}, workspace, workspace_bytes, scal, flags, reaction);
}

extern "C" int pcnn_varcoef_bc_pcg_iterate_reaction(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, double tol,
                                                    int first_iteration, int iterations, const double* Vinv_h, const double* V_h, const double* lam_h,
                                                    const double* VinvT_w, const double* VT_w, const double* lam_w, void* workspace, size_t workspace_bytes,
                                                    double* scal, int* flags, const float* reaction) {
  return vc_iterate<true, false, true>(h, "pcnn_varcoef_bc_pcg_iterate_reaction", N, H, W, neumann_mask, rho, dx, tol, first_iteration, iterations,
                                       VcBasis{Vinv_h, V_h, lam_h, VinvT_w, VT_w, lam_w}, workspace, workspace_bytes, scal, flags, reaction);
}

extern "C" int pcnn_varcoef_bc_pcg_finish_reaction(pcnn_handle h, int N, int H, int W, int neumann_mask, void* workspace, const float* left, const float* right,
                                                   const float* bottom, const float* top, float* soln) {
  return vc_finish(h, "pcnn_varcoef_bc_pcg_finish_reaction", N, H, W, neumann_mask, workspace, left, right, bottom, top, soln, true);
}

extern "C" int pcnn_varcoef_reaction_field(pcnn_handle h, int64_t total, float lo, float hi, float* g) {
  PCNN_REQUIRE(h, h && g && total >= 1, "pcnn_varcoef_reaction_field: bad argument");
  PCNN_REQUIRE(h, lo >= 0.f && hi >= lo && hi < INFINITY, "pcnn_varcoef_reaction_field: need 0 <= lo <= hi, got %g, %g", (double)lo, (double)hi);
  int64_t blocks = pcnn_cdiv64(total, 256);
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(varcoef_density_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, total, lo, hi, g);
  PCNN_CHECK_LAUNCH(h, "pcnn_varcoef_reaction_field");
  return 0;
}
