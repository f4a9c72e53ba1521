// Training-side operators of the variable-density problem div((1/rho) grad u) = f (DESIGN.md sections 17 and 20): the flux-form residual loss with
// its gradient, and the Jacobi sweep of the same operator with its adjoint - w.r.t. u (fused), and w.r.t. u, rho and rhs (section 25).  fp32 on one-channel (N,H,W) fields, one spacing per sample (dy = dx),
// rho on every node.  The discretisation is that of csrc/varcoef.hip (section 16), held once in flux_form.h (pcnn_beta_face, pcnn_flux_residual, the
// FLUX_ROWS x FLUX_COLS tile of the loss kernels - that of varcoef_apply_kernel - and its LDS loader pcnn_load_nodes):
//   beta_face = 2 / (rho_a + rho_b),   (L u)[i,j] = sum over the four faces of beta_face (u[neighbour] - u[i,j]) / dx^2 = -(A u)[i,j]
// on the (H-2) x (W-2) interior nodes; here the ring of u is part of the field (the model predicts it), so L maps all H W nodes to the interior.
// The face coefficients are never stored: every kernel builds them from an LDS tile of rho.  No atomics: the loss sums are per-tile partials
// (fixed tree) added per sample by a second one-block stage in a fixed order.  A sample's blocks read nothing of another sample.
// The sweeps' walker, tile frame, launch chain and launch checks are sweep_common.h's, shared with stencil.hip.
// Per-edge Neumann boundaries (the *_bc_* entry points, BC = true; section 20): the unknowns are fd_unknowns(H, W, neumann_mask), a Neumann edge's
// nodes included.  Such a node has no outward neighbour; u and rho are read with the mirrored index there (vc_mirror of flux_form.h, or the
// mirrored LDS offset of the sweeps), which makes the inward face of that direction count twice - the closure of varcoef.hip with g = 0.  The loss
// weights every unknown by w = w_i w_j, 1/2 on a Neumann edge's row (vc_weight): W L is symmetric on the unknowns, so the gradient stays a
// gather.  BC = false is the all-Dirichlet code with its operation order; neumann_mask 0 runs it.
#include <math.h>
#include "flux_form.h"
#include "sweep_common.h"

#define VJ_TILE 64         // output tile edge of the sweeps
#define VJ_HALO_MAX 8      // fused sweeps per launch: four LDS buffers of at most (64 + 2 * 8 + 2)^2 floats (107.6 KB)
#define VJ_THREADS 512

namespace {

constexpr int RED_THREADS = 256;

// the unknowns of a kernel: the interior (BC = false), or those of the mask
template <bool BC>
__device__ __forceinline__ FdUnknowns vt_unknowns(int H, int W, int mask) { return fd_unknowns(H, W, BC ? mask : 0); }

// part[n][tile] = the tile's sum of (L pred - rhs)^2 (BC: of w (L pred - rhs)^2).  grid (column tiles, row tiles, N) over the unknowns
template <bool BC>
__global__ __launch_bounds__(FLUX_THREADS) void vc_pi_partials_kernel(int H, int W, int tiles, int mask, const float* __restrict__ pred,
                                                                      const float* __restrict__ rho, const float* __restrict__ rhs,
                                                                      const float* __restrict__ dx, float* __restrict__ part) {
  constexpr int LR = FLUX_ROWS + 2, LC = FLUX_COLS + 2;
  __shared__ float us[LR][LC];
  __shared__ float rs[LR][LC];
  __shared__ float red[FLUX_THREADS];
  const FdUnknowns un = vt_unknowns<BC>(H, W, mask);
  const int nh = un.mh, nw = un.mw, n = blockIdx.z, I0 = blockIdx.y * FLUX_ROWS, J0 = blockIdx.x * FLUX_COLS;
  const int Y0 = un.i0 + I0 - 1, X0 = un.j0 + J0 - 1;                  // LDS (r, c) is node (Y0 + r, X0 + c); unknown (I0 + r, J0 + c) sits at (r + 1, c + 1)
  const int64_t img = (int64_t)n * H * W;
  if (BC) {
    pcnn_load_nodes_mirrored<LR, LC>(us, pred + img, H, W, Y0, X0, mask, 0.f);
    pcnn_load_nodes_mirrored<LR, LC>(rs, rho + img, H, W, Y0, X0, mask, 1.f);
  } else {
    pcnn_load_nodes<LR, LC>(us, pred + img, H, W, Y0, X0, 0.f);
    pcnn_load_nodes<LR, LC>(rs, rho + img, H, W, Y0, X0, 1.f);
  }
  __syncthreads();
  const float h = dx[n], inv_h2 = 1.f / (h * h);
  const int c = threadIdx.x % FLUX_COLS, r0 = (threadIdx.x / FLUX_COLS) * FLUX_RPT;
  float s = 0.f;
  if (J0 + c < nw) {
#pragma unroll
    for (int k = 0; k < FLUX_RPT; ++k) {
      const int r = r0 + k;
      if (I0 + r < nh) {
        const int a = r + 1, b = c + 1;
        const float e = pcnn_flux_residual(us[a][b], rs[a][b], us[a - 1][b], rs[a - 1][b], us[a + 1][b], rs[a + 1][b], us[a][b - 1], rs[a][b - 1],
                                           us[a][b + 1], rs[a][b + 1], inv_h2, rhs[img + (int64_t)(Y0 + a) * W + X0 + b]);
        s += BC ? (float)vc_weight(I0 + r, J0 + c, nh, nw, mask) * (e * e) : e * e;
      }
    }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  pcnn_block_sum<float, FLUX_THREADS>(red, threadIdx.x);
  if (threadIdx.x == 0) part[(int64_t)n * tiles + blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// out[n] = the sample's partials added in a fixed order (in fp64: the second stage costs nothing and adds no rounding of its own)
__global__ __launch_bounds__(RED_THREADS) void vc_pi_reduce_kernel(int tiles, const float* __restrict__ part, float* __restrict__ out) {
  __shared__ double red[RED_THREADS];
  const int n = blockIdx.x, t = threadIdx.x;
  double v = 0.0;
  for (int k = t; k < tiles; k += RED_THREADS) v += (double)part[(int64_t)n * tiles + k];
  red[t] = v;
  __syncthreads();
  pcnn_block_sum<double, RED_THREADS>(red, t);
  if (t == 0) out[n] = (float)red[0];
}

// dpred += coef[n] * 2 L^T e, e = L pred - rhs.  Gather form: e on the tile's nodes and a one-node halo (zero outside the interior), then
// (L^T e)[p] = sum over the faces of p of beta_face (e[neighbour] - e[p]) / dx^2 - the operator is symmetric, and on a ring node, where e[p] = 0,
// the same expression is the sum of beta_face e[interior neighbour].  grid (column tiles, row tiles, N) over ALL nodes
// BC: dpred += coef[n] * 2 L^T (w .* e).  e is held on the unknowns, zero on Dirichlet nodes and - beyond a Neumann edge - as its mirror image.
// w_c L_cp = w_p L_pc between unknowns, so at an unknown p the sum is w_p times the same expression (the mirrored e and rho double the inward face);
// at a Dirichlet node, which is nobody's doubled neighbour, it is the sum of beta_face w_c e_c over the unknown neighbours c.
template <bool BC>
__global__ __launch_bounds__(FLUX_THREADS) void vc_pi_bwd_kernel(int H, int W, int mask, const float* __restrict__ pred, const float* __restrict__ rho,
                                                                 const float* __restrict__ rhs, const float* __restrict__ dx, const float* __restrict__ coef,
                                                                 float* __restrict__ dpred) {
  constexpr int LR = FLUX_ROWS + 4, LC = FLUX_COLS + 4, ER = FLUX_ROWS + 2, EC = FLUX_COLS + 2;
  __shared__ float us[LR][LC];
  __shared__ float rs[LR][LC];
  __shared__ float es[ER][EC];
  const FdUnknowns un = vt_unknowns<BC>(H, W, mask);
  const int n = blockIdx.z, I0 = blockIdx.y * FLUX_ROWS, J0 = blockIdx.x * FLUX_COLS;     // us / rs (r, c) is node (I0 - 2 + r, J0 - 2 + c); es: (I0 - 1 + r, J0 - 1 + c)
  const int64_t img = (int64_t)n * H * W;
  if (BC) {
    pcnn_load_nodes_mirrored<LR, LC>(us, pred + img, H, W, I0 - 2, J0 - 2, mask, 0.f);
    pcnn_load_nodes_mirrored<LR, LC>(rs, rho + img, H, W, I0 - 2, J0 - 2, mask, 1.f);
  } else {
    pcnn_load_nodes<LR, LC>(us, pred + img, H, W, I0 - 2, J0 - 2, 0.f);
    pcnn_load_nodes<LR, LC>(rs, rho + img, H, W, I0 - 2, J0 - 2, 1.f);
  }
  __syncthreads();
  const float h = dx[n], inv_h2 = 1.f / (h * h);
  pcnn_flux_residual_halo<BC, ER, EC, LC>(es, us, rs, rhs + img, H, W, I0, J0, mask, un, inv_h2, [](float v, int, int) { return v; });
  __syncthreads();
  const float scale = 2.f * coef[n] * inv_h2;
  const int c = threadIdx.x % FLUX_COLS, r0 = (threadIdx.x / FLUX_COLS) * FLUX_RPT;
  if (J0 + c < W) {
#pragma unroll
    for (int k = 0; k < FLUX_RPT; ++k) {
      const int r = r0 + k;
      if (I0 + r < H) {
        const int a = r + 1, b = c + 1;                  // in es; rs is one further in
        const float ec = es[a][b], rc = rs[a + 1][b + 1];
        const float b0 = pcnn_beta_face(rc, rs[a][b + 1]), b1 = pcnn_beta_face(rc, rs[a + 2][b + 1]), b2 = pcnn_beta_face(rc, rs[a + 1][b]),
                    b3 = pcnn_beta_face(rc, rs[a + 1][b + 2]);
        float g;
        if (BC) {
          const int ii = I0 + r - un.i0, jj = J0 + c - un.j0;                         // as an unknown
          if (ii >= 0 && ii < un.mh && jj >= 0 && jj < un.mw) {
            g = (float)vc_weight(ii, jj, un.mh, un.mw, mask) * ((b0 * (es[a - 1][b] - ec) + b1 * (es[a + 1][b] - ec)) + (b2 * (es[a][b - 1] - ec) + b3 * (es[a][b + 1] - ec)));
          } else {                                                                  // a Dirichlet node: e is zero on it, on its edge and beyond it
            const float w0 = (float)vc_weight(ii - 1, jj, un.mh, un.mw, mask), w1 = (float)vc_weight(ii + 1, jj, un.mh, un.mw, mask);
            const float w2 = (float)vc_weight(ii, jj - 1, un.mh, un.mw, mask), w3 = (float)vc_weight(ii, jj + 1, un.mh, un.mw, mask);
            g = (b0 * (w0 * es[a - 1][b]) + b1 * (w1 * es[a + 1][b])) + (b2 * (w2 * es[a][b - 1]) + b3 * (w3 * es[a][b + 1]));
          }
        } else {
          g = (b0 * (es[a - 1][b] - ec) + b1 * (es[a + 1][b] - ec)) + (b2 * (es[a][b - 1] - ec) + b3 * (es[a][b + 1] - ec));
        }
        dpred[img + (int64_t)(I0 + r) * W + J0 + c] += scale * g;
      }
    }
  }
}

// k sweeps in one launch by temporal blocking (DESIGN.md sections 11 and 17).  A workgroup owns a VJ_TILE^2 tile of one sample; after k sweeps the
// tile depends on u within k nodes of it, clipped to the image where the frozen ring ends the dependence.  Sweep s of k computes the tile grown by
// k - s nodes, ping-ponging between two LDS buffers; the last one stores the tile.  The arithmetic of a point does not depend on k or on the tile,
// so any split of n sweeps into launches gives the same bits.
//   BWD == false: u -> out; fb holds dx^2 rhs.
//   BWD == true:  u is d(out), out is d(u); fb holds 1 / (sum of the node's four face coefficients) on interior nodes - the adjoint's gather
//                 needs the diagonal of its NEIGHBOURS, so rho is held one node further out than u.
//   BC: the unknowns are computed instead of the interior; a Neumann edge node reads its inward neighbour in place of the missing outward one (the LDS
//       offset is mirrored; the neighbour lies in the clipped region of the sweep before, as any neighbour does), so its diagonal holds that face
//       twice, and the adjoint's gather takes a Neumann edge node's share twice at its inward neighbour.
template <bool BWD, bool BC>
__global__ __launch_bounds__(VJ_THREADS) void vc_jacobi_kernel(int H, int W, int k, int mask, const float* __restrict__ rho, const float* __restrict__ u,
                                                               const float* __restrict__ rhs, const float* __restrict__ dx, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int n = blockIdx.z, tid = threadIdx.x, g0 = k + (BWD ? 1 : 0);
  const FdUnknowns un = vt_unknowns<BC>(H, W, mask);
  pcnn_frame<VJ_TILE> f(H, W);
  int y0, y1, x0, x1;
  f.grow(g0, g0, y0, y1, x0, x1);                                     // the LDS frame: the tile grown by g0 nodes, clipped to the image
  f.hold(y0, y1, x0, x1);
  const int LW = f.LW;
  const int S = (VJ_TILE + 2 * g0) * (VJ_TILE + 2 * g0);              // floats per buffer as the host sized them
  float* src = lds;
  float* dst = lds + S;
  float* fb = lds + 2 * S;
  float* rb = lds + 3 * S;
  const int64_t img = (int64_t)n * H * W;
  const float h = dx[n], h2 = h * h;
  auto unknown = [&](int y, int x) { return y >= un.i0 && y <= un.i1 && x >= un.j0 && x <= un.j1; };
  // LDS offsets of the neighbours towards y-1, y+1, x-1, x+1 of the unknown at offset c; BC: mirrored where the image ends (a Neumann edge node)
  auto up = [&](int c, int y) { return (BC && y == 0) ? c + LW : c - LW; };
  auto down = [&](int c, int y) { return (BC && y == H - 1) ? c - LW : c + LW; };
  auto left = [&](int c, int x) { return (BC && x == 0) ? c + 1 : c - 1; };
  auto right = [&](int c, int x) { return (BC && x == W - 1) ? c - 1 : c + 1; };

  pcnn_for_points<VJ_THREADS>(tid, y0, x0, y1 - y0, LW, [&](int y, int x) { rb[f.at(y, x)] = rho[img + (int64_t)y * W + x]; });
  {
    f.grow(k, k, y0, y1, x0, x1);
    pcnn_for_points<VJ_THREADS>(tid, y0, x0, y1 - y0, x1 - x0, [&](int y, int x) { src[f.at(y, x)] = u[img + (int64_t)y * W + x]; });
    if (BWD) {
      __syncthreads();
      pcnn_for_points<VJ_THREADS>(tid, y0, x0, y1 - y0, x1 - x0, [&](int y, int x) {
        const int c = f.at(y, x);
        float v = 0.f;
        if (unknown(y, x)) {
          const float rc = rb[c];
          v = 1.f / ((pcnn_beta_face(rc, rb[up(c, y)]) + pcnn_beta_face(rc, rb[down(c, y)])) +
                     (pcnn_beta_face(rc, rb[left(c, x)]) + pcnn_beta_face(rc, rb[right(c, x)])));
        }
        fb[c] = v;
      });
    } else {
      f.grow(k - 1, k - 1, y0, y1, x0, x1);
      pcnn_for_points<VJ_THREADS>(tid, y0, x0, y1 - y0, x1 - x0, [&](int y, int x) { fb[f.at(y, x)] = h2 * rhs[img + (int64_t)y * W + x]; });
    }
  }
  __syncthreads();

  auto point = [&](const float* in, int c, int y, int x) -> float {
    const bool interior = unknown(y, x);
    const float rc = rb[c];
    if (!BWD) {
      if (!interior) return in[c];
      const int cu = up(c, y), cd = down(c, y), cl = left(c, x), cr = right(c, x);
      const float b0 = pcnn_beta_face(rc, rb[cu]), b1 = pcnn_beta_face(rc, rb[cd]), b2 = pcnn_beta_face(rc, rb[cl]), b3 = pcnn_beta_face(rc, rb[cr]);
      const float num = (b0 * in[cu] + b1 * in[cd]) + (b2 * in[cl] + b3 * in[cr]);
      return (num - fb[c]) / ((b0 + b1) + (b2 + b3));
    }
    // adjoint: gather from the unknown neighbours p, each of which read this node with weight beta_face / diagonal(p) - twice where p is a Neumann
    // edge node and this node its inward neighbour (p then sits on row 0 / H-1 or column 0 / W-1 of the image)
    const bool in_x = x >= un.j0 && x <= un.j1, in_y = y >= un.i0 && y <= un.i1;
    float acc = 0.f;
    if (in_x) {
      if (y - 1 >= un.i0 && y - 1 <= un.i1) acc += ((BC && y - 1 == 0) ? 2.f : 1.f) * (pcnn_beta_face(rc, rb[c - LW]) * (fb[c - LW] * in[c - LW]));
      if (y + 1 >= un.i0 && y + 1 <= un.i1) acc += ((BC && y + 1 == H - 1) ? 2.f : 1.f) * (pcnn_beta_face(rc, rb[c + LW]) * (fb[c + LW] * in[c + LW]));
    }
    if (in_y) {
      if (x - 1 >= un.j0 && x - 1 <= un.j1) acc += ((BC && x - 1 == 0) ? 2.f : 1.f) * (pcnn_beta_face(rc, rb[c - 1]) * (fb[c - 1] * in[c - 1]));
      if (x + 1 >= un.j0 && x + 1 <= un.j1) acc += ((BC && x + 1 == W - 1) ? 2.f : 1.f) * (pcnn_beta_face(rc, rb[c + 1]) * (fb[c + 1] * in[c + 1]));
    }
    return (interior ? 0.f : in[c]) + acc;
  };

  for (int s = 1; s <= k; ++s) {
    f.grow(k - s, k - s, y0, y1, x0, x1);
    pcnn_for_points<VJ_THREADS>(tid, y0, x0, y1 - y0, x1 - x0, [&](int y, int x) {
      const int c = f.at(y, x);
      const float v = point(src, c, y, x);
      if (s == k) out[img + (int64_t)y * W + x] = v;
      else dst[c] = v;
    });
    __syncthreads();
    float* t = src; src = dst; dst = t;
  }
}

template <bool BWD, bool BC>
int vj_launch(pcnn_handle_s* h, int N, int H, int W, int k, int mask, const float* rho, const float* u, const float* rhs, const float* dx, float* out) {
  const dim3 grid((unsigned)pcnn_cdiv(W, VJ_TILE), (unsigned)pcnn_cdiv(H, VJ_TILE), (unsigned)N);
  const int e = VJ_TILE + 2 * (k + (BWD ? 1 : 0));
  const size_t lds = (size_t)4 * e * e * sizeof(float);
  PCNN_REQUIRE_LDS(h, lds, "pcnn_varcoef_jacobi: %zu bytes of LDS for %d fused sweeps", lds, k);
  pcnn_launch_lds(h, vc_jacobi_kernel<BWD, BC>, grid, VJ_THREADS, lds, H, W, k, mask, rho, u, rhs, dx, out);
  return 0;
}

// One sweep of the smoother's backward with the gradients of its DATA.  The sweep took u (iterate t) to un (iterate t + 1);
// gin is d loss / d un.  With a_c = gin_c / D_c on the unknowns (D_c = sum_k m_k beta_k) and 0 on every other node:
//   gout_k  = sum over the unknown neighbours c of k of m beta a_c  (+ gin_k on a frozen node)      - the arithmetic of vc_jacobi_kernel<true, .>
//   drhs_c += -h^2 a_c
//   drho_p += -1/2 (a_p sum_k beta_k^2 (u_k - un_p)  +  sum over the unknown neighbours c of p of m beta^2 a_c (u_p - un_c))
// the first sum over the four (mirrored: a Neumann edge node's inward face twice) faces of p if p is an unknown, the second p's share of the faces
// its neighbours read it through.  A gather on the flux_form.h tile: grid (column tiles, row tiles, N) over ALL nodes, one thread per output, no
// atomics.  a is formed as (1 / D) * gin and gout summed in the order of vc_jacobi_kernel's adjoint, so gout has its bits.  first: drho / drhs are
// written instead of added to (the last sweep comes first).  gout, drho, drhs may each be NULL.
__global__ __launch_bounds__(FLUX_THREADS) void vc_jacobi_bwd_inputs_kernel(int H, int W, int mask, int first, const float* __restrict__ rho,
                                                                            const float* __restrict__ u, const float* __restrict__ un,
                                                                            const float* __restrict__ gin, const float* __restrict__ dx,
                                                                            float* __restrict__ gout, float* __restrict__ drho, float* __restrict__ drhs) {
  constexpr int LR = FLUX_ROWS + 4, LC = FLUX_COLS + 4, ER = FLUX_ROWS + 2, EC = FLUX_COLS + 2;
  __shared__ float rs[LR][LC];                            // rho: (r, c) is node (I0 - 2 + r, J0 - 2 + c), mirrored beyond a Neumann edge
  __shared__ float us[ER][EC];                            // u, mirrored: (r, c) is node (I0 - 1 + r, J0 - 1 + c), as are ns and as
  __shared__ float ns[ER][EC];                            // un, read on unknowns only
  __shared__ float as[ER][EC];                            // a
  const FdUnknowns uk = fd_unknowns(H, W, mask);
  const int n = blockIdx.z, I0 = blockIdx.y * FLUX_ROWS, J0 = blockIdx.x * FLUX_COLS;
  const int64_t img = (int64_t)n * H * W;
  pcnn_load_nodes_mirrored<LR, LC>(rs, rho + img, H, W, I0 - 2, J0 - 2, mask, 1.f);
  pcnn_load_nodes_mirrored<ER, EC>(us, u + img, H, W, I0 - 1, J0 - 1, mask, 0.f);
  pcnn_load_nodes<ER, EC>(ns, un + img, H, W, I0 - 1, J0 - 1, 0.f);
  __syncthreads();
  for (int e = threadIdx.x; e < ER * EC; e += FLUX_THREADS) {
    const int r = e / EC, c = e % EC, i = I0 - 1 + r, j = J0 - 1 + c;
    float v = 0.f;
    if (i >= uk.i0 && i <= uk.i1 && j >= uk.j0 && j <= uk.j1) {
      const int a = r + 1, b = c + 1;
      const float rc = rs[a][b];
      const float inv_d = 1.f / ((pcnn_beta_face(rc, rs[a - 1][b]) + pcnn_beta_face(rc, rs[a + 1][b])) +
                                 (pcnn_beta_face(rc, rs[a][b - 1]) + pcnn_beta_face(rc, rs[a][b + 1])));
      v = inv_d * gin[img + (int64_t)i * W + j];
    }
    as[r][c] = v;
  }
  __syncthreads();
  const float h = dx[n], h2 = h * h;
  const int c = threadIdx.x % FLUX_COLS, r0 = (threadIdx.x / FLUX_COLS) * FLUX_RPT;
  const int j = J0 + c;
  if (j >= W) return;
  const bool in_x = j >= uk.j0 && j <= uk.j1;
  const bool has_l = j - 1 >= uk.j0 && j - 1 <= uk.j1, has_r = j + 1 >= uk.j0 && j + 1 <= uk.j1;      // the neighbour's column holds unknowns
  const float ml = (mask && j - 1 == 0) ? 2.f : 1.f, mr = (mask && j + 1 == W - 1) ? 2.f : 1.f;       // ... on a Neumann edge: it reads this node twice
#pragma unroll
  for (int k = 0; k < FLUX_RPT; ++k) {
    const int r = r0 + k, i = I0 + r;
    if (i >= H) break;
    const int a = r + 1, b = c + 1;                       // in us / ns / as; rs is one further in
    const int64_t at = img + (int64_t)i * W + j;
    const bool in_y = i >= uk.i0 && i <= uk.i1, unknown = in_x && in_y;
    const bool has_u = in_x && i - 1 >= uk.i0 && i - 1 <= uk.i1, has_d = in_x && i + 1 >= uk.i0 && i + 1 <= uk.i1;
    const float mu = (mask && i - 1 == 0) ? 2.f : 1.f, md = (mask && i + 1 == H - 1) ? 2.f : 1.f;
    const float rc = rs[a + 1][b + 1];
    const float b0 = pcnn_beta_face(rc, rs[a][b + 1]), b1 = pcnn_beta_face(rc, rs[a + 2][b + 1]), b2 = pcnn_beta_face(rc, rs[a + 1][b]),
                b3 = pcnn_beta_face(rc, rs[a + 1][b + 2]);
    if (gout) {
      float acc = 0.f;
      if (has_u) acc += mu * (b0 * as[a - 1][b]);
      if (has_d) acc += md * (b1 * as[a + 1][b]);
      if (in_y && has_l) acc += ml * (b2 * as[a][b - 1]);
      if (in_y && has_r) acc += mr * (b3 * as[a][b + 1]);
      gout[at] = (unknown ? 0.f : gin[at]) + acc;
    }
    const float ac = as[a][b];
    if (drhs) {
      const float v = unknown ? -(h2 * ac) : 0.f;
      drhs[at] = first ? v : drhs[at] + v;
    }
    if (drho) {
      const float up = us[a][b];
      float own = 0.f, shared = 0.f;
      if (unknown) {
        const float q = ns[a][b];
        own = ac * (((b0 * b0) * (us[a - 1][b] - q) + (b1 * b1) * (us[a + 1][b] - q)) + ((b2 * b2) * (us[a][b - 1] - q) + (b3 * b3) * (us[a][b + 1] - q)));
      }
      if (has_u) shared += mu * ((b0 * b0) * (as[a - 1][b] * (up - ns[a - 1][b])));
      if (has_d) shared += md * ((b1 * b1) * (as[a + 1][b] * (up - ns[a + 1][b])));
      if (in_y && has_l) shared += ml * ((b2 * b2) * (as[a][b - 1] * (up - ns[a][b - 1])));
      if (in_y && has_r) shared += mr * ((b3 * b3) * (as[a][b + 1] * (up - ns[a][b + 1])));
      const float v = -0.5f * (own + shared);
      drho[at] = first ? v : drho[at] + v;
    }
  }
}

__global__ void assemble_density_input_kernel(int N, int H, int W, const float* __restrict__ stack, int use_pos, float* __restrict__ out, int ldo) {
  const int64_t hw = (int64_t)H * W, total = (int64_t)N * hw;
  const float pi = 3.14159265358979323846f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / hw, p = i - n * hw;
    const int x = p % W; const int y = p / W;
    out[i * ldo] = stack[2 * n * hw + p];
    out[i * ldo + 1] = stack[(2 * n + 1) * hw + p];
    if (use_pos) {                                       // the two channels of pcnn_assemble_input, same arithmetic
      const float ly = H > 1 ? (float)y * (1.0f / (float)(H - 1)) : 0.f;
      const float lx = W > 1 ? (float)x * (1.0f / (float)(W - 1)) : 0.f;
      out[i * ldo + 2] = cosf(pi * ly);
      out[i * ldo + 3] = cosf(pi * lx);
    }
  }
}

bool vt_shape_ok(int N, int H, int W) { return pcnn_grid_ok(N, H, W) && H >= 3 && W >= 3 && pcnn_cdiv(H, FLUX_ROWS) <= 65535; }

// The bodies of the entry points: the all-Dirichlet names pass mask 0, which runs the BC = false kernels; `who` names the caller in a refusal.
int vt_pi_loss_partials(pcnn_handle h, const char* who, int N, int H, int W, int mask, const float* pred, const float* rho, const float* rhs, const float* dx,
                        float* out) {
  PCNN_REQUIRE(h, h && pred && rho && rhs && dx && out, "%s: null argument", who);
  PCNN_REQUIRE(h, mask >= 0 && mask < 16, "%s: neumann_mask %d not in 0..15", who, mask);
  PCNN_REQUIRE(h, vt_shape_ok(N, H, W), "%s: batch %d of %d x %d grids unsupported", who, N, H, W);
  const FdUnknowns un = fd_unknowns(H, W, mask);
  const dim3 grid(pcnn_cdiv(un.mw, FLUX_COLS), pcnn_cdiv(un.mh, FLUX_ROWS), N);
  const int tiles = (int)(grid.x * grid.y);
  if (int rc = pcnn_reserve(h, h->aux_ws, (size_t)N * tiles * sizeof(float), 0, who)) return rc;
  float* part = static_cast<float*>(h->aux_ws.p);
  if (mask) hipLaunchKernelGGL(vc_pi_partials_kernel<true>, grid, dim3(FLUX_THREADS), 0, h->stream, H, W, tiles, mask, pred, rho, rhs, dx, part);
  else hipLaunchKernelGGL(vc_pi_partials_kernel<false>, grid, dim3(FLUX_THREADS), 0, h->stream, H, W, tiles, 0, pred, rho, rhs, dx, part);
  hipLaunchKernelGGL(vc_pi_reduce_kernel, dim3(N), dim3(RED_THREADS), 0, h->stream, tiles, part, out);
  PCNN_CHECK_LAUNCH(h, who);
  return 0;
}

int vt_pi_loss_bwd(pcnn_handle h, const char* who, int N, int H, int W, int mask, const float* pred, const float* rho, const float* rhs, const float* dx,
                   const float* coef, float* dpred) {
  PCNN_REQUIRE(h, h && pred && rho && rhs && dx && coef && dpred, "%s: null argument", who);
  PCNN_REQUIRE(h, mask >= 0 && mask < 16, "%s: neumann_mask %d not in 0..15", who, mask);
  PCNN_REQUIRE(h, vt_shape_ok(N, H, W), "%s: batch %d of %d x %d grids unsupported", who, N, H, W);
  PCNN_REQUIRE(h, dpred != pred && dpred != rho && dpred != rhs, "%s: dpred must not alias an input", who);
  const dim3 grid(pcnn_cdiv(W, FLUX_COLS), pcnn_cdiv(H, FLUX_ROWS), N);
  if (mask) hipLaunchKernelGGL(vc_pi_bwd_kernel<true>, grid, dim3(FLUX_THREADS), 0, h->stream, H, W, mask, pred, rho, rhs, dx, coef, dpred);
  else hipLaunchKernelGGL(vc_pi_bwd_kernel<false>, grid, dim3(FLUX_THREADS), 0, h->stream, H, W, 0, pred, rho, rhs, dx, coef, dpred);
  PCNN_CHECK_LAUNCH(h, who);
  return 0;
}

int vt_jacobi_fwd(pcnn_handle h, const char* who, int N, int H, int W, int mask, const float* rho, const float* u, const float* rhs, const float* dx, int n_sweeps,
                  float* out) {
  PCNN_REQUIRE(h, h && rho && u && rhs && dx && out, "%s: null argument", who);
  PCNN_REQUIRE(h, mask >= 0 && mask < 16, "%s: neumann_mask %d not in 0..15", who, mask);
  PCNN_REQUIRE(h, vt_shape_ok(N, H, W) && n_sweeps >= 1, "%s: needs N in 1..65535, H, W >= 3, n_sweeps >= 1 (got %d, %d x %d, %d sweeps)", who, N, H, W, n_sweeps);
  PCNN_REQUIRE(h, out != u && out != rhs && out != rho, "%s: out must not alias an input", who);
  return pcnn_sweep_chain(h, who, N, H, W, n_sweeps, VJ_HALO_MAX, u, out, [&](int k, const float* in, float* to) {
    return mask ? vj_launch<false, true>(h, N, H, W, k, mask, rho, in, rhs, dx, to) : vj_launch<false, false>(h, N, H, W, k, 0, rho, in, rhs, dx, to);
  });
}

int vt_jacobi_bwd(pcnn_handle h, const char* who, int N, int H, int W, int mask, const float* rho, const float* dx, const float* dout, int n_sweeps, float* du) {
  PCNN_REQUIRE(h, h && rho && dx && dout && du, "%s: null argument", who);
  PCNN_REQUIRE(h, mask >= 0 && mask < 16, "%s: neumann_mask %d not in 0..15", who, mask);
  PCNN_REQUIRE(h, vt_shape_ok(N, H, W) && n_sweeps >= 1, "%s: needs N in 1..65535, H, W >= 3, n_sweeps >= 1 (got %d, %d x %d, %d sweeps)", who, N, H, W, n_sweeps);
  PCNN_REQUIRE(h, du != dout && du != rho, "%s: du must not alias an input", who);
  return pcnn_sweep_chain(h, who, N, H, W, n_sweeps, VJ_HALO_MAX, dout, du, [&](int k, const float* in, float* to) {
    return mask ? vj_launch<true, true>(h, N, H, W, k, mask, rho, in, nullptr, dx, to) : vj_launch<true, false>(h, N, H, W, k, 0, rho, in, nullptr, dx, to);
  });
}

// fields of N H W floats the backward below keeps in the handle's auxiliary scratch: the n iterates u^1 .. u^n and two gradients in turn
size_t vt_bwd_inputs_fields(int n_sweeps) { return (size_t)n_sweeps + 2; }

// The backward of n sweeps w.r.t. u0, rho and rhs.  Sweep t needs the iterates u^t and u^(t+1): they are recomputed with the forward's own kernel, one
// sweep per launch, into the scratch (n fields), then the sweeps are walked backwards with one vc_jacobi_bwd_inputs_kernel launch each.
int vt_jacobi_bwd_inputs(pcnn_handle h, const char* who, int N, int H, int W, int mask, const float* rho, const float* u0, const float* rhs, const float* dx,
                         const float* dout, int n_sweeps, float* du, float* drho, float* drhs) {
  PCNN_REQUIRE(h, h && rho && u0 && rhs && dx && dout, "%s: null argument", who);
  PCNN_REQUIRE(h, mask >= 0 && mask < 16, "%s: neumann_mask %d not in 0..15", who, mask);
  PCNN_REQUIRE(h, vt_shape_ok(N, H, W) && n_sweeps >= 1, "%s: needs N in 1..65535, H, W >= 3, n_sweeps >= 1 (got %d, %d x %d, %d sweeps)", who, N, H, W, n_sweeps);
  if (!du && !drho && !drhs) return 0;
  const float* ins[] = {rho, u0, rhs, dout};
  float* outs[] = {du, drho, drhs};
  for (int o = 0; o < 3; ++o) {
    if (!outs[o]) continue;
    for (const float* in : ins) PCNN_REQUIRE(h, outs[o] != in, "%s: an output must not alias an input", who);
    for (int p = 0; p < o; ++p) PCNN_REQUIRE(h, outs[o] != outs[p], "%s: the outputs must not alias each other", who);
  }
  if (!drho && !drhs) return vt_jacobi_bwd(h, who, N, H, W, mask, rho, dx, dout, n_sweeps, du);      // u alone: the fused adjoint, which needs no iterates
  const size_t field = (size_t)N * H * W;
  if (int rc = pcnn_reserve(h, h->aux_ws, vt_bwd_inputs_fields(n_sweeps) * field * sizeof(float), 0, who)) return rc;
  float* ws = static_cast<float*>(h->aux_ws.p);
  auto iterate = [&](int t) -> const float* { return t == 0 ? u0 : ws + (size_t)(t - 1) * field; };     // u^t
  float* g[2] = {ws + (size_t)n_sweeps * field, ws + (size_t)(n_sweeps + 1) * field};
  for (int t = 0; t < n_sweeps; ++t) {
    float* to = ws + (size_t)t * field;
    if (int rc = mask ? vj_launch<false, true>(h, N, H, W, 1, mask, rho, iterate(t), rhs, dx, to) : vj_launch<false, false>(h, N, H, W, 1, 0, rho, iterate(t), rhs, dx, to))
      return rc;
  }
  const dim3 grid(pcnn_cdiv(W, FLUX_COLS), pcnn_cdiv(H, FLUX_ROWS), N);
  const float* gin = dout;
  for (int t = n_sweeps - 1; t >= 0; --t) {
    float* gout = t == 0 ? du : g[t & 1];
    hipLaunchKernelGGL(vc_jacobi_bwd_inputs_kernel, grid, dim3(FLUX_THREADS), 0, h->stream, H, W, mask, t == n_sweeps - 1 ? 1 : 0, rho, iterate(t), iterate(t + 1), gin,
                       dx, gout, drho, drhs);
    gin = gout;
  }
  PCNN_CHECK_LAUNCH(h, who);
  return 0;
}

}  // namespace

extern "C" int pcnn_varcoef_bc_jacobi_bwd_inputs(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* u0, const float* rhs,
                                                 const float* dx, const float* dout, int n_sweeps, float* du, float* drho, float* drhs) {
  return vt_jacobi_bwd_inputs(h, "pcnn_varcoef_bc_jacobi_bwd_inputs", N, H, W, neumann_mask, rho, u0, rhs, dx, dout, n_sweeps, du, drho, drhs);
}

extern "C" size_t pcnn_varcoef_jacobi_bwd_inputs_workspace(int N, int H, int W, int n_sweeps) {
  if (!vt_shape_ok(N, H, W) || n_sweeps < 1) return 0;
  return vt_bwd_inputs_fields(n_sweeps) * (size_t)N * H * W * sizeof(float);
}

extern "C" int pcnn_varcoef_pi_loss_partials(pcnn_handle h, int N, int H, int W, const float* pred, const float* rho, const float* rhs, const float* dx,
                                             float* out) {
  return vt_pi_loss_partials(h, "pcnn_varcoef_pi_loss_partials", N, H, W, 0, pred, rho, rhs, dx, out);
}

extern "C" int pcnn_varcoef_pi_loss_bwd(pcnn_handle h, int N, int H, int W, const float* pred, const float* rho, const float* rhs, const float* dx,
                                        const float* coef, float* dpred) {
  return vt_pi_loss_bwd(h, "pcnn_varcoef_pi_loss_bwd", N, H, W, 0, pred, rho, rhs, dx, coef, dpred);
}

extern "C" int pcnn_varcoef_jacobi_max_sweeps(void) { return VJ_HALO_MAX; }

extern "C" int pcnn_varcoef_jacobi_fwd(pcnn_handle h, int N, int H, int W, const float* rho, const float* u, const float* rhs, const float* dx, int n_sweeps,
                                       float* out) {
  return vt_jacobi_fwd(h, "pcnn_varcoef_jacobi_fwd", N, H, W, 0, rho, u, rhs, dx, n_sweeps, out);
}

extern "C" int pcnn_varcoef_jacobi_bwd(pcnn_handle h, int N, int H, int W, const float* rho, const float* dx, const float* dout, int n_sweeps, float* du) {
  return vt_jacobi_bwd(h, "pcnn_varcoef_jacobi_bwd", N, H, W, 0, rho, dx, dout, n_sweeps, du);
}

extern "C" int pcnn_varcoef_bc_pi_loss_partials(pcnn_handle h, int N, int H, int W, const float* pred, const float* rho, const float* rhs, const float* dx,
                                                float* out, int neumann_mask) {
  return vt_pi_loss_partials(h, "pcnn_varcoef_bc_pi_loss_partials", N, H, W, neumann_mask, pred, rho, rhs, dx, out);
}

extern "C" int pcnn_varcoef_bc_pi_loss_bwd(pcnn_handle h, int N, int H, int W, const float* pred, const float* rho, const float* rhs, const float* dx,
                                           const float* coef, float* dpred, int neumann_mask) {
  return vt_pi_loss_bwd(h, "pcnn_varcoef_bc_pi_loss_bwd", N, H, W, neumann_mask, pred, rho, rhs, dx, coef, dpred);
}

extern "C" int pcnn_varcoef_bc_jacobi_fwd(pcnn_handle h, int N, int H, int W, const float* rho, const float* u, const float* rhs, const float* dx, int n_sweeps,
                                          float* out, int neumann_mask) {
  return vt_jacobi_fwd(h, "pcnn_varcoef_bc_jacobi_fwd", N, H, W, neumann_mask, rho, u, rhs, dx, n_sweeps, out);
}

extern "C" int pcnn_varcoef_bc_jacobi_bwd(pcnn_handle h, int N, int H, int W, const float* rho, const float* dx, const float* dout, int n_sweeps, float* du,
                                          int neumann_mask) {
  return vt_jacobi_bwd(h, "pcnn_varcoef_bc_jacobi_bwd", N, H, W, neumann_mask, rho, dx, dout, n_sweeps, du);
}

extern "C" int pcnn_assemble_density_input(pcnn_handle h, int N, int H, int W, const float* stack, int use_pos, float* out, int ldo) {
  PCNN_REQUIRE(h, h && stack && out && N >= 1 && H >= 1 && W >= 1 && ldo >= (use_pos ? 4 : 2), "pcnn_assemble_density_input: bad argument");
  int64_t blocks = pcnn_cdiv64((int64_t)N * H * W, 256);
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(assemble_density_input_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, N, H, W, stack, use_pos, out, ldo);
  PCNN_CHECK_LAUNCH(h, "pcnn_assemble_density_input");
  return 0;
}
