// Per-sample error statistics of a prediction in one pass over pred, target and rhs (evaluate / predict / validation, DESIGN.md section 14;
// model.solve of the variable-density problem, section 18; the opt-in residual metrics of the variable-density model, section 21):
// out[n] = {sum|e|, sum e^2, max|e|, sum t^2, max|t|, sum r^2, max|r|, sum f^2}, e = pred - target, t = target over all H W points;
// r = the residual of pred against rhs, f = rhs over the (H-2)(W-2) interior points.  One kernel, three residuals:
//   pcnn_error_stats:          the 3 x 3 second-order FD Laplacian of pred minus rhs, one spacing per sample and axis (FivePoint);
//   pcnn_varcoef_error_stats:  the flux-form operator of div((1/rho) grad u) = f applied to pred, minus rhs (FluxForm: pcnn_flux_residual of
//                              flux_form.h, the one the training loss uses).  The prediction's own edge values act as the Dirichlet neighbours of r.
//                              Only with zero (homogeneous) edge values is sum r^2 / sum f^2 the ||b - A x||^2 / ||b||^2 of the conjugate-gradient
//                              solve: with other edge values b holds the boundary terms and sum f^2 is not ||b||^2.
//   pcnn_varcoef_bc_error_stats:  that residual over the unknowns fd_unknowns(H, W, neumann_mask) - a Neumann edge's nodes included, their outward
//                              neighbour read at the mirrored index, so the inward face counts twice (du/dn = 0, the closure of section 20) - and
//                              the two sums weighted by w = vc_weight: sum w r^2, max|r|, sum w f^2 (FluxFormBC).  Mask 0 gives the bits of
//                              pcnn_varcoef_error_stats.
// No atomics, a fixed order everywhere: equal inputs give equal bits.
#include "flux_form.h"

namespace {

constexpr int ES_STATS = 8;
constexpr int ES_BANDS = 64;     // workgroups per sample = lanes of the combining wave
constexpr int ES_WAVES = 16;     // waves per workgroup: one image row per wave at a time

// sums where `mx` is false, maxima where it is true, over the 64 lanes of a wave in a fixed butterfly order
__device__ __forceinline__ float es_wave_reduce(float v, bool mx) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const float o = __shfl_xor(v, m);
    v = mx ? fmaxf(v, o) : v + o;
  }
  return v;
}

__device__ __forceinline__ bool es_is_max(int k) { return k == 2 || k == 4 || k == 6; }

// The residual r at an interior point, built per sample from (n, H, W, pointers); dx is null where rhs is not given, and then neither dx nor rho
// is read.  at(row, x, p, f): row = y W, p = pred there, f = rhs there.
struct FivePoint {                                 // dx (N, 2): column 0 the H axis
  static constexpr bool uses_rho = false, per_edge = false;
  const float* pn;
  int W;
  float ay = 0.f, ax = 0.f;
  __device__ __forceinline__ FivePoint(int n, int H, int W_, const float* pn_, const float* rho, const float* dx, int) : pn(pn_), W(W_) {
    if (dx) { ay = 1.0f / (dx[2 * n] * dx[2 * n]); ax = 1.0f / (dx[2 * n + 1] * dx[2 * n + 1]); }
  }
  __device__ __forceinline__ float at(int64_t row, int x, float p, float f) const {
    return (pn[row - W + x] - 2.0f * p + pn[row + W + x]) * ay + (pn[row + x - 1] - 2.0f * p + pn[row + x + 1]) * ax - f;
  }
};
struct FluxForm {                                  // dx (N,): dy = dx; rho is read here alone: with rhs, on interior points and their neighbours
  static constexpr bool uses_rho = true, per_edge = false;
  const float* pn;
  const float* dn;
  int W;
  float inv_h2 = 0.f;
  __device__ __forceinline__ FluxForm(int n, int H, int W_, const float* pn_, const float* rho, const float* dx, int)
      : pn(pn_), dn(dx ? rho + (int64_t)n * H * W_ : nullptr), W(W_) {
    if (dx) inv_h2 = 1.0f / (dx[n] * dx[n]);
  }
  __device__ __forceinline__ float at(int64_t row, int x, float p, float f) const {
    return pcnn_flux_residual(p, dn[row + x], pn[row - W + x], dn[row - W + x], pn[row + W + x], dn[row + W + x], pn[row + x - 1], dn[row + x - 1],
                              pn[row + x + 1], dn[row + x + 1], inv_h2, f);
  }
};
// FluxForm over the unknowns of a Neumann mask, which is uniform per launch, so everything an edge changes is a scalar.  set_row(y), once per row
// and wave, says whether the row holds unknowns and fixes the two rows its neighbours are read from (vc_mirror: beyond a Neumann edge the inward
// row a second time) and the row's weight.  Of a wave's column strides only the first and the last hold column 0 / W - 1: the kernel asks `ends`
// there alone, and flux(row, x, xl, xr, ...) is one code path (two paths cost two more registers and the second workgroup of a CU).
struct FluxFormBC {
  static constexpr bool uses_rho = true, per_edge = true;
  const float* pn;
  const float* dn;
  int H, W, mask;
  FdUnknowns un;
  float inv_h2 = 0.f;
  int64_t up = 0, dw = 0;                          // y' W of the rows towards i - 1 / i + 1 of the current row
  float wy = 1.f;
  __device__ __forceinline__ FluxFormBC(int n, int H_, int W_, const float* pn_, const float* rho, const float* dx, int mask_)
      : pn(pn_), dn(dx ? rho + (int64_t)n * H_ * W_ : nullptr), H(H_), W(W_), mask(mask_), un(fd_unknowns(H_, W_, mask_)) {
    if (dx) inv_h2 = 1.0f / (dx[n] * dx[n]);
  }
  __device__ __forceinline__ bool set_row(int y) {                  // y: the same in every lane of the wave
    if (y < un.i0 || y > un.i1) return false;
    up = (int64_t)vc_mirror(y - 1, H, mask & 1, mask & 2) * W;
    dw = (int64_t)vc_mirror(y + 1, H, mask & 1, mask & 2) * W;
    wy = (y == 0 || y == H - 1) ? 0.5f : 1.f;                       // row 0 / H - 1 holds unknowns only as a Neumann edge
    return true;
  }
  __device__ __forceinline__ float flux(int64_t row, int x, int xl, int xr, float p, float f) const {
    return pcnn_flux_residual(p, dn[row + x], pn[up + x], dn[up + x], pn[dw + x], dn[dw + x], pn[row + xl], dn[row + xl], pn[row + xr], dn[row + xr],
                              inv_h2, f);
  }
  // The first and last column stride: false where column x holds no unknown; at column 0 / W - 1 - an unknown only as a Neumann edge - the
  // neighbour beyond the edge becomes the mirrored column (vc_mirror(-1) = 1, vc_mirror(W) = W - 2) and the weight halves.
  __device__ __forceinline__ bool ends(int x, int* xl, int* xr, float* w) const {
    if (x < un.j0 || x > un.j1) return false;
    if (x == 0) { *xl = 1; *w = 0.5f * wy; }
    if (x == W - 1) { *xr = W - 2; *w = 0.5f * wy; }
    return true;
  }
};

// grid (ES_BANDS, N): workgroup (b, n) owns rows [b rpb, (b + 1) rpb) of sample n, rpb = ceil(H / ES_BANDS).  Wave w takes the band's rows w, w + 16,
// ...; its lanes stride over the columns, so every load of a row is one coalesced request.  The residual's neighbours are plain loads of the rows
// above and below: inside a band they hit the lines the neighbouring wave just fetched, across a band edge they come from L2.  A neighbour is
// loaded only for 0 < y < H - 1 and 0 < x < W - 1, so every index stays inside sample n.  Residual::per_edge: only at an unknown, the neighbour
// beyond a Neumann edge at its mirrored index (inside the field: H, W >= 3), and s_r2 / s_f2 take w r^2 / w f^2 - w = 1 exactly under mask 0, so
// that mask adds what FluxForm adds, in its order.  `mask` is read by that residual alone.
template <class Residual>
__global__ __launch_bounds__(ES_WAVES * 64) void stats_partials_kernel(int H, int W, const float* __restrict__ pred, const float* __restrict__ tgt,
                                                                       const float* __restrict__ rho, const float* __restrict__ rhs,
                                                                       const float* __restrict__ dx, float* __restrict__ part, int mask) {
  __shared__ float red[ES_WAVES][ES_STATS];
  const int n = blockIdx.y, b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int rpb = (H + ES_BANDS - 1) / ES_BANDS;
  const int y0 = b * rpb < H ? b * rpb : H, y1 = y0 + rpb < H ? y0 + rpb : H;
  const int64_t base = (int64_t)n * H * W;
  const float* pn = pred + base;
  const float* tn = tgt ? tgt + base : nullptr;
  const float* fn = rhs ? rhs + base : nullptr;
  Residual res(n, H, W, pn, rho, fn ? dx : nullptr, mask);
  float s_ae = 0.f, s_e2 = 0.f, m_e = 0.f, s_t2 = 0.f, m_t = 0.f, s_r2 = 0.f, m_r = 0.f, s_f2 = 0.f;
  if constexpr (Residual::per_edge) {
    const int klast = (W - 1) >> 6;                                 // the column stride that holds column W - 1; stride 0 holds column 0
    for (int y = y0 + wv; y < y1; y += ES_WAVES) {
      const int64_t row = (int64_t)y * W;
      const bool yin = fn && res.set_row(__builtin_amdgcn_readfirstlane(y));
      for (int x = lane, k = 0; x < W; x += 64, ++k) {
        const float p = pn[row + x];
        if (tn) {
          const float t = tn[row + x], e = p - t;
          s_ae += fabsf(e); s_e2 += e * e; m_e = fmaxf(m_e, fabsf(e));
          s_t2 += t * t; m_t = fmaxf(m_t, fabsf(t));
        }
        if (!yin) continue;
        int xl = x - 1, xr = x + 1;
        float w = res.wy;
        if ((k == 0 || k == klast) && !res.ends(x, &xl, &xr, &w)) continue;      // a scalar test: the strides between see no edge
        const float f = fn[row + x], r = res.flux(row, x, xl, xr, p, f);
        s_r2 += w * (r * r); m_r = fmaxf(m_r, fabsf(r)); s_f2 += w * (f * f);
      }
    }
  } else {
    for (int y = y0 + wv; y < y1; y += ES_WAVES) {
      const int64_t row = (int64_t)y * W;
      const bool yin = fn && y > 0 && y < H - 1;
      for (int x = lane; x < W; x += 64) {
        const float p = pn[row + x];
        if (tn) {
          const float t = tn[row + x], e = p - t;
          s_ae += fabsf(e); s_e2 += e * e; m_e = fmaxf(m_e, fabsf(e));
          s_t2 += t * t; m_t = fmaxf(m_t, fabsf(t));
        }
        if (yin && x > 0 && x < W - 1) {
          const float f = fn[row + x], r = res.at(row, x, p, f);
          s_r2 += r * r; m_r = fmaxf(m_r, fabsf(r)); s_f2 += f * f;
        }
      }
    }
  }
  float v[ES_STATS] = {s_ae, s_e2, m_e, s_t2, m_t, s_r2, m_r, s_f2};
#pragma unroll
  for (int k = 0; k < ES_STATS; ++k) v[k] = es_wave_reduce(v[k], es_is_max(k));
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < ES_STATS; ++k) red[wv][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < ES_STATS) {
    const int k = threadIdx.x;
    float a = red[0][k];
    for (int w = 1; w < ES_WAVES; ++w) a = es_is_max(k) ? fmaxf(a, red[w][k]) : a + red[w][k];
    part[((int64_t)n * ES_BANDS + b) * ES_STATS + k] = a;
  }
}

// one wave per sample: lane b holds band b's partials, the same butterfly combines them
__global__ __launch_bounds__(64) void stats_final_kernel(const float* __restrict__ part, float* __restrict__ out) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const float* p = part + ((int64_t)n * ES_BANDS + lane) * ES_STATS;
#pragma unroll
  for (int k = 0; k < ES_STATS; ++k) {
    const float v = es_wave_reduce(p[k], es_is_max(k));
    if (lane == 0) out[(int64_t)n * ES_STATS + k] = v;
  }
}

// the argument checks (each in the caller's name) and the two launches of the three entry points
template <class Residual>
int stats_launch(pcnn_handle h, const char* who, int N, int H, int W, int mask, const float* pred, const float* target, const float* rho, const float* rhs,
                 const float* dx, float* out) {
  PCNN_REQUIRE(h, h && pred && out, "%s: null argument", who);
  PCNN_REQUIRE(h, N >= 1 && N <= 65535 && H >= 1 && W >= 1, "%s: bad shape %d x %d x %d (1 <= N <= 65535)", who, N, H, W);
  PCNN_REQUIRE(h, mask >= 0 && mask <= 15, "%s: neumann_mask %d not in 0..15", who, mask);
  PCNN_REQUIRE(h, !Residual::uses_rho || !rhs || rho, "%s: rhs needs rho", who);
  PCNN_REQUIRE(h, !rhs || dx, "%s: rhs needs dx", who);
  PCNN_REQUIRE(h, !rhs || (H >= 3 && W >= 3), "%s: the residual needs H, W >= 3 (got %d x %d)", who, H, W);
  static_assert(ES_BANDS == 64, "stats_final_kernel combines one band per lane of a wave");
  const size_t need = (size_t)N * ES_BANDS * ES_STATS * sizeof(float);
  if (pcnn_reserve(h, h->scratch, need, PCNN_SCRATCH_FLOOR, who)) return 1;
  float* part = static_cast<float*>(h->scratch.p);
  hipLaunchKernelGGL(stats_partials_kernel<Residual>, dim3(ES_BANDS, N), dim3(ES_WAVES * 64), 0, h->stream, H, W, pred, target, rho, rhs, dx, part, mask);
  hipLaunchKernelGGL(stats_final_kernel, dim3(N), dim3(64), 0, h->stream, part, out);
  PCNN_CHECK_LAUNCH(h, who);
  return 0;
}

}  // namespace

extern "C" int pcnn_error_stats(pcnn_handle h, int N, int H, int W, const float* pred, const float* target, const float* rhs, const float* dx, float* out) {
  return stats_launch<FivePoint>(h, "pcnn_error_stats", N, H, W, 0, pred, target, nullptr, rhs, dx, out);
}

extern "C" int pcnn_varcoef_error_stats(pcnn_handle h, int N, int H, int W, const float* pred, const float* target, const float* rho, const float* rhs,
                                        const float* dx, float* out) {
  return stats_launch<FluxForm>(h, "pcnn_varcoef_error_stats", N, H, W, 0, pred, target, rho, rhs, dx, out);
}

extern "C" int pcnn_varcoef_bc_error_stats(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* pred, const float* target, const float* rho,
                                           const float* rhs, const float* dx, float* out) {
  return stats_launch<FluxFormBC>(h, "pcnn_varcoef_bc_error_stats", N, H, W, neumann_mask, pred, target, rho, rhs, dx, out);
}
