// Per-sample error statistics of a prediction of the variable-density problem div((1/rho) grad u) = f in one pass over pred, target, rho and rhs
// (model.solve).  out[n] has the layout of pcnn_error_stats:
//   {sum|e|, sum e^2, max|e|, sum t^2, max|t|, sum r^2, max|r|, sum f^2},   e = pred - target, t = target over all H W points;
//   r = the flux-form operator of section 16 applied to pred itself, minus rhs, f = rhs over the (H-2)(W-2) interior points.
// The prediction's own edge values act as the Dirichlet neighbours of r.  Only with zero (homogeneous) edge values is sum r^2 / sum f^2 the
// ||b - A x||^2 / ||b||^2 of the conjugate-gradient solve: with other edge values b holds the boundary terms and sum f^2 is not ||b||^2.
// Operation order of one r, all in fp32, no contraction (uc, rc: the node's pred and rho; index 0..3: the neighbours towards i-1, i+1, j-1, j+1):
//   b_k = 2 / (rc + r_k),  d_k = u_k - uc,  s = (b_0 d_0 + b_1 d_1) + (b_2 d_2 + b_3 d_3),  r = s * (1 / (dx dx)) - f
// which is the flux_residual of varcoef_train.hip restated (that file's kernels keep their own copy, so their bits cannot move).
// The band layout and the reduction tree are those of error_stats.hip: no atomics, a fixed order everywhere, equal inputs give equal bits.
#include "pcnn_internal.h"

namespace {

constexpr int VS_STATS = 8;
constexpr int VS_BANDS = 64;     // workgroups per sample = lanes of the combining wave
constexpr int VS_WAVES = 16;     // waves per workgroup: one image row per wave at a time

// sums where `mx` is false, maxima where it is true, over the 64 lanes of a wave in a fixed butterfly order
__device__ __forceinline__ float vs_wave_reduce(float v, bool mx) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const float o = __shfl_xor(v, m);
    v = mx ? fmaxf(v, o) : v + o;
  }
  return v;
}

__device__ __forceinline__ bool vs_is_max(int k) { return k == 2 || k == 4 || k == 6; }

// grid (VS_BANDS, N): workgroup (b, n) owns rows [b rpb, (b + 1) rpb) of sample n, rpb = ceil(H / VS_BANDS).  Wave w takes the band's rows w, w + 16,
// ...; its lanes stride over the columns, so every load of a row is one coalesced request.  The neighbours of pred and rho are plain loads of the
// rows above and below: inside a band they hit the lines the neighbouring wave just fetched, across a band edge they come from L2.  A neighbour is
// loaded only for 0 < y < H - 1 and 0 < x < W - 1, so every index stays inside sample n; rho is read only there and only with rhs.
__global__ __launch_bounds__(VS_WAVES * 64) void varcoef_stats_partials_kernel(int H, int W, const float* __restrict__ pred, const float* __restrict__ tgt,
                                                                               const float* __restrict__ rho, const float* __restrict__ rhs,
                                                                               const float* __restrict__ dx, float* __restrict__ part) {
  __shared__ float red[VS_WAVES][VS_STATS];
  const int n = blockIdx.y, b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int rpb = (H + VS_BANDS - 1) / VS_BANDS;
  const int y0 = b * rpb < H ? b * rpb : H, y1 = y0 + rpb < H ? y0 + rpb : H;
  const int64_t base = (int64_t)n * H * W;
  const float* pn = pred + base;
  const float* tn = tgt ? tgt + base : nullptr;
  const float* fn = rhs ? rhs + base : nullptr;
  const float* dn = rhs ? rho + base : nullptr;
  float inv_h2 = 0.f;
  if (fn) inv_h2 = 1.0f / (dx[n] * dx[n]);
  float s_ae = 0.f, s_e2 = 0.f, m_e = 0.f, s_t2 = 0.f, m_t = 0.f, s_r2 = 0.f, m_r = 0.f, s_f2 = 0.f;
  for (int y = y0 + wv; y < y1; y += VS_WAVES) {
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
        const float f = fn[row + x], rc = dn[row + x];
        const float b0 = 2.f / (rc + dn[row - W + x]), b1 = 2.f / (rc + dn[row + W + x]);
        const float b2 = 2.f / (rc + dn[row + x - 1]), b3 = 2.f / (rc + dn[row + x + 1]);
        const float s = (b0 * (pn[row - W + x] - p) + b1 * (pn[row + W + x] - p)) + (b2 * (pn[row + x - 1] - p) + b3 * (pn[row + x + 1] - p));
        const float r = s * inv_h2 - f;
        s_r2 += r * r; m_r = fmaxf(m_r, fabsf(r)); s_f2 += f * f;
      }
    }
  }
  float v[VS_STATS] = {s_ae, s_e2, m_e, s_t2, m_t, s_r2, m_r, s_f2};
#pragma unroll
  for (int k = 0; k < VS_STATS; ++k) v[k] = vs_wave_reduce(v[k], vs_is_max(k));
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < VS_STATS; ++k) red[wv][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < VS_STATS) {
    const int k = threadIdx.x;
    float a = red[0][k];
    for (int w = 1; w < VS_WAVES; ++w) a = vs_is_max(k) ? fmaxf(a, red[w][k]) : a + red[w][k];
    part[((int64_t)n * VS_BANDS + b) * VS_STATS + k] = a;
  }
}

// one wave per sample: lane b holds band b's partials, the same butterfly combines them
__global__ __launch_bounds__(64) void varcoef_stats_final_kernel(const float* __restrict__ part, float* __restrict__ out) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const float* p = part + ((int64_t)n * VS_BANDS + lane) * VS_STATS;
#pragma unroll
  for (int k = 0; k < VS_STATS; ++k) {
    const float v = vs_wave_reduce(p[k], vs_is_max(k));
    if (lane == 0) out[(int64_t)n * VS_STATS + k] = v;
  }
}

}  // namespace

extern "C" int pcnn_varcoef_error_stats(pcnn_handle h, int N, int H, int W, const float* pred, const float* target, const float* rho, const float* rhs,
                                        const float* dx, float* out) {
  PCNN_REQUIRE(h, h && pred && out, "pcnn_varcoef_error_stats: null argument");
  PCNN_REQUIRE(h, N >= 1 && N <= 65535 && H >= 1 && W >= 1, "pcnn_varcoef_error_stats: bad shape %d x %d x %d (1 <= N <= 65535)", N, H, W);
  PCNN_REQUIRE(h, !rhs || rho, "pcnn_varcoef_error_stats: rhs needs rho");
  PCNN_REQUIRE(h, !rhs || dx, "pcnn_varcoef_error_stats: rhs needs dx");
  PCNN_REQUIRE(h, !rhs || (H >= 3 && W >= 3), "pcnn_varcoef_error_stats: the residual needs H, W >= 3 (got %d x %d)", H, W);
  static_assert(VS_BANDS == 64, "varcoef_stats_final_kernel combines one band per lane of a wave");
  const size_t need = (size_t)N * VS_BANDS * VS_STATS * sizeof(float);
  if (pcnn_reserve(h, h->scratch, need, PCNN_SCRATCH_FLOOR, "pcnn_varcoef_error_stats")) return 1;
  float* part = static_cast<float*>(h->scratch.p);
  hipLaunchKernelGGL(varcoef_stats_partials_kernel, dim3(VS_BANDS, N), dim3(VS_WAVES * 64), 0, h->stream, H, W, pred, target, rho, rhs, dx, part);
  hipLaunchKernelGGL(varcoef_stats_final_kernel, dim3(N), dim3(64), 0, h->stream, part, out);
  PCNN_CHECK_LAUNCH(h, "pcnn_varcoef_error_stats");
  return 0;
}
