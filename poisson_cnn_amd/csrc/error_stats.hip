// Per-sample error statistics of a prediction in one pass over pred, target and rhs (evaluate / predict / validation):
// out[n] = {sum|e|, sum e^2, max|e|, sum t^2, max|t|, sum r^2, max|r|, sum f^2}, e = pred - target, t = target over all H W points;
// r = the 3 x 3 second-order FD Laplacian of pred minus rhs, f = rhs over the (H-2)(W-2) interior points.
#include "pcnn_internal.h"

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

// grid (ES_BANDS, N): workgroup (b, n) owns rows [b rpb, (b + 1) rpb) of sample n, rpb = ceil(H / ES_BANDS).  Wave w takes the band's rows w, w + 16,
// ...; its lanes stride over the columns, so every load of a row is one coalesced request.  The stencil's neighbours are plain loads of the rows above
// and below: inside a band they hit the lines the neighbouring wave just fetched, across a band edge they come from L2.  A neighbour row is touched
// only for 0 < y < H - 1, so every index stays inside sample n.
__global__ __launch_bounds__(ES_WAVES * 64) void error_stats_partials_kernel(int H, int W, const float* __restrict__ pred, const float* __restrict__ tgt,
                                                                             const float* __restrict__ rhs, const float* __restrict__ dx,
                                                                             float* __restrict__ part) {
  __shared__ float red[ES_WAVES][ES_STATS];
  const int n = blockIdx.y, b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int rpb = (H + ES_BANDS - 1) / ES_BANDS;
  const int y0 = b * rpb < H ? b * rpb : H, y1 = y0 + rpb < H ? y0 + rpb : H;
  const int64_t base = (int64_t)n * H * W;
  const float* pn = pred + base;
  const float* tn = tgt ? tgt + base : nullptr;
  const float* fn = rhs ? rhs + base : nullptr;
  float ay = 0.f, ax = 0.f;
  if (fn) { ay = 1.0f / (dx[2 * n] * dx[2 * n]); ax = 1.0f / (dx[2 * n + 1] * dx[2 * n + 1]); }
  float s_ae = 0.f, s_e2 = 0.f, m_e = 0.f, s_t2 = 0.f, m_t = 0.f, s_r2 = 0.f, m_r = 0.f, s_f2 = 0.f;
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
        const float f = fn[row + x];
        const float r = (pn[row - W + x] - 2.0f * p + pn[row + W + x]) * ay + (pn[row + x - 1] - 2.0f * p + pn[row + x + 1]) * ax - f;
        s_r2 += r * r; m_r = fmaxf(m_r, fabsf(r)); s_f2 += f * f;
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
__global__ __launch_bounds__(64) void error_stats_final_kernel(const float* __restrict__ part, float* __restrict__ out) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const float* p = part + ((int64_t)n * ES_BANDS + lane) * ES_STATS;
#pragma unroll
  for (int k = 0; k < ES_STATS; ++k) {
    const float v = es_wave_reduce(p[k], es_is_max(k));
    if (lane == 0) out[(int64_t)n * ES_STATS + k] = v;
  }
}

}  // namespace

extern "C" int pcnn_error_stats(pcnn_handle h, int N, int H, int W, const float* pred, const float* target, const float* rhs, const float* dx, float* out) {
  PCNN_REQUIRE(h, h && pred && out, "pcnn_error_stats: null argument");
  PCNN_REQUIRE(h, N >= 1 && N <= 65535 && H >= 1 && W >= 1, "pcnn_error_stats: bad shape %d x %d x %d (1 <= N <= 65535)", N, H, W);
  PCNN_REQUIRE(h, !rhs || dx, "pcnn_error_stats: rhs needs dx");
  PCNN_REQUIRE(h, !rhs || (H >= 3 && W >= 3), "pcnn_error_stats: the residual needs H, W >= 3 (got %d x %d)", H, W);
  static_assert(ES_BANDS == 64, "error_stats_final_kernel combines one band per lane of a wave");
  const size_t need = (size_t)N * ES_BANDS * ES_STATS * sizeof(float);
  if (pcnn_reserve(h, h->scratch, need, PCNN_SCRATCH_FLOOR, "pcnn_error_stats")) return 1;
  float* part = static_cast<float*>(h->scratch.p);
  hipLaunchKernelGGL(error_stats_partials_kernel, dim3(ES_BANDS, N), dim3(ES_WAVES * 64), 0, h->stream, H, W, pred, target, rhs, dx, part);
  hipLaunchKernelGGL(error_stats_final_kernel, dim3(N), dim3(64), 0, h->stream, part, out);
  PCNN_CHECK_LAUNCH(h, "pcnn_error_stats");
  return 0;
}
