// Wide-channel convolution family (UNet baseline, models/UNet.py): SAME k x k convolutions with any channel counts, their data and filter
// gradients, and the kernel == stride transposed convolution of deconvupscale - all as implicit GEMMs on v_mfma_f32_32x32x2_f32 (exact fp32
// in every math mode).  Two engines:
//   wide_gemm_rows : C[m, n] = sum_k A[m, k] B[k, n], m = pixels of a grid, k = (tap, channel) gathered from an NHWC tensor with a
//                    stride / pad map, B = a dense filter matrix; epilogue bias / dropout / activation (forward) or act' of the producer
//                    (data gradient), store or accumulate, optional depth-to-space scatter (transposed convolution forward).
//   wide_gemm_pix  : C[m, n] = sum_p A[m, p] B[p, n], m = (tap, channel) gathered as above, p = pixels (split-K over p), B = an NHWC
//                    tensor: filter gradients.  Partials go to a workspace and are reduced in a fixed order (deterministic).
// Tiles: 256 threads = 2 x 2 waves; a wave owns TM x TN accumulators of 32 x 32 (TM = TN = 2: 128 x 128 block tile; TM = 4, TN = 1:
// 256 x 64 for narrow N).  K steps of 16 go through LDS with a one-tile register prefetch.
#include <algorithm>
#include "pcnn_internal.h"

namespace {

constexpr int KT = 16;       // K per LDS stage
constexpr int NT = 256;      // threads per workgroup

__host__ __device__ inline uint32_t fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}
// include/pcnn.h "dropout mask": keep element idx iff hash >= threshold
__device__ inline bool drop_keep(uint32_t seed, uint32_t layer, uint64_t idx, uint32_t thresh) {
  uint32_t h = fmix32(seed ^ (layer * 0x9E3779B9u));
  h = fmix32(h ^ (uint32_t)(idx >> 32));
  h = fmix32(h ^ (uint32_t)idx);
  return h >= thresh;
}

struct RowArgs {
  const float* x; int Hx, Wx, Cx, ldx;          // gathered operand: A[m, (tap, c)] = x[img, hm*stride + ty - pt, wm*stride + tx - pl, c]
  int Hm, Wm; long long M;                      // rows: the pixels of an (M / (Hm Wm)) x Hm x Wm grid
  int kh, kw, stride, pt, pl;
  const float* w; int Ncol; int transb;         // B[(tap, c), n] = w[(tap*Cx + c)*Ncol + n]; transb (one tap): w[n*Cx + c]
  const float* bias;
  float* y; int ldy;
  int scatter, Hy, Wy, Cy, spt, spl;            // scatter = f > 0: column n = (a*f + b)*Cy + co -> y[img, hm*f + a - spt, wm*f + b - spl, co]
  int act; float alpha;
  uint32_t thresh; float dscale; uint32_t seed, layer;
  const float* act_out; int ld_act;             // bwd: multiply by act'(act_out) (and the dropout mask of the producer)
  int bwd, accumulate, vecx, vecw;
};

template <int TM, int TN>
__global__ __launch_bounds__(NT) void wide_gemm_rows(RowArgs a) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int NA = KT * BM / NT, NB = KT * BN / NT;
  __shared__ float As[KT][BM];
  __shared__ float Bs[KT][BN];
  __shared__ int rimg[BM], rhy[BM], rwx[BM];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long long m0 = (long long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int HWm = a.Hm * a.Wm;

  // A loader: row am, channels akg*NA .. +NA of the stage
  const int am = t % BM, akg = t / BM;
  const long long mA = m0 + am;
  const bool rowv = mA < a.M;
  int img = 0, hm = 0, wm = 0;
  if (rowv) { img = (int)(mA / HWm); int r = (int)(mA - (long long)img * HWm); hm = r / a.Wm; wm = r - hm * a.Wm; }
  const int hy0 = hm * a.stride - a.pt, wx0 = wm * a.stride - a.pl;
  if (a.scatter && akg == 0) { rimg[am] = img * a.Hy; rhy[am] = hm * a.scatter - a.spt; rwx[am] = wm * a.scatter - a.spl; }
  // B loader
  constexpr int BG = BN / NB;                   // column groups of NB
  const int bk = t / BG, bn = (t % BG) * NB;    // non-transposed: row bk, columns bn .. +NB
  const int tbn = t % BN, tbk = (t / BN) * NB;  // transposed: column tbn, rows tbk .. +NB

  const int cch = (a.Cx + KT - 1) / KT;
  const int T = a.kh * a.kw * cch;
  float ra[NA], rb[NB];

  auto load = [&](int it) {
    const int tap = it / cch, c0 = (it - tap * cch) * KT;
    const int ty = tap / a.kw, tx = tap - ty * a.kw;
    {
      const int hy = hy0 + ty, wx = wx0 + tx, c = c0 + akg * NA;
      const bool v = rowv && hy >= 0 && hy < a.Hx && wx >= 0 && wx < a.Wx;
      const float* p = a.x + (((long long)img * a.Hx + hy) * a.Wx + wx) * a.ldx + c;
      if (v && a.vecx && c + NA <= a.Cx) {
#pragma unroll
        for (int j = 0; j < NA; j += 4) { float4 q = *(const float4*)(p + j); ra[j] = q.x; ra[j + 1] = q.y; ra[j + 2] = q.z; ra[j + 3] = q.w; }
      } else {
#pragma unroll
        for (int j = 0; j < NA; ++j) ra[j] = (v && c + j < a.Cx) ? p[j] : 0.f;
      }
    }
    if (!a.transb) {
      const int c = c0 + bk, n = n0 + bn;
      const float* p = a.w + ((long long)tap * a.Cx + c) * a.Ncol + n;
      if (c < a.Cx && a.vecw && n + NB <= a.Ncol) {
#pragma unroll
        for (int j = 0; j < NB; j += 4) { float4 q = *(const float4*)(p + j); rb[j] = q.x; rb[j + 1] = q.y; rb[j + 2] = q.z; rb[j + 3] = q.w; }
      } else {
#pragma unroll
        for (int j = 0; j < NB; ++j) rb[j] = (c < a.Cx && n + j < a.Ncol) ? p[j] : 0.f;
      }
    } else {
      const int n = n0 + tbn, c = c0 + tbk;
      const float* p = a.w + (long long)n * a.Cx + c;
#pragma unroll
      for (int j = 0; j < NB; ++j) rb[j] = (n < a.Ncol && c + j < a.Cx) ? p[j] : 0.f;
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x16{0.f};

  const int wr = wv >> 1, wc = wv & 1, li = lane & 31, lk = lane >> 5;
  load(0);
  for (int it = 0; it < T; ++it) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NA; ++j) As[akg * NA + j][am] = ra[j];
    if (!a.transb) {
#pragma unroll
      for (int j = 0; j < NB; ++j) Bs[bk][bn + j] = rb[j];
    } else {
#pragma unroll
      for (int j = 0; j < NB; ++j) Bs[tbk + j][tbn] = rb[j];
    }
    __syncthreads();
    if (it + 1 < T) load(it + 1);
#pragma unroll
    for (int s = 0; s < KT / 2; ++s) {
      float av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = As[2 * s + lk][(wr * TM + i) * 32 + li];
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[j] = Bs[2 * s + lk][(wc * TN + j) * 32 + li];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
  }

  // epilogue: lane holds column li of each 32 x 32 tile, rows (r & 3) + 8 (r >> 2) + 4 lk
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + (wc * TN + j) * 32 + li;
    if (n >= a.Ncol) continue;
    int co = n, fa = 0, fb = 0;
    if (a.scatter) { const int ab = n / a.Cy; co = n - ab * a.Cy; fa = ab / a.scatter; fb = ab - fa * a.scatter; }
    const float bz = (!a.bwd && a.bias) ? a.bias[co] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (wr * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        const long long m = m0 + row;
        if (m >= a.M) continue;
        float v = acc[i][j][r];
        long long off;
        if (a.scatter) {
          const int hy = rhy[row] + fa, wx = rwx[row] + fb;
          if (hy < 0 || hy >= a.Hy || wx < 0 || wx >= a.Wy) continue;
          off = ((long long)(rimg[row] + hy) * a.Wy + wx) * a.ldy + co;
        } else {
          off = m * a.ldy + n;
        }
        if (!a.bwd) {
          v += bz;
          if (a.thresh) v = drop_keep(a.seed, a.layer, (uint64_t)m * a.Ncol + n, a.thresh) ? v * a.dscale : 0.f;
          v = pcnn_act(v, a.act, a.alpha);
        } else if (a.act_out) {
          const float o = a.act_out[m * a.ld_act + n];
          if (a.act == PCNN_ACT_RELU) {
            v = o > 0.f ? v * a.dscale : 0.f;                         // with dropout before the ReLU, a > 0 implies "kept"
          } else {
            v *= pcnn_act_grad_from_out(o, a.act, a.alpha);
            if (a.thresh) v = drop_keep(a.seed, a.layer, (uint64_t)m * a.Ncol + n, a.thresh) ? v * a.dscale : 0.f;
          }
        }
        if (a.accumulate) v += a.y[off];
        a.y[off] = v;
      }
    }
  }
}

struct PixArgs {
  const float* x; int Hx, Wx, Cx, ldx;          // A[(tap, c), p] = x[img, hm*stride + ty - pt, wm*stride + tx - pl, c]; row kh*kw*Cx = ones (bias_row)
  int Hm, Wm; long long P;                      // K: the pixels of an (P / (Hm Wm)) x Hm x Wm grid
  int kh, kw, stride, pt, pl, bias_row;
  const float* b; int ldb; int Ncol; int vecb;  // B[p, n] = b[p*ldb + n]
  float* part; int Mrows;                       // part[split][Mrows][Ncol]
  int tiles_per_split; long long ktiles;
};

template <int TM, int TN>
__global__ __launch_bounds__(NT) void wide_gemm_pix(PixArgs a) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int NA = KT * BM / NT, NB = KT * BN / NT;
  constexpr int AG = BM / NA, BG = BN / NB;
  __shared__ float As[KT][BM + 4];
  __shared__ float Bs[KT][BN];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int HWm = a.Hm * a.Wm;
  const int taps = a.kh * a.kw;

  // A loader: pixel akk of the stage, rows am .. +NA (tap / channel of each row precomputed)
  const int akk = t / AG, am = (t % AG) * NA;
  int tyx[NA], aoff[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int m = m0 + am + j;
    if (m < taps * a.Cx) {
      const int tap = m / a.Cx, c = m - tap * a.Cx, ty = tap / a.kw, tx = tap - ty * a.kw;
      tyx[j] = (ty << 16) | tx;
      aoff[j] = (ty * a.Wx + tx) * a.ldx + c;
    } else {
      tyx[j] = (m == taps * a.Cx && a.bias_row) ? -1 : -2;
      aoff[j] = 0;
    }
  }
  const int bk = t / BG, bn = (t % BG) * NB;

  const long long kt0 = (long long)blockIdx.z * a.tiles_per_split;
  const long long kt1 = min(kt0 + a.tiles_per_split, a.ktiles);
  float ra[NA], rb[NB];

  auto load = [&](long long kt) {
    {
      const long long p = kt * KT + akk;
      const bool pv = p < a.P;
      int img = 0, hm = 0, wm = 0;
      if (pv) { img = (int)(p / HWm); int r = (int)(p - (long long)img * HWm); hm = r / a.Wm; wm = r - hm * a.Wm; }
      const int hy0 = hm * a.stride - a.pt, wx0 = wm * a.stride - a.pl;
      const long long base = (((long long)img * a.Hx + hy0) * a.Wx + wx0) * a.ldx;
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        float v = 0.f;
        if (pv) {
          if (tyx[j] >= 0) {
            const int hy = hy0 + (tyx[j] >> 16), wx = wx0 + (tyx[j] & 0xffff);
            if (hy >= 0 && hy < a.Hx && wx >= 0 && wx < a.Wx) v = a.x[base + aoff[j]];
          } else if (tyx[j] == -1) {
            v = 1.f;
          }
        }
        ra[j] = v;
      }
    }
    {
      const long long p = kt * KT + bk;
      const int n = n0 + bn;
      const float* q = a.b + p * a.ldb + n;
      if (p < a.P && a.vecb && n + NB <= a.Ncol) {
#pragma unroll
        for (int j = 0; j < NB; j += 4) { float4 u = *(const float4*)(q + j); rb[j] = u.x; rb[j + 1] = u.y; rb[j + 2] = u.z; rb[j + 3] = u.w; }
      } else {
#pragma unroll
        for (int j = 0; j < NB; ++j) rb[j] = (p < a.P && n + j < a.Ncol) ? q[j] : 0.f;
      }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x16{0.f};

  const int wr = wv >> 1, wc = wv & 1, li = lane & 31, lk = lane >> 5;
  if (kt0 < kt1) load(kt0);
  for (long long kt = kt0; kt < kt1; ++kt) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NA; ++j) As[akk][am + j] = ra[j];
#pragma unroll
    for (int j = 0; j < NB; ++j) Bs[bk][bn + j] = rb[j];
    __syncthreads();
    if (kt + 1 < kt1) load(kt + 1);
#pragma unroll
    for (int s = 0; s < KT / 2; ++s) {
      float av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = As[2 * s + lk][(wr * TM + i) * 32 + li];
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[j] = Bs[2 * s + lk][(wc * TN + j) * 32 + li];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
  }

  float* out = a.part + (long long)blockIdx.z * a.Mrows * a.Ncol;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + (wc * TN + j) * 32 + li;
    if (n >= a.Ncol) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + (wr * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (m < a.Mrows) out[(long long)m * a.Ncol + n] = acc[i][j][r];
      }
  }
}

// dw[m, n] = sum over splits in order; the bias row (m == rows_w) goes to dbias
__global__ void wide_reduce_splits(const float* part, int splits, long long count, int Ncol, long long rows_w, float* dw, float* dbias) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  float s = 0.f;
  for (int z = 0; z < splits; ++z) s += part[(long long)z * count + i];
  const long long m = i / Ncol;
  if (m < rows_w) dw[i] = s;
  else if (dbias) dbias[i - m * Ncol] = s;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int launch_rows(pcnn_handle_s* h, RowArgs& a, const char* name) {
  a.vecx = (a.Cx % 4 == 0 && pcnn_quads_ok(a.x, a.ldx)) ? 1 : 0;
  a.vecw = (!a.transb && a.Ncol % 4 == 0 && aligned16(a.w)) ? 1 : 0;
  if (a.M <= 0 || a.Ncol <= 0) return 0;
  if (a.Ncol <= 64) {
    dim3 g((unsigned)pcnn_cdiv64(a.M, 256), (unsigned)pcnn_cdiv(a.Ncol, 64));
    hipLaunchKernelGGL((wide_gemm_rows<4, 1>), g, dim3(NT), 0, h->stream, a);
  } else {
    dim3 g((unsigned)pcnn_cdiv64(a.M, 128), (unsigned)pcnn_cdiv(a.Ncol, 128));
    hipLaunchKernelGGL((wide_gemm_rows<2, 2>), g, dim3(NT), 0, h->stream, a);
  }
  PCNN_CHECK_LAUNCH(h, name);
  return 0;
}

// split-K plan of a filter gradient: ~2 workgroups per CU (256 CUs), at most 256 splits, at least 8 stages per split
struct PixPlan { int wide; int Mrows; long long ktiles; int per, splits; };
PixPlan plan_pix(int Mrows, int Ncol, long long P) {
  PixPlan q;
  q.wide = Ncol > 64;
  q.Mrows = Mrows;
  const long long mn = q.wide ? pcnn_cdiv64(Mrows, 128) * pcnn_cdiv64(Ncol, 128) : pcnn_cdiv64(Mrows, 256) * pcnn_cdiv64(Ncol, 64);
  q.ktiles = pcnn_cdiv64(P, KT);
  long long s = pcnn_cdiv64(512, mn);
  s = std::min<long long>(s, 256);
  s = std::min<long long>(s, std::max<long long>(1, q.ktiles / 8));
  s = std::max<long long>(s, 1);
  q.per = (int)pcnn_cdiv64(q.ktiles, s);
  q.splits = (int)pcnn_cdiv64(q.ktiles, q.per);
  return q;
}

int launch_pix(pcnn_handle_s* h, PixArgs& a, const PixPlan& q, float* dw, float* dbias, void* ws, size_t ws_bytes, const char* name) {
  const long long count = (long long)q.Mrows * a.Ncol;
  const size_t need = (size_t)q.splits * (size_t)count * sizeof(float);
  PCNN_REQUIRE(h, ws_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", name, ws_bytes, need);
  a.part = (float*)ws;
  a.Mrows = q.Mrows;
  a.tiles_per_split = q.per;
  a.ktiles = q.ktiles;
  a.vecb = (a.Ncol % 4 == 0 && pcnn_quads_ok(a.b, a.ldb)) ? 1 : 0;
  if (q.wide) {
    dim3 g((unsigned)pcnn_cdiv(q.Mrows, 128), (unsigned)pcnn_cdiv(a.Ncol, 128), (unsigned)q.splits);
    hipLaunchKernelGGL((wide_gemm_pix<2, 2>), g, dim3(NT), 0, h->stream, a);
  } else {
    dim3 g((unsigned)pcnn_cdiv(q.Mrows, 256), (unsigned)pcnn_cdiv(a.Ncol, 64), (unsigned)q.splits);
    hipLaunchKernelGGL((wide_gemm_pix<4, 1>), g, dim3(NT), 0, h->stream, a);
  }
  PCNN_CHECK_LAUNCH(h, name);
  const long long rows_w = (long long)a.kh * a.kw * a.Cx;
  hipLaunchKernelGGL(wide_reduce_splits, dim3((unsigned)pcnn_cdiv64(count, 256)), dim3(256), 0, h->stream, (const float*)ws, q.splits, count, a.Ncol,
                     rows_w, dw, dbias);
  PCNN_CHECK_LAUNCH(h, name);
  return 0;
}

void set_dropout(RowArgs& a, const pcnn_wide_desc* d) {
  a.thresh = 0; a.dscale = 1.f; a.seed = d->dropout_seed; a.layer = d->dropout_layer;
  if (d->dropout_rate > 0.f) {
    const double th = (double)d->dropout_rate * 4294967296.0;
    a.thresh = th >= 4294967295.0 ? 4294967295u : (uint32_t)th;
    a.dscale = 1.f / (1.f - d->dropout_rate);
  }
}

int check_desc(pcnn_handle_s* h, const pcnn_wide_desc* d, const char* name) {
  PCNN_REQUIRE(h, d, "%s: null descriptor", name);
  PCNN_REQUIRE(h, d->N > 0 && d->H > 0 && d->W > 0 && d->Ho > 0 && d->Wo > 0 && d->Cin > 0 && d->Cout > 0, "%s: empty shape", name);
  PCNN_REQUIRE(h, d->ldx >= d->Cin && d->ldy >= d->Cout, "%s: channel stride smaller than the channel count", name);
  PCNN_REQUIRE(h, d->H < 65536 && d->W < 65536, "%s: image too large", name);
  PCNN_REQUIRE(h, d->dropout_rate >= 0.f && d->dropout_rate < 1.f, "%s: dropout rate %g outside [0, 1)", name, d->dropout_rate);
  return 0;
}

int deconv_pads(pcnn_handle_s* h, const pcnn_wide_desc* d, int Hc, int Wc, int Hf, int Wf, int* pt, int* pl, const char* name) {
  const int f = d->k;
  PCNN_REQUIRE(h, f >= 1 && f <= 8, "%s: f = %d unsupported", name, f);
  PCNN_REQUIRE(h, Hc == pcnn_cdiv(Hf, f) && Wc == pcnn_cdiv(Wf, f), "%s: coarse %dx%d is not ceil(%dx%d / %d)", name, Hc, Wc, Hf, Wf, f);
  *pt = (Hc * f - Hf) / 2;
  *pl = (Wc * f - Wf) / 2;
  return 0;
}

}  // namespace

extern "C" {

int pcnn_wide_conv2d_fwd(pcnn_handle h, const pcnn_wide_desc* d, const float* x, const float* w, const float* bias, float* y) {
  if (check_desc(h, d, "pcnn_wide_conv2d_fwd")) return 1;
  PCNN_REQUIRE(h, d->k % 2 == 1 && d->k <= 7 && d->Ho == d->H && d->Wo == d->W, "pcnn_wide_conv2d_fwd: SAME convolution with odd k <= 7 only");
  RowArgs a = {};
  a.x = x; a.Hx = d->H; a.Wx = d->W; a.Cx = d->Cin; a.ldx = d->ldx;
  a.Hm = d->H; a.Wm = d->W; a.M = (long long)d->N * d->H * d->W;
  a.kh = a.kw = d->k; a.stride = 1; a.pt = a.pl = d->k / 2;
  a.w = w; a.Ncol = d->Cout; a.bias = bias; a.y = y; a.ldy = d->ldy;
  a.act = d->act; a.alpha = d->act_alpha; set_dropout(a, d);
  a.accumulate = d->accumulate;
  return launch_rows(h, a, "pcnn_wide_conv2d_fwd");
}

int pcnn_wide_conv2d_dgrad(pcnn_handle h, const pcnn_wide_desc* d, const float* dz, const float* wf, const float* act_out, float* dx) {
  if (check_desc(h, d, "pcnn_wide_conv2d_dgrad")) return 1;
  PCNN_REQUIRE(h, d->k % 2 == 1 && d->k <= 7 && d->Ho == d->H && d->Wo == d->W, "pcnn_wide_conv2d_dgrad: SAME convolution with odd k <= 7 only");
  RowArgs a = {};
  a.x = dz; a.Hx = d->H; a.Wx = d->W; a.Cx = d->Cin; a.ldx = d->ldx;
  a.Hm = d->H; a.Wm = d->W; a.M = (long long)d->N * d->H * d->W;
  a.kh = a.kw = d->k; a.stride = 1; a.pt = a.pl = d->k / 2;
  a.w = wf; a.Ncol = d->Cout; a.y = dx; a.ldy = d->ldy;
  a.act = d->act; a.alpha = d->act_alpha; set_dropout(a, d);
  a.act_out = act_out; a.ld_act = d->ld_act_out; a.bwd = 1; a.accumulate = d->accumulate;
  return launch_rows(h, a, "pcnn_wide_conv2d_dgrad");
}

size_t pcnn_wide_conv2d_wgrad_workspace(const pcnn_wide_desc* d) {
  const PixPlan q = plan_pix(d->k * d->k * d->Cin + 1, d->Cout, (long long)d->N * d->H * d->W);
  return (size_t)q.splits * q.Mrows * d->Cout * sizeof(float);
}

int pcnn_wide_conv2d_wgrad(pcnn_handle h, const pcnn_wide_desc* d, const float* x, const float* dz, float* dw, float* dbias, void* ws, size_t ws_bytes) {
  if (check_desc(h, d, "pcnn_wide_conv2d_wgrad")) return 1;
  PCNN_REQUIRE(h, d->k % 2 == 1 && d->k <= 7 && d->Ho == d->H && d->Wo == d->W, "pcnn_wide_conv2d_wgrad: SAME convolution with odd k <= 7 only");
  PixArgs a = {};
  a.x = x; a.Hx = d->H; a.Wx = d->W; a.Cx = d->Cin; a.ldx = d->ldx;
  a.Hm = d->H; a.Wm = d->W; a.P = (long long)d->N * d->H * d->W;
  a.kh = a.kw = d->k; a.stride = 1; a.pt = a.pl = d->k / 2; a.bias_row = 1;
  a.b = dz; a.ldb = d->ldy; a.Ncol = d->Cout;
  const PixPlan q = plan_pix(d->k * d->k * d->Cin + 1, d->Cout, a.P);
  return launch_pix(h, a, q, dw, dbias, ws, ws_bytes, "pcnn_wide_conv2d_wgrad");
}

int pcnn_wide_deconv_fwd(pcnn_handle h, const pcnn_wide_desc* d, const float* x, const float* k, const float* bias, float* y) {
  if (check_desc(h, d, "pcnn_wide_deconv_fwd")) return 1;
  PCNN_REQUIRE(h, d->dropout_rate == 0.f && !d->accumulate, "pcnn_wide_deconv_fwd: no dropout / accumulate");
  int pt, pl;
  if (deconv_pads(h, d, d->H, d->W, d->Ho, d->Wo, &pt, &pl, "pcnn_wide_deconv_fwd")) return 1;
  RowArgs a = {};
  a.x = x; a.Hx = d->H; a.Wx = d->W; a.Cx = d->Cin; a.ldx = d->ldx;
  a.Hm = d->H; a.Wm = d->W; a.M = (long long)d->N * d->H * d->W;
  a.kh = a.kw = 1; a.stride = 1;
  a.w = k; a.Ncol = d->k * d->k * d->Cout; a.transb = 1;                 // TF (f, f, Cout, Cin) = B^T of the per-pixel GEMM
  a.bias = bias; a.y = y; a.ldy = d->ldy;
  a.scatter = d->k; a.Hy = d->Ho; a.Wy = d->Wo; a.Cy = d->Cout; a.spt = pt; a.spl = pl;
  a.act = d->act; a.alpha = d->act_alpha; set_dropout(a, d);
  return launch_rows(h, a, "pcnn_wide_deconv_fwd");
}

int pcnn_wide_deconv_bwd_data(pcnn_handle h, const pcnn_wide_desc* d, const float* dz, const float* k, const float* act_out, float* dx) {
  if (check_desc(h, d, "pcnn_wide_deconv_bwd_data")) return 1;
  int pt, pl;
  if (deconv_pads(h, d, d->Ho, d->Wo, d->H, d->W, &pt, &pl, "pcnn_wide_deconv_bwd_data")) return 1;
  RowArgs a = {};
  a.x = dz; a.Hx = d->H; a.Wx = d->W; a.Cx = d->Cin; a.ldx = d->ldx;    // fine grid, Cin = the deconvolution's Cout
  a.Hm = d->Ho; a.Wm = d->Wo; a.M = (long long)d->N * d->Ho * d->Wo;
  a.kh = a.kw = d->k; a.stride = d->k; a.pt = pt; a.pl = pl;
  a.w = k; a.Ncol = d->Cout; a.y = dx; a.ldy = d->ldy;                    // B[(a, b, co), ci] = k[a, b, co, ci]
  a.act = d->act; a.alpha = d->act_alpha; set_dropout(a, d);
  a.act_out = act_out; a.ld_act = d->ld_act_out; a.bwd = 1; a.accumulate = d->accumulate;
  return launch_rows(h, a, "pcnn_wide_deconv_bwd_data");
}

size_t pcnn_wide_deconv_bwd_filter_workspace(const pcnn_wide_desc* d) {
  const PixPlan q = plan_pix(d->k * d->k * d->Cout, d->Cin, (long long)d->N * d->H * d->W);
  return (size_t)q.splits * q.Mrows * d->Cin * sizeof(float);
}

int pcnn_wide_deconv_bwd_filter(pcnn_handle h, const pcnn_wide_desc* d, const float* x, const float* dz, float* dk, void* ws, size_t ws_bytes) {
  if (check_desc(h, d, "pcnn_wide_deconv_bwd_filter")) return 1;
  int pt, pl;
  if (deconv_pads(h, d, d->H, d->W, d->Ho, d->Wo, &pt, &pl, "pcnn_wide_deconv_bwd_filter")) return 1;
  PixArgs a = {};
  a.x = dz; a.Hx = d->Ho; a.Wx = d->Wo; a.Cx = d->Cout; a.ldx = d->ldy;  // rows (a, b, co) gathered from the fine gradient
  a.Hm = d->H; a.Wm = d->W; a.P = (long long)d->N * d->H * d->W;         // pixels of the coarse input
  a.kh = a.kw = d->k; a.stride = d->k; a.pt = pt; a.pl = pl; a.bias_row = 0;
  a.b = x; a.ldb = d->ldx; a.Ncol = d->Cin;
  const PixPlan q = plan_pix(d->k * d->k * d->Cout, d->Cin, a.P);
  return launch_pix(h, a, q, dk, nullptr, ws, ws_bytes, "pcnn_wide_deconv_bwd_filter");
}

}  // extern "C"
