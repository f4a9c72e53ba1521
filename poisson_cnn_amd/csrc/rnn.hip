// Recurrence kernels of Dirichlet_BC_RNN (models/Dirichlet_BC_RNN.py:24-30: tf.keras.layers.LSTM / GRU, return_sequences=True, batch-major).
//
// A recurrent layer is split in two.  Everything that is parallel over time - the input projection x_t W + b, and in the backward
// dX = dZ W^T, dW, dU, db - is a 1x1 convolution over all N T rows and runs on the wide-convolution engines (csrc/conv_wide.hip).  What is
// left is the dependent chain over t, and that is this file: ONE launch per layer and direction for the whole sequence.
//
// Mapping.  The samples of a batch do not interact, so a workgroup owns ONE sample and runs all T steps alone: no grid barrier, no flag or
// spin between workgroups, no residency requirement (a grid larger than the machine simply queues).  Inside the workgroup thread 4k + g owns
// gate column g of unit k: its column of U (forward) or its row segment U[k, g u : (g+1) u] (backward, the product with U^T) stays in
// registers for the whole launch; h_{t-1} (forward) or dZ_t (backward) is broadcast through a double-buffered LDS array, so a step costs one
// __syncthreads().  The four gates of a unit sit in four neighbouring lanes and are exchanged with lane shuffles; c, dc and the dh carry
// live in registers.  The products are fp32 FMAs on the vector ALUs in a fixed order: exact fp32 in every math mode, deterministic, no atomics.
// Why not the matrix cores: v_mfma_f32_32x32x2_f32 has the same fp32 peak per CU as the vector ALUs, and needs 32 samples per workgroup to
// fill a tile - batch 50 would occupy 2 CUs instead of 50.
#include "pcnn_internal.h"

namespace {

struct RnnArgs {
  int T, u, act, rec, reverse;
  const float* zx; long long sn_zx; int ld_zx;
  const float* U;
  const float* rbias;
  float* h; long long sn_h; int ld_h;
  float* h2; long long sn_h2; int ld_h2;
  float* saved;                                   // (N, T, (G + 1) u) dense
  const float* dh; long long sn_dh; int ld_dh;
  float* dzx; long long sn_dzx; int ld_dzx;
  float* dzh; long long sn_dzh; int ld_dzh;
};

// recurrent_activation: 'sigmoid' or Keras' hard_sigmoid = clip(0.2 x + 0.5, 0, 1).  exp(-x) = inf for very negative x gives 1 / inf = 0: no NaN.
__device__ __forceinline__ float rnn_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float rnn_rec(float x, int rec) {
  return rec == PCNN_RNN_HARD_SIGMOID ? fminf(fmaxf(0.2f * x + 0.5f, 0.0f), 1.0f) : rnn_sigmoid(x);
}
__device__ __forceinline__ float rnn_rec_grad(float s, int rec) {
  return rec == PCNN_RNN_HARD_SIGMOID ? ((s > 0.0f && s < 1.0f) ? 0.2f : 0.0f) : s * (1.0f - s);
}
// tanh in a saturating form: e = expm1(-2|x|) lies in [-1, 0], so -e / (2 + e) lies in [0, 1] for every x, infinities included
__device__ __forceinline__ float rnn_tanh(float x) {
  const float e = expm1f(-2.0f * fabsf(x));
  return copysignf(-e / (2.0f + e), x);
}
__device__ __forceinline__ float rnn_act(float x, int act) {
  switch (act) {
    case PCNN_RNN_ACT_TANH: return rnn_tanh(x);
    case PCNN_RNN_ACT_SIGMOID: return rnn_sigmoid(x);
    case PCNN_RNN_ACT_RELU: return fmaxf(x, 0.0f);
    default: return x;
  }
}
__device__ __forceinline__ float rnn_act_grad(float a, int act) {   // from the OUTPUT a = act(x)
  switch (act) {
    case PCNN_RNN_ACT_TANH: return 1.0f - a * a;
    case PCNN_RNN_ACT_SIGMOID: return a * (1.0f - a);
    case PCNN_RNN_ACT_RELU: return a > 0.0f ? 1.0f : 0.0f;
    default: return 1.0f;
  }
}

__device__ __forceinline__ float quad(float v, int q) { return __shfl(v, (int)((threadIdx.x & 60u) | (unsigned)q), 64); }

// sum_j v[j] * w[j] over UP values, v broadcast from LDS as float4; four chains in a fixed order
template <int UP>
__device__ __forceinline__ float dot_lds(const float* v, const float (&w)[UP]) {
  const float4* v4 = reinterpret_cast<const float4*>(v);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
  for (int j = 0; j < UP / 4; ++j) {
    const float4 q = v4[j];
    a0 = fmaf(q.x, w[4 * j + 0], a0);
    a1 = fmaf(q.y, w[4 * j + 1], a1);
    a2 = fmaf(q.z, w[4 * j + 2], a2);
    a3 = fmaf(q.w, w[4 * j + 3], a3);
  }
  return (a0 + a1) + (a2 + a3);
}

// Forward.  Block = 4 * units threads rounded up to a wave; grid = N.  UP: units padded to a compiled size (padding lives in registers and LDS
// only, as zeros).  Step s reads the projected gates at input position tau = reverse ? T - 1 - s : s and writes h and the saved values at s.
// saved per step: LSTM [i | f | c~ | o | c] (activated gates and the new cell state), GRU [z | r | h~ | (h U + b1)_h].
template <int UP, int CELL>
__global__ __launch_bounds__(512) void rnn_fwd_kernel(RnnArgs a) {
  constexpr int G = CELL == PCNN_RNN_LSTM ? 4 : 3;
  const int n = blockIdx.x, tid = threadIdx.x, k = tid >> 2, g = tid & 3, u = a.u;
  const bool unit = k < u, live = unit && g < G;
  __shared__ __align__(16) float hs[2][UP];
  float ucol[UP];
#pragma unroll
  for (int j = 0; j < UP; ++j) ucol[j] = (live && j < u) ? a.U[(long long)j * G * u + g * u + k] : 0.0f;
  const float rb = (CELL == PCNN_RNN_GRU && live && a.rbias) ? a.rbias[g * u + k] : 0.0f;
  for (int j = tid; j < 2 * UP; j += blockDim.x) (&hs[0][0])[j] = 0.0f;
  const float* zx = a.zx + n * a.sn_zx + g * u + k;
  float* sv = a.saved + (long long)n * a.T * (G + 1) * u;
  float c = 0.0f, hreg = 0.0f;
  float znext = live ? zx[(long long)(a.reverse ? a.T - 1 : 0) * a.ld_zx] : 0.0f;
  __syncthreads();
  for (int s = 0; s < a.T; ++s) {
    const float zxv = znext;
    if (s + 1 < a.T) znext = live ? zx[(long long)(a.reverse ? a.T - 2 - s : s + 1) * a.ld_zx] : 0.0f;
    const float m = dot_lds<UP>(hs[s & 1], ucol);
    float hn;
    float* svs = sv + (long long)s * (G + 1) * u;
    if (CELL == PCNN_RNN_LSTM) {
      const float pre = zxv + m;
      const float val = g == 2 ? rnn_act(pre, a.act) : rnn_rec(pre, a.rec);
      const float gi = quad(val, 0), gf = quad(val, 1), gc = quad(val, 2), go = quad(val, 3);
      c = gf * c + gi * gc;
      hn = go * rnn_act(c, a.act);
      if (live) svs[g * u + k] = val;
      if (unit && g == 1) svs[4 * u + k] = c;
    } else {
      const float mh = m + rb;
      const float sg = rnn_rec(zxv + mh, a.rec);
      const float r = quad(sg, 1);
      const float val = g == 2 ? rnn_act(zxv + r * mh, a.act) : sg;
      const float z = quad(val, 0), hh = quad(val, 2), mhh = quad(mh, 2);
      hn = z * hreg + (1.0f - z) * hh;
      hreg = hn;
      if (live) svs[g * u + k] = val;
      if (unit && g == 3) svs[3 * u + k] = mhh;
    }
    if (unit && g == 0) {
      hs[(s + 1) & 1][k] = hn;
      a.h[n * a.sn_h + (long long)s * a.ld_h + k] = hn;
      if (a.h2) a.h2[n * a.sn_h2 + (long long)s * a.ld_h2 + k] = hn;
    }
    __syncthreads();
  }
}

// Backward: the same structure from s = T - 1 down to 0.  Carries dh (and dc) in registers, adds the incoming gradient of h_s, forms dZ_s,
// stores it (dzx at the input position tau, dzh at s: for the GRU the two differ in the h~ block, for a reversed LSTM only in position)
// and the next carry dh_{s-1} = dZ_s U^T (+ the direct paths): thread 4k + g holds U[k, g u : (g+1) u], reads block g of dZ_s from LDS and
// the four partial sums of a unit are added across its lanes.
template <int UP, int CELL>
__global__ __launch_bounds__(512) void rnn_bwd_kernel(RnnArgs a) {
  constexpr int G = CELL == PCNN_RNN_LSTM ? 4 : 3;
  constexpr int LS = ((UP + 27) / 32) * 32 + 4;       // block stride, = 4 mod 32 floats: the four gate blocks' float4 reads fall into different banks
  const int n = blockIdx.x, tid = threadIdx.x, k = tid >> 2, g = tid & 3, u = a.u;
  const bool unit = k < u, live = unit && g < G;
  __shared__ __align__(16) float dzs[2][4 * LS];
  float urow[UP];
#pragma unroll
  for (int j = 0; j < UP; ++j) urow[j] = (live && j < u) ? a.U[(long long)k * G * u + g * u + j] : 0.0f;
  for (int j = tid; j < 8 * LS; j += blockDim.x) (&dzs[0][0])[j] = 0.0f;
  const int row = (G + 1) * u;
  const float* sv = a.saved + (long long)n * a.T * row;
  const float* dhp = a.dh + n * a.sn_dh + k;
  const float* hp = a.h + n * a.sn_h + k;
  float* dzx = a.dzx + n * a.sn_dzx + g * u + k;
  float* dzh = a.dzh + n * a.sn_dzh + g * u + k;
  const bool two = a.dzh != a.dzx;
  float dhc = 0.0f, dc = 0.0f;
  // lane-private loads of step s: every lane its own gate value; the three other values a unit needs are spread over its lanes
  auto load_own = [&](int s) { return live ? sv[(long long)s * row + g * u + k] : 0.0f; };
  auto load_aux = [&](int s) {
    float v = 0.0f;
    if (unit) {
      if (CELL == PCNN_RNN_LSTM) {
        if (g == 0) v = sv[(long long)s * row + 4 * u + k];
        else if (g == 1) v = s > 0 ? sv[(long long)(s - 1) * row + 4 * u + k] : 0.0f;
        else if (g == 2) v = dhp[(long long)s * a.ld_dh];
      } else {
        if (g == 0) v = dhp[(long long)s * a.ld_dh];
        else if (g == 1) v = s > 0 ? hp[(long long)(s - 1) * a.ld_h] : 0.0f;
        else if (g == 3) v = sv[(long long)s * row + 3 * u + k];
      }
    }
    return v;
  };
  float own = load_own(a.T - 1), aux = load_aux(a.T - 1);
  __syncthreads();
  for (int s = a.T - 1; s >= 0; --s) {
    const int tau = a.reverse ? a.T - 1 - s : s;
    float mine_x, mine_h, direct;
    if (CELL == PCNN_RNN_LSTM) {
      const float gi = quad(own, 0), gf = quad(own, 1), gc = quad(own, 2), go = quad(own, 3);
      const float cs = quad(aux, 0), cp = quad(aux, 1), dh = quad(aux, 2) + dhc;
      const float ac = rnn_act(cs, a.act);
      const float dcn = dc + dh * go * rnn_act_grad(ac, a.act);
      mine_x = g == 0 ? dcn * gc * rnn_rec_grad(gi, a.rec)
             : g == 1 ? dcn * cp * rnn_rec_grad(gf, a.rec)
             : g == 2 ? dcn * gi * rnn_act_grad(gc, a.act)
                      : dh * ac * rnn_rec_grad(go, a.rec);
      mine_h = mine_x;
      dc = dcn * gf;
      direct = 0.0f;
    } else {
      const float z = quad(own, 0), r = quad(own, 1), hh = quad(own, 2);
      const float dh = quad(aux, 0) + dhc, hprev = quad(aux, 1), mhh = quad(aux, 3);
      const float dpre = dh * (1.0f - z) * rnn_act_grad(hh, a.act);
      mine_x = g == 0 ? dh * (hprev - hh) * rnn_rec_grad(z, a.rec)
             : g == 1 ? dpre * mhh * rnn_rec_grad(r, a.rec)
                      : dpre;
      mine_h = g == 2 ? dpre * r : mine_x;
      direct = dh * z;
    }
    if (live) {
      dzx[(long long)tau * a.ld_dzx] = mine_x;
      if (two) dzh[(long long)s * a.ld_dzh] = mine_h;
      dzs[s & 1][g * LS + k] = mine_h;
    }
    __syncthreads();
    if (s > 0) { own = load_own(s - 1); aux = load_aux(s - 1); }
    float p = dot_lds<UP>(&dzs[s & 1][g * LS], urow);
    p += __shfl_xor(p, 1, 64);
    p += __shfl_xor(p, 2, 64);
    dhc = p + direct;
  }
}

static int pick_up(int u) { return u <= 8 ? 8 : u <= 32 ? 32 : u <= 64 ? 64 : u <= 100 ? 100 : 128; }

template <int CELL>
static void launch(bool fwd, int up, dim3 grid, dim3 block, hipStream_t st, const RnnArgs& a) {
#define PCNN_RNN_CASE(UPV)                                                                   \
  case UPV:                                                                                  \
    if (fwd) hipLaunchKernelGGL((rnn_fwd_kernel<UPV, CELL>), grid, block, 0, st, a);         \
    else hipLaunchKernelGGL((rnn_bwd_kernel<UPV, CELL>), grid, block, 0, st, a);             \
    break;
  switch (up) {
    PCNN_RNN_CASE(8)
    PCNN_RNN_CASE(32)
    PCNN_RNN_CASE(64)
    PCNN_RNN_CASE(100)
    PCNN_RNN_CASE(128)
  }
#undef PCNN_RNN_CASE
}

static int check_desc(pcnn_handle h, const pcnn_rnn_desc* d, const char* name) {
  PCNN_REQUIRE(h, d, "%s: null descriptor", name);
  PCNN_REQUIRE(h, d->cell == PCNN_RNN_LSTM || d->cell == PCNN_RNN_GRU, "%s: cell must be PCNN_RNN_LSTM or PCNN_RNN_GRU", name);
  PCNN_REQUIRE(h, d->N > 0 && d->T > 0, "%s: empty shape", name);
  PCNN_REQUIRE(h, d->units >= 1 && d->units <= PCNN_RNN_MAX_UNITS, "%s: units = %d outside [1, %d]", name, d->units, PCNN_RNN_MAX_UNITS);
  PCNN_REQUIRE(h, d->act >= PCNN_RNN_ACT_LINEAR && d->act <= PCNN_RNN_ACT_RELU, "%s: unknown activation %d", name, d->act);
  PCNN_REQUIRE(h, d->rec_act == PCNN_RNN_SIGMOID || d->rec_act == PCNN_RNN_HARD_SIGMOID, "%s: unknown recurrent activation %d", name, d->rec_act);
  return 0;
}

static int run(pcnn_handle h, const pcnn_rnn_desc* d, bool fwd, RnnArgs& a, const char* name) {
  a.T = d->T; a.u = d->units; a.act = d->act; a.rec = d->rec_act; a.reverse = d->reverse ? 1 : 0;
  const dim3 grid((unsigned)d->N), block((unsigned)(pcnn_cdiv(4 * d->units, 64) * 64));
  if (d->cell == PCNN_RNN_LSTM) launch<PCNN_RNN_LSTM>(fwd, pick_up(d->units), grid, block, h->stream, a);
  else launch<PCNN_RNN_GRU>(fwd, pick_up(d->units), grid, block, h->stream, a);
  PCNN_CHECK_LAUNCH(h, name);
  return 0;
}

}  // namespace

extern "C" {

size_t pcnn_rnn_saved_floats(const pcnn_rnn_desc* d) {
  if (!d) return 0;
  return (size_t)d->N * d->T * ((d->cell == PCNN_RNN_LSTM ? 4 : 3) + 1) * d->units;
}

int pcnn_rnn_fwd(pcnn_handle h, const pcnn_rnn_desc* d, const float* zx, const float* U, const float* rbias, float* hout, float* hout2,
                 float* saved) {
  if (check_desc(h, d, "pcnn_rnn_fwd")) return 1;
  const int Gu = (d->cell == PCNN_RNN_LSTM ? 4 : 3) * d->units;
  PCNN_REQUIRE(h, zx && U && hout && saved, "pcnn_rnn_fwd: null tensor");
  PCNN_REQUIRE(h, d->ld_zx >= Gu && d->ld_h >= d->units && (!hout2 || d->ld_h2 >= d->units), "pcnn_rnn_fwd: row stride smaller than the row");
  PCNN_REQUIRE(h, d->cell == PCNN_RNN_GRU || !rbias, "pcnn_rnn_fwd: the LSTM has no recurrent bias");
  RnnArgs a = {};
  a.zx = zx; a.sn_zx = d->sn_zx; a.ld_zx = d->ld_zx;
  a.U = U; a.rbias = rbias;
  a.h = hout; a.sn_h = d->sn_h; a.ld_h = d->ld_h;
  a.h2 = hout2; a.sn_h2 = d->sn_h2; a.ld_h2 = d->ld_h2;
  a.saved = saved;
  return run(h, d, true, a, "pcnn_rnn_fwd");
}

int pcnn_rnn_bwd(pcnn_handle h, const pcnn_rnn_desc* d, const float* U, const float* saved, const float* hout, const float* dh, float* dzx,
                 float* dzh) {
  if (check_desc(h, d, "pcnn_rnn_bwd")) return 1;
  const int Gu = (d->cell == PCNN_RNN_LSTM ? 4 : 3) * d->units;
  PCNN_REQUIRE(h, U && saved && hout && dh && dzx && dzh, "pcnn_rnn_bwd: null tensor");
  PCNN_REQUIRE(h, d->ld_dzx >= Gu && d->ld_dzh >= Gu && d->ld_h >= d->units && d->ld_dh >= d->units, "pcnn_rnn_bwd: row stride smaller than the row");
  PCNN_REQUIRE(h, dzh != dzx || (d->cell == PCNN_RNN_LSTM && !d->reverse && d->sn_dzh == d->sn_dzx && d->ld_dzh == d->ld_dzx),
               "pcnn_rnn_bwd: dzh may alias dzx only for a forward-running LSTM");
  RnnArgs a = {};
  a.U = U; a.saved = const_cast<float*>(saved);
  a.h = const_cast<float*>(hout); a.sn_h = d->sn_h; a.ld_h = d->ld_h;
  a.dh = dh; a.sn_dh = d->sn_dh; a.ld_dh = d->ld_dh;
  a.dzx = dzx; a.sn_dzx = d->sn_dzx; a.ld_dzx = d->ld_dzx;
  a.dzh = dzh; a.sn_dzh = d->sn_dzh; a.ld_dzh = d->ld_dzh;
  return run(h, d, false, a, "pcnn_rnn_bwd");
}

}  // extern "C"
