// Shared declarations of the tiled spectral convolution: spectral_conv.hip (32-point tiles, mixing kernels, host side) and spectral64.hip
// (64-point tiles).  Spectrum layout for a tile size T (T = 32 or 64): items (tile x channel group of 32) are T*T rows of 32 floats
// (128-byte channel vectors); rows [0,T): column fx = 0 (real in x, half-complex in y: Re fy = 0..T/2, then Im fy = 1..T/2-1),
// [T,2T): fx = T/2, then for fx = 1..T/2-1: 2T + 2T (fx-1) + {fy | T + fy} = Re | Im of the complex column (tools/spectral_model.py,
// tools/spectral_model64.py).  T*T/2 mixing slots.
#pragma once
#include "pcnn_internal.h"
#include <type_traits>

namespace pcnn_spec {

constexpr int RS = 32;                       // floats between consecutive spectrum rows of an item
// floats between consecutive items: rows x RS plus SP_PAD - the per-frequency kernels gather the same row of many items, i.e. they walk
// memory with the item stride; a power-of-two stride maps those accesses onto few HBM channels
constexpr int SP_PAD = 32;
__host__ __device__ __forceinline__ int64_t sp_item(int64_t item, int rows) { return item * ((int64_t)rows * RS + SP_PAD); }
__host__ __device__ __forceinline__ size_t sp_bytes(size_t items, int rows) { return items * ((size_t)rows * RS + SP_PAD) * sizeof(float); }

// ---- row order inside an item.  CANONICAL order (the matrix-core transform family, the debug exports and the tests): the header comment above.
// The FFT family (spectral_fft.hip, the default) interleaves the real and the imaginary row of a frequency in blocks of SP_P frequencies, so that
// the per-frequency kernels - which read / write the (Re, Im) row pair of ONE frequency of every item - find the pair inside one 256 P-byte piece of the
// item instead of T rows (4 / 8 KB) apart: row(k, part) = 2 P (k / P) + P part + k % P inside a column block, k = frequency index of the column (complex
// column: fy = 0..T-1; real column: the pair index, k = 0 the two real frequencies fy = 0 | T/2, k >= 1: Re | Im of fy = k).  P = T (T/2 for the real
// columns) IS the canonical order.  The mixing kernels only follow the slot tables (rr, ri), built from the same function for each family.
constexpr int SP_P = 1;
__host__ __device__ constexpr int sp_blk(int P, int k, int part) { return 2 * P * (k / P) + P * part + (k % P); }
__host__ __device__ constexpr int sp_pc(int T, int P) { return P < T ? P : T; }             // block size of a complex column
__host__ __device__ constexpr int sp_pr(int T, int P) { return P < T / 2 ? P : T / 2; }     // ... of a real column
// complex column of a T-point tile: row (inside the column's 2 T rows) of part (0 real, 1 imaginary) of frequency fy
__host__ __device__ constexpr int sp_row_c(int T, int fy, int part, int P = SP_P) { return sp_blk(sp_pc(T, P), fy, part); }
// real column: row (inside the column's T rows) of half-complex entry s (s <= T/2: Re fy = s; s > T/2: Im fy = s - T/2)
__host__ __device__ constexpr int sp_row_r(int T, int s, int P = SP_P) {
  return s == T / 2 ? sp_blk(sp_pr(T, P), 0, 1) : (s < T / 2 ? sp_blk(sp_pr(T, P), s, 0) : sp_blk(sp_pr(T, P), s - T / 2, 1));
}
// canonical row r of an item -> its row in the order with block size P
__host__ __device__ constexpr int sp_row_from_canonical(int T, int r, int P = SP_P) {
  return r < 2 * T ? (r / T) * T + sp_row_r(T, r % T, P) : 2 * T + ((r - 2 * T) / (2 * T)) * 2 * T + sp_row_c(T, (r - 2 * T) % T, ((r - 2 * T) % (2 * T)) / T, P);
}
static_assert(sp_row_from_canonical(32, 5, 64) == 5 && sp_row_from_canonical(32, 16, 64) == 16 && sp_row_from_canonical(32, 64 + 37, 64) == 64 + 37 && sp_row_from_canonical(64, 128 + 64 + 9, 64) == 128 + 64 + 9, "P >= T is the canonical order");
static_assert(sp_row_from_canonical(32, 16, 1) == 1 && sp_row_from_canonical(32, 3, 1) == 6 && sp_row_from_canonical(32, 16 + 3, 1) == 7 && sp_row_from_canonical(32, 64 + 32 + 5, 1) == 64 + 11, "P = 1: Re | Im adjacent");
// the mixing slots (rr, ri, kind, 0) of a tile size in the order with block size P: T^2 / 2 of them (kind 1: the slot packs two REAL frequencies)
inline void sp_build_slots(int T, int P, int* slots) {
  int n = 0;
  auto put = [&](int rr, int ri, int kind) { slots[4 * n] = rr; slots[4 * n + 1] = ri; slots[4 * n + 2] = kind; slots[4 * n + 3] = 0; ++n; };
  for (int b = 0; b < 2; ++b) {
    put(b * T + sp_row_r(T, 0, P), b * T + sp_row_r(T, T / 2, P), 1);
    for (int fy = 1; fy < T / 2; ++fy) put(b * T + sp_row_r(T, fy, P), b * T + sp_row_r(T, T / 2 + fy, P), 0);
  }
  for (int fx = 1; fx < T / 2; ++fx)
    for (int fy = 0; fy < T; ++fy) put(2 * T + 2 * T * (fx - 1) + sp_row_c(T, fy, 0, P), 2 * T + 2 * T * (fx - 1) + sp_row_c(T, fy, 1, P), 0);
}

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
__device__ __forceinline__ f32x4 zero4() { f32x4 z = {0.f, 0.f, 0.f, 0.f}; return z; }
// Workgroup barrier that orders LDS traffic only (__syncthreads() also drains vmcnt, i.e. waits for the next item's prefetch loads and the
// spectrum stores in flight; the prefetched registers are waited for where they are consumed, global stores need no ordering here).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// accumulator register r of lane (half) <-> row of the 32x32 tile
__device__ __forceinline__ int acc_row(int r, int half) { return 8 * (r >> 2) + 4 * half + (r & 3); }

// 4 x 4 transpose between the four lanes of a quad and four registers: lane i, register j  <->  lane j, register i.  A 16-byte load gives a
// lane four consecutive CHANNELS of one pixel (or spectrum row), the MFMA operand layout wants a lane to hold ONE channel of four pixels:
// two DPP exchange steps (neighbours, then pairs) convert between the two, so that every global access of the transform kernels moves
// 16 bytes per lane - the texture-address path takes a wave instruction every ~16 cycles whatever its width, and at 4 bytes per lane the
// transforms' loads and stores occupied it for as long as their MFMAs occupy the matrix pipe (in-kernel stamps).
__device__ __forceinline__ float dpp_quad_swap1(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, true)); }   // [1,0,3,2]
__device__ __forceinline__ float dpp_quad_swap2(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xf, 0xf, true)); }   // [2,3,0,1]
__device__ __forceinline__ void quad_transpose(float& r0, float& r1, float& r2, float& r3, bool odd, bool upper) {
  { const float t = dpp_quad_swap1(odd ? r0 : r1); if (odd) r0 = t; else r1 = t; }
  { const float t = dpp_quad_swap1(odd ? r2 : r3); if (odd) r2 = t; else r3 = t; }
  { const float t = dpp_quad_swap2(upper ? r0 : r2); if (upper) r0 = t; else r2 = t; }
  { const float t = dpp_quad_swap2(upper ? r1 : r3); if (upper) r1 = t; else r3 = t; }
}

struct FwdParams {
  const float* x = nullptr; float* sp = nullptr; const float* tab = nullptr;
  int H = 0, W = 0, C = 0, ld = 0, groups = 1, cstride = 32, cvalid = 32;
  int tiles_x = 1, tiles_y = 1, tile0 = 0, ntile = 1;
  int Vy = 0, Vx = 0, oy = 0, ox = 0, pad_mode = PCNN_PAD_CONSTANT; float pad_value = 0.f;
  int ylim = 0, xlim = 0;                    // the window holds values only in its first ylim x xlim entries (gradient / input tiles of the backward pass)
  int ext_y = 1 << 30, ext_x = 1 << 30;      // ... and only where the tile grid coordinate (ty Vy + r, tx Vx + c) lies inside ext_y x ext_x
  int pack = 1, cpt = 32, tgx = 1;           // layers of <= 16 channels: `pack` x-adjacent tiles share the 32 lanes (lane = cpt * tile + channel, cpt = 32 / pack);
                                             // tgx = tile groups per tile row; an "item" is then a tile GROUP and tile0 / ntile count groups
};

struct InvParams {
  const float* sp = nullptr; const float* tab = nullptr;
  float* y = nullptr; const float* bias = nullptr; const float* bn_scale = nullptr; const float* bn_shift = nullptr; const float* res = nullptr;
  float* act_out = nullptr; unsigned* absmax = nullptr;
  int Ho = 0, Wo = 0, C = 0, ldy = 0, ld_res = 0, ld_act = 0, groups = 1, cstride = 32, cvalid = 32, act = PCNN_ACT_LINEAR; float alpha = 0.f;
  int tiles_x = 1, tiles_y = 1, tile0 = 0, ntile = 1, Vy = 0, Vx = 0;
  int flip = 0;                    // store output pixel (y, x) at (Ho-1-y, Wo-1-x): the input-partitioned weight gradient comes out tap-reversed
  int pack = 1, cpt = 32, tgx = 1; // tile packing, as in FwdParams (flip requires pack == 1)
  // POST (data-gradient launches only): the activation backward of the layer that PRODUCED this convolution's input, applied to the gradient
  // before it is stored - v = (conv + residual); y2 (if given) receives v, y receives v * act'(gact) where gact is that layer's saved
  // activation output, and every lane adds what it stored into bsum[(block 8 + wave) 64 + lane] (the bias gradient's partial sums)
  const float* gact = nullptr; float* y2 = nullptr; float* bsum = nullptr;
  int ld_gact = 0, ld_y2 = 0, gmode = 0; float galpha = 1.f;
};

// ---- host side shared by the four transform back ends (matrix-core / FFT family x 32 / 64 points)
// workspace header: the constant tables of both tile sizes, then two slot tables per tile size (the canonical row order of the matrix-core family and
// the FFT family's interleaved order, above); the per-call regions follow at O_REST
constexpr int TAB32_FLOATS = 7168, TAB64_FLOATS = 32768;       // spectral_conv.hip build_tables / spectral64.hip build_tables64
constexpr size_t O_TAB32 = 0, O_SLOTS32 = O_TAB32 + ((TAB32_FLOATS * 4 + 255) & ~255), O_TAB64 = O_SLOTS32 + 512 * 16,
                 O_SLOTS64 = O_TAB64 + TAB64_FLOATS * 4, O_SLOTS32F = O_SLOTS64 + 2048 * 16, O_SLOTS64F = O_SLOTS32F + 512 * 16, O_REST = O_SLOTS64F + 2048 * 16;
static_assert(O_REST % 256 == 0, "workspace header alignment");
void build_tables64(float* tab, int* slots);                 // TAB64_FLOATS floats, 2048 x int4 slots (canonical order)

// POST: an inverse kernel runs at most POST_BLOCKS workgroups, and every (workgroup, wave) adds its lanes' bias-gradient partial sums into slots of 64 floats
// of its own (Xform::post_slots of them); the fused backward sizes the buffer for the back end that needs most
constexpr int POST_BLOCKS = 256, POST_SLOTS_MAX = POST_BLOCKS * 8 * 4;

// One transform back end: everything the host side needs to know about it.  The four records are defined next to their kernels
// (spectral_conv.hip, spectral64.hip, spectral_fft.hip); the launchers take the same parameter blocks and set p.ntile themselves.
struct Xform {
  int family;                      // PCNN_XFORM_MFMA | PCNN_XFORM_FFT
  int T, rows, nslot;              // tile size, spectrum rows per item (T^2), mixing slots (T^2 / 2)
  int P;                           // block size of its row order (sp_blk); >= T: the canonical order
  size_t tab_off, slots_off;       // its table block and slot table in the workspace header
  void (*fwd)(pcnn_handle h, FwdParams p, int ntile);
  void (*inv)(pcnn_handle h, InvParams p, int ntile);
  void (*post_bias)(pcnn_handle h, const float* bsum, int pack, int cpt, int C, float* dbias);   // POST partial sums of `inv` -> dbias
  void (*fwd_multi)(pcnn_handle h, const FwdParams* tab, int count, int max_items);   // `count` one-tile transforms (filters) from a device table of parameter blocks in one launch; null: the back end has no such kernel
  int post_slots;                  // 64-float POST partial-sum slots `inv` writes (<= POST_SLOTS_MAX)
  const float* tab; const int4* slots;   // resolved against the handle's current workspace by xform_of (spectral_conv.hip)
};
extern const Xform XFORM_MFMA32, XFORM_MFMA64, XFORM_FFT32, XFORM_FFT64;

// The epilogue variants of an inverse kernel, chosen once for all four back ends: launch(flag<TANH>, flag<RES>, flag<POST>, params) starts the
// instantiation <TANH, RES, POST> with the back end's own launch geometry.  alpha / galpha arrive at the kernel as the slope of the negative side
// (1 linear, 0 relu, the given slope for leaky relu); tanh has its own instantiation, and POST implies a linear convolution epilogue.
template <bool B> using flag = std::integral_constant<bool, B>;
template <typename Launch>
void dispatch_epilogue(InvParams p, Launch launch) {
  auto slope = [](int act, float alpha) { return act == PCNN_ACT_LINEAR ? 1.f : (act == PCNN_ACT_RELU ? 0.f : alpha); };
  if (p.gact) {                                                        // data gradient + the producer's activation backward
    p.alpha = 1.f; p.galpha = slope(p.gmode, p.galpha);
    if (p.res) launch(flag<false>{}, flag<true>{}, flag<true>{}, p); else launch(flag<false>{}, flag<false>{}, flag<true>{}, p);
  } else if (p.act == PCNN_ACT_TANH) {
    if (p.res) launch(flag<true>{}, flag<true>{}, flag<false>{}, p); else launch(flag<true>{}, flag<false>{}, flag<false>{}, p);
  } else {
    p.alpha = slope(p.act, p.alpha);
    if (p.res) launch(flag<false>{}, flag<true>{}, flag<false>{}, p); else launch(flag<false>{}, flag<false>{}, flag<false>{}, p);
  }
}

}  // namespace pcnn_spec
