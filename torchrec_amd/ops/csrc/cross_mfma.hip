// Fused DCN-v2 low-rank cross layer for MI355X (gfx950), bf16 MFMA.
//
// One layer (reference: torchrec/modules/crossnet.py LowRankCrossNet), with
// V [r, N], W [N, r], b [N]:
//   t = x_l V^T          [B, r]
//   s = t W^T + b        [B, N]
//   y = x_0 * s + x_l    [B, N]
//
// Forward, one launch: a workgroup owns kBM = 32 rows. Phase 1 computes its
// [32, r] slice of t on v_mfma_f32_16x16x32_bf16 (fp32 accumulate), rounds it
// ONCE to bf16 and parks it in LDS; phase 2 streams W through LDS, reads the
// t slice as the other operand and applies +b, x_0*, +x_l on the fp32
// accumulators before the single bf16 store of y. The [B, r] intermediate is
// never read back from global memory (it is written there only when the
// backward will need it).
//
// Backward-data, one launch, g = dL/dy:
//   u    = bf16(g * x_0)                     (staged for the MFMA, also stored)
//   dt   = bf16(u W)           [32, r] slice in LDS, also stored
//   dx_l = bf16(g + dt V)
//   dx0_acc += g * (t W^T + b)               fp32, one thread per element
// Phase A is the forward's phase 1 with the product staged; phase B walks the
// N tiles once and runs both K = r products against the two LDS slices (dt
// and the saved t), so s is recomputed rather than saved.
//
// Every product is written so that both operands are row-major with K
// contiguous (V for x V^T, W for t W^T; the backward takes W^T and V^T
// copies, made once per call on the host side), which makes every fragment a
// 16-B ds_read_b128 of 8 consecutive k.
//
// Operand order is swapped, mfma(weights, activations): D'[n][m], so lane l
// holds FOUR CONSECUTIVE COLUMNS n = (l>>4)*4 + i of row m = l&15 — 8-B bf16
// stores / 16-B fp32 accesses in the epilogues instead of 2-B scatters.
//
// Pipeline: a [rows, 64] weight tile (128-B LDS rows, XOR-swizzled like
// interaction_mfma.hip) is double-buffered; the global loads of step s+1 are
// issued into registers before the MFMA loop of step s and written to the
// other buffer after it, one barrier per step. The loop is flat over
// (column pass, k step), so the prefetch also crosses pass boundaries.
//
// Each wave owns all 32 rows and a quarter of the pass's columns.

#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <algorithm>
#include <tuple>

#include "common.h"

namespace trec_amd {

namespace {

// Device code of this file is built without the packed fp32 VALU forms
// (v_pk_{add,mul,fma}_f32). A function only inlines into one with the same
// target features, so everything the kernels call is defined below — no
// header helpers (min/max, threadIdx, __syncthreads, uint4 constructors)
// between the push and the pop.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

typedef __attribute__((ext_vector_type(8))) __bf16 cbf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 cbf16x4;
typedef __attribute__((ext_vector_type(4))) float cf32x4;
typedef __attribute__((ext_vector_type(4))) unsigned cu32x4;  // one 16-B chunk

__device__ __forceinline__ int ctid() { return __builtin_amdgcn_workitem_id_x(); }
// workgroup barrier with LDS/global visibility (what __syncthreads expands to)
__device__ __forceinline__ void csync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ int cmin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int cmax(int a, int b) { return a > b ? a : b; }

constexpr int kBM = 32;        // rows per workgroup (two 16-row MFMA tiles)
constexpr int kKT = 64;        // k per staged tile: 128-B LDS rows
constexpr int kRowB = kKT * 2; // staged row bytes
constexpr int kCThreads = 256;
constexpr int kATile = kBM * kRowB;  // 4 KB activation stage
constexpr int kMaxRank = 512;

inline hipStream_t cross_stream() {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

// XOR-swizzle of the 16-B slots inside a row of rb bytes (rb % 64 == 0).
__device__ __forceinline__ int cswz(int row, int byte_in_row, int rb) {
  return byte_in_row ^ (((row & 7) << 4) & (rb - 16));
}

// This thread's share of a [ROWS, 64] bf16 tile of a row-major matrix with
// leading dimension ld: rows [r0, r0 + ROWS) clipped to rmax, columns
// [k0, k0 + 64) clipped to kmax. Clipped chunks read as zero, never as memory.
template <int ROWS>
__device__ __forceinline__ void tile_gload(const __bf16* __restrict__ src, int64_t ld,
                                           int64_t r0, int64_t rmax, int k0, int kmax,
                                           cu32x4 (&v)[ROWS * 8 / kCThreads]) {
#pragma unroll
  for (int i = 0; i < ROWS * 8 / kCThreads; ++i) {
    const int c = ctid() + i * kCThreads;
    const int row = c >> 3, kc = (c & 7) * 8;
    v[i] = (r0 + row < rmax && k0 + kc < kmax)
               ? *reinterpret_cast<const cu32x4*>(src + (r0 + row) * ld + k0 + kc)
               : cu32x4{0u, 0u, 0u, 0u};
  }
}

template <int ROWS>
__device__ __forceinline__ void tile_sstore(char* tile, const cu32x4 (&v)[ROWS * 8 / kCThreads]) {
#pragma unroll
  for (int i = 0; i < ROWS * 8 / kCThreads; ++i) {
    const int c = ctid() + i * kCThreads;
    const int row = c >> 3;
    *reinterpret_cast<cu32x4*>(tile + row * kRowB + cswz(row, (c & 7) * 16, kRowB)) = v[i];
  }
}

__device__ __forceinline__ cbf16x8 frag(const char* tile, int rb, int row, int kbyte) {
  return *reinterpret_cast<const cbf16x8*>(tile + row * rb + cswz(row, kbyte, rb));
}

// acc[mi][ni] += W_tile(ni) x A(mi)^T over nsub 32-wide k sub-steps.
// a: activation rows 0..31 (row bytes a_rb, k starting at byte a_k);
// wt: staged weight tile, this wave's rows start at wrow0; ntv of the NT
// 16-column tiles are inside the matrix (wave-uniform).
template <int NT>
__device__ __forceinline__ void mma_step(cf32x4 (&acc)[2][NT], const char* a, int a_rb,
                                         int a_k, const char* wt, int wrow0, int ntv,
                                         int nsub, int l) {
  for (int kk = 0; kk < nsub; ++kk) {
    const int kb = kk * 64 + ((l >> 4) << 4);
    const cbf16x8 a0 = frag(a, a_rb, l & 15, a_k + kb);
    const cbf16x8 a1 = frag(a, a_rb, 16 + (l & 15), a_k + kb);
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      if (ni < ntv) {
        const cbf16x8 wf = frag(wt, kRowB, wrow0 + ni * 16 + (l & 15), kb);
        acc[0][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, a0, acc[0][ni], 0, 0, 0);
        acc[1][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, a1, acc[1][ni], 0, 0, 0);
      }
    }
  }
}

template <int NT>
__device__ __forceinline__ void zero_acc(cf32x4 (&acc)[2][NT]) {
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = cf32x4{0.f, 0.f, 0.f, 0.f};
}

// Round a wave's accumulators to bf16 (the ONE rounding of t / dt) into the
// [32, r] LDS slice; cbase is the wave's first column.
template <int NT>
__device__ __forceinline__ void acc_to_slice(const cf32x4 (&acc)[2][NT], char* slice, int rb,
                                             int cbase, int ntv, int l) {
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      if (ni < ntv) {
        const int row = mi * 16 + (l & 15);
        const int col = cbase + ni * 16 + ((l >> 4) << 2);
        cbf16x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = static_cast<__bf16>(acc[mi][ni][i]);
        *reinterpret_cast<cbf16x4*>(slice + row * rb + cswz(row, col * 2, rb)) = v;
      }
    }
}

// LDS slice -> global [B, r] rows of this workgroup (the same bf16 values).
__device__ __forceinline__ void slice_to_global(const char* slice, int r, int64_t row0,
                                                int64_t B, __bf16* __restrict__ dst) {
  const int cpr = r >> 3, rb = r * 2;
  for (int c = ctid(); c < kBM * cpr; c += kCThreads) {
    const int row = c / cpr, kc = c - row * cpr;
    if (row0 + row < B)
      *reinterpret_cast<cu32x4*>(dst + (row0 + row) * r + kc * 8) =
          *reinterpret_cast<const cu32x4*>(slice + row * rb + cswz(row, kc * 16, rb));
  }
}

__device__ __forceinline__ void global_to_slice(const __bf16* __restrict__ src, int r,
                                                int64_t row0, int64_t B, char* slice) {
  const int cpr = r >> 3, rb = r * 2;
  for (int c = ctid(); c < kBM * cpr; c += kCThreads) {
    const int row = c / cpr, kc = c - row * cpr;
    *reinterpret_cast<cu32x4*>(slice + row * rb + cswz(row, kc * 16, rb)) =
        (row0 + row < B) ? *reinterpret_cast<const cu32x4*>(src + (row0 + row) * r + kc * 8)
                         : cu32x4{0u, 0u, 0u, 0u};
  }
}

__device__ __forceinline__ cf32x4 bf4_to_f4(const __bf16* p) {
  const cbf16x4 v = *reinterpret_cast<const cbf16x4*>(p);
  return cf32x4{static_cast<float>(v[0]), static_cast<float>(v[1]), static_cast<float>(v[2]),
                static_cast<float>(v[3])};
}

// Phase 1 of both kernels: slice[32, r] = bf16(A W1^T) with K = N, where A is
// x_l (PRODUCT = false) or bf16(g * x_0) (PRODUCT = true; a is g, a2 is x_0
// and the product is also stored to u_out on the first column pass).
// w1 is [r, N] row-major. stage: 2 x (4 KB + 32 KB).
template <bool PRODUCT>
__device__ __forceinline__ void rank_phase(const __bf16* __restrict__ a,
                                           const __bf16* __restrict__ a2,
                                           const __bf16* __restrict__ w1, int64_t row0, int64_t B,
                                           int N, int r, char* slice, char* stage,
                                           __bf16* __restrict__ u_out) {
  constexpr int NT = 4, NC = 256, WT = NC * kRowB, BUF = kATile + WT;
  const int l = ctid() & 63, w = ctid() >> 6;
  const int nk = (N + kKT - 1) / kKT;
  const int steps = nk * ((r + NC - 1) / NC);
  cu32x4 ra[1], ra2[1], rw[8];

  auto fetch = [&](int s) {
    const int ch = s / nk, k0 = (s - ch * nk) * kKT;
    tile_gload<kBM>(a, N, row0, B, k0, N, ra);
    if (PRODUCT) tile_gload<kBM>(a2, N, row0, B, k0, N, ra2);
    tile_gload<NC>(w1, N, ch * NC, r, k0, N, rw);
  };
  auto commit = [&](int s) {
    char* buf = stage + (s & 1) * BUF;
    if (PRODUCT) {
      const cbf16x8 g8 = *reinterpret_cast<const cbf16x8*>(&ra[0]);
      const cbf16x8 x8 = *reinterpret_cast<const cbf16x8*>(&ra2[0]);
      cbf16x8 u8;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        u8[e] = static_cast<__bf16>(static_cast<float>(g8[e]) * static_cast<float>(x8[e]));
      ra[0] = *reinterpret_cast<const cu32x4*>(&u8);
      const int ch = s / nk, k0 = (s - ch * nk) * kKT;
      const int row = ctid() >> 3, kc = (ctid() & 7) * 8;
      if (ch == 0 && row0 + row < B && k0 + kc < N)
        *reinterpret_cast<cu32x4*>(u_out + (row0 + row) * N + k0 + kc) = ra[0];
    }
    tile_sstore<kBM>(buf, ra);
    tile_sstore<NC>(buf + kATile, rw);
  };

  cf32x4 acc[2][NT];
  zero_acc(acc);
  fetch(0);
  commit(0);
  csync();
  for (int s = 0; s < steps; ++s) {
    const int ch = s / nk, ks = s - ch * nk;
    if (s + 1 < steps) fetch(s + 1);
    const char* buf = stage + (s & 1) * BUF;
    const int cbase = ch * NC + w * (NT * 16);
    const int ntv = cmin(NT, cmax(0, (r - cbase) >> 4));
    mma_step<NT>(acc, buf, kRowB, 0, buf + kATile, w * (NT * 16), ntv,
                 cmin(2, (N - ks * kKT) >> 5), l);
    if (ks == nk - 1) {
      acc_to_slice<NT>(acc, slice, r * 2, cbase, ntv, l);
      zero_acc(acc);
    }
    if (s + 1 < steps) commit(s + 1);
    csync();
  }
}

__global__ void __launch_bounds__(kCThreads) lowrank_cross_fwd_kernel(
    const __bf16* __restrict__ x0, const __bf16* __restrict__ xl,
    const __bf16* __restrict__ V,  // [r, N]
    const __bf16* __restrict__ W,  // [N, r]
    const float* __restrict__ bias, int64_t B, int N, int r, __bf16* __restrict__ y,
    __bf16* __restrict__ t_out /* [B, r] or nullptr */) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int NT = 4, NC = 256, WT = NC * kRowB;
  const int l = ctid() & 63, w = ctid() >> 6;
  const int64_t row0 = static_cast<int64_t>(__builtin_amdgcn_workgroup_id_x()) * kBM;
  const int rb = r * 2;
  char* slice = lds;
  char* stage = lds + kBM * rb;

  rank_phase<false>(xl, nullptr, V, row0, B, N, r, slice, stage, nullptr);
  if (t_out != nullptr) slice_to_global(slice, r, row0, B, t_out);

  // phase 2: y[:, pass] = x_0 * (t W^T + b) + x_l, K = r from the slice
  const int nk = (r + kKT - 1) / kKT;
  const int steps = nk * ((N + NC - 1) / NC);
  cu32x4 rw[8];
  auto fetch = [&](int s) {
    const int ch = s / nk;
    tile_gload<NC>(W, r, ch * NC, N, (s - ch * nk) * kKT, r, rw);
  };
  cf32x4 acc[2][NT];
  zero_acc(acc);
  fetch(0);
  tile_sstore<NC>(stage, rw);
  csync();
  for (int s = 0; s < steps; ++s) {
    const int ch = s / nk, ks = s - ch * nk;
    if (s + 1 < steps) fetch(s + 1);
    const int cbase = ch * NC + w * (NT * 16);
    const int ntv = cmin(NT, cmax(0, (N - cbase) >> 4));
    mma_step<NT>(acc, slice, rb, ks * kRowB, stage + (s & 1) * WT, w * (NT * 16), ntv,
                 cmin(2, (r - ks * kKT) >> 5), l);
    if (ks == nk - 1) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
          const int64_t row = row0 + mi * 16 + (l & 15);
          const int col = cbase + ni * 16 + ((l >> 4) << 2);
          if (ni < ntv && row < B) {
            const int64_t off = row * N + col;
            const cf32x4 a0 = bf4_to_f4(x0 + off), al = bf4_to_f4(xl + off);
            const cf32x4 bb = *reinterpret_cast<const cf32x4*>(bias + col);
            cbf16x4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i)
              o[i] = static_cast<__bf16>(a0[i] * (acc[mi][ni][i] + bb[i]) + al[i]);
            *reinterpret_cast<cbf16x4*>(y + off) = o;
          }
        }
      zero_acc(acc);
    }
    if (s + 1 < steps) tile_sstore<NC>(stage + ((s + 1) & 1) * WT, rw);
    csync();
  }
}

__global__ void __launch_bounds__(kCThreads) lowrank_cross_bwd_kernel(
    const __bf16* __restrict__ g, const __bf16* __restrict__ x0,
    const __bf16* __restrict__ t,   // [B, r] saved by the forward
    const __bf16* __restrict__ Wt,  // [r, N] = W^T
    const __bf16* __restrict__ Vt,  // [N, r] = V^T
    const __bf16* __restrict__ W,   // [N, r]
    const float* __restrict__ bias, int64_t B, int N, int r, __bf16* __restrict__ dxl,
    __bf16* __restrict__ u_out, __bf16* __restrict__ dt_out, float* __restrict__ dx0_acc) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int NT = 2, NC = 128, WT = NC * kRowB;  // phase B: two weight tiles per step
  const int l = ctid() & 63, w = ctid() >> 6;
  const int64_t row0 = static_cast<int64_t>(__builtin_amdgcn_workgroup_id_x()) * kBM;
  const int rb = r * 2;
  char* dts = lds;
  char* ts = lds + kBM * rb;
  char* stage = ts + kBM * rb;

  global_to_slice(t, r, row0, B, ts);
  rank_phase<true>(g, x0, Wt, row0, B, N, r, dts, stage, u_out);
  slice_to_global(dts, r, row0, B, dt_out);

  // phase B: per 128-column pass, p = dt V (rows of V^T) and q = t W^T (rows
  // of W), both K = r; stage buffer = [V^T tile | W tile] x 2
  const int nk = (r + kKT - 1) / kKT;
  const int steps = nk * ((N + NC - 1) / NC);
  cu32x4 rv[4], rw[4];
  auto fetch = [&](int s) {
    const int ch = s / nk, k0 = (s - ch * nk) * kKT;
    tile_gload<NC>(Vt, r, ch * NC, N, k0, r, rv);
    tile_gload<NC>(W, r, ch * NC, N, k0, r, rw);
  };
  auto commit = [&](int s) {
    char* buf = stage + (s & 1) * (2 * WT);
    tile_sstore<NC>(buf, rv);
    tile_sstore<NC>(buf + WT, rw);
  };
  cf32x4 p[2][NT], q[2][NT];
  zero_acc(p);
  zero_acc(q);
  fetch(0);
  commit(0);
  csync();
  for (int s = 0; s < steps; ++s) {
    const int ch = s / nk, ks = s - ch * nk;
    if (s + 1 < steps) fetch(s + 1);
    const char* buf = stage + (s & 1) * (2 * WT);
    const int cbase = ch * NC + w * (NT * 16);
    const int ntv = cmin(NT, cmax(0, (N - cbase) >> 4));
    const int nsub = cmin(2, (r - ks * kKT) >> 5);
    mma_step<NT>(p, dts, rb, ks * kRowB, buf, w * (NT * 16), ntv, nsub, l);
    mma_step<NT>(q, ts, rb, ks * kRowB, buf + WT, w * (NT * 16), ntv, nsub, l);
    if (ks == nk - 1) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
          const int64_t row = row0 + mi * 16 + (l & 15);
          const int col = cbase + ni * 16 + ((l >> 4) << 2);
          if (ni < ntv && row < B) {
            const int64_t off = row * N + col;
            const cf32x4 gg = bf4_to_f4(g + off);
            const cf32x4 bb = *reinterpret_cast<const cf32x4*>(bias + col);
            cf32x4 d0 = *reinterpret_cast<const cf32x4*>(dx0_acc + off);
            cbf16x4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              o[i] = static_cast<__bf16>(gg[i] + p[mi][ni][i]);
              d0[i] += gg[i] * (q[mi][ni][i] + bb[i]);
            }
            *reinterpret_cast<cbf16x4*>(dxl + off) = o;
            *reinterpret_cast<cf32x4*>(dx0_acc + off) = d0;
          }
        }
      zero_acc(p);
      zero_acc(q);
    }
    if (s + 1 < steps) commit(s + 1);
    csync();
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

const __bf16* bfp(const at::Tensor& t) {
  return reinterpret_cast<const __bf16*>(t.data_ptr<at::BFloat16>());
}
__bf16* bfp_mut(at::Tensor& t) { return reinterpret_cast<__bf16*>(t.data_ptr<at::BFloat16>()); }

// both kernels may ask for more than the 64 KB default of dynamic LDS; raise
// the cap once per process (not per launch, so nothing but the launch itself
// happens inside a graph capture)
void allow_big_lds() {
  static const bool once = [] {
    TREC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(lowrank_cross_fwd_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kLdsBytesPerCU));
    TREC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(lowrank_cross_bwd_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kLdsBytesPerCU));
    return true;
  }();
  (void)once;
}

void check_cross_shapes(const at::Tensor& x0, const at::Tensor& xl, const at::Tensor& V,
                        const at::Tensor& W, const at::Tensor& b) {
  TORCH_CHECK(x0.is_cuda() && x0.dim() == 2 && xl.sizes() == x0.sizes(),
              "lowrank_cross: x0/xl must be matching [B, N] GPU tensors");
  const int64_t N = x0.size(1), r = V.dim() == 2 ? V.size(0) : -1;
  TORCH_CHECK(V.dim() == 2 && V.size(1) == N && W.dim() == 2 && W.size(0) == N &&
                  W.size(1) == r && b.numel() == N,
              "lowrank_cross: need V [r, N], W [N, r], b [N]");
  TORCH_CHECK(x0.scalar_type() == at::kBFloat16 && xl.scalar_type() == at::kBFloat16 &&
                  V.scalar_type() == at::kBFloat16 && W.scalar_type() == at::kBFloat16,
              "lowrank_cross: bf16 operands only");
  TORCH_CHECK(N % 32 == 0 && N > 0, "lowrank_cross needs N % 32 == 0");
  TORCH_CHECK(r % 32 == 0 && r >= 32 && r <= kMaxRank,
              "lowrank_cross needs r % 32 == 0, 32 <= r <= 512");
}

}  // namespace

std::tuple<at::Tensor, at::Tensor> lowrank_cross_fwd(const at::Tensor& x0, const at::Tensor& xl,
                                                     const at::Tensor& V, const at::Tensor& W,
                                                     const at::Tensor& b, bool save_t) {
  check_cross_shapes(x0, xl, V, W, b);
  const int64_t B = x0.size(0);
  const int N = x0.size(1), r = V.size(0);
  auto y = at::empty({B, N}, x0.options());
  auto t = at::empty({save_t ? B : 0, r}, x0.options());
  if (B == 0) return {y, t};
  auto x0c = x0.contiguous(), xlc = xl.contiguous(), Vc = V.contiguous(), Wc = W.contiguous();
  auto bf = b.to(at::kFloat).contiguous();
  const int lds_bytes = kBM * r * 2 + 2 * (kATile + 256 * kRowB);
  static_assert(kBM * kMaxRank * 2 + 2 * (kATile + 256 * kRowB) <= kLdsBytesPerCU);
  allow_big_lds();
  hipLaunchKernelGGL(lowrank_cross_fwd_kernel, dim3((B + kBM - 1) / kBM), dim3(kCThreads),
                     lds_bytes, cross_stream(), bfp(x0c), bfp(xlc), bfp(Vc), bfp(Wc),
                     bf.data_ptr<float>(), B, N, r, bfp_mut(y), save_t ? bfp_mut(t) : nullptr);
  TREC_HIP_CHECK(hipGetLastError());
  return {y, t};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> lowrank_cross_bwd(
    const at::Tensor& g, const at::Tensor& x0, const at::Tensor& xl, const at::Tensor& t,
    const at::Tensor& V, const at::Tensor& W, const at::Tensor& b, at::Tensor dx0_acc) {
  check_cross_shapes(x0, xl, V, W, b);
  const int64_t B = x0.size(0);
  const int N = x0.size(1), r = V.size(0);
  TORCH_CHECK(g.sizes() == x0.sizes() && g.scalar_type() == at::kBFloat16,
              "lowrank_cross_bwd: g must be bf16 [B, N]");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == B && t.size(1) == r &&
                  t.scalar_type() == at::kBFloat16,
              "lowrank_cross_bwd: t must be the bf16 [B, r] the forward saved");
  TORCH_CHECK(dx0_acc.sizes() == x0.sizes() && dx0_acc.scalar_type() == at::kFloat &&
                  dx0_acc.is_contiguous() && dx0_acc.is_cuda(),
              "lowrank_cross_bwd: dx0_acc must be a contiguous fp32 [B, N] buffer");
  auto dxl = at::empty({B, N}, x0.options());
  auto u = at::empty({B, N}, x0.options());
  auto dt = at::empty({B, r}, x0.options());
  if (B == 0) return {dxl, u, dt};
  auto gc = g.contiguous(), x0c = x0.contiguous(), tc = t.contiguous();
  // K-contiguous copies for the two products that contract the other index
  auto Wt = W.t().contiguous(), Vt = V.t().contiguous(), Wc = W.contiguous();
  auto bf = b.to(at::kFloat).contiguous();
  const int lds_bytes = 2 * kBM * r * 2 + 2 * (kATile + 256 * kRowB);
  static_assert(2 * kBM * kMaxRank * 2 + 2 * (kATile + 256 * kRowB) <= kLdsBytesPerCU);
  static_assert(2 * 2 * 128 * kRowB <= 2 * (kATile + 256 * kRowB));
  allow_big_lds();
  hipLaunchKernelGGL(lowrank_cross_bwd_kernel, dim3((B + kBM - 1) / kBM), dim3(kCThreads),
                     lds_bytes, cross_stream(), bfp(gc), bfp(x0c), bfp(tc), bfp(Wt), bfp(Vt),
                     bfp(Wc), bf.data_ptr<float>(), B, N, r, bfp_mut(dxl), bfp_mut(u),
                     bfp_mut(dt), dx0_acc.data_ptr<float>());
  TREC_HIP_CHECK(hipGetLastError());
  return {dxl, u, dt};
}

}  // namespace trec_amd
