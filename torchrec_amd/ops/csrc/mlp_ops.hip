// Fused MLP backward helpers for MI355X (gfx950).
//
// relu_bwd_colsum_partial: one pass over dY producing BOTH the relu-masked
// gradient g = dY * (y > 0) and a small fp32 [G, N] table of bias-gradient
// partials (block-cooperative: 8 column lanes x 32 row lanes, LDS fold, one
// partial row per block, G*N*4 B <= 256 KB). Replaces torch's separate
// compare + mul + column reduce (three dY-sized passes) with one. 16-bit
// dtypes move as 8-element (16 B) vectors per lane (Guideline 13: scalar
// bf16 loads are ~2.5x slower).
// splitk_fold_bias: sums the S split-K wgrad chunks AND folds the partial
// table into db in one launch (trailing blocks), so a ReLU layer's backward
// tail is two kernels. relu_bwd_col_sum (non-split path) = partial kernel +
// one cast-fused final fold. All reduction orders are fixed: bitwise
// repeatable, no atomics, no counters.

#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <cstdint>
#include <type_traits>

#include "common.h"

namespace trec_amd {

static inline hipStream_t mlp_stream() {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

// ---------------------------------------------------------------------------
// relu mask + bias-grad partials. A 256-thread block owns a column tile of
// kColLanes * VPT columns and a contiguous group of rows; thread (rl, cl)
// owns one 16 B column vector and visits rows rl, rl + 32, ... of the group,
// kRowUnroll rows of loads in flight. A wave covers 8 rows x 128 B.
// ---------------------------------------------------------------------------
constexpr int kColLanes = 8;
constexpr int kRowLanes = kBlockThreads / kColLanes;  // 32
constexpr int kRowUnroll = 4;
constexpr int kMaxGroups = 256;                  // blockIdx.y range, fold depth
constexpr int64_t kPartialElems = 256 * 1024 / 4;  // G * N <= 64 Ki floats

template <typename scalar_t, int VPT, bool VEC>
__global__ void __launch_bounds__(kBlockThreads) relu_bwd_colsum_partial_kernel(
    const scalar_t* __restrict__ dy, const scalar_t* __restrict__ y, int64_t M,
    int64_t N, int64_t rows_per_group, scalar_t* __restrict__ g,
    float* __restrict__ partial /* [gridDim.y, N] */) {
  constexpr int TILE_N = kColLanes * VPT;
  __shared__ float red[kRowLanes][TILE_N];
  const int cl = threadIdx.x % kColLanes;
  const int rl = threadIdx.x / kColLanes;
  const int64_t c0 = static_cast<int64_t>(blockIdx.x) * TILE_N + cl * VPT;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rows_per_group;
  const int64_t r1 = min(M, r0 + rows_per_group);
  float acc[VPT];
#pragma unroll
  for (int v = 0; v < VPT; ++v) acc[v] = 0.f;
  if (c0 < N) {
    if constexpr (VEC) {
      // N % VPT == 0 and 16 B-aligned bases: every chunk is whole and aligned
      for (int64_t r = r0 + rl; r < r1; r += kRowLanes * kRowUnroll) {
        uint4 qy[kRowUnroll], qd[kRowUnroll];
#pragma unroll
        for (int u = 0; u < kRowUnroll; ++u) {
          const int64_t rr = r + u * kRowLanes;
          qy[u] = make_uint4(0, 0, 0, 0);
          qd[u] = make_uint4(0, 0, 0, 0);
          if (rr < r1) {
            qy[u] = *reinterpret_cast<const uint4*>(y + rr * N + c0);
            qd[u] = *reinterpret_cast<const uint4*>(dy + rr * N + c0);
          }
        }
#pragma unroll
        for (int u = 0; u < kRowUnroll; ++u) {
          const int64_t rr = r + u * kRowLanes;
          if (rr < r1) {
            const scalar_t* py = reinterpret_cast<const scalar_t*>(&qy[u]);
            const scalar_t* pd = reinterpret_cast<const scalar_t*>(&qd[u]);
            uint4 qo;
            scalar_t* po = reinterpret_cast<scalar_t*>(&qo);
#pragma unroll
            for (int v = 0; v < VPT; ++v) {
              float gv = (emb2float(py[v]) > 0.f) ? emb2float(pd[v]) : 0.f;
              po[v] = float2emb(gv, scalar_t{});
              acc[v] += gv;
            }
            *reinterpret_cast<uint4*>(g + rr * N + c0) = qo;
          }
        }
      }
    } else {
      // scalar tail path: N % VPT != 0 (row bases lose 16 B alignment)
      for (int64_t r = r0 + rl; r < r1; r += kRowLanes) {
        const int64_t base = r * N + c0;
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
          if (c0 + v < N) {
            float gv = (emb2float(y[base + v]) > 0.f) ? emb2float(dy[base + v]) : 0.f;
            g[base + v] = float2emb(gv, scalar_t{});
            acc[v] += gv;
          }
        }
      }
    }
  }
#pragma unroll
  for (int v = 0; v < VPT; ++v) red[rl][cl * VPT + v] = acc[v];
  __syncthreads();
  // fixed-order fold of the 32 row lanes: one partial row per block
  if (threadIdx.x < TILE_N) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * TILE_N + threadIdx.x;
    if (c < N) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < kRowLanes; ++k) s += red[k][threadIdx.x];
      partial[static_cast<int64_t>(blockIdx.y) * N + c] = s;
    }
  }
}

// Fold one 16-column tile of the [G, N] partial table into db: 16 row lanes
// each sum rows rl, rl + 16, ... in ascending order, then lane 0 folds the 16
// lane sums through LDS in ascending order. Whole block must call this.
constexpr int kFoldCols = 16;
constexpr int kFoldRows = kBlockThreads / kFoldCols;  // 16

template <typename o_t>
__device__ __forceinline__ void fold_partial_tile(
    const float* __restrict__ partial, int G, int64_t N, int64_t tile,
    o_t* __restrict__ db, float (*red)[kFoldCols]) {
  const int cl = threadIdx.x % kFoldCols;
  const int rl = threadIdx.x / kFoldCols;
  const int64_t c = tile * kFoldCols + cl;
  float acc = 0.f;
  if (c < N) {
#pragma unroll 4
    for (int grp = rl; grp < G; grp += kFoldRows)
      acc += partial[static_cast<int64_t>(grp) * N + c];
  }
  red[rl][cl] = acc;
  __syncthreads();
  if (rl == 0 && c < N) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kFoldRows; ++k) s += red[k][cl];
    db[c] = float2emb(s, o_t{});
  }
}

template <typename o_t>
__global__ void __launch_bounds__(kBlockThreads) colsum_final_cast_kernel(
    const float* __restrict__ partial, int G, int64_t N, o_t* __restrict__ out) {
  __shared__ float red[kFoldRows][kFoldCols];
  fold_partial_tile<o_t>(partial, G, N, blockIdx.x, out, red);
}

// Split-K chunk sum + bias-grad fold in one launch. Blocks [0, sum_blocks)
// sum the S chunks of parts [S, E] elementwise (fp32 accumulate in chunk
// order, one rounding); blocks [sum_blocks, gridDim.x) each fold one column
// tile of partial [G, N] into db.
constexpr int kChunkUnroll = 8;

template <typename scalar_t, int VPT, bool VEC>
__global__ void __launch_bounds__(kBlockThreads) splitk_fold_bias_kernel(
    const scalar_t* __restrict__ parts, int S, int64_t E,
    scalar_t* __restrict__ dw, int sum_blocks, const float* __restrict__ partial,
    int G, int64_t N, scalar_t* __restrict__ db) {
  __shared__ float red[kFoldRows][kFoldCols];
  if (static_cast<int>(blockIdx.x) >= sum_blocks) {
    fold_partial_tile<scalar_t>(partial, G, N, blockIdx.x - sum_blocks, db, red);
    return;
  }
  const int64_t chunks = (E + VPT - 1) / VPT;
  for (int64_t it = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       it < chunks; it += static_cast<int64_t>(sum_blocks) * blockDim.x) {
    const int64_t base = it * VPT;
    float acc[VPT];
#pragma unroll
    for (int v = 0; v < VPT; ++v) acc[v] = 0.f;
    if constexpr (VEC) {
      // E % VPT == 0 and 16 B-aligned bases
      for (int s0 = 0; s0 < S; s0 += kChunkUnroll) {
        uint4 q[kChunkUnroll];
#pragma unroll
        for (int u = 0; u < kChunkUnroll; ++u) {
          q[u] = make_uint4(0, 0, 0, 0);
          if (s0 + u < S)
            q[u] = *reinterpret_cast<const uint4*>(
                parts + static_cast<int64_t>(s0 + u) * E + base);
        }
#pragma unroll
        for (int u = 0; u < kChunkUnroll; ++u) {
          if (s0 + u < S) {
            const scalar_t* p = reinterpret_cast<const scalar_t*>(&q[u]);
#pragma unroll
            for (int v = 0; v < VPT; ++v) acc[v] += emb2float(p[v]);
          }
        }
      }
      uint4 qo;
      scalar_t* po = reinterpret_cast<scalar_t*>(&qo);
#pragma unroll
      for (int v = 0; v < VPT; ++v) po[v] = float2emb(acc[v], scalar_t{});
      *reinterpret_cast<uint4*>(dw + base) = qo;
    } else {
      for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int v = 0; v < VPT; ++v)
          if (base + v < E) acc[v] += emb2float(parts[static_cast<int64_t>(s) * E + base + v]);
      }
#pragma unroll
      for (int v = 0; v < VPT; ++v)
        if (base + v < E) dw[base + v] = float2emb(acc[v], scalar_t{});
    }
  }
}

static inline bool aligned16(const void* p) {
  return reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

// launches the partial kernel; dy / yc / g contiguous [M, N], M, N > 0.
// Returns partial [G, N] fp32 with G = min(256, 64Ki / N, row tiles).
static at::Tensor launch_relu_bwd_partial(const at::Tensor& dy, const at::Tensor& yc,
                                          at::Tensor& g) {
  const int64_t M = dy.size(0), N = dy.size(1);
  const int64_t row_tiles = (M + kRowLanes - 1) / kRowLanes;
  int64_t G = std::min<int64_t>(kMaxGroups, std::max<int64_t>(1, kPartialElems / N));
  G = std::max<int64_t>(1, std::min(G, row_tiles));
  // whole row tiles per group, then drop groups left empty by the rounding
  const int64_t rows_per_group = (row_tiles + G - 1) / G * kRowLanes;
  G = (M + rows_per_group - 1) / rows_per_group;
  auto partial = at::empty({G, N}, dy.options().dtype(at::kFloat));
  auto stream = mlp_stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(at::kHalf, at::kBFloat16, dy.scalar_type(),
                                  "relu_bwd_colsum_partial", [&] {
    if constexpr (std::is_same_v<scalar_t, double>) {
      TORCH_CHECK(false, "fp64 unsupported");
    } else {
      using dev_t = typename DevType<scalar_t>::type;
      constexpr int VPT = 16 / sizeof(dev_t);
      const int64_t col_tiles = (N + kColLanes * VPT - 1) / (kColLanes * VPT);
      TORCH_CHECK(col_tiles <= INT32_MAX, "relu_bwd_colsum_partial: N too large");
      const dev_t* pdy = reinterpret_cast<const dev_t*>(dy.data_ptr<scalar_t>());
      const dev_t* py = reinterpret_cast<const dev_t*>(yc.data_ptr<scalar_t>());
      dev_t* pg = reinterpret_cast<dev_t*>(g.data_ptr<scalar_t>());
      dim3 grid(static_cast<unsigned>(col_tiles), static_cast<unsigned>(G));
      const bool vec = N % VPT == 0 && aligned16(pdy) && aligned16(py) && aligned16(pg);
      if (vec) {
        hipLaunchKernelGGL((relu_bwd_colsum_partial_kernel<dev_t, VPT, true>), grid,
                           dim3(kBlockThreads), 0, stream, pdy, py, M, N,
                           rows_per_group, pg, partial.data_ptr<float>());
      } else {
        hipLaunchKernelGGL((relu_bwd_colsum_partial_kernel<dev_t, VPT, false>), grid,
                           dim3(kBlockThreads), 0, stream, pdy, py, M, N,
                           rows_per_group, pg, partial.data_ptr<float>());
      }
    }
  });
  return partial;
}

static void check_relu_bwd_args(const at::Tensor& grad_out, const at::Tensor& y) {
  TORCH_CHECK(grad_out.dim() == 2 && grad_out.is_cuda() && y.is_cuda());
  TORCH_CHECK(grad_out.sizes() == y.sizes() && grad_out.scalar_type() == y.scalar_type());
}

std::tuple<at::Tensor, at::Tensor> relu_bwd_colsum_partial(const at::Tensor& grad_out,
                                                           const at::Tensor& y) {
  check_relu_bwd_args(grad_out, y);
  int64_t M = grad_out.size(0), N = grad_out.size(1);
  auto dy = grad_out.contiguous();
  auto yc = y.contiguous();
  auto g = at::empty_like(dy);
  if (M == 0 || N == 0)
    return {g, at::empty({0, N}, dy.options().dtype(at::kFloat))};
  auto partial = launch_relu_bwd_partial(dy, yc, g);
  return {g, partial};
}

std::tuple<at::Tensor, at::Tensor> relu_bwd_col_sum(const at::Tensor& grad_out,
                                                    const at::Tensor& y) {
  check_relu_bwd_args(grad_out, y);
  int64_t M = grad_out.size(0), N = grad_out.size(1);
  auto dy = grad_out.contiguous();
  auto yc = y.contiguous();
  auto g = at::empty_like(dy);
  auto db = at::empty({N}, dy.options());  // bias grad in the grad dtype
  if (M == 0 || N == 0) {
    db.zero_();
    return {g, db};
  }
  auto partial = launch_relu_bwd_partial(dy, yc, g);
  auto stream = mlp_stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(at::kHalf, at::kBFloat16, dy.scalar_type(),
                                  "relu_bwd_col_sum", [&] {
    if constexpr (std::is_same_v<scalar_t, double>) {
      TORCH_CHECK(false, "fp64 unsupported");
    } else {
      using dev_t = typename DevType<scalar_t>::type;
      int ftiles = (int)((N + kFoldCols - 1) / kFoldCols);
      hipLaunchKernelGGL((colsum_final_cast_kernel<dev_t>), dim3(ftiles),
                         dim3(kBlockThreads), 0, stream, partial.data_ptr<float>(),
                         (int)partial.size(0), N,
                         reinterpret_cast<dev_t*>(db.data_ptr<scalar_t>()));
    }
  });
  return {g, db};
}

// parts [S, N, K] (the split-K bmm output), partial [G, N] fp32 ->
// dW [N, K] = sum_s parts[s], db [N] = sum_g partial[g], both in parts' dtype.
std::tuple<at::Tensor, at::Tensor> splitk_fold_bias(const at::Tensor& parts,
                                                    const at::Tensor& partial) {
  TORCH_CHECK(parts.dim() == 3 && parts.is_cuda() && partial.is_cuda());
  TORCH_CHECK(partial.dim() == 2 && partial.scalar_type() == at::kFloat);
  TORCH_CHECK(partial.size(1) == parts.size(1),
              "splitk_fold_bias: partial [G, N] must match parts [S, N, K]");
  auto pc = parts.contiguous();
  auto pp = partial.contiguous();
  const int64_t S = pc.size(0), N = pc.size(1), K = pc.size(2);
  const int64_t G = pp.size(0);
  TORCH_CHECK(S <= INT32_MAX && G <= INT32_MAX);
  auto dw = at::empty({N, K}, pc.options());
  auto db = at::empty({N}, pc.options());
  if (N == 0) return {dw, db};
  const int64_t E = N * K;
  auto stream = mlp_stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(at::kHalf, at::kBFloat16, pc.scalar_type(),
                                  "splitk_fold_bias", [&] {
    if constexpr (std::is_same_v<scalar_t, double>) {
      TORCH_CHECK(false, "fp64 unsupported");
    } else {
      using dev_t = typename DevType<scalar_t>::type;
      constexpr int VPT = 16 / sizeof(dev_t);
      const int64_t chunks = (E + VPT - 1) / VPT;
      const int sum_blocks = E > 0 ? grid_for(chunks, kBlockThreads) : 0;
      const int64_t fold_blocks = (N + kFoldCols - 1) / kFoldCols;
      TORCH_CHECK(fold_blocks <= INT32_MAX - sum_blocks, "splitk_fold_bias: N too large");
      const dev_t* pin = reinterpret_cast<const dev_t*>(pc.data_ptr<scalar_t>());
      dev_t* pdw = reinterpret_cast<dev_t*>(dw.data_ptr<scalar_t>());
      dev_t* pdb = reinterpret_cast<dev_t*>(db.data_ptr<scalar_t>());
      dim3 grid(static_cast<unsigned>(sum_blocks + fold_blocks));
      const bool vec = E % VPT == 0 && aligned16(pin) && aligned16(pdw);
      if (vec) {
        hipLaunchKernelGGL((splitk_fold_bias_kernel<dev_t, VPT, true>), grid,
                           dim3(kBlockThreads), 0, stream, pin, (int)S, E, pdw,
                           sum_blocks, pp.data_ptr<float>(), (int)G, N, pdb);
      } else {
        hipLaunchKernelGGL((splitk_fold_bias_kernel<dev_t, VPT, false>), grid,
                           dim3(kBlockThreads), 0, stream, pin, (int)S, E, pdw,
                           sum_blocks, pp.data_ptr<float>(), (int)G, N, pdb);
      }
    }
  });
  return {dw, db};
}

// relu mask only: g = dy * (y > 0) — one vectorized pass; the bias grad
// comes out of the wgrad GEMM's BGRADB epilogue (lt_gemm.hip), so the
// column-sum machinery is skipped entirely on that path.
template <typename scalar_t, int VPT>
__global__ void __launch_bounds__(kBlockThreads) relu_bwd_mask_kernel(
    const scalar_t* __restrict__ dy, const scalar_t* __restrict__ y, int64_t n,
    scalar_t* __restrict__ g) {
  const int64_t chunks = (n + VPT - 1) / VPT;
  for (int64_t it = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       it < chunks; it += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t base = it * VPT;
    if (base + VPT <= n) {
      uint4 qy = *reinterpret_cast<const uint4*>(y + base);
      uint4 qd = *reinterpret_cast<const uint4*>(dy + base);
      const scalar_t* py = reinterpret_cast<const scalar_t*>(&qy);
      const scalar_t* pd = reinterpret_cast<const scalar_t*>(&qd);
      uint4 qo;
      scalar_t* po = reinterpret_cast<scalar_t*>(&qo);
#pragma unroll
      for (int v = 0; v < VPT; ++v)
        po[v] = (emb2float(py[v]) > 0.f) ? pd[v] : float2emb(0.f, scalar_t{});
      *reinterpret_cast<uint4*>(g + base) = qo;
    } else {
      for (int64_t i = base; i < n; ++i)
        g[i] = (emb2float(y[i]) > 0.f) ? dy[i] : float2emb(0.f, scalar_t{});
    }
  }
}

at::Tensor relu_bwd_mask(const at::Tensor& grad_out, const at::Tensor& y) {
  TORCH_CHECK(grad_out.is_cuda() && grad_out.sizes() == y.sizes());
  auto dy = grad_out.contiguous();
  auto yc = y.contiguous();
  auto g = at::empty_like(dy);
  int64_t n = dy.numel();
  if (n == 0) return g;
  auto stream = mlp_stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(at::kHalf, at::kBFloat16, dy.scalar_type(),
                                  "relu_bwd_mask", [&] {
    if constexpr (std::is_same_v<scalar_t, double>) {
      TORCH_CHECK(false, "fp64 unsupported");
    } else {
      using dev_t = typename DevType<scalar_t>::type;
      constexpr int VPT = sizeof(dev_t) == 2 ? 8 : 4;
      int grid = grid_for((n + VPT - 1) / VPT, kBlockThreads);
      hipLaunchKernelGGL((relu_bwd_mask_kernel<dev_t, VPT>), dim3(grid),
                         dim3(kBlockThreads), 0, stream,
                         reinterpret_cast<const dev_t*>(dy.data_ptr<scalar_t>()),
                         reinterpret_cast<const dev_t*>(yc.data_ptr<scalar_t>()), n,
                         reinterpret_cast<dev_t*>(g.data_ptr<scalar_t>()));
    }
  });
  return g;
}

// ---------------------------------------------------------------------------
// fused BCE-with-logits (mean reduction). torch's BCEWithLogitsLoss expands
// to ~12 launch-floor kernels per step inside the captured graph
// (log_sigmoid fwd chain + sigmoid/sub/scale bwd); these two kernels do one
// pass each. fwd: deterministic two-level mean of
//   max(x,0) - x*y + log1p(exp(-|x|)); bwd: dx = go * (sigmoid(x) - y) / B.
// ---------------------------------------------------------------------------

__device__ __forceinline__ float bce_ldf(float v) { return v; }
__device__ __forceinline__ float bce_ldf(__half v) { return __half2float(v); }
__device__ __forceinline__ float bce_ldf(__hip_bfloat16 v) { return __bfloat162float(v); }

template <typename x_t>
__global__ void __launch_bounds__(kBlockThreads) bce_logits_partial_kernel(
    const x_t* __restrict__ logits, const float* __restrict__ labels, int64_t B,
    float* __restrict__ partial /* [G] */) {
  __shared__ float red[kBlockThreads / kWaveSize];
  float acc = 0.f;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       i < B; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    float x = bce_ldf(logits[i]);
    float y = labels[i];
    acc += fmaxf(x, 0.f) - x * y + log1pf(__expf(-fabsf(x)));
  }
  // wave then block reduce
  for (int off = kWaveSize / 2; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, kWaveSize);
  int wave = threadIdx.x / kWaveSize;
  if (threadIdx.x % kWaveSize == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < kBlockThreads / kWaveSize; ++w) s += red[w];
    partial[blockIdx.x] = s;
  }
}

__global__ void bce_logits_final_kernel(const float* __restrict__ partial, int G,
                                        float inv_B, float* __restrict__ out) {
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += partial[g];
    *out = s * inv_B;
  }
}

template <typename x_t>
__global__ void __launch_bounds__(kBlockThreads) bce_logits_bwd_kernel(
    const x_t* __restrict__ logits, const float* __restrict__ labels,
    const float* __restrict__ grad_out, float inv_B, int64_t B,
    x_t* __restrict__ dx) {
  float g = *grad_out * inv_B;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
       i < B; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    float x = bce_ldf(logits[i]);
    float sig = 1.f / (1.f + __expf(-x));
    dx[i] = float2emb(g * (sig - labels[i]), x_t{});
  }
}

at::Tensor bce_with_logits_fwd(const at::Tensor& logits, const at::Tensor& labels) {
  TORCH_CHECK(logits.is_cuda() && labels.scalar_type() == at::kFloat);
  int64_t B = logits.numel();
  auto out = at::empty({}, logits.options().dtype(at::kFloat));
  auto stream = mlp_stream();
  int G = std::min<int64_t>(512, (B + kBlockThreads - 1) / kBlockThreads);
  G = std::max(G, 1);
  auto partial = at::empty({G}, logits.options().dtype(at::kFloat));
  AT_DISPATCH_FLOATING_TYPES_AND2(at::kHalf, at::kBFloat16, logits.scalar_type(),
                                  "bce_fwd", [&] {
    if constexpr (std::is_same_v<scalar_t, double>) {
      TORCH_CHECK(false, "fp64 unsupported");
    } else {
      using dev_t = typename DevType<scalar_t>::type;
      hipLaunchKernelGGL((bce_logits_partial_kernel<dev_t>), dim3(G),
                         dim3(kBlockThreads), 0, stream,
                         reinterpret_cast<const dev_t*>(logits.data_ptr<scalar_t>()),
                         labels.data_ptr<float>(), B, partial.data_ptr<float>());
    }
  });
  hipLaunchKernelGGL(bce_logits_final_kernel, dim3(1), dim3(kWaveSize), 0, stream,
                     partial.data_ptr<float>(), G, B > 0 ? 1.f / B : 0.f,
                     out.data_ptr<float>());
  return out;
}

at::Tensor bce_with_logits_bwd(const at::Tensor& logits, const at::Tensor& labels,
                               const at::Tensor& grad_out) {
  int64_t B = logits.numel();
  auto dx = at::empty_like(logits);
  if (B == 0) return dx;
  auto stream = mlp_stream();
  int grid = grid_for(B, kBlockThreads);
  AT_DISPATCH_FLOATING_TYPES_AND2(at::kHalf, at::kBFloat16, logits.scalar_type(),
                                  "bce_bwd", [&] {
    if constexpr (std::is_same_v<scalar_t, double>) {
      TORCH_CHECK(false, "fp64 unsupported");
    } else {
      using dev_t = typename DevType<scalar_t>::type;
      hipLaunchKernelGGL((bce_logits_bwd_kernel<dev_t>), dim3(grid),
                         dim3(kBlockThreads), 0, stream,
                         reinterpret_cast<const dev_t*>(logits.data_ptr<scalar_t>()),
                         labels.data_ptr<float>(),
                         grad_out.data_ptr<float>(), 1.f / B, B,
                         reinterpret_cast<dev_t*>(dx.data_ptr<scalar_t>()));
    }
  });
  return dx;
}

}  // namespace trec_amd
