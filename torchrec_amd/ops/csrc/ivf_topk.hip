// IVF-Flat fine stage for MI355X (gfx950): top-k by inner product restricted
// to the corpus lists each query probes, on the select path of mips_topk.hip.
//
//   corpus rows are stored list by list, list l = rows
//   [list_offsets[l], list_offsets[l+1]); probes[b, p] names the lists query b
//   searches (-1: none). result[b] = the k best (score desc, row asc) among
//   the union of b's probed lists.
//
// The work is LIST-MAJOR: a list is read from HBM once per 32 queries that
// probe it, not once per query. Three parts, no host synchronisation:
//
// Plan (index-only, four small kernels):
//   * clear the per-list counters; count the (query, probe-rank) PAIRS per
//     list with atomics (a pair whose probe is -1 instead clears its
//     workspace slot, which nobody else writes);
//   * one workgroup scans ceil(count / 32) over the lists into each list's
//     first TILE, labels the tiles with their list, marks the unused slots of
//     a list's last tile and the tiles past the total -1, and clears the
//     counters again;
//   * scatter: a pair takes slot j = atomicAdd(counter[list]) of its list,
//     i.e. slot j % 32 of tile first[list] + j / 32. Which pair lands in which
//     slot varies from run to run; a query's result does not depend on it.
//   The tile count depends on the data, so the scan kernel is launched over
//   the shape-only bound T_max = P / 32 + min(nlist, P), P = B * nprobe
//   (sum of ceil(c_l / 32) <= sum of floor(c_l / 32) + non-empty lists).
//
// Scan kernel, grid (T_max, splits S), 4 waves, instantiated per Dp / 32: a
// workgroup owns one tile. Its up to 32 queries are GATHERED through the tile
// table into the B operand of v_mfma_f32_16x16x32_bf16 and stay in registers
// (fragment layout, bf16 rounding and zero fill of mips_topk_partial_kernel);
// the list's rows (row range `split` of S of them) stream as the A operand
// with the flat kernel's three-buffer step loop and clamped unconditional
// loads; scores go through the shared threshold / buffer / rank-select code
// (topk_select.h). Unused query slots never push. Every live query's sorted
// best k go to ws[b, p, split, :k], zero keys past the rows it has, so every
// valid pair's slot is fully written and ws needs no initialisation.
//
// Merge: mips_topk_merge_kernel over the nprobe * S sorted partials of a query.

#include <torch/extension.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <algorithm>
#include <limits>
#include <mutex>
#include <tuple>

#include "common.h"
#include "topk_select.h"

namespace trec_amd {

namespace {

constexpr int kPlanThreads = 1024;  // the one workgroup of the tile scan
constexpr int kMaxProbe = 128;
constexpr int kMaxLists = 65536;

__global__ void __launch_bounds__(kThreads) ivf_plan_clear_kernel(int* __restrict__ cnt,
                                                                  int nlist) {
  for (int l = blockIdx.x * kThreads + threadIdx.x; l < nlist; l += gridDim.x * kThreads)
    cnt[l] = 0;
}

// A probe outside [0, nlist) is "no list", -1 included.
__global__ void __launch_bounds__(kThreads) ivf_plan_count_kernel(
    const int64_t* __restrict__ probes, int64_t P, int nlist, int* __restrict__ cnt,
    u64* __restrict__ ws, int64_t slot_keys) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t pair = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; pair < P;
       pair += stride) {
    const int64_t list = probes[pair];
    if (list >= 0 && list < nlist) {
      atomicAdd(&cnt[list], 1);
    } else {
      for (int64_t j = 0; j < slot_keys; ++j) ws[pair * slot_keys + j] = 0;
    }
  }
}

// One workgroup. Thread t owns the lists [t * per, (t + 1) * per).
__global__ void __launch_bounds__(kPlanThreads) ivf_plan_tiles_kernel(
    int* __restrict__ cnt, int* __restrict__ first_tile, int* __restrict__ tile_list,
    int* __restrict__ tile_pairs, int nlist, int64_t t_max) {
  __shared__ int part[kPlanThreads];
  const int tid = threadIdx.x;
  const int per = (nlist + kPlanThreads - 1) / kPlanThreads;
  const int l0 = tid * per < nlist ? tid * per : nlist;
  const int l1 = l0 + per < nlist ? l0 + per : nlist;
  int sum = 0;
  for (int l = l0; l < l1; ++l) sum += (cnt[l] + kQT - 1) / kQT;
  part[tid] = sum;
  __syncthreads();
  for (int off = 1; off < kPlanThreads; off <<= 1) {
    const int v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  const int total = part[kPlanThreads - 1];  // <= t_max, see the file comment
  int64_t t = part[tid] - sum;
  for (int l = l0; l < l1; ++l) {
    const int c = cnt[l];
    first_tile[l] = static_cast<int>(t);
    cnt[l] = 0;  // the scatter counts up again
    for (int j = 0; j < c; j += kQT, ++t) {
      tile_list[t] = l;
      for (int s = c - j; s < kQT; ++s) tile_pairs[t * kQT + s] = -1;
    }
  }
  for (int64_t u = total + tid; u < t_max; u += kPlanThreads) tile_list[u] = -1;
}

__global__ void __launch_bounds__(kThreads) ivf_plan_scatter_kernel(
    const int64_t* __restrict__ probes, int64_t P, int nlist, int* __restrict__ cnt,
    const int* __restrict__ first_tile, int* __restrict__ tile_pairs) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t pair = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; pair < P;
       pair += stride) {
    const int64_t list = probes[pair];
    if (list >= 0 && list < nlist) {
      const int j = atomicAdd(&cnt[list], 1);
      tile_pairs[(static_cast<int64_t>(first_tile[list]) + j / kQT) * kQT + j % kQT] =
          static_cast<int>(pair);
    }
  }
}

template <int DK>
__global__ void __launch_bounds__(kThreads) ivf_scan_kernel(
    const void* __restrict__ queries, int q_is_bf16, int q_vec,
    const __bf16* __restrict__ corpus, const float* __restrict__ bias /* or nullptr */,
    const int64_t* __restrict__ list_offsets, const int* __restrict__ tile_list,
    const int* __restrict__ tile_pairs, int64_t N, int D, int nprobe, int k, int S, int cap,
    u64* __restrict__ ws) {
  const int list = tile_list[blockIdx.x];
  if (list < 0) return;  // a surplus workgroup; the same for every thread

  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int Dp = DK * 32;
  Sel sel;
  sel.buf = reinterpret_cast<u64*>(lds);
  sel.thr = sel.buf + kQT * cap;
  sel.thr_s = reinterpret_cast<float*>(sel.thr + kQT);
  sel.cnt = reinterpret_cast<int*>(sel.thr_s + kQT);
  sel.mask = reinterpret_cast<unsigned*>(sel.cnt + kQT);
  sel.cap = cap;
  sel.limit = cap - kStepRows;
  sel_init(sel, kQT);

  const int l = lane_id(), w = wave_id();
  const int split = blockIdx.y;
  // The tile's pairs: lane s (and s + 32) holds slot s. Live slots are a
  // prefix, the plan fills them in order.
  const int my_pair = tile_pairs[static_cast<int64_t>(blockIdx.x) * kQT + l % kQT];
  const int nq = __popcll(__ballot(my_pair >= 0 && l < kQT));
  const int ng = nq > 16 ? 2 : 1;  // query groups with a live query

  // the gathered query tile: B operand, lane holds 8 consecutive k of the
  // query in slot g * 16 + (l & 15)
  mbf16x8 bq[kQG][DK];
#pragma unroll
  for (int g = 0; g < kQG; ++g) {
    const int pair = __shfl(my_pair, g * 16 + (l & 15), kWaveSize);
    const int64_t q = pair / nprobe;
#pragma unroll
    for (int ks = 0; ks < DK; ++ks) {
      const int kk0 = ks * 32 + (l >> 4) * 8;
      mbf16x8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = static_cast<__bf16>(0.f);
      if (pair >= 0 && kk0 < D) {
        if (q_vec && q_is_bf16) {
          v = *reinterpret_cast<const mbf16x8*>(static_cast<const __bf16*>(queries) + q * D + kk0);
        } else if (q_vec) {
          const mf32x4* p =
              reinterpret_cast<const mf32x4*>(static_cast<const float*>(queries) + q * D + kk0);
          const mf32x4 lo = p[0], hi = p[1];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] = static_cast<__bf16>(lo[e]);
            v[4 + e] = static_cast<__bf16>(hi[e]);
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if (kk0 + e < D) {
              v[e] = q_is_bf16
                         ? static_cast<const __bf16*>(queries)[q * D + kk0 + e]
                         : static_cast<__bf16>(static_cast<const float*>(queries)[q * D + kk0 + e]);
            }
          }
        }
      }
      bq[g][ks] = v;
    }
  }

  // this workgroup's rows: range `split` of S of the list, in whole steps.
  // The offsets are clamped into [0, N] so that no table can send a load
  // outside the corpus.
  int64_t lb = list_offsets[list], le = list_offsets[list + 1];
  lb = lb < 0 ? 0 : (lb > N ? N : lb);
  le = le < lb ? lb : (le > N ? N : le);
  int64_t per = (le - lb + S - 1) / S;
  per = per < kStepRows ? kStepRows : (per + kStepRows - 1) / kStepRows * kStepRows;
  const int64_t n_begin = lb + split * per;
  const int64_t n_end = n_begin + per < le ? n_begin + per : le;
  const int steps =
      n_end > n_begin ? static_cast<int>((n_end - n_begin + kStepRows - 1) / kStepRows) : 0;

  // One step's operands for this lane, as in mips_topk_partial_kernel: loads
  // are unconditional, a row past the range reads the range's last row and
  // its scores are dropped by the row test. Only called when steps > 0.
  struct StepData {
    mbf16x8 a[DK];
    float bv[4];
  };
  auto load = [&](StepData& d, int t) {
    const int64_t r0 = n_begin + static_cast<int64_t>(t) * kStepRows + w * 16;
    int64_t row = r0 + (l & 15);
    row = row < n_end ? row : n_end - 1;
    const __bf16* p = corpus + row * Dp + (l >> 4) * 8;
#pragma unroll
    for (int ks = 0; ks < DK; ++ks) d.a[ks] = *reinterpret_cast<const mbf16x8*>(p + ks * 32);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int64_t br = r0 + (l >> 4) * 4 + i;
      br = br < n_end ? br : n_end - 1;
      d.bv[i] = bias != nullptr ? bias[br] : 0.f;
    }
  };

  auto step = [&](const StepData& d, int t) {
    mf32x4 acc[kQG];
#pragma unroll
    for (int g = 0; g < kQG; ++g) acc[g] = mf32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < DK; ++ks) {
#pragma unroll
      for (int g = 0; g < kQG; ++g) {
        if (g < ng)
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(d.a[ks], bq[g][ks], acc[g], 0, 0, 0);
      }
    }

    const int64_t r_base = n_begin + static_cast<int64_t>(t) * kStepRows + w * 16 + (l >> 4) * 4;
#pragma unroll
    for (int g = 0; g < kQG; ++g) {
      const int q = g * 16 + (l & 15);
      if (q < nq) {  // an unused slot never pushes
        const float ts = sel.thr_s[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float sc = acc[g][i] + d.bv[i];
          if (r_base + i < n_end && sc >= ts) {  // a NaN score never passes
            const u64 key = make_key(sc, static_cast<int>(r_base + i));
            if (key > sel.thr[q]) sel_push(sel, q, key, t);
          }
        }
      }
    }

    unsigned m;
    if (sel_step_end(sel, t, &m)) {
      for (int idx = 0; m != 0; ++idx, m &= m - 1) {
        if ((idx & 3) == w) wave_rank_select(sel, __ffs(m) - 1, k);
      }
      wg_sync();
    }
  };

  if (steps > 0) {
    StepData d0, d1, d2;
    load(d0, 0);
    load(d1, 1);
    for (int t = 0; t < steps; t += 3) {
      load(d2, t + 2);
      step(d0, t);
      if (t + 1 >= steps) break;
      load(d0, t + 3);
      step(d1, t + 1);
      if (t + 2 >= steps) break;
      load(d1, t + 4);
      step(d2, t + 2);
    }
  }

  for (int q = w; q < nq; q += kThreads / kWaveSize) {
    wave_rank_select(sel, q, k);
    const int n = sel.cnt[q];
    const int64_t pair = __shfl(my_pair, q, kWaveSize);
    u64* dst = ws + (pair * S + split) * k;
    for (int j = l; j < k; j += kWaveSize) dst[j] = j < n ? sel.buf[q * cap + j] : 0;
  }
}

template <int DK>
void launch_scan(dim3 grid, int lds_bytes, const void* q, int q_is_bf16, int q_vec,
                 const __bf16* c, const float* bias, const int64_t* list_offsets,
                 const int* tile_list, const int* tile_pairs, int64_t N, int D, int nprobe, int k,
                 int S, int cap, u64* ws) {
  // cap = 256 needs a little more than the 64 KB default of dynamic LDS;
  // raised once per device, so a graph capture records only the launch
  static std::mutex mu;
  static uint64_t raised = 0;  // bit per device ordinal
  int dev = 0;
  TREC_HIP_CHECK(hipGetDevice(&dev));
  {
    std::lock_guard<std::mutex> lock(mu);
    if (dev >= 64 || !((raised >> dev) & 1)) {
      TREC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ivf_scan_kernel<DK>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         kLdsBytesPerCU));
      if (dev < 64) raised |= uint64_t{1} << dev;
    }
  }
  hipLaunchKernelGGL(ivf_scan_kernel<DK>, grid, dim3(kThreads), lds_bytes, mips_stream(), q,
                     q_is_bf16, q_vec, c, bias, list_offsets, tile_list, tile_pairs, N, D, nprobe,
                     k, S, cap, ws);
}

}  // namespace

std::tuple<at::Tensor, at::Tensor> ivf_topk(const at::Tensor& queries, const at::Tensor& corpus,
                                            const at::Tensor& list_offsets,
                                            const at::Tensor& probes,
                                            const c10::optional<at::Tensor>& row_bias, int64_t k,
                                            int64_t splits) {
  TORCH_CHECK(queries.is_cuda() && corpus.is_cuda() && queries.dim() == 2 && corpus.dim() == 2,
              "ivf_topk: queries [B, D] and corpus [N, Dp] must be 2-D GPU tensors");
  TORCH_CHECK(corpus.device() == queries.device() && list_offsets.device() == queries.device() &&
                  probes.device() == queries.device(),
              "ivf_topk: tensors on different devices");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(queries.device());
  const int64_t B = queries.size(0), D = queries.size(1);
  const int64_t N = corpus.size(0), Dp = corpus.size(1);
  TORCH_CHECK(D >= 1 && D <= kMaxD, "ivf_topk: need 1 <= D <= 256, got ", D);
  TORCH_CHECK(k >= 1 && k <= kMaxK, "ivf_topk: need 1 <= k <= 128, got ", k);
  TORCH_CHECK(Dp % 32 == 0 && Dp == (D + 31) / 32 * 32,
              "ivf_topk: corpus width must be D rounded up to a multiple of 32, got ", Dp);
  TORCH_CHECK(corpus.scalar_type() == at::kBFloat16 && corpus.is_contiguous() &&
                  reinterpret_cast<uintptr_t>(corpus.data_ptr()) % 16 == 0,
              "ivf_topk: corpus must be contiguous, 16-byte aligned bf16");
  TORCH_CHECK(queries.scalar_type() == at::kFloat || queries.scalar_type() == at::kBFloat16,
              "ivf_topk: queries must be fp32 or bf16");
  TORCH_CHECK(N < std::numeric_limits<int32_t>::max() && splits >= 0 && splits <= 65535,
              "ivf_topk: need N < 2^31 - 1 and 0 <= splits <= 65535");
  TORCH_CHECK(list_offsets.scalar_type() == at::kLong && list_offsets.dim() == 1 &&
                  list_offsets.numel() >= 2 && list_offsets.numel() - 1 <= kMaxLists,
              "ivf_topk: list_offsets must be int64 [nlist + 1] with 1 <= nlist <= 65536");
  TORCH_CHECK(probes.scalar_type() == at::kLong && probes.dim() == 2 && probes.size(0) == B &&
                  probes.size(1) >= 1 && probes.size(1) <= kMaxProbe,
              "ivf_topk: probes must be int64 [B, nprobe] with 1 <= nprobe <= 128");
  const int64_t nlist = list_offsets.numel() - 1, nprobe = probes.size(1);
  const int64_t P = B * nprobe;
  TORCH_CHECK(P < (int64_t{1} << 31), "ivf_topk: need B * nprobe < 2^31");
  const float* bias = nullptr;
  at::Tensor bias_c;
  if (row_bias.has_value() && row_bias->defined()) {
    TORCH_CHECK(row_bias->device() == queries.device() && row_bias->numel() == N &&
                    row_bias->scalar_type() == at::kFloat,
                "ivf_topk: row_bias must be an fp32 [N] GPU tensor");
    bias_c = row_bias->contiguous();
    bias = bias_c.data_ptr<float>();
  }
  auto out_s = at::empty({B, k}, queries.options().dtype(at::kFloat));
  auto out_i = at::empty({B, k}, queries.options().dtype(at::kLong));
  if (B == 0) return {out_s, out_i};
  auto qc = queries.contiguous();
  auto offs = list_offsets.contiguous();
  auto pr = probes.contiguous();

  // tile bound and split count from the shapes alone
  const int64_t t_max = P / kQT + std::min(nlist, P);
  int64_t S = splits;
  if (S == 0) {
    S = std::min<int64_t>((kTargetBlocks + t_max - 1) / t_max,
                          (N / nlist + kMinSplitRows - 1) / kMinSplitRows);
    S = std::max<int64_t>(1, std::min<int64_t>(S, 65535));
  }
  TORCH_CHECK(nprobe * S * k < (int64_t{1} << 30), "ivf_topk: nprobe * splits * k too large");
  const int64_t ws_bytes = P * S * k * 8;
  TORCH_CHECK(ws_bytes <= (int64_t{1} << 34), "ivf_topk: the workspace B * nprobe * splits * k",
              " * 8 = ", ws_bytes, " bytes exceeds 16 GiB; search in smaller batches");
  auto ws = at::empty({B, nprobe, S, k}, queries.options().dtype(at::kLong));
  u64* ws_p = reinterpret_cast<u64*>(ws.data_ptr<int64_t>());
  // plan: per-list counters, first tiles, the tiles' lists, the tiles' pairs
  auto plan = at::empty({2 * nlist + t_max * (1 + kQT)}, queries.options().dtype(at::kInt));
  int* cnt = plan.data_ptr<int>();
  int* first_tile = cnt + nlist;
  int* tile_list = first_tile + nlist;
  int* tile_pairs = tile_list + t_max;

  const hipStream_t stream = mips_stream();
  const int64_t* pr_p = pr.data_ptr<int64_t>();
  const int nl = static_cast<int>(nlist);
  hipLaunchKernelGGL(ivf_plan_clear_kernel, dim3(grid_for(nlist, kThreads)), dim3(kThreads), 0,
                     stream, cnt, nl);
  hipLaunchKernelGGL(ivf_plan_count_kernel, dim3(grid_for(P, kThreads)), dim3(kThreads), 0, stream,
                     pr_p, P, nl, cnt, ws_p, S * k);
  hipLaunchKernelGGL(ivf_plan_tiles_kernel, dim3(1), dim3(kPlanThreads), 0, stream, cnt,
                     first_tile, tile_list, tile_pairs, nl, t_max);
  hipLaunchKernelGGL(ivf_plan_scatter_kernel, dim3(grid_for(P, kThreads)), dim3(kThreads), 0,
                     stream, pr_p, P, nl, cnt, first_tile, tile_pairs);
  TREC_HIP_CHECK(hipGetLastError());

  const int cap = k <= 64 ? 128 : 256;
  const int lds_bytes = kQT * cap * 8 + kQT * (8 + 4 + 4) + 16;
  const dim3 grid(static_cast<unsigned>(t_max), static_cast<unsigned>(S));
  const int q_is_bf16 = qc.scalar_type() == at::kBFloat16;
  const int q_vec = D % 8 == 0 && reinterpret_cast<uintptr_t>(qc.data_ptr()) % 16 == 0;
  const __bf16* cp = reinterpret_cast<const __bf16*>(corpus.data_ptr<at::BFloat16>());
#define TREC_IVF_CASE(DK)                                                                      \
  case DK:                                                                                     \
    launch_scan<DK>(grid, lds_bytes, qc.data_ptr(), q_is_bf16, q_vec, cp, bias,                \
                    offs.data_ptr<int64_t>(), tile_list, tile_pairs, N, static_cast<int>(D),   \
                    static_cast<int>(nprobe), static_cast<int>(k), static_cast<int>(S), cap,   \
                    ws_p);                                                                     \
    break;
  switch (Dp / 32) {
    TREC_IVF_CASE(1)
    TREC_IVF_CASE(2)
    TREC_IVF_CASE(3)
    TREC_IVF_CASE(4)
    TREC_IVF_CASE(5)
    TREC_IVF_CASE(6)
    TREC_IVF_CASE(7)
    TREC_IVF_CASE(8)
    default:
      TORCH_CHECK(false, "ivf_topk: unsupported width");
  }
#undef TREC_IVF_CASE
  TREC_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(mips_topk_merge_kernel, dim3(static_cast<unsigned>(B)), dim3(kThreads), 0,
                     stream, ws_p, static_cast<int>(nprobe * S), static_cast<int>(k),
                     out_s.data_ptr<float>(), out_i.data_ptr<int64_t>());
  TREC_HIP_CHECK(hipGetLastError());
  return {out_s, out_i};
}

}  // namespace trec_amd
