// Exhaustive top-k by inner product over a bf16 corpus for MI355X (gfx950):
// fused score-and-select on v_mfma_f32_16x16x32_bf16. The [B, N] score matrix
// is never written to memory.
//
//   scores[b, n] = q[b] . c[n] (+ row_bias[n]),  bf16 operands, fp32 accumulate
//   result[b]    = the k best (score desc, id asc), in that order
//
// A (score, id) pair travels as one 64-bit KEY: the order-preserving image of
// the fp32 score in the high word, ~id in the low word. "Better" under the
// contract's order is then plain unsigned key > key, ties included, and the
// empty slot is key 0 (decoded as -inf / -1).
//
// Partial kernel, grid (query tiles of 32) x (corpus splits S), 4 waves:
//   * the query tile is the B operand and lives in REGISTERS for the life of
//     the workgroup (2 groups of 16 queries x Dp/32 fragments, rounded to bf16
//     RNE and zero-filled past D / B while loading); no LDS in the GEMM.
//   * the corpus slice streams as the A operand straight from global memory:
//     wave w of step t owns rows [t*64 + w*16, +16), a lane's fragment is one
//     16-B load of 8 consecutive k of one row. The step loop is unrolled by
//     three over three named register buffers (fragments and the rows' bias),
//     so the loads of steps t+1 and t+2 are outstanding under step t's MFMAs
//     and no loaded register is copied. (As compiled, the waits in two of the
//     three sub-steps are non-zero vmcnt; one vmcnt(0) per triple remains at
//     the loop head, so one to two steps are in flight. See docs/KERNELS.md.)
//   * in the 16x16 result lane l holds rows (l>>4)*4 + 0..3 of query l&15, so
//     it tests its 4 scores against that query's threshold (the k-th best key
//     so far, in LDS) with no cross-lane traffic; the common case is one fp32
//     compare per score. Survivors are pushed to the query's LDS buffer of
//     cap = 128 (k <= 64) or 256 keys through an LDS counter.
//   * a step can push at most 64 keys per query. A query whose count passes
//     cap - 64 is flagged in a bit mask; after the step's barrier every wave
//     reads the same mask and the flagged queries are reduced, one wave each,
//     to their best k by rank-select (rank = number of better keys; keys are
//     unique, so rank is also the sorted position), which raises the
//     threshold. The masks rotate through three words so that the step's one
//     barrier is enough when nothing is flagged: word t%3 is written before
//     barrier t, read after it, and cleared by thread 0 after barrier t+1.
//   * at the end of the slice every query is reduced once more and its sorted
//     keys go to the [B, S, k] workspace, or, when S == 1, decoded straight to
//     the outputs.
// Merge kernel, one workgroup per query: the S sorted partials are read
// position-major (all heads first, so the threshold is tight after the first
// step) and run through the same threshold / buffer / rank-select machinery
// with all 256 threads on the one query (cap 512).
//
// Scores must not be NaN: a NaN never passes a threshold test and is dropped
// (the CPU reference's torch.sort would rank it first); +-inf are ordered.
//
// S depends on the shapes only, so a search has no host synchronisation and
// can be captured in a graph.
//
// The key, the select machinery and the merge kernel live in topk_select.h,
// which ivf_topk.hip shares.

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

template <int DK>
__global__ void __launch_bounds__(kThreads) mips_topk_partial_kernel(
    const void* __restrict__ queries, int q_is_bf16, int q_vec,
    const __bf16* __restrict__ corpus,
    const float* __restrict__ bias /* or nullptr */, int64_t B, int64_t N, int D, int k, int S,
    int64_t rows_per_split, int cap, u64* __restrict__ ws, float* __restrict__ out_s,
    int64_t* __restrict__ out_i) {
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
  const int64_t q0 = static_cast<int64_t>(blockIdx.x) * kQT;
  const int split = blockIdx.y;
  const int ng = (B - q0 > 16) ? 2 : 1;  // query groups with a live query

  // the query tile: B operand, lane holds 8 consecutive k of query l&15.
  // Rows whose width allows it (q_vec: D % 8 == 0) are read as 16-B vectors.
  mbf16x8 bq[kQG][DK];
#pragma unroll
  for (int g = 0; g < kQG; ++g) {
    const int64_t q = q0 + g * 16 + (l & 15);
#pragma unroll
    for (int ks = 0; ks < DK; ++ks) {
      const int kk0 = ks * 32 + (l >> 4) * 8;
      mbf16x8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = static_cast<__bf16>(0.f);
      if (q < B && kk0 < D) {
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

  const int64_t n_begin = split * rows_per_split;
  const int64_t n_end = n_begin + rows_per_split < N ? n_begin + rows_per_split : N;
  const int steps =
      n_end > n_begin ? static_cast<int>((n_end - n_begin + kStepRows - 1) / kStepRows) : 0;

  // One step's operands for this lane: the A fragments and the bias of its
  // four result rows. Loads are unconditional (no wait is forced by a branch):
  // a row past the slice reads the slice's last row instead, and its scores
  // are dropped by the row test of the select. Only called when steps > 0.
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
      if (g < ng && q0 + q < B) {
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

  // Three named buffers, the loop unrolled by three: step t computes from
  // buffer t % 3 while the loads of t + 1 and t + 2 are in flight, and no
  // loaded register is ever copied (a copy would wait for its load).
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

  for (int q = w; q < kQT; q += kThreads / kWaveSize) {
    if (q0 + q >= B) break;
    wave_rank_select(sel, q, k);
    const int n = sel.cnt[q];
    for (int j = l; j < k; j += kWaveSize) {
      const u64 key = j < n ? sel.buf[q * cap + j] : 0;
      if (S == 1) key_store(key, out_s + (q0 + q) * k + j, out_i + (q0 + q) * k + j);
      else ws[((q0 + q) * S + split) * k + j] = key;
    }
  }
}

template <int DK>
void launch_partial(dim3 grid, int lds_bytes, const void* q, int q_is_bf16, int q_vec,
                    const __bf16* c, const float* bias, int64_t B, int64_t N, int D, int k, int S,
                    int64_t per, int cap, u64* ws, float* out_s, int64_t* out_i) {
  // cap = 256 asks for a little more than the 64 KB default of dynamic LDS;
  // raise the limit once per device (the caller has made the tensors' device
  // current), not per launch, so a graph capture records only the launch
  static std::mutex mu;
  static uint64_t raised = 0;  // bit per device ordinal
  int dev = 0;
  TREC_HIP_CHECK(hipGetDevice(&dev));
  {
    std::lock_guard<std::mutex> lock(mu);
    if (dev >= 64 || !((raised >> dev) & 1)) {
      TREC_HIP_CHECK(hipFuncSetAttribute(
          reinterpret_cast<const void*>(mips_topk_partial_kernel<DK>),
          hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytesPerCU));
      if (dev < 64) raised |= uint64_t{1} << dev;
    }
  }
  hipLaunchKernelGGL(mips_topk_partial_kernel<DK>, grid, dim3(kThreads), lds_bytes,
                     mips_stream(), q, q_is_bf16, q_vec, c, bias, B, N, D, k, S, per, cap, ws,
                     out_s, out_i);
}

}  // namespace

std::tuple<at::Tensor, at::Tensor> mips_topk(const at::Tensor& queries, const at::Tensor& corpus,
                                             const c10::optional<at::Tensor>& row_bias, int64_t k,
                                             int64_t splits) {
  TORCH_CHECK(queries.is_cuda() && corpus.is_cuda() && queries.dim() == 2 && corpus.dim() == 2,
              "mips_topk: queries [B, D] and corpus [N, Dp] must be 2-D GPU tensors");
  TORCH_CHECK(corpus.device() == queries.device(), "mips_topk: tensors on different devices");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(queries.device());
  const int64_t B = queries.size(0), D = queries.size(1);
  const int64_t N = corpus.size(0), Dp = corpus.size(1);
  TORCH_CHECK(D >= 1 && D <= kMaxD, "mips_topk: need 1 <= D <= 256, got ", D);
  TORCH_CHECK(k >= 1 && k <= kMaxK, "mips_topk: need 1 <= k <= 128, got ", k);
  TORCH_CHECK(Dp % 32 == 0 && Dp == (D + 31) / 32 * 32,
              "mips_topk: corpus width must be D rounded up to a multiple of 32, got ", Dp);
  TORCH_CHECK(corpus.scalar_type() == at::kBFloat16 && corpus.is_contiguous() &&
                  reinterpret_cast<uintptr_t>(corpus.data_ptr()) % 16 == 0,
              "mips_topk: corpus must be contiguous, 16-byte aligned bf16");
  TORCH_CHECK(queries.scalar_type() == at::kFloat || queries.scalar_type() == at::kBFloat16,
              "mips_topk: queries must be fp32 or bf16");
  TORCH_CHECK(N < std::numeric_limits<int32_t>::max() && splits >= 0 && splits <= 65535,
              "mips_topk: need N < 2^31 - 1 and 0 <= splits <= 65535");
  const float* bias = nullptr;
  at::Tensor bias_c;
  if (row_bias.has_value() && row_bias->defined()) {
    TORCH_CHECK(row_bias->device() == queries.device() && row_bias->numel() == N &&
                    row_bias->scalar_type() == at::kFloat,
                "mips_topk: row_bias must be an fp32 [N] GPU tensor");
    bias_c = row_bias->contiguous();
    bias = bias_c.data_ptr<float>();
  }
  auto out_s = at::empty({B, k}, queries.options().dtype(at::kFloat));
  auto out_i = at::empty({B, k}, queries.options().dtype(at::kLong));
  if (B == 0) return {out_s, out_i};
  auto qc = queries.contiguous();

  // split count from the shapes alone
  const int64_t tiles = (B + kQT - 1) / kQT;
  int64_t S = splits;
  if (S == 0) {
    S = std::min<int64_t>((kTargetBlocks + tiles - 1) / tiles,
                          (N + kMinSplitRows - 1) / kMinSplitRows);
    S = std::max<int64_t>(1, std::min<int64_t>(S, 65535));
  }
  int64_t per = (N + S - 1) / S;
  per = std::max<int64_t>(kStepRows, (per + kStepRows - 1) / kStepRows * kStepRows);

  at::Tensor ws;
  u64* ws_p = nullptr;
  if (S > 1) {
    TORCH_CHECK(S * k < (int64_t{1} << 30), "mips_topk: splits * k too large");
    ws = at::empty({B, S, k}, queries.options().dtype(at::kLong));
    ws_p = reinterpret_cast<u64*>(ws.data_ptr<int64_t>());
  }
  const int cap = k <= 64 ? 128 : 256;
  static_assert(kMaxK <= 256 - kStepRows && kMaxK <= kMergeCap - kThreads);
  const int lds_bytes = kQT * cap * 8 + kQT * (8 + 4 + 4) + 16;
  const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(S));
  const int q_is_bf16 = qc.scalar_type() == at::kBFloat16;
  const int q_vec = D % 8 == 0 && reinterpret_cast<uintptr_t>(qc.data_ptr()) % 16 == 0;
  const __bf16* cp = reinterpret_cast<const __bf16*>(corpus.data_ptr<at::BFloat16>());
#define TREC_MIPS_CASE(DK)                                                                    \
  case DK:                                                                                    \
    launch_partial<DK>(grid, lds_bytes, qc.data_ptr(), q_is_bf16, q_vec, cp, bias, B, N,      \
                       static_cast<int>(D), static_cast<int>(k), static_cast<int>(S), per,    \
                       cap, ws_p, out_s.data_ptr<float>(), out_i.data_ptr<int64_t>());        \
    break;
  switch (Dp / 32) {
    TREC_MIPS_CASE(1)
    TREC_MIPS_CASE(2)
    TREC_MIPS_CASE(3)
    TREC_MIPS_CASE(4)
    TREC_MIPS_CASE(5)
    TREC_MIPS_CASE(6)
    TREC_MIPS_CASE(7)
    TREC_MIPS_CASE(8)
    default:
      TORCH_CHECK(false, "mips_topk: unsupported width");
  }
#undef TREC_MIPS_CASE
  TREC_HIP_CHECK(hipGetLastError());
  if (S > 1) {
    hipLaunchKernelGGL(mips_topk_merge_kernel, dim3(static_cast<unsigned>(B)), dim3(kThreads), 0,
                       mips_stream(), ws_p, static_cast<int>(S), static_cast<int>(k),
                       out_s.data_ptr<float>(), out_i.data_ptr<int64_t>());
    TREC_HIP_CHECK(hipGetLastError());
  }
  return {out_s, out_i};
}

}  // namespace trec_amd
