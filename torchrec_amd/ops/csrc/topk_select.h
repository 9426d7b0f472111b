// The select machinery shared by the top-k kernels (mips_topk.hip,
// ivf_topk.hip): the 64-bit (score, ~id) key, the per-query LDS candidate
// state with its threshold, the rank-select reduction and the kernel that
// merges sorted partials. See mips_topk.hip for how the pieces are used.
#pragma once

#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <limits>

#include "common.h"

namespace trec_amd {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 mbf16x8;
typedef __attribute__((ext_vector_type(4))) float mf32x4;
using u64 = unsigned long long;

constexpr int kQT = 32;         // queries per workgroup (two 16-query MFMA groups)
constexpr int kQG = kQT / 16;
constexpr int kStepRows = 64;   // corpus rows per step: 4 waves x 16
constexpr int kThreads = 256;
constexpr int kMaxK = 128;
constexpr int kMaxD = 256;
constexpr int kMergeCap = 512;  // k + one step of 256 pushes fits
constexpr int kMergeLoads = 16; // keys per thread per merge chunk
constexpr int kTargetBlocks = 2 * kNumCU;
constexpr int kMinSplitRows = 2048;

__device__ __forceinline__ void wg_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// orders one wave's LDS traffic (its lanes exchange data through LDS)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ u64 make_key(float s, int id) {
  s += 0.0f;  // -0 -> +0: equal scores must give equal high words
  unsigned u = __float_as_uint(s);
  u ^= static_cast<unsigned>(static_cast<int>(u) >> 31) | 0x80000000u;
  return (static_cast<u64>(u) << 32) | (0xFFFFFFFFu - static_cast<unsigned>(id));
}
__device__ __forceinline__ float key_score(u64 key) {
  const unsigned v = static_cast<unsigned>(key >> 32);
  return __uint_as_float((v & 0x80000000u) ? (v ^ 0x80000000u) : ~v);
}
__device__ __forceinline__ void key_store(u64 key, float* s, int64_t* id) {
  *s = key ? key_score(key) : -std::numeric_limits<float>::infinity();
  *id = key ? static_cast<int64_t>(0xFFFFFFFFu - static_cast<unsigned>(key)) : -1;
}

// Per-query candidate state in LDS.
struct Sel {
  u64* buf;        // [queries, cap]
  u64* thr;        // k-th best key so far (0: everything passes)
  float* thr_s;    // its score, for the one-compare fast path
  int* cnt;
  unsigned* mask;  // [3] queries to reduce, rotating by step
  int cap;
  int limit;       // cap - (most pushes per query per step)
};

__device__ __forceinline__ void sel_init(const Sel& s, int nq) {
  const int t = threadIdx.x;
  if (t < nq) {
    s.thr[t] = 0;
    s.thr_s[t] = -std::numeric_limits<float>::infinity();
    s.cnt[t] = 0;
  }
  if (t < 3) s.mask[t] = 0;
  wg_sync();
}

// cnt <= limit at the start of every step, so pos < cap here.
__device__ __forceinline__ void sel_push(const Sel& s, int q, u64 key, int step) {
  const int pos = atomicAdd(&s.cnt[q], 1);
  s.buf[q * s.cap + pos] = key;
  if (pos + 1 > s.limit) atomicOr(&s.mask[step % 3], 1u << q);
}

// After a step's pushes: one barrier; true (for every thread alike) when
// some query has to be reduced. *m is the mask.
__device__ __forceinline__ bool sel_step_end(const Sel& s, int step, unsigned* m) {
  wg_sync();
  if (threadIdx.x == 0) s.mask[(step + 2) % 3] = 0;
  *m = __builtin_amdgcn_readfirstlane(s.mask[step % 3]);
  return *m != 0;
}

// Reduce query q to its best min(cnt, k) keys, sorted, and raise its
// threshold. PER * (threads taking part) == cap. WG: all 256 threads work on
// the one query (and synchronise as a workgroup), else one wave does.
template <int PER, bool WG>
__device__ __forceinline__ void rank_select(const Sel& s, int q, int k) {
  constexpr int NT = WG ? kThreads : kWaveSize;
  const int t = WG ? static_cast<int>(threadIdx.x) : lane_id();
  u64* buf = s.buf + q * s.cap;
  const int n = s.cnt[q];
  u64 mine[PER];
  int rank[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    mine[j] = (t + j * NT < n) ? buf[t + j * NT] : 0;
    rank[j] = 0;
  }
#pragma unroll 4
  for (int e = 0; e < n; ++e) {
    const u64 key = buf[e];  // same address in every lane: an LDS broadcast
#pragma unroll
    for (int j = 0; j < PER; ++j) rank[j] += (key > mine[j]) ? 1 : 0;
  }
  if (WG) wg_sync(); else wave_sync();  // every read before the first write
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (t + j * NT < n && rank[j] < k) {
      buf[rank[j]] = mine[j];
      if (rank[j] == k - 1) {
        s.thr[q] = mine[j];
        s.thr_s[q] = key_score(mine[j]);
      }
    }
  }
  if (t == 0) s.cnt[q] = n < k ? n : k;
  if (WG) wg_sync(); else wave_sync();
}

__device__ __forceinline__ void wave_rank_select(const Sel& s, int q, int k) {
  if (s.cap == 2 * kWaveSize) rank_select<2, false>(s, q, k);
  else rank_select<4, false>(s, q, k);
}

__global__ void __launch_bounds__(kThreads) mips_topk_merge_kernel(
    const u64* __restrict__ ws, int S, int k, float* __restrict__ out_s,
    int64_t* __restrict__ out_i) {
  __shared__ u64 buf[kMergeCap];
  __shared__ u64 thr[1];
  __shared__ float thr_s[1];
  __shared__ int cnt[1];
  __shared__ unsigned mask[3];
  Sel sel{buf, thr, thr_s, cnt, mask, kMergeCap, kMergeCap - kThreads};
  sel_init(sel, 1);

  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int total = S * k;
  const u64* src = ws + b * total;
  int step = 0;
  for (int base = 0; base < total; base += kThreads * kMergeLoads) {
    // position-major: element t is entry t / S of partial t % S
    u64 keys[kMergeLoads];
#pragma unroll
    for (int i = 0; i < kMergeLoads; ++i) {
      const int t = base + i * kThreads + tid;
      keys[i] = t < total ? src[(t % S) * k + t / S] : 0;
    }
#pragma unroll
    for (int i = 0; i < kMergeLoads; ++i) {
      if (base + i * kThreads < total) {  // the same for every thread
        if (keys[i] > thr[0]) sel_push(sel, 0, keys[i], step);
        unsigned m;
        if (sel_step_end(sel, step, &m)) rank_select<kMergeCap / kThreads, true>(sel, 0, k);
        ++step;
      }
    }
  }
  rank_select<kMergeCap / kThreads, true>(sel, 0, k);
  const int n = cnt[0];
  for (int j = tid; j < k; j += kThreads)
    key_store(j < n ? buf[j] : 0, out_s + b * k + j, out_i + b * k + j);
}

inline hipStream_t mips_stream() {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

}  // namespace

}  // namespace trec_amd
