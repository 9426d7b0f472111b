// OCP microscaling (MXFP8 / MXFP4) wire codec for the quantized all-to-all,
// MI355X (gfx950).
//
// Wire, per group of 32 consecutive fp32 values of the logical message:
//   MXFP8: 32 e4m3fn bytes (element i in byte i) + 1 E8M0 scale byte = 33 B
//   MXFP4: 16 bytes of e2m1 (element 2k low nibble, 2k+1 high nibble)
//          + 1 E8M0 scale byte                                        = 17 B
// Scale: E = (biased exponent of amax) - 127 - emax, +1 when the mantissa of
// amax lies above that of elem_max (448 = 1.75 * 2^8, 6 = 1.5 * 2^2), i.e.
// the smallest E at which amax * 2^-E <= elem_max; clamped to [-127, 127],
// stored as E + 127. A non-finite group stores 0xFF and zero codes and
// decodes to NaN; an all-zero group stores 0 and zero codes. Every scaling
// step is a multiply by a power of two, so encode and decode are exact
// against the plain-PyTorch reference (distributed/qcomm_codecs.py).
//
// Work split: a workgroup of 256 threads owns a tile of 256 groups (32 KB of
// fp32, 8448 B / 4352 B of wire). 256 is a multiple of 16, so with 33- and
// 17-byte groups every tile's wire range starts 16-byte aligned.
//
// Encode: eight lanes per group, eight passes per tile. All eight float4
// loads of a thread are issued before the first is used. The group amax is a
// max over the |x| bit patterns (NaN and Inf sort above every finite value)
// in three DPP steps inside the eight lanes. Each lane packs its four values
// (one dword of e4m3, or two bytes of e2m1), writes them and (lane 0) the
// scale byte to their wire positions in an LDS image of the tile; after one
// barrier the image leaves as 16-byte stores. Only the last tile can have a
// wire tail that is not a multiple of 16 bytes; those < 16 bytes go out as
// bytes, so nothing is written past encoded_numel.
//
// Decode is the mirror: 16-byte loads of the tile's wire range into LDS (the
// last tile's tail as bytes), one barrier, then each lane reads its codes and
// the group's scale byte from LDS, converts and stores one float4.
//
// Addressing is flat (the logical message is contiguous) or slab: the message
// is the concatenation over ranks r of a [B, d_r] block, and each block is a
// column slab of one row-major [B, sum_D] matrix (the pooled all-to-all's
// output / grad_output). d_r % 32 == 0, so a group never straddles a row.
// The table of column offsets (world size + 1 ints) is searched once per
// tile; a thread then only walks forward from that block.

#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include "common.h"
#include "mx_quant.h"

namespace trec_amd {

namespace {

constexpr int kMxTileGroups = 256;  // groups per workgroup (multiple of 16)
constexpr int kMxThreads = 256;
constexpr int kMxLanesPerGroup = 8;  // one float4 each
constexpr int kMxGroupsPerPass = kMxThreads / kMxLanesPerGroup;
constexpr int kMxPasses = kMxTileGroups / kMxGroupsPerPass;

// Slab addressing: col_off[r] is the first column of block r (col_off[n] is
// sum_D), so block r starts at logical group B * col_off[r] / 32.
struct MxSlab {
  const int* col_off;
  int n_blocks;
  int B;
  int64_t ld;
};

// Device code of this file is built without the packed fp32 VALU forms (see
// cross_mfma.hip): everything the kernels call is defined between the push
// and the pop or in mx_quant.h (built the same way; shared with
// mx_linear.hip), with builtins rather than header helpers.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

typedef __attribute__((ext_vector_type(4))) float mf32x4;
typedef __attribute__((ext_vector_type(4))) unsigned mu32x4;
// code words sit at odd byte offsets of the LDS image (33- / 17-byte groups)
typedef unsigned __attribute__((aligned(1))) mu32_u;
typedef unsigned short __attribute__((aligned(1))) mu16_u;

__device__ __forceinline__ int mtid() { return __builtin_amdgcn_workitem_id_x(); }
__device__ __forceinline__ void msync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Element offset of logical group g. Flat: g * 32. Slab: row and column of
// the group inside its block; groups are asked for in increasing order, so
// the block index only moves forward from the tile's first block.
template <bool SLAB>
struct MxCursor {
  MxSlab s;
  int r, g_begin, g_end, c0, gpr;

  __device__ __forceinline__ void enter(int block) {
    r = block;
    c0 = s.col_off[r];
    const int c1 = s.col_off[r + 1];
    gpr = (c1 - c0) >> 5;
    g_begin = s.B * (c0 >> 5);
    g_end = s.B * (c1 >> 5);
  }

  // g0 < total groups: the block with first_group(r) <= g0 < first_group(r+1)
  __device__ __forceinline__ MxCursor(const MxSlab& slab, int g0) : s(slab) {
    if constexpr (SLAB) {
      int lo = 0, hi = s.n_blocks;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s.B * (s.col_off[mid] >> 5) <= g0) lo = mid; else hi = mid;
      }
      enter(lo);
    }
  }

  // g < total groups
  __device__ __forceinline__ int64_t at(int g) {
    if constexpr (SLAB) {
      while (g >= g_end) enter(r + 1);
      const int lg = g - g_begin;
      const int row = lg / gpr;
      return static_cast<int64_t>(row) * s.ld + c0 + ((lg - row * gpr) << 5);
    } else {
      return static_cast<int64_t>(g) << 5;
    }
  }
};

template <int FMT, bool SLAB>
__global__ __launch_bounds__(kMxThreads) void qcomm_mx_encode_kernel(
    const float* __restrict__ src, uint8_t* __restrict__ wire, int n_groups, MxSlab slab) {
  using F = MxFmt<FMT>;
  __shared__ __attribute__((aligned(16))) uint8_t img[kMxTileGroups * F::kGroupBytes];
  const int t = mtid();
  const int j = t & (kMxLanesPerGroup - 1);
  const int gsub = t >> 3;
  const int tile = __builtin_amdgcn_workgroup_id_x();
  const int g0 = tile * kMxTileGroups;
  const int left = n_groups - g0;
  const int ng = left < kMxTileGroups ? left : kMxTileGroups;

  MxCursor<SLAB> cur(slab, g0);
  mf32x4 v[kMxPasses];
#pragma unroll
  for (int p = 0; p < kMxPasses; ++p) {
    const int gl = p * kMxGroupsPerPass + gsub;
    v[p] = mf32x4{0.f, 0.f, 0.f, 0.f};
    if (gl < ng) v[p] = *reinterpret_cast<const mf32x4*>(src + cur.at(g0 + gl) + 4 * j);
  }

#pragma unroll
  for (int p = 0; p < kMxPasses; ++p) {
    const int gl = p * kMxGroupsPerPass + gsub;
    const unsigned b0 = mbits(v[p][0]), b1 = mbits(v[p][1]), b2 = mbits(v[p][2]),
                   b3 = mbits(v[p][3]);
    const MxScale sc = mx_scale_of<F::kEmax, F::kMantMax>(group8_umax(mx_amax4(b0, b1, b2, b3)));
    const bool special = sc.special;
    const unsigned scale_byte = sc.byte;
    const float inv = mpow2(-sc.E);
    if (gl < ng) {
      uint8_t* gp = img + gl * F::kGroupBytes;
      if constexpr (FMT == kFmtMxfp8) {
        const unsigned codes =
            mx_fp8_pack4(v[p][0], v[p][1], v[p][2], v[p][3], inv, b0, b1, b2, b3);
        *reinterpret_cast<mu32_u*>(gp + 4 * j) = special ? 0u : codes;
      } else {
        const unsigned codes =
            mx_fp4_pack4(v[p][0], v[p][1], v[p][2], v[p][3], inv, b0, b1, b2, b3);
        *reinterpret_cast<mu16_u*>(gp + 2 * j) = static_cast<unsigned short>(special ? 0u : codes);
      }
      if (j == 0) gp[F::kScaleAt] = static_cast<uint8_t>(scale_byte);
    }
  }
  msync();

  const int nbytes = ng * F::kGroupBytes;
  const int nvec = nbytes >> 4;
  uint8_t* out = wire + static_cast<int64_t>(tile) * (kMxTileGroups * F::kGroupBytes);
  for (int i = t; i < nvec; i += kMxThreads)
    reinterpret_cast<mu32x4*>(out)[i] = reinterpret_cast<const mu32x4*>(img)[i];
  // last tile only: fewer than 16 trailing bytes
  for (int i = (nvec << 4) + t; i < nbytes; i += kMxThreads) out[i] = img[i];
}

template <int FMT, bool SLAB>
__global__ __launch_bounds__(kMxThreads) void qcomm_mx_decode_kernel(
    const uint8_t* __restrict__ wire, float* __restrict__ dst, int n_groups, MxSlab slab) {
  using F = MxFmt<FMT>;
  __shared__ __attribute__((aligned(16))) uint8_t img[kMxTileGroups * F::kGroupBytes];
  const int t = mtid();
  const int j = t & (kMxLanesPerGroup - 1);
  const int gsub = t >> 3;
  const int tile = __builtin_amdgcn_workgroup_id_x();
  const int g0 = tile * kMxTileGroups;
  const int left = n_groups - g0;
  const int ng = left < kMxTileGroups ? left : kMxTileGroups;

  const int nbytes = ng * F::kGroupBytes;
  const int nvec = nbytes >> 4;
  const uint8_t* in = wire + static_cast<int64_t>(tile) * (kMxTileGroups * F::kGroupBytes);
  for (int i = t; i < nvec; i += kMxThreads)
    reinterpret_cast<mu32x4*>(img)[i] = reinterpret_cast<const mu32x4*>(in)[i];
  for (int i = (nvec << 4) + t; i < nbytes; i += kMxThreads) img[i] = in[i];
  msync();

  MxCursor<SLAB> cur(slab, g0);
#pragma unroll
  for (int p = 0; p < kMxPasses; ++p) {
    const int gl = p * kMxGroupsPerPass + gsub;
    if (gl < ng) {
      const uint8_t* gp = img + gl * F::kGroupBytes;
      const int sb = gp[F::kScaleAt];
      const float scale = mpow2(sb - 127);
      mf32x4 o;
      if constexpr (FMT == kFmtMxfp8) {
        const int w = static_cast<int>(*reinterpret_cast<const mu32_u*>(gp + 4 * j));
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
        const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
        o = mf32x4{lo[0] * scale, lo[1] * scale, hi[0] * scale, hi[1] * scale};
      } else {
        const unsigned w = *reinterpret_cast<const mu16_u*>(gp + 2 * j);
        const auto lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 0);
        const auto hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 1);
        o = mf32x4{lo[0] * scale, lo[1] * scale, hi[0] * scale, hi[1] * scale};
      }
      if (sb == 0xFF) {
        const float nan = __builtin_nanf("");
        o = mf32x4{nan, nan, nan, nan};
      }
      *reinterpret_cast<mf32x4*>(dst + cur.at(g0 + gl) + 4 * j) = o;
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

inline hipStream_t mx_stream() {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

int mx_group_bytes(int64_t fmt) {
  TORCH_CHECK(fmt == kFmtMxfp8 || fmt == kFmtMxfp4, "qcomm_mx: unknown format id ", fmt);
  return fmt == kFmtMxfp8 ? MxFmt<kFmtMxfp8>::kGroupBytes : MxFmt<kFmtMxfp4>::kGroupBytes;
}

// Validates the slab description against the [B, sum_D] matrix. An empty
// col_off selects flat addressing.
MxSlab mx_slab(const at::Tensor& col_off, const at::Tensor& mat, int64_t B) {
  MxSlab s{nullptr, 0, 0, 0};
  if (col_off.numel() == 0) return s;
  TORCH_CHECK(col_off.is_cuda() && col_off.scalar_type() == at::kInt && col_off.is_contiguous() &&
                  col_off.numel() >= 2,
              "qcomm_mx: col_off must be a device int32 vector of n_blocks + 1 entries");
  TORCH_CHECK(mat.dim() == 2 && mat.size(0) == B && mat.is_contiguous() && mat.size(1) % 32 == 0,
              "qcomm_mx: slab mode takes a contiguous [B, sum_D] matrix with sum_D % 32 == 0");
  s.col_off = col_off.data_ptr<int>();
  s.n_blocks = static_cast<int>(col_off.numel() - 1);
  s.B = static_cast<int>(B);
  s.ld = mat.size(1);
  return s;
}

template <int FMT>
void launch_encode(const float* src, uint8_t* wire, int n_groups, const MxSlab& s) {
  const dim3 grid((n_groups + kMxTileGroups - 1) / kMxTileGroups), block(kMxThreads);
  if (s.col_off != nullptr)
    hipLaunchKernelGGL((qcomm_mx_encode_kernel<FMT, true>), grid, block, 0, mx_stream(), src, wire,
                       n_groups, s);
  else
    hipLaunchKernelGGL((qcomm_mx_encode_kernel<FMT, false>), grid, block, 0, mx_stream(), src,
                       wire, n_groups, s);
}

template <int FMT>
void launch_decode(const uint8_t* wire, float* dst, int n_groups, const MxSlab& s) {
  const dim3 grid((n_groups + kMxTileGroups - 1) / kMxTileGroups), block(kMxThreads);
  if (s.col_off != nullptr)
    hipLaunchKernelGGL((qcomm_mx_decode_kernel<FMT, true>), grid, block, 0, mx_stream(), wire, dst,
                       n_groups, s);
  else
    hipLaunchKernelGGL((qcomm_mx_decode_kernel<FMT, false>), grid, block, 0, mx_stream(), wire,
                       dst, n_groups, s);
}

}  // namespace

int64_t qcomm_mx_tile_groups() { return kMxTileGroups; }

// fp32 message -> int8 wire. Flat: any contiguous src. Slab (col_off given):
// src is the [B, sum_D] matrix and sum_D == col_off[-1] (checked by the
// caller, which built col_off).
at::Tensor qcomm_mx_encode(const at::Tensor& src, int64_t fmt, const at::Tensor& col_off,
                           int64_t B) {
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == at::kFloat, "qcomm_mx_encode: fp32 on GPU");
  const int gb = mx_group_bytes(fmt);
  at::Tensor x = src.contiguous();
  if (reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 != 0) x = x.clone();
  TORCH_CHECK(x.numel() % 32 == 0, "qcomm_mx_encode: numel % 32 != 0");
  TORCH_CHECK(x.numel() / 32 < (int64_t{1} << 31) - kMxTileGroups, "qcomm_mx_encode: too large");
  const int n_groups = static_cast<int>(x.numel() / 32);
  const MxSlab s = mx_slab(col_off, x, B);
  at::Tensor wire = at::empty({static_cast<int64_t>(n_groups) * gb}, x.options().dtype(at::kChar));
  if (n_groups == 0) return wire;
  uint8_t* wp = reinterpret_cast<uint8_t*>(wire.data_ptr<int8_t>());
  if (fmt == kFmtMxfp8)
    launch_encode<kFmtMxfp8>(x.data_ptr<float>(), wp, n_groups, s);
  else
    launch_encode<kFmtMxfp4>(x.data_ptr<float>(), wp, n_groups, s);
  TREC_HIP_CHECK(hipGetLastError());
  return wire;
}

// int8 wire -> fp32, into ``out``: flat [numel], or with col_off the
// contiguous [B, sum_D] matrix. Every element of ``out`` is written.
void qcomm_mx_decode(const at::Tensor& wire, at::Tensor out, int64_t fmt,
                     const at::Tensor& col_off, int64_t B) {
  TORCH_CHECK(wire.is_cuda() && wire.element_size() == 1, "qcomm_mx_decode: byte wire on GPU");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat && out.is_contiguous() &&
                  reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
              "qcomm_mx_decode: out must be contiguous, 16-byte aligned fp32 on GPU");
  const int gb = mx_group_bytes(fmt);
  const int64_t numel = out.numel();
  TORCH_CHECK(numel % 32 == 0, "qcomm_mx_decode: numel % 32 != 0");
  TORCH_CHECK(numel / 32 < (int64_t{1} << 31) - kMxTileGroups, "qcomm_mx_decode: too large");
  const int n_groups = static_cast<int>(numel / 32);
  TORCH_CHECK(wire.numel() == static_cast<int64_t>(n_groups) * gb,
              "qcomm_mx_decode: wire has ", wire.numel(), " bytes, expected ",
              static_cast<int64_t>(n_groups) * gb);
  at::Tensor w = wire.contiguous();
  if (reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 != 0) w = w.clone();
  const MxSlab s = mx_slab(col_off, out, B);
  if (n_groups == 0) return;
  const uint8_t* wp = reinterpret_cast<const uint8_t*>(w.data_ptr());
  if (fmt == kFmtMxfp8)
    launch_decode<kFmtMxfp8>(wp, out.data_ptr<float>(), n_groups, s);
  else
    launch_decode<kFmtMxfp4>(wp, out.data_ptr<float>(), n_groups, s);
  TREC_HIP_CHECK(hipGetLastError());
}

}  // namespace trec_amd
