// MXFP8 linear layer for serving, MI355X (gfx950), on the block-scaled MFMA
// v_mfma_scale_f32_16x16x128_f8f6f4.
//
//   y = act( Qx(x) . Qw(W)^T + b )
//
// x [M, K] fp32 or bf16, W [N, K], b [N] fp32 or absent, act none or ReLU, y
// fp32 or bf16. Q is the MXFP8 quantization of the qcomm codec (mx_quant.h;
// oracle distributed/qcomm_codecs.py) on groups of 32 consecutive k of a
// row: e4m3fn codes and one E8M0 scale byte per group, a ragged last group
// padded with zeros. Products and sums are fp32 inside the MFMA and across K
// steps; bias and activation act on the fp32 accumulator; y rounds once.
//
// Non-finite inputs: a group holding NaN or Inf stores zero codes and the
// scale byte 0xFF, which E8M0 defines as NaN. The MFMA multiplies the
// group's products by that scale, so every output the group feeds is NaN:
// the whole output row for a group of x, the whole output column for a group
// of W. (ReLU keeps NaN: the compare that clears negatives is false for it.)
//
// Weights are packed once (mx_linear_pack_weight): codes uint8 [N, Kp], Kp =
// K rounded up to 128, zero codes in the padding; scales uint8 [N, Kp / 32].
// A thread owns four consecutive k, eight lanes a group, as in the codec.
//
// Operand layout of the 16x16x128 MFMA with 8-bit operands, as measured on
// the MI355X (each operand is 8 VGPRs = 32 bytes): lane l, with kb = l >> 4,
// supplies for operand row l & 15 the k bytes [16 kb, 16 kb + 16) in
// registers 0-3 and [64 + 16 kb, 64 + 16 kb + 16) in registers 4-7. The scale
// of the 32-block j (k in [32 j, 32 j + 32)) is taken from the lanes with
// kb = j, byte 0 of their scale VGPR under op_sel 0. So a lane's 32 bytes are
// NOT one MX group: the halves of lanes kb = 0, 1 make up blocks 0 and 2,
// those of kb = 2, 3 blocks 1 and 3, while lane group kb carries block kb's
// scale. (Reading 32 consecutive bytes per lane gives the right sum only
// where all four scales of a row are equal.) Operand order is
// the project's swapped one, mfma(weights, activations): D'[n][m], so lane l
// ends with the four consecutive columns n = 4 (l >> 4) + i of row m = l & 15
// and the epilogue stores 16 B of fp32 or 8 B of bf16.
//
// GEMM: a workgroup owns a [BM, BN] output tile and walks K in steps of 128.
// Per step the [BN, 128] weight codes go global -> registers -> LDS as 16-B
// chunks (128-B rows, the 16-B slots XOR-swizzled with row & 7 as in
// cross_mfma.hip) with one scale dword per row; the [BM, 128] activation
// slice is loaded as fp32 / bf16, four k per thread, and quantized in
// registers (group amax over eight lanes in three DPP steps, packed convert)
// on its way to LDS. Quantized activations never reach global memory. The
// stage is double-buffered: the global loads of step s + 1 are issued before
// the MFMA loop of step s and written to the other buffer after it, one
// barrier per step.
//
// Two instantiations, chosen on the host (mx_pick_big):
//   small  BM 16, BN  32, 2 waves (one 16x16 tile each): serving batches; a
//          1024-wide layer at M = 16 still makes 32 workgroups.
//   big    BM 64, BN 128, 4 waves (2 x 4 tiles each): taken once its grid has
//          a workgroup for every CU; reads each weight byte M / 64 times
//          instead of M / 16 and quantizes x N / 128 times instead of N / 32.
// Rows, columns and k outside the matrices read as zero, never as memory;
// stores are clipped. One launch on the current stream, no host sync, no
// allocation but the output.
//
// MXFP8 between layers (XT / OT = uint8_t). An activation may arrive, and a
// result may leave, as the pair a packed weight is: codes uint8 [M, Kp] and
// scales uint8 [M, Kp / 32], groups of 32 consecutive features of a row.
//   in   the [BM, 128] code slice takes the weight codes' road (16-B chunks,
//        the same swizzle) and one scale dword per row and step lands in
//        kAScale: no float load, no amax, no convert. The K walk and the MFMA
//        sequence of an output element are those of the float-in path.
//   out  after bias and ReLU the epilogue quantizes groups of 32 output
//        columns. A lane holds columns 4 (l >> 4) + i of row l & 15 of a
//        16 x 16 tile, so a group is two adjacent tiles and its amax spans
//        the four l >> 4 lane groups of both: the lane's values in registers,
//        then lane ^ 16 and lane ^ 32. Big tile: a wave's 64 columns are
//        contiguous, both tiles are its own. Small tile: its two waves hold
//        one half each and swap their 16 row maxima through the stage buffers,
//        which are free after the K walk's last barrier, at one more barrier
//        (measured against a one-wave 16 x 32 instantiation, which was 18-29%
//        slower per layer: half the lanes issue the stage's loads). Columns
//        at or past N count as zero. Each lane stores one dword of four codes
//        per tile and one lane per row and group the scale byte. The last
//        column workgroup also writes the padding up to Np = N rounded up to
//        128 (zero codes, scale 0), so the pair is the next layer's operand
//        as it stands.
//
// MXFP4 weights (WF = kFmtMxfp4, W4A8). The MFMA takes a format per operand:
// cbsz 4 makes the first (weight) operand e2m1 in 4 VGPRs, blgp 0 leaves the
// activations e4m3, so everything on the activation side and all three
// epilogues are shared with WF = kFmtMxfp8. Packed weight: codes uint8
// [N, Kp / 2] in natural order (element 2k in the low, 2k + 1 in the high
// nibble of byte k, the qcomm codec's MXFP4 bytes), scales [N, Kp / 32] as
// before. Operand layout, measured on the MI355X with one-hot probes (one
// e2m1 1.0 in one nibble of one register of one lane; the e4m3 operand, in
// the layout above, holds bit m of k in row m, so the output row spells k):
// lane l, kb = l >> 4, supplies for operand row l & 15 the 32 nibbles of k
// [32 kb, 32 kb + 32): register r holds k [32 kb + 8 r, 32 kb + 8 r + 8),
// nibble i of it k 32 kb + 8 r + i. Registers 4-7 are not read. Block j's
// scale still comes from byte 0 of the scale register of the lanes with
// kb = j, for either operand; bytes 1-3 are ignored. So, unlike e4m3, a lane
// group's registers ARE one MX group, and a lane reads bytes [16 kb, 16 kb +
// 16) of the row's 64 in one 16-B piece. Stage: 64-B weight rows, four 16-B
// chunks per row (NW = BN * 4 / T: one per thread in the small tile, two in
// the big one, half the e4m3 count), the slot XORed with (row >> 2) & 3: four
// rows span the banks' 256 B, so the 16 rows a lane group reads hit 16
// different 16-B bank groups. Every e2m1 value is an e4m3 value: the decoded
// weight repacked as MXFP8 through the e4m3 kernel gives the same result up
// to the MFMA's internal summation (bit-equal at the three smallest test
// shapes, within 2e-3 absolute at K = 300, 479 and 1024 on the test inputs).

#include <torch/extension.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <tuple>
#include <type_traits>
#include <vector>

#include "common.h"
#include "mx_quant.h"

namespace trec_amd {

namespace {

// Device code of this file is built without the packed fp32 VALU forms (see
// cross_mfma.hip): everything the kernels call is defined between the push
// and the pop or in mx_quant.h, with builtins rather than header helpers.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

typedef __attribute__((ext_vector_type(4))) float lf32x4;
typedef __attribute__((ext_vector_type(4))) __bf16 lbf16x4;
typedef __attribute__((ext_vector_type(4))) unsigned lu32x4;  // one 16-B chunk
typedef __attribute__((ext_vector_type(8))) int li32x8;       // one MFMA operand

constexpr int kKStep = 128;    // k per MFMA and per staged tile: 128-B LDS rows
constexpr int kSlotsPerRow = kKStep / 4;  // 4-k activation slots in a staged row
constexpr int kPackThreads = 256;

__device__ __forceinline__ int ltid() { return __builtin_amdgcn_workitem_id_x(); }
__device__ __forceinline__ void lsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// XOR-swizzle of the 16-B slots inside a 128-B row
__device__ __forceinline__ int lswz(int row, int byte_in_row) {
  return byte_in_row ^ ((row & 7) << 4);
}
// ... and of the four 16-B slots inside a 64-B row of e2m1 weight codes: four
// rows fill the 256 B the banks span, so the slot turns with row >> 2 and the
// 16 rows a lane group reads (one slot each) land on 16 different bank groups
__device__ __forceinline__ int lswz4(int row, int byte_in_row) {
  return byte_in_row ^ (((row >> 2) & 3) << 4);
}

__device__ __forceinline__ lf32x4 to_f4(lf32x4 v) { return v; }
__device__ __forceinline__ lf32x4 to_f4(lbf16x4 v) {
  return lf32x4{static_cast<float>(v[0]), static_cast<float>(v[1]), static_cast<float>(v[2]),
                static_cast<float>(v[3])};
}
__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(__bf16 v) { return static_cast<float>(v); }

template <typename T>
struct Vec4Of;
template <>
struct Vec4Of<float> {
  using type = lf32x4;
};
template <>
struct Vec4Of<__bf16> {
  using type = lbf16x4;
};

// Four consecutive values of a row of length K starting at k (k % 4 == 0);
// values at or past K read as zero. vec: K % 4 == 0 and the base is aligned
// to the vector, so k < K puts all four inside the row.
template <typename T>
__device__ __forceinline__ lf32x4 load4_clipped(const T* __restrict__ row, int k, int K, bool vec) {
  if (vec) {
    if (k < K) return to_f4(*reinterpret_cast<const typename Vec4Of<T>::type*>(row + k));
    return lf32x4{0.f, 0.f, 0.f, 0.f};
  }
  lf32x4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = k + i < K ? to_f(row[k + i]) : 0.f;
  return v;
}

// Quantize this lane's four values of an MX group spread over eight lanes.
__device__ __forceinline__ void quant4(lf32x4 v, unsigned& codes, unsigned& scale_byte) {
  const unsigned b0 = mbits(v[0]), b1 = mbits(v[1]), b2 = mbits(v[2]), b3 = mbits(v[3]);
  using F = MxFmt<kFmtMxfp8>;
  const MxScale sc = mx_scale_of<F::kEmax, F::kMantMax>(group8_umax(mx_amax4(b0, b1, b2, b3)));
  const unsigned c = mx_fp8_pack4(v[0], v[1], v[2], v[3], mpow2(-sc.E), b0, b1, b2, b3);
  codes = sc.special ? 0u : c;
  scale_byte = sc.byte;
}

// W [N, K] fp32 -> codes [N, Kp] (WF MXFP4: [N, Kp / 2], element 2k in the
// low nibble of byte k), scales [N, Kp / 32]. A thread owns four k of one
// (row, group) and writes a dword (two bytes); padding groups come out as
// zero codes and scale 0.
template <int WF>
__global__ __launch_bounds__(kPackThreads) void mx_linear_pack_kernel(
    const float* __restrict__ W, int64_t N, int K, int Kp, uint8_t* __restrict__ codes,
    uint8_t* __restrict__ scales) {
  const int G = Kp >> 5;
  const int64_t slot =
      static_cast<int64_t>(__builtin_amdgcn_workgroup_id_x()) * kPackThreads + ltid();
  const int64_t gi = slot >> 3;  // (row, group), the same for the eight lanes
  const int j = static_cast<int>(slot & 7);
  const bool live = gi < N * G;
  const int64_t row = gi / G;
  const int g = static_cast<int>(gi - row * G);
  const int k = g * 32 + j * 4;
  lf32x4 v{0.f, 0.f, 0.f, 0.f};
  if (live) v = load4_clipped(W + row * K, k, K, (K & 3) == 0);
  unsigned c, sb;
  if constexpr (WF == kFmtMxfp8) {
    quant4(v, c, sb);  // every lane takes part in the DPP max
    if (live) *reinterpret_cast<unsigned*>(codes + row * Kp + k) = c;
  } else {
    const unsigned b0 = mbits(v[0]), b1 = mbits(v[1]), b2 = mbits(v[2]), b3 = mbits(v[3]);
    using F = MxFmt<kFmtMxfp4>;
    const MxScale sc = mx_scale_of<F::kEmax, F::kMantMax>(group8_umax(mx_amax4(b0, b1, b2, b3)));
    c = mx_fp4_pack4(v[0], v[1], v[2], v[3], mpow2(-sc.E), b0, b1, b2, b3);
    sb = sc.byte;
    if (live)
      *reinterpret_cast<unsigned short*>(codes + row * (Kp >> 1) + (k >> 1)) =
          static_cast<unsigned short>(sc.special ? 0u : c);
  }
  if (live && j == 0) scales[row * G + g] = static_cast<uint8_t>(sb);
}

// One buffer of the stage: [weight codes | activation codes | weight scale
// dwords | activation scale dwords]. A weight row of a step is 128 B of e4m3
// or 64 B of e2m1 codes.
template <int WF, int BM, int BN>
struct Stage {
  static constexpr int kWRow = WF == kFmtMxfp4 ? kKStep / 2 : kKStep;
  static constexpr int kWCodes = 0;
  static constexpr int kACodes = BN * kWRow;
  static constexpr int kWScale = kACodes + BM * kKStep;
  static constexpr int kAScale = kWScale + BN * 4;
  static constexpr int kBytes = kAScale + BM * 4;
};

// The MFMA operand of lane group kb for a row: k bytes [16 kb, 16 kb + 16)
// in registers 0-3 and [64 + 16 kb, 64 + 16 kb + 16) in registers 4-7
__device__ __forceinline__ li32x8 operand(const char* tile, int row, int kb) {
  const char* r = tile + row * kKStep;
  const lu32x4 lo = *reinterpret_cast<const lu32x4*>(r + lswz(row, kb * 16));
  const lu32x4 hi = *reinterpret_cast<const lu32x4*>(r + lswz(row, 64 + kb * 16));
  return li32x8{static_cast<int>(lo[0]), static_cast<int>(lo[1]), static_cast<int>(lo[2]),
                static_cast<int>(lo[3]), static_cast<int>(hi[0]), static_cast<int>(hi[1]),
                static_cast<int>(hi[2]), static_cast<int>(hi[3])};
}

// The e2m1 weight operand of lane group kb for a row: the 32 nibbles of k
// [32 kb, 32 kb + 32), bytes [16 kb, 16 kb + 16) of the 64-B row, in registers
// 0-3, element 2k in the low nibble; registers 4-7 are not read (cbsz 4)
__device__ __forceinline__ li32x8 operand4(const char* tile, int row, int kb) {
  const lu32x4 v = *reinterpret_cast<const lu32x4*>(tile + row * (kKStep / 2) +
                                                    lswz4(row, kb * 16));
  return li32x8{static_cast<int>(v[0]), static_cast<int>(v[1]), static_cast<int>(v[2]),
                static_cast<int>(v[3]), 0, 0, 0, 0};
}

// max over the four l >> 4 lane groups of a wave (all 64 lanes take part)
__device__ __forceinline__ unsigned kb4_umax(unsigned a, int l) {
  a = mumax(a, static_cast<unsigned>(
                   __builtin_amdgcn_ds_bpermute((l ^ 16) << 2, static_cast<int>(a))));
  a = mumax(a, static_cast<unsigned>(
                   __builtin_amdgcn_ds_bpermute((l ^ 32) << 2, static_cast<int>(a))));
  return a;
}

// WF: the weights' element format, kFmtMxfp8 (wcodes [N, Kp]) or kFmtMxfp4
// (wcodes [N, Kp / 2]); activations are MXFP8 in both.
// XT uint8_t: x is the activation's codes [M, Kp] and xscales its scale bytes
// [M, Kp / 32]. OT uint8_t: y is the result's codes [M, Np] and yscales its
// scale bytes [M, Np / 32], Np = N rounded up to 128.
template <int WF, typename XT, typename OT, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(WM* WN * 64) void mx_linear_fwd_kernel(
    const XT* __restrict__ x, const uint8_t* __restrict__ xscales,
    const uint8_t* __restrict__ wcodes, const uint8_t* __restrict__ wscales,
    const float* __restrict__ bias /* or nullptr */, int64_t M, int N, int K, int Kp, bool x_vec,
    bool relu, OT* __restrict__ y, uint8_t* __restrict__ yscales) {
  constexpr bool kMxIn = std::is_same_v<XT, uint8_t>, kMxOut = std::is_same_v<OT, uint8_t>;
  constexpr int T = WM * WN * 64;
  constexpr int TM = BM / 16 / WM, TN = BN / 16 / WN;  // MFMA tiles per wave
  constexpr bool kW4 = WF == kFmtMxfp4;
  constexpr int CW = kW4 ? 4 : 8, LW = kW4 ? 2 : 3;    // 16-B chunks of a weight row, log2
  constexpr int NW = BN * CW / T;                      // 16-B weight chunks per thread
  // activation per thread: 16-B code chunks, or 4-k float slots
  constexpr int NA = kMxIn ? BM * 8 / T : BM * 32 / T;
  static_assert(BM % (16 * WM) == 0 && BN % (16 * WN) == 0 && NW >= 1 && NA >= 1 && BN <= T);
  // MXFP8 out: a wave holds both 16 x 16 tiles of each of its 32-column groups,
  // or (the 16 x 32 tile) one tile of the group its two waves share
  constexpr int HT = TN == 1 ? 1 : 2, NG = TN == 1 ? 1 : TN / 2;
  static_assert(BM <= T && (!kMxOut || TN % 2 == 0 || (TN == 1 && TM == 1 && WM == 1 && WN == 2)));
  using S = Stage<WF, BM, BN>;
  __shared__ __attribute__((aligned(16))) char lds[2 * S::kBytes];

  const int t = ltid(), l = t & 63, w = t >> 6;
  const int wm = w / WN, wn = w - wm * WN;
  const int64_t m0 = static_cast<int64_t>(__builtin_amdgcn_workgroup_id_x()) * BM;
  const int n0 = __builtin_amdgcn_workgroup_id_y() * BN;
  const int G = Kp >> 5;
  const int steps = Kp / kKStep;
  const int64_t wld = kW4 ? Kp >> 1 : Kp;  // bytes of a weight code row

  lu32x4 rw[NW];
  unsigned rws = 0, ras = 0;
  std::conditional_t<kMxIn, lu32x4, lf32x4> ra[NA];

  auto fetch = [&](int s) {
    const int k0 = s * kKStep;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int c = t + i * T;
      const int row = c >> LW;
      rw[i] = n0 + row < N
                  ? *reinterpret_cast<const lu32x4*>(wcodes + static_cast<int64_t>(n0 + row) * wld +
                                                     (kW4 ? k0 >> 1 : k0) + (c & (CW - 1)) * 16)
                  : lu32x4{0u, 0u, 0u, 0u};
    }
    if (t < BN)
      rws = n0 + t < N ? *reinterpret_cast<const unsigned*>(
                             wscales + static_cast<int64_t>(n0 + t) * G + (k0 >> 5))
                       : 0u;
    if constexpr (kMxIn) {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int c = t + i * T;
        const int row = c >> 3;
        ra[i] = m0 + row < M ? *reinterpret_cast<const lu32x4*>(x + (m0 + row) * Kp + k0 +
                                                                (c & 7) * 16)
                             : lu32x4{0u, 0u, 0u, 0u};
      }
      if (t < BM)
        ras = m0 + t < M
                  ? *reinterpret_cast<const unsigned*>(xscales + (m0 + t) * G + (k0 >> 5))
                  : 0u;
    } else {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int c = t + i * T;
        const int row = c >> 5;
        ra[i] = m0 + row < M
                    ? load4_clipped(x + (m0 + row) * K, k0 + (c % kSlotsPerRow) * 4, K, x_vec)
                    : lf32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  };
  auto commit = [&](int s) {
    char* buf = lds + (s & 1) * S::kBytes;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int c = t + i * T;
      const int row = c >> LW;
      const int at = kW4 ? lswz4(row, (c & 3) * 16) : lswz(row, (c & 7) * 16);
      *reinterpret_cast<lu32x4*>(buf + S::kWCodes + row * S::kWRow + at) = rw[i];
    }
    if (t < BN) *reinterpret_cast<unsigned*>(buf + S::kWScale + t * 4) = rws;
    if constexpr (kMxIn) {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int c = t + i * T;
        const int row = c >> 3;
        *reinterpret_cast<lu32x4*>(buf + S::kACodes + row * kKStep + lswz(row, (c & 7) * 16)) =
            ra[i];
      }
      if (t < BM) *reinterpret_cast<unsigned*>(buf + S::kAScale + t * 4) = ras;
    } else {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int c = t + i * T;
        const int row = c >> 5, q = c % kSlotsPerRow;
        unsigned codes, sb;
        quant4(ra[i], codes, sb);
        *reinterpret_cast<unsigned*>(buf + S::kACodes + row * kKStep + lswz(row, q * 4)) = codes;
        if ((q & 7) == 0) buf[S::kAScale + row * 4 + (q >> 3)] = static_cast<char>(sb);
      }
    }
  };

  lf32x4 acc[TM][TN];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) acc[mi][ni] = lf32x4{0.f, 0.f, 0.f, 0.f};

  // tiles of this wave that lie inside the matrix (wave-uniform)
  const int64_t mrem = M - m0 - wm * (TM * 16);
  const int nrem = N - n0 - wn * (TN * 16);
  const int tmv = mrem <= 0 ? 0 : (mrem >= TM * 16 ? TM : static_cast<int>((mrem + 15) >> 4));
  const int tnv = nrem <= 0 ? 0 : (nrem >= TN * 16 ? TN : (nrem + 15) >> 4);
  const int kb = l >> 4;

  fetch(0);
  commit(0);
  lsync();
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) fetch(s + 1);
    const char* buf = lds + (s & 1) * S::kBytes;
    if (tmv > 0) {
      li32x8 wf[TN];
      int ws[TN];
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) {
        const int row = (wn * TN + ni) * 16 + (l & 15);
        if constexpr (kW4)
          wf[ni] = operand4(buf + S::kWCodes, row, kb);
        else
          wf[ni] = operand(buf + S::kWCodes, row, kb);
        ws[ni] = static_cast<unsigned char>(buf[S::kWScale + row * 4 + kb]);
      }
#pragma unroll
      for (int mi = 0; mi < TM; ++mi) {
        if (mi < tmv) {
          const int row = (wm * TM + mi) * 16 + (l & 15);
          const li32x8 af = operand(buf + S::kACodes, row, kb);
          const int as = static_cast<unsigned char>(buf[S::kAScale + row * 4 + kb]);
#pragma unroll
          for (int ni = 0; ni < TN; ++ni)
            if (ni < tnv)
              acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                  wf[ni], af, acc[mi][ni], kW4 ? 4 : 0, 0, 0, ws[ni], 0, as);
        }
      }
    }
    if (s + 1 < steps) commit(s + 1);
    lsync();
  }

  if constexpr (kMxOut) {
    // Every column of the tile is stored (n0 + BN <= Np); only rows clip.
    const int Np = (N + kKStep - 1) / kKStep * kKStep, Gn = Np >> 5;
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
      if (mi < tmv) {  // wave-uniform: the lane exchange below sees all 64 lanes
        const int64_t row = m0 + (wm * TM + mi) * 16 + (l & 15);
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
          const int col = n0 + (wn * TN + HT * gi) * 16 + (kb << 2);
          lf32x4 o[HT];
          unsigned b[HT][4];
#pragma unroll
          for (int h = 0; h < HT; ++h) {
            o[h] = acc[mi][HT * gi + h];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int c = col + h * 16 + i;
              if (bias != nullptr && c < N) o[h][i] += bias[c];
              if (relu) o[h][i] = o[h][i] < 0.f ? 0.f : o[h][i];
              if (c >= N) o[h][i] = 0.f;
              b[h][i] = mbits(o[h][i]);
            }
          }
          using F = MxFmt<kFmtMxfp8>;
          unsigned amax = mx_amax4(b[0][0], b[0][1], b[0][2], b[0][3]);
          if constexpr (HT == 2) amax = mumax(amax, mx_amax4(b[1][0], b[1][1], b[1][2], b[1][3]));
          amax = kb4_umax(amax, l);
          if constexpr (HT == 1) {
            // the other half of the group is the neighbouring wave's: swap
            // row maxima through the stage, free since the K walk's last
            // barrier (one row tile, so every wave arrives exactly once)
            unsigned* xch = reinterpret_cast<unsigned*>(lds);
            if (kb == 0) xch[w * 16 + (l & 15)] = amax;
            lsync();
            amax = mumax(amax, xch[(w ^ 1) * 16 + (l & 15)]);
          }
          const MxScale sc = mx_scale_of<F::kEmax, F::kMantMax>(amax);
          const float inv = mpow2(-sc.E);
          if (row < M) {
            uint8_t* dst = y + row * Np + col;
#pragma unroll
            for (int h = 0; h < HT; ++h) {
              const unsigned c = mx_fp8_pack4(o[h][0], o[h][1], o[h][2], o[h][3], inv, b[h][0],
                                              b[h][1], b[h][2], b[h][3]);
              *reinterpret_cast<unsigned*>(dst + h * 16) = sc.special ? 0u : c;
            }
            if (kb == 0 && (HT == 2 || wn == 0))
              yscales[row * Gn + (col >> 5)] = static_cast<uint8_t>(sc.byte);
          }
        }
      }
    }
    // the padding groups between the last column tile and Np
    const int pad0 = n0 + BN;
    if (pad0 >= N && pad0 < Np) {
      const int pg = (Np - pad0) >> 5;  // 1 to 3 groups, eight code dwords each
      for (int idx = t; idx < BM * pg * 8; idx += T) {
        const int r = idx / (pg * 8), d = idx - r * (pg * 8);
        if (m0 + r < M) *reinterpret_cast<unsigned*>(y + (m0 + r) * Np + pad0 + d * 4) = 0u;
      }
      for (int idx = t; idx < BM * pg; idx += T) {
        const int r = idx / pg, g = idx - r * pg;
        if (m0 + r < M) yscales[(m0 + r) * Gn + (pad0 >> 5) + g] = 0;
      }
    }
  } else {
    const bool n_vec = (N & 3) == 0;
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) {
        const int64_t row = m0 + (wm * TM + mi) * 16 + (l & 15);
        const int col = n0 + (wn * TN + ni) * 16 + (kb << 2);
        if (mi < tmv && ni < tnv && row < M && col < N) {
          lf32x4 o = acc[mi][ni];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (bias != nullptr && col + i < N) o[i] += bias[col + i];
            if (relu) o[i] = o[i] < 0.f ? 0.f : o[i];
          }
          OT* dst = y + row * N + col;
          if (n_vec) {
            if constexpr (sizeof(OT) == 4) {
              *reinterpret_cast<lf32x4*>(dst) = o;
            } else {
              *reinterpret_cast<lbf16x4*>(dst) =
                  lbf16x4{static_cast<__bf16>(o[0]), static_cast<__bf16>(o[1]),
                          static_cast<__bf16>(o[2]), static_cast<__bf16>(o[3])};
            }
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (col + i < N) dst[i] = static_cast<OT>(o[i]);
          }
        }
      }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

inline hipStream_t mxl_stream() {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

constexpr int kSmallBM = 16, kSmallBN = 32, kBigBM = 64, kBigBN = 128;

// The big tile once its grid has a workgroup for every CU.
bool mx_pick_big(int64_t M, int64_t N) {
  return ((M + kBigBM - 1) / kBigBM) * ((N + kBigBN - 1) / kBigBN) >= kNumCU;
}

// What the launch needs beyond the element types. xscales / yscales are null
// unless that side is MXFP8.
struct FwdArgs {
  const void* x;
  const uint8_t* xscales;
  const uint8_t *codes, *scales;
  const float* bias;
  int64_t M;
  int N, K, Kp;
  bool x_vec, relu;
  void* y;
  uint8_t* yscales;
};

template <int WF, typename XT, typename OT>
void launch_fwd(const FwdArgs& a) {
  const XT* xp = static_cast<const XT*>(a.x);
  OT* yp = static_cast<OT*>(a.y);
  if (mx_pick_big(a.M, a.N)) {
    const dim3 grid((a.M + kBigBM - 1) / kBigBM, (a.N + kBigBN - 1) / kBigBN);
    hipLaunchKernelGGL((mx_linear_fwd_kernel<WF, XT, OT, kBigBM, kBigBN, 2, 2>), grid, dim3(256), 0,
                       mxl_stream(), xp, a.xscales, a.codes, a.scales, a.bias, a.M, a.N, a.K, a.Kp,
                       a.x_vec, a.relu, yp, a.yscales);
  } else {
    const dim3 grid((a.M + kSmallBM - 1) / kSmallBM, (a.N + kSmallBN - 1) / kSmallBN);
    hipLaunchKernelGGL((mx_linear_fwd_kernel<WF, XT, OT, kSmallBM, kSmallBN, 1, 2>), grid, dim3(128),
                       0, mxl_stream(), xp, a.xscales, a.codes, a.scales, a.bias, a.M, a.N, a.K,
                       a.Kp, a.x_vec, a.relu, yp, a.yscales);
  }
}

template <int WF, typename XT>
void launch_fwd_out(const FwdArgs& a, int64_t output_format) {
  if (output_format == 0)
    launch_fwd<WF, XT, float>(a);
  else if (output_format == 1)
    launch_fwd<WF, XT, __bf16>(a);
  else
    launch_fwd<WF, XT, uint8_t>(a);
}

template <int WF>
void launch_fwd_in(const FwdArgs& a, bool mx_in, bool is_f32, int64_t output_format) {
  if (mx_in)
    launch_fwd_out<WF, uint8_t>(a, output_format);
  else if (is_f32)
    launch_fwd_out<WF, float>(a, output_format);
  else
    launch_fwd_out<WF, __bf16>(a, output_format);
}

void check_weight_format(const char* op, int64_t weight_format) {
  TORCH_CHECK(weight_format == kFmtMxfp8 || weight_format == kFmtMxfp4, op,
              ": weight format must be 0 (mxfp8) or 1 (mxfp4), got ", weight_format);
}

// x: fp32 / bf16 [M, K], or with xscales the codes [M, Kp] of an MXFP8
// activation. output_format: 0 fp32, 1 bf16, 2 MXFP8 (y is then the codes
// [M, Np] and the second tensor the scales [M, Np / 32]; otherwise the second
// tensor is undefined). weight_format: kFmtMxfp8 (codes [N, Kp]) or kFmtMxfp4
// (codes [N, Kp / 2]).
std::tuple<at::Tensor, at::Tensor> mx_fwd(const char* op, const at::Tensor& x,
                                          const c10::optional<at::Tensor>& xscales,
                                          const at::Tensor& codes, const at::Tensor& scales,
                                          const c10::optional<at::Tensor>& bias, int64_t K,
                                          bool relu, int64_t output_format,
                                          int64_t weight_format) {
  const bool mx_in = xscales.has_value() && xscales->defined();
  check_weight_format(op, weight_format);
  TORCH_CHECK(K >= 1 && K < (int64_t{1} << 30), op, ": K is ", K);
  const int64_t Kp = (K + kKStep - 1) / kKStep * kKStep;
  const int64_t wld = weight_format == kFmtMxfp4 ? Kp / 2 : Kp;
  if (mx_in) {
    TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.scalar_type() == at::kByte &&
                    x.size(1) == Kp && x.is_contiguous(),
                op, ": activation codes must be contiguous uint8 [M, ", Kp, "] on the GPU");
    TORCH_CHECK(xscales->is_cuda() && xscales->scalar_type() == at::kByte &&
                    xscales->dim() == 2 && xscales->size(0) == x.size(0) &&
                    xscales->size(1) == Kp / 32 && xscales->is_contiguous() &&
                    xscales->device() == x.device(),
                op, ": activation scales must be contiguous uint8 [M, ", Kp / 32,
                "] on the codes' device");
    TORCH_CHECK(x.size(0) == 0 || (reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                                   reinterpret_cast<uintptr_t>(xscales->data_ptr()) % 4 == 0),
                op, ": activation codes must be 16-byte and scales 4-byte aligned");
  } else {
    TORCH_CHECK(x.is_cuda() && x.dim() == 2 &&
                    (x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16),
                op, ": x must be an fp32 or bf16 [M, K] GPU tensor");
    TORCH_CHECK(x.size(1) == K, op, ": x has ", x.size(1), " columns, K is ", K);
  }
  TORCH_CHECK(codes.is_cuda() && codes.scalar_type() == at::kByte && codes.dim() == 2 &&
                  codes.size(1) == wld && codes.is_contiguous() && codes.size(0) >= 1,
              op, ": codes must be contiguous uint8 [N, ", wld, "]");
  const int64_t N = codes.size(0);
  TORCH_CHECK(scales.is_cuda() && scales.scalar_type() == at::kByte && scales.dim() == 2 &&
                  scales.size(0) == N && scales.size(1) == Kp / 32 && scales.is_contiguous(),
              op, ": scales must be contiguous uint8 [N, ", Kp / 32, "]");
  TORCH_CHECK(codes.device() == x.device() && scales.device() == x.device(), op, ": codes (",
              codes.device(), ") and scales (", scales.device(), ") must be on x's device (",
              x.device(), ")");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(codes.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(scales.data_ptr()) % 4 == 0,
              op, ": codes must be 16-byte and scales 4-byte aligned");
  TORCH_CHECK(N < (int64_t{1} << 31) - kBigBN && N / kSmallBN < 65535, op, ": N too large");
  TORCH_CHECK(output_format >= 0 && output_format <= 2, op,
              ": output format must be 0 (fp32), 1 (bf16) or 2 (mxfp8), got ", output_format);
  const float* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == at::kFloat && bias->numel() == N &&
                    bias->is_contiguous() && bias->device() == x.device(),
                op, ": bias must be a contiguous fp32 [N] tensor on x's device");
    bp = bias->data_ptr<float>();
  }
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  const int64_t M = x.size(0);
  at::Tensor y, ys;
  if (output_format == 2) {
    const int64_t Np = (N + kKStep - 1) / kKStep * kKStep;
    y = at::empty({M, Np}, x.options().dtype(at::kByte));
    ys = at::empty({M, Np / 32}, x.options().dtype(at::kByte));
  } else {
    y = at::empty({M, N}, x.options().dtype(output_format == 1 ? at::kBFloat16 : at::kFloat));
  }
  if (M == 0) return {y, ys};
  const at::Tensor xc = x.contiguous();
  const bool is_f32 = xc.scalar_type() == at::kFloat;
  FwdArgs a;
  a.x = xc.data_ptr();
  a.xscales = mx_in ? xscales->data_ptr<uint8_t>() : nullptr;
  a.codes = codes.data_ptr<uint8_t>();
  a.scales = scales.data_ptr<uint8_t>();
  a.bias = bp;
  a.M = M;
  a.N = static_cast<int>(N);
  a.K = static_cast<int>(K);
  a.Kp = static_cast<int>(Kp);
  a.x_vec = !mx_in && K % 4 == 0 &&
            reinterpret_cast<uintptr_t>(xc.data_ptr()) % (is_f32 ? 16 : 8) == 0;
  a.relu = relu;
  a.y = y.data_ptr();
  a.yscales = output_format == 2 ? ys.data_ptr<uint8_t>() : nullptr;
  if (weight_format == kFmtMxfp4)
    launch_fwd_in<kFmtMxfp4>(a, mx_in, is_f32, output_format);
  else
    launch_fwd_in<kFmtMxfp8>(a, mx_in, is_f32, output_format);
  TREC_HIP_CHECK(hipGetLastError());
  return {y, ys};
}

}  // namespace

int64_t mx_linear_widest_tile() { return kBigBN; }

std::tuple<at::Tensor, at::Tensor> mx_linear_pack_weight(const at::Tensor& W,
                                                         int64_t weight_format) {
  check_weight_format("mx_linear_pack_weight", weight_format);
  TORCH_CHECK(W.is_cuda() && W.dim() == 2 && W.scalar_type() == at::kFloat,
              "mx_linear_pack_weight: W must be an fp32 [N, K] GPU tensor");
  const int64_t N = W.size(0), K = W.size(1);
  TORCH_CHECK(N >= 1 && K >= 1 && K < (int64_t{1} << 30), "mx_linear_pack_weight: bad shape");
  const int64_t Kp = (K + kKStep - 1) / kKStep * kKStep;
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(W.device());
  at::Tensor Wc = W.contiguous();
  if (reinterpret_cast<uintptr_t>(Wc.data_ptr()) % 16 != 0) Wc = Wc.clone();
  const bool w4 = weight_format == kFmtMxfp4;
  at::Tensor codes = at::empty({N, w4 ? Kp / 2 : Kp}, W.options().dtype(at::kByte));
  at::Tensor scales = at::empty({N, Kp / 32}, W.options().dtype(at::kByte));
  const int64_t slots = N * (Kp / 32) * 8;
  const dim3 grid((slots + kPackThreads - 1) / kPackThreads);
  if (w4)
    hipLaunchKernelGGL(mx_linear_pack_kernel<kFmtMxfp4>, grid, dim3(kPackThreads), 0, mxl_stream(),
                       Wc.data_ptr<float>(), N, static_cast<int>(K), static_cast<int>(Kp),
                       codes.data_ptr<uint8_t>(), scales.data_ptr<uint8_t>());
  else
    hipLaunchKernelGGL(mx_linear_pack_kernel<kFmtMxfp8>, grid, dim3(kPackThreads), 0, mxl_stream(),
                       Wc.data_ptr<float>(), N, static_cast<int>(K), static_cast<int>(Kp),
                       codes.data_ptr<uint8_t>(), scales.data_ptr<uint8_t>());
  TREC_HIP_CHECK(hipGetLastError());
  return {codes, scales};
}

// output_dtype: 0 fp32, 1 bf16 (the op-level code of the TBE ops)
at::Tensor mx_linear_fwd(const at::Tensor& x, const at::Tensor& codes, const at::Tensor& scales,
                         const c10::optional<at::Tensor>& bias, int64_t K, bool relu,
                         int64_t output_dtype, int64_t weight_format) {
  TORCH_CHECK(output_dtype == 0 || output_dtype == 1,
              "mx_linear_fwd: output_dtype must be 0 (fp32) or 1 (bf16), got ", output_dtype);
  return std::get<0>(
      mx_fwd("mx_linear_fwd", x, c10::nullopt, codes, scales, bias, K, relu, output_dtype,
             weight_format));
}

// The forms with an MXFP8 activation on either side: x_scales given, x is the
// codes of an activation of K features; output_format 2, the result is
// {codes [M, Np], scales [M, Np / 32]} instead of {y}.
std::vector<at::Tensor> mx_linear_fwd_act(const at::Tensor& x,
                                          const c10::optional<at::Tensor>& x_scales,
                                          const at::Tensor& codes, const at::Tensor& scales,
                                          const c10::optional<at::Tensor>& bias, int64_t K,
                                          bool relu, int64_t output_format,
                                          int64_t weight_format) {
  auto [y, ys] = mx_fwd("mx_linear_fwd_act", x, x_scales, codes, scales, bias, K, relu,
                        output_format, weight_format);
  if (output_format == 2) return {y, ys};
  return {y};
}

}  // namespace trec_amd
