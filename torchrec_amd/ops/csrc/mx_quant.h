// Device helpers of the OCP MX quantizers (qcomm_codec.hip, mx_linear.hip):
// group amax over eight lanes, amax -> E8M0 scale, four fp32 -> four e4m3 or
// four e2m1 codes. The scale rule and its special cases are the ones written out at the
// top of qcomm_codec.hip; distributed/qcomm_codecs.py is the oracle.
//
// Everything here is built without the packed fp32 VALU forms (see
// cross_mfma.hip), so it inlines into the kernels of those files, and uses
// builtins rather than header helpers.
#pragma once

#include <cstdint>

namespace trec_amd {

// Element formats: bytes of a wire group and where its scale byte sits
// (qcomm_codec.hip), the exponent of elem_max and elem_max's mantissa bits.
constexpr int kFmtMxfp8 = 0;
constexpr int kFmtMxfp4 = 1;

template <int FMT>
struct MxFmt;
template <>
struct MxFmt<kFmtMxfp8> {
  static constexpr int kGroupBytes = 33, kScaleAt = 32, kEmax = 8;
  static constexpr unsigned kMantMax = 0x600000u;  // 448 = 1.75 * 2^8
};
template <>
struct MxFmt<kFmtMxfp4> {
  static constexpr int kGroupBytes = 17, kScaleAt = 16, kEmax = 2;
  static constexpr unsigned kMantMax = 0x400000u;  // 6 = 1.5 * 2^2
};

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

__device__ __forceinline__ unsigned mumax(unsigned a, unsigned b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned mbits(float v) { return __builtin_bit_cast(unsigned, v); }

// 2^e for e in [-127, 127]; 2^-127 is the fp32 subnormal 0x00400000.
__device__ __forceinline__ float mpow2(int e) {
  return __builtin_bit_cast(float, e > -127 ? static_cast<unsigned>(e + 127) << 23 : 0x00400000u);
}

// max over the eight lanes of a group: lane^1, lane^2 by quad permutes, then
// the other quad by a mirror of the half row (every lane of a quad already
// holds the quad's max).
__device__ __forceinline__ unsigned group8_umax(unsigned a) {
  a = mumax(a, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(a), 0xB1, 0xF, 0xF, false)));
  a = mumax(a, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(a), 0x4E, 0xF, 0xF, false)));
  a = mumax(a, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(a), 0x141, 0xF, 0xF, false)));
  return a;
}

// |x| bit pattern max of four values (NaN and Inf sort above every finite value)
__device__ __forceinline__ unsigned mx_amax4(unsigned b0, unsigned b1, unsigned b2, unsigned b3) {
  return mumax(mumax(b0 & 0x7FFFFFFFu, b1 & 0x7FFFFFFFu), mumax(b2 & 0x7FFFFFFFu, b3 & 0x7FFFFFFFu));
}

// The group's scale from its amax bits: E (clamped), the stored byte and
// whether the group stores zero codes (non-finite or all zero).
struct MxScale {
  int E;
  unsigned byte;
  bool special;
};

template <int EMAX, unsigned MANT_MAX>
__device__ __forceinline__ MxScale mx_scale_of(unsigned a) {
  const int ex = static_cast<int>(a >> 23);
  const bool nonfinite = ex == 255;
  int E = ex - 127 - EMAX + ((a & 0x7FFFFFu) > MANT_MAX ? 1 : 0);
  E = E < -127 ? -127 : (E > 127 ? 127 : E);
  MxScale s;
  s.E = E;
  s.byte = nonfinite ? 0xFFu : (a == 0u ? 0u : static_cast<unsigned>(E + 127));
  s.special = nonfinite || a == 0u;
  return s;
}

// Four values times inv = 2^-E -> four e4m3fn codes, element i in byte i.
// The clamp acts only where E was clamped; the convert rounds to nearest even
// and the sign bit is taken from x itself (b0..b3 are the values' bits).
__device__ __forceinline__ unsigned mx_fp8_pack4(float v0, float v1, float v2, float v3, float inv,
                                                 unsigned b0, unsigned b1, unsigned b2,
                                                 unsigned b3) {
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_fmed3f(v0 * inv, -448.f, 448.f),
                                      __builtin_amdgcn_fmed3f(v1 * inv, -448.f, 448.f), w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_fmed3f(v2 * inv, -448.f, 448.f),
                                      __builtin_amdgcn_fmed3f(v3 * inv, -448.f, 448.f), w, true);
  const unsigned signs = ((b0 >> 31) << 7) | ((b1 >> 31) << 15) | ((b2 >> 31) << 23) |
                         ((b3 >> 31) << 31);
  return (static_cast<unsigned>(w) & 0x7F7F7F7Fu) | signs;
}

// Four values times inv = 2^-E -> four e2m1 codes in the low 16 bits,
// element i in nibble i. The scaled convert runs with a unit scale: the
// multiply already applied 2^-E, which also covers E = -127 (a subnormal
// factor the instruction's exponent-only scale operand cannot carry). Clamp
// and signs as in mx_fp8_pack4.
__device__ __forceinline__ unsigned mx_fp4_pack4(float v0, float v1, float v2, float v3, float inv,
                                                 unsigned b0, unsigned b1, unsigned b2,
                                                 unsigned b3) {
  unsigned w = 0;
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, __builtin_amdgcn_fmed3f(v0 * inv, -6.f, 6.f),
                                               __builtin_amdgcn_fmed3f(v1 * inv, -6.f, 6.f), 1.0f,
                                               0);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, __builtin_amdgcn_fmed3f(v2 * inv, -6.f, 6.f),
                                               __builtin_amdgcn_fmed3f(v3 * inv, -6.f, 6.f), 1.0f,
                                               1);
  const unsigned signs = ((b0 >> 31) << 3) | ((b1 >> 31) << 7) | ((b2 >> 31) << 11) |
                         ((b3 >> 31) << 15);
  return (w & 0x7777u) | signs;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace trec_amd
