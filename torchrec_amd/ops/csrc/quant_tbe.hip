// Rowwise-quantized inference TBE for MI355X (gfx950): the INT8 kernels, and
// below them the n-bit (INT8/INT4/INT2 and FP8, mixed per table) kernels.
//
// MI355X-native equivalent of the reference's IntNBitTableBatchedEmbeddingBags
// (reference torchrec/distributed/quant_embedding_kernel.py:237; kernel spec:
// triton_tbe _nbit_TBE_forward_kernel :3051 with per-row scale/bias and
// cacheline-aligned rows :3429).
//
// Row format: [uint8 x D][fp16 scale][fp16 bias], padded to 16 B so rows load
// as uchar4/uint4. Dequant: w = q * scale + bias.
//
// FP8 row format: [e4m3fn codes: D bytes][fp16 scale][2 zero bytes][zero
// padding], stride round_up(D + 4, 16) (the INT8 stride), D % 4 == 0. The
// codes are OCP e4m3fn, the format gfx950 converts natively (NOT MI300's
// e4m3fnuz). No bias: e4m3 is signed.
//   amax    = max |x| over the row
//   scale_h = the smallest fp16 >= amax / 448 (round UP, so |x| / scale_h
//             <= 448 and nothing saturates); amax == 0 gives scale_h = 0 and
//             all codes 0
//   code    = e4m3fn_rne(clamp(x / float(scale_h), -448, 448)); the NaN
//             codes 0x7f / 0xff are never produced
//   dequant = decode(code) * float(scale_h), in fp32
// Inputs are assumed finite with amax <= 448 * 65504.

#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <hip/hip_fp16.h>

#include "common.h"
#include "quant_remap.h"

namespace trec_amd {

// UVM-capable pointer: host-pinned packed tables are addressed by the
// kernels over PCIe (QUANT_UVM compute kernel)
template <typename T>
static T* uvm_ptr(const at::Tensor& t) {
  if (t.numel() == 0) return nullptr;
  if (t.is_cuda()) return t.data_ptr<T>();
  TORCH_CHECK(t.is_pinned(), "quant TBE host-resident tensors must be pinned");
  void* dp = nullptr;
  TREC_HIP_CHECK(hipHostGetDevicePointer(&dp, t.data_ptr(), 0));
  return static_cast<T*>(dp);
}


static inline hipStream_t q_stream() {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

__host__ __device__ inline int64_t int8_row_stride(int D) {
  return ((D + 4 /*scale+bias*/ + 15) / 16) * 16;
}

// ---------------------------------------------------------------------------
// fp32 [R, D] -> int8 rowwise quantized [R, row_stride] bytes
// ---------------------------------------------------------------------------

// one wave quantises one row; lane l of the wave. Shared by the whole-table
// kernel and quant_tbe_update_rows_kernel. Writes [0, D + 4) of orow only.
__device__ __forceinline__ void quantize_row_int8(const float* __restrict__ row, int D,
                                                  uint8_t* __restrict__ orow, int l) {
  float mn = INFINITY, mx = -INFINITY;
  for (int d = l; d < D; d += kWaveSize) {
    float v = row[d];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int off = kWaveSize / 2; off > 0; off >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, off, kWaveSize));
    mx = fmaxf(mx, __shfl_xor(mx, off, kWaveSize));
  }
  float scale = (mx - mn) / 255.f;
  float inv = scale > 0.f ? 1.f / scale : 0.f;
  for (int d = l; d < D; d += kWaveSize) {
    float q = (row[d] - mn) * inv;
    orow[d] = static_cast<uint8_t>(fminf(fmaxf(q + 0.5f, 0.f), 255.f));
  }
  if (l == 0) {
    __half* sb = reinterpret_cast<__half*>(orow + D);
    sb[0] = __float2half(scale);
    sb[1] = __float2half(mn);
  }
}

__global__ void quantize_rowwise_int8_kernel(const float* __restrict__ w, int64_t R, int D,
                                             int64_t stride, uint8_t* __restrict__ out) {
  // one wave per row
  int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / kWaveSize;
  int64_t n_waves = (static_cast<int64_t>(gridDim.x) * blockDim.x) / kWaveSize;
  int l = lane_id();
  for (int64_t r = wave; r < R; r += n_waves) quantize_row_int8(w + r * D, D, out + r * stride, l);
}

at::Tensor quantize_rowwise_int8(const at::Tensor& weights) {
  TORCH_CHECK(weights.is_cuda() && weights.dim() == 2 && weights.scalar_type() == at::kFloat);
  int64_t R = weights.size(0);
  int D = weights.size(1);
  int64_t stride = int8_row_stride(D);
  auto out = at::empty({R, stride}, weights.options().dtype(at::kByte));
  if (R == 0) return out;
  auto w = weights.contiguous();
  hipLaunchKernelGGL(quantize_rowwise_int8_kernel,
                     dim3(grid_for(R * kWaveSize, kBlockThreads)), dim3(kBlockThreads), 0,
                     q_stream(), w.data_ptr<float>(), R, D, stride,
                     out.data_ptr<uint8_t>());
  return out;
}

// ---------------------------------------------------------------------------
// pooled int8 forward: same slot scheme as the fp32 TBE
//
// out_t (float / __hip_bfloat16 / __half) is the output element type of all
// four forward kernels below. Dequant, per-sample weight, the pool and the
// MEAN scale stay in fp32 registers; the value is rounded once (to nearest
// even, float2emb) in Vec4<out_t>::store. A 2-byte quad is an 8-byte store:
// an output segment starts at a multiple of 4 elements, which is all it needs.
// ---------------------------------------------------------------------------

// op-level output_dtype code (the training TBE's): 0 fp32, 1 bf16, 2 fp16
static at::ScalarType quant_out_scalar_type(int64_t output_dtype, const char* op) {
  TORCH_CHECK(output_dtype >= 0 && output_dtype <= 2, op,
              ": output_dtype must be 0 (fp32), 1 (bf16) or 2 (fp16), got ", output_dtype);
  return output_dtype == 1 ? at::kBFloat16 : (output_dtype == 2 ? at::kHalf : at::kFloat);
}

template <typename out_t, int LPS, int CHUNKS>
__global__ void __launch_bounds__(kBlockThreads) tbe_fwd_pooled_int8_kernel(
    const uint8_t* __restrict__ qweights,
    const int64_t* __restrict__ table_byte_offsets,  // [T]
    const int32_t* __restrict__ dims,                // [T]
    const int32_t* __restrict__ feat_table,          // [F]
    const int64_t* __restrict__ d_out_offsets,       // [F+1]
    const int64_t* __restrict__ indices,
    const int64_t* __restrict__ offsets,  // [F*B+1]
    const float* __restrict__ psw, int F, int B, int64_t total_D, bool mean_pool,
    out_t* __restrict__ out) {
  int sl = threadIdx.x % LPS;
  int64_t slot = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / LPS;
  int64_t n_slots = (static_cast<int64_t>(gridDim.x) * blockDim.x) / LPS;
  int64_t n_bags = static_cast<int64_t>(F) * B;
  for (int64_t bag = slot; bag < n_bags; bag += n_slots) {
    int f = bag / B;
    int b = bag - static_cast<int64_t>(f) * B;
    int t = feat_table[f];
    int D = dims[t];
    int64_t stride = int8_row_stride(D);
    const uint8_t* tab = qweights + table_byte_offsets[t];
    float4 acc[CHUNKS];
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    int64_t i0 = offsets[bag], i1 = offsets[bag + 1];
    for (int64_t i = i0; i < i1; ++i) {
      const uint8_t* row = tab + indices[i] * stride;
      const __half* sb = reinterpret_cast<const __half*>(row + D);
      float scale = __half2float(sb[0]);
      float bias = __half2float(sb[1]);
      float w = psw ? psw[i] : 1.f;
#pragma unroll
      for (int c = 0; c < CHUNKS; ++c) {
        int col4 = c * LPS + sl;
        if (col4 * 4 < D) {
          uchar4 q = reinterpret_cast<const uchar4*>(row)[col4];
          acc[c].x += w * (q.x * scale + bias);
          acc[c].y += w * (q.y * scale + bias);
          acc[c].z += w * (q.z * scale + bias);
          acc[c].w += w * (q.w * scale + bias);
        }
      }
    }
    float s = 1.f;
    if (mean_pool && i1 > i0) s = 1.f / static_cast<float>(i1 - i0);
    out_t* orow = out + static_cast<int64_t>(b) * total_D + d_out_offsets[f];
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      int col4 = c * LPS + sl;
      if (col4 * 4 < D)
        Vec4<out_t>::store(
            orow, col4, make_float4(acc[c].x * s, acc[c].y * s, acc[c].z * s, acc[c].w * s));
    }
  }
}

at::Tensor tbe_forward_pooled_int8(
    const at::Tensor& qweights, const at::Tensor& table_byte_offsets, const at::Tensor& dims,
    const at::Tensor& feat_table, const at::Tensor& d_out_offsets, const at::Tensor& indices,
    const at::Tensor& offsets, const at::Tensor& per_sample_weights, int64_t B,
    int64_t total_D, int64_t max_D, bool mean_pool, int64_t output_dtype) {
  TORCH_CHECK((qweights.is_cuda() || qweights.is_pinned()) && qweights.scalar_type() == at::kByte);
  TORCH_CHECK(max_D % 4 == 0 && max_D <= 2048);
  auto out_st = quant_out_scalar_type(output_dtype, "tbe_forward_pooled_int8");
  int F = feat_table.numel();
  auto out = at::empty({B, total_D}, indices.options().dtype(out_st));
  if (B == 0 || F == 0) return out;
  const float* psw_ptr =
      per_sample_weights.numel() > 0 ? per_sample_weights.data_ptr<float>() : nullptr;
  auto stream = q_stream();
  int lps = (max_D <= 64) ? 16 : (max_D <= 128 ? 32 : 64);
  int chunks = (int)((max_D + lps * 4 - 1) / (lps * 4));
  int grid = grid_for(static_cast<int64_t>(F) * B * lps, kBlockThreads);
#define TBE_Q_LAUNCH_T(out_t, LPS, CHUNKS)                                                \
  hipLaunchKernelGGL((tbe_fwd_pooled_int8_kernel<out_t, LPS, CHUNKS>), dim3(grid),        \
                     dim3(kBlockThreads), 0, stream, uvm_ptr<uint8_t>(qweights),           \
                     table_byte_offsets.data_ptr<int64_t>(), dims.data_ptr<int32_t>(),    \
                     feat_table.data_ptr<int32_t>(), d_out_offsets.data_ptr<int64_t>(),   \
                     indices.data_ptr<int64_t>(), offsets.data_ptr<int64_t>(), psw_ptr,   \
                     F, (int)B, total_D, mean_pool, static_cast<out_t*>(out.data_ptr()))
#define TBE_Q_LAUNCH(LPS, CHUNKS)                                  \
  do {                                                             \
    if (output_dtype == 1) TBE_Q_LAUNCH_T(__hip_bfloat16, LPS, CHUNKS); \
    else if (output_dtype == 2) TBE_Q_LAUNCH_T(__half, LPS, CHUNKS);    \
    else TBE_Q_LAUNCH_T(float, LPS, CHUNKS);                       \
  } while (0)
  if (lps == 16) TBE_Q_LAUNCH(16, 1);
  else if (lps == 32) TBE_Q_LAUNCH(32, 1);
  else switch (chunks) {
    case 1: TBE_Q_LAUNCH(64, 1); break;
    case 2: TBE_Q_LAUNCH(64, 2); break;
    case 3: case 4: TBE_Q_LAUNCH(64, 4); break;
    default: TBE_Q_LAUNCH(64, 8); break;
  }
#undef TBE_Q_LAUNCH
#undef TBE_Q_LAUNCH_T
  return out;
}

// sequence int8 forward: out[n] = dequant(row(idx[n]))
template <typename out_t, int LPS, int CHUNKS>
__global__ void __launch_bounds__(kBlockThreads) tbe_fwd_seq_int8_kernel(
    const uint8_t* __restrict__ qweights, const int64_t* __restrict__ table_byte_offsets,
    const int32_t* __restrict__ dims, const int32_t* __restrict__ feat_table,
    const int64_t* __restrict__ feat_val_offsets, const int64_t* __restrict__ indices, int F,
    int64_t N, int64_t D_out, out_t* __restrict__ out) {
  int sl = threadIdx.x % LPS;
  int64_t slot = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / LPS;
  int64_t n_slots = (static_cast<int64_t>(gridDim.x) * blockDim.x) / LPS;
  for (int64_t n = slot; n < N; n += n_slots) {
    int f = upper_bound_segment(feat_val_offsets, F, n);
    int t = feat_table[f];
    int D = dims[t];
    int64_t stride = int8_row_stride(D);
    const uint8_t* row = qweights + table_byte_offsets[t] + indices[n] * stride;
    const __half* sb = reinterpret_cast<const __half*>(row + D);
    float scale = __half2float(sb[0]);
    float bias = __half2float(sb[1]);
    out_t* orow = out + n * D_out;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      int col4 = c * LPS + sl;
      if (col4 * 4 < D) {
        uchar4 q = reinterpret_cast<const uchar4*>(row)[col4];
        Vec4<out_t>::store(orow, col4,
                           make_float4(q.x * scale + bias, q.y * scale + bias,
                                       q.z * scale + bias, q.w * scale + bias));
      }
    }
  }
}

at::Tensor tbe_forward_seq_int8(
    const at::Tensor& qweights, const at::Tensor& table_byte_offsets, const at::Tensor& dims,
    const at::Tensor& feat_table, const at::Tensor& feat_val_offsets, const at::Tensor& indices,
    int64_t D_out, int64_t max_D, int64_t output_dtype) {
  TORCH_CHECK((qweights.is_cuda() || qweights.is_pinned()) && max_D % 4 == 0 && max_D <= 2048);
  auto out_st = quant_out_scalar_type(output_dtype, "tbe_forward_seq_int8");
  int64_t N = indices.numel();
  auto out = at::empty({N, D_out}, indices.options().dtype(out_st));
  if (N == 0) return out;
  int F = feat_table.numel();
  auto stream = q_stream();
  int lps = (max_D <= 64) ? 16 : (max_D <= 128 ? 32 : 64);
  int chunks = (int)((max_D + lps * 4 - 1) / (lps * 4));
  int grid = grid_for(N * lps, kBlockThreads);
#define TBE_QS_LAUNCH_T(out_t, LPS, CHUNKS)                                               \
  hipLaunchKernelGGL((tbe_fwd_seq_int8_kernel<out_t, LPS, CHUNKS>), dim3(grid),           \
                     dim3(kBlockThreads), 0, stream, uvm_ptr<uint8_t>(qweights),           \
                     table_byte_offsets.data_ptr<int64_t>(), dims.data_ptr<int32_t>(),    \
                     feat_table.data_ptr<int32_t>(), feat_val_offsets.data_ptr<int64_t>(),\
                     indices.data_ptr<int64_t>(), F, N, D_out,                            \
                     static_cast<out_t*>(out.data_ptr()))
#define TBE_QS_LAUNCH(LPS, CHUNKS)                                  \
  do {                                                              \
    if (output_dtype == 1) TBE_QS_LAUNCH_T(__hip_bfloat16, LPS, CHUNKS); \
    else if (output_dtype == 2) TBE_QS_LAUNCH_T(__half, LPS, CHUNKS);    \
    else TBE_QS_LAUNCH_T(float, LPS, CHUNKS);                       \
  } while (0)
  if (lps == 16) TBE_QS_LAUNCH(16, 1);
  else if (lps == 32) TBE_QS_LAUNCH(32, 1);
  else switch (chunks) {
    case 1: TBE_QS_LAUNCH(64, 1); break;
    case 2: TBE_QS_LAUNCH(64, 2); break;
    case 3: case 4: TBE_QS_LAUNCH(64, 4); break;
    default: TBE_QS_LAUNCH(64, 8); break;
  }
#undef TBE_QS_LAUNCH
#undef TBE_QS_LAUNCH_T
  return out;
}

// ===========================================================================
// n-bit rows (INT8 / INT4 / INT2, and FP8), mixed per table in one launch.
//
// Row = [codes: D*bits/8 B][fp16 scale][fp16 bias][zero pad], stride rounded
// up to 16 B; D*bits % 32 == 0 so a row is a whole number of 32-bit code
// words. Element e sits at bit (e*bits)%32 of word e*bits/32, low bits first.
// For bits == 8 this is byte-for-byte the INT8 format above.
// ===========================================================================

__host__ __device__ inline int64_t nbit_row_stride(int code_bytes) {
  return ((code_bytes + 4 /*scale+bias*/ + 15) / 16) * 16;
}

// ZERO_PAD: the whole-table quantiser also zeroes the row's padding; the
// in-place row update leaves every byte past code_bytes + 4 as it is.
template <int BITS, bool ZERO_PAD = true>
__device__ __forceinline__ void quantize_row_nbit(const float* __restrict__ row, int D,
                                                  uint8_t* __restrict__ orow, int64_t stride,
                                                  int l) {
  constexpr int EPW = 32 / BITS;
  constexpr float kLevels = static_cast<float>((1 << BITS) - 1);
  float mn = INFINITY, mx = -INFINITY;
  for (int d = l; d < D; d += kWaveSize) {
    float v = row[d];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int off = kWaveSize / 2; off > 0; off >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, off, kWaveSize));
    mx = fmaxf(mx, __shfl_xor(mx, off, kWaveSize));
  }
  // codes are taken against the STORED fp16 scale/bias: at 4 and 2 bits the
  // fp16 rounding is no longer small next to a step
  __half scale_h = __float2half((mx - mn) / kLevels);
  __half bias_h = __float2half(mn);
  float scale = __half2float(scale_h);
  float bias = __half2float(bias_h);
  int n_words = D / EPW;
  uint32_t* owords = reinterpret_cast<uint32_t*>(orow);
  for (int wi = l; wi < n_words; wi += kWaveSize) {
    uint32_t word = 0;
    if (scale != 0.f) {
#pragma unroll
      for (int j = 0; j < EPW; ++j) {
        float q = floorf((row[wi * EPW + j] - bias) / scale + 0.5f);
        q = fminf(fmaxf(q, 0.f), kLevels);
        word |= static_cast<uint32_t>(q) << (j * BITS);
      }
    }
    owords[wi] = word;
  }
  if (l == 0) {
    __half* sb = reinterpret_cast<__half*>(owords + n_words);
    sb[0] = scale_h;
    sb[1] = bias_h;
  }
  // padding is part of the packed buffer (state dicts, RW row slices): zero it
  if constexpr (ZERO_PAD) {
    int n_pad = static_cast<int>(stride / 4) - n_words - 1;
    for (int k = l; k < n_pad; k += kWaveSize) owords[n_words + 1 + k] = 0u;
  }
}

template <int BITS>
__global__ void quantize_rowwise_nbit_kernel(const float* __restrict__ w, int64_t R, int D,
                                             int64_t stride, uint8_t* __restrict__ out) {
  // one wave per row
  int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / kWaveSize;
  int64_t n_waves = (static_cast<int64_t>(gridDim.x) * blockDim.x) / kWaveSize;
  int l = lane_id();
  for (int64_t r = wave; r < R; r += n_waves)
    quantize_row_nbit<BITS>(w + r * D, D, out + r * stride, stride, l);
}

at::Tensor quantize_rowwise_nbit(const at::Tensor& weights, int64_t bits) {
  TORCH_CHECK(weights.is_cuda() && weights.dim() == 2 && weights.scalar_type() == at::kFloat);
  TORCH_CHECK(bits == 4 || bits == 2, "quantize_rowwise_nbit: bits must be 4 or 2, got ", bits);
  int64_t R = weights.size(0);
  int D = weights.size(1);
  TORCH_CHECK((static_cast<int64_t>(D) * bits) % 32 == 0, "quantize_rowwise_nbit: D*bits (",
              D, "*", bits, ") must be a multiple of 32");
  int64_t stride = nbit_row_stride(static_cast<int>(D * bits / 8));
  auto out = at::empty({R, stride}, weights.options().dtype(at::kByte));
  if (R == 0) return out;
  auto w = weights.contiguous();
  int grid = grid_for(R * kWaveSize, kBlockThreads);
  if (bits == 4)
    hipLaunchKernelGGL(quantize_rowwise_nbit_kernel<4>, dim3(grid), dim3(kBlockThreads), 0,
                       q_stream(), w.data_ptr<float>(), R, D, stride, out.data_ptr<uint8_t>());
  else
    hipLaunchKernelGGL(quantize_rowwise_nbit_kernel<2>, dim3(grid), dim3(kBlockThreads), 0,
                       q_stream(), w.data_ptr<float>(), R, D, stride, out.data_ptr<uint8_t>());
  return out;
}

// ---------------------------------------------------------------------------
// fp32 [R, D] -> FP8 (e4m3fn) rowwise-scaled rows (format: top of this file)
// ---------------------------------------------------------------------------

// smallest fp16 >= v, for finite v >= 0: round to nearest, then step up once if
// that fell short. Plain arithmetic (the CPU reference does the same), no
// rounding-mode intrinsic.
__device__ __forceinline__ __half half_round_up(float v) {
  __half h = __float2half(v);
  if (__half2float(h) < v) {
    uint16_t b = __half_as_ushort(h);
    h = __ushort_as_half(static_cast<uint16_t>(b + 1));
  }
  return h;
}

__device__ __forceinline__ float fp8_prescale(float x, float scale) {
  return fminf(fmaxf(x / scale, -448.f), 448.f);
}

// one wave quantises one row (ZERO_PAD as in quantize_row_nbit)
template <bool ZERO_PAD = true>
__device__ __forceinline__ void quantize_row_fp8(const float* __restrict__ row, int D,
                                                 uint8_t* __restrict__ orow, int64_t stride,
                                                 int l) {
  int n_words = D / 4;
  float amax = 0.f;
  for (int d = l; d < D; d += kWaveSize) amax = fmaxf(amax, fabsf(row[d]));
#pragma unroll
  for (int off = kWaveSize / 2; off > 0; off >>= 1)
    amax = fmaxf(amax, __shfl_xor(amax, off, kWaveSize));
  __half scale_h = half_round_up(amax / 448.f);
  // codes are taken against the STORED scale
  float scale = __half2float(scale_h);
  uint32_t* owords = reinterpret_cast<uint32_t*>(orow);
  for (int wi = l; wi < n_words; wi += kWaveSize) {
    int word = 0;
    if (scale != 0.f) {
      const float* x = row + wi * 4;
      // packed convert: two floats -> two e4m3fn bytes (round to nearest
      // even) into the low / high half of the word
      word = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_prescale(x[0], scale),
                                             fp8_prescale(x[1], scale), word, false);
      word = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_prescale(x[2], scale),
                                             fp8_prescale(x[3], scale), word, true);
    }
    owords[wi] = static_cast<uint32_t>(word);
  }
  // scale + the two reserved zero bytes are one word
  if (l == 0) owords[n_words] = static_cast<uint32_t>(__half_as_ushort(scale_h));
  if constexpr (ZERO_PAD) {
    int n_pad = static_cast<int>(stride / 4) - n_words - 1;
    for (int k = l; k < n_pad; k += kWaveSize) owords[n_words + 1 + k] = 0u;
  }
}

__global__ void quantize_rowwise_fp8_kernel(const float* __restrict__ w, int64_t R, int D,
                                            int64_t stride, uint8_t* __restrict__ out) {
  // one wave per row
  int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / kWaveSize;
  int64_t n_waves = (static_cast<int64_t>(gridDim.x) * blockDim.x) / kWaveSize;
  int l = lane_id();
  for (int64_t r = wave; r < R; r += n_waves)
    quantize_row_fp8(w + r * D, D, out + r * stride, stride, l);
}

at::Tensor quantize_rowwise_fp8(const at::Tensor& weights) {
  TORCH_CHECK(weights.is_cuda() && weights.dim() == 2 && weights.scalar_type() == at::kFloat);
  int64_t R = weights.size(0);
  int D = weights.size(1);
  TORCH_CHECK(D > 0 && D % 4 == 0, "quantize_rowwise_fp8: D (", D, ") must be a multiple of 4");
  int64_t stride = nbit_row_stride(D);
  auto out = at::empty({R, stride}, weights.options().dtype(at::kByte));
  if (R == 0) return out;
  auto w = weights.contiguous();
  hipLaunchKernelGGL(quantize_rowwise_fp8_kernel,
                     dim3(grid_for(R * kWaveSize, kBlockThreads)), dim3(kBlockThreads), 0,
                     q_stream(), w.data_ptr<float>(), R, D, stride, out.data_ptr<uint8_t>());
  return out;
}

// Per-table format code, the values of weight_bits[t]: 8 / 4 / 2 are the
// integer widths; FP8 rows are 8 bits wide too, so they carry a code of
// their own whose low byte is still the width.
constexpr int kFormatFp8 = 0x108;

// Lane mapping. A lane owns one code unit of every row per chunk: the 32-bit
// word at INT8 (4 columns) and INT4 (8 columns), the 16-bit half-word at INT2
// (8 columns). A lane that owned a whole INT2 word would store four float4 at
// a 64 B lane stride; that form measured 39 us against INT8's 33.5 us at the
// bench shape, so no lane owns more than 8 columns (32 B, two float4).
// With a 2-byte out_t the 8 columns are 16 B, but a segment start is only a
// multiple of 4 elements (a D=20 table in front puts it at byte 40), so they
// go out as two 8-byte quads like the fp32 pair, never as one 16-byte store.
// An FP8 row maps like an INT8 row: the 32-bit word, 4 columns.
template <int FMT>
struct CodeUnit {
  static constexpr int BITS = FMT & 0xff;
  static constexpr int kCols = BITS == 8 ? 4 : 8;  // output columns per lane
  static constexpr int kBits = kCols * BITS;       // 32, 32, 16
  __device__ static __forceinline__ uint32_t load(const uint8_t* __restrict__ row, int ui) {
    if constexpr (kBits == 32) return reinterpret_cast<const uint32_t*>(row)[ui];
    else return reinterpret_cast<const uint16_t*>(row)[ui];
  }
};

// One lane's share of a bag. The format is a template parameter so the
// accumulators stay in registers; the caller switches on the bag's table.
template <typename out_t, int FMT, int LPS, int CHUNKS>
__device__ __forceinline__ void pool_bag_nbit(
    const uint8_t* __restrict__ tab, int D, const int64_t* __restrict__ indices,
    const float* __restrict__ psw, int64_t i0, int64_t i1, bool mean_pool,
    out_t* __restrict__ orow, int sl) {
  constexpr int BITS = CodeUnit<FMT>::BITS;
  constexpr int COLS = CodeUnit<FMT>::kCols;
  constexpr uint32_t kMask = (1u << BITS) - 1u;
  int code_bytes = D * BITS / 8;
  int n_units = D / COLS;
  int64_t stride = nbit_row_stride(code_bytes);
  float acc[CHUNKS][COLS];
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c)
#pragma unroll
    for (int j = 0; j < COLS; ++j) acc[c][j] = 0.f;
  for (int64_t i = i0; i < i1; ++i) {
    const uint8_t* row = tab + indices[i] * stride;
    // same address across the slot: one broadcast load
    const __half* sb = reinterpret_cast<const __half*>(row + code_bytes);
    float scale = __half2float(sb[0]);
    float bias = __half2float(sb[1]);  // FP8: the reserved bytes, unused
    float w = psw ? psw[i] : 1.f;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      int ui = c * LPS + sl;
      if (ui < n_units) {
        uint32_t unit = CodeUnit<FMT>::load(row, ui);
        if constexpr (FMT == kFormatFp8) {
          // packed convert: the low / high two e4m3fn bytes -> two floats
          auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(unit), false);
          auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(unit), true);
          acc[c][0] += w * (lo[0] * scale);
          acc[c][1] += w * (lo[1] * scale);
          acc[c][2] += w * (hi[0] * scale);
          acc[c][3] += w * (hi[1] * scale);
        } else {
#pragma unroll
          for (int j = 0; j < COLS; ++j) {
            float q = static_cast<float>((unit >> (j * BITS)) & kMask);
            acc[c][j] += w * (q * scale + bias);
          }
        }
      }
    }
  }
  float s = 1.f;
  if (mean_pool && i1 > i0) s = 1.f / static_cast<float>(i1 - i0);
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    int ui = c * LPS + sl;
    if (ui < n_units) {
#pragma unroll
      for (int k = 0; k < COLS / 4; ++k)
        Vec4<out_t>::store(orow, ui * (COLS / 4) + k,
                           make_float4(acc[c][4 * k] * s, acc[c][4 * k + 1] * s,
                                       acc[c][4 * k + 2] * s, acc[c][4 * k + 3] * s));
    }
  }
}

template <typename out_t, int LPS, int CHUNKS>
__global__ void __launch_bounds__(kBlockThreads) tbe_fwd_pooled_nbit_kernel(
    const uint8_t* __restrict__ qweights,
    const int64_t* __restrict__ table_byte_offsets,  // [T]
    const int32_t* __restrict__ dims,                // [T]
    const int32_t* __restrict__ weight_bits,         // [T] 8 / 4 / 2 / kFormatFp8
    const int32_t* __restrict__ feat_table,          // [F]
    const int64_t* __restrict__ d_out_offsets,       // [F+1]
    const int64_t* __restrict__ indices,
    const int64_t* __restrict__ offsets,  // [F*B+1]
    const float* __restrict__ psw, int F, int B, int64_t total_D, bool mean_pool,
    out_t* __restrict__ out) {
  int sl = threadIdx.x % LPS;
  int64_t slot = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / LPS;
  int64_t n_slots = (static_cast<int64_t>(gridDim.x) * blockDim.x) / LPS;
  int64_t n_bags = static_cast<int64_t>(F) * B;
  for (int64_t bag = slot; bag < n_bags; bag += n_slots) {
    int f = bag / B;
    int b = bag - static_cast<int64_t>(f) * B;
    int t = feat_table[f];
    int bits = weight_bits[t];
    int D = dims[t];
    const uint8_t* tab = qweights + table_byte_offsets[t];
    out_t* orow = out + static_cast<int64_t>(b) * total_D + d_out_offsets[f];
    int64_t i0 = offsets[bag], i1 = offsets[bag + 1];
    // bits is uniform within a slot; a wave diverges only where neighbouring
    // slots sit on a boundary between tables of different width. A slot
    // covers units [0, LPS*CHUNKS); lanes past this row's own unit count (a
    // narrow table in a module whose max is large) load and store nothing.
    if (bits == 8)
      pool_bag_nbit<out_t, 8, LPS, CHUNKS>(tab, D, indices, psw, i0, i1, mean_pool, orow, sl);
    else if (bits == 4)
      pool_bag_nbit<out_t, 4, LPS, CHUNKS>(tab, D, indices, psw, i0, i1, mean_pool, orow, sl);
    else if (bits == kFormatFp8)
      pool_bag_nbit<out_t, kFormatFp8, LPS, CHUNKS>(tab, D, indices, psw, i0, i1, mean_pool,
                                                    orow, sl);
    else
      pool_bag_nbit<out_t, 2, LPS, CHUNKS>(tab, D, indices, psw, i0, i1, mean_pool, orow, sl);
  }
}

// slot width / chunk count from the widest row in lane units (CodeUnit:
// D/4 at INT8 and FP8, D/8 at INT4 and INT2)
#define TBE_NBIT_DISPATCH(LAUNCH, max_units)                    \
  do {                                                          \
    if ((max_units) <= 8) LAUNCH(8, 1);                         \
    else if ((max_units) <= 16) LAUNCH(16, 1);                  \
    else if ((max_units) <= 32) LAUNCH(32, 1);                  \
    else if ((max_units) <= 64) LAUNCH(64, 1);                  \
    else if ((max_units) <= 128) LAUNCH(64, 2);                 \
    else if ((max_units) <= 256) LAUNCH(64, 4);                 \
    else LAUNCH(64, 8);                                         \
  } while (0)

static inline int nbit_lps(int64_t max_units) {
  return max_units <= 8 ? 8 : (max_units <= 16 ? 16 : (max_units <= 32 ? 32 : 64));
}

static void check_nbit_args(const at::Tensor& qweights, const at::Tensor& dims,
                            const at::Tensor& weight_bits, int64_t max_units) {
  TORCH_CHECK((qweights.is_cuda() || qweights.is_pinned()) && qweights.scalar_type() == at::kByte);
  TORCH_CHECK(weight_bits.scalar_type() == at::kInt && weight_bits.numel() == dims.numel(),
              "weight_bits must be int32 [T]");
  TORCH_CHECK(max_units >= 1 && max_units <= 512,
              "n-bit TBE rows must be 1..512 lane units (D/4 at INT8/FP8, D/8 at INT4/INT2), got ",
              max_units);
}

at::Tensor tbe_forward_pooled_nbit(
    const at::Tensor& qweights, const at::Tensor& table_byte_offsets, const at::Tensor& dims,
    const at::Tensor& weight_bits, const at::Tensor& feat_table,
    const at::Tensor& d_out_offsets, const at::Tensor& indices, const at::Tensor& offsets,
    const at::Tensor& per_sample_weights, int64_t B, int64_t total_D, int64_t max_units,
    bool mean_pool, int64_t output_dtype) {
  check_nbit_args(qweights, dims, weight_bits, max_units);
  // every table's D*bits % 32 == 0 makes D % 4 == 0, so rows store as float4
  TORCH_CHECK(total_D % 4 == 0, "n-bit TBE needs D*bits % 32 == 0 for every table");
  auto out_st = quant_out_scalar_type(output_dtype, "tbe_forward_pooled_nbit");
  int F = feat_table.numel();
  auto out = at::empty({B, total_D}, indices.options().dtype(out_st));
  if (B == 0 || F == 0) return out;
  const float* psw_ptr =
      per_sample_weights.numel() > 0 ? per_sample_weights.data_ptr<float>() : nullptr;
  auto stream = q_stream();
  int grid = grid_for(static_cast<int64_t>(F) * B * nbit_lps(max_units), kBlockThreads);
#define TBE_NB_LAUNCH_T(out_t, LPS, CHUNKS)                                               \
  hipLaunchKernelGGL((tbe_fwd_pooled_nbit_kernel<out_t, LPS, CHUNKS>), dim3(grid),        \
                     dim3(kBlockThreads), 0, stream, uvm_ptr<uint8_t>(qweights),           \
                     table_byte_offsets.data_ptr<int64_t>(), dims.data_ptr<int32_t>(),    \
                     weight_bits.data_ptr<int32_t>(), feat_table.data_ptr<int32_t>(),     \
                     d_out_offsets.data_ptr<int64_t>(), indices.data_ptr<int64_t>(),      \
                     offsets.data_ptr<int64_t>(), psw_ptr, F, (int)B, total_D, mean_pool, \
                     static_cast<out_t*>(out.data_ptr()))
#define TBE_NB_LAUNCH(LPS, CHUNKS)                                  \
  do {                                                              \
    if (output_dtype == 1) TBE_NB_LAUNCH_T(__hip_bfloat16, LPS, CHUNKS); \
    else if (output_dtype == 2) TBE_NB_LAUNCH_T(__half, LPS, CHUNKS);    \
    else TBE_NB_LAUNCH_T(float, LPS, CHUNKS);                       \
  } while (0)
  TBE_NBIT_DISPATCH(TBE_NB_LAUNCH, max_units);
#undef TBE_NB_LAUNCH
#undef TBE_NB_LAUNCH_T
  return out;
}

// sequence n-bit forward: out[n] = dequant(row(idx[n])), same lane mapping
template <typename out_t, int FMT, int LPS, int CHUNKS>
__device__ __forceinline__ void dequant_row_nbit(const uint8_t* __restrict__ row, int D,
                                                 int D_out, out_t* __restrict__ orow, int sl) {
  constexpr int BITS = CodeUnit<FMT>::BITS;
  constexpr int COLS = CodeUnit<FMT>::kCols;
  constexpr uint32_t kMask = (1u << BITS) - 1u;
  const __half* sb = reinterpret_cast<const __half*>(row + D * BITS / 8);
  float scale = __half2float(sb[0]);
  float bias = __half2float(sb[1]);
  // an output row holds D_out columns: never store past it
  int n_units = min(D, D_out) / COLS;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    int ui = c * LPS + sl;
    if (ui < n_units) {
      uint32_t unit = CodeUnit<FMT>::load(row, ui);
      if constexpr (FMT == kFormatFp8) {
        auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(unit), false);
        auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(unit), true);
        Vec4<out_t>::store(orow, ui, make_float4(lo[0] * scale, lo[1] * scale, hi[0] * scale,
                                                 hi[1] * scale));
      } else {
#pragma unroll
        for (int k = 0; k < COLS / 4; ++k) {
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            v[j] = static_cast<float>((unit >> ((4 * k + j) * BITS)) & kMask) * scale + bias;
          Vec4<out_t>::store(orow, ui * (COLS / 4) + k, make_float4(v[0], v[1], v[2], v[3]));
        }
      }
    }
  }
}

template <typename out_t, int LPS, int CHUNKS>
__global__ void __launch_bounds__(kBlockThreads) tbe_fwd_seq_nbit_kernel(
    const uint8_t* __restrict__ qweights, const int64_t* __restrict__ table_byte_offsets,
    const int32_t* __restrict__ dims, const int32_t* __restrict__ weight_bits,
    const int32_t* __restrict__ feat_table, const int64_t* __restrict__ feat_val_offsets,
    const int64_t* __restrict__ indices, int F, int64_t N, int D_out,
    out_t* __restrict__ out) {
  int sl = threadIdx.x % LPS;
  int64_t slot = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / LPS;
  int64_t n_slots = (static_cast<int64_t>(gridDim.x) * blockDim.x) / LPS;
  for (int64_t n = slot; n < N; n += n_slots) {
    int f = upper_bound_segment(feat_val_offsets, F, n);
    int t = feat_table[f];
    int bits = weight_bits[t];
    int D = dims[t];
    const uint8_t* row =
        qweights + table_byte_offsets[t] + indices[n] * nbit_row_stride(D * (bits & 0xff) / 8);
    out_t* orow = out + n * D_out;
    if (bits == 8) dequant_row_nbit<out_t, 8, LPS, CHUNKS>(row, D, D_out, orow, sl);
    else if (bits == 4) dequant_row_nbit<out_t, 4, LPS, CHUNKS>(row, D, D_out, orow, sl);
    else if (bits == kFormatFp8)
      dequant_row_nbit<out_t, kFormatFp8, LPS, CHUNKS>(row, D, D_out, orow, sl);
    else dequant_row_nbit<out_t, 2, LPS, CHUNKS>(row, D, D_out, orow, sl);
  }
}

at::Tensor tbe_forward_seq_nbit(
    const at::Tensor& qweights, const at::Tensor& table_byte_offsets, const at::Tensor& dims,
    const at::Tensor& weight_bits, const at::Tensor& feat_table,
    const at::Tensor& feat_val_offsets, const at::Tensor& indices, int64_t D_out,
    int64_t max_units, int64_t output_dtype) {
  check_nbit_args(qweights, dims, weight_bits, max_units);
  TORCH_CHECK(D_out % 4 == 0 && D_out <= 4096,
              "n-bit TBE needs D*bits % 32 == 0 for every table");
  auto out_st = quant_out_scalar_type(output_dtype, "tbe_forward_seq_nbit");
  int64_t N = indices.numel();
  auto out = at::empty({N, D_out}, indices.options().dtype(out_st));
  if (N == 0) return out;
  int F = feat_table.numel();
  auto stream = q_stream();
  int grid = grid_for(N * nbit_lps(max_units), kBlockThreads);
#define TBE_NBS_LAUNCH_T(out_t, LPS, CHUNKS)                                              \
  hipLaunchKernelGGL((tbe_fwd_seq_nbit_kernel<out_t, LPS, CHUNKS>), dim3(grid),           \
                     dim3(kBlockThreads), 0, stream, uvm_ptr<uint8_t>(qweights),           \
                     table_byte_offsets.data_ptr<int64_t>(), dims.data_ptr<int32_t>(),    \
                     weight_bits.data_ptr<int32_t>(), feat_table.data_ptr<int32_t>(),     \
                     feat_val_offsets.data_ptr<int64_t>(), indices.data_ptr<int64_t>(), F, \
                     N, (int)D_out, static_cast<out_t*>(out.data_ptr()))
#define TBE_NBS_LAUNCH(LPS, CHUNKS)                                  \
  do {                                                               \
    if (output_dtype == 1) TBE_NBS_LAUNCH_T(__hip_bfloat16, LPS, CHUNKS); \
    else if (output_dtype == 2) TBE_NBS_LAUNCH_T(__half, LPS, CHUNKS);    \
    else TBE_NBS_LAUNCH_T(float, LPS, CHUNKS);                       \
  } while (0)
  TBE_NBIT_DISPATCH(TBE_NBS_LAUNCH, max_units);
#undef TBE_NBS_LAUNCH
#undef TBE_NBS_LAUNCH_T
#undef TBE_NBIT_DISPATCH
  return out;
}

// ===========================================================================
// In-place row update of a served table from fp32 rows (online delta
// publishing; reference IntNBitTableBatchedEmbeddingBags in-place update).
//
// Contract:
//  * Entry n of table t's segment (upd_offsets[t] <= n < upd_offsets[t+1]) has
//    the global row id r = upd_rows[n] and the fp32 row at values +
//    val_offsets[t] + (n - upd_offsets[t]) * dims[t]. It is applied only if
//    row_lo[t] <= r < row_hi[t], to local row r - row_lo[t]; every other entry
//    is dropped here, on the device. [0, rows) bounds-checks an unsharded
//    table; a shard's own global row range lets every rank take the same full
//    delta and keep its rows. An entry whose local row would end past the
//    table's bytes in qweights (a window wider than the table) is dropped too.
//  * The first code_bytes + 4 bytes of an applied row are exactly what the
//    table's own whole-table quantiser writes for that fp32 row: format 8 is
//    quantize_row_int8 (NOT quantize_row_nbit<8>: the scale rounds
//    differently), any D; 4 / 2 are quantize_row_nbit; kFormatFp8 is
//    quantize_row_fp8.
//  * No other byte of qweights changes: not the row's padding, not its
//    neighbours, not another table.
//  * Ids within one table's segment must be unique; duplicates with different
//    values race.
//  * Ordered against lookups on the same stream only: a lookup running on
//    another stream may see codes and scale of different versions.
//  * applied[t] counts table t's applied entries. No host sync, no device
//    value read on the host: capturable in a graph.
//
// Lane mapping: one wave per entry (grid-stride over N), so the window test,
// the table search and the format switch are wave-uniform; inside a row the
// lanes stride over elements (INT8) or 32-bit code words (INT4/INT2/FP8) as
// in the whole-table quantisers, whose __device__ bodies these are.
//
// Counting: atomics on one address serialise. One atomicAdd per applied entry
// made the kernel 54 us at N = 4096, the same at every format (a whole-table
// requantise of 100k rows is 46 us). So a wave takes kUpdateEntriesPerWave
// entries, sums what it applied per table, the block's waves pool their sums
// in LDS and one lane issues one vector atomicAdd per table and block.
// ===========================================================================

constexpr int kUpdateEntriesPerWave = 4;

__global__ void __launch_bounds__(kBlockThreads) quant_tbe_update_rows_kernel(
    uint8_t* __restrict__ qweights, int64_t qweights_bytes,
    const int64_t* __restrict__ table_byte_offsets,  // [T]
    const int32_t* __restrict__ dims,                // [T]
    const int32_t* __restrict__ weight_bits,         // [T] 8 / 4 / 2 / kFormatFp8
    const int64_t* __restrict__ row_lo,              // [T]
    const int64_t* __restrict__ row_hi,              // [T]
    const int64_t* __restrict__ upd_offsets,         // [T+1]
    const int64_t* __restrict__ upd_rows,            // [N]
    const float* __restrict__ values, const int64_t* __restrict__ val_offsets,  // [T]
    int T, int64_t N, unsigned long long* __restrict__ applied) {
  constexpr int kWaves = kBlockThreads / kWaveSize;
  __shared__ int s_table[kWaves];
  __shared__ unsigned long long s_count[kWaves];
  int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / kWaveSize;
  int64_t n_waves = (static_cast<int64_t>(gridDim.x) * blockDim.x) / kWaveSize;
  int l = lane_id();
  // entries this wave applied to table pend_t and has not added to applied yet
  int pend_t = 0;
  unsigned long long pend = 0;
  for (int64_t n = wave; n < N; n += n_waves) {
    int t = upper_bound_segment(upd_offsets, T, n);
    int64_t r = upd_rows[n];
    int64_t lo = row_lo[t];
    if (r < lo || r >= row_hi[t]) continue;
    int bits = weight_bits[t];
    int D = dims[t];
    int64_t stride = bits == 8 ? int8_row_stride(D) : nbit_row_stride(D * (bits & 0xff) / 8);
    int64_t row_byte = table_byte_offsets[t] + (r - lo) * stride;
    int64_t table_end = t + 1 < T ? table_byte_offsets[t + 1] : qweights_bytes;
    if (row_byte + stride > table_end) continue;
    const float* src = values + val_offsets[t] + (n - upd_offsets[t]) * D;
    uint8_t* dst = qweights + row_byte;
    if (bits == 8) quantize_row_int8(src, D, dst, l);
    else if (bits == 4) quantize_row_nbit<4, false>(src, D, dst, stride, l);
    else if (bits == kFormatFp8) quantize_row_fp8<false>(src, D, dst, stride, l);
    else quantize_row_nbit<2, false>(src, D, dst, stride, l);
    if (t != pend_t) {
      if (pend != 0 && l == 0) atomicAdd(applied + pend_t, pend);
      pend_t = t;
      pend = 0;
    }
    ++pend;
  }
  // every thread of the block gets here (the loop has no return): the waves
  // pool what they still hold, and one lane adds it once per table
  if (l == 0) {
    s_table[wave_id()] = pend_t;
    s_count[wave_id()] = pend;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 0; i < kWaves; ++i) {
      unsigned long long c = s_count[i];
      if (c == 0) continue;
      for (int j = i + 1; j < kWaves; ++j)
        if (s_table[j] == s_table[i]) {
          c += s_count[j];
          s_count[j] = 0;
        }
      atomicAdd(applied + s_table[i], c);
    }
  }
}

at::Tensor quant_tbe_update_rows(
    at::Tensor qweights, const at::Tensor& table_byte_offsets, const at::Tensor& dims,
    const at::Tensor& weight_bits, const at::Tensor& row_lo, const at::Tensor& row_hi,
    const at::Tensor& upd_offsets, const at::Tensor& upd_rows, const at::Tensor& values,
    const at::Tensor& val_offsets) {
  TORCH_CHECK((qweights.is_cuda() || qweights.is_pinned()) &&
                  qweights.scalar_type() == at::kByte && qweights.is_contiguous(),
              "quant_tbe_update_rows: qweights must be contiguous uint8 on the device or pinned");
  int64_t T = dims.numel();
  auto is_i64 = [](const at::Tensor& t, int64_t n) {
    return t.is_cuda() && t.scalar_type() == at::kLong && t.is_contiguous() && t.numel() == n;
  };
  TORCH_CHECK(dims.is_cuda() && dims.scalar_type() == at::kInt && dims.is_contiguous(),
              "quant_tbe_update_rows: dims must be int32 [T] on the device");
  TORCH_CHECK(weight_bits.is_cuda() && weight_bits.scalar_type() == at::kInt &&
                  weight_bits.is_contiguous() && weight_bits.numel() == T,
              "quant_tbe_update_rows: weight_bits must be int32 [T] on the device");
  TORCH_CHECK(is_i64(table_byte_offsets, T) && is_i64(row_lo, T) && is_i64(row_hi, T) &&
                  is_i64(val_offsets, T) && is_i64(upd_offsets, T + 1),
              "quant_tbe_update_rows: table_byte_offsets, row_lo, row_hi, val_offsets [T] and "
              "upd_offsets [T+1] must be int64 on the device");
  int64_t N = upd_rows.numel();
  TORCH_CHECK(is_i64(upd_rows, N), "quant_tbe_update_rows: upd_rows must be int64 on the device");
  TORCH_CHECK(values.is_cuda() && values.scalar_type() == at::kFloat && values.is_contiguous(),
              "quant_tbe_update_rows: values must be contiguous fp32 on the device");
  auto applied = at::zeros({T}, upd_rows.options());
  if (N == 0 || T == 0) return applied;
  int64_t n_waves = (N + kUpdateEntriesPerWave - 1) / kUpdateEntriesPerWave;
  hipLaunchKernelGGL(quant_tbe_update_rows_kernel,
                     dim3(grid_for(n_waves * kWaveSize, kBlockThreads)),
                     dim3(kBlockThreads), 0, q_stream(), uvm_ptr<uint8_t>(qweights),
                     qweights.numel(), table_byte_offsets.data_ptr<int64_t>(),
                     dims.data_ptr<int32_t>(), weight_bits.data_ptr<int32_t>(),
                     row_lo.data_ptr<int64_t>(), row_hi.data_ptr<int64_t>(),
                     upd_offsets.data_ptr<int64_t>(), upd_rows.data_ptr<int64_t>(),
                     values.data_ptr<float>(), val_offsets.data_ptr<int64_t>(), (int)T, N,
                     reinterpret_cast<unsigned long long*>(applied.data_ptr<int64_t>()));
  return applied;
}

// ===========================================================================
// Bounds check and pruning remap of a lookup's ids, in front of the four
// forward kernels and of quant_tbe_update_rows (reference
// IntNBitTableBatchedEmbeddingBags: index_remapping + bounds check).
//
// Contract:
//  * out[n] is the physical row of indices[n], or -1 where the id is dropped:
//    an id outside [0, logical_rows[t]) of its table t, or one whose remap
//    entry is -1 (pruned). The per-id decision is quant_remap_id
//    (quant_remap.h). indices is never written.
//  * Id n belongs to segment f where seg_offsets[f * seg_stride] <= n <
//    seg_offsets[(f + 1) * seg_stride], f in [0, F), and to table
//    feat_table[f]. The pooled path hands in the KJT offsets [F*B+1] with
//    stride B, the sequence path feat_val_offsets [F+1] with stride 1, the
//    row update upd_offsets [T+1] with stride 1 and feat_table = arange(T).
//  * remap_offsets[t] is the start of table t's int32 [logical_rows[t]]
//    segment in remap, or -1 where the table has none. remap is read only at
//    an id that passed the range test.
//  * oob_counts[t] += the out-of-range ids of table t (cumulative; pruned ids
//    are ordinary traffic and are not counted).
//  * A table built for checking has an all-zero row in front of its rows, so
//    the lookups read row -1 as zeros in every format and add weight * 0.
//  * No host read: capturable in a graph.
//
// Lane mapping: one thread per id, grid-stride, so a wave reads 64
// consecutive ids (512 B) and writes 64 consecutive rows. The segment search
// reads F+1 strided words that stay in cache; the remap read is a gather.
// Traffic: N * 16 B (id in, row out) + 4 B per remapped id.
//
// Counting: atomics on one address serialise (54 us for 4096 of them in the
// update kernel above). Out-of-range ids are summed per wave where the wave's
// bad ids share a table (ids arrive sorted by feature, so they nearly always
// do), then per block in an LDS table, and one lane issues one vector
// atomicAdd per table and block. Only T > kRemapLdsTables counts with direct
// global atomics.
// ===========================================================================

constexpr int kRemapLdsTables = 1024;

__device__ __forceinline__ int upper_bound_segment_strided(const int64_t* offs, int64_t stride,
                                                           int n, int64_t x) {
  int lo = 0, hi = n;  // invariant: offs[lo*stride] <= x < offs[hi*stride]
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (offs[mid * stride] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kBlockThreads) quant_tbe_remap_indices_kernel(
    const int64_t* __restrict__ indices,      // [N]
    const int64_t* __restrict__ seg_offsets,  // [F*seg_stride + 1]
    int64_t seg_stride,
    const int32_t* __restrict__ feat_table,     // [F]
    const int64_t* __restrict__ logical_rows,   // [T]
    const int64_t* __restrict__ remap_offsets,  // [T], -1: no remap
    const int32_t* __restrict__ remap, int F, int T, int64_t N, int64_t* __restrict__ out,
    unsigned long long* __restrict__ oob_counts) {
  __shared__ unsigned int s_oob[kRemapLdsTables];
  const bool use_lds = T <= kRemapLdsTables;
  if (use_lds) {
    for (int t = threadIdx.x; t < T; t += kBlockThreads) s_oob[t] = 0u;
    __syncthreads();
  }
  int l = lane_id();
  int64_t step = static_cast<int64_t>(gridDim.x) * kBlockThreads;
  // every lane of a wave makes the same number of trips (the ballots below
  // need the whole wave): the bound is on the wave's first id
  int64_t first = static_cast<int64_t>(blockIdx.x) * kBlockThreads + (threadIdx.x - l);
  for (int64_t base = first; base < N; base += step) {
    int64_t n = base + l;
    bool bad = false;
    int t = 0;
    if (n < N) {
      int64_t idx = indices[n];
      int f = upper_bound_segment_strided(seg_offsets, seg_stride, F, n);
      t = feat_table[f];
      int64_t ro = remap_offsets[t];
      out[n] = quant_remap_id(idx, logical_rows[t], (ro >= 0 && remap) ? remap + ro : nullptr,
                              &bad);
    }
    unsigned long long bad_mask = __ballot(bad);
    if (bad_mask == 0ull) continue;
    int leader = __ffsll(bad_mask) - 1;
    int t0 = __shfl(t, leader, kWaveSize);
    if (!use_lds) {
      if (bad) atomicAdd(oob_counts + t, 1ull);
    } else if (__ballot(bad && t == t0) == bad_mask) {
      if (l == leader) atomicAdd(&s_oob[t0], static_cast<unsigned int>(__popcll(bad_mask)));
    } else if (bad) {
      atomicAdd(&s_oob[t], 1u);
    }
  }
  if (use_lds) {
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += kBlockThreads) {
      unsigned int c = s_oob[t];
      if (c != 0u) atomicAdd(oob_counts + t, static_cast<unsigned long long>(c));
    }
  }
}

at::Tensor quant_tbe_remap_indices(
    const at::Tensor& indices, const at::Tensor& seg_offsets, int64_t seg_stride,
    const at::Tensor& feat_table, const at::Tensor& logical_rows,
    const at::Tensor& remap_offsets, const at::Tensor& remap, at::Tensor oob_counts) {
  const char* op = "quant_tbe_remap_indices: ";
  auto on_dev = [](const at::Tensor& t, at::ScalarType st) {
    return t.is_cuda() && t.scalar_type() == st && t.is_contiguous();
  };
  int64_t N = indices.numel();
  int64_t F = feat_table.numel();
  int64_t T = logical_rows.numel();
  TORCH_CHECK(on_dev(indices, at::kLong) && indices.dim() == 1, op,
              "indices must be contiguous int64 [N] on the device");
  TORCH_CHECK(on_dev(feat_table, at::kInt), op, "feat_table must be int32 [F] on the device");
  TORCH_CHECK(seg_stride >= 1 && on_dev(seg_offsets, at::kLong) &&
                  seg_offsets.numel() >= F * seg_stride + 1,
              op, "seg_offsets must be int64 with at least F * seg_stride + 1 entries");
  TORCH_CHECK(on_dev(logical_rows, at::kLong) && on_dev(remap_offsets, at::kLong) &&
                  remap_offsets.numel() == T && on_dev(oob_counts, at::kLong) &&
                  oob_counts.numel() == T,
              op, "logical_rows, remap_offsets and oob_counts must be int64 [T] on the device");
  TORCH_CHECK(remap.numel() == 0 || on_dev(remap, at::kInt), op,
              "remap must be int32 on the device");
  auto out = at::empty_like(indices);
  if (N == 0) return out;
  TORCH_CHECK(F > 0 && T > 0, op, "ids without a feature or a table");
  hipLaunchKernelGGL(quant_tbe_remap_indices_kernel, dim3(grid_for(N, kBlockThreads)),
                     dim3(kBlockThreads), 0, q_stream(), indices.data_ptr<int64_t>(),
                     seg_offsets.data_ptr<int64_t>(), seg_stride, feat_table.data_ptr<int32_t>(),
                     logical_rows.data_ptr<int64_t>(), remap_offsets.data_ptr<int64_t>(),
                     remap.numel() > 0 ? remap.data_ptr<int32_t>() : nullptr, (int)F, (int)T, N,
                     out.data_ptr<int64_t>(),
                     reinterpret_cast<unsigned long long*>(oob_counts.data_ptr<int64_t>()));
  return out;
}

}  // namespace trec_amd
