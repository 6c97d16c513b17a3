// Conversions between this library's packed Linears and the checkpoint layout of the other GPTQ tools (qweight / qzeros /
// scales / g_idx; include/gptq_hip.h, "Checkpoints of other GPTQ tools").  The bit layout of qweight is the same on both
// sides; what differs is the ORDER of the code rows (original column order + g_idx there, permuted order + perm here), the
// zero points (integers bit-packed along N there, fp32 zero*scale here) and the scales (fp16 there, fp32 here).  Three
// kernels, all HBM-bound, no LDS: lanes run along N so that every load and store of packed words is a contiguous run.
#include "common.h"

namespace gptq {

// Code j (0..31) of a 32-code stream of BITS little-endian words: at bit BITS * j, across a word boundary at 3 bits
// (j = 10 and j = 21).  `j` is a compile-time constant after unrolling, so the words stay in registers.
template <int BITS>
__device__ __forceinline__ void stream_put(uint32_t (&w)[BITS], int j, uint32_t v) {
  const int bit = BITS * j, word = bit >> 5, off = bit & 31;
  w[word] |= v << off;
  if (off + BITS > 32) w[(word + 1) % BITS] |= v >> (32 - off);    // (% BITS: only keeps the index in range for the compiler)
}

template <int BITS>
__device__ __forceinline__ uint32_t stream_get(const uint32_t (&w)[BITS], int j) {
  const int bit = BITS * j, word = bit >> 5, off = bit & 31;
  uint32_t v = w[word] >> off;
  if (off + BITS > 32) v |= w[(word + 1) % BITS] << (32 - off);
  return v & ((1u << BITS) - 1);
}

// Code row j of `out` = code row row_src[j] of `in`.  Thread = (column n, 32-row output group): for each of its 32 output
// rows it loads the word (two at a 3-bit straddle) of the source row's group that holds the code -- the source row is the
// same for the whole workgroup, so row_src and the word index are wave-uniform and the load is one contiguous run along N --
// extracts the code at stream bit BITS * (r % 32) and ORs it into BITS output words kept in registers.  A source word is
// fetched once per code it holds (32 / BITS times in all); the repeats of a run of rows that moves together hit L2.
template <int BITS>
__global__ __launch_bounds__(256) void repack_rows_kernel(const int32_t* __restrict__ in,
                                                          const int32_t* __restrict__ row_src, int n_in, int n_out,
                                                          int32_t* __restrict__ out) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  const int go = blockIdx.y;                         // output group; the grid has exactly n_in / 32 of them
  if (n >= n_out) return;
  uint32_t w[BITS];
#pragma unroll
  for (int k = 0; k < BITS; ++k) w[k] = 0;
  // all 32 (3 bits: 64) loads are issued before the first is used: no load sits under a branch, a row outside the matrix
  // reads row 0 and packs code 0 (never a stray read), and the word after a 3-bit straddle is the same word again where
  // there is no straddle (the selects are wave-uniform)
  uint32_t lo[32], hi[BITS == 3 ? 32 : 1];
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int r = row_src[go * 32 + j];
    const int rc = (unsigned)r < (unsigned)n_in ? r : 0;
    const int bit = BITS * (rc & 31), word = bit >> 5, off = bit & 31;
    const long base = ((long)(rc >> 5) * BITS + word) * n_out + n;
    lo[j] = (uint32_t)in[base];
    if (BITS == 3) hi[j] = (uint32_t)in[base + (off > 29 ? n_out : 0)];
  }
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int r = row_src[go * 32 + j];
    const int off = (BITS * (r & 31)) & 31;
    uint32_t v = lo[j] >> off;
    if (BITS == 3) v |= off > 29 ? (hi[j] << 1) << (31 - off) : 0u;
    v = (unsigned)r < (unsigned)n_in ? v & ((1u << BITS) - 1) : 0u;
    stream_put<BITS>(w, j, v);
  }
#pragma unroll
  for (int k = 0; k < BITS; ++k) out[((long)go * BITS + k) * n_out + n] = (int32_t)w[k];
}

// Our grids -> the stored zero points and fp16 scales.  Thread = (group row g, block of 32 columns): it reads its 32
// scales / zeros, writes the 32 fp16 scales and the BITS words of the block's zero-point stream, so no word has two
// writers.  The tables hold G * N entries against K * N codes: three orders of magnitude below the repack's traffic.
template <int BITS>
__global__ __launch_bounds__(64) void qzeros_pack_kernel(const float* __restrict__ scales,
                                                         const float* __restrict__ zeros, int G, int N, int zero_offset,
                                                         int32_t* __restrict__ qzeros, __half* __restrict__ scales16,
                                                         int32_t* __restrict__ flags) {
  const int nb = blockIdx.x * 64 + threadIdx.x;      // 32-column block
  const int g = blockIdx.y;
  const float maxq = (float)((1 << BITS) - 1), mid = (float)(1 << (BITS - 1)), lo = (float)zero_offset;
  int f = 0;
  if (nb < N / 32) {
    const long base = (long)g * N + nb * 32;
    uint32_t w[BITS];
#pragma unroll
    for (int k = 0; k < BITS; ++k) w[k] = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const float s = scales[base + j], zs = zeros[base + j];
      const float z = rintf(zs / s);                 // IEEE division; the integer zero point of an untouched grid
      if (z * s != zs) f |= 1;                       // (also every nan)
      const bool in_range = z >= lo && z <= maxq;
      if (!in_range) f |= 2;
      const __half h = __float2half_rn(s);
      const float hs = __half2float(h);
      if (!(fabsf(hs) > 0.f && fabsf(hs) <= 65504.f)) f |= 4;       // 0, inf or nan as fp16
      if (hs != s) f |= 8;
      if (z != mid) f |= 16;
      scales16[base + j] = h;
      stream_put<BITS>(w, j, in_range ? (uint32_t)((int)z - zero_offset) : 0u);
    }
#pragma unroll
    for (int k = 0; k < BITS; ++k) qzeros[(long)g * (N / 32 * BITS) + nb * BITS + k] = (int32_t)w[k];
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) f |= __shfl_xor(f, d);            // one atomic per wave that has something to say
  if (threadIdx.x == 0 && f) atomicOr(flags, f);
}

// The inverse: scales = (float)scales16, zeros = (float)(v + zero_offset) * scales (one fp32 rounding).
template <int BITS>
__global__ __launch_bounds__(64) void qzeros_unpack_kernel(const int32_t* __restrict__ qzeros,
                                                           const __half* __restrict__ scales16, int G, int N,
                                                           int zero_offset, float* __restrict__ scales,
                                                           float* __restrict__ zeros) {
  const int nb = blockIdx.x * 64 + threadIdx.x;
  const int g = blockIdx.y;
  if (nb >= N / 32) return;
  uint32_t w[BITS];
#pragma unroll
  for (int k = 0; k < BITS; ++k) w[k] = (uint32_t)qzeros[(long)g * (N / 32 * BITS) + nb * BITS + k];
  const long base = (long)g * N + nb * 32;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const float s = __half2float(scales16[base + j]);
    scales[base + j] = s;
    zeros[base + j] = (float)((int)stream_get<BITS>(w, j) + zero_offset) * s;
  }
}

#define GPTQ_INTEROP_BITS(bits, GO)                                                                                 \
  do {                                                                                                              \
    if ((bits) == 2) GO(2);                                                                                         \
    else if ((bits) == 3) GO(3);                                                                                    \
    else if ((bits) == 8) GO(8);                                                                                    \
    else GO(4);                                                                                                     \
  } while (0)

}  // namespace gptq

using namespace gptq;

static int check_qzeros_shape(const char* who, int G, int N, int bits, int zero_offset) {
  GPTQ_CHECK_ARG(bits == 2 || bits == 3 || bits == 4 || bits == 8, "%s: bits must be 2, 3, 4 or 8", who);
  GPTQ_CHECK_ARG(G > 0 && N > 0 && G <= 65535, "%s: bad sizes", who);
  GPTQ_CHECK_ARG(N % 32 == 0, "%s: N must be a multiple of 32", who);
  GPTQ_CHECK_ARG(zero_offset == 0 || zero_offset == 1, "%s: zero_offset must be 0 (gptq_v2) or 1 (gptq)", who);
  return GPTQ_OK;
}

extern "C" int gptq_repack_rows(const int32_t* qweight_in, const int32_t* row_src, int in_features, int out_features,
                                int bits, int32_t* qweight_out, gptq_stream_t stream) {
  GPTQ_CHECK_ARG(qweight_in && row_src && qweight_out, "gptq_repack_rows: null pointer");
  GPTQ_CHECK_ARG(bits == 2 || bits == 3 || bits == 4 || bits == 8, "gptq_repack_rows: bits must be 2, 3, 4 or 8");
  GPTQ_CHECK_ARG(out_features > 0 && in_features > 0, "gptq_repack_rows: bad sizes");
  GPTQ_CHECK_ARG(in_features % 32 == 0, "gptq_repack_rows: in_features must be a multiple of 32");
  GPTQ_CHECK_ARG(in_features / 32 <= 65535, "gptq_repack_rows: in_features too large");
  const uintptr_t a = reinterpret_cast<uintptr_t>(qweight_in), b = reinterpret_cast<uintptr_t>(qweight_out);
  const uintptr_t bytes = (uintptr_t)(in_features / 32) * bits * out_features * sizeof(int32_t);
  GPTQ_CHECK_ARG(a + bytes <= b || b + bytes <= a, "gptq_repack_rows: qweight_out must not overlap qweight_in");
  const dim3 grid(cdiv(out_features, 256), in_features / 32);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define RR(B) repack_rows_kernel<B><<<grid, 256, 0, s>>>(qweight_in, row_src, in_features, out_features, qweight_out)
  GPTQ_INTEROP_BITS(bits, RR);
#undef RR
  GPTQ_CHECK_LAUNCH("repack_rows_kernel");
  return GPTQ_OK;
}

extern "C" int gptq_qzeros_pack(const float* scales, const float* zeros, int G, int N, int bits, int zero_offset,
                                int32_t* qzeros, void* scales16, int32_t* flags, gptq_stream_t stream) {
  GPTQ_CHECK_ARG(scales && zeros && qzeros && scales16 && flags, "gptq_qzeros_pack: null pointer");
  if (int rc = check_qzeros_shape("gptq_qzeros_pack", G, N, bits, zero_offset)) return rc;
  const dim3 grid(cdiv(N / 32, 64), G);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define ZP(B) qzeros_pack_kernel<B><<<grid, 64, 0, s>>>(scales, zeros, G, N, zero_offset, qzeros, static_cast<__half*>(scales16), flags)
  GPTQ_INTEROP_BITS(bits, ZP);
#undef ZP
  GPTQ_CHECK_LAUNCH("qzeros_pack_kernel");
  return GPTQ_OK;
}

extern "C" int gptq_qzeros_unpack(const int32_t* qzeros, const void* scales16, int G, int N, int bits, int zero_offset,
                                  float* scales, float* zeros, gptq_stream_t stream) {
  GPTQ_CHECK_ARG(qzeros && scales16 && scales && zeros, "gptq_qzeros_unpack: null pointer");
  if (int rc = check_qzeros_shape("gptq_qzeros_unpack", G, N, bits, zero_offset)) return rc;
  const dim3 grid(cdiv(N / 32, 64), G);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define ZU(B) qzeros_unpack_kernel<B><<<grid, 64, 0, s>>>(qzeros, static_cast<const __half*>(scales16), G, N, zero_offset, scales, zeros)
  GPTQ_INTEROP_BITS(bits, ZU);
#undef ZU
  GPTQ_CHECK_LAUNCH("qzeros_unpack_kernel");
  return GPTQ_OK;
}
