// Transposed packed 2/3/4/8-bit dequant GEMM: the gradient of the packed Linears with respect to their input,
//   dx[m][c(k)] = sum_n dy[m][n] * W16[k][n],   c(k) = perm ? perm[k] : k,
//   W16[k][n]   = round_to_dy_dtype(scales[g][n] * q[k][n] - zeros[g][n]),   g = groupsize > 0 ? k / groupsize : 0.
//
// Arithmetic contract:
//   * W16 is formed with a separate fp32 multiply and a separate fp32 subtract (no contraction; zeros is the stored
//     zero*scale, as in the forward) and rounded once, to nearest even, to the type of dy (fp16 or bf16): the mat-vec's
//     formula, which a numpy float32 reference reproduces bit for bit;
//   * the MFMAs (v_mfma_f32_16x16x32_{f16,bf16}) run on dy against W16: every product is exact in fp32 and the sum over
//     n is an fp32 chain;
//   * the result is rounded once to the output type (fp32, fp16 or bf16);
//   * columns of dy and qweight at or past N contribute nothing (they are never read);
//   * deterministic: no atomics.  Where the N range is split (small M), chunk c writes its partial sums to the caller's
//     workspace [S][M][K] and a second kernel adds them in chunk order.
//
// Tiling (lane l holds A[l&15][8(l>>4)+j] and B[8(l>>4)+j][l&15], j = 0..7; the contraction index is n):
//   * the codes need no transpose.  Lane (h = l>>4, i = l&15) of a wave owns the 8 consecutive storage rows
//     k = kw + 8i + t, t = 0..7 and, per step of 32 n, the 8 columns n0 + 8h + j.  The 8 codes of one column are one
//     packed word at 4 bits, a 16-bit half of a word at 2 bits, two whole words at 8 bits and a 24-bit window of the
//     96-bit stream at 3 bits (at most two words: the forward's alignbit, along the other axis).  Code t of column j is
//     element j of the lane's B fragment of output tile t, so the 8 x 8 block a lane loaded feeds 8 tiles of 16 x 16
//     whose column i is row k = kw + 8i + t: a wave covers 128 rows of K, and only the store mapping is interleaved --
//     a lane ends up with 8 CONSECUTIVE k of each of its output rows, one 16- or 32-byte store;
//   * the A fragment is 8 consecutive n of one row of dy: one 16-byte load, straight from global memory.  Nothing goes
//     through LDS and the waves never synchronise; the 4 waves of a workgroup take 4 adjacent 128-row blocks of K and
//     read the same dy tile (the intent is that the cache serves the repeats; not profiled);
//   * a wave owns MSUB x 8 tiles: MSUB * 16 rows of dy, 128 rows of K.  The loads of step s + 1 are issued before
//     step s is decoded and multiplied (meant to overlap; how far they do is not profiled);
//   * the grid of a lane's 8 rows is one table row (groupsize is a multiple of 32, so of 8).
//   A lane's packed loads are 32-byte pieces on 16 different rows per wave: if that turns out sector-bound, staging the
//   words through LDS with coalesced loads is the next step.  tools/bench_qgemm.py --backward measures the whole call.
#include <algorithm>

#include "common.h"

namespace gptq {

typedef _Float16 qt_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 qt_b8 __attribute__((ext_vector_type(8)));
typedef float qt_f4 __attribute__((ext_vector_type(4)));

constexpr int QT_KW = 128;            // rows of K per wave
constexpr int QT_KB = 4 * QT_KW;      // rows of K per workgroup
constexpr int QT_TARGET_WG = 512;     // the N split aims at two workgroups per CU
constexpr int QT_FULL_TILES = 256;    // from this many output tiles on the N range is not split

template <typename DT> struct QtFrag;
template <> struct QtFrag<__half> {
  typedef qt_h8 type;
  typedef _Float16 elem;
  static __device__ __forceinline__ qt_f4 mfma(type a, type b, qt_f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ elem round16(float v) { return (elem)v; }
};
template <> struct QtFrag<__hip_bfloat16> {
  typedef qt_b8 type;
  typedef __bf16 elem;
  static __device__ __forceinline__ qt_f4 mfma(type a, type b, qt_f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ elem round16(float v) {
    return __builtin_bit_cast(elem, __float2bfloat16(v));    // round to nearest even
  }
};

template <int BITS> constexpr int qt_nrows() { return BITS == 3 || BITS == 8 ? 2 : 1; }

// One step of a lane: the packed words, the grid and the dy fragments of its 8 columns n0 .. n0 + 7
template <int BITS, int MSUB> struct QtStep {
  uint32_t w[qt_nrows<BITS>()][8];
  float s[8], z[8];
  uint4 a[MSUB];
};

// 8 consecutive 32-bit values p[0..7] (p 16-byte aligned when `vec`), those at or past `left` read as 0
__device__ __forceinline__ void qt_load8(uint32_t (&out)[8], const uint32_t* __restrict__ p, int left, bool vec) {
  if (vec && left >= 8) {
    const uint4 lo = *reinterpret_cast<const uint4*>(p), hi = *reinterpret_cast<const uint4*>(p + 4);
    out[0] = lo.x; out[1] = lo.y; out[2] = lo.z; out[3] = lo.w;
    out[4] = hi.x; out[5] = hi.y; out[6] = hi.z; out[7] = hi.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = j < left ? p[j] : 0u;
  }
}

// code t of the lane's 8 rows in column j.  hh: which 8-row block of its 32-row group the lane owns.
template <int BITS> __device__ __forceinline__ uint32_t qt_code(const uint32_t (&w)[qt_nrows<BITS>()][8], int j, int t, int hh) {
  if constexpr (BITS == 4) {
    return (w[0][j] >> (4 * t)) & 15u;
  } else if constexpr (BITS == 2) {
    return (w[0][j] >> (16 * (hh & 1) + 2 * t)) & 3u;
  } else if constexpr (BITS == 8) {
    return (w[t >> 2][j] >> (8 * (t & 3))) & 255u;
  } else {
    const uint32_t win = __builtin_amdgcn_alignbit(w[1][j], w[0][j], (24 * hh) & 31);
    return (win >> (3 * t)) & 7u;
  }
}

__device__ __forceinline__ void qt_store(void* y, int y_dtype, size_t idx, float v) {
  if (y_dtype == GPTQ_F32) static_cast<float*>(y)[idx] = v;
  else if (y_dtype == GPTQ_F16) static_cast<__half*>(y)[idx] = __float2half(v);
  else static_cast<__hip_bfloat16*>(y)[idx] = __float2bfloat16(v);
}

__device__ __forceinline__ uint32_t qt_pack16(int y_dtype, float lo, float hi) {
  if (y_dtype == GPTQ_F16) return (uint32_t)__half_as_ushort(__float2half(lo)) | ((uint32_t)__half_as_ushort(__float2half(hi)) << 16);
  return (uint32_t)__builtin_bit_cast(unsigned short, __float2bfloat16(lo)) |
         ((uint32_t)__builtin_bit_cast(unsigned short, __float2bfloat16(hi)) << 16);
}

// Grid: (blocks of 512 rows of K, row tiles of dy, N chunks).  Block: 256 threads.  `part` != nullptr: write the
// chunk's partial sums to part[chunk][M][K] in storage order; otherwise write dx (scattered by perm where given).
template <int BITS, typename DT, int MSUB>
__global__ __launch_bounds__(256) void qgemm_t_kernel(const DT* __restrict__ dy, int lddy, int M,
                                                      const int32_t* __restrict__ qw, const float* __restrict__ scales,
                                                      const float* __restrict__ zeros, const int32_t* __restrict__ perm,
                                                      int K, int N, int groupsize, int chunk_steps, void* __restrict__ dx,
                                                      int dx_dtype, int lddx, float* __restrict__ part, bool avec,
                                                      bool wvec, bool yvec) {
  typedef typename QtFrag<DT>::type F;
  constexpr int NR = qt_nrows<BITS>();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 4, i = lane & 15;
  const int kb = (blockIdx.x * 4 + wave) * QT_KW + 8 * i;  // the lane's 8 storage rows: kb .. kb + 7
  const bool kin = kb < K;                                 // (K % 32 == 0: all 8 or none)
  const int m0 = blockIdx.y * (MSUB * 16);
  const int nsteps = (N + 31) / 32;
  const int sbeg = blockIdx.z * chunk_steps;
  const int send = min(nsteps, sbeg + chunk_steps);
  if ((blockIdx.x * 4 + wave) * QT_KW >= K) return;        // wave-uniform; the waves never synchronise

  const int ks = kb >> 5, hh = (kb >> 3) & 3;              // 32-row group and the lane's 8-row block in it
  int wrow[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r)
    wrow[r] = BITS == 4 ? 4 * ks + hh : BITS == 2 ? 2 * ks + (hh >> 1) : BITS == 8 ? 8 * ks + 2 * hh + r
                                                                      : 3 * ks + (r == 0 ? (24 * hh) >> 5 : (24 * hh + 23) >> 5);
  const int grow = groupsize > 0 && kin ? kb / groupsize : 0;
  const uint32_t* wp[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) wp[r] = reinterpret_cast<const uint32_t*>(qw) + (size_t)wrow[r] * N;
  const uint32_t* sp = reinterpret_cast<const uint32_t*>(scales) + (size_t)grow * N;
  const uint32_t* zp = reinterpret_cast<const uint32_t*>(zeros) + (size_t)grow * N;

  auto load = [&](int step, QtStep<BITS, MSUB>& st) {
    const int n0 = step * 32 + 8 * h;
    const int left = kin ? N - n0 : 0;                     // columns at or past N, and rows past K, read as 0
    uint32_t tmp[8];
#pragma unroll
    for (int r = 0; r < NR; ++r) qt_load8(st.w[r], wp[r] + n0, left, wvec);
    qt_load8(tmp, sp + n0, left, wvec);
#pragma unroll
    for (int j = 0; j < 8; ++j) st.s[j] = __uint_as_float(tmp[j]);
    qt_load8(tmp, zp + n0, left, wvec);
#pragma unroll
    for (int j = 0; j < 8; ++j) st.z[j] = __uint_as_float(tmp[j]);
#pragma unroll
    for (int ms = 0; ms < MSUB; ++ms) {
      const int row = m0 + 16 * ms + i;
      st.a[ms] = make_uint4(0, 0, 0, 0);
      if (row < M && n0 < N) {
        const uint16_t* q = reinterpret_cast<const uint16_t*>(dy + (size_t)row * lddy + n0);
        if (avec && n0 + 8 <= N) {
          st.a[ms] = *reinterpret_cast<const uint4*>(q);
        } else {
          uint32_t e[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) e[j] = n0 + j < N ? q[j] : 0u;
          st.a[ms] = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
        }
      }
    }
  };

  qt_f4 acc[MSUB][8];
#pragma unroll
  for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[ms][t] = qt_f4{0.f, 0.f, 0.f, 0.f};

  QtStep<BITS, MSUB> cur, nxt;
  if (sbeg < send) load(sbeg, cur);
  for (int step = sbeg; step < send; ++step) {
    if (step + 1 < send) load(step + 1, nxt);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      F b;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float q = (float)qt_code<BITS>(cur.w, j, t, hh);
        b[j] = QtFrag<DT>::round16(__fsub_rn(__fmul_rn(cur.s[j], q), cur.z[j]));
      }
#pragma unroll
      for (int ms = 0; ms < MSUB; ++ms) acc[ms][t] = QtFrag<DT>::mfma(__builtin_bit_cast(F, cur.a[ms]), b, acc[ms][t]);
    }
    if (step + 1 < send) cur = nxt;
  }

  // ---- epilogue: acc[ms][t][r] is row m0 + 16 ms + 4 h + r of dy, storage row kb + t ----
  if (!kin) return;
  int pk[8];
  if (perm && !part) {
#pragma unroll
    for (int t = 0; t < 8; ++t) pk[t] = perm[kb + t];
  }
#pragma unroll
  for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + 16 * ms + 4 * h + r;
      if (row >= M) continue;
      float v[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) v[t] = acc[ms][t][r];
      if (part) {
        float* p = part + ((size_t)blockIdx.z * M + row) * K + kb;
        if (yvec) {
          *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
          *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
        } else {
#pragma unroll
          for (int t = 0; t < 8; ++t) p[t] = v[t];
        }
      } else if (perm) {
#pragma unroll
        for (int t = 0; t < 8; ++t)
          if ((unsigned)pk[t] < (unsigned)K) qt_store(dx, dx_dtype, (size_t)row * lddx + pk[t], v[t]);   // never a stray write
      } else if (yvec && dx_dtype == GPTQ_F32) {
        float* p = static_cast<float*>(dx) + (size_t)row * lddx + kb;
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
      } else if (yvec) {
        uint16_t* p = static_cast<uint16_t*>(dx) + (size_t)row * lddx + kb;
        *reinterpret_cast<uint4*>(p) = make_uint4(qt_pack16(dx_dtype, v[0], v[1]), qt_pack16(dx_dtype, v[2], v[3]),
                                                  qt_pack16(dx_dtype, v[4], v[5]), qt_pack16(dx_dtype, v[6], v[7]));
      } else {
#pragma unroll
        for (int t = 0; t < 8; ++t) qt_store(dx, dx_dtype, (size_t)row * lddx + kb + t, v[t]);
      }
    }
}

// dx[m][c(k)] = sum over the S chunk partials in chunk order, rounded once
__global__ __launch_bounds__(256) void qgemm_t_reduce_kernel(const float* __restrict__ part, int S, int M, int K,
                                                             const int32_t* __restrict__ perm, void* __restrict__ dx,
                                                             int dx_dtype, int lddx) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t MK = (size_t)M * K;
  if (idx >= MK) return;
  const int row = (int)(idx / K), k = (int)(idx % K);
  float v = part[idx];
  for (int s = 1; s < S; ++s) v += part[(size_t)s * MK + idx];
  const int c = perm ? perm[k] : k;
  if ((unsigned)c < (unsigned)K) qt_store(dx, dx_dtype, (size_t)row * lddx + c, v);
}

// Tile configuration and N split: a pure function of the shape, so that the workspace query needs no device.  For
// M <= 32 there is one row tile, so S depends on the row-tile class (M <= 16, M <= 32) and not on M, and the workspace
// grows with M inside a class.  For M > 32 the tile count grows with M, S can fall as M grows, and the workspace is
// not monotonic in M.
struct QtPlan { int msub, bm, chunk_steps, S; };

static QtPlan qt_plan(int M, int K, int N, int bits) {
  QtPlan p;
  p.msub = M <= 16 ? 1 : M <= 32 ? 2 : 4;
  p.bm = p.msub * 16;
  const int nsteps = cdiv(N, 32);
  const long tiles = (long)cdiv(K, QT_KB) * cdiv(M, p.bm);
  long S = tiles >= QT_FULL_TILES ? 1 : (QT_TARGET_WG + tiles - 1) / tiles;
  S = std::min<long>(S, std::max(1, nsteps / 2));                        // at least 2 steps of 32 n per chunk
  // the partials' write + read (8 bytes per row of the tile, chunk and k) stay below twice the packed bytes (N bits / 8 per k)
  S = std::min<long>(S, std::max<long>(1, ((long)N * bits) / (32L * p.bm)));
  S = std::max<long>(1, std::min<long>(S, 64));
  p.chunk_steps = cdiv(nsteps, S);
  p.S = cdiv(nsteps, p.chunk_steps);
  return p;
}

static size_t qt_workspace_bytes(const QtPlan& p, int M, int K) {
  return p.S > 1 ? (size_t)p.S * M * K * sizeof(float) : 0;
}

template <int BITS, typename DT>
static void qt_launch(const QtPlan& p, const void* dy, int lddy, int M, const int32_t* qw, const float* sc, const float* zr,
                      const int32_t* perm, int K, int N, int groupsize, void* dx, int dx_dtype, int lddx, float* part,
                      bool avec, bool wvec, bool yvec, hipStream_t s) {
  const dim3 grid(cdiv(K, QT_KB), cdiv(M, p.bm), p.S);
  const DT* dp = static_cast<const DT*>(dy);
#define QT_GO(MS)                                                                                                     \
  qgemm_t_kernel<BITS, DT, MS><<<grid, 256, 0, s>>>(dp, lddy, M, qw, sc, zr, perm, K, N, groupsize, p.chunk_steps, dx, \
                                                    dx_dtype, lddx, part, avec, wvec, yvec)
  if (p.msub == 4) QT_GO(4);
  else if (p.msub == 2) QT_GO(2);
  else QT_GO(1);
#undef QT_GO
}

}  // namespace gptq

using namespace gptq;

extern "C" size_t gptq_quant_gemm_t_workspace_bytes(int M, int K, int N, int bits, int groupsize) {
  (void)groupsize;
  if (M <= 0 || N <= 0 || K <= 0 || K % 32 || (bits != 2 && bits != 3 && bits != 4 && bits != 8)) return 0;
  return qt_workspace_bytes(qt_plan(M, K, N, bits), M, K);
}

extern "C" int gptq_quant_gemm_t(const void* dy, int dy_dtype, int lddy, int M, const int32_t* qweight, const float* scales,
                                 const float* zeros, const int32_t* perm, int K, int N, int bits, int groupsize, void* dx,
                                 int dx_dtype, int lddx, void* workspace, size_t workspace_bytes, gptq_stream_t stream) {
  const char* who = "gptq_quant_gemm_t";
  hipStream_t s = static_cast<hipStream_t>(stream);
  GPTQ_CHECK_ARG(dy && qweight && scales && zeros && dx, "%s: null pointer", who);
  GPTQ_CHECK_ARG(bits == 2 || bits == 3 || bits == 4 || bits == 8, "%s: bits must be 2, 3, 4 or 8", who);
  GPTQ_CHECK_ARG(M >= 1 && N >= 1 && K >= 32 && K % 32 == 0, "%s: need M >= 1, N >= 1 and K a positive multiple of 32", who);
  GPTQ_CHECK_ARG(dy_dtype == GPTQ_F16 || dy_dtype == GPTQ_BF16, "%s: dy must be fp16 or bf16", who);
  GPTQ_CHECK_ARG(dx_dtype == GPTQ_F32 || dx_dtype == GPTQ_F16 || dx_dtype == GPTQ_BF16, "%s: dx must be fp32, fp16 or bf16", who);
  GPTQ_CHECK_ARG(lddy >= N && lddx >= K, "%s: lddy must be >= N and lddx >= K", who);
  GPTQ_CHECK_ARG(groupsize <= 0 || (groupsize % 32 == 0 && K % groupsize == 0),
                 "%s: groupsize must be a multiple of 32 that divides K", who);
  GPTQ_CHECK_ARG(!perm || groupsize > 0, "%s: perm needs grouped grids (groupsize > 0)", who);
  GPTQ_CHECK_ARG((size_t)M * K * 256 < ((size_t)1 << 62) && (size_t)M * lddy < ((size_t)1 << 62) &&
                     (size_t)(K / 32 * bits) * N < ((size_t)1 << 60), "%s: shape too large", who);
  const QtPlan p = qt_plan(M, K, N, bits);
  GPTQ_CHECK_ARG(cdiv(M, p.bm) <= 65535, "%s: M too large", who);
  const size_t need = qt_workspace_bytes(p, M, K);
  GPTQ_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace),
                 "%s: workspace of %zu bytes needed (%s_workspace_bytes)", who, need, who);
  float* part = need ? static_cast<float*>(workspace) : nullptr;
  GPTQ_CHECK_ARG(!part || reinterpret_cast<uintptr_t>(part) % 4 == 0, "%s: workspace must be 4-byte aligned", who);
  const bool avec = reinterpret_cast<uintptr_t>(dy) % 16 == 0 && lddy % 8 == 0;
  const bool wvec = N % 4 == 0 && reinterpret_cast<uintptr_t>(qweight) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(scales) % 16 == 0 && reinterpret_cast<uintptr_t>(zeros) % 16 == 0;
  const bool yvec = part ? reinterpret_cast<uintptr_t>(part) % 16 == 0
                         : reinterpret_cast<uintptr_t>(dx) % 16 == 0 && lddx % 8 == 0;
  const int gs = groupsize > 0 ? groupsize : 0;
#define QT_B(B, DT) qt_launch<B, DT>(p, dy, lddy, M, qweight, scales, zeros, perm, K, N, gs, dx, dx_dtype, lddx, part, avec, wvec, yvec, s)
  if (dy_dtype == GPTQ_F16) {
    if (bits == 2) QT_B(2, __half);
    else if (bits == 3) QT_B(3, __half);
    else if (bits == 8) QT_B(8, __half);
    else QT_B(4, __half);
  } else {
    if (bits == 2) QT_B(2, __hip_bfloat16);
    else if (bits == 3) QT_B(3, __hip_bfloat16);
    else if (bits == 8) QT_B(8, __hip_bfloat16);
    else QT_B(4, __hip_bfloat16);
  }
#undef QT_B
  GPTQ_CHECK_LAUNCH(who);
  if (part) {
    const size_t MK = (size_t)M * K;
    GPTQ_CHECK_ARG((MK + 255) / 256 <= 0x7fffffffu, "%s: shape too large", who);
    qgemm_t_reduce_kernel<<<dim3((unsigned)((MK + 255) / 256)), 256, 0, s>>>(part, p.S, M, K, perm, dx, dx_dtype, lddx);
    GPTQ_CHECK_LAUNCH(who);
  }
  return GPTQ_OK;
}
