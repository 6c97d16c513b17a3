// Packed dequant GEMM on int8 activations ("W4A8" and its 2/3/8-bit siblings): the opt-in prefill path of the packed Linears.
//
// Arithmetic contract (include/gptq_hip.h, DESIGN.md "Dequant GEMM on int8 activations"):
//   activation quantization, one grid per token row m of x [M, K] (fp16 / bf16, widened to fp32 exactly):
//       a = max_k |x[m][k]|,  sx[m] = a / 127.0f (IEEE division; 1.0f when a == 0),
//       xq[m][k] = (int8) clamp(rintf(x[m][c(k)] / sx[m]), -127, 127),   c(k) = perm ? perm[k] : k;
//   GEMM, for each output (m, n) and each group g of K (per-row grids: one group = all of K):
//       I_g = sum_{k in g} q[k][n] * xq[m][k],   X_g = sum_{k in g} xq[m][k]          (int32, exact in any order)
//       y[m][n] = sx[m] * sum_g (s[g][n] * float(I_g) - z[g][n] * float(X_g)) + bias[n]
//   everything after the integers is fp32 (separate multiplies, subtract and adds: the file is built without FMA
//   contraction), the groups are added in ascending g, and the result is rounded once to the output type.  The K split
//   cuts only BETWEEN groups (fp32 partials, added in chunk order by a second kernel) or, for per-row grids, writes the
//   int32 partial I and X of every chunk, which the second kernel adds exactly before the one fp32 evaluation.  No
//   atomics: the same call gives the same bits.  |I_g| <= 255 * 127 * K stays below 2^31 up to K = 65536; larger K is
//   refused before any launch.
//
// Tiling (v_mfma_i32_16x16x64_i8): a lane (h = lane >> 4, c = lane & 15) feeds 16 bytes of A (row c) and 16 bytes of B
// (column c); byte j of lane group h is the same k slot in A and in B, and D has column c, rows 4h + r in its 4 registers
// (the C/D map of every 16x16 MFMA).  Integer sums do not depend on the order of k, so the kernel only has to put the SAME
// k into byte (h, j) of A and of B:
//   * the 16 bytes of lane group h are the k range [16h, 16h + 16) of the 64-k step;
//   * B comes straight from the packed words with no conversion: 4-bit = two words, `w & 0x0f0f0f0f` (k 0,2,4,6 of the
//     word) and `(w >> 4) & 0x0f0f0f0f` (k 1,3,5,7); 2-bit = one word, four shifts under 0x03030303 (register a, byte b =
//     code 4b + a); 8-bit = four words, `w ^ 0x80808080` (q - 128 as a signed byte; 128 * X_g is added back as an exact
//     integer); 3-bit = 48 bits of the 96-bit group stream, four 12-bit fields spread to bytes (natural k order);
//   * the A bytes are permuted to the same order ONCE, while the xq tile is staged into LDS (v_perm_b32);
//   * X_g comes from the same A fragments through one more MFMA against a B of all ones (every column of that D holds
//     the row sums, in the accumulator's own row layout);
//   * a wave owns MSUB x 4 output tiles of 16 x 16 and a lane the 4 ADJACENT columns 4c + t, so the packed words of a
//     step arrive as 16-byte loads (the layout of qgemm.hip); a workgroup is 4 waves, WM along M and 4 / WM along N;
//   * the xq tile (BM rows x 256 k) goes through LDS; tile t + 1 and its packed words are in flight while t is computed;
//   * a group that ends in the middle of a 64-k step (groupsize an odd multiple of 32) runs the step as two half steps:
//     the same B, the A bytes of the other half zeroed.  The K % 64 == 32 tail is a step whose upper A half is zero.
#include <algorithm>

#include "common.h"

namespace gptq {

typedef int a8_i4 __attribute__((ext_vector_type(4)));

constexpr int A8_KT = 256;             // k per staged xq tile (4 MFMA steps of 64)
constexpr int A8_LDX = A8_KT + 16;     // LDS row pitch in bytes (+16: rows do not start on one bank)
constexpr int A8_TARGET_WG = 512;      // split-K aims at two workgroups per CU
constexpr int A8_MAX_K = 65536;        // 255 * 127 * K < 2^31
constexpr int A8_QC = 2;               // act_quant: 16-element chunks a thread keeps in registers (K <= 8192: one pass)

// ------------------------------------------------------------------------------------------------ act_quant
template <typename XT> __device__ __forceinline__ float a8_to_f32(uint32_t h);
template <> __device__ __forceinline__ float a8_to_f32<__half>(uint32_t h) {
  return __half2float(__ushort_as_half((unsigned short)h));
}
template <> __device__ __forceinline__ float a8_to_f32<__hip_bfloat16>(uint32_t h) { return __uint_as_float(h << 16); }

// 16 consecutive storage positions k .. k + 15 of one row as 8 words of two 16-bit patterns each
template <bool PERM>
__device__ __forceinline__ void a8_load16(uint32_t (&e)[8], const uint16_t* __restrict__ xr, int k, int K,
                                          const int32_t* __restrict__ perm, bool xvec) {
  if (PERM) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int4 p = *reinterpret_cast<const int4*>(perm + k + 4 * j);
      const int pk[4] = {p.x, p.y, p.z, p.w};
      uint32_t v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (unsigned)pk[i] < (unsigned)K ? xr[pk[i]] : 0u;   // never a stray read
      e[2 * j] = v[0] | (v[1] << 16);
      e[2 * j + 1] = v[2] | (v[3] << 16);
    }
  } else if (xvec) {
    const uint4 a = *reinterpret_cast<const uint4*>(xr + k), b = *reinterpret_cast<const uint4*>(xr + k + 8);
    e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w; e[4] = b.x; e[5] = b.y; e[6] = b.z; e[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = xr[k + 2 * j] | ((uint32_t)xr[k + 2 * j + 1] << 16);
  }
}

template <typename XT> __device__ __forceinline__ float a8_absmax16(const uint32_t (&e)[8]) {
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    a = fmaxf(a, fmaxf(fabsf(a8_to_f32<XT>(e[j] & 0xffffu)), fabsf(a8_to_f32<XT>(e[j] >> 16))));
  return a;
}

template <typename XT>
__device__ __forceinline__ void a8_quant_store16(const uint32_t (&e)[8], float s, int8_t* __restrict__ q, bool qvec) {
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t pair = e[2 * j + (i >> 1)];
      const float v = a8_to_f32<XT>((i & 1) ? pair >> 16 : pair & 0xffffu) / s;       // true division, then half-even
      const int c = (int)fminf(fmaxf(rintf(v), -127.f), 127.f);
      o |= ((uint32_t)c & 0xffu) << (8 * i);
    }
    w[j] = o;
  }
  if (qvec) {
    *reinterpret_cast<uint4*>(q) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) q[j] = (int8_t)(w[j >> 2] >> (8 * (j & 3)));
  }
}

// One workgroup per token row: row maximum (registers, wave shuffles, LDS), then quantize and store.  Rows of up to
// 256 * 16 * A8_QC elements are read once; longer rows are read a second time.
template <typename XT, bool PERM>
__global__ __launch_bounds__(256) void act_quant_kernel(const uint16_t* __restrict__ x, int ldx, int M, int K,
                                                        const int32_t* __restrict__ perm, int8_t* __restrict__ xq, int ldq,
                                                        float* __restrict__ sx, bool xvec, bool qvec) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int nch = K / 16;
  for (int row = blockIdx.x; row < M; row += gridDim.x) {
    const uint16_t* xr = x + (size_t)row * ldx;
    int8_t* qr = xq + (size_t)row * ldq;
    uint32_t cache[A8_QC][8];
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < A8_QC; ++i) {
      const int c = tid + 256 * i;
      if (c < nch) {
        a8_load16<PERM>(cache[i], xr, 16 * c, K, perm, xvec);
        a = fmaxf(a, a8_absmax16<XT>(cache[i]));
      }
    }
    for (int c = tid + 256 * A8_QC; c < nch; c += 256) {
      uint32_t e[8];
      a8_load16<PERM>(e, xr, 16 * c, K, perm, xvec);
      a = fmaxf(a, a8_absmax16<XT>(e));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a = fmaxf(a, __shfl_xor(a, o));
    if ((tid & 63) == 0) red[tid >> 6] = a;
    __syncthreads();
    a = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float s = a == 0.f ? 1.0f : a / 127.0f;
    if (tid == 0) sx[row] = s;
#pragma unroll
    for (int i = 0; i < A8_QC; ++i) {
      const int c = tid + 256 * i;
      if (c < nch) a8_quant_store16<XT>(cache[i], s, qr + 16 * c, qvec);
    }
    for (int c = tid + 256 * A8_QC; c < nch; c += 256) {
      uint32_t e[8];
      a8_load16<PERM>(e, xr, 16 * c, K, perm, xvec);
      a8_quant_store16<XT>(e, s, qr + 16 * c, qvec);
    }
    __syncthreads();                                       // `red` is reused by the next row
  }
}

// ------------------------------------------------------------------------------------------------ GEMM
// The packed words of one 64-k step for the lane's 4 columns: the word rows that hold the lane group's 16 codes.  Rows at
// or past `rows` (the K % 64 == 32 tail) and columns at or past N read as 0.
template <int BITS> constexpr int a8_nwords() { return BITS == 2 ? 1 : BITS == 8 ? 4 : 2; }

template <int BITS>
__device__ __forceinline__ void a8_load_words(uint32_t (&out)[a8_nwords<BITS>()][4], const int32_t* __restrict__ qw, int kb, int col, int N,
                                              int rows, bool wvec, int h) {
  constexpr int NW = a8_nwords<BITS>();
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    // a step is 2 * BITS word rows.  4-bit: words 2h, 2h + 1; 2-bit: word h; 8-bit: words 4h .. 4h + 3; 3-bit: the 48-bit
    // half (h & 1) of the 96-bit stream of 32-group (h >> 1): its words (h & 1) and (h & 1) + 1
    const int r = kb * (2 * BITS) + (BITS == 4 ? 2 * h + i : BITS == 2 ? h : BITS == 8 ? 4 * h + i
                                                                                      : 3 * (h >> 1) + (h & 1) + i);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < rows) {
      const int32_t* p = qw + (size_t)r * N + col;
      if (wvec && col + 3 < N) {
        v = *reinterpret_cast<const uint4*>(p);
      } else {
        v.x = col + 0 < N ? (uint32_t)p[0] : 0u;
        v.y = col + 1 < N ? (uint32_t)p[1] : 0u;
        v.z = col + 2 < N ? (uint32_t)p[2] : 0u;
        v.w = col + 3 < N ? (uint32_t)p[3] : 0u;
      }
    }
    out[i][0] = v.x; out[i][1] = v.y; out[i][2] = v.z; out[i][3] = v.w;
  }
}

// four 3-bit codes (12 bits) -> four bytes
__device__ __forceinline__ uint32_t a8_spread3(uint32_t t) {
  const uint32_t u = (t | (t << 10)) & 0x003f003fu;
  return (u | (u << 5)) & 0x07070707u;
}

// the lane's B fragment of column tile t: 16 codes of one column as bytes, in the k order the A staging mirrors
template <int BITS> __device__ __forceinline__ a8_i4 a8_fragment(const uint32_t (&w)[a8_nwords<BITS>()][4], int t, int h) {
  uint32_t v[a8_nwords<BITS>()];
#pragma unroll
  for (int i = 0; i < a8_nwords<BITS>(); ++i) v[i] = w[i][t];
  uint32_t f[4];
  if constexpr (BITS == 4) {
    f[0] = v[0] & 0x0f0f0f0fu;
    f[1] = (v[0] >> 4) & 0x0f0f0f0fu;
    f[2] = v[1] & 0x0f0f0f0fu;
    f[3] = (v[1] >> 4) & 0x0f0f0f0fu;
  } else if constexpr (BITS == 2) {
#pragma unroll
    for (int a = 0; a < 4; ++a) f[a] = (v[0] >> (2 * a)) & 0x03030303u;
  } else if constexpr (BITS == 8) {
#pragma unroll
    for (int a = 0; a < 4; ++a) f[a] = v[a] ^ 0x80808080u;
  } else {
    // the 48 bits: low 32 = (v1:v0) >> 16 (h & 1), high 16 in the low half of `hi`
    const uint32_t sh = 16 * (h & 1);
    const uint32_t lo = __builtin_amdgcn_alignbit(v[1], v[0], sh);
    const uint32_t hi = (v[1] >> sh) & 0xffffu;
    f[0] = a8_spread3(lo & 0xfffu);
    f[1] = a8_spread3((lo >> 12) & 0xfffu);
    f[2] = a8_spread3(__builtin_amdgcn_alignbit(hi, lo, 24) & 0xfffu);
    f[3] = a8_spread3((hi >> 4) & 0xfffu);
  }
  return a8_i4{(int)f[0], (int)f[1], (int)f[2], (int)f[3]};
}

// 16 xq bytes of one lane group (k 0..15 in d.x .. d.w) in the byte order of the B fragment
template <int BITS> __device__ __forceinline__ uint4 a8_permute_a(uint4 d) {
  if constexpr (BITS == 4) {                                // per 8 k: 0,2,4,6 | 1,3,5,7
    return make_uint4(__builtin_amdgcn_perm(d.y, d.x, 0x06040200u), __builtin_amdgcn_perm(d.y, d.x, 0x07050301u),
                      __builtin_amdgcn_perm(d.w, d.z, 0x06040200u), __builtin_amdgcn_perm(d.w, d.z, 0x07050301u));
  } else if constexpr (BITS == 2) {                         // register a, byte b = k 4b + a: a 4 x 4 byte transpose
    const uint32_t p = __builtin_amdgcn_perm(d.y, d.x, 0x05010400u), q = __builtin_amdgcn_perm(d.y, d.x, 0x07030602u);
    const uint32_t r = __builtin_amdgcn_perm(d.w, d.z, 0x05010400u), s = __builtin_amdgcn_perm(d.w, d.z, 0x07030602u);
    return make_uint4(__builtin_amdgcn_perm(r, p, 0x05040100u), __builtin_amdgcn_perm(r, p, 0x07060302u),
                      __builtin_amdgcn_perm(s, q, 0x05040100u), __builtin_amdgcn_perm(s, q, 0x07060302u));
  } else {
    return d;
  }
}

__device__ __forceinline__ void a8_store_y(void* __restrict__ y, int y_dtype, size_t i, float v) {
  if (y_dtype == GPTQ_F32) static_cast<float*>(y)[i] = v;
  else if (y_dtype == GPTQ_F16) static_cast<__half*>(y)[i] = __float2half(v);
  else static_cast<__hip_bfloat16*>(y)[i] = __float2bfloat16(v);
}

// Grid: (column tiles, row tiles, K chunks).  Block: 256 threads.  `gs`: the group size in k (per-row grids: K, one
// table row).  `part`: fp32 partial sums [chunk][M][N] (grouped grids, chunks end on group ends); `ipart` / `xpart`: the
// int32 partial I [chunk][M][N] and X [chunk][M] of per-row grids; neither: write Y.
template <int BITS, int MSUB, int WM>
__global__ __launch_bounds__(256) void qgemm_a8_kernel(const int8_t* __restrict__ xq, int ldq, const float* __restrict__ rs,
                                                       int M, const int32_t* __restrict__ qw,
                                                       const float* __restrict__ scales, const float* __restrict__ zeros,
                                                       const float* __restrict__ bias, int K, int N, int gs,
                                                       int chunk_blocks, void* __restrict__ y, int y_dtype, int ldy,
                                                       float* __restrict__ part, int32_t* __restrict__ ipart,
                                                       int32_t* __restrict__ xpart, bool xvec, bool wvec) {
  constexpr int WN = 4 / WM;
  constexpr int BM = WM * MSUB * 16, BN = WN * 64;
  constexpr int XCH = BM * (A8_KT / 16) / 256;             // 16-byte xq chunks per thread and tile (BM / 16)
  static_assert(XCH >= 1, "tile too small");
  __shared__ __attribute__((aligned(16))) uint8_t xs[BM * A8_LDX];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % WM, wn = wave / WM;
  const int h = lane >> 4, c16 = lane & 15;
  const int m0 = blockIdx.y * BM;
  const int col = blockIdx.x * BN + wn * 64 + 4 * c16;     // the lane's 4 columns: col .. col + 3
  const int nblocks = (K + 63) / 64;
  const int wrows = K / 32 * BITS;
  const int kbeg = blockIdx.z * chunk_blocks;
  const int kend = min(nblocks, kbeg + chunk_blocks);
  const int ntiles = (kend - kbeg + 3) / 4;
  const bool intpart = ipart != nullptr;

  // ---- xq staging: thread t takes 16-byte chunk t + 256 i of the tile (row (t >> 4) + 16 i, k 16 (t & 15)) ----
  uint4 xr[XCH];
  auto load_x = [&](int tile) {
    const int k = (kbeg + 4 * tile) * 64 + 16 * (tid & 15);
    const bool kin = k < min(K, kend * 64);                  // (K % 16 == 0: a chunk is inside or outside as a whole)
#pragma unroll
    for (int i = 0; i < XCH; ++i) {
      const int row = m0 + (tid >> 4) + 16 * i;
      xr[i] = make_uint4(0, 0, 0, 0);
      if (kin && row < M) {
        const int8_t* p = xq + (size_t)row * ldq + k;
        if (xvec) {
          xr[i] = *reinterpret_cast<const uint4*>(p);
        } else {
          const uint8_t* q = reinterpret_cast<const uint8_t*>(p);
          uint32_t w[4];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            w[j] = q[4 * j] | ((uint32_t)q[4 * j + 1] << 8) | ((uint32_t)q[4 * j + 2] << 16) | ((uint32_t)q[4 * j + 3] << 24);
          xr[i] = make_uint4(w[0], w[1], w[2], w[3]);
        }
      }
    }
  };
  auto store_x = [&]() {
#pragma unroll
    for (int i = 0; i < XCH; ++i) {
      const int r = (tid >> 4) + 16 * i;
      *reinterpret_cast<uint4*>(&xs[r * A8_LDX + 16 * (tid & 15)]) = a8_permute_a<BITS>(xr[i]);
    }
  };

  // ---- packed words: one tile (4 steps) ahead ----
  constexpr int NW = a8_nwords<BITS>();
  uint32_t wcur[4][NW][4], wnxt[4][NW][4];                 // (plain words: nothing vector-typed, so they stay in registers)
  auto load_w = [&](int tile, uint32_t (&w)[4][NW][4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int kb = kbeg + 4 * tile + s;
      if (kb < kend) a8_load_words<BITS>(w[s], qw, kb, col, N, wrows, wvec, h);
    }
  };

  a8_i4 acc[MSUB][4], xacc[MSUB];                          // open group: I (q - 128 at 8 bits) and X, the lane's 4 rows
  float tot[MSUB][4][4];                                   // closed groups
#pragma unroll
  for (int i = 0; i < MSUB; ++i) {
    xacc[i] = a8_i4{0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc[i][t] = a8_i4{0, 0, 0, 0};
#pragma unroll
      for (int r = 0; r < 4; ++r) tot[i][t][r] = 0.f;
    }
  }
  const a8_i4 ones = a8_i4{0x01010101, 0x01010101, 0x01010101, 0x01010101};

  // close the open group on table row `grow`: tot += s * float(I) - z * float(X), then restart acc and xacc
  auto close = [&](int grow) {
    float s4[4], z4[4];
    const float* sp = scales + (size_t)grow * N + col;
    const float* zp = zeros + (size_t)grow * N + col;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s4[t] = col + t < N ? sp[t] : 0.f;
      z4[t] = col + t < N ? zp[t] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < MSUB; ++i) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int I = BITS == 8 ? acc[i][t][r] + 128 * xacc[i][r] : acc[i][t][r];
          tot[i][t][r] += s4[t] * (float)I - z4[t] * (float)xacc[i][r];
        }
        acc[i][t] = a8_i4{0, 0, 0, 0};
      }
      xacc[i] = a8_i4{0, 0, 0, 0};
    }
  };

  int gcur = (kbeg * 64) / gs;                             // table row of the open group and the k at which it ends
  int gend = (gcur + 1) * gs;

  load_x(0);
  load_w(0, wcur);
  for (int tile = 0; tile < ntiles; ++tile) {
    store_x();
    __syncthreads();
    if (tile + 1 < ntiles) {
      load_x(tile + 1);
      load_w(tile + 1, wnxt);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int kb = kbeg + 4 * tile + s;
      if (kb < kend) {                                     // workgroup-uniform
        a8_i4 b[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) b[t] = a8_fragment<BITS>(wcur[s], t, h);
        const int k0 = kb * 64;
        const bool split = gend == k0 + 32 && k0 + 32 < K;  // the open group ends in the middle of this step
        const int nsub = split ? 2 : 1;
        for (int u = 0; u < nsub; ++u) {
          const bool on = !split || (h >> 1) == u;          // half step u keeps the A bytes of lane groups 2u, 2u + 1
#pragma unroll
          for (int i = 0; i < MSUB; ++i) {
            const int r0 = wm * MSUB * 16 + 16 * i;
            uint4 av = *reinterpret_cast<const uint4*>(&xs[(r0 + c16) * A8_LDX + 64 * s + 16 * h]);
            if (!on) av = make_uint4(0, 0, 0, 0);
            const a8_i4 a = a8_i4{(int)av.x, (int)av.y, (int)av.z, (int)av.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[i][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[t], acc[i][t], 0, 0, 0);
            xacc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, ones, xacc[i], 0, 0, 0);
          }
          const int kdone = split && u == 0 ? k0 + 32 : min(k0 + 64, K);
          if (!intpart && (kdone == gend || (kb + 1 == kend && u == nsub - 1))) {
            close(gcur);
            ++gcur;
            gend += gs;
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < NW; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) wcur[s][i][t] = wnxt[s][i][t];
  }

  // ---- epilogue: element r of subtile (i, t) is row 16 i + 4 h + r, column col + t ----
#pragma unroll
  for (int i = 0; i < MSUB; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wm * MSUB * 16 + 16 * i + 4 * h + r;
      if (row >= M) continue;
      if (intpart && blockIdx.x == 0 && wn == 0 && c16 == 0) xpart[(size_t)blockIdx.z * M + row] = xacc[i][r];
      const float rscale = rs[row];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int c = col + t;
        if (c >= N) continue;
        if (intpart) {
          ipart[((size_t)blockIdx.z * M + row) * N + c] = BITS == 8 ? acc[i][t][r] + 128 * xacc[i][r] : acc[i][t][r];
        } else if (part) {
          part[((size_t)blockIdx.z * M + row) * N + c] = tot[i][t][r];
        } else {
          a8_store_y(y, y_dtype, (size_t)row * ldy + c, rscale * tot[i][t][r] + (bias ? bias[c] : 0.f));
        }
      }
    }
}

// Y = sx * (sum over the S fp32 chunk partials in chunk order) + bias, rounded once
__global__ __launch_bounds__(256) void qgemm_a8_reduce_kernel(const float* __restrict__ part, int S, int M, int N,
                                                              const float* __restrict__ rs, const float* __restrict__ bias,
                                                              void* __restrict__ y, int y_dtype, int ldy) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t MN = (size_t)M * N;
  if (i >= MN) return;
  const int row = (int)(i / N), c = (int)(i % N);
  float v = part[i];
  for (int s = 1; s < S; ++s) v += part[(size_t)s * MN + i];
  a8_store_y(y, y_dtype, (size_t)row * ldy + c, rs[row] * v + (bias ? bias[c] : 0.f));
}

// per-row grids: I and X are the exact int32 sums of the chunk partials; one fp32 evaluation of the contract
__global__ __launch_bounds__(256) void qgemm_a8_reduce_int_kernel(const int32_t* __restrict__ ipart,
                                                                  const int32_t* __restrict__ xpart, int S, int M, int N,
                                                                  const float* __restrict__ rs,
                                                                  const float* __restrict__ scales,
                                                                  const float* __restrict__ zeros,
                                                                  const float* __restrict__ bias, void* __restrict__ y,
                                                                  int y_dtype, int ldy) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t MN = (size_t)M * N;
  if (i >= MN) return;
  const int row = (int)(i / N), c = (int)(i % N);
  int I = 0, X = 0;
  for (int s = 0; s < S; ++s) {
    I += ipart[(size_t)s * MN + i];
    X += xpart[(size_t)s * M + row];
  }
  const float v = scales[c] * (float)I - zeros[c] * (float)X;
  a8_store_y(y, y_dtype, (size_t)row * ldy + c, rs[row] * v + (bias ? bias[c] : 0.f));
}

// Tile configuration and K split: a pure function of the shape, so that the workspace query needs no device.
struct A8Plan { int msub, wm, bm, bn, chunk_blocks, S; bool intpart; };

static A8Plan a8_plan(int M, int K, int N, int bits, int groupsize) {
  A8Plan p;
  if (M <= 16) { p.msub = 1; p.wm = 1; }
  else if (M <= 32) { p.msub = 2; p.wm = 1; }
  else if (M <= 64) { p.msub = 4; p.wm = 1; }
  else { p.msub = 4; p.wm = 2; }
  p.bm = p.wm * p.msub * 16;
  p.bn = (4 / p.wm) * 64;
  const int blocks = cdiv(K, 64);
  // a chunk is whole groups: a multiple of lcm(64, groupsize) k.  Per-row grids split anywhere (exact int32 partials).
  const int unit = groupsize <= 0 ? 1 : groupsize % 64 == 0 ? groupsize / 64 : groupsize / 32;
  const int units = cdiv(blocks, unit);
  const long tiles = (long)cdiv(M, p.bm) * cdiv(N, p.bn);
  long S = (A8_TARGET_WG + tiles - 1) / tiles;
  S = std::min<long>(S, std::max(1, blocks / 4));                       // at least one xq tile per chunk
  // the partials' write + read must stay below the packed weights' bytes (K bits / 8 per column)
  S = std::min<long>(S, std::max<long>(1, ((long)K * bits / 8) / (8L * M)));
  S = std::max<long>(1, std::min<long>(std::min<long>(S, 64), units));
  p.chunk_blocks = cdiv(units, S) * unit;
  p.S = cdiv(blocks, p.chunk_blocks);
  p.intpart = p.S > 1 && groupsize <= 0;
  return p;
}

// fp32 partials [S][M][N], or int32 partials I [S][M][N] (rounded up to 256 bytes) + X [S][M]
static size_t a8_workspace_bytes(const A8Plan& p, int M, int N) {
  if (p.S <= 1) return 0;
  const size_t part = (size_t)p.S * M * N * 4;
  return p.intpart ? align_up(part, 256) + (size_t)p.S * M * 4 : part;
}

template <int BITS>
static void a8_launch(const A8Plan& p, const int8_t* xq, int ldq, const float* rs, int M, const int32_t* qw,
                      const float* sc, const float* zr, const float* bias, int K, int N, int gs, void* y, int y_dtype,
                      int ldy, float* part, int32_t* ipart, int32_t* xpart, bool xvec, bool wvec, hipStream_t s) {
  const dim3 grid(cdiv(N, p.bn), cdiv(M, p.bm), p.S);
#define A8_GO(MS, WMV)                                                                                                  \
  qgemm_a8_kernel<BITS, MS, WMV><<<grid, 256, 0, s>>>(xq, ldq, rs, M, qw, sc, zr, bias, K, N, gs, p.chunk_blocks, y,     \
                                                      y_dtype, ldy, part, ipart, xpart, xvec, wvec)
  if (p.wm == 2) A8_GO(4, 2);
  else if (p.msub == 4) A8_GO(4, 1);
  else if (p.msub == 2) A8_GO(2, 1);
  else A8_GO(1, 1);
#undef A8_GO
}

static bool a8_bits_ok(int bits) { return bits == 2 || bits == 3 || bits == 4 || bits == 8; }

}  // namespace gptq

using namespace gptq;

extern "C" int gptq_quant_act_rows(const void* x, int x_dtype, int ldx, int M, int K, const int32_t* perm, int8_t* xq,
                                   int ldq, float* sx, gptq_stream_t stream) {
  const char* who = "gptq_quant_act_rows";
  GPTQ_CHECK_ARG(x && xq && sx, "%s: null pointer", who);
  GPTQ_CHECK_ARG(x_dtype == GPTQ_F16 || x_dtype == GPTQ_BF16, "%s: x must be fp16 or bf16", who);
  GPTQ_CHECK_ARG(M >= 1 && K >= 32 && K % 32 == 0, "%s: need M >= 1 and K a positive multiple of 32", who);
  GPTQ_CHECK_ARG(ldx >= K && ldq >= K, "%s: ldx and ldq must be >= K", who);
  GPTQ_CHECK_ARG(!perm || reinterpret_cast<uintptr_t>(perm) % 16 == 0, "%s: perm must be 16-byte aligned", who);
  GPTQ_CHECK_ARG(reinterpret_cast<uintptr_t>(x) % 2 == 0 && reinterpret_cast<uintptr_t>(sx) % 4 == 0,
                 "%s: x / sx must be aligned to their element size", who);
  GPTQ_CHECK_ARG((size_t)M * ldx < ((size_t)1 << 62) && (size_t)M * ldq < ((size_t)1 << 62), "%s: shape too large", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool xvec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && ldx % 8 == 0;
  const bool qvec = reinterpret_cast<uintptr_t>(xq) % 16 == 0 && ldq % 16 == 0;
  const dim3 grid(std::min(M, 8192));
  const uint16_t* xp = static_cast<const uint16_t*>(x);
#define A8_Q(XT, PM) act_quant_kernel<XT, PM><<<grid, 256, 0, s>>>(xp, ldx, M, K, perm, xq, ldq, sx, xvec, qvec)
  if (x_dtype == GPTQ_F16) {
    if (perm) A8_Q(__half, true);
    else A8_Q(__half, false);
  } else {
    if (perm) A8_Q(__hip_bfloat16, true);
    else A8_Q(__hip_bfloat16, false);
  }
#undef A8_Q
  GPTQ_CHECK_LAUNCH(who);
  return GPTQ_OK;
}

extern "C" size_t gptq_quant_gemm_a8_workspace_bytes(int M, int K, int N, int bits, int groupsize) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 32 || K > A8_MAX_K || !a8_bits_ok(bits)) return 0;
  if (groupsize > 0 && (groupsize % 32 || K % groupsize)) return 0;
  return a8_workspace_bytes(a8_plan(M, K, N, bits, groupsize), M, N);
}

extern "C" int gptq_quant_gemm_a8(const int8_t* xq, int ldq, const float* sx, int M, const int32_t* qweight,
                                  const float* scales, const float* zeros, const float* bias, int K, int N, int bits,
                                  int groupsize, void* y, int y_dtype, int ldy, void* workspace, size_t workspace_bytes,
                                  gptq_stream_t stream) {
  const char* who = "gptq_quant_gemm_a8";
  GPTQ_CHECK_ARG(xq && sx && qweight && scales && zeros && y, "%s: null pointer", who);
  GPTQ_CHECK_ARG(a8_bits_ok(bits), "%s: bits must be 2, 3, 4 or 8", who);
  GPTQ_CHECK_ARG(M >= 1 && N >= 1 && K >= 32 && K % 32 == 0, "%s: need M >= 1, N >= 1 and K a positive multiple of 32", who);
  GPTQ_CHECK_ARG(K <= A8_MAX_K, "%s: K must be at most %d (the int32 sums of 255 * 127 per term)", who, A8_MAX_K);
  GPTQ_CHECK_ARG(y_dtype == GPTQ_F32 || y_dtype == GPTQ_F16 || y_dtype == GPTQ_BF16, "%s: y must be fp32, fp16 or bf16", who);
  GPTQ_CHECK_ARG(ldq >= K && ldy >= N, "%s: ldq must be >= K and ldy >= N", who);
  GPTQ_CHECK_ARG(groupsize <= 0 || (groupsize % 32 == 0 && K % groupsize == 0),
                 "%s: groupsize must be a multiple of 32 that divides K", who);
  GPTQ_CHECK_ARG((size_t)M * N * 16 < ((size_t)1 << 62) && (size_t)M * ldq < ((size_t)1 << 62), "%s: shape too large", who);
  const A8Plan p = a8_plan(M, K, N, bits, groupsize);
  GPTQ_CHECK_ARG(cdiv(M, p.bm) <= 65535, "%s: M too large", who);
  const size_t need = a8_workspace_bytes(p, M, N);
  GPTQ_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace),
                 "%s: workspace of %zu bytes needed (%s_workspace_bytes)", who, need, who);
  GPTQ_CHECK_ARG(need == 0 || reinterpret_cast<uintptr_t>(workspace) % 4 == 0, "%s: workspace must be 4-byte aligned", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* part = need && !p.intpart ? static_cast<float*>(workspace) : nullptr;
  int32_t* ipart = p.intpart ? static_cast<int32_t*>(workspace) : nullptr;
  int32_t* xpart = p.intpart ? reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + align_up((size_t)p.S * M * N * 4, 256))
                             : nullptr;
  const bool xvec = reinterpret_cast<uintptr_t>(xq) % 16 == 0 && ldq % 16 == 0;
  const bool wvec = reinterpret_cast<uintptr_t>(qweight) % 16 == 0 && N % 4 == 0;
  const int gs = groupsize > 0 ? groupsize : K;
#define A8_B(B) a8_launch<B>(p, xq, ldq, sx, M, qweight, scales, zeros, bias, K, N, gs, y, y_dtype, ldy, part, ipart, xpart, xvec, wvec, s)
  if (bits == 2) A8_B(2);
  else if (bits == 3) A8_B(3);
  else if (bits == 8) A8_B(8);
  else A8_B(4);
#undef A8_B
  GPTQ_CHECK_LAUNCH(who);
  if (need) {
    const size_t MN = (size_t)M * N;
    const dim3 grid((unsigned)((MN + 255) / 256));
    if (p.intpart)
      qgemm_a8_reduce_int_kernel<<<grid, 256, 0, s>>>(ipart, xpart, p.S, M, N, sx, scales, zeros, bias, y, y_dtype, ldy);
    else
      qgemm_a8_reduce_kernel<<<grid, 256, 0, s>>>(part, p.S, M, N, sx, bias, y, y_dtype, ldy);
    GPTQ_CHECK_LAUNCH(who);
  }
  return GPTQ_OK;
}
