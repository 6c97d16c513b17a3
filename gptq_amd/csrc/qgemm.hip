// Packed 2/3/4/8-bit dequant GEMM  Y[M, N] = X[M, K] . Wdeq[K, N] (+ bias[N]),  Wdeq[k][n] = scale[g][n]*q[k][n] - zeros[g][n]
// (multi-token forward of the packed Linears; the single-token case stays on matvec.hip).
//
// Arithmetic contract (the mat-vec's, hoisted the same way):
//   * the MFMAs run on the exact integer codes (0..255 are exact in fp16 and bf16) against fp16/bf16 activations, so every
//     product is exact and the k-sum is an fp32 chain;
//   * the grid is applied in fp32 once per group of K (per-row grids: once per K chunk):
//       y += s[g][n] * sum_{k in g}(q x) - z[g][n] * sum_{k in g}(x),
//     the activation sums coming from the staged fp16/bf16 values in fp32;
//   * bias is added in fp32 and the result is rounded once to the output type.
//
// Tiling (v_mfma_f32_16x16x32_{f16,bf16}; lane l holds A[l&15][8(l>>4)+j] and B[8(l>>4)+j][l&15], j = 0..7):
//   * one B fragment of a lane is 8 consecutive k of one column: 4-bit = exactly one packed word, 3-bit = a 24-bit window
//     of the 96-bit group stream, at most two words (alignbit), 2-bit = one 16-bit half of a word, 8-bit = two whole
//     words;
//   * a wave owns MSUB x 4 output tiles of 16 x 16: MSUB*16 rows, 64 columns.  Its lane (l&15) holds the 4 ADJACENT
//     columns 4(l&15) + t of the four column tiles t, so the packed words of a step arrive as one 16-byte load per lane;
//   * a workgroup is 4 waves, WM along M and 4/WM along N; the X tile (BM rows x 128 k) is staged through LDS with the
//     per-(row, 32-k) sums, and each wave decodes its own packed words straight from global memory into registers;
//   * the X tile and the packed words of tile t+1 are in flight while tile t is computed;
//   * small M is bound by the packed-weight bytes, and N / 256 column tiles cannot fill 256 CUs: the K range is split into
//     S chunks; each chunk writes its partial sums to the caller's workspace [S][M][N] and a second kernel adds them in
//     chunk order (fixed order: the same call gives bit-identical Y).
//
// Act-order storage (gptq_quant_gemm_perm): packed row k multiplies x[:, perm[k]].  Y is the plain kernel's on the
// gathered X = x[:, perm], with the same plan, so it is bit-identical to gptq_quant_gemm on a copy of x[:, perm].  The
// gather happens either inside the X staging (PERM: a thread reads its 8 perm entries once per tile and gathers 8 single
// elements per row; M <= 4, where it saves the pre-pass launch) or in a pre-pass into the workspace (larger M: the fused
// form turns one 16-byte load per row and chunk into 8 scattered 2-byte loads, 64 per thread and tile at BM = 128, and
// was measured 1.3x at M = 16 and 2-4x at M >= 128; the pre-pass costs 1-8 %).
#include <algorithm>

#include "common.h"

namespace gptq {

typedef _Float16 qg_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 qg_b8 __attribute__((ext_vector_type(8)));
typedef float qg_f4 __attribute__((ext_vector_type(4)));

constexpr int QG_KT = 128;            // k per staged X tile (4 MFMA k-steps)
constexpr int QG_LDX = QG_KT + 8;     // LDS row pitch in 16-bit elements (+16 bytes: rows do not start on one bank)
constexpr int QG_TARGET_WG = 512;     // split-K aims at two workgroups per CU

template <typename XT> struct QgFrag;
template <> struct QgFrag<__half> {
  typedef qg_h8 type;
  typedef _Float16 elem;
  static __device__ __forceinline__ qg_f4 mfma(type a, type b, qg_f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ float to_f32(uint32_t h) {
    return __half2float(__ushort_as_half((unsigned short)h));
  }
};
template <> struct QgFrag<__hip_bfloat16> {
  typedef qg_b8 type;
  typedef __bf16 elem;
  static __device__ __forceinline__ qg_f4 mfma(type a, type b, qg_f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ float to_f32(uint32_t h) { return __uint_as_float(h << 16); }
};

// 8 codes of one B fragment (code j at bit BITS*j of `win`) -> 8 exact fp16 / bf16 values
template <int BITS, typename XT> __device__ __forceinline__ typename QgFrag<XT>::type qg_decode(uint32_t win) {
  typename QgFrag<XT>::type f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (typename QgFrag<XT>::elem)(float)((win >> (BITS * j)) & ((1u << BITS) - 1));
  return f;
}
// 8-bit: the fragment is two whole words, bytes 0..3 of `lo` then of `hi`
template <typename XT> __device__ __forceinline__ typename QgFrag<XT>::type qg_decode_bytes(uint32_t lo, uint32_t hi) {
  typename QgFrag<XT>::type f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] = (typename QgFrag<XT>::elem)(float)((lo >> (8 * j)) & 0xffu);
    f[4 + j] = (typename QgFrag<XT>::elem)(float)((hi >> (8 * j)) & 0xffu);
  }
  return f;
}

template <typename YT> __device__ __forceinline__ void qg_store(YT* p, float v);
template <> __device__ __forceinline__ void qg_store<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void qg_store<__half>(__half* p, float v) { *p = __float2half(v); }
template <> __device__ __forceinline__ void qg_store<__hip_bfloat16>(__hip_bfloat16* p, float v) { *p = __float2bfloat16(v); }

// The packed words of one k-step for the lane's 4 columns: w[0] (4-bit, and 2-bit: the word that holds the lane's 16-bit
// half), w[0] / w[1] = low / high word of the 24-bit window (3-bit) or of the fragment's 8 bytes (8-bit).  Columns at or
// past N read as 0 (their outputs are never stored).
template <int BITS> constexpr int qg_nwords() { return BITS == 3 || BITS == 8 ? 2 : 1; }
template <int BITS> struct QgWords { uint4 w[qg_nwords<BITS>()]; };

template <int BITS>
__device__ __forceinline__ void qg_load_words(QgWords<BITS>& out, const int32_t* __restrict__ qw, int ks, int col, int N,
                                              bool wvec, int h) {
  constexpr int NW = qg_nwords<BITS>();
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    // 4-bit: word h of the group; 3-bit: words (24h) / 32 and (24h + 23) / 32 of the group's three; 2-bit: word h / 2 of
    // the group's two; 8-bit: words 2h and 2h + 1 of the group's eight
    const int r = BITS == 4 ? h : BITS == 2 ? h >> 1 : BITS == 8 ? 2 * h + i
                                                                 : (i == 0 ? (24 * h) >> 5 : (24 * h + 23) >> 5);
    const int32_t* p = qw + (size_t)(ks * BITS + r) * N + col;
    if (wvec && col + 3 < N) {
      out.w[i] = *reinterpret_cast<const uint4*>(p);
    } else {
      out.w[i].x = col + 0 < N ? (uint32_t)p[0] : 0u;
      out.w[i].y = col + 1 < N ? (uint32_t)p[1] : 0u;
      out.w[i].z = col + 2 < N ? (uint32_t)p[2] : 0u;
      out.w[i].w = col + 3 < N ? (uint32_t)p[3] : 0u;
    }
  }
}

template <int BITS> __device__ __forceinline__ uint32_t qg_window(const QgWords<BITS>& w, int t, int h) {
  const uint32_t lo = t == 0 ? w.w[0].x : t == 1 ? w.w[0].y : t == 2 ? w.w[0].z : w.w[0].w;
  if (BITS == 4) return lo;
  if (BITS == 2) return lo >> (16 * (h & 1));            // (the decode masks the 8 codes out of the low 16 bits)
  const uint32_t hi = t == 0 ? w.w[BITS == 3].x : t == 1 ? w.w[BITS == 3].y : t == 2 ? w.w[BITS == 3].z : w.w[BITS == 3].w;
  return __builtin_amdgcn_alignbit(hi, lo, (24 * h) & 31);
}

// the lane's B fragment of column tile t: 8 consecutive k of one column as exact fp16 / bf16 values
template <int BITS, typename XT>
__device__ __forceinline__ typename QgFrag<XT>::type qg_fragment(const QgWords<BITS>& w, int t, int h) {
  if constexpr (BITS == 8) {
    const uint32_t lo = t == 0 ? w.w[0].x : t == 1 ? w.w[0].y : t == 2 ? w.w[0].z : w.w[0].w;
    const uint32_t hi = t == 0 ? w.w[1].x : t == 1 ? w.w[1].y : t == 2 ? w.w[1].z : w.w[1].w;
    return qg_decode_bytes<XT>(lo, hi);
  } else {
    return qg_decode<BITS, XT>(qg_window<BITS>(w, t, h));
  }
}

// Grid: (column tiles, row tiles, K chunks).  Block: 256 threads.  `part` != nullptr: write the chunk's partial sums
// to part[chunk][M][N] (no bias); otherwise write Y (+ bias).
template <int BITS, typename XT, typename YT, bool GROUPED, int MSUB, int WM, bool PERM = false>
__global__ __launch_bounds__(256) void qgemm_kernel(const XT* __restrict__ x, int ldx, int M, const int32_t* __restrict__ qw,
                                                    const float* __restrict__ scales, const float* __restrict__ zeros,
                                                    const float* __restrict__ bias, int K, int N, int groupsize,
                                                    int chunk_steps, YT* __restrict__ y, int ldy, float* __restrict__ part,
                                                    bool xvec, bool wvec, const int32_t* __restrict__ perm = nullptr) {
  typedef typename QgFrag<XT>::type F;
  constexpr int WN = 4 / WM;
  constexpr int BM = WM * MSUB * 16, BN = WN * 64;
  constexpr int XCH = BM * (QG_KT / 8) / 256;              // 16-byte X chunks per thread and tile (BM / 16)
  static_assert(XCH >= 1, "tile too small");
  __shared__ __attribute__((aligned(16))) uint16_t xs[BM * QG_LDX];
  __shared__ __attribute__((aligned(16))) float xsum[QG_KT / 32][BM];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % WM, wn = wave / WM;
  const int h = lane >> 4, c16 = lane & 15;
  const int m0 = blockIdx.y * BM;
  const int col = blockIdx.x * BN + wn * 64 + 4 * c16;     // the lane's 4 columns: col .. col + 3
  const int ksteps = K / 32;
  const int kbeg = blockIdx.z * chunk_steps;
  const int kend = min(ksteps, kbeg + chunk_steps);
  const int ntiles = (kend - kbeg + 3) / 4;

  // ---- X staging: thread t takes 16-byte chunk t + 256 i of the tile (row (t >> 4) + 16 i, k 8 (t & 15)) ----
  uint4 xr[XCH];
  auto load_x = [&](int tile) {
    const int k = (kbeg + 4 * tile) * 32 + 8 * (tid & 15);
    const bool kin = k < kend * 32;
    int pk[8];                                               // PERM: the input columns of the chunk's 8 storage rows
    if (PERM && kin) {
      const int4 a = *reinterpret_cast<const int4*>(perm + k), b = *reinterpret_cast<const int4*>(perm + k + 4);
      pk[0] = a.x; pk[1] = a.y; pk[2] = a.z; pk[3] = a.w; pk[4] = b.x; pk[5] = b.y; pk[6] = b.z; pk[7] = b.w;
    }
#pragma unroll
    for (int i = 0; i < XCH; ++i) {
      const int row = m0 + (tid >> 4) + 16 * i;
      xr[i] = make_uint4(0, 0, 0, 0);
      if (kin && row < M) {
        const XT* p = x + (size_t)row * ldx + k;
        if (PERM) {
          const uint16_t* q = reinterpret_cast<const uint16_t*>(x + (size_t)row * ldx);
          uint32_t e[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) e[j] = (unsigned)pk[j] < (unsigned)K ? q[pk[j]] : 0u;   // never a stray read
          xr[i].x = e[0] | (e[1] << 16);
          xr[i].y = e[2] | (e[3] << 16);
          xr[i].z = e[4] | (e[5] << 16);
          xr[i].w = e[6] | (e[7] << 16);
        } else if (xvec) {
          xr[i] = *reinterpret_cast<const uint4*>(p);
        } else {
          const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
          xr[i].x = q[0] | ((uint32_t)q[1] << 16);
          xr[i].y = q[2] | ((uint32_t)q[3] << 16);
          xr[i].z = q[4] | ((uint32_t)q[5] << 16);
          xr[i].w = q[6] | ((uint32_t)q[7] << 16);
        }
      }
    }
  };
  auto store_x = [&]() {
#pragma unroll
    for (int i = 0; i < XCH; ++i) {
      const int r = (tid >> 4) + 16 * i;
      *reinterpret_cast<uint4*>(&xs[r * QG_LDX + 8 * (tid & 15)]) = xr[i];
      const uint32_t v[4] = {xr[i].x, xr[i].y, xr[i].z, xr[i].w};
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) s += QgFrag<XT>::to_f32(v[j] & 0xffffu) + QgFrag<XT>::to_f32(v[j] >> 16);
      s += __shfl_xor(s, 1);                              // the 4 chunks of one 32-k segment sit on 4 adjacent lanes
      s += __shfl_xor(s, 2);
      if ((tid & 3) == 0) xsum[(tid & 15) >> 2][r] = s;
    }
  };

  // ---- packed words: one tile (4 k-steps) ahead ----
  QgWords<BITS> wcur[4], wnxt[4];
  auto load_w = [&](int tile, QgWords<BITS> (&w)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int ks = kbeg + 4 * tile + s;
      if (ks < kend) qg_load_words<BITS>(w[s], qw, ks, col, N, wvec, h);
    }
  };

  qg_f4 acc[MSUB][4], tot[MSUB][4];                        // tot: closed groups (grouped grids)
  float sx[MSUB][4];                                       // sum of x over the open group, the lane's 4 rows per subtile
#pragma unroll
  for (int i = 0; i < MSUB; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc[i][t] = qg_f4{0.f, 0.f, 0.f, 0.f};
      if (GROUPED) tot[i][t] = qg_f4{0.f, 0.f, 0.f, 0.f};
      sx[i][t] = 0.f;
    }

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
      const int ks = kbeg + 4 * tile + s;
      if (ks < kend) {                                     // workgroup-uniform
        F b[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) b[t] = qg_fragment<BITS, XT>(wcur[s], t, h);
#pragma unroll
        for (int i = 0; i < MSUB; ++i) {
          const int r0 = wm * MSUB * 16 + 16 * i;
          const F a = __builtin_bit_cast(F, *reinterpret_cast<const uint4*>(&xs[(r0 + c16) * QG_LDX + 32 * s + 8 * h]));
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[i][t] = QgFrag<XT>::mfma(a, b[t], acc[i][t]);
          const float4 xv = *reinterpret_cast<const float4*>(&xsum[s][r0 + 4 * h]);
          sx[i][0] += xv.x; sx[i][1] += xv.y; sx[i][2] += xv.z; sx[i][3] += xv.w;
        }
        if (GROUPED && (((ks + 1) * 32) % groupsize == 0 || ks + 1 == kend)) {
          // close the group: tot += s * acc - z * sx, then restart acc and sx
          const int grow = (ks * 32) / groupsize;
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
              for (int r = 0; r < 4; ++r) tot[i][t][r] += s4[t] * acc[i][t][r] - z4[t] * sx[i][r];
              acc[i][t] = qg_f4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) sx[i][r] = 0.f;
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) wcur[s] = wnxt[s];
  }

  // per-row grids: one table row, applied to the whole chunk
  qg_f4 res[MSUB][4];
#pragma unroll
  for (int i = 0; i < MSUB; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (GROUPED) {
        res[i][t] = tot[i][t];
      } else {
        const float sc = col + t < N ? scales[col + t] : 0.f, zc = col + t < N ? zeros[col + t] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) res[i][t][r] = sc * acc[i][t][r] - zc * sx[i][r];
      }
    }

  // ---- epilogue: acc element r of subtile (i, t) is row 16 i + 4 h + r, column col + t ----
#pragma unroll
  for (int i = 0; i < MSUB; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wm * MSUB * 16 + 16 * i + 4 * h + r;
      if (row >= M) continue;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int c = col + t;
        if (c >= N) continue;
        if (part) {
          part[((size_t)blockIdx.z * M + row) * N + c] = res[i][t][r];
        } else {
          qg_store<YT>(y + (size_t)row * ldy + c, res[i][t][r] + (bias ? bias[c] : 0.f));
        }
      }
    }
}

// Gather pre-pass of the act-order GEMM: xg[m][j] = x[m][perm[j]] (16-bit elements), xg row-major with K columns.
// Thread = 8 consecutive j of one row: two 16-byte loads of perm, 8 gathered elements (the row sits in L2), one 16-byte
// store.  An index outside the row gathers 0.
__global__ __launch_bounds__(256) void qgemm_gather_kernel(const uint16_t* __restrict__ x, int ldx, int M, int K,
                                                           const int32_t* __restrict__ perm, uint16_t* __restrict__ xg) {
  const int j = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (j >= K) return;
  const int4 a = *reinterpret_cast<const int4*>(perm + j), b = *reinterpret_cast<const int4*>(perm + j + 4);
  const int pk[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  for (int row = blockIdx.y; row < M; row += gridDim.y) {
    const uint16_t* q = x + (size_t)row * ldx;
    uint32_t e[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) e[t] = (unsigned)pk[t] < (unsigned)K ? q[pk[t]] : 0u;
    *reinterpret_cast<uint4*>(xg + (size_t)row * K + j) =
        make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
  }
}

// Y = sum over the S chunk partials in chunk order (+ bias), rounded once
template <typename YT>
__global__ __launch_bounds__(256) void qgemm_reduce_kernel(const float* __restrict__ part, int S, int M, int N,
                                                           const float* __restrict__ bias, YT* __restrict__ y, int ldy) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t MN = (size_t)M * N;
  if (i >= MN) return;
  const int row = (int)(i / N), c = (int)(i % N);
  float v = part[i];
  for (int s = 1; s < S; ++s) v += part[(size_t)s * MN + i];
  qg_store<YT>(y + (size_t)row * ldy + c, v + (bias ? bias[c] : 0.f));
}

// Tile configuration and K split: a pure function of the shape, so that the workspace query needs no device.
struct QgPlan { int msub, wm, bm, bn, chunk_steps, S; };

static QgPlan qg_plan(int M, int K, int N, int bits) {
  QgPlan p;
  if (M <= 16) { p.msub = 1; p.wm = 1; }
  else if (M <= 32) { p.msub = 2; p.wm = 1; }
  else if (M <= 64) { p.msub = 4; p.wm = 1; }
  else { p.msub = 4; p.wm = 2; }
  p.bm = p.wm * p.msub * 16;
  p.bn = (4 / p.wm) * 64;
  const int ksteps = K / 32;
  const long tiles = (long)cdiv(M, p.bm) * cdiv(N, p.bn);
  long S = (QG_TARGET_WG + tiles - 1) / tiles;
  S = std::min<long>(S, std::max(1, ksteps / 8));                       // at least 8 k-steps (2 X tiles) per chunk
  // the partials' write + read must stay below the packed weights' bytes (K bits / 8 per column)
  S = std::min<long>(S, std::max<long>(1, ((long)K * bits / 8) / (8L * M)));
  S = std::max<long>(1, std::min<long>(S, 64));
  p.chunk_steps = cdiv(ksteps, S);
  p.S = cdiv(ksteps, p.chunk_steps);
  return p;
}

static size_t qg_workspace_bytes(const QgPlan& p, int M, int N) {
  return p.S > 1 ? (size_t)p.S * M * N * sizeof(float) : 0;
}

// Act-order GEMM: up to this M the gather is fused into the X staging, above it a pre-pass gathers X into the workspace
// ("act-order GEMM": measured on the Llama-7B Linears).
static int qg_perm_fused_max_m() {
  static const int m = tune_knob("GPTQ_QG_PERM_FUSED_M", 4);
  return m;
}
static bool qg_perm_prepass(int M) { return M > qg_perm_fused_max_m(); }
// bytes of the partials (rounded up to 256) + the gathered X of the pre-pass
static size_t qg_perm_workspace_bytes(const QgPlan& p, int M, int K, int N) {
  const size_t part = qg_workspace_bytes(p, M, N);
  return qg_perm_prepass(M) ? align_up(part, 256) + (size_t)M * K * sizeof(uint16_t) : part;
}

template <int BITS, typename XT, typename YT, bool GROUPED>
static void qg_launch_cfg(const QgPlan& p, const void* x, int ldx, int M, const int32_t* qw, const float* sc,
                          const float* zr, const float* bias, int K, int N, int groupsize, void* y, int ldy, float* part,
                          bool xvec, bool wvec, hipStream_t s, const int32_t* perm) {
  const dim3 grid(cdiv(N, p.bn), cdiv(M, p.bm), p.S);
  const XT* xp = static_cast<const XT*>(x);
  YT* yp = static_cast<YT*>(y);
#define QG_GO(MS, WMV, PM)                                                                                          \
  qgemm_kernel<BITS, XT, YT, GROUPED, MS, WMV, PM><<<grid, 256, 0, s>>>(xp, ldx, M, qw, sc, zr, bias, K, N,         \
                                                                       groupsize, p.chunk_steps, yp, ldy, part, xvec, \
                                                                       wvec, perm)
  if constexpr (GROUPED) {                                 // the act-order format always has grouped grids
    if (perm) {
      if (p.wm == 2) QG_GO(4, 2, true);
      else if (p.msub == 4) QG_GO(4, 1, true);
      else if (p.msub == 2) QG_GO(2, 1, true);
      else QG_GO(1, 1, true);
      return;
    }
  }
  if (p.wm == 2) QG_GO(4, 2, false);
  else if (p.msub == 4) QG_GO(4, 1, false);
  else if (p.msub == 2) QG_GO(2, 1, false);
  else QG_GO(1, 1, false);
#undef QG_GO
}

template <int BITS, typename XT, typename YT>
static void qg_launch(const QgPlan& p, const void* x, int ldx, int M, const int32_t* qw, const float* sc,
                      const float* zr, const float* bias, int K, int N, int groupsize, void* y, int ldy, float* part,
                      bool xvec, bool wvec, hipStream_t s, const int32_t* perm) {
  if (groupsize > 0)
    qg_launch_cfg<BITS, XT, YT, true>(p, x, ldx, M, qw, sc, zr, bias, K, N, groupsize, y, ldy, part, xvec, wvec, s, perm);
  else
    qg_launch_cfg<BITS, XT, YT, false>(p, x, ldx, M, qw, sc, zr, bias, K, N, groupsize, y, ldy, part, xvec, wvec, s, perm);
}

template <int BITS, typename XT>
static void qg_launch_y(int y_dtype, const QgPlan& p, const void* x, int ldx, int M, const int32_t* qw, const float* sc,
                        const float* zr, const float* bias, int K, int N, int groupsize, void* y, int ldy, float* part,
                        bool xvec, bool wvec, hipStream_t s, const int32_t* perm) {
  if (part) y_dtype = GPTQ_F32;                          // the partials are fp32; Y is written by the reduction
  if (y_dtype == GPTQ_F32) qg_launch<BITS, XT, float>(p, x, ldx, M, qw, sc, zr, bias, K, N, groupsize, y, ldy, part, xvec, wvec, s, perm);
  else if (y_dtype == GPTQ_F16) qg_launch<BITS, XT, __half>(p, x, ldx, M, qw, sc, zr, bias, K, N, groupsize, y, ldy, part, xvec, wvec, s, perm);
  else qg_launch<BITS, XT, __hip_bfloat16>(p, x, ldx, M, qw, sc, zr, bias, K, N, groupsize, y, ldy, part, xvec, wvec, s, perm);
}

}  // namespace gptq

using namespace gptq;

extern "C" size_t gptq_quant_gemm_workspace_bytes(int M, int K, int N, int bits, int groupsize) {
  (void)groupsize;
  if (M <= 0 || N <= 0 || K <= 0 || K % 32 || (bits != 2 && bits != 3 && bits != 4 && bits != 8)) return 0;
  return qg_workspace_bytes(qg_plan(M, K, N, bits), M, N);
}

static int quant_gemm_impl(const char* who, const void* x, int x_dtype, int ldx, int M, const int32_t* qweight,
                           const float* scales, const float* zeros, const int32_t* perm, const float* bias, int K, int N,
                           int bits, int groupsize, void* y, int y_dtype, int ldy, void* workspace,
                           size_t workspace_bytes, hipStream_t s) {
  GPTQ_CHECK_ARG(x && qweight && scales && zeros && y, "%s: null pointer", who);
  GPTQ_CHECK_ARG(bits == 2 || bits == 3 || bits == 4 || bits == 8, "%s: bits must be 2, 3, 4 or 8", who);
  GPTQ_CHECK_ARG(M >= 1 && N >= 1 && K >= 32 && K % 32 == 0, "%s: need M >= 1, N >= 1 and K a positive multiple of 32", who);
  GPTQ_CHECK_ARG(x_dtype == GPTQ_F16 || x_dtype == GPTQ_BF16, "%s: x must be fp16 or bf16", who);
  GPTQ_CHECK_ARG(y_dtype == GPTQ_F32 || y_dtype == GPTQ_F16 || y_dtype == GPTQ_BF16, "%s: y must be fp32, fp16 or bf16", who);
  GPTQ_CHECK_ARG(ldx >= K && ldy >= N, "%s: ldx must be >= K and ldy >= N", who);
  GPTQ_CHECK_ARG(groupsize <= 0 || (groupsize % 32 == 0 && K % groupsize == 0),
                 "%s: groupsize must be a multiple of 32 that divides K", who);
  GPTQ_CHECK_ARG(!perm || groupsize > 0, "%s: perm needs grouped grids (groupsize > 0)", who);
  GPTQ_CHECK_ARG(!perm || reinterpret_cast<uintptr_t>(perm) % 16 == 0, "%s: perm must be 16-byte aligned", who);
  GPTQ_CHECK_ARG((size_t)M * N * 16 < ((size_t)1 << 62) && (size_t)M * ldx < ((size_t)1 << 62), "%s: shape too large", who);
  const QgPlan p = qg_plan(M, K, N, bits);
  GPTQ_CHECK_ARG(cdiv(M, p.bm) <= 65535, "%s: M too large", who);
  const size_t need = perm ? qg_perm_workspace_bytes(p, M, K, N) : qg_workspace_bytes(p, M, N);
  GPTQ_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace),
                 "%s: workspace of %zu bytes needed (%s_workspace_bytes)", who, need, who);
  float* part = qg_workspace_bytes(p, M, N) ? static_cast<float*>(workspace) : nullptr;
  if (perm && qg_perm_prepass(M)) {                      // gather X into the workspace, then the plain kernel
    GPTQ_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    uint16_t* xg = reinterpret_cast<uint16_t*>(static_cast<char*>(workspace) + align_up(qg_workspace_bytes(p, M, N), 256));
    const dim3 gg(cdiv(K, 256 * 8), std::min(M, 65535));
    qgemm_gather_kernel<<<gg, 256, 0, s>>>(static_cast<const uint16_t*>(x), ldx, M, K, perm, xg);
    GPTQ_CHECK_LAUNCH(who);
    x = xg;
    ldx = K;
    perm = nullptr;
  }
  const bool xvec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && ldx % 8 == 0;
  const bool wvec = reinterpret_cast<uintptr_t>(qweight) % 16 == 0 && N % 4 == 0;
  const int gs = groupsize > 0 ? groupsize : 0;
#define QG_Y(B, XT) qg_launch_y<B, XT>(y_dtype, p, x, ldx, M, qweight, scales, zeros, bias, K, N, gs, y, ldy, part, xvec, wvec, s, perm)
  if (x_dtype == GPTQ_F16) {
    if (bits == 2) QG_Y(2, __half);
    else if (bits == 3) QG_Y(3, __half);
    else if (bits == 8) QG_Y(8, __half);
    else QG_Y(4, __half);
  } else {
    if (bits == 2) QG_Y(2, __hip_bfloat16);
    else if (bits == 3) QG_Y(3, __hip_bfloat16);
    else if (bits == 8) QG_Y(8, __hip_bfloat16);
    else QG_Y(4, __hip_bfloat16);
  }
#undef QG_Y
  GPTQ_CHECK_LAUNCH(who);
  if (part) {
    const size_t MN = (size_t)M * N;
    const dim3 grid((unsigned)((MN + 255) / 256));
    if (y_dtype == GPTQ_F32) qgemm_reduce_kernel<float><<<grid, 256, 0, s>>>(part, p.S, M, N, bias, static_cast<float*>(y), ldy);
    else if (y_dtype == GPTQ_F16) qgemm_reduce_kernel<__half><<<grid, 256, 0, s>>>(part, p.S, M, N, bias, static_cast<__half*>(y), ldy);
    else qgemm_reduce_kernel<__hip_bfloat16><<<grid, 256, 0, s>>>(part, p.S, M, N, bias, static_cast<__hip_bfloat16*>(y), ldy);
    GPTQ_CHECK_LAUNCH(who);
  }
  return GPTQ_OK;
}

extern "C" int gptq_quant_gemm(const void* x, int x_dtype, int ldx, int M, const int32_t* qweight, const float* scales,
                               const float* zeros, const float* bias, int K, int N, int bits, int groupsize, void* y,
                               int y_dtype, int ldy, void* workspace, size_t workspace_bytes, gptq_stream_t stream) {
  return quant_gemm_impl("gptq_quant_gemm", x, x_dtype, ldx, M, qweight, scales, zeros, nullptr, bias, K, N, bits,
                         groupsize, y, y_dtype, ldy, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

extern "C" size_t gptq_quant_gemm_perm_workspace_bytes(int M, int K, int N, int bits, int groupsize) {
  (void)groupsize;
  if (M <= 0 || N <= 0 || K <= 0 || K % 32 || (bits != 2 && bits != 3 && bits != 4 && bits != 8)) return 0;
  return qg_perm_workspace_bytes(qg_plan(M, K, N, bits), M, K, N);
}

extern "C" int gptq_quant_gemm_perm(const void* x, int x_dtype, int ldx, int M, const int32_t* qweight,
                                    const float* scales, const float* zeros, const int32_t* perm, const float* bias, int K,
                                    int N, int bits, int groupsize, void* y, int y_dtype, int ldy, void* workspace,
                                    size_t workspace_bytes, gptq_stream_t stream) {
  return quant_gemm_impl("gptq_quant_gemm_perm", x, x_dtype, ldx, M, qweight, scales, zeros, perm, bias, K, N, bits,
                         groupsize, y, y_dtype, ldy, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
