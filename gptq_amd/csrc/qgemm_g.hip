// Grid gradients of the packed Linears: the gradients of
//   y[m][n] = sum_k x[m][c(k)] * (scales[g][n]*q[k][n] - zeros[g][n]) + bias[n],   c(k) = perm ? perm[k] : k,
// with respect to the stored scales, zeros (= zero*scale) and bias, the integer codes q staying frozen:
//   A[k][n]       = sum_m x[m][c(k)] * dy[m][n]                 (the dense weight gradient: never stored)
//   dscales[g][n] =  sum_{k in g} q[k][n] * A[k][n]
//   dzeros[g][n]  = -sum_{k in g} A[k][n]
//   dbias[n]      =  sum_m dy[m][n],                            g = groupsize > 0 ? k / groupsize : 0.
//
// Arithmetic contract:
//   * the MFMAs (v_mfma_f32_16x16x32_{f16,bf16}) run on x against dy: every product is exact in fp32 and the sum over m
//     is an fp32 chain (dbias is the same chain against a fragment of ones);
//   * q * A is one fp32 multiply by the exact integer code;
//   * the sums over the k of a group are fp32 adds in a fixed order: the 4 rows a lane holds, the two 16-row blocks of a
//     32-row slab, the 4 lane groups of the wave (two butterfly steps), the slabs of a segment in ascending order, then
//     -- where a group spans several segments or the tokens are split -- the partials in ascending (segment, token
//     chunk) order in a second kernel;
//   * nothing is rounded to 16 bits; dzeros is negated once (exact);
//   * rows of x and dy at or past M and columns of dy at or past N contribute nothing (they are never read);
//   * deterministic: no atomics, the same call gives bit-identical outputs.
//
// Tiling.  Both operands have the contraction index (tokens) as their slow dimension, so both are staged token-major,
// exactly as they lie in memory, and the MFMA fragments (8 consecutive contraction indices per lane) come from gfx950's
// transposing LDS read, as in the Hessian's X^T X:
//   * a workgroup (4 waves) owns 128 rows of K x 128 columns of N and walks its tokens in stages of 32: the [32][128] tile
//     of x and that of dy go global -> registers -> LDS (one stage ahead in registers, two LDS buffers, one barrier per
//     stage).  LDS rows are 288 bytes (256 + 32 pad);
//   * one MFMA k-step is one stage.  Lane group h = lane >> 4 takes LDS rows 4h + j (element j < 4) and 16 + 4h + j - 4
//     (j >= 4) of both operands: which token is which contraction index is free as long as the operands agree, and this
//     choice puts the 8 rows a 32-lane half reads at once (4h + q, h = 0, 1) on 8 different 32-byte bank slots
//     (row * 288 mod 256 = 32 * row), so the transposed reads are conflict-free; rows 8h + j, the natural order, would
//     put rows 0 and 8 on one slot;
//   * wave w owns the 32-row slab w of the tile (one row of packed 32-code groups) against all 128 columns:
//     2 x 8 accumulator tiles, 4 transposed reads of x and 16 of dy per 16 MFMAs;
//   * epilogue: acc[b][nb][r] is storage row 32w + 16b + 4h + r, column 16nb + (lane & 15).  The 4 codes of a lane's rows
//     are 4 * bits consecutive bits of the slab's stream of 32 * bits bits: a window of one or two packed words.  The
//     lane sums q*A and A over its 8 rows, the wave over its lane groups, and the 4 slab sums meet in LDS;
//   * slabs of one tile that lie in the same group are added there: seg = gcd(4, slabs per group) slabs make one
//     segment.  Where a segment is a whole group (groupsize 32, 64, 128) and the tokens are not split the kernel writes
//     dscales / dzeros itself; otherwise (per-row grids, larger or odd groups, split tokens) segment partials go to
//     the workspace [2][chunks][K / (32 seg)][N] and qgemm_g_reduce_kernel adds them;
//   * the token range is split into `chunks` (grid z) when the K x N tiles alone would leave the chip mostly empty;
//   * dbias: wave 0 of the workgroups of the first K tile multiplies a fragment of ones with its dy fragments -- one
//     more MFMA per column block, in the same launch;
//   * act-order: x[:, perm] is gathered once into the workspace by a pre-pass and the plain kernel runs on the copy.
//     The alternative, gathering while staging, would redo the 2-byte gather for every one of the N / 128 column tiles
//     (86 times at N = 11008) in place of two 16-byte loads per thread; the pre-pass moves M * K * 4 bytes once.  The
//     choice is reasoned, tools/bench_qgemm.py --grid-grad measures the whole call.
#include <algorithm>

#include "common.h"

namespace gptq {

typedef short gg_s4 __attribute__((__vector_size__(4 * sizeof(short))));
typedef short gg_s8 __attribute__((ext_vector_type(8)));
typedef _Float16 gg_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 gg_b8 __attribute__((ext_vector_type(8)));
typedef float gg_f4 __attribute__((ext_vector_type(4)));

constexpr int GG_TK = 128;             // rows of K per workgroup (4 slabs of 32, one per wave)
constexpr int GG_TN = 128;             // columns of N per workgroup
constexpr int GG_BM = 32;              // tokens per stage = one MFMA k-step
constexpr int GG_ROW = 144;            // LDS row stride in 16-bit elements (128 + 16 pad = 288 B)
constexpr int GG_TILE = GG_BM * GG_ROW;
constexpr int GG_TARGET_WG = 512;      // the token split aims at two workgroups per CU
constexpr int GG_FULL_TILES = 256;     // from this many K x N tiles on the tokens are not split
constexpr int GG_MAX_CHUNKS = 64;

template <bool BF16>
__device__ __forceinline__ gg_f4 gg_mfma(gg_s8 a, gg_s8 b, gg_f4 c) {
  if (BF16) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(gg_b8, a), __builtin_bit_cast(gg_b8, b), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(gg_h8, a), __builtin_bit_cast(gg_h8, b), c, 0, 0, 0);
}

// this thread's 2 x 16-byte pieces of the [32 tokens][128 channels] tile of P at token m0, channel c0; tokens at or past
// M and channels at or past C read as 0
__device__ __forceinline__ void gg_load(const unsigned short* __restrict__ P, long ld, int m0, int M, int c0, int C, bool vec,
                                        uint4 r[2]) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int v = threadIdx.x + 256 * e;
    const int m = m0 + (v >> 4), c = c0 + (v & 15) * 8;
    r[e] = make_uint4(0, 0, 0, 0);
    if (m < M && c < C) {
      const unsigned short* p = P + (long)m * ld + c;
      if (vec && c + 8 <= C) {
        r[e] = *reinterpret_cast<const uint4*>(p);
      } else {
        uint32_t t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = c + j < C ? p[j] : 0u;
        r[e] = make_uint4(t[0] | (t[1] << 16), t[2] | (t[3] << 16), t[4] | (t[5] << 16), t[6] | (t[7] << 16));
      }
    }
  }
}

__device__ __forceinline__ void gg_store(unsigned short* S, const uint4 r[2]) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int v = threadIdx.x + 256 * e;
    *reinterpret_cast<uint4*>(S + (v >> 4) * GG_ROW + (v & 15) * 8) = r[e];
  }
}

// the fragment of 16 channels at p: LDS rows 4h + j and 16 + 4h + j of the lane's group (p already holds row 4h + q)
__device__ __forceinline__ gg_s8 gg_frag(const unsigned short* p) {
  const gg_s4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) gg_s4*)(p));
  const gg_s4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) gg_s4*)(p + 16 * GG_ROW));
  return gg_s8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
}

struct GgOut {
  float* ds;        // direct: dscales [G][N]; otherwise the partials [chunks][P][N]
  float* dz;        // the same for dzeros
  float* db;        // dbias [N] (chunks == 1) or its partials [chunks][N]; nullptr: no bias gradient
  int seg;          // slabs per segment: 1, 2 or 4
  int P;            // segments in K: K / (32 seg)
};

// Grid: (K tiles, N tiles, token chunks).  Block: 256 threads.
template <int BITS, bool BF16>
__global__ __launch_bounds__(256) void qgemm_g_kernel(const unsigned short* __restrict__ x, int ldx,
                                                      const unsigned short* __restrict__ dy, int lddy, int M,
                                                      const uint32_t* __restrict__ qw, int K, int N, int chunk_steps,
                                                      GgOut out, bool xvec, bool dvec) {
  __shared__ __attribute__((aligned(16))) unsigned short sm[2][2][GG_TILE];   // [buffer][x, dy]
  __shared__ float red[2][4][GG_TN];                                          // [S, Z][slab][column]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 4, i = lane & 15, q = (lane >> 2) & 3, p = lane & 3;
  const int k0 = blockIdx.x * GG_TK, n0 = blockIdx.y * GG_TN;
  const int nsteps = (M + GG_BM - 1) / GG_BM;
  const int sbeg = blockIdx.z * chunk_steps, send = min(nsteps, sbeg + chunk_steps);
  const bool live = k0 + 32 * wave < K;                       // wave-uniform: a slab past K only helps staging
  const bool ones = out.db != nullptr && blockIdx.x == 0 && wave == 0;
  const int nbmax = min(8, (N - n0 + 15) >> 4);               // column blocks with a column below N

  gg_f4 acc[2][8], accb[8];
#pragma unroll
  for (int nb = 0; nb < 8; ++nb) {
    acc[0][nb] = acc[1][nb] = accb[nb] = gg_f4{0.f, 0.f, 0.f, 0.f};
  }
  const short one = BF16 ? (short)0x3F80 : (short)0x3C00;
  const gg_s8 fone = gg_s8{one, one, one, one, one, one, one, one};
  const int frag_off = (4 * h + q) * GG_ROW + 4 * p;

  uint4 rx[2], rd[2];
  if (sbeg < send) {
    gg_load(x, ldx, sbeg * GG_BM, M, k0, K, xvec, rx);
    gg_load(dy, lddy, sbeg * GG_BM, M, n0, N, dvec, rd);
    gg_store(sm[0][0], rx);
    gg_store(sm[0][1], rd);
  }
  __syncthreads();
  int cur = 0;
  for (int s = sbeg; s < send; ++s) {
    const bool more = s + 1 < send;
    if (more) {
      gg_load(x, ldx, (s + 1) * GG_BM, M, k0, K, xvec, rx);
      gg_load(dy, lddy, (s + 1) * GG_BM, M, n0, N, dvec, rd);
    }
    if (live) {
      const unsigned short* xs = sm[cur][0] + frag_off + 32 * wave;
      const unsigned short* ds = sm[cur][1] + frag_off;
      const gg_s8 fa0 = gg_frag(xs), fa1 = gg_frag(xs + 16);
#pragma unroll
      for (int nb = 0; nb < 8; ++nb) {
        if (nb < nbmax) {
          const gg_s8 fb = gg_frag(ds + 16 * nb);
          acc[0][nb] = gg_mfma<BF16>(fa0, fb, acc[0][nb]);
          acc[1][nb] = gg_mfma<BF16>(fa1, fb, acc[1][nb]);
          if (ones) accb[nb] = gg_mfma<BF16>(fone, fb, accb[nb]);
        }
      }
    }
    if (more) {
      gg_store(sm[cur ^ 1][0], rx);
      gg_store(sm[cur ^ 1][1], rd);
    }
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue: the slab sums of this wave ----
  if (live) {
    const int slab = (k0 >> 5) + wave;
    const uint32_t mask = (1u << BITS) - 1u;
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) {
      const int n = n0 + 16 * nb + i;
      float sq = 0.f, sa = 0.f;
      if (nb < nbmax && n < N) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int off = BITS * 4 * (4 * b + h);               // first bit of the 4 codes in the slab's stream
          const int lo = off >> 5, hi = min(lo + 1, BITS - 1);
          const uint32_t wlo = qw[(size_t)(slab * BITS + lo) * N + n];
          const uint32_t whi = qw[(size_t)(slab * BITS + hi) * N + n];
          const uint32_t win = (uint32_t)((((uint64_t)whi << 32) | wlo) >> (off & 31));
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float a = acc[b][nb][r];
            const float c = (float)((win >> (BITS * r)) & mask);
            sq = __fadd_rn(sq, __fmul_rn(c, a));
            sa = __fadd_rn(sa, a);
          }
        }
      }
      sq = __fadd_rn(sq, __shfl_xor(sq, 16));
      sa = __fadd_rn(sa, __shfl_xor(sa, 16));
      sq = __fadd_rn(sq, __shfl_xor(sq, 32));
      sa = __fadd_rn(sa, __shfl_xor(sa, 32));
      if (h == 0) {
        red[0][wave][16 * nb + i] = sq;
        red[1][wave][16 * nb + i] = sa;
      }
    }
    if (ones && h == 0) {
#pragma unroll
      for (int nb = 0; nb < 8; ++nb) {
        const int n = n0 + 16 * nb + i;
        if (nb < nbmax && n < N) out.db[(size_t)blockIdx.z * N + n] = accb[nb][0];
      }
    }
  } else if (h == 0) {
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) red[0][wave][16 * nb + i] = red[1][wave][16 * nb + i] = 0.f;
  }
  __syncthreads();

  // ---- the segments of this tile: thread = (S or Z, column) ----
  const int which = tid >> 7, col = tid & 127, n = n0 + col;
  if (n >= N) return;
  float* dst = which ? out.dz : out.ds;
  for (int sg = 0; sg < 4 / out.seg; ++sg) {
    const int pi = blockIdx.x * (4 / out.seg) + sg;
    if (pi >= out.P) break;
    float v = red[which][sg * out.seg][col];
    for (int w = 1; w < out.seg; ++w) v = __fadd_rn(v, red[which][sg * out.seg + w][col]);
    dst[((size_t)blockIdx.z * out.P + pi) * N + n] = which ? -v : v;
  }
}

// out[g][n] = the partials of group g in ascending (segment, chunk) order; dbias[n] = its chunk partials in order.
// Thread = one output: [0, G N) dscales, [G N, 2 G N) dzeros, then N of dbias (where it has partials).
__global__ __launch_bounds__(256) void qgemm_g_reduce_kernel(const float* __restrict__ ps, const float* __restrict__ pz,
                                                             const float* __restrict__ pb, int chunks, int P, int per_group,
                                                             int G, int N, float* __restrict__ dscales,
                                                             float* __restrict__ dzeros, float* __restrict__ dbias) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t GN = (size_t)G * N;
  if (ps && idx < 2 * GN) {
    const bool z = idx >= GN;
    const size_t o = z ? idx - GN : idx;
    const int g = (int)(o / N), n = (int)(o % N);
    const float* part = z ? pz : ps;
    float v = 0.f;
    for (int s = 0; s < per_group; ++s)
      for (int c = 0; c < chunks; ++c) {
        const float t = part[((size_t)c * P + (size_t)g * per_group + s) * N + n];
        v = s == 0 && c == 0 ? t : __fadd_rn(v, t);
      }
    (z ? dzeros : dscales)[o] = v;
  } else if (pb && idx >= 2 * GN && idx < 2 * GN + N) {
    const int n = (int)(idx - 2 * GN);
    float v = pb[n];
    for (int c = 1; c < chunks; ++c) v = __fadd_rn(v, pb[(size_t)c * N + n]);
    dbias[n] = v;
  }
}

// xp[m][k] = x[m][perm[k]] (an entry of perm outside [0, K) reads as 0: never a stray read)
__global__ __launch_bounds__(256) void qgemm_g_gather_kernel(const unsigned short* __restrict__ x, int ldx, int M, int K,
                                                             const int32_t* __restrict__ perm,
                                                             unsigned short* __restrict__ xp) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)M * K) return;
  const int m = (int)(idx / K), k = (int)(idx % K);
  const int c = perm[k];
  xp[idx] = (unsigned)c < (unsigned)K ? x[(size_t)m * ldx + c] : (unsigned short)0;
}

// The plan is a pure function of the shape, so the workspace queries need no device.
struct GgPlan {
  int seg, P, per_group, G;      // slabs per segment, segments in K, segments per group, groups
  int chunk_steps, chunks;       // token stages per chunk, chunks
  bool direct;                   // the kernel writes dscales / dzeros itself
};

static GgPlan gg_plan(int M, int K, int N, int groupsize) {
  GgPlan p;
  const int slabs = K / 32;
  const int gslabs = groupsize > 0 ? groupsize / 32 : slabs;     // slabs per group
  p.seg = gslabs % 4 == 0 ? 4 : gslabs % 2 == 0 ? 2 : 1;
  p.P = slabs / p.seg;
  p.per_group = gslabs / p.seg;
  p.G = slabs / gslabs;
  const int nsteps = cdiv(M, GG_BM);
  const long tiles = (long)cdiv(K, GG_TK) * cdiv(N, GG_TN);
  long S = tiles >= GG_FULL_TILES ? 1 : (GG_TARGET_WG + tiles - 1) / tiles;
  S = std::min<long>(S, std::max(1, nsteps / 2));                // at least 2 stages of 32 tokens per chunk
  S = std::max<long>(1, std::min<long>(S, GG_MAX_CHUNKS));
  p.chunk_steps = cdiv(nsteps, S);
  p.chunks = cdiv(nsteps, p.chunk_steps);
  p.direct = p.per_group == 1 && p.chunks == 1;
  return p;
}

static size_t gg_workspace_bytes(const GgPlan& p, int M, int K, int N, bool with_perm) {
  Carver c(nullptr);
  if (!p.direct) {
    c.take<float>((size_t)p.chunks * p.P * N);
    c.take<float>((size_t)p.chunks * p.P * N);
  }
  if (p.chunks > 1) c.take<float>((size_t)p.chunks * N);
  if (with_perm) c.take<unsigned short>((size_t)M * K);
  return c.off ? c.used() : 0;
}

static bool gg_shape_ok(int M, int K, int N, int bits, int groupsize) {
  return M > 0 && N > 0 && K >= 32 && K % 32 == 0 && (bits == 2 || bits == 3 || bits == 4 || bits == 8) &&
         (groupsize <= 0 || (groupsize % 32 == 0 && K % groupsize == 0));
}

}  // namespace gptq

using namespace gptq;

extern "C" size_t gptq_quant_gemm_grid_grad_workspace_bytes(int M, int K, int N, int bits, int groupsize) {
  if (!gg_shape_ok(M, K, N, bits, groupsize)) return 0;
  return gg_workspace_bytes(gg_plan(M, K, N, groupsize), M, K, N, false);
}

extern "C" size_t gptq_quant_gemm_grid_grad_perm_workspace_bytes(int M, int K, int N, int bits, int groupsize) {
  if (!gg_shape_ok(M, K, N, bits, groupsize)) return 0;
  return gg_workspace_bytes(gg_plan(M, K, N, groupsize), M, K, N, true);
}

extern "C" int gptq_quant_gemm_grid_grad(const void* x, int x_dtype, int ldx, const void* dy, int lddy, int M,
                                         const int32_t* qweight, const int32_t* perm, int K, int N, int bits,
                                         int groupsize, float* dscales, float* dzeros, float* dbias, void* workspace,
                                         size_t workspace_bytes, gptq_stream_t stream) {
  const char* who = "gptq_quant_gemm_grid_grad";
  hipStream_t s = static_cast<hipStream_t>(stream);
  GPTQ_CHECK_ARG(x && dy && qweight && dscales && dzeros, "%s: null pointer", who);
  GPTQ_CHECK_ARG(bits == 2 || bits == 3 || bits == 4 || bits == 8, "%s: bits must be 2, 3, 4 or 8", who);
  GPTQ_CHECK_ARG(M >= 1 && N >= 1 && K >= 32 && K % 32 == 0, "%s: need M >= 1, N >= 1 and K a positive multiple of 32", who);
  GPTQ_CHECK_ARG(x_dtype == GPTQ_F16 || x_dtype == GPTQ_BF16, "%s: x and dy must be fp16 or bf16", who);
  GPTQ_CHECK_ARG(ldx >= K && lddy >= N, "%s: ldx must be >= K and lddy >= N", who);
  GPTQ_CHECK_ARG(groupsize <= 0 || (groupsize % 32 == 0 && K % groupsize == 0),
                 "%s: groupsize must be a multiple of 32 that divides K", who);
  GPTQ_CHECK_ARG(!perm || groupsize > 0, "%s: perm needs grouped grids (groupsize > 0)", who);
  GPTQ_CHECK_ARG((size_t)M * K < ((size_t)1 << 40) && (size_t)M * ldx < ((size_t)1 << 62) &&
                     (size_t)M * lddy < ((size_t)1 << 62) && (size_t)(K / 32 * bits) * N < ((size_t)1 << 60) &&
                     (size_t)K * N < ((size_t)1 << 40),
                 "%s: shape too large", who);
  GPTQ_CHECK_ARG(cdiv(N, GG_TN) <= 65535, "%s: N too large", who);
  const GgPlan p = gg_plan(M, K, N, groupsize);
  const size_t need = gg_workspace_bytes(p, M, K, N, perm != nullptr);
  GPTQ_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace),
                 "%s: workspace of %zu bytes needed (%s%s_workspace_bytes)", who, need, who, perm ? "_perm" : "");
  GPTQ_CHECK_ARG(need == 0 || reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "%s: workspace must be 16-byte aligned", who);
  Carver c(workspace);
  float *ps = nullptr, *pz = nullptr, *pb = nullptr;
  if (!p.direct) {
    ps = c.take<float>((size_t)p.chunks * p.P * N);
    pz = c.take<float>((size_t)p.chunks * p.P * N);
  }
  if (p.chunks > 1) pb = c.take<float>((size_t)p.chunks * N);
  const unsigned short* xs = static_cast<const unsigned short*>(x);
  if (perm) {
    unsigned short* xp = c.take<unsigned short>((size_t)M * K);
    const size_t MK = (size_t)M * K;
    qgemm_g_gather_kernel<<<dim3((unsigned)((MK + 255) / 256)), 256, 0, s>>>(xs, ldx, M, K, perm, xp);
    GPTQ_CHECK_LAUNCH(who);
    xs = xp;
    ldx = K;
  }
  GgOut out;
  out.ds = p.direct ? dscales : ps;
  out.dz = p.direct ? dzeros : pz;
  out.db = !dbias ? nullptr : p.chunks > 1 ? pb : dbias;
  out.seg = p.seg;
  out.P = p.P;
  const bool xvec = reinterpret_cast<uintptr_t>(xs) % 16 == 0 && ldx % 8 == 0;
  const bool dvec = reinterpret_cast<uintptr_t>(dy) % 16 == 0 && lddy % 8 == 0;
  const dim3 grid(cdiv(K, GG_TK), cdiv(N, GG_TN), p.chunks);
  const unsigned short* dp = static_cast<const unsigned short*>(dy);
  const uint32_t* qp = reinterpret_cast<const uint32_t*>(qweight);
#define GG_GO(B, BF) qgemm_g_kernel<B, BF><<<grid, 256, 0, s>>>(xs, ldx, dp, lddy, M, qp, K, N, p.chunk_steps, out, xvec, dvec)
  if (x_dtype == GPTQ_F16) {
    if (bits == 2) GG_GO(2, false);
    else if (bits == 3) GG_GO(3, false);
    else if (bits == 8) GG_GO(8, false);
    else GG_GO(4, false);
  } else {
    if (bits == 2) GG_GO(2, true);
    else if (bits == 3) GG_GO(3, true);
    else if (bits == 8) GG_GO(8, true);
    else GG_GO(4, true);
  }
#undef GG_GO
  GPTQ_CHECK_LAUNCH(who);
  if (!p.direct || (dbias && p.chunks > 1)) {
    const size_t total = 2 * (size_t)p.G * N + N;
    qgemm_g_reduce_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, s>>>(
        ps, pz, dbias ? pb : nullptr, p.chunks, p.P, p.per_group, p.G, N, dscales, dzeros, dbias);
    GPTQ_CHECK_LAUNCH(who);
  }
  return GPTQ_OK;
}
