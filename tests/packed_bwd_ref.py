"""Reference side of the packed backward tests (gptq_quant_gemm_t / quant_matmul_t), independent of the code under test.

Nothing here calls gptq_amd.  The bit layouts come from packed_ref (3 / 4 bits) and packed_ref_wide (2 / 8 bits), and
every reference is computed from `unpack(qweight)`, i.e. from the buffer the kernel is actually given.

The contract:

    dx[m][c(k)] = sum_n dy[m][n] * W16[k][n],   c(k) = perm[k] if perm is given else k
    W16[k][n]   = round_to_dy_dtype(scales[g][n] * q[k][n] - zeros[g][n]),   g = k // groupsize (0 for per-row grids)

W16 is formed in float32 with a separate multiply and subtract and rounded once to the 16-bit type of dy: numpy float32
reproduces that bit for bit, so W16 is part of the reference.  dy (fp16 / bf16) times W16 is exact in fp32; only the fp32
sum over n rounds, and the result is rounded once to y_dtype.

* `dyadic_bwd_case`: dy = small integers / 4, scales 2^-6..2^-8, zeros = integer * scale with |q - zero| <= 255, so W16 =
  scale * (q - zero) is exact in fp16 and in bf16 (8 significant bits).  Every product and partial sum is a multiple of
  lsb = min(scale) / 4; while T = sum_n |dy W16| stays below 2^24 lsb no fp32 operation rounds, in any order, and the
  kernel must EQUAL the reference.
* `realistic_bwd_case`: the weights of packed_ref.realistic_case against a realistic dy.  The bar is derived:
  an fp32 chain of N exact products is off by at most N 2^-24 T (each of the N - 1 adds rounds a partial sum of
  magnitude <= T by at most 2^-24 T), plus half an ulp of y_dtype at the reference value for the final rounding.
"""
from __future__ import annotations

import types

import numpy as np

import packed_ref as R0
import packed_ref_wide as RW

TWO24 = float(2 ** 24)
BITS = (2, 3, 4, 8)
BWD_KINDS = ("randn", "outlier", "tiny_scale")
torch_dtype = R0.torch_dtype
assert_equal_bits = R0.assert_equal_bits


def pack(codes, bits):
    return R0.pack(codes, bits) if bits in (3, 4) else RW.pack(codes, bits)


def unpack(qweight, bits):
    return R0.unpack(qweight, bits) if bits in (3, 4) else RW.unpack(qweight, bits)


def w16(qweight, scales, zeros, bits, groupsize, dy_dtype):
    """W16 [K, N] as fp64 values: float32 multiply, float32 subtract, one rounding to dy_dtype (through torch)."""
    import torch
    codes = unpack(np.asarray(qweight), bits)
    K, N = codes.shape
    s = np.asarray(scales, dtype=np.float32).reshape(-1, N)
    z = np.asarray(zeros, dtype=np.float32).reshape(-1, N)
    grp = np.arange(K) // groupsize if groupsize > 0 else np.zeros(K, dtype=np.int64)
    prod = (s[grp] * codes.astype(np.float32)).astype(np.float32)       # a separate fp32 multiply ...
    w32 = (prod - z[grp]).astype(np.float32)                            # ... and a separate fp32 subtract
    return torch.from_numpy(w32).to(torch_dtype(dy_dtype)).double().numpy()


def _scatter(a, perm):
    if perm is None:
        return a
    out = np.zeros_like(a)
    out[:, np.asarray(perm, dtype=np.int64)] = a
    return out


def ref_dx64(dy, qweight, scales, zeros, bits, groupsize, perm, dy_dtype):
    """(fp64 dx [M, K], T [M, K] = sum_n |dy W16|), both scattered by perm."""
    W = w16(qweight, scales, zeros, bits, groupsize, dy_dtype)
    d = np.asarray(dy.double().numpy() if hasattr(dy, "double") else dy, dtype=np.float64)
    return _scatter(d @ W.T, perm), _scatter(np.abs(d) @ np.abs(W).T, perm)


def round_to(a64, y_dtype):
    """fp64 -> y_dtype (torch tensor) with ONE rounding.  (A conversion through fp32 would round twice; the mantissa is
    cut here directly, to nearest even.)"""
    import torch
    a = np.asarray(a64, dtype=np.float64)
    if y_dtype == "f32":
        return torch.from_numpy(a.astype(np.float32))
    p, emin = {"f16": (10, -14), "bf16": (7, -126)}[y_dtype]
    m, e = np.frexp(a)                                       # a = m 2^e, 0.5 <= |m| < 1
    e = np.maximum(e - 1, emin)                              # exponent of the binade (subnormals: emin)
    q = np.ldexp(1.0, e - p)                                 # the ulp there
    r = np.rint(a / q) * q                                   # nearest, ties to even (exact: a / q has <= 53 bits)
    return torch.from_numpy(r).to(torch_dtype(y_dtype))     # r is a number of y_dtype (or past its range: inf)


def ref_dx(dy, qweight, scales, zeros, bits, groupsize, perm, dy_dtype, y_dtype):
    """The contract's dx as a torch tensor of y_dtype: unpack, W16 in float32 rounded to dy_dtype, fp64 product, scatter
    by perm, one rounding."""
    dx, _ = ref_dx64(dy, qweight, scales, zeros, bits, groupsize, perm, dy_dtype)
    return round_to(dx, y_dtype)


def half_ulp(ref64, y_dtype):
    """Half an ulp of y_dtype at the (fp64) reference values."""
    p, emin = {"f32": (23, -126), "f16": (10, -14), "bf16": (7, -126)}[y_dtype]
    _, e = np.frexp(np.asarray(ref64, dtype=np.float64))
    return 0.5 * np.ldexp(1.0, np.maximum(e - 1, emin) - p)


def derived_bar(ref64, T, N, y_dtype):
    """|dx - ref| <= N 2^-24 T + half an ulp of y_dtype at ref (module docstring)."""
    return N * 2.0 ** -24 * T + half_ulp(ref64, y_dtype)


def dyadic_bwd_case(bits, K, N, groupsize, M, perm=False, seed=0, dy_dtype="f16"):
    """Exact-arithmetic inputs (module docstring).  Namespace: codes [K, N], qweight, scales / zeros fp32 ([G, N] or [N]),
    perm (int32 [K] or None), dy (torch [M, N] in dy_dtype), ref (fp64 [M, K], scattered), T, lsb, headroom =
    max T / lsb / 2^24 (< 1 by construction)."""
    import torch
    assert K % 32 == 0 and (groupsize <= 0 or (groupsize % 32 == 0 and K % groupsize == 0))
    rng = np.random.default_rng([seed, bits, K, N, max(groupsize, 0), M, int(bool(perm)), 91])
    maxq = 2 ** bits - 1
    c = types.SimpleNamespace(bits=bits, K=K, N=N, groupsize=groupsize, M=M, dy_dtype=dy_dtype)
    c.codes = rng.integers(0, maxq + 1, (K, N), dtype=np.uint8)
    c.codes[rng.integers(0, K), :] = maxq                    # the largest code is always there
    G = K // groupsize if groupsize > 0 else 1
    sc = np.ldexp(1.0, -rng.integers(6, 9, (G, N))).astype(np.float32)
    zint = rng.integers(0, maxq + 1, (G, N))                 # |q - zero| <= maxq <= 255
    zr = (zint * sc.astype(np.float64)).astype(np.float32)
    c.scales, c.zeros = (sc, zr) if groupsize > 0 else (sc[0], zr[0])
    c.perm = rng.permutation(K).astype(np.int32) if perm else None
    c.qweight = pack(c.codes, bits)
    assert np.array_equal(unpack(c.qweight, bits), c.codes)
    c.lsb = float(sc.min()) / 4.0
    dseed = int(rng.integers(0, 2 ** 31))
    for R in (16, 8, 4, 2, 1):
        di = np.random.default_rng(dseed).integers(-R, R + 1, (M, N))
        c.dy = torch.from_numpy((di / 4.0).astype(np.float32)).to(torch_dtype(dy_dtype))
        c.dy_range = R
        c.ref, c.T = ref_dx64(c.dy, c.qweight, c.scales, c.zeros, bits, groupsize, c.perm, dy_dtype)
        c.headroom = float(c.T.max()) / c.lsb / TWO24
        if c.headroom < 1.0:
            return c
    raise ValueError(f"dyadic_bwd_case: no dy range keeps {bits}-bit K={K} N={N} g={groupsize} exact "
                     f"(headroom {c.headroom:.3g} at dy in {{-1, 0, 1}} / 4)")


def realistic_bwd_case(kind, bits, K, N, groupsize, M, seed=0, dy_dtype="f16"):
    """The weights of packed_ref.realistic_case (0.02 * randn on a min/max grid per group; `tiny_scale`: grid steps around
    1e-6) against dy = 0.1 * randn rounded to dy_dtype (`outlier`: four of the N columns times 100).  Same namespace as
    dyadic_bwd_case, no exactness claim."""
    import torch
    assert kind in BWD_KINDS and bits in (3, 4)
    w = R0.realistic_case(kind, bits, K, N, groupsize, 1, seed=seed, x_dtype="f16")
    rng = np.random.default_rng([seed, bits, K, N, max(groupsize, 0), M, BWD_KINDS.index(kind), 92])
    c = types.SimpleNamespace(bits=bits, K=K, N=N, groupsize=groupsize, M=M, dy_dtype=dy_dtype, kind=kind, perm=None)
    c.codes, c.qweight, c.scales, c.zeros, c.bias = w.codes, w.qweight, w.scales, w.zeros, w.bias
    dy = 0.1 * rng.standard_normal((M, N))
    if kind == "outlier":
        dy[:, rng.choice(N, 4, replace=False)] *= 100.0
    c.dy = torch.from_numpy(dy.astype(np.float32)).to(torch_dtype(dy_dtype))
    c.ref, c.T = ref_dx64(c.dy, c.qweight, c.scales, c.zeros, bits, groupsize, None, dy_dtype)
    return c


# ------------------------------------------------------------------------------------------------ the GPU table
F16, BF16 = "f16", "bf16"
# (K, N, groupsize); -1: per-row grids.  32 x 4: one 3-bit stream, one partly filled step; 96 x 20: N no multiple of 8
# or 32, K no multiple of the wave's 128 rows; 160 x 100 and 256 x 264: more than one tile each way (N = 264: the N range
# is split at M <= 16); groupsize 32 and 64 where they divide K.  64 x 1040 reaches the N split at 2 and 3 bits, and at
# the two-subtile plan (M = 17).  544 x 40: a second workgroup along K (512 rows each), whose first wave is partly
# filled.  Every row runs at every width, both dy types, y = fp32 and y = dy's type, every M.
BWD_EXACT = [
    (32, 4, -1), (96, 20, -1), (160, 100, -1), (160, 100, 32), (256, 264, -1), (256, 264, 32), (256, 264, 64),
    (64, 1040, 32), (544, 40, 32),
]
BWD_MS = (1, 3, 17, 130)
BWD_DY = (F16, BF16)


def bwd_case_id(row):
    K, N, gs = row
    return f"{K}x{N}-" + ("row" if gs <= 0 else f"g{gs}")


def dev(a, device):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
