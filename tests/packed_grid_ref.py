"""Reference side of the grid-gradient tests (gptq_quant_gemm_grid_grad / quant_grid_grad), independent of the code
under test.

Nothing here calls gptq_amd.  The bit layouts come from packed_ref (3 / 4 bits) and packed_ref_wide (2 / 8 bits), and
every reference is computed from `unpack(qweight)`, i.e. from the buffer the kernel is actually given.

The contract (c(k) = perm[k] if perm is given else k, g = k // groupsize, 0 for per-row grids):

    y[m][n]       = sum_k x[m][c(k)] * (scales[g][n] * q[k][n] - zeros[g][n]) + bias[n]
    A[k][n]       = sum_m x[m][c(k)] * dy[m][n]
    dscales[g][n] =  sum_{k in g} q[k][n] * A[k][n]
    dzeros[g][n]  = -sum_{k in g} A[k][n]
    dbias[n]      =  sum_m dy[m][n]

x and dy are fp16 / bf16, so every product x * dy is exact in fp32; the kernel rounds only in its fp32 sums and in the one
multiply by the integer code.

* `dyadic_grid_case`: x and dy are small integers / 4, so every product is a multiple of 1 / 16 and so is every partial
  sum, also after the multiply by an integer code.  While max(T_S, T_Z) * 16 < 2^24, with T_S = sum_m sum_{k in g} |x dy| q
  and T_Z = sum_m sum_{k in g} |x dy|, no fp32 operation rounds, in any order, and the kernel must EQUAL the reference.
* `realistic_grid_case`: the weights of packed_ref.realistic_case against x = randn and dy = 0.1 * randn.  The bar is
  derived: A is a chain of M exact products (each add rounds a partial sum of magnitude <= its share of T by 2^-24), q * A
  is one more rounding, and the sum over the rows of a group at most `rows_in_group` more, each relative to a magnitude
  that T bounds: |dS - ref| <= (M + rows_in_group + 1) 2^-24 T_S, the same with T_Z for dZ, and M 2^-24 sum_m |dy| for dB.
"""
from __future__ import annotations

import types

import numpy as np

import packed_ref as R0
import packed_ref_wide as RW

TWO24 = float(2 ** 24)
BITS = (2, 3, 4, 8)
GRID_KINDS = ("randn", "outlier")
torch_dtype = R0.torch_dtype
assert_equal_bits = R0.assert_equal_bits


def pack(codes, bits):
    return R0.pack(codes, bits) if bits in (3, 4) else RW.pack(codes, bits)


def unpack(qweight, bits):
    return R0.unpack(qweight, bits) if bits in (3, 4) else RW.unpack(qweight, bits)


def _f64(a):
    return np.asarray(a.double().numpy() if hasattr(a, "double") else a, dtype=np.float64)


def ref_grid_grad64(x, dy, qweight, bits, groupsize, perm):
    """(dS, dZ, dB, T_S, T_Z) in fp64.  x [M, K] in ORIGINAL column order, dy [M, N]; dS / dZ / T_S / T_Z are [G, N]
    for grouped grids and [N] for per-row ones (groupsize <= 0), dB is [N]."""
    q = unpack(np.asarray(qweight), bits).astype(np.float64)
    K, N = q.shape
    X, D = _f64(x).reshape(-1, K), _f64(dy).reshape(-1, N)
    if perm is not None:
        X = X[:, np.asarray(perm, dtype=np.int64)]           # storage row k pairs with x[:, perm[k]]
    A = X.T @ D
    Aabs = np.abs(X).T @ np.abs(D)
    gs = groupsize if groupsize > 0 else K
    G = K // gs

    def per_group(a):
        s = a.reshape(G, gs, N).sum(1)
        return s if groupsize > 0 else s[0]

    return per_group(q * A), -per_group(A), D.sum(0), per_group(q * Aabs), per_group(Aabs)


def grid_bars(T_S, T_Z, dy, M, K, groupsize):
    """The derived bars (module docstring) for dS, dZ and dB."""
    rows = groupsize if groupsize > 0 else K
    u = 2.0 ** -24
    return (M + rows + 1) * u * T_S, (M + rows + 1) * u * T_Z, M * u * np.abs(_f64(dy)).sum(0)


def dyadic_grid_case(bits, K, N, groupsize, M, perm=False, seed=0, dtype="f16"):
    """Exact-arithmetic inputs (module docstring).  Namespace: codes [K, N], qweight, perm (int32 [K] or None), x (torch
    [M, K]) and dy (torch [M, N]) in `dtype`, value_range R, T_S / T_Z at all M tokens and headroom = max(T_S, T_Z) * 16 /
    2^24 (< 1 by construction; T only shrinks with fewer tokens, so every prefix x[:m], dy[:m] is exact too)."""
    import torch
    assert K % 32 == 0 and (groupsize <= 0 or (groupsize % 32 == 0 and K % groupsize == 0))
    rng = np.random.default_rng([seed, bits, K, N, max(groupsize, 0), M, int(bool(perm)), 93])
    maxq = 2 ** bits - 1
    c = types.SimpleNamespace(bits=bits, K=K, N=N, groupsize=groupsize, M=M, dtype=dtype)
    c.codes = rng.integers(0, maxq + 1, (K, N), dtype=np.uint8)
    c.codes[rng.integers(0, K), :] = maxq                    # the largest code is always there
    c.perm = rng.permutation(K).astype(np.int32) if perm else None
    c.qweight = pack(c.codes, bits)
    assert np.array_equal(unpack(c.qweight, bits), c.codes)
    vseed = int(rng.integers(0, 2 ** 31))
    for R in (16, 8, 4, 2, 1):
        vr = np.random.default_rng(vseed)
        xi, di = vr.integers(-R, R + 1, (M, K)), vr.integers(-R, R + 1, (M, N))
        c.x = torch.from_numpy((xi / 4.0).astype(np.float32)).to(torch_dtype(dtype))
        c.dy = torch.from_numpy((di / 4.0).astype(np.float32)).to(torch_dtype(dtype))
        c.value_range = R
        _, _, _, c.T_S, c.T_Z = ref_grid_grad64(c.x, c.dy, c.qweight, bits, groupsize, c.perm)
        c.headroom = max(float(c.T_S.max()), float(c.T_Z.max())) * 16.0 / TWO24
        if c.headroom < 1.0:
            return c
    raise ValueError(f"dyadic_grid_case: no value range keeps {bits}-bit K={K} N={N} g={groupsize} M={M} exact "
                     f"(headroom {c.headroom:.3g} at values in {{-1, 0, 1}} / 4)")


def realistic_grid_case(kind, bits, K, N, groupsize, M, seed=0, dtype="f16"):
    """The weights of packed_ref.realistic_case (0.02 * randn on a min/max grid per group) against x = randn and dy = 0.1 *
    randn rounded to `dtype` (`outlier`: four columns of x and four of dy times 100).  Namespace: codes, qweight,
    scales, zeros, bias, x, dy, the fp64 reference dS / dZ / dB with T_S / T_Z, and the derived bars bar_S / bar_Z /
    bar_B.  No exactness claim."""
    import torch
    assert kind in GRID_KINDS and bits in (3, 4)
    w = R0.realistic_case("randn", bits, K, N, groupsize, 1, seed=seed, x_dtype="f16")
    rng = np.random.default_rng([seed, bits, K, N, max(groupsize, 0), M, GRID_KINDS.index(kind), 94])
    c = types.SimpleNamespace(bits=bits, K=K, N=N, groupsize=groupsize, M=M, dtype=dtype, kind=kind, perm=None)
    c.codes, c.qweight, c.scales, c.zeros, c.bias = w.codes, w.qweight, w.scales, w.zeros, w.bias
    x, dy = rng.standard_normal((M, K)), 0.1 * rng.standard_normal((M, N))
    if kind == "outlier":
        x[:, rng.choice(K, 4, replace=False)] *= 100.0
        dy[:, rng.choice(N, 4, replace=False)] *= 100.0
    c.x = torch.from_numpy(x.astype(np.float32)).to(torch_dtype(dtype))
    c.dy = torch.from_numpy(dy.astype(np.float32)).to(torch_dtype(dtype))
    c.dS, c.dZ, c.dB, c.T_S, c.T_Z = ref_grid_grad64(c.x, c.dy, c.qweight, bits, groupsize, None)
    c.bar_S, c.bar_Z, c.bar_B = grid_bars(c.T_S, c.T_Z, c.dy, M, K, groupsize)
    return c


# ------------------------------------------------------------------------------------------------ the GPU table
F16, BF16 = "f16", "bf16"
# (K, N, groupsize); -1: per-row grids.  A workgroup owns 128 rows of K (4 slabs of 32) x 128 columns and walks the tokens
# in stages of 32.  32 x 4: one slab, one partly filled column block; 96 x 20 and 160 x 100: K no multiple of the tile, an
# odd number of slabs per group (segments of one slab); 256 x 264: more than one tile each way, per-row grids in segments
# of 4 slabs, groups of 32 / 64 rows written by the kernel itself (segments of 1 / 2 slabs); 64 x 1040: many column
# tiles; 544 x 40: five K tiles, the last one a single slab.  The last two rows reach what the others do not: a GROUPED
# grid that spans several segments (192 x 24, groups of 96 rows = 3 segments) and a group that is exactly one tile
# (256 x 40, groups of 128 rows).  Every M <= 64 is one token chunk; M = 130 (5 stages) is split into two chunks.
GRID_EXACT = [
    (32, 4, -1), (96, 20, -1), (160, 100, -1), (160, 100, 32), (256, 264, -1), (256, 264, 32), (256, 264, 64),
    (64, 1040, 32), (544, 40, 32), (544, 40, -1), (192, 24, 96), (256, 40, 128),
]
GRID_MS = (1, 3, 17, 130)
GRID_DT = (F16, BF16)
GRID_PERM = [(160, 100, 32), (256, 264, 64), (64, 1040, 32)]


def grid_case_id(row):
    K, N, gs = row
    return f"{K}x{N}-" + ("row" if gs <= 0 else f"g{gs}")


def dev(a, device):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
