"""Reference side of the int8-activation packed GEMM tests (quant_matmul_a8), independent of the code under test.

Nothing here calls gptq_amd.  The bit layouts are those of packed_ref (3 / 4 bits) and packed_ref_wide (2 / 8 bits), by
import; every reference is computed from `unpack(qweight)`, i.e. from the buffer a kernel is given.

The contract (include/gptq_hip.h):

    a = max_k |x[m][k]| (fp32),  sx[m] = a / 127 (IEEE fp32; 1 when a == 0),
    xq[m][k] = clamp(rint(x[m][c(k)] / sx[m]), -127, 127)         (true division, half-even; c(k) = perm[k] or k)
    I_g = sum_{k in g} q[k][n] xq[m][k],  X_g = sum_{k in g} xq[m][k]                                   (exact integers)
    y[m][n] = sx[m] * sum_g (s[g][n] float(I_g) - z[g][n] float(X_g)) + bias[n]     (fp32, one rounding to the output)

* `quantize_ref`: the activation quantization in torch fp32 on the CPU, exactly as written.
* `gemm_ref`: the GEMM in int64 / fp64, with the magnitude T = sx * sum_g (|s I_g| + |z X_g|) + |bias|.
* `dyadic_case`: inputs on which NO fp32 operation of the contract rounds, in any order.  x = integers in [-127, 127]
  times 2^-j with at least one +-127 per row, so sx = 2^-j exactly and xq are those integers (asserted here through
  `quantize_ref`).  scales 2^-6..2^-8, zeros = integer * scale, bias a multiple of 2^-8: every term s I_g, z X_g and every
  partial sum of them is a multiple of lsb = 2^-8, and as long as  T_in = sum_g (|s I_g| + |z X_g|) + |bias| 2^j  stays
  below 2^24 lsb = 2^16, every |I_g|, |X_g| and |zero_int X_g| is below 2^24 (exact int -> float conversions and
  products), every partial fp32 sum is exact, and so are the multiplication by sx = 2^-j and the bias add.  The kernel's
  fp32 output must EQUAL the fp64 reference, and its fp16 / bf16 output the single rounding of it.
* `realistic_case`: 0.02 * randn weights on a min/max grid against the activation kinds of packed_ref.REALISTIC_KINDS.
"""
from __future__ import annotations

import types

import numpy as np

import packed_ref as R0
import packed_ref_wide as RW

TWO24 = float(2 ** 24)
BITS = (2, 3, 4, 8)
REALISTIC_KINDS = R0.REALISTIC_KINDS
MAX_K = 65536

torch_dtype = R0.torch_dtype
assert_equal_bits = R0.assert_equal_bits


def pack(codes, bits):
    return R0.pack(codes, bits) if bits in (3, 4) else RW.pack(codes, bits)


def unpack(qweight, bits):
    return R0.unpack(qweight, bits) if bits in (3, 4) else RW.unpack(qweight, bits)


# ------------------------------------------------------------------------------------------------ the contract
def quantize_ref(x, perm=None):
    """x [M, K] torch fp16 / bf16 (CPU) -> (xq int8 [M, K], sx fp32 [M]) in torch fp32, exactly as the contract reads."""
    import torch
    xf = x.detach().cpu().float()
    if perm is not None:
        xf = xf[:, torch.as_tensor(np.asarray(perm)).long()]
    a = xf.abs().amax(dim=1)
    sx = a / torch.full_like(a, 127.0)                       # (a tensor divisor: a true fp32 division)
    sx = torch.where(a == 0, torch.ones_like(sx), sx)
    q = torch.round(xf / sx[:, None]).clamp(-127, 127)       # torch.round is half-even
    return q.to(torch.int8), sx


def group_sums(codes, xq, groupsize):
    """I [G, M, N] and X [G, M] as int64 from codes [K, N] and xq [M, K]."""
    K, N = codes.shape
    gs = groupsize if groupsize > 0 else K
    assert K <= MAX_K                                        # every sum below 2^31: exact in an fp64 matmul
    q = codes.astype(np.float64).reshape(K // gs, gs, N)
    a = np.asarray(xq).astype(np.float64).reshape(-1, K // gs, gs).transpose(1, 0, 2)   # [G, M, gs]
    return np.matmul(a, q).astype(np.int64), a.sum(axis=2).astype(np.int64)


def gemm_ref(codes, scales, zeros, groupsize, xq, sx, bias=None):
    """fp64 y and the magnitude T (module docstring), both [M, N]."""
    N = codes.shape[1]
    s = np.asarray(scales, dtype=np.float64).reshape(-1, N)
    z = np.asarray(zeros, dtype=np.float64).reshape(-1, N)
    I, X = group_sums(codes, xq, groupsize)
    I, X = I.astype(np.float64), X.astype(np.float64)[:, :, None]
    inner = (s[:, None, :] * I - z[:, None, :] * X).sum(axis=0)
    mag = (np.abs(s[:, None, :] * I) + np.abs(z[:, None, :] * X)).sum(axis=0)
    sxd = np.asarray(sx, dtype=np.float64)[:, None]
    ref, T = sxd * inner, sxd * mag
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        ref, T = ref + b, T + np.abs(b)
    return ref, T


def emulate_fp32(c, order, seed=0):
    """The contract after the integers in numpy fp32: float(I_g), float(X_g), s * I - z * X per group, the groups added
    in `order` ('forward', 'reverse' or 'shuffled'), times sx, plus bias."""
    N = c.N
    s = np.asarray(c.scales, dtype=np.float32).reshape(-1, N)
    z = np.asarray(c.zeros, dtype=np.float32).reshape(-1, N)
    I, X = group_sums(c.unpacked, c.xq, c.groupsize)
    If, Xf = I.astype(np.float32), X.astype(np.float32)
    assert np.array_equal(If.astype(np.int64), I) and np.array_equal(Xf.astype(np.int64), X)
    idx = list(range(I.shape[0]))
    if order == "reverse":
        idx.reverse()
    elif order == "shuffled":
        np.random.default_rng(seed).shuffle(idx)
    tot = np.zeros(I.shape[1:], dtype=np.float32)
    for g in idx:
        tot = tot + (s[g][None, :] * If[g] - z[g][None, :] * Xf[g][:, None])
    y = np.asarray(c.sx, dtype=np.float32)[:, None] * tot
    return y + c.bias[None, :] if c.bias is not None else y


def _grids(rng, bits, K, N, groupsize):
    maxq = 2 ** bits - 1
    G = K // groupsize if groupsize > 0 else 1
    sc = np.ldexp(1.0, -rng.integers(6, 9, (G, N))).astype(np.float32)
    zint = rng.integers(0, maxq + 1, (G, N))
    zr = (zint * sc.astype(np.float64)).astype(np.float32)
    return (sc, zr) if groupsize > 0 else (sc[0], zr[0])


def dyadic_case(bits, K, N, groupsize, M, j=3, perm=False, seed=0, x_dtype="f16"):
    """Exact-arithmetic inputs (module docstring).  Namespace: codes [K, N] uint8 (storage order), qweight, unpacked,
    scales / zeros fp32 ([G, N], or [N] for groupsize <= 0), bias, perm (int32 [K] or None), x (torch [M, K] in x_dtype,
    ORIGINAL column order), xq int8 [M, K] and sx fp32 [M] (storage order, = quantize_ref(x, perm)), ref / T (fp64 [M, N]),
    x_range, and headroom = max T_in / 2^16 (< 1 by construction)."""
    import torch
    assert bits in BITS and K % 32 == 0 and (groupsize <= 0 or (groupsize % 32 == 0 and K % groupsize == 0))
    rng = np.random.default_rng([seed, bits, K, N, max(groupsize, 0), M, int(bool(perm)), j, 88])
    maxq = 2 ** bits - 1
    c = types.SimpleNamespace(bits=bits, K=K, N=N, groupsize=groupsize, M=M, x_dtype=x_dtype, j=j)
    c.codes = rng.integers(0, maxq + 1, (K, N), dtype=np.uint8)
    c.codes[rng.integers(0, K), :] = maxq                    # the largest code is always there
    c.scales, c.zeros = _grids(rng, bits, K, N, groupsize)
    c.bias = (rng.integers(-512, 513, N) / 256.0).astype(np.float32)
    c.perm = rng.permutation(K).astype(np.int32) if perm else None
    c.qweight = pack(c.codes, bits)
    c.unpacked = unpack(c.qweight, bits)
    assert np.array_equal(c.unpacked, c.codes)
    xseed = int(rng.integers(0, 2 ** 31))
    for R in (127, 64, 32, 16, 8, 4, 2, 1):
        r2 = np.random.default_rng(xseed)
        xi = r2.integers(-R, R + 1, (M, K))                  # storage order
        xi[np.arange(M), r2.integers(0, K, M)] = 127 * r2.choice([-1, 1], M)
        xs = np.ldexp(xi.astype(np.float64), -j)
        xo = np.empty_like(xs)
        if perm:
            xo[:, c.perm] = xs                                # x[:, perm[k]] = storage column k
        else:
            xo = xs
        c.x = torch.from_numpy(xo.astype(np.float32)).to(torch_dtype(x_dtype))
        assert np.array_equal(c.x.double().numpy(), xo)       # |integer| <= 127: exact in fp16 and bf16
        xq, sx = quantize_ref(c.x, c.perm)
        c.xq, c.sx = xq.numpy(), sx.numpy()
        assert np.array_equal(c.xq, xi) and np.all(c.sx == np.float32(2.0 ** -j))
        c.x_range = R
        c.ref, c.T = gemm_ref(c.unpacked, c.scales, c.zeros, groupsize, c.xq, c.sx, c.bias)
        c.headroom = float((c.T / c.sx[:, None].astype(np.float64)).max()) / 2.0 ** 16
        if c.headroom < 1.0:
            return c
    raise ValueError(f"dyadic_case: no x range keeps {bits}-bit K={K} N={N} g={groupsize} exact (headroom {c.headroom:.3g})")


def realistic_case(kind, bits, K, N, groupsize, M, seed=0, x_dtype="f16"):
    """0.02 * randn weights on a min/max grid per group (per column for groupsize <= 0) against `kind` activations
    rounded to x_dtype (the kinds of packed_ref.realistic_case).  Namespace as dyadic_case without xq / sx / ref: the
    GPU test computes the reference from the kernel's own (xq, sx)."""
    import torch
    assert kind in REALISTIC_KINDS and bits in BITS
    rng = np.random.default_rng([seed, bits, K, N, max(groupsize, 0), M, REALISTIC_KINDS.index(kind), 89])
    maxq = 2 ** bits - 1
    c = types.SimpleNamespace(bits=bits, K=K, N=N, groupsize=groupsize, M=M, x_dtype=x_dtype, kind=kind, perm=None)
    W = 0.02 * rng.standard_normal((K, N))
    if kind == "tiny_scale":
        W *= 1e-4
    gs = groupsize if groupsize > 0 else K
    Wg = W.reshape(K // gs, gs, N)
    lo, hi = np.minimum(Wg.min(1), 0.0), np.maximum(Wg.max(1), 0.0)
    sc = ((hi - lo) / maxq).astype(np.float32)
    zint = np.round(-lo / sc)
    codes = np.clip(np.round(Wg / sc[:, None, :]) + zint[:, None, :], 0, maxq)
    c.codes = codes.reshape(K, N).astype(np.uint8)
    zr = (zint * sc).astype(np.float32)
    c.scales, c.zeros = (sc, zr) if groupsize > 0 else (sc[0], zr[0])
    c.bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    x = rng.standard_normal((M, K))
    if kind == "relu":
        x = np.maximum(x, 0.0)
    elif kind == "mean3":
        x = x + 3.0
    elif kind == "outlier":
        x[:, rng.choice(K, 4, replace=False)] *= 100.0
    elif kind == "subnormal":
        x = x * 2.0 ** -20
    c.x = torch.from_numpy(x.astype(np.float32)).to(torch_dtype(x_dtype))
    c.qweight = pack(c.codes, bits)
    c.unpacked = unpack(c.qweight, bits)
    assert np.array_equal(c.unpacked, c.codes)
    return c


def realistic_bar(c, xq, sx, out_dtype_eps):
    """(ref, bar): the fp64 formula on the given (xq, sx) and the derived bound c T + u_out |ref|,
    c = (4 G + 4) 2^-24: per group two int -> float conversions, two products and two adds, then the scale and the bias."""
    ref, T = gemm_ref(c.unpacked, c.scales, c.zeros, c.groupsize, xq, sx, c.bias)
    G = c.K // c.groupsize if c.groupsize > 0 else 1
    return ref, (4 * G + 4) * 2.0 ** -24 * T + out_dtype_eps * np.abs(ref)


# ------------------------------------------------------------------------------------------------ the exact-case table
F32, F16, BF16 = "f32", "f16", "bf16"
# (K, N, groupsize, Ms, output dtype, bias, input form, j); every row runs at 2, 3, 4 and 8 bits.  groupsize -1: per-row
# grids.  Axes: grids per-row / g32 / g64 / g96 / g128 / g = K; K 32, 96, 160, 1056 (all with a K % 64 == 32 tail) where K
# admits the groupsize -- none of them is a multiple of 64, so g64 and g128 run at K = 192, 384 and 1152 (a ragged last
# xq tile; a K % 64 tail cannot exist there); M 1, 15, 16, 17, 33, 65, 129; N 1, 7, 64, 257, 520; fp32 / fp16 / bf16
# output, with and without bias; x given as a tensor ('x') or as the pair ('pair').  Small M at K >= 1056 split K: int32
# partials for per-row grids, fp32 partials between groups for grouped ones; larger M at the same K does not split.
GEMM_EXACT = [
    (32, 1, -1, (1,), F32, True, "x", 3),
    (32, 7, 32, (15, 16), F16, False, "pair", 0),             # g32 = K
    (96, 64, 32, (17,), BF16, True, "pair", 5),
    (96, 257, 96, (33,), F32, False, "x", 3),                 # g96 = K
    (160, 520, 32, (65,), F16, True, "x", 2),
    (160, 7, 160, (129,), F32, True, "pair", 4),              # g = K over 2.5 steps
    (160, 257, -1, (17, 129), BF16, False, "x", 3),
    (1056, 257, -1, (1, 17), F32, True, "x", 3),              # per-row K split: int32 partials
    (1056, 520, 32, (1, 33), F32, False, "pair", 3),          # grouped K split: fp32 partials
    (1056, 7, 96, (15, 65), F16, True, "x", 1),               # 96-groups: every other step is two half steps
    (1056, 64, 1056, (16, 129), F32, True, "pair", 3),        # g = K: one chunk, no split
    (192, 257, 64, (17,), F32, True, "x", 3),
    (1152, 7, 64, (1, 129), BF16, True, "pair", 3),
    (384, 257, 128, (33,), F16, False, "x", 3),
    (1152, 520, 128, (1, 17, 65), F32, True, "x", 6),
]


def case_id(row):
    K, N, gs = row[:3]
    return f"{K}x{N}-" + ("row" if gs <= 0 else f"g{gs}")


def grid_kind(K, gs):
    return "row" if gs <= 0 else "gK" if gs == K else f"g{gs}"
