"""Reference side of the 2- and 8-bit packed tests, independent of the code under test (in the manner of packed_ref.py).

Nothing here calls gptq_amd to build an input or a reference.  The bit layout is written out from its one-sentence
definition -- qweight is int32 [K/32*bits, N]; code i of a column sits in word i // (32/bits) at bit
bits * (i % (32/bits)): the 4-bit rule with 16 two-bit or 4 eight-bit codes per word -- and every reference is computed
in fp64 from `unpack(qweight)`, i.e. from the buffer a kernel is actually given.  (packed_ref.pack / _finish are NOT
used: they know 3 and 4 bits only.  What is shared with that module is width-agnostic: the device copies, the bit-equality
assertion and the GEMM runner.)

`dyadic_case`: inputs for which fp32 arithmetic is EXACT.  x = small integers / 4, scales 2^-6..2^-8, zeros = integer *
scale, bias a multiple of 2^-8.  Every product and every partial sum, in any order, is an integer multiple of
lsb = min(scale) / 4, and as long as the contract magnitude

    T = sum_k (s q_k + z) |x_k| + |bias|

stays below 2^24 lsb no fp32 operation rounds, so the GEMM's output must EQUAL the fp64 reference.  The mat-vec decodes a
code c through the fp16 mantissa as 1024 + c 2^p against x 2^-p, i.e. it sums (c + 1024 2^-p) x and removes the constant
part per group: p = 8 at 2 bits, p = 2 at 8 bits, so the constant is MV_CONST = 4 (2-bit) and 256 (8-bit) per unit of x
and its sufficient bound is

    T_mv = sum_k (s (q_k + MV_CONST[bits]) + z) |x_k| + |bias|  <  2^24 lsb.

`dyadic_case` picks the x range so that T_mv (which covers T) stays below 2^24 lsb and raises if no range does.

`realistic_case`: 0.02 * randn weights on a min/max grid against activations with a mean, for the float bars.
"""
from __future__ import annotations

import types

import numpy as np

import packed_ref as R0

TWO24 = float(2 ** 24)
WIDE_BITS = (2, 8)
MV_CONST = {2: 4.0, 8: 256.0}          # 1024 * 2^-p of the mat-vec's mantissa decode (p = 8 / p = 2)

torch_dtype = R0.torch_dtype
dev_tensors = R0.dev_tensors
assert_equal_bits = R0.assert_equal_bits
run_gemm_exact = R0.run_gemm_exact


# ------------------------------------------------------------------------------------------------ bit layouts
def _pack_pow2(codes, bits):
    codes = np.asarray(codes)
    K, N = codes.shape
    cpw = 32 // bits
    assert K % 32 == 0 and int(codes.max(initial=0)) < 2 ** bits and int(codes.min(initial=0)) >= 0
    c = codes.reshape(K // cpw, cpw, N).astype(np.uint32)
    words = np.zeros((K // cpw, N), dtype=np.uint32)
    for j in range(cpw):
        words |= c[:, j] << np.uint32(bits * j)
    return words.view(np.int32)


def _unpack_pow2(qweight, bits):
    q = np.ascontiguousarray(qweight).view(np.uint32)
    cpw = 32 // bits
    codes = np.empty((q.shape[0], cpw, q.shape[1]), dtype=np.uint8)
    for j in range(cpw):
        codes[:, j] = ((q >> np.uint32(bits * j)) & np.uint32(2 ** bits - 1)).astype(np.uint8)
    return codes.reshape(q.shape[0] * cpw, q.shape[1])


def pack2(codes):
    """codes [K, N] (0..3) -> int32 [K/16, N]: code i in word i // 16 at bit 2 * (i % 16)."""
    return _pack_pow2(codes, 2)


def unpack2(qweight):
    return _unpack_pow2(qweight, 2)


def pack8(codes):
    """codes [K, N] (0..255) -> int32 [K/4, N]: code i in byte i % 4 of word i // 4."""
    return _pack_pow2(codes, 8)


def unpack8(qweight):
    return _unpack_pow2(qweight, 8)


def pack(codes, bits):
    return {2: pack2, 8: pack8}[bits](codes)


def unpack(qweight, bits):
    return {2: unpack2, 8: unpack8}[bits](qweight)


# ------------------------------------------------------------------------------------------------ fp64 contract
def reference_and_magnitude(codes, scales, zeros, groupsize, x, bias, bits):
    """fp64 y = x @ (s q - z) + bias, T = |x| @ (s q + |z|) + |bias| and T_mv = |x| @ (s (q + MV_CONST) + |z|) + |bias|.
    codes [K, N]; x [M, K] in storage order (gathered by perm where there is one)."""
    K, N = codes.shape
    x = np.asarray(x, dtype=np.float64)
    s = np.asarray(scales, dtype=np.float64)
    z = np.asarray(zeros, dtype=np.float64)
    if groupsize <= 0:
        s, z = s.reshape(1, -1), z.reshape(1, -1)
    grp = np.arange(K) // groupsize if groupsize > 0 else np.zeros(K, dtype=np.int64)
    q = codes.astype(np.float64)
    sk, zk = s[grp], z[grp]
    xa = np.abs(x)
    ref = x @ (sk * q - zk)
    T = xa @ (sk * q + np.abs(zk))
    Tmv = T + MV_CONST[bits] * (xa @ sk)
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        ref, T, Tmv = ref + b, T + np.abs(b), Tmv + np.abs(b)
    return ref, T, Tmv


def _finish(c):
    """Packed words, fp64 reference, magnitudes; the reference is computed from unpack(qweight)."""
    if getattr(c, "qweight", None) is None:
        c.qweight = pack(c.codes, c.bits)
        c.unpacked = unpack(c.qweight, c.bits)
        assert np.array_equal(c.unpacked, c.codes)
    xs = c.x.double().numpy()
    c.xg = xs[:, c.perm] if c.perm is not None else xs       # storage order: packed row k multiplies x[:, perm[k]]
    c.ref, c.T, c.T_mv = reference_and_magnitude(c.unpacked, c.scales, c.zeros, c.groupsize, c.xg, c.bias, c.bits)
    return c


def dyadic_case(bits, K, N, groupsize, M, perm=False, seed=0, x_dtype="f16"):
    """Exact-arithmetic inputs (module docstring).  Returns a namespace: codes [K, N] uint8 (storage order), qweight,
    scales / zeros fp32 ([G, N], or [N] for groupsize <= 0), zero_int, bias, perm (int32 [K] or None), x (torch [M, K] in
    x_dtype, ORIGINAL column order), xg (fp64, storage order), ref (fp64 [M, N]), T, T_mv, lsb, headroom = max T / lsb /
    2^24 and headroom_mv (the same with T_mv; < 1 by construction)."""
    import torch
    assert bits in WIDE_BITS
    assert K % 32 == 0 and (groupsize <= 0 or (groupsize % 32 == 0 and K % groupsize == 0))
    rng = np.random.default_rng([seed, bits, K, N, max(groupsize, 0), M, int(bool(perm)), 77])
    maxq = 2 ** bits - 1
    c = types.SimpleNamespace(bits=bits, K=K, N=N, groupsize=groupsize, M=M, x_dtype=x_dtype)
    c.codes = rng.integers(0, maxq + 1, (K, N), dtype=np.uint8)
    c.codes[rng.integers(0, K), :] = maxq                    # the largest code is always there
    G = K // groupsize if groupsize > 0 else 1
    sc = np.ldexp(1.0, -rng.integers(6, 9, (G, N))).astype(np.float32)
    zint = rng.integers(0, maxq + 1, (G, N))
    zr = (zint * sc.astype(np.float64)).astype(np.float32)
    c.zero_int = zint.astype(np.float32) if groupsize > 0 else zint.astype(np.float32)[0]
    c.scales, c.zeros = (sc, zr) if groupsize > 0 else (sc[0], zr[0])
    c.bias = (rng.integers(-512, 513, N) / 256.0).astype(np.float32)
    c.perm = rng.permutation(K).astype(np.int32) if perm else None
    c.lsb = float(sc.min()) / 4.0
    xseed = int(rng.integers(0, 2 ** 31))
    for R in (16, 8, 4, 2, 1):
        xi = np.random.default_rng(xseed).integers(-R, R + 1, (M, K))
        c.x = torch.from_numpy((xi / 4.0).astype(np.float32)).to(torch_dtype(x_dtype))
        c.x_range = R
        _finish(c)
        c.headroom = float(c.T.max()) / c.lsb / TWO24
        c.headroom_mv = float(c.T_mv.max()) / c.lsb / TWO24
        if c.headroom_mv < 1.0:
            return c
    raise ValueError(f"dyadic_case: no x range keeps {bits}-bit K={K} N={N} g={groupsize} exact "
                     f"(headroom {c.headroom_mv:.3g} at x in {{-1, 0, 1}} / 4)")


def realistic_case(bits, K, N, groupsize, M, seed=0, x_dtype="f16"):
    """0.02 * randn weights on a min/max grid per group (per column for groupsize <= 0) against randn + 1 activations
    rounded to x_dtype.  Same namespace as dyadic_case plus Wdeq = s (q - zint) [K, N] in fp64 (no exactness claim)."""
    import torch
    rng = np.random.default_rng([seed, bits, K, N, max(groupsize, 0), M, 78])
    maxq = 2 ** bits - 1
    c = types.SimpleNamespace(bits=bits, K=K, N=N, groupsize=groupsize, M=M, x_dtype=x_dtype, perm=None)
    W = 0.02 * rng.standard_normal((K, N))
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
    c.x = torch.from_numpy((rng.standard_normal((M, K)) + 1.0).astype(np.float32)).to(torch_dtype(x_dtype))
    _finish(c)
    grp = np.arange(K) // gs
    c.Wdeq = sc.astype(np.float64)[grp] * c.unpacked - zr.astype(np.float64)[grp]
    return c


def emulate_fp32(c, seed=0, matvec=False):
    """The kernels' contract in fp32 numpy with a shuffled summation order: per group (per-row grids: per 256-k chunk)
    acc = sum(q x) and sx = sum(x) over a seeded permutation of the group's k, y += s acc - z sx, then + bias.
    matvec=True carries the mat-vec's constant part: acc over q + MV_CONST, minus MV_CONST sx."""
    rng = np.random.default_rng(seed)
    K, N = c.codes.shape
    x = c.xg.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), c.xg)
    s = np.asarray(c.scales, dtype=np.float32).reshape(-1, N)
    z = np.asarray(c.zeros, dtype=np.float32).reshape(-1, N)
    gs = c.groupsize if c.groupsize > 0 else 256
    k0c = np.float32(MV_CONST[c.bits])
    y = np.zeros((x.shape[0], N), dtype=np.float32)
    for g, k0 in enumerate(range(0, K, gs)):
        idx = k0 + rng.permutation(min(gs, K - k0))
        row = g if c.groupsize > 0 else 0
        xq = x[:, idx]
        q = c.codes[idx].astype(np.float32)
        sx = np.zeros(x.shape[0], dtype=np.float32)
        for j in range(xq.shape[1]):
            sx = sx + xq[:, j]
        acc = (xq @ (q + k0c) - k0c * sx[:, None]) if matvec else xq @ q
        y = y + (s[row][None, :] * acc - z[row][None, :] * sx[:, None])
    return y + c.bias[None, :]


# ------------------------------------------------------------------------------------------------ exact-case tables
F16, BF16 = "f16", "bf16"
# (K, N, groupsize, Ms, x dtype, perm); every row runs at 2 and 8 bits.  groupsize -1: per-row grids.  Classes: K = 32
# (one k-step), 96 / 160 (ragged last X tile), 1056 (33 steps), 1408 (split-K chunks that end inside a 128-group), 2048 (a
# group over two X tiles); N = 1, 3, 65, 255, 1001 (odd: the 16-byte word loads fall back); groupsize -1, 32, 96, 128,
# 512, K; M on both sides of every tile plan; both x types; with and without perm (M <= 4: fused gather, else pre-pass).
GEMM_EXACT = [
    (32, 1, -1, (1, 2, 3), F16, False),
    (32, 3, 32, (1, 4, 5), BF16, True),                      # groupsize == K
    (96, 65, 96, (15, 16, 17), F16, True),                   # groupsize == K, not a power of two
    (96, 255, 32, (31, 32, 33), BF16, False),
    (160, 65, 32, (63, 64, 65), F16, True),                  # 5 k-steps: ragged last X tile
    (160, 3, 160, (127, 128, 129), BF16, False),
    (1056, 255, 32, (1, 17, 129), F16, False),               # 33 k-steps
    (1056, 65, -1, (2, 33, 65), BF16, False),
    (1056, 1001, 96, (1, 4, 16), F16, True),
    (1408, 1001, 128, (1, 3, 16, 17), F16, False),           # split-K chunks cut the 128-groups
    (1408, 1000, 128, (4, 5, 129), BF16, True),
    (2048, 1001, 512, (1, 64, 65), BF16, True),              # groups over two X tiles
    (2048, 255, 2048, (3, 128), F16, True),                  # one group = K
    (2048, 65, -1, (1, 32, 33), F16, False),
]
# (in_f, width, groupsize); -1: the per-row entry points, > 0: vecquant_matmul_grouped with and without perm.
MATVEC_EXACT = [
    (32, 1, -1), (96, 130, 96), (416, 257, -1), (416, 255, 32), (416, 1000, 32), (1408, 4096, 128), (1408, 3, -1),
    (1408, 1000, -1), (2048, 260, 512), (4096, 256, 128), (4096, 1000, -1),
]
# out x in of the pack / dequant layout checks (513 x 1056 with 16-byte rows reaches the wide-tile pack kernel)
PACK_OUT = (1, 63, 513)
PACK_IN = (32, 96, 1056)


def case_id(row):
    return R0.case_id(row)


def run_matvec_exact(Q, dev, c, entry, what=""):
    """One mat-vec entry point on row 0 of the case, `mul` preloaded with the dyadic bias.  entry: 'row', 'rowh',
    'grouped', 'groupedh' (h: fp16 x); a case with perm goes through the grouped entry's perm argument."""
    import torch
    qw, s, z, b, perm = dev_tensors(c, dev)
    half = entry.endswith("h")
    x = c.x[0].to(dev).to(torch.float16 if half else torch.float32)
    mul = b.clone()
    if entry in ("row", "rowh"):
        fn = {2: Q.vecquant2matmul, 8: Q.vecquant8matmul}[c.bits]
        fn(x, qw, mul, s.reshape(-1, 1), z.reshape(-1, 1))
    else:
        Q.vecquant_matmul_grouped(x, qw, mul, s, z, c.bits, c.groupsize, perm=perm)
    ref = torch.from_numpy(c.ref[0]).to(dev).float()
    assert_equal_bits(mul, ref, f"{what} mat-vec '{entry}' {c.bits}-bit {c.K}x{c.N} g{c.groupsize}"
                      + (" perm" if perm is not None else ""))


def matvec_entries(groupsize):
    return ("grouped", "groupedh") if groupsize > 0 else ("row", "rowh")
