"""Reference side of the packed forward tests, independent of the code under test.

Nothing here calls gptq_amd to build an input or a reference: the bit layouts are written out from their description
(DESIGN.md "Packed weights": 3-bit = code j of a 32-group at bit 3j of the group's 96-bit little-endian stream of three
int32 words; 4-bit = nibble i % 8 of word i // 8; qweight int32 [K/32*bits, N]), and every reference is computed in fp64
from `unpack(qweight)`, i.e. from the buffer a kernel is actually given.

Two families of inputs:

* `dyadic_case`: inputs for which fp32 arithmetic is EXACT.  x = small integers / 4, scales 2^-6..2^-8, zeros = integer
  * scale, bias a multiple of 2^-8.  Every product and every partial sum, in any order, is then an integer multiple of
  lsb = min(scale) / 4, and as long as the contract magnitude T = sum_k (s q_k + z)|x_k| + |bias| stays below 2^24 lsb
  no fp32 operation rounds: MFMA-internal adds, split-K partials, the mat-vec's atomics.  The kernel's output must EQUAL
  the fp64 reference.  The mat-vec's second-generation kernel also sums the constant part 1024 * 2^-p * x (at most 32 per
  unit of x), so its sufficient bound is T_mv with q + 32 in place of q; `dyadic_case` picks the x range so that T_mv
  stays below 2^24 lsb (which covers the GEMM's T as well) and raises if no range does.
* `realistic_case`: 0.02 * randn weights on a real min/max grid per group (codes cluster round the zero point like GPTQ
  output) against activations that are not zero-mean randn, for float bars proportional to T.

The `--exact-sweep` entry point runs a handful of exact cases in a fresh process (for library builds whose kernel
selection is read from the environment once per process).
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TWO24 = float(2 ** 24)
X_DTYPES = ("f16", "bf16", "f32")
REALISTIC_KINDS = ("randn", "relu", "mean3", "outlier", "subnormal", "tiny_scale")


def torch_dtype(name):
    import torch
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[name]


# ------------------------------------------------------------------------------------------------ bit layouts
def pack3(codes):
    """codes [K, N] (0..7) -> int32 [K/32*3, N]: code j of a 32-group at bit 3j of the little-endian 96-bit stream."""
    codes = np.asarray(codes)
    K, N = codes.shape
    assert K % 32 == 0 and int(codes.max(initial=0)) <= 7
    c = codes.reshape(K // 32, 32, N).astype(np.uint64)
    words = np.zeros((K // 32, 3, N), dtype=np.uint64)
    for j in range(32):
        word, off = divmod(3 * j, 32)
        v = c[:, j] << np.uint64(off)                       # up to bit 34: the part past bit 31 belongs to the next word
        words[:, word] |= v & np.uint64(0xFFFFFFFF)
        if off > 29:
            words[:, word + 1] |= v >> np.uint64(32)
    return words.reshape(K // 32 * 3, N).astype(np.uint32).view(np.int32)


def unpack3(qweight):
    """int32 [K/32*3, N] -> codes [K, N] uint8."""
    q = np.ascontiguousarray(qweight).view(np.uint32).astype(np.uint64)
    G, N = q.shape[0] // 3, q.shape[1]
    q = q.reshape(G, 3, N)
    lo = q[:, 0] | (q[:, 1] << np.uint64(32))               # bits 0..63
    hi = q[:, 1] | (q[:, 2] << np.uint64(32))               # bits 32..95
    codes = np.empty((G, 32, N), dtype=np.uint8)
    for j in range(32):
        bit = 3 * j
        v = (lo >> np.uint64(bit)) if bit + 3 <= 64 else (hi >> np.uint64(bit - 32))
        codes[:, j] = (v & np.uint64(7)).astype(np.uint8)
    return codes.reshape(G * 32, N)


def pack4(codes):
    """codes [K, N] (0..15) -> int32 [K/8, N]: nibble i % 8 of word i // 8."""
    codes = np.asarray(codes)
    K, N = codes.shape
    assert K % 8 == 0 and int(codes.max(initial=0)) <= 15
    c = codes.reshape(K // 8, 8, N).astype(np.uint32)
    words = np.zeros((K // 8, N), dtype=np.uint32)
    for j in range(8):
        words |= c[:, j] << np.uint32(4 * j)
    return words.view(np.int32)


def unpack4(qweight):
    q = np.ascontiguousarray(qweight).view(np.uint32)
    codes = np.empty((q.shape[0], 8, q.shape[1]), dtype=np.uint8)
    for j in range(8):
        codes[:, j] = ((q >> np.uint32(4 * j)) & np.uint32(15)).astype(np.uint8)
    return codes.reshape(q.shape[0] * 8, q.shape[1])


def pack(codes, bits):
    return pack3(codes) if bits == 3 else pack4(codes)


def unpack(qweight, bits):
    return unpack3(qweight) if bits == 3 else unpack4(qweight)


# ------------------------------------------------------------------------------------------------ fp64 contract
def _group_rows(K, groupsize):
    return np.arange(K) // groupsize if groupsize > 0 else np.zeros(K, dtype=np.int64)


def _tables(scales, zeros, groupsize):
    s = np.asarray(scales, dtype=np.float64)
    z = np.asarray(zeros, dtype=np.float64)
    if groupsize <= 0:
        s, z = s.reshape(1, -1), z.reshape(1, -1)
    return s, z


def reference_and_magnitude(codes, scales, zeros, groupsize, x, bias=None):
    """fp64 y = x @ (s q - z) + bias, T = |x| @ (s q + z) + |bias| and T_mv = |x| @ (s (q + 32) + z) + |bias|.
    codes [K, N]; x [M, K] already in storage order (gathered by perm where there is one).  K is walked in slabs so that
    the 36864 x 9216 shape never holds a dense fp64 matrix."""
    K, N = codes.shape
    x = np.asarray(x, dtype=np.float64)
    s, z = _tables(scales, zeros, groupsize)
    grp = _group_rows(K, groupsize)
    ref = np.zeros((x.shape[0], N))
    T = np.zeros_like(ref)
    Tmv = np.zeros_like(ref)
    slab = max(32, min(K, (1 << 25) // max(N, 1) // 32 * 32))
    for k0 in range(0, K, slab):
        k1 = min(K, k0 + slab)
        q = codes[k0:k1].astype(np.float64)
        sk, zk = s[grp[k0:k1]], z[grp[k0:k1]]
        xs, xa = x[:, k0:k1], np.abs(x[:, k0:k1])
        sq = sk * q
        ref += xs @ (sq - zk)
        t = xa @ (sq + np.abs(zk))
        T += t
        Tmv += t + 32.0 * (xa @ sk)
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        ref += b
        T += np.abs(b)
        Tmv += np.abs(b)
    return ref, T, Tmv


def contract_magnitude(codes, scales, zeros, groupsize, x, bias=None, matvec=False):
    """T = sum_k (s_g q_k + z_g) |x_k| + |bias| per output element [M, N]; matvec=True: T_mv with q_k + 32."""
    _, T, Tmv = reference_and_magnitude(codes, scales, zeros, groupsize, x, bias)
    return Tmv if matvec else T


def _finish(c):
    """Packed words, fp64 reference, magnitudes; the reference is computed from unpack(qweight)."""
    if getattr(c, "qweight", None) is None:
        c.qweight = pack(c.codes, c.bits)
        c.unpacked = unpack(c.qweight, c.bits)
        assert np.array_equal(c.unpacked, c.codes)
    back = c.unpacked
    xs = c.x.double().numpy()
    c.xg = xs[:, c.perm] if c.perm is not None else xs       # storage order: packed row k multiplies x[:, perm[k]]
    c.ref, c.T, c.T_mv = reference_and_magnitude(back, c.scales, c.zeros, c.groupsize, c.xg, c.bias)
    return c


def dyadic_case(bits, K, N, groupsize, M, perm=False, seed=0, x_dtype="f16"):
    """Exact-arithmetic inputs (module docstring).  Returns a namespace: codes [K, N] uint8 (storage order), qweight,
    scales / zeros fp32 ([G, N], or [N] for groupsize <= 0), bias, perm (int32 [K] or None), x (torch [M, K] in x_dtype,
    ORIGINAL column order), xg (fp64, storage order), ref (fp64 [M, N]), T, T_mv, lsb, headroom = max T / lsb / 2^24 and
    headroom_mv (the same with T_mv; < 1 by construction)."""
    import torch
    assert K % 32 == 0 and (groupsize <= 0 or (groupsize % 32 == 0 and K % groupsize == 0))
    rng = np.random.default_rng([seed, bits, K, N, max(groupsize, 0), M, int(bool(perm))])
    maxq = 2 ** bits - 1
    c = types.SimpleNamespace(bits=bits, K=K, N=N, groupsize=groupsize, M=M, x_dtype=x_dtype)
    c.codes = rng.integers(0, maxq + 1, (K, N), dtype=np.uint8)
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
        if N > 1024 and R > 1:                               # cheap look at 64 columns first: skip a range that is too wide
            _, _, t = reference_and_magnitude(c.codes[:, :64], sc[:, :64] if groupsize > 0 else sc[0, :64],
                                              zr[:, :64] if groupsize > 0 else zr[0, :64], groupsize,
                                              np.abs(xi / 4.0)[:, c.perm] if perm else np.abs(xi / 4.0))
            if float(t.max()) / c.lsb / TWO24 >= 0.9:
                continue
        _finish(c)
        c.headroom = float(c.T.max()) / c.lsb / TWO24
        c.headroom_mv = float(c.T_mv.max()) / c.lsb / TWO24
        if c.headroom_mv < 1.0:
            return c
    raise ValueError(f"dyadic_case: no x range keeps {bits}-bit K={K} N={N} g={groupsize} exact "
                     f"(headroom {c.headroom_mv:.3g} at x in {{-1, 0, 1}} / 4)")


def realistic_case(kind, bits, K, N, groupsize, M, seed=0, x_dtype="f16"):
    """0.02 * randn weights on a min/max grid per group (per column for groupsize <= 0) against `kind` activations
    rounded to x_dtype.  Same namespace as dyadic_case (no perm, no exactness claim)."""
    import torch
    assert kind in REALISTIC_KINDS
    rng = np.random.default_rng([seed, bits, K, N, max(groupsize, 0), M, REALISTIC_KINDS.index(kind)])
    maxq = 2 ** bits - 1
    c = types.SimpleNamespace(bits=bits, K=K, N=N, groupsize=groupsize, M=M, x_dtype=x_dtype, kind=kind, perm=None)
    W = 0.02 * rng.standard_normal((K, N))
    if kind == "tiny_scale":
        W *= 1e-4                                            # grid steps around 1e-6
    gs = groupsize if groupsize > 0 else K
    Wg = W.reshape(K // gs, gs, N)
    lo, hi = np.minimum(Wg.min(1), 0.0), np.maximum(Wg.max(1), 0.0)
    sc = ((hi - lo) / maxq).astype(np.float32)               # [G, N]
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
    return _finish(c)


def emulate_fp32(c, seed=0, matvec=False):
    """The kernels' contract in fp32 numpy with a shuffled summation order: per group (per-row grids: per 256-k chunk,
    like a K split) acc = sum(q x) and sx = sum(x) over a seeded permutation of the group's k, y += s acc - z sx, then
    + bias.  matvec=True also carries the second-generation mat-vec's constant part: acc over q + 32, minus 32 sx."""
    rng = np.random.default_rng(seed)
    K, N = c.codes.shape
    x = c.xg.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), c.xg)
    s, z = _tables(c.scales, c.zeros, c.groupsize)
    s, z = s.astype(np.float32), z.astype(np.float32)
    gs = c.groupsize if c.groupsize > 0 else 256
    y = np.zeros((x.shape[0], N), dtype=np.float32)
    for g, k0 in enumerate(range(0, K, gs)):
        idx = k0 + rng.permutation(min(gs, K - k0))
        row = g if c.groupsize > 0 else 0
        xq = x[:, idx]
        q = c.codes[idx].astype(np.float32)
        sx = np.zeros(x.shape[0], dtype=np.float32)
        for j in range(xq.shape[1]):                         # a plain fp32 chain in the shuffled order
            sx = sx + xq[:, j]
        if matvec:
            acc = xq @ (q + np.float32(32.0)) - np.float32(32.0) * sx[:, None]
        else:
            acc = xq @ q
        y = y + (s[row][None, :] * acc - z[row][None, :] * sx[:, None])
    return y + c.bias[None, :]


# ------------------------------------------------------------------------------------------------ exact-case tables
F16, BF16 = "f16", "bf16"
# (K, N, groupsize, Ms, x dtype, perm); every row runs at 3 and 4 bits.  groupsize -1: per-row grids.
GEMM_EXACT = [
    (32, 1, -1, (1, 2, 3), F16, False),
    (32, 3, 32, (1, 4, 5), BF16, True),                      # groupsize == K
    (96, 5, 96, (15, 16, 17), F16, True),                    # groupsize == K, not a power of two
    (96, 63, 32, (31, 32, 33), BF16, False),
    (160, 65, 32, (63, 64, 65), F16, True),                  # 5 k-steps: ragged last X tile
    (160, 130, 160, (127, 128, 129), BF16, False),
    (1056, 255, 32, (1, 17, 255), F16, False),               # 33 k-steps
    (1056, 257, -1, (2, 33, 257), BF16, False),
    (1152, 130, 96, (1, 5, 65, 129), F16, True),
    (1408, 1001, 128, (1, 3, 16, 17), F16, False),           # split-K chunks of 9 / 11 / 15 steps cut the 128-groups
    (1408, 1000, 64, (4, 129), BF16, True),
    (2048, 4096, 256, (1, 2, 33), F16, False),               # groups over two X tiles
    (2048, 1001, 512, (1, 64, 65), BF16, True),
    (2048, 255, 2048, (3, 128), F16, True),                  # one group = K
    (4096, 1000, 128, (1, 15, 257), F16, True),
    (4096, 4096, -1, (1, 5, 32), BF16, False),
    (4096, 257, 64, (2, 31, 63), F16, False),
    (4096, 3, 512, (1, 127), BF16, True),
]
# (in_f, width, groupsize); -1: the per-row entry points, > 0: vecquant_matmul_grouped with and without perm.
MATVEC_EXACT = [
    (32, 1, -1), (32, 4096, 32), (96, 3, 32), (96, 130, 96), (416, 255, 32), (416, 257, -1), (416, 1000, -1),
    (1152, 1000, 96), (1408, 4096, 128), (1408, 130, 64), (1408, 3, -1), (4096, 1000, 256), (4096, 4096, 512),
    (4096, 257, 4096), (4096, 130, -1), (4096, 4096, -1), (4096, 1, 128), (36864, 9216, -1),
]
# the child-process sweeps (diagnostic library): fused-gather GEMM kernels at every tile plan, mat-vec workgroup sizes
SWEEP_GEMM_PERM = [(160, 65, 32, (17, 33), F16), (1152, 130, 96, (65, 129), BF16), (1408, 1001, 128, (17, 129), F16),
                   (2048, 257, 512, (33, 65), BF16)]
SWEEP_MATVEC = [(416, 1000, 32), (416, 257, -1), (1408, 4096, 128), (1408, 130, 64), (4096, 1000, 512), (4096, 1000, -1)]


def case_id(row):
    K, N, gs = row[:3]
    return f"{K}x{N}-" + ("row" if gs <= 0 else f"g{gs}")


# ------------------------------------------------------------------------------------------------ GPU runners
def dev_tensors(c, dev):
    """The case's operands on `dev` (qweight, scales, zeros, bias, perm or None)."""
    import torch
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t(c.qweight), t(c.scales), t(c.zeros), t(c.bias), t(c.perm)


def assert_equal_bits(got, want, what):
    import torch
    if not torch.equal(got, want):
        g, w = got.double().cpu(), want.double().cpu()
        bad = (g != w) | (g.isnan() != w.isnan())
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact reference; "
                             f"first at {i}: got {float(g[i])!r}, want {float(w[i])!r}")


def run_gemm_exact(G, dev, c, Ms, what=""):
    """quant_matmul on rows [:m] of the case for every m in Ms: fp32 output == reference, the same call twice gives the
    same bits, rounded output == the single rounding of the exact value, bias=None as well."""
    import torch
    qw, s, z, b, perm = dev_tensors(c, dev)
    ref = torch.from_numpy(c.ref).to(dev)
    nobias = ref - b.double()
    xdt = torch_dtype(c.x_dtype)
    for m in Ms:
        x = c.x[:m].to(dev)
        tag = f"{what} {c.bits}-bit {c.K}x{c.N} g{c.groupsize} M={m} {c.x_dtype}" + (" perm" if perm is not None else "")
        y = G.quant_matmul(x, qw, s, z, c.bits, c.groupsize, bias=b, out_dtype=torch.float32, perm=perm)
        assert_equal_bits(y, ref[:m].float(), tag + " fp32")
        y2 = G.quant_matmul(x, qw, s, z, c.bits, c.groupsize, bias=b, out_dtype=torch.float32, perm=perm)
        assert_equal_bits(y2, y, tag + " second call")
        yo = G.quant_matmul(x, qw, s, z, c.bits, c.groupsize, bias=b, perm=perm)
        assert yo.dtype == xdt
        assert_equal_bits(yo, ref[:m].float().to(xdt), tag + " rounded output")
        yn = G.quant_matmul(x, qw, s, z, c.bits, c.groupsize, bias=None, out_dtype=torch.float32, perm=perm)
        assert_equal_bits(yn, nobias[:m].float(), tag + " no bias")


def run_matvec_exact(Q, dev, c, entry, what=""):
    """One mat-vec entry point on row 0 of the case, `mul` preloaded with the dyadic bias.  entry: '3', '3faster', '4',
    '4h', 'grouped', 'groupedh' (h: fp16 x); a case with perm goes through the grouped entry's perm argument."""
    import torch
    qw, s, z, b, perm = dev_tensors(c, dev)
    half = entry in ("3faster", "4h", "groupedh")
    x = c.x[0].to(dev).to(torch.float16 if half else torch.float32)
    mul = b.clone()
    if entry == "3":
        Q.vecquant3matmul(x, qw, mul, s.reshape(-1, 1), z.reshape(-1, 1))
    elif entry == "3faster":
        Q.vecquant3matmul_faster(x, qw, mul, s.reshape(-1, 1), z.reshape(-1, 1))
    elif entry in ("4", "4h"):
        Q.vecquant4matmul(x, qw, mul, s.reshape(-1, 1), z.reshape(-1, 1))
    else:
        Q.vecquant_matmul_grouped(x, qw, mul, s, z, c.bits, c.groupsize, perm=perm)
    ref = torch.from_numpy(c.ref[0]).to(dev).float()
    assert_equal_bits(mul, ref, f"{what} mat-vec '{entry}' {c.bits}-bit {c.K}x{c.N} g{c.groupsize}"
                      + (" perm" if perm is not None else ""))


def matvec_entries(bits, groupsize):
    if groupsize > 0:
        return ("grouped", "groupedh")
    return ("3", "3faster") if bits == 3 else ("4", "4h")


def _exact_sweep(which):
    """Child-process entry: exact sweeps on whatever library GPTQ_HIP_LIB names, with the environment's kernel knobs."""
    import torch
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import gptq_amd
    from gptq_amd import quant_cuda
    dev = torch.device("cuda:0")
    n = 0
    if which == "gemm-perm":
        for bits in (3, 4):
            for K, N, gs, Ms, xd in SWEEP_GEMM_PERM:
                c = dyadic_case(bits, K, N, gs, max(Ms), perm=True, seed=17, x_dtype=xd)
                run_gemm_exact(gptq_amd, dev, c, Ms, "sweep")
                n += len(Ms)
    elif which == "matvec":
        for bits in (3, 4):
            for K, N, gs in SWEEP_MATVEC:
                for perm in ((False, True) if gs > 0 else (False,)):
                    c = dyadic_case(bits, K, N, gs, 1, perm=perm, seed=19, x_dtype=F16)
                    for entry in matvec_entries(bits, gs):
                        run_matvec_exact(quant_cuda, dev, c, entry, "sweep")
                        n += 1
    else:
        raise SystemExit(f"unknown sweep {which!r}")
    torch.cuda.synchronize()
    print(f"exact sweep {which}: {n} bit-equal")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--exact-sweep":
        _exact_sweep(sys.argv[2])
    else:
        raise SystemExit("usage: packed_ref.py --exact-sweep {gemm-perm|matvec}")
