"""The checkpoint layout of the other GPTQ tools, written from its definition in numpy, independent of the kernels.

One Linear with K inputs, N outputs, `bits` in {2, 3, 4, 8} and G groups (group_size -1: G = 1), K % 32 == N % 32 == 0:

  qweight int32 [K/32*bits, N]  codes in ORIGINAL input order; code i of a 32-code group at bit bits*i of the group's
                                little-endian stream of `bits` words
  g_idx   int32 [K]             the group of every original input column
  scales  fp16  [G, N]
  qzeros  int32 [G, N/32*bits]  stored value v of column n at bit bits*(n % 32) of the stream of `bits` words starting at
                                word (n / 32)*bits;  'gptq': v = z - 1,  'gptq_v2': v = z  (z the integer zero point)
  bias    fp16  [N]             only where the Linear has one
  W[n][k] = scales[g_idx[k]][n] * (code[k][n] - z[g_idx[k]][n])

The packers below use the LOOP form -- per output word, OR the codes in at their shifts, the three words of the 3-bit
case written out -- not the bit-stream form (bit = bits*j, word = bit / 32, ...) the kernels use.  On import under 'gptq'
the zero point is v + 1 WITHOUT masking (a stored 2^bits - 1 gives 2^bits).
"""
from __future__ import annotations

import numpy as np

BITS = (2, 3, 4, 8)
ZERO_OFFSET = {"gptq": 1, "gptq_v2": 0}
M32 = np.uint64(0xFFFFFFFF)


def _u(x):
    return np.uint64(x)


def pack_rows(codes, bits):
    """codes [K, ...] (0 .. 2^bits - 1) -> int32 [K/32*bits, ...], packed along axis 0."""
    codes = np.asarray(codes)
    K = codes.shape[0]
    assert K % 32 == 0 and bits in BITS and int(codes.max(initial=0)) < 2 ** bits and int(codes.min(initial=0)) >= 0
    c = codes.reshape((K // 32, 32) + codes.shape[1:]).astype(np.uint64)
    words = np.zeros((K // 32, bits) + codes.shape[1:], dtype=np.uint64)
    if bits == 3:
        for j in range(10):
            words[:, 0] |= c[:, j] << _u(3 * j)
        words[:, 0] |= (c[:, 10] << _u(30)) & M32                # the low two bits of code 10 ...
        words[:, 1] |= c[:, 10] >> _u(2)                         # ... and its high bit
        for j in range(10):
            words[:, 1] |= c[:, 11 + j] << _u(3 * j + 1)
        words[:, 1] |= (c[:, 21] << _u(31)) & M32                # the low bit of code 21 ...
        words[:, 2] |= c[:, 21] >> _u(1)                         # ... and its high two bits
        for j in range(10):
            words[:, 2] |= c[:, 22 + j] << _u(3 * j + 2)
    else:
        per_word = 32 // bits
        for k in range(bits):
            for j in range(per_word):
                words[:, k] |= c[:, per_word * k + j] << _u(bits * j)
    assert int(words.max(initial=0)) <= 0xFFFFFFFF
    return words.reshape((K // 32 * bits,) + codes.shape[1:]).astype(np.uint32).view(np.int32)


def unpack_rows(q, bits):
    """int32 [K/32*bits, ...] -> uint8 codes [K, ...]."""
    q = np.ascontiguousarray(q).view(np.uint32).astype(np.uint64)
    assert q.shape[0] % bits == 0
    G = q.shape[0] // bits
    w = q.reshape((G, bits) + q.shape[1:])
    codes = np.zeros((G, 32) + q.shape[1:], dtype=np.uint64)
    if bits == 3:
        for j in range(10):
            codes[:, j] = (w[:, 0] >> _u(3 * j)) & _u(7)
        codes[:, 10] = (w[:, 0] >> _u(30)) | ((w[:, 1] & _u(1)) << _u(2))
        for j in range(10):
            codes[:, 11 + j] = (w[:, 1] >> _u(3 * j + 1)) & _u(7)
        codes[:, 21] = (w[:, 1] >> _u(31)) | ((w[:, 2] & _u(3)) << _u(1))
        for j in range(10):
            codes[:, 22 + j] = (w[:, 2] >> _u(3 * j + 2)) & _u(7)
    else:
        per_word = 32 // bits
        for k in range(bits):
            for j in range(per_word):
                codes[:, per_word * k + j] = (w[:, k] >> _u(bits * j)) & _u(2 ** bits - 1)
    return codes.reshape((G * 32,) + q.shape[1:]).astype(np.uint8)


def pack_qzeros(stored, bits):
    """stored values [G, N] -> int32 [G, N/32*bits], packed along N."""
    return np.ascontiguousarray(pack_rows(np.asarray(stored).T, bits).T)


def unpack_qzeros(qzeros, bits):
    """int32 [G, N/32*bits] -> stored values [G, N] (int64)."""
    return np.ascontiguousarray(unpack_rows(np.ascontiguousarray(np.asarray(qzeros).T), bits).T).astype(np.int64)


def zero_points(qzeros, bits, checkpoint_format):
    """The integer zero points a reader of the format uses: stored + offset, not masked."""
    return unpack_qzeros(qzeros, bits) + ZERO_OFFSET[checkpoint_format]


def g_idx_of(K, group_size, perm=None):
    """The group of every original column: k // group_size, or with act-order g_idx[perm[j]] = j // group_size."""
    grp = (np.arange(K) // group_size if group_size > 0 else np.zeros(K, dtype=np.int64)).astype(np.int32)
    if perm is None:
        return grp
    g = np.empty(K, dtype=np.int32)
    g[np.asarray(perm)] = grp
    return g


def perm_of(g_idx):
    """The storage order of an act-order import: a stable argsort of g_idx."""
    return np.argsort(np.asarray(g_idx), kind="stable").astype(np.int32)


def dense_weight(t, bits, checkpoint_format):
    """W [N, K] fp32 from the foreign tensors `t` (numpy): scales[g_idx[k]][n] * (code[k][n] - z[g_idx[k]][n])."""
    codes = unpack_rows(t["qweight"], bits).astype(np.int64)                        # [K, N]
    K = codes.shape[0]
    g = np.asarray(t["g_idx"]).astype(np.int64) if t.get("g_idx") is not None else np.zeros(K, dtype=np.int64)
    z = zero_points(t["qzeros"], bits, checkpoint_format)
    s = np.asarray(t["scales"]).astype(np.float32)
    return np.ascontiguousarray((s[g] * (codes - z[g]).astype(np.float32)).T)


def foreign_tensors(codes_orig, scales16, zint, g_idx, bits, checkpoint_format, bias=None):
    """The tensors of the format from their meaning: codes [K, N] in original order, fp16 scales and integer zero points
    [G, N], g_idx [K], bias [N] or None."""
    off = ZERO_OFFSET[checkpoint_format]
    stored = np.asarray(zint).astype(np.int64) - off
    assert stored.min() >= 0 and stored.max() < 2 ** bits
    t = {"qweight": pack_rows(codes_orig, bits), "qzeros": pack_qzeros(stored, bits),
         "scales": np.asarray(scales16, dtype=np.float16), "g_idx": np.asarray(g_idx, dtype=np.int32)}
    if bias is not None:
        t["bias"] = np.asarray(bias, dtype=np.float16)
    return t


def own_to_foreign(codes_storage, scales, zint, group_size, bits, checkpoint_format, perm=None, bias=None):
    """What exporting a packed module must give: its codes [K, N] in STORAGE order (row j = input column perm[j]), its
    fp32 scales and integer zero points [G, N]."""
    codes_storage = np.asarray(codes_storage)
    K = codes_storage.shape[0]
    orig = codes_storage
    if perm is not None:
        orig = np.empty_like(codes_storage)
        orig[np.asarray(perm)] = codes_storage
    b = None if bias is None or not np.any(np.asarray(bias) != 0) else bias
    return foreign_tensors(orig, np.asarray(scales).astype(np.float16), zint, g_idx_of(K, group_size, perm), bits,
                           checkpoint_format, b)
