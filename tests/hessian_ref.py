"""Reference side of the exact Hessian tests, independent of the code under test.

Nothing here calls gptq_amd to build an input or an expectation.  The operation is gptq.py:42-65 with a multi-sample batch,

    H[i, j] <- fl(fl(alpha * H[i, j]) + fl(beta * v[i, j]))   for i <= j,     v = sum over slabs of X^T X,
    alpha = float32(n / (n + b)),  beta = float32(2 / (n + b))                (n, b, n + b in fp64),

and every byte outside the upper triangle of the [C, C] window -- the strict lower triangle, the columns C..ldh-1 -- keeps
its bits (include/gptq_hip.h; the epilogues are written without contraction, csrc/gemm_f32.h and csrc/hessian.hip).

`exact_case` makes inputs for which v is EXACT in fp32 whatever the order of the adds and whatever the K split: X holds
multiples of 1/8 with |x| <= 4 (representable in fp16, bf16 and fp32), so every product and every partial sum is a multiple
of 1/64, and while  B = max_ij (sum_tokens |x_i||x_j| + |H0_ij|) * 64  stays below 2^24 no fp32 add of them rounds -- MFMA
accumulators, K-split partial tiles, the fixup's sum.  `exact_case` raises when B reaches 2^24.  With v exact the output
of every kernel path is determined and must equal `expected` bit for bit.  Two families of (n, b):

* single epilogue: any (n, b), e.g. n = 2, b = 1.  alpha and beta are not dyadic, so the two products and the add round,
  and ONE application of the epilogue defines the bits.  The library applies it once per launch: only for n_x <= 16 slabs
  (MAX_XLIST) on the batched kernels, and only for n_x = 1 on the per-slab kernels (ragged 16-bit, fp32).  `exact_case`
  refuses anything else.
* dyadic: n + b a power of two for every problem and H0 a multiple of 2^k'/64 where alpha = n'/2^k' in lowest terms:
  alpha * h, beta * v and their sum are exact too (the bound then also counts the output in units of beta/64), so the
  result does not depend on how the slabs are chunked.  Used wherever n_x > 16 or a per-slab kernel sees n_x > 1.

`kernel_path` and `big_plan` restate the documented dispatch and work-split rules of csrc/hessian.hip in plain Python.  They
only choose and label cases (tests/test_hessian_ref_cpu.py checks that the tables reach every branch); no expected value
depends on them.

The `--exact-sweep` entry point runs a short list of exact cases through the C ABI in a fresh process, for library builds
and settings that are read from the environment once per process.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TWO24 = float(2 ** 24)
X_DTYPES = ("f16", "bf16", "f32")
SENT32 = 0x7FC5A5A5                                          # a quiet-NaN bit pattern: H pad columns and guard rows
MAX_XLIST, MAX_PROB, BIG_MAXSEG = 16, 8, 4                   # documented constants of csrc/hessian.hip
# nsamples_before per problem for batch_total = 4: n + 4 = 4, 8, 16, ... (dyadic family)
DYADIC_B = 4
DYADIC_N = (0, 4, 12, 28, 60, 124, 252, 508, 1020, 2044)


def torch_dtype(name):
    import torch
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[name]


def _is_pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def _per_problem(v, n):
    return [int(v)] * n if np.isscalar(v) else [int(a) for a in v]


# ------------------------------------------------------------------------------------------------ dispatch, restated
def kernel_path(C, tokens, ldx, offset, dtype):
    """Which kernel the library documents for ONE problem shape outside the 256 x 256 path: 'f32' (hessian_kernel<float>),
    'dma' (hessian16_dma_kernel: 16-bit, C % 128 == 0, tokens % 64 == 0, ldx % 8 == 0, 16-byte aligned slabs) or 'ragged'
    (hessian16_kernel).  The suffix says whether the loads are vector loads."""
    if dtype == "f32":
        return "f32-vec" if (offset % 4 == 0 and ldx % 4 == 0) else "f32-scalar"
    aligned = offset % 8 == 0 and ldx % 8 == 0
    if aligned and C % 128 == 0 and tokens % 64 == 0:
        return "dma"
    return "ragged-vec" if aligned else "ragged-scalar"


def big_eligible(C, tokens, ldx, offset, dtype):
    """The 256 x 256 kernel's condition on one problem."""
    return dtype != "f32" and C % 256 == 0 and ldx % 8 == 0 and tokens % 64 == 0 and offset % 8 == 0


def big_tiles(C):
    return (C // 256) * (C // 256 + 1) // 2


def _cdiv(a, b):
    return -(-a // b)


def big_plan(total_tiles, n_cu, nk_all, split=True):
    """The work split of hessian_launch_big for one launch group: `total_tiles` 256 x 256 tiles, `nk_all` 32-token stages
    per tile, sized for `n_cu` compute units.  Whole rounds of n_cu tiles run whole-K; the left-over tiles are cut along K
    when the last round would run under 90 % full and a run still has 8 stages; `chunk` (stages per run) is rounded up to
    an even number; from 60 % of a round on, and while a tail run touches at most 4 tiles (cdiv(chunk, tail_len) + 1 <= 4),
    the layout is heads + tails instead of equal runs.  Returns a namespace with a `label`."""
    p = types.SimpleNamespace(total=total_tiles, n_cu=n_cu, nk_all=nk_all, full=total_tiles // n_cu * n_cu, split=False,
                              chunk=0, odd_rounded=False, workers=0, head=0, ntail=0, run_tiles=1)
    p.left = total_tiles - p.full
    if split and p.left > 0 and p.left * 10 < n_cu * 9 and p.left * nk_all >= 8 * n_cu:
        p.split = True
        chunk = _cdiv(p.left * nk_all, n_cu)
        p.odd_rounded = chunk % 2 == 1
        p.chunk = chunk + chunk % 2
        p.workers = _cdiv(p.left * nk_all, p.chunk)
        tail_len = nk_all - p.chunk
        seq, length = nk_all, p.left * nk_all                # the (tile, stage) sequence the runs cut
        if tail_len > 0 and _cdiv(p.chunk, tail_len) + 1 <= BIG_MAXSEG and p.left * 10 >= n_cu * 6:
            p.head = p.chunk
            p.ntail = _cdiv(p.left * tail_len, p.chunk)
            p.workers = p.left + p.ntail
            seq, length = tail_len, p.left * tail_len
        runs = p.ntail if p.head else p.workers
        p.run_tiles = max((min((w + 1) * p.chunk, length) - 1) // seq - (w * p.chunk) // seq + 1 for w in range(runs))
    if not p.split:
        p.label = f"{p.total} tiles on {n_cu} CUs: no split ({p.full} whole-K, {p.left} left whole-K)"
    elif p.head:
        p.label = (f"{p.total} tiles on {n_cu} CUs: {p.full} whole-K, {p.left} left, heads of {p.head} + {p.ntail} tail "
                   f"runs of {p.chunk} over up to {p.run_tiles} tiles")
    else:
        p.label = (f"{p.total} tiles on {n_cu} CUs: {p.full} whole-K, {p.left} left, {p.workers} equal runs of {p.chunk}"
                   + (" (odd chunk rounded up)" if p.odd_rounded else "") + f" over up to {p.run_tiles} tiles")
    return p


def big_plans(widths, tokens, n_x, n_cu, split=True):
    """The plans of every launch group of one call whose problems are all eligible: problems go out MAX_PROB per group,
    slabs MAX_XLIST per group."""
    out = []
    for p0 in range(0, len(widths), MAX_PROB):
        tiles = sum(big_tiles(c) for c in widths[p0:p0 + MAX_PROB])
        for i0 in range(0, n_x, MAX_XLIST):
            out.append(big_plan(tiles, n_cu, tokens // 32 * min(MAX_XLIST, n_x - i0), split))
    return out


# ------------------------------------------------------------------------------------------------ exact inputs
def _dyadic_h_unit(n, b):
    """alpha = n / (n + b) = n' / 2^k' in lowest terms -> H0 in multiples of 2^k' / 64 (alpha * h is then a multiple of
    1/64)."""
    tot = n + b
    assert _is_pow2(tot)
    g = int(np.gcd(n, tot)) if n else tot
    return (tot // g) / 64.0


def exact_case(C, tokens, n_x, n_prob=1, dtype="f16", nsamples_before=2, batch_total=1, seed=0, ldx_pad=0, ldh_pad=0,
               offset=0):
    """Exact inputs for one library call (module docstring).  C, nsamples_before, ldx_pad, ldh_pad and offset are one
    value or one per problem.  Returns a namespace: Cs, tokens, n_x, n_prob, dtype, nb, batch, ldx, ldh, offset (lists),
    family ('dyadic' or 'single'), Xs[p][i] (float32 [tokens, C], multiples of 1/8), H0[p] (float32 [C, C], filled
    everywhere), bound (B / 2^24, < 1) and x_range.

    X: integers k / 8 drawn per channel and per token, so a swapped, dropped or doubled row or column changes v; about
    1 % exact zeros; slab 0 has one all-zero token; one channel is all zero; the last channel holds only +-4 (except in
    the all-zero token).  H0: multiples of 1/64 (dyadic family: of 2^k'/64) in the lower triangle as well."""
    Cs = _per_problem(C, n_prob)
    nb = _per_problem(nsamples_before, n_prob)
    ldx = [c + v for c, v in zip(Cs, _per_problem(ldx_pad, n_prob))]
    ldh = [c + v for c, v in zip(Cs, _per_problem(ldh_pad, n_prob))]
    off = _per_problem(offset, n_prob)
    assert len(Cs) == len(nb) == n_prob and dtype in X_DTYPES and tokens > 0 and n_x > 0 and batch_total > 0
    c = types.SimpleNamespace(Cs=Cs, tokens=tokens, n_x=n_x, n_prob=n_prob, dtype=dtype, nb=nb, batch=batch_total,
                              ldx=ldx, ldh=ldh, offset=off, seed=seed)
    c.family = "dyadic" if all(_is_pow2(n + batch_total) for n in nb) else "single"
    if c.family == "single":
        if n_x > MAX_XLIST:
            raise ValueError(f"exact_case: {n_x} slabs go out in chunks of {MAX_XLIST}; a non-dyadic (n, b) = "
                             f"({nb}, {batch_total}) does not define the bits")
        per_slab = [kernel_path(Cs[p], tokens, ldx[p], off[p], dtype) != "dma" and
                    not big_eligible(Cs[p], tokens, ldx[p], off[p], dtype) for p in range(n_prob)]
        if n_x > 1 and any(per_slab):
            raise ValueError("exact_case: the per-slab kernels apply the epilogue once per slab; a non-dyadic (n, b) "
                             "with n_x > 1 does not define the bits")
    total_tokens = tokens * n_x
    if 16.0 * total_tokens * 64.0 >= TWO24 and max(Cs) >= 2:
        raise ValueError(f"exact_case: {total_tokens} tokens of a +-4 channel cannot stay exact (bound "
                         f"{16.0 * total_tokens * 64.0 / TWO24:.3g} x 2^24)")
    c.Xs, c.H0, bounds = [], [], []
    for p in range(n_prob):
        Cp = Cs[p]
        rng = np.random.default_rng([seed, p, Cp, tokens, n_x, nb[p], batch_total])
        unit = _dyadic_h_unit(nb[p], batch_total) if c.family == "dyadic" else 1.0 / 64.0
        H0 = (rng.integers(-16, 17, (Cp, Cp)) * unit).astype(np.float32)
        alpha, beta = nb[p] / (nb[p] + batch_total), 2.0 / (nb[p] + batch_total)
        xseed = int(rng.integers(0, 2 ** 31))
        ok = False
        for R in (32, 16, 8, 4, 2):
            r = np.random.default_rng(xseed)
            k = r.integers(-R, R + 1, (n_x, tokens, Cp))
            k[r.random(k.shape) < 0.01] = 0
            if Cp >= 2:
                k[:, :, Cp - 1] = 32 * (2 * r.integers(0, 2, (n_x, tokens)) - 1)       # only +-4
            if Cp >= 3:
                k[:, :, Cp // 2] = 0                                                   # an all-zero channel
            if tokens >= 2:
                k[0, tokens // 2, :] = 0                                               # an all-zero token
            xa = np.abs(k.reshape(-1, Cp)).astype(np.float64) / 8.0
            vabs = xa.T @ xa
            B = float((vabs * 64.0 + np.abs(H0.astype(np.float64)) * 64.0).max())
            if c.family == "dyadic":                          # the output, in units of min(1, beta) / 64, must fit too
                out_lsb = min(1.0, beta) / 64.0
                B = max(B, float((alpha * np.abs(H0.astype(np.float64)) + beta * vabs).max()) / out_lsb)
            if B < TWO24:
                ok = True
                break
        if not ok:
            raise ValueError(f"exact_case: C={Cp} tokens={tokens} n_x={n_x} (n, b)=({nb[p]}, {batch_total}) cannot stay "
                             f"exact: bound {B / TWO24:.3g} x 2^24 at |x| <= 1/4")
        c.x_range = R
        c.Xs.append([(k[i] / 8.0).astype(np.float32) for i in range(n_x)])
        c.H0.append(H0)
        bounds.append(B / TWO24)
    c.bound = max(bounds)
    return c


def pad_h(H0, ldh):
    """[C, C] -> [C, ldh] with the sentinel bit pattern in the pad columns."""
    C = H0.shape[0]
    out = np.full((C, ldh), SENT32, dtype=np.uint32).view(np.float32)
    out[:, :C] = H0
    return out


def expected(H0, Xs, nsamples_before, batch_total):
    """The documented result of ONE update.  H0: float32 [C, ldh] (ldh >= C; whatever sits right of column C is carried
    over), Xs: the slabs [tokens, C].  v in fp64 (asserted to round-trip through fp32), then the epilogue in numpy
    float32 on the upper triangle; everything else keeps H0's bits."""
    H0 = np.ascontiguousarray(H0, dtype=np.float32)
    C = H0.shape[0]
    v = np.zeros((C, C))
    for x in Xs:
        x = np.asarray(x, dtype=np.float64)
        assert x.shape[1] == C
        v += x.T @ x
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v), "X^T X is not exact in fp32: not an exact case"
    n_after = float(nsamples_before) + float(batch_total)
    alpha = np.float32(float(nsamples_before) / n_after)
    beta = np.float32(2.0 / n_after)
    h = H0[:, :C]
    upd = (alpha * h).astype(np.float32) + (beta * v32).astype(np.float32)
    assert upd.dtype == np.float32
    out = H0.copy()
    up = np.triu(np.ones((C, C), dtype=bool))
    out[:, :C][up] = upd[up]
    return out


def expected_case(c):
    """Per problem: expected [C, ldh] of the whole call (pad columns = sentinel)."""
    return [expected(pad_h(c.H0[p], c.ldh[p]), c.Xs[p], c.nb[p], c.batch) for p in range(c.n_prob)]


# ------------------------------------------------------------------------------------------------ exact-case tables
F16, BF16, F32 = "f16", "bf16", "f32"
SINGLE = dict(nsamples_before=2, batch_total=1)              # alpha = 2/3, beta = 2/3: both round
# Ragged and scalar paths, every row with every dtype: (C, tokens, ldx pad, base offset in elements, ldh pad, n_x).
# n_x > 1 rows are dyadic (per-slab epilogues).  Corners: C = 1 with tokens = 1; tokens = 1 at a full tile; C = 129 with
# tokens = 65 and an odd ldx (129 and 137), scalar and misaligned.
RAGGED = [
    (1, 1, 0, 0, 0, 1), (1, 129, 1, 1, 1, 2), (7, 15, 3, 4, 5, 1), (8, 64, 0, 8, 0, 1), (8, 63, 8, 0, 1, 3),
    (64, 100, 8, 0, 5, 1), (127, 65, 1, 1, 0, 1), (128, 1, 0, 4, 1, 1), (128, 15, 8, 8, 5, 2), (129, 65, 0, 1, 5, 1),
    (129, 65, 8, 0, 1, 1), (130, 63, 3, 4, 0, 1), (200, 129, 0, 0, 1, 1), (200, 64, 8, 8, 5, 2), (257, 100, 1, 0, 0, 1),
    (257, 64, 3, 4, 5, 1), (320, 129, 0, 0, 0, 1), (320, 64, 8, 1, 1, 1), (320, 15, 1, 8, 5, 2),
]
# Aligned 128 x 128 path, fp16 and bf16: (C, tokens, n_x, n_prob, ldx pad (% 8 == 0), ldh pad, family).  The last row is
# the same shape as the second-last at tokens = 96: it must fall to the ragged kernel.
ALIGNED = [
    (128, 64, 1, 1, 8, 1, "single"), (128, 192, 3, 3, 0, 0, "single"), (384, 64, 16, 8, 8, 5, "single"),
    (384, 192, 17, 1, 16, 3, "dyadic"), (384, 64, 33, 9, 8, 1, "dyadic"), (1024, 2048, 1, 1, 8, 8, "single"),
    (1024, 64, 3, 9, 0, 4, "single"), (1024, 192, 16, 3, 8, 0, "single"), (128, 2048, 3, 8, 24, 7, "dyadic"),
    (384, 192, 3, 3, 8, 5, "dyadic"), (384, 96, 3, 3, 8, 5, "dyadic"),
]
# 256 x 256 path through gptq_hessian_accum_mixed in the default environment (>= 100 eligible tiles in the call):
# name -> (widths, tokens, n_x, dtype, n_cu, family, branch this row is in the table for at that n_cu)
W105 = [1280] * 7                                            # 7 x 15 = 105 tiles; 256 tokens x 3 slabs = 24 stages
BIG = {
    "nosplit-cu35": (W105, 256, 3, F16, 35, "single", "no-split"),
    "equal-cu24": (W105, 256, 3, F16, 24, "single", "equal-cross-odd"),
    "heads2-cu29": (W105, 256, 3, F16, 29, "single", "heads-2"),
    "heads3-cu29": (W105, 448, 1, F16, 29, "single", "heads-3"),      # 14 stages: tails of 4 under runs of 10
    "widths-nx17": ([2304, 1280, 768, 1280, 512, 1280, 256], 64, 17, BF16, 0, "dyadic", "slabs>16"),
    "prob10-cu24": ([1280, 256, 1280, 1280, 256, 1280, 1280, 1280, 256, 1280], 256, 3, F16, 24, "single", "problems>8"),
    "device": (W105, 256, 3, F16, 0, "single", "device"),
}
# (n, b) per family
def family_args(family, n_prob, n_x):
    if family == "dyadic":
        return dict(nsamples_before=[DYADIC_N[p % len(DYADIC_N)] for p in range(n_prob)], batch_total=DYADIC_B)
    return dict(nsamples_before=[2 + p for p in range(n_prob)], batch_total=n_x)     # a different alpha per problem


def ragged_case(row, dtype, seed=1):
    C, tokens, ldx_pad, off, ldh_pad, n_x = row
    kw = family_args("dyadic", 1, n_x) if n_x > 1 else SINGLE
    return exact_case(C, tokens, n_x, 1, dtype, seed=seed, ldx_pad=ldx_pad, ldh_pad=ldh_pad, offset=off, **kw)


def aligned_case(row, dtype, seed=2):
    C, tokens, n_x, n_prob, ldx_pad, ldh_pad, family = row
    return exact_case(C, tokens, n_x, n_prob, dtype, seed=seed, ldx_pad=ldx_pad, ldh_pad=ldh_pad,
                      **family_args(family, n_prob, n_x))


def big_case(name, seed=3):
    widths, tokens, n_x, dtype, n_cu, family, _ = BIG[name]
    n = len(widths)
    # a different ldx / ldh pad per problem (ldx stays a multiple of 8)
    return exact_case(widths, tokens, n_x, n, dtype, seed=seed, ldx_pad=[8 * (p % 3) for p in range(n)],
                      ldh_pad=[(0, 1, 5, 8)[p % 4] for p in range(n)], **family_args(family, n, n_x))


def mixed_rest_case(seed=4):
    """105 eligible tiles plus problems the 256 x 256 kernel refuses: three of C = 320 (two share (C, ldx, ldh), one has
    another ldh: two `rest` groups), and one of C = 256 whose slabs sit 2 elements off a 16-byte boundary."""
    widths = [1280, 320, 1280, 1280, 256, 320, 1280, 1280, 320, 1280, 1280]
    n = len(widths)
    ldx_pad = [8 if w == 320 else 0 for w in widths]
    ldh_pad = [0] * n
    ldh_pad[8] = 3
    offset = [2 if w == 256 else 0 for w in widths]
    return exact_case(widths, 64, 2, n, F16, seed=seed, ldx_pad=ldx_pad, ldh_pad=ldh_pad, offset=offset,
                      **family_args("dyadic", n, 2))


def ragged_id(row):
    return "C{}-t{}-ldx+{}-off{}-ldh+{}-nx{}".format(*row)


def aligned_id(row):
    return "C{}-t{}-nx{}-p{}-{}".format(row[0], row[1], row[2], row[3], row[6])


# ------------------------------------------------------------------------------------------------ GPU side
def bits_equal(a, b):
    """Same shape and the same 32-bit patterns (NaN sentinels and -0.0 compared as bits)."""
    import torch
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def device_slab(x, dtype, ldx, offset, dev, guard=2):
    """One slab on the device: [tokens, C] inside an allocation of (tokens + guard) rows of ldx elements that starts
    `offset` elements after a 16-byte boundary; pad channels and guard rows hold NaN, so a read outside the [tokens, C]
    window that stays inside the allocation poisons H.  Returns (view [tokens, C], keep-alive)."""
    import torch
    tokens, C = x.shape
    tdt = torch_dtype(dtype)
    n = (tokens + guard) * ldx
    flat = torch.full((n + offset + 16,), float("nan"), dtype=tdt, device=dev)
    assert flat.data_ptr() % 16 == 0
    body = flat[offset:offset + n].view(tokens + guard, ldx)
    body[:tokens, :C] = torch.from_numpy(x).to(dev).to(tdt)
    view = body[:tokens, :C]
    assert view.data_ptr() % 16 == (offset * flat.element_size()) % 16 and view.stride(0) == ldx
    return view, flat


def device_h(H0, ldh, dev):
    """H on the device: rows 1..C of a [C + 2, ldh] buffer whose pad columns and two guard rows hold the sentinel."""
    import torch
    C = H0.shape[0]
    full = np.full((C + 2, ldh), SENT32, dtype=np.uint32).view(np.float32)
    full[1:C + 1] = pad_h(H0, ldh)
    buf = torch.from_numpy(full).to(dev)
    return buf[1:C + 1], buf


def expected_buffer(exp, ldh):
    C = exp.shape[0]
    full = np.full((C + 2, ldh), SENT32, dtype=np.uint32).view(np.float32)
    full[1:C + 1] = exp
    return full


def upload(c, dev):
    """Device operands of a case: c.dX[p][i] views, c.dH[p] views, c.dHbuf[p] whole buffers."""
    c.dX, c.dH, c.dHbuf, c._keep = [], [], [], []
    for p in range(c.n_prob):
        xs = []
        for i in range(c.n_x):
            v, keep = device_slab(c.Xs[p][i], c.dtype, c.ldx[p], c.offset[p], dev)
            xs.append(v)
            c._keep.append(keep)
        c.dX.append(xs)
        h, buf = device_h(c.H0[p], c.ldh[p], dev)
        c.dH.append(h)
        c.dHbuf.append(buf)
    return c


def reset_h(c, dev):
    import torch
    for p in range(c.n_prob):
        c.dHbuf[p].copy_(torch.from_numpy(expected_buffer(pad_h(c.H0[p], c.ldh[p]), c.ldh[p])).to(dev))


def _arrays(c):
    import ctypes
    n = c.n_prob
    Hp = (ctypes.c_void_p * n)(*[h.data_ptr() for h in c.dH])
    Xp = (ctypes.c_void_p * (n * c.n_x))(*[x.data_ptr() for xs in c.dX for x in xs])
    ints = lambda v: (ctypes.c_int * n)(*v)
    return Hp, Xp, ints


def call_mixed(c, dev, n_cu=0):
    import torch
    from gptq_amd import _lib
    code = {"f32": _lib.F32, "f16": _lib.F16, "bf16": _lib.BF16}[c.dtype]
    Hp, Xp, ints = _arrays(c)
    with torch.cuda.device(dev):
        _lib.call("gptq_hessian_accum_mixed", c.n_prob, Hp, ints(c.ldh), Xp, c.n_x, code, ints(c.ldx), ints(c.Cs),
                  c.tokens, ints(c.nb), c.batch, n_cu, _lib.stream(dev))
    torch.cuda.synchronize()


def call_group(c, dev):
    """gptq_hessian_accum_group (one problem with one slab: gptq_hessian_accum): all problems share C, ldx, ldh."""
    import torch
    from gptq_amd import _lib
    assert len(set(c.Cs)) == len(set(c.ldx)) == len(set(c.ldh)) == 1
    code = {"f32": _lib.F32, "f16": _lib.F16, "bf16": _lib.BF16}[c.dtype]
    Hp, Xp, ints = _arrays(c)
    with torch.cuda.device(dev):
        if c.n_prob == 1 and c.n_x == 1:
            _lib.call("gptq_hessian_accum", c.dH[0].data_ptr(), c.ldh[0], c.dX[0][0].data_ptr(), code, c.ldx[0], c.Cs[0],
                      c.tokens, c.nb[0], c.batch, _lib.stream(dev))
        else:
            _lib.call("gptq_hessian_accum_group", c.n_prob, Hp, c.ldh[0], Xp, c.n_x, code, c.ldx[0], c.Cs[0], c.tokens,
                      ints(c.nb), c.batch, _lib.stream(dev))
    torch.cuda.synchronize()


def assert_case_exact(c, what, want=None):
    """Every H buffer of the case (guard rows, pad columns and lower triangle included) == the expectation, as bits."""
    import torch
    want = expected_case(c) if want is None else want
    for p in range(c.n_prob):
        got = c.dHbuf[p].cpu()
        exp = torch.from_numpy(expected_buffer(want[p], c.ldh[p]))
        if bits_equal(got, exp):
            continue
        g, w = got.numpy().view(np.int32), exp.numpy().view(np.int32)
        bad = np.argwhere(g != w)
        r, col = int(bad[0][0]) - 1, int(bad[0][1])
        C = c.Cs[p]
        where = ("a guard row" if r < 0 or r >= C else "a pad column" if col >= C else
                 "the strict lower triangle" if r > col else "the upper triangle")
        raise AssertionError(
            f"{what}: problem {p} (C={C}, ldx={c.ldx[p]}, ldh={c.ldh[p]}, n={c.nb[p]}, b={c.batch}, {c.family}): {len(bad)} "
            f"of {g.size} words differ from the exact reference; first at row {r}, column {col} in {where} (256-tile "
            f"({r // 256}, {col // 256}), 128-tile ({r // 128}, {col // 128})): got {got.numpy()[r + 1, col]!r} "
            f"(0x{int(g[r + 1, col]) & 0xFFFFFFFF:08x}), want {exp.numpy()[r + 1, col]!r} "
            f"(0x{int(w[r + 1, col]) & 0xFFFFFFFF:08x}); rows {sorted(set(int(b[0]) - 1 for b in bad))[:8]} ...")
    return want


# cases of the child-process sweep: name -> builder.  Under GPTQ_HESS_BIG=2 / 3 every eligible one takes the 256 x 256
# kernel (with / without the K split), under 0 none does.
def _sweep_cases():
    return [
        ("C512-t64-nx5-p3-f16", lambda: exact_case(512, 64, 5, 3, F16, seed=11, ldx_pad=8, ldh_pad=3,
                                                    **family_args("single", 3, 5))),
        ("C1280x7-t256-nx3-f16", lambda: big_case("device", seed=12)),
        ("C3072-t128-nx1-p2-bf16", lambda: exact_case(3072, 128, 1, 2, BF16, seed=13, ldh_pad=[0, 8],
                                                       **family_args("single", 2, 1))),
        ("widths-nx17-bf16", lambda: big_case("widths-nx17", seed=14)),
        ("mixed-with-rest-f16", lambda: mixed_rest_case(seed=15)),
        ("C1024-t96-nx3-p2-f16", lambda: exact_case(1024, 96, 3, 2, F16, seed=16, **family_args("dyadic", 2, 3))),
        ("prob10-f16", lambda: big_case("prob10-cu24", seed=17)),
    ]


def _exact_sweep(n_cu):
    """Child-process entry: the sweep on whatever library GPTQ_HIP_LIB names, with the environment's kernel knobs.  Stops
    at the first mismatch."""
    import torch
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    dev = torch.device("cuda:0")
    for name, make in _sweep_cases():
        c = upload(make(), dev)
        call_mixed(c, dev, n_cu)
        try:
            assert_case_exact(c, f"sweep {name} n_cu={n_cu}")
        except AssertionError as e:
            print(f"exact: {name} MISMATCH\n{e}", flush=True)
            raise SystemExit(1)
        print(f"exact: {name} OK", flush=True)
        del c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--exact-sweep":
        budget = int(sys.argv[sys.argv.index("--n-cu") + 1]) if "--n-cu" in sys.argv else 0
        _exact_sweep(budget)
    else:
        raise SystemExit("usage: hessian_ref.py --exact-sweep [--n-cu N]")
