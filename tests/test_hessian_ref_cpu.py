"""tests/hessian_ref.py on the CPU: every table row builds and is exact, `expected` agrees with the oracle on the formula,
and the case tables reach every branch of the documented dispatch and work split (checked with `big_plan`)."""
import numpy as np
import pytest
import torch

import hessian_ref as R
from oracle import gptq_oracle as O


def _check_exact(c):
    assert c.bound < 1.0
    for p in range(c.n_prob):
        X = np.concatenate(c.Xs[p], 0).astype(np.float64)
        assert np.array_equal(X * 8, np.round(X * 8)) and np.abs(X).max() <= 4.0
        for dt in R.X_DTYPES:                                # representable in every input type
            t = torch.from_numpy(np.concatenate(c.Xs[p], 0))
            assert torch.equal(t.to(R.torch_dtype(dt)).float(), t)
        v = X.T @ X
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)          # fp64 reference round-trips
        assert float(((np.abs(X).T @ np.abs(X)) * 64 + np.abs(c.H0[p]) * 64.0).max()) < R.TWO24
        assert np.array_equal(c.H0[p] * 64, np.round(c.H0[p].astype(np.float64) * 64))
        assert (np.tril(c.H0[p], -1) != 0).any() or c.Cs[p] < 4                    # the lower triangle is filled
        C = c.Cs[p]
        if C >= 2 and c.tokens >= 2:
            assert set(np.abs(np.delete(X[:, C - 1], c.tokens // 2))) == {4.0}
            assert not X[c.tokens // 2].any()
        if C >= 3:
            assert not X[:, C // 2].any()
    want = R.expected_case(c)
    for p in range(c.n_prob):
        C = c.Cs[p]
        H0 = R.pad_h(c.H0[p], c.ldh[p])
        low = np.tril(np.ones((C, C), dtype=bool), -1)
        assert np.array_equal(want[p][:, :C][low].view(np.int32), H0[:, :C][low].view(np.int32))
        assert np.array_equal(want[p][:, C:].view(np.int32), H0[:, C:].view(np.int32))
        if c.family == "dyadic":                             # chunk by chunk (alpha = 1 after the first) gives the same bits
            v = sum(x.astype(np.float64).T @ x.astype(np.float64) for x in c.Xs[p])
            n, b = c.nb[p], c.batch
            exact = (n / (n + b)) * c.H0[p].astype(np.float64) + (2.0 / (n + b)) * v
            assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
            up = np.triu(np.ones((C, C), dtype=bool))
            assert np.array_equal(want[p][:, :C][up].astype(np.float64), exact[up])
    return want


@pytest.mark.parametrize("dtype", R.X_DTYPES)
def test_ragged_table_builds_and_is_exact(dtype):
    for row in R.RAGGED:
        c = R.ragged_case(row, dtype)
        _check_exact(c)
        path = R.kernel_path(c.Cs[0], c.tokens, c.ldx[0], c.offset[0], dtype)
        assert path != "dma", row                            # this table is for the ragged / fp32 kernels


def test_ragged_table_covers_every_axis_value_and_both_load_kinds():
    cols = list(zip(*R.RAGGED))
    assert set(cols[0]) == {1, 7, 8, 64, 127, 128, 129, 130, 200, 257, 320}
    assert set(cols[1]) == {1, 15, 63, 64, 65, 100, 129}
    assert set(cols[2]) == {0, 1, 3, 8} and set(cols[3]) == {0, 1, 4, 8} and set(cols[4]) == {0, 1, 5}
    assert (1, 1) in {(r[0], r[1]) for r in R.RAGGED}
    assert any(r[0] == 129 and r[1] == 65 and (r[0] + r[2]) % 2 == 1 and r[3] % 8 != 0 for r in R.RAGGED)
    for dt in R.X_DTYPES:
        paths = {R.kernel_path(r[0], r[1], r[0] + r[2], r[3], dt) for r in R.RAGGED}
        assert paths == ({"f32-vec", "f32-scalar"} if dt == "f32" else {"ragged-vec", "ragged-scalar"}), paths


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_aligned_table_builds_and_is_exact(dtype):
    for row in R.ALIGNED:
        c = R.aligned_case(row, dtype)
        assert c.family == row[6]
        _check_exact(c)
        assert len(set(c.nb)) == c.n_prob                    # a different nsamples_before per problem
        for p in range(c.n_prob):
            path = R.kernel_path(c.Cs[p], c.tokens, c.ldx[p], c.offset[p], dtype)
            assert path == ("ragged-vec" if c.tokens == 96 else "dma"), row
        # in the default environment the 256 x 256 kernel must not take these (fewer than 100 eligible tiles)
        tiles = sum(R.big_tiles(C) for C in c.Cs if R.big_eligible(C, c.tokens, c.ldx[0], 0, dtype))
        assert tiles < 100, row
    cols = list(zip(*R.ALIGNED))
    assert set(cols[0]) == {128, 384, 1024} and set(cols[1]) == {64, 96, 192, 2048}
    assert set(cols[2]) == {1, 3, 16, 17, 33} and set(cols[3]) == {1, 3, 8, 9}
    assert all(r[4] % 8 == 0 for r in R.ALIGNED) and any(r[4] > 0 and r[5] > 0 for r in R.ALIGNED)


def test_big_tables_build_and_are_exact():
    for name in R.BIG:
        c = R.big_case(name)
        _check_exact(c)
        assert all(R.big_eligible(c.Cs[p], c.tokens, c.ldx[p], c.offset[p], c.dtype) for p in range(c.n_prob)), name
        assert sum(R.big_tiles(C) for C in c.Cs) >= 100, name
    c = R.mixed_rest_case()
    _check_exact(c)
    elig = [R.big_eligible(c.Cs[p], c.tokens, c.ldx[p], c.offset[p], c.dtype) for p in range(c.n_prob)]
    assert sum(R.big_tiles(C) for C, e in zip(c.Cs, elig) if e) >= 100
    rest = {(c.Cs[p], c.ldx[p], c.ldh[p]) for p in range(c.n_prob) if not elig[p]}
    assert len(rest) == 3 and sum(not e for e in elig) == 4   # two C = 320 problems share a group
    assert any(c.Cs[p] == 256 and c.offset[p] % 8 != 0 for p in range(c.n_prob))
    for _, make in R._sweep_cases():
        _check_exact(make())


def test_hand_derived_plans():
    """The two starting points derived by hand from hessian_launch_big: 105 tiles (7 problems of C = 1280), 24 stages
    (256 tokens x 3 slabs)."""
    p = R.big_plan(105, 24, 24)
    assert (p.full, p.left, p.split, p.chunk, p.odd_rounded, p.head, p.workers) == (96, 9, True, 10, True, 0, 22)
    p = R.big_plan(105, 29, 24)
    assert (p.full, p.left, p.split, p.chunk, p.head, p.ntail, p.workers) == (87, 18, True, 16, 16, 9, 27)
    assert not R.big_plan(105, 29, 24, split=False).split


def test_plan_coverage():
    """Every branch of the work split is reached by a row of the 256 x 256 table at the budget it names, and the
    device-sized rows reach a split round at n_cu = 256."""
    seen = set()
    for name, (widths, tokens, n_x, dtype, n_cu, family, branch) in R.BIG.items():
        plans = R.big_plans(widths, tokens, n_x, n_cu or 256)
        if len(widths) > R.MAX_PROB:
            assert len(plans) >= 2
            seen.add("problems>8")
        if n_x > R.MAX_XLIST:
            assert len(plans) >= 2 and family == "dyadic"
            seen.add("slabs>16")
        for p in plans:
            if not p.split:
                seen.add("no-split")
            elif p.head == 0:
                if p.run_tiles >= 2:
                    seen.add("equal-cross")
                if p.odd_rounded:
                    seen.add("odd-chunk")
            else:
                seen.add("heads-2" if p.run_tiles == 2 else "heads-3" if p.run_tiles >= 3 else "heads-1")
                assert p.run_tiles <= R.BIG_MAXSEG
            if p.split:
                assert p.chunk % 2 == 0 and p.chunk <= p.nk_all
        got = {"equal-cross-odd": {"equal-cross", "odd-chunk"}, "device": set()}.get(branch, {branch})
        assert got <= seen, (name, branch, seen)
    assert {"no-split", "equal-cross", "odd-chunk", "heads-2", "heads-3", "problems>8", "slabs>16"} <= seen, seen
    w, t, nx = R.BIG["device"][:3]
    assert all(p.split for p in R.big_plans(w, t, nx, 256))


def test_expected_agrees_with_the_oracle_on_the_formula():
    """hessian_add_batch scales X by sqrt(2 / n) before the product and rounds in another order: a loose bar."""
    for (n, b, C, tokens, dtype) in [(2, 1, 37, 50, "f32"), (0, 4, 64, 33, "f32"), (5, 3, 130, 64, "f16"),
                                     (2, 3, 128, 64, "bf16")]:
        c = R.exact_case(C, tokens, b, 1, dtype, nsamples_before=n, batch_total=b, seed=5)     # one slab per sample
        want = R.expected(c.H0[0], c.Xs[0], n, b)
        H = torch.from_numpy(c.H0[0].copy())
        assert O.hessian_add_batch(H, n, torch.from_numpy(np.stack(c.Xs[0]))) == n + b
        up = np.triu(np.ones((C, C), dtype=bool))
        err = np.abs(H.numpy().astype(np.float64) - want)[up].max() / np.abs(want[up]).max()
        assert err < 1e-5, (n, b, err)
        assert np.array_equal(want[~up], c.H0[0][~up])


def test_exact_case_refuses_what_cannot_be_exact():
    with pytest.raises(ValueError, match="cannot stay exact"):
        R.exact_case(128, 2048, 16, 1, "f16", **R.family_args("dyadic", 1, 16))       # 32768 tokens of +-4
    with pytest.raises(ValueError, match="chunks of 16"):
        R.exact_case(128, 64, 17, 1, "f16", nsamples_before=2, batch_total=1)           # non-dyadic over two chunks
    with pytest.raises(ValueError, match="per-slab"):
        R.exact_case(130, 64, 2, 1, "f16", nsamples_before=2, batch_total=1)            # ragged kernel, one epilogue per slab
    with pytest.raises(ValueError, match="cannot stay exact"):
        R.exact_case(64, 64, 1, 1, "f16", nsamples_before=2 ** 22 - 4, batch_total=4)   # dyadic output below 2^-24 units
    with pytest.raises(AssertionError, match="not exact"):
        R.expected(np.zeros((2, 2), np.float32), [np.full((3, 2), 4097.0)], 0, 1)       # 3 * 4097^2 needs 26 bits


def test_bits_equal_sees_nan_payloads_and_signed_zero():
    a = torch.tensor([0.0, 1.0, float("nan")])
    b = a.clone()
    assert R.bits_equal(a, b)
    b[0] = -0.0
    assert not R.bits_equal(a, b)
    s = torch.from_numpy(np.array([R.SENT32, R.SENT32 ^ 1], dtype=np.uint32).view(np.float32))
    assert not R.bits_equal(s[:1], s[1:]) and R.bits_equal(s[:1], s[:1].clone())
