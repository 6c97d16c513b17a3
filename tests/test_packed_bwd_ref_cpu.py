"""The packed backward without a GPU: tests/packed_bwd_ref.py (the reference side of tests/test_gpu_packed_bwd.py) is
pinned against a plain triple loop, every dyadic row of the GPU table is shown to be exact in fp32, and the public surface
is checked as far as it goes without a device: symbols, the workspace query, validation before any launch."""
import os
import re

import numpy as np
import pytest
import torch

import packed_bwd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the reference side
def _to16(v, dtype):
    return float(torch.tensor(np.float32(v)).to(R.torch_dtype(dtype)).double())


@pytest.mark.parametrize("dy_dtype", R.BWD_DY)
@pytest.mark.parametrize("groupsize,perm", [(-1, False), (32, False), (32, True)])
@pytest.mark.parametrize("bits", R.BITS)
def test_ref_dx_against_a_triple_loop(bits, groupsize, perm, dy_dtype):
    M, K, N = 2, 32, 5
    rng = np.random.default_rng([bits, max(groupsize, 0), int(perm)])
    codes = rng.integers(0, 2 ** bits, (K, N), dtype=np.uint8)
    qw = R.pack(codes, bits)
    s = (0.01 + 0.02 * rng.random(N)).astype(np.float32)
    z = (s * rng.integers(0, 2 ** bits, N)).astype(np.float32)
    sc, zr = (s.reshape(1, N), z.reshape(1, N)) if groupsize > 0 else (s, z)
    p = rng.permutation(K).astype(np.int32) if perm else None
    dy = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).to(R.torch_dtype(dy_dtype))
    want = np.zeros((M, K))
    T = np.zeros((M, K))
    for m in range(M):
        for k in range(K):
            acc = t = 0.0
            for n in range(N):
                w = _to16(np.float32(np.float32(s[n] * np.float32(codes[k, n])) - z[n]), dy_dtype)
                acc += float(dy[m, n]) * w
                t += abs(float(dy[m, n]) * w)
            want[m, p[k] if perm else k] = acc
            T[m, p[k] if perm else k] = t
    got, gotT = R.ref_dx64(dy, qw, sc, zr, bits, groupsize, p, dy_dtype)
    assert np.allclose(got, want, rtol=1e-13, atol=1e-15) and np.allclose(gotT, T, rtol=1e-13, atol=1e-15)
    for yd in ("f32", "f16", "bf16"):
        y = R.ref_dx(dy, qw, sc, zr, bits, groupsize, p, dy_dtype, yd)
        assert y.dtype == R.torch_dtype(yd) and tuple(y.shape) == (M, K)
        assert (np.abs(y.double().numpy() - got) <= R.half_ulp(got, yd)).all()      # one rounding


def test_round_to_rounds_once():
    # 1 + 2^-11 + 2^-30 lies above the fp16 tie at 1 + 2^-11: one rounding goes up, a detour through fp32 would not
    v = np.array([1.0 + 2.0 ** -11 + 2.0 ** -30, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, -3 * 2.0 ** -25, 0.0])
    got = R.round_to(v, "f16").double().numpy()
    assert np.array_equal(got, [1.0 + 2.0 ** -10, 1.0, 1.0 + 2.0 ** -9, 0.0, -2.0 ** -23, 0.0])
    assert np.array_equal(R.round_to(np.array([1.0 + 2.0 ** -8 + 2.0 ** -40]), "bf16").double().numpy(), [1.0 + 2.0 ** -7])
    assert np.array_equal(R.half_ulp(np.array([1.0, 1.5, 2.0, 2.0 ** -20]), "f16"),
                          [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -25])


@pytest.mark.parametrize("dy_dtype", R.BWD_DY)
@pytest.mark.parametrize("bits", R.BITS)
@pytest.mark.parametrize("row", R.BWD_EXACT, ids=[R.bwd_case_id(r) for r in R.BWD_EXACT])
def test_every_dyadic_case_of_the_gpu_table_is_exact(row, bits, dy_dtype):
    K, N, gs = row
    c = R.dyadic_bwd_case(bits, K, N, gs, max(R.BWD_MS), perm=False, seed=1, dy_dtype=dy_dtype)
    assert c.headroom < 1.0 and (c.T >= np.abs(c.ref)).all()
    # dy, W16 and so every product and partial sum are multiples of the lsb the bound is counted in
    W = R.w16(c.qweight, c.scales, c.zeros, bits, gs, dy_dtype)
    s = np.asarray(c.scales, dtype=np.float64).reshape(-1, N)
    z = np.asarray(c.zeros, dtype=np.float64).reshape(-1, N)
    grp = np.arange(K) // gs if gs > 0 else np.zeros(K, dtype=np.int64)
    assert np.array_equal(W, s[grp] * c.codes - z[grp])                          # W16 = s (q - zero) is exact in 16 bits
    assert np.array_equal(W / (4 * c.lsb), np.round(W / (4 * c.lsb)))
    assert np.array_equal(c.dy.double().numpy() * 4.0, np.round(c.dy.double().numpy() * 4.0))
    assert np.array_equal(c.ref.astype(np.float32).astype(np.float64), c.ref)    # the reference is an fp32 number
    assert int(c.codes.max()) == 2 ** bits - 1
    # an fp32 chain in a shuffled order of n gives the same bits
    order = np.random.default_rng(3).permutation(N)
    acc = np.zeros((c.M, K), dtype=np.float32)
    d32, W32 = c.dy.float().numpy(), W.astype(np.float32)
    for n in order:
        acc = acc + d32[:, n:n + 1] * W32[:, n][None, :]
    assert np.array_equal(acc.astype(np.float64), c.ref)


def test_dyadic_bwd_case_refuses_what_cannot_be_exact():
    with pytest.raises(ValueError):
        R.dyadic_bwd_case(8, 32, 1 << 17, -1, 1, seed=0)


def test_table_covers_what_the_kernel_can_get_wrong():
    rows = set(R.BWD_EXACT)
    assert {(32, 4, -1), (96, 20, -1), (160, 100, -1), (160, 100, 32), (256, 264, -1), (256, 264, 32), (256, 264, 64)} <= rows
    assert set(R.BWD_MS) == {1, 3, 17, 130} and set(R.BWD_DY) == {"f16", "bf16"} and set(R.BITS) == {2, 3, 4, 8}


# ------------------------------------------------------------------------------------------------ the public surface
def test_header_and_binding_carry_the_new_symbols():
    from gptq_amd import _lib
    text = open(os.path.join(ROOT, "include", "gptq_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+gptq_quant_gemm_t\s*\(", text)
    assert re.search(r"\bsize_t\s+gptq_quant_gemm_t_workspace_bytes\s*\(", text)
    assert "gptq_quant_gemm_t" in _lib.EXPORTS and "gptq_quant_gemm_t_workspace_bytes" in _lib.EXPORTS
    assert len(_lib._SIGNATURES["gptq_quant_gemm_t"][1]) == 18
    import gptq_amd
    assert callable(gptq_amd.quant_matmul_t)


def test_workspace_query_needs_no_device():
    from gptq_amd import _lib
    from gptq_amd.build import build_library
    build_library(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, "gptq_quant_gemm_t") and lib.gptq_hip_abi_version() == 2
    query = lib.gptq_quant_gemm_t_workspace_bytes
    for bits in R.BITS:
        assert query(1, 32, 1, bits, -1) >= 0                                     # the smallest shape
        for K, N, gs in ((4096, 4096, -1), (4096, 11008, 128), (11008, 4096, 128), (256, 264, 32), (32, 4, -1)):
            sizes = [query(M, K, N, bits, gs) for M in range(1, 17)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (bits, K, N, sizes)
            assert all(s % 4 == 0 for s in sizes)
        assert query(1, 4096, 4096, bits, -1) > 0                                 # too few tiles at M = 1: the N range is split
        assert query(1, 4096, 4096, bits, -1) % (4096 * 4) == 0                   # S chunks of M x K fp32
    for bad in (0, 1, 5, 16):
        assert query(4, 4096, 4096, bad, -1) == 0
    assert query(0, 4096, 4096, 4, -1) == 0 and query(4, 48, 4096, 4, -1) == 0


def test_quant_matmul_t_validates_before_any_launch():
    import gptq_amd
    K, N, bits = 64, 16, 4
    g = torch.zeros(3, N, dtype=torch.float16)
    qw = torch.zeros(K // 32 * bits, N, dtype=torch.int32)
    s, z = torch.ones(N), torch.zeros(N)
    with pytest.raises(ValueError):                       # fp32 grad
        gptq_amd.quant_matmul_t(g.float(), qw, s, z, bits)
    with pytest.raises(ValueError):                       # N mismatch
        gptq_amd.quant_matmul_t(torch.zeros(3, N + 1, dtype=torch.float16), qw, s, z, bits)
    with pytest.raises(ValueError):                       # qweight height no multiple of bits
        gptq_amd.quant_matmul_t(g, torch.zeros(7, N, dtype=torch.int32), s, z, bits)
    with pytest.raises(ValueError):                       # grouped tables of another groupsize
        gptq_amd.quant_matmul_t(g, qw, torch.ones(1, N), torch.zeros(1, N), bits, 32)
    with pytest.raises(ValueError):                       # perm needs grouped grids
        gptq_amd.quant_matmul_t(g, qw, s, z, bits, -1, perm=torch.arange(K, dtype=torch.int32))
    with pytest.raises(ValueError):
        gptq_amd.quant_matmul_t(g, qw, s, z, 5)
    with pytest.raises(ValueError):
        gptq_amd.quant_matmul_t(g, qw, s, z, bits, out_dtype=torch.float64)
    if not torch.cuda.is_available():
        from gptq_amd import _lib
        with pytest.raises(_lib.GptqHipError):            # no CPU path
            gptq_amd.quant_matmul_t(g, qw, s, z, bits)


def test_fp32_activations_under_autograd_raise():
    import gptq_amd
    K, N = 64, 16
    for m in (gptq_amd.Quant4Linear(K, N, multi_token=True), gptq_amd.QuantGroupLinear(4, 32, K, N, multi_token=True)):
        for shape in ((K,), (3, K)):
            x = torch.zeros(shape, dtype=torch.float32, requires_grad=True)
            with pytest.raises(ValueError, match="backward through packed Linears needs fp16/bf16 activations"):
                m(x)
    x = torch.zeros(3, K, dtype=torch.float32, requires_grad=True)
    with pytest.raises(ValueError, match="backward through packed Linears needs fp16/bf16 activations"):
        gptq_amd.quant_matmul(x, torch.zeros(K // 8, N, dtype=torch.int32), torch.ones(N), torch.zeros(N), 4)
