"""The grid gradients without a GPU: tests/packed_grid_ref.py (the reference side of tests/test_gpu_packed_grid_grad.py)
is pinned against torch.autograd on the dense fp64 formula, every dyadic row of the GPU table is shown to be exact in
fp32, and the public surface is checked as far as it goes without a device: the workspace queries and the plans they
reveal, validation before any launch, the parameter / buffer switch."""
import numpy as np
import pytest
import torch

import packed_grid_ref as R


# ------------------------------------------------------------------------------------------------ the reference side
@pytest.mark.parametrize("groupsize,perm", [(-1, False), (32, False), (64, True)])
@pytest.mark.parametrize("bits", R.BITS)
def test_reference_equals_autograd_of_the_dense_formula(bits, groupsize, perm):
    M, K, N = 5, 128, 7
    rng = np.random.default_rng([bits, max(groupsize, 0), int(perm), 1])
    codes = rng.integers(0, 2 ** bits, (K, N), dtype=np.uint8)
    qw = R.pack(codes, bits)
    G = K // groupsize if groupsize > 0 else 1
    p = rng.permutation(K).astype(np.int32) if perm else None
    x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).half()
    dy = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).half()
    s = torch.from_numpy(0.01 + 0.02 * rng.random((G, N))).requires_grad_()
    z = torch.from_numpy(0.1 * rng.random((G, N))).requires_grad_()
    b = torch.from_numpy(rng.standard_normal(N)).requires_grad_()
    grp = torch.arange(K) // groupsize if groupsize > 0 else torch.zeros(K, dtype=torch.long)
    xs = x.double()[:, torch.from_numpy(p).long()] if perm else x.double()
    y = xs @ (s[grp] * torch.from_numpy(R.unpack(qw, bits).astype(np.float64)) - z[grp]) + b
    gs_, gz_, gb_ = torch.autograd.grad((y * dy.double()).sum(), (s, z, b))
    dS, dZ, dB, T_S, T_Z = R.ref_grid_grad64(x, dy, qw, bits, groupsize, p)
    want = (G, N) if groupsize > 0 else (N,)
    assert dS.shape == want and dZ.shape == want and dB.shape == (N,) and T_S.shape == want and T_Z.shape == want
    for got, ref in ((dS, gs_), (dZ, gz_), (dB, gb_)):
        ref = ref.numpy().reshape(got.shape)
        assert np.allclose(got, ref, rtol=1e-12, atol=1e-12), float(np.abs(got - ref).max())
    assert (T_S >= np.abs(dS) - 1e-12).all() and (T_Z >= np.abs(dZ) - 1e-12).all()
    assert (T_S <= (2 ** bits - 1) * T_Z + 1e-12).all()


@pytest.mark.parametrize("bits", R.BITS)
@pytest.mark.parametrize("row", R.GRID_EXACT, ids=[R.grid_case_id(r) for r in R.GRID_EXACT])
def test_every_dyadic_case_of_the_gpu_table_is_exact(row, bits):
    K, N, gs = row
    c = R.dyadic_grid_case(bits, K, N, gs, max(R.GRID_MS), perm=False, seed=1)
    assert c.headroom < 1.0 and int(c.codes.max()) == 2 ** bits - 1
    x, dy = c.x.double().numpy(), c.dy.double().numpy()
    assert np.array_equal(x * 4.0, np.round(x * 4.0)) and np.array_equal(dy * 4.0, np.round(dy * 4.0))
    for dt in R.GRID_DT:                                     # the values are the same numbers in both 16-bit types
        assert torch.equal(c.x.to(R.torch_dtype(dt)).double(), c.x.double())
    dS, dZ, dB, T_S, T_Z = R.ref_grid_grad64(c.x, c.dy, c.qweight, bits, gs, None)
    for a in (dS, dZ, dB):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)        # the reference is an fp32 number
    # an fp32 evaluation in a shuffled order of tokens and rows gives the same bits
    rng = np.random.default_rng(3)
    A = np.zeros((K, N), dtype=np.float32)
    x32, d32 = c.x.float().numpy(), c.dy.float().numpy()
    for m in rng.permutation(c.M):
        A = A + x32[m][:, None] * d32[m][None, :]
    g = gs if gs > 0 else K
    accS = np.zeros((K // g, N), dtype=np.float32)
    accZ = np.zeros((K // g, N), dtype=np.float32)
    for k in rng.permutation(K):
        accS[k // g] = accS[k // g] + c.codes[k].astype(np.float32) * A[k]
        accZ[k // g] = accZ[k // g] + A[k]
    assert np.array_equal(accS.astype(np.float64).reshape(dS.shape), dS)
    assert np.array_equal(-accZ.astype(np.float64).reshape(dZ.shape), dZ)


@pytest.mark.parametrize("row", R.GRID_PERM, ids=R.grid_case_id)
def test_perm_cases_are_exact_and_perm_is_a_gather(row):
    K, N, gs = row
    c = R.dyadic_grid_case(4, K, N, gs, max(R.GRID_MS), perm=True, seed=2)
    assert c.headroom < 1.0
    a = R.ref_grid_grad64(c.x, c.dy, c.qweight, 4, gs, c.perm)
    b = R.ref_grid_grad64(c.x[:, torch.from_numpy(c.perm).long()], c.dy, c.qweight, 4, gs, None)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_dyadic_grid_case_refuses_what_cannot_be_exact():
    with pytest.raises(ValueError):
        R.dyadic_grid_case(8, 1 << 16, 2, -1, 1 << 11, seed=0)


def test_table_covers_what_the_issue_lists():
    rows = set(R.GRID_EXACT)
    assert {(32, 4, -1), (96, 20, -1), (160, 100, -1), (160, 100, 32), (256, 264, -1), (256, 264, 32), (256, 264, 64),
            (64, 1040, 32), (544, 40, 32), (544, 40, -1)} <= rows
    assert set(R.GRID_MS) == {1, 3, 17, 130} and set(R.GRID_DT) == {"f16", "bf16"} and set(R.BITS) == {2, 3, 4, 8}
    assert set(R.GRID_PERM) == {(160, 100, 32), (256, 264, 64), (64, 1040, 32)}


def test_realistic_bars_scale_with_the_chain_lengths():
    c = R.realistic_grid_case("outlier", 4, 64, 40, 32, 8, seed=1)
    assert np.allclose(c.bar_S, (8 + 32 + 1) * 2.0 ** -24 * c.T_S) and np.allclose(c.bar_Z, (8 + 32 + 1) * 2.0 ** -24 * c.T_Z)
    assert np.allclose(c.bar_B, 8 * 2.0 ** -24 * np.abs(c.dy.double().numpy()).sum(0))
    r = R.realistic_grid_case("randn", 3, 64, 40, -1, 8, seed=1)
    assert r.dS.shape == (40,) and np.allclose(r.bar_S, (8 + 64 + 1) * 2.0 ** -24 * r.T_S)


# ------------------------------------------------------------------------------------------------ the public surface
def test_workspace_queries_need_no_device_and_show_both_plans():
    from gptq_amd import _lib
    from gptq_amd.build import build_library
    build_library(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, "gptq_quant_gemm_grid_grad") and lib.gptq_hip_abi_version() == 2
    q, qp = lib.gptq_quant_gemm_grid_grad_workspace_bytes, lib.gptq_quant_gemm_grid_grad_perm_workspace_bytes
    for bits in R.BITS:
        assert q(2048, 4096, 4096, bits, 128) == 0           # a group is one K tile, enough tiles: one pass
        assert q(2048, 4096, 4096, bits, 32) == 0 and q(2048, 4096, 4096, bits, 64) == 0
        # per-row grids: one partial per K tile for dscales and for dzeros
        assert q(2048, 4096, 4096, bits, -1) == 2 * (4096 // 128) * 4096 * 4
        assert q(2048, 4096, 4096, bits, 256) == 2 * (4096 // 128) * 4096 * 4
        assert q(16, 256, 264, bits, 64) == 0 and q(130, 256, 264, bits, 64) > 0      # few tiles, 5 stages: tokens split
        # with perm the gathered copy of x is added (16-bit, M x K)
        assert qp(2048, 4096, 4096, bits, 128) == 2048 * 4096 * 2
        assert qp(130, 256, 264, bits, 64) >= q(130, 256, 264, bits, 64) + 130 * 256 * 2
    for bad in (0, 1, 5, 16):
        assert q(4, 4096, 4096, bad, -1) == 0
    assert q(0, 4096, 4096, 4, -1) == 0 and q(4, 48, 4096, 4, -1) == 0 and q(4, 4096, 4096, 4, 48) == 0
    # far smaller than the dense [K, N] fp32 gradient it replaces
    assert q(2048, 4096, 11008, 4, -1) * 16 < 4096 * 11008 * 4


def test_python_wrapper_validates_before_any_launch():
    import gptq_amd as G
    qw = torch.zeros((64 // 32 * 4, 40), dtype=torch.int32)
    x, dy = torch.zeros(3, 64, dtype=torch.float16), torch.zeros(3, 40, dtype=torch.float16)
    perm = torch.arange(64, dtype=torch.int32)
    with pytest.raises(ValueError, match="x must be fp16 or bf16"):
        G.quant_grid_grad(x.float(), dy, qw, 4)
    with pytest.raises(ValueError, match="grad must have x's dtype"):
        G.quant_grid_grad(x, dy.bfloat16(), qw, 4)
    with pytest.raises(ValueError, match="perm .* needs grouped grids"):
        G.quant_grid_grad(x, dy, qw, 4, -1, perm=perm)
    with pytest.raises(ValueError, match="bits must be"):
        G.quant_grid_grad(x, dy, qw, 5)
    with pytest.raises(ValueError, match="groupsize"):
        G.quant_grid_grad(x, dy, qw, 4, 48)
    with pytest.raises(ValueError, match="output features"):
        G.quant_grid_grad(x, dy[:, :39], qw, 4)
    with pytest.raises(ValueError, match="numbers of tokens"):
        G.quant_grid_grad(x, dy[:2], qw, 4)
    with pytest.raises(ValueError, match="input features"):
        G.quant_grid_grad(x[:, :32], dy, qw, 4)


def test_trainable_grids_is_opt_in_and_keeps_the_state_dict_keys():
    import gptq_amd as G
    model = torch.nn.Sequential(G.Quant3Linear(64, 40), G.QuantGroupLinear(4, 32, 64, 40, act_order=True),
                                torch.nn.Linear(40, 8))
    packed = list(model)[:2]
    for m in packed:
        assert not list(m.parameters())
    keys = sorted(model.state_dict())
    saved = {k: v.clone() for k, v in model.state_dict().items()}
    params = G.trainable_grids(model, zeros=False)
    assert len(params) == 4 and all(isinstance(p, torch.nn.Parameter) and p.dtype == torch.float32 for p in params)
    for m in packed:
        assert sorted(n for n, _ in m.named_parameters()) == ["bias", "scales"]
        assert "zeros" in dict(m.named_buffers()) and "qweight" in dict(m.named_buffers())
    assert packed[0].scales.shape == (40, 1) and packed[1].scales.shape == (2, 40)
    assert sorted(model.state_dict()) == keys
    model.load_state_dict(saved)                             # a checkpoint of buffers loads into parameters ...
    with torch.no_grad():
        packed[0].scales.add_(1.0)
    trained = {k: v.clone() for k, v in model.state_dict().items()}
    assert G.frozen_grids(model) == 4
    for m in packed:
        assert not list(m.parameters())
    assert sorted(model.state_dict()) == keys and bool((packed[0].scales == 1.0).all())
    model.load_state_dict(saved)                             # ... and back
    model.load_state_dict(trained)
    assert len(G.trainable_grids(model)) == 6 and G.frozen_grids(model) == 6
