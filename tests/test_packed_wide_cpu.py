"""2- and 8-bit packing without a GPU: tests/packed_ref_wide.py (the reference side of tests/test_gpu_packed_wide.py) is
pinned -- layout round trips, word / bit position of single codes, exactness of every dyadic table row -- and the public
surface of the new widths is checked as far as it goes without a device: symbols, validation before any launch, no CPU
fallback, module buffers."""
import os
import re

import numpy as np
import pytest
import torch

import packed_ref_wide as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = list(R.WIDE_BITS)


# ------------------------------------------------------------------------------------------------ the reference side
@pytest.mark.parametrize("bits", BITS)
def test_pack_unpack_round_trip(bits):
    rng = np.random.default_rng(bits)
    codes = rng.integers(0, 2 ** bits, (96, 37), dtype=np.uint8)
    qw = R.pack(codes, bits)
    assert qw.dtype == np.int32 and qw.shape == (96 // 32 * bits, 37)
    assert np.array_equal(R.unpack(qw, bits), codes)
    assert np.array_equal(R.pack(R.unpack(qw, bits), bits), qw)
    full = np.full((32, 2), 2 ** bits - 1, dtype=np.uint8)          # all ones: every bit of every word is used
    assert np.array_equal(R.pack(full, bits).view(np.uint32), np.full((bits, 2), 0xFFFFFFFF, dtype=np.uint32))


@pytest.mark.parametrize("bits", BITS)
def test_single_code_sits_where_the_format_says(bits):
    """Code i of a column sits in word i // (32/bits) at bit bits * (i % (32/bits)), and nowhere else."""
    cpw = 32 // bits
    for i in range(64):
        for v in (1, 2 ** bits - 1):
            one = np.zeros((64, 3), dtype=np.uint8)
            one[i, 1] = v
            qw = R.pack(one, bits).view(np.uint32)
            want = np.zeros((64 // cpw, 3), dtype=np.uint32)
            want[i // cpw, 1] = np.uint32(v) << np.uint32(bits * (i % cpw))
            assert np.array_equal(qw, want), (bits, i, v)
    # the 4-bit rule itself, written the same way, gives packed_ref's own 4-bit layout
    import packed_ref as R4
    codes = np.random.default_rng(4).integers(0, 16, (64, 5), dtype=np.uint8)
    assert np.array_equal(R._pack_pow2(codes, 4), R4.pack4(codes))


def _check_exact(c):
    assert c.headroom < 1.0 and c.headroom_mv < 1.0, (c.headroom, c.headroom_mv)
    assert (c.T_mv >= c.T).all() and (c.T >= np.abs(c.ref)).all()
    # every operand is a multiple of the lsb the bound is counted in, and the reference is an fp32 number
    assert np.array_equal(c.xg * 4.0, np.round(c.xg * 4.0))
    assert np.array_equal(c.bias.astype(np.float64) / c.lsb, np.round(c.bias.astype(np.float64) / c.lsb))
    assert np.array_equal(c.ref.astype(np.float32).astype(np.float64), c.ref)
    assert int(c.codes.max()) == 2 ** c.bits - 1
    for seed, mv in ((1, False), (2, True)):
        y = R.emulate_fp32(c, seed=seed, matvec=mv)
        assert y.dtype == np.float32
        assert np.array_equal(y.astype(np.float64), c.ref), f"fp32 is not exact for this case (matvec={mv})"


def test_tables_cover_the_classes():
    assert len(R.GEMM_EXACT) >= 10 and len(R.MATVEC_EXACT) >= 8
    Ks = {r[0] for r in R.GEMM_EXACT}
    Ns = {r[1] for r in R.GEMM_EXACT}
    gss = {r[2] if r[2] != r[0] else "K" for r in R.GEMM_EXACT}
    Ms = {m for r in R.GEMM_EXACT for m in r[3]}
    assert {32, 96, 160, 1056, 1408, 2048} <= Ks
    assert {1, 3, 65, 255, 1001} <= Ns
    assert {-1, 32, 96, 128, 512, "K"} <= gss
    assert {1, 16, 17, 32, 33, 64, 65, 128, 129} <= Ms
    assert {r[4] for r in R.GEMM_EXACT} == {"f16", "bf16"} and {r[5] for r in R.GEMM_EXACT} == {False, True}
    assert any(r[5] and min(r[3]) <= 4 for r in R.GEMM_EXACT) and any(r[5] and max(r[3]) > 4 for r in R.GEMM_EXACT)
    for row in ((32, 1, -1), (96, 130, 96), (416, 257, -1), (416, 255, 32), (1408, 4096, 128), (1408, 3, -1)):
        assert row in R.MATVEC_EXACT
    assert any(r[0] == 4096 for r in R.MATVEC_EXACT)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("row", R.GEMM_EXACT, ids=[R.case_id(r) for r in R.GEMM_EXACT])
def test_gemm_table_is_exact_in_fp32(bits, row):
    K, N, gs, Ms, xd, perm = row
    _check_exact(R.dyadic_case(bits, K, N, gs, max(Ms), perm=perm, seed=1, x_dtype=xd))


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("row", R.MATVEC_EXACT, ids=[R.case_id(r) for r in R.MATVEC_EXACT])
def test_matvec_table_is_exact_in_fp32(bits, row):
    K, N, gs = row
    for perm in ((False, True) if gs > 0 else (False,)):
        _check_exact(R.dyadic_case(bits, K, N, gs, 1, perm=perm, seed=2, x_dtype="f16"))


def test_dyadic_case_refuses_what_cannot_be_exact():
    with pytest.raises(ValueError):
        R.dyadic_case(8, 1 << 17, 2, -1, 1, seed=0, x_dtype="f32")


# ------------------------------------------------------------------------------------------------ the public surface
def test_header_and_binding_agree_on_the_new_symbols():
    from gptq_amd import _lib
    text = open(os.path.join(ROOT, "include", "gptq_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("gptq_vecquant2matmul", "gptq_vecquant8matmul"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.EXPORTS
        assert _lib._SIGNATURES[name] == _lib._SIGNATURES["gptq_vecquant4matmul"]      # the 4-bit signature


def test_library_exports_the_new_symbols_and_sizes_workspaces():
    from gptq_amd import _lib
    from gptq_amd.build import build_library
    build_library(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, "gptq_vecquant2matmul") and hasattr(lib, "gptq_vecquant8matmul")
    assert lib.gptq_hip_abi_version() == 2                                             # new symbols, same ABI
    for bits in BITS:
        small = lib.gptq_quant_gemm_workspace_bytes(2, 4096, 4096, bits, -1)
        assert small > 0 and small % (2 * 4096 * 4) == 0                               # S chunks of M x N fp32
        assert lib.gptq_quant_gemm_workspace_bytes(2048, 4096, 11008, bits, 128) == 0
        assert lib.gptq_quant_gemm_perm_workspace_bytes(17, 4096, 4096, bits, 128) >= 17 * 4096 * 2   # the gathered X
    for bad in (0, 1, 5, 6, 7, 16):
        assert lib.gptq_quant_gemm_workspace_bytes(2, 4096, 4096, bad, -1) == 0
        assert lib.gptq_quant_gemm_perm_workspace_bytes(17, 4096, 4096, bad, 128) == 0


@pytest.mark.parametrize("bits", BITS)
def test_validation_raises_before_any_launch(bits):
    import gptq_amd
    from gptq_amd import quant as Q
    from gptq_amd import quant_cuda
    K, N = 64, 16
    x = torch.zeros(3, K, dtype=torch.float16)
    qw = torch.zeros(K // 32 * bits, N, dtype=torch.int32)
    s, z = torch.ones(N), torch.zeros(N)
    with pytest.raises(ValueError):                       # qweight of another width's height
        gptq_amd.quant_matmul(x, torch.zeros(K // 32 * 4, N, dtype=torch.int32), s, z, bits)
    with pytest.raises(ValueError):                       # K mismatch
        gptq_amd.quant_matmul(torch.zeros(3, 96, dtype=torch.float16), qw, s, z, bits)
    with pytest.raises(ValueError):                       # grouped tables of another groupsize
        gptq_amd.quant_matmul(x, qw, torch.ones(1, N), torch.zeros(1, N), bits, 32)
    with pytest.raises(ValueError):                       # perm needs grouped grids
        gptq_amd.quant_matmul(x, qw, s, z, bits, -1, perm=torch.arange(K, dtype=torch.int32))
    for bad in (1, 5, 16):
        with pytest.raises(ValueError):
            gptq_amd.quant_matmul(x, qw, s, z, bad)
        with pytest.raises(ValueError):
            Q.pack_codes(torch.zeros(N, K, dtype=torch.uint8), bad)
        with pytest.raises(ValueError):
            Q._pack(torch.zeros(N, K), s, z, bad)
        with pytest.raises(ValueError):
            Q.pack_grouped(torch.zeros(N, K), torch.ones(2, N), torch.zeros(2, N), 32, bad)
        with pytest.raises(ValueError):
            Q.dequant_packed(qw, torch.ones(1, N), torch.zeros(1, N), bad, -1)
        with pytest.raises(ValueError):
            gptq_amd.QuantGroupLinear(bad, 32, K, N)
        with pytest.raises(ValueError):
            quant_cuda.vecquant_matmul_grouped(torch.zeros(K), qw, torch.zeros(N), torch.ones(2, N), torch.zeros(2, N),
                                               bad, 32)
    with pytest.raises(ValueError):                       # in_features no multiple of 32
        Q.pack_codes(torch.zeros(N, 48, dtype=torch.uint8), bits)
    with pytest.raises(ValueError):
        Q.pack_grouped(torch.zeros(N, K), torch.ones(2, N), torch.zeros(2, N), 48, bits)
    with pytest.raises(ValueError):                       # tables of another shape
        Q.pack_grouped(torch.zeros(N, K), torch.ones(1, N), torch.zeros(1, N), 32, bits)
    with pytest.raises(ValueError):
        gptq_amd.QuantGroupLinear(bits, 48, 96, N)
    from gptq_amd.sequential import make_packed_skeleton, pack_model
    with pytest.raises(ValueError):
        pack_model(torch.nn.Sequential(torch.nn.Linear(K, N)), {}, 5)
    with pytest.raises(ValueError):
        make_packed_skeleton(torch.nn.Sequential(torch.nn.Linear(K, N)), ["0"], 6)


@pytest.mark.parametrize("bits", BITS)
def test_without_gpu_is_a_loud_failure(bits):
    import gptq_amd
    from gptq_amd import _lib
    from gptq_amd import quant as Q
    from gptq_amd import quant_cuda
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    K, N = 64, 16
    qw = torch.zeros(K // 32 * bits, N, dtype=torch.int32)
    s, z = torch.ones(N), torch.zeros(N)
    with pytest.raises(_lib.GptqHipError):
        gptq_amd.quant_matmul(torch.zeros(3, K, dtype=torch.float16), qw, s, z, bits)
    with pytest.raises(_lib.GptqHipError):
        Q.pack_codes(torch.zeros(N, K, dtype=torch.uint8), bits)
    with pytest.raises(_lib.GptqHipError):
        Q._pack(torch.zeros(N, K), s, z, bits)
    with pytest.raises(_lib.GptqHipError):
        Q.pack_grouped(torch.zeros(N, K), torch.ones(2, N), torch.zeros(2, N), 32, bits)
    with pytest.raises(_lib.GptqHipError):
        Q.dequant_packed(qw, torch.ones(1, N), torch.zeros(1, N), bits, -1)
    fn = {2: quant_cuda.vecquant2matmul, 8: quant_cuda.vecquant8matmul}[bits]
    with pytest.raises(_lib.GptqHipError):
        fn(torch.zeros(K), qw, torch.zeros(N), s, z)
    with pytest.raises(_lib.GptqHipError):
        quant_cuda.vecquant_matmul_grouped(torch.zeros(K), qw, torch.zeros(N), torch.ones(2, N), torch.zeros(2, N), bits, 32)
    cls = {2: gptq_amd.Quant2Linear, 8: gptq_amd.Quant8Linear}[bits]
    for m in (cls(K, N), cls(K, N, multi_token=True), gptq_amd.QuantGroupLinear(bits, 32, K, N, multi_token=True)):
        with pytest.raises(_lib.GptqHipError):
            m(torch.zeros(1, 1, K, dtype=torch.float16))
    with pytest.raises(_lib.GptqHipError):
        cls(K, N, multi_token=True)(torch.zeros(1, 3, K, dtype=torch.float16))
    with pytest.raises(_lib.GptqHipError):
        cls(K, N).pack(torch.nn.Linear(K, N), torch.ones(N, 1), torch.zeros(N, 1))


@pytest.mark.parametrize("bits", BITS)
def test_module_buffers_and_state_dict(bits):
    import gptq_amd
    from gptq_amd.quant import PACKED_LINEAR
    K, N, gs = 96, 10, 32
    cls = {2: gptq_amd.Quant2Linear, 8: gptq_amd.Quant8Linear}[bits]
    assert PACKED_LINEAR[bits] is cls and cls.bits == bits
    m = cls(K, N)
    sd = m.state_dict()
    assert sorted(sd) == ["bias", "qweight", "scales", "zeros"] == sorted(gptq_amd.Quant4Linear(K, N).state_dict())
    assert sd["qweight"].shape == (K // 32 * bits, N) and sd["qweight"].dtype == torch.int32
    assert sd["scales"].shape == (N, 1) and sd["zeros"].shape == (N, 1) and sd["bias"].shape == (N,)
    assert m.multi_token is False
    with pytest.raises(ValueError):
        m(torch.zeros(2, K, dtype=torch.float16))         # the reference's single-token guard stays the default
    for act in (False, True):
        g = gptq_amd.QuantGroupLinear(bits, gs, K, N, act_order=act)
        sd = g.state_dict()
        assert sorted(sd) == sorted(["bias", "qweight", "scales", "zeros"] + (["perm"] if act else []))
        assert sd["qweight"].shape == (K // 32 * bits, N) and sd["qweight"].dtype == torch.int32
        assert sd["scales"].shape == (K // gs, N) and sd["zeros"].shape == (K // gs, N)
        if act:
            assert sd["perm"].shape == (K,) and sd["perm"].dtype == torch.int32
        assert torch.equal(g.g_idx, (torch.arange(K) // gs).int())
    # skeletons: the named Linears become the width's module
    from gptq_amd.sequential import make_packed_skeleton

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.act, self.fc2 = torch.nn.Linear(K, N), torch.nn.ReLU(), torch.nn.Linear(K, N)

    net = Net()
    make_packed_skeleton(net, ["fc1"], bits, multi_token=True)
    assert isinstance(net.fc1, cls) and net.fc1.multi_token and isinstance(net.fc2, torch.nn.Linear)
    make_packed_skeleton(net, ["fc2"], bits, groupsize=gs, act_order=True)
    assert isinstance(net.fc2, gptq_amd.QuantGroupLinear) and net.fc2.bits == bits and net.fc2.act_order
    mk = {2: gptq_amd.make_quant2, 8: gptq_amd.make_quant8}[bits]
    net = Net()
    mk(net, ["fc2"])
    assert isinstance(net.fc2, cls) and isinstance(net.fc1, torch.nn.Linear)
    assert gptq_amd.set_multi_token(net) == 1 and net.fc2.multi_token
