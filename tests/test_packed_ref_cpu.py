"""Pins tests/packed_ref.py, the reference side of the packed forward tests, without a GPU: its bit layouts against a
reference-made fixture and the oracle, the exactness of every dyadic case the GPU file runs, and the room the float bar
leaves over a plain fp32 evaluation of the kernels' contract."""
import numpy as np
import pytest
import torch

import packed_ref as R
from conftest import load_golden


@pytest.fixture(scope="module")
def O():
    from oracle import gptq_oracle
    return gptq_oracle


@pytest.mark.parametrize("bits", [3, 4])
def test_pack_reproduces_reference_made_fixture(bits):
    g = load_golden("g4_pack")
    W, scale, zero = (torch.from_numpy(g[f"b{bits}_{k}"]) for k in ("W", "scale", "zero"))
    codes = torch.round((W + zero * scale) / scale).to(torch.int).t().contiguous().numpy()     # [in, out]
    assert codes.min() >= 0 and codes.max() <= 2 ** bits - 1
    assert np.array_equal(R.pack(codes, bits), g[f"b{bits}_qweight"])
    assert np.array_equal(R.unpack(g[f"b{bits}_qweight"], bits), codes)


@pytest.mark.parametrize("bits", [3, 4])
def test_layouts_agree_with_oracle(O, bits):
    rng = np.random.default_rng(bits)
    codes = rng.integers(0, 2 ** bits, (96, 37), dtype=np.uint8)
    for j, v in ((10, 5), (21, 6), (42, 7), (53, 3)):         # 3-bit: codes 10 and 21 of a group straddle two words
        codes[j] = v
    opack, ounpack = (O.pack3, O.unpack3) if bits == 3 else (O.pack4, O.unpack4)
    qw = R.pack(codes, bits)
    assert qw.dtype == np.int32 and qw.shape == (96 // 32 * bits, 37)
    assert np.array_equal(qw, opack(codes.astype(np.uint32)))
    assert np.array_equal(R.unpack(qw, bits), ounpack(qw).astype(np.uint8))
    assert np.array_equal(R.unpack(qw, bits), codes)
    # every single-code pattern at the straddling positions survives the round trip
    if bits == 3:
        for j in (10, 21):
            for v in range(8):
                one = np.zeros((32, 1), dtype=np.uint8)
                one[j] = v
                assert np.array_equal(R.unpack3(R.pack3(one)), one)
                assert np.array_equal(R.pack3(one), O.pack3(one.astype(np.uint32)))


@pytest.mark.parametrize("bits", [3, 4])
def test_reference_agrees_with_oracle_matvec(O, bits):
    c = R.dyadic_case(bits, 416, 37, -1, 1, seed=5, x_dtype="f32")
    y = O.dequant_matvec(c.x[0].numpy(), c.qweight, c.bias, c.scales, c.zeros, bits)
    assert np.array_equal(y, c.ref[0])
    r = R.realistic_case("relu", bits, 416, 37, -1, 1, seed=5, x_dtype="f32")
    y = O.dequant_matvec(r.x[0].numpy(), r.qweight, r.bias, r.scales, r.zeros, bits)
    assert np.allclose(y, r.ref[0], rtol=1e-12, atol=1e-12)
    assert np.array_equal(R.contract_magnitude(r.codes, r.scales, r.zeros, -1, r.xg, r.bias), r.T)
    assert (r.T_mv >= r.T).all() and (r.T >= np.abs(r.ref)).all()


def _check_exact(c):
    assert c.headroom < 1.0 and c.headroom_mv < 1.0, (c.headroom, c.headroom_mv)
    # every operand is a multiple of the lsb the bound is counted in, and the reference is an fp32 number
    assert np.array_equal(c.xg * 4.0, np.round(c.xg * 4.0))
    assert np.array_equal(c.bias.astype(np.float64) / c.lsb, np.round(c.bias.astype(np.float64) / c.lsb))
    assert np.array_equal(c.ref.astype(np.float32).astype(np.float64), c.ref)
    for seed, mv in ((1, False), (2, True)):
        y = R.emulate_fp32(c, seed=seed, matvec=mv)
        assert y.dtype == np.float32
        assert np.array_equal(y.astype(np.float64), c.ref), f"fp32 is not exact for this case (matvec={mv})"


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("row", R.GEMM_EXACT, ids=[R.case_id(r) for r in R.GEMM_EXACT])
def test_gemm_table_is_exact_in_fp32(bits, row):
    K, N, gs, Ms, xd, perm = row
    _check_exact(R.dyadic_case(bits, K, N, gs, max(Ms), perm=perm, seed=1, x_dtype=xd))


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("row", R.MATVEC_EXACT, ids=[R.case_id(r) for r in R.MATVEC_EXACT])
def test_matvec_table_is_exact_in_fp32(bits, row):
    K, N, gs = row
    for perm in ((False, True) if gs > 0 else (False,)):
        _check_exact(R.dyadic_case(bits, K, N, gs, 1, perm=perm, seed=2, x_dtype="f16"))


@pytest.mark.parametrize("bits", [3, 4])
def test_sweep_tables_are_exact_in_fp32(bits):
    for K, N, gs, Ms, xd in R.SWEEP_GEMM_PERM:
        _check_exact(R.dyadic_case(bits, K, N, gs, max(Ms), perm=True, seed=17, x_dtype=xd))
    for K, N, gs in R.SWEEP_MATVEC:
        for perm in ((False, True) if gs > 0 else (False,)):
            _check_exact(R.dyadic_case(bits, K, N, gs, 1, perm=perm, seed=19, x_dtype="f16"))


def test_dyadic_case_refuses_what_cannot_be_exact():
    with pytest.raises(ValueError):
        R.dyadic_case(4, 1 << 20, 2, -1, 1, seed=0, x_dtype="f32")


def test_fc2_shape_needs_a_narrow_x_range():
    c = R.dyadic_case(3, 36864, 64, -1, 1, seed=0, x_dtype="f16")
    assert c.x_range < 16 and c.headroom_mv < 1.0


@pytest.mark.parametrize("kind", R.REALISTIC_KINDS)
@pytest.mark.parametrize("bits,gs", [(4, 128), (3, 32), (4, -1)], ids=["4bit-g128", "3bit-g32", "4bit-row"])
def test_float_bar_leaves_room_over_fp32_contract(kind, bits, gs):
    """The reference alone stays within the bar: fp32 evaluation of the contract, error <= bar / 10 per element."""
    K, N, M = 4096, 96, 7
    worst = {}
    for xd in ("f16", "bf16", "f32"):
        c = R.realistic_case(kind, bits, K, N, gs, M, seed=3, x_dtype=xd)
        for mv in (False, True):
            n_chain = (K + K // (gs if gs > 0 else K) + 8) if mv else ((gs if gs > 0 else K) + K // (gs if gs > 0 else K) + 1 + 2)
            coef = min(1.1 * n_chain * 2.0 ** -24, 5e-5)
            err = np.abs(R.emulate_fp32(c, seed=4, matvec=mv).astype(np.float64) - c.ref)
            bar = coef * (c.T_mv if mv else c.T)
            worst[(xd, mv)] = float((err / bar).max())
    print(f"{kind} {bits}-bit g{gs}: fp32 contract error / bar, worst element: "
          + ", ".join(f"{k[0]}{'-mv' if k[1] else ''} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= 0.1, worst


def test_realistic_codes_cluster_round_the_zero_point():
    c = R.realistic_case("randn", 4, 1024, 64, 128, 1, seed=0)
    z = (c.zeros.astype(np.float64) / c.scales)[np.arange(1024) // 128]
    assert np.abs(c.codes - z).mean() < 2.5 and c.codes.min() == 0 and c.codes.max() == 15
    sub = R.realistic_case("subnormal", 4, 256, 8, 128, 2, seed=0, x_dtype="f16")
    ax = sub.x.abs().float()
    assert float(ax.max()) < 2.0 ** -14 and float(ax[ax > 0].min()) >= 2.0 ** -24     # fp16 subnormals, not flushed
