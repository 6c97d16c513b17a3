"""The backward of the packed Linears on the GPU: gptq_quant_gemm_t / quant_matmul_t against tests/packed_bwd_ref.py
(bit for bit on dyadic inputs, within the derived bar on realistic ones), and autograd through the modules."""
import functools

import numpy as np
import pytest
import torch

import packed_bwd_ref as R

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def G():
    import gptq_amd
    return gptq_amd


@pytest.fixture(scope="module")
def device():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _dyadic(bits, K, N, gs, dy_dtype):
    return R.dyadic_bwd_case(bits, K, N, gs, max(R.BWD_MS), perm=False, seed=1, dy_dtype=dy_dtype)


def _operands(c, device):
    return R.dev(c.qweight, device), R.dev(c.scales, device), R.dev(c.zeros, device)


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("dy_dtype", R.BWD_DY)
@pytest.mark.parametrize("bits", R.BITS)
@pytest.mark.parametrize("row", R.BWD_EXACT, ids=[R.bwd_case_id(r) for r in R.BWD_EXACT])
def test_dx_equals_the_reference_on_dyadic_inputs(G, device, row, bits, dy_dtype):
    K, N, gs = row
    c = _dyadic(bits, K, N, gs, dy_dtype)
    qw, s, z = _operands(c, device)
    for m in R.BWD_MS:
        dy = c.dy[:m].to(device)
        for yd in ("f32", dy_dtype):
            want = R.round_to(c.ref[:m], yd).to(device)
            got = G.quant_matmul_t(dy, qw, s, z, bits, gs, out_dtype=DT[yd])
            assert got.dtype == DT[yd] and tuple(got.shape) == (m, K)
            R.assert_equal_bits(got, want, f"{bits}-bit {K}x{N} g{gs} M={m} dy {dy_dtype} y {yd}")


def test_the_table_reaches_the_split_path(G):
    from gptq_amd import _lib
    q = _lib.load().gptq_quant_gemm_t_workspace_bytes
    for bits in R.BITS:
        assert any(q(m, K, N, bits, gs) > 0 for K, N, gs in R.BWD_EXACT for m in R.BWD_MS), bits
        assert any(q(m, K, N, bits, gs) == 0 for K, N, gs in R.BWD_EXACT for m in R.BWD_MS), bits


# ------------------------------------------------------------------------------------------------ perm
@pytest.mark.parametrize("bits", R.BITS)
@pytest.mark.parametrize("row", [(160, 100, 32), (256, 264, 64), (64, 1040, 32)], ids=R.bwd_case_id)
def test_perm_scatters_the_plain_result(G, device, row, bits):
    K, N, gs = row
    c = R.dyadic_bwd_case(bits, K, N, gs, max(R.BWD_MS), perm=True, seed=2, dy_dtype="bf16" if bits & 1 else "f16")
    qw, s, z = _operands(c, device)
    perm = R.dev(c.perm, device)
    for m in R.BWD_MS:
        dy = c.dy[:m].to(device)
        for yd in ("f32", c.dy_dtype):
            plain = G.quant_matmul_t(dy, qw, s, z, bits, gs, out_dtype=DT[yd])
            want = torch.empty_like(plain)
            want[:, perm.long()] = plain
            got = G.quant_matmul_t(dy, qw, s, z, bits, gs, out_dtype=DT[yd], perm=perm)
            R.assert_equal_bits(got, want, f"perm {bits}-bit {K}x{N} g{gs} M={m} y {yd}")
            R.assert_equal_bits(got, R.round_to(c.ref[:m], yd).to(device), f"perm vs reference {bits}-bit M={m} y {yd}")


def test_perm_without_groups_raises(G, device):
    from gptq_amd import _lib
    c = _dyadic(4, 160, 100, -1, "f16")
    qw, s, z = _operands(c, device)
    perm = torch.arange(160, dtype=torch.int32, device=device)
    dy = c.dy[:3].to(device)
    with pytest.raises(ValueError):
        G.quant_matmul_t(dy, qw, s, z, 4, -1, perm=perm)
    dx = torch.full((3, 160), 7.0, device=device)
    with pytest.raises(_lib.GptqHipError, match="perm needs grouped grids"):
        _lib.call("gptq_quant_gemm_t", _lib.ptr(dy), _lib.F16, 100, 3, _lib.ptr(qw), _lib.ptr(s), _lib.ptr(z), _lib.ptr(perm),
                  160, 100, 4, -1, _lib.ptr(dx), _lib.F32, 160, 0, 0, _lib.stream(device))
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all())


# ------------------------------------------------------------------------------------------------ tolerance
@pytest.mark.parametrize("dy_dtype,yd", [("f16", "f32"), ("bf16", "bf16")])
@pytest.mark.parametrize("M", [1, 64])
@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("kind", R.BWD_KINDS)
def test_realistic_inputs_stay_within_the_derived_bar(G, device, kind, bits, M, dy_dtype, yd):
    K, N, gs = 256, 264, 64
    c = R.realistic_bwd_case(kind, bits, K, N, gs, M, seed=5, dy_dtype=dy_dtype)
    qw, s, z = _operands(c, device)
    got = G.quant_matmul_t(c.dy.to(device), qw, s, z, bits, gs, out_dtype=DT[yd]).double().cpu().numpy()
    err = np.abs(got - c.ref)
    bar = R.derived_bar(c.ref, c.T, N, yd)
    worst = float((err / bar).max())
    print(f"{kind} {bits}-bit M={M} dy {dy_dtype} y {yd}: worst err / bar = {worst:.3g}")
    assert np.isfinite(got).all() and (err <= bar).all(), worst


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("M", [1, 130])
def test_two_calls_give_the_same_bits(G, device, M):
    for bits, dy_dtype in ((3, "f16"), (4, "bf16")):
        c = R.realistic_bwd_case("randn", bits, 256, 264, 64, M, seed=6, dy_dtype=dy_dtype)
        qw, s, z = _operands(c, device)
        dy = c.dy.to(device)
        a = G.quant_matmul_t(dy, qw, s, z, bits, 64, out_dtype=torch.float32)
        b = G.quant_matmul_t(dy, qw, s, z, bits, 64, out_dtype=torch.float32)
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_return_before_any_launch(G, device):
    from gptq_amd import _lib
    K, N, bits, gs, M = 256, 264, 4, 64, 1
    c = _dyadic(bits, K, N, gs, "f16")
    qw, s, z = _operands(c, device)
    dy = c.dy[:M].to(device)
    dx = torch.full((M, K), 7.0, device=device)
    nbytes = _lib.load().gptq_quant_gemm_t_workspace_bytes(M, K, N, bits, gs)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)

    def call(dy_ptr=_lib.ptr(dy), dy_dtype=_lib.F16, lddy=N, qw_ptr=_lib.ptr(qw), s_ptr=_lib.ptr(s), z_ptr=_lib.ptr(z),
             k=K, dx_ptr=_lib.ptr(dx), dx_dtype=_lib.F32, lddx=K, ws_ptr=_lib.ptr(ws), ws_bytes=nbytes, b=bits, g=gs):
        _lib.call("gptq_quant_gemm_t", dy_ptr, dy_dtype, lddy, M, qw_ptr, s_ptr, z_ptr, 0, k, N, b, g, dx_ptr, dx_dtype,
                  lddx, ws_ptr, ws_bytes, _lib.stream(device))

    bad = [dict(dy_dtype=_lib.F32), dict(k=K + 16), dict(ws_bytes=nbytes - 1), dict(ws_ptr=0), dict(dy_ptr=0),
           dict(qw_ptr=0), dict(s_ptr=0), dict(z_ptr=0), dict(dx_ptr=0), dict(lddy=N - 1), dict(lddx=K - 1),
           dict(dx_dtype=5), dict(b=5), dict(g=48)]
    for kw in bad:
        with pytest.raises(_lib.GptqHipError, match="invalid argument"):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all())                         # nothing ran
    with pytest.raises(ValueError):
        G.quant_matmul_t(dy.float(), qw, s, z, bits, gs)
    call()                                                 # and the good call runs
    R.assert_equal_bits(dx, R.round_to(c.ref[:M], "f32").to(device), "raw call")


# ------------------------------------------------------------------------------------------------ autograd
def _module(G, device, kind):
    """A 64 -> 40 packed Linear with realistic 4-bit weights, its operands for quant_matmul_t and the case."""
    K, N = 64, 40
    gs = -1 if kind == "row" else 32
    c = R.realistic_bwd_case("randn", 4, K, N, gs, 1, seed=7)
    qw, s, z = _operands(c, device)
    bias = R.dev(c.bias, device)
    perm = None
    if kind == "row":
        m = G.Quant4Linear(K, N, multi_token=True).to(device)
        m.qweight, m.scales, m.zeros, m.bias = qw, s.reshape(-1, 1), z.reshape(-1, 1), bias
    else:
        m = G.QuantGroupLinear(4, gs, K, N, multi_token=True, act_order=kind == "act").to(device)
        m.qweight, m.scales, m.zeros, m.bias = qw, s, z, bias
        if kind == "act":
            perm = torch.from_numpy(np.random.default_rng(8).permutation(K).astype(np.int32)).to(device)
            m.perm = perm
    return m, (qw, s, z, 4, gs), perm, c


@pytest.mark.parametrize("kind", ["row", "group", "act"])
def test_x_grad_through_a_packed_linear(G, device, kind):
    m, (qw, s, z, bits, gs), perm, c = _module(G, device, kind)
    K, N, M = 64, 40, 5
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((M, K)).astype(np.float32)).to(device).half()
    with torch.no_grad():
        y0 = m(x)
    assert y0.grad_fn is None
    xg = x.clone().requires_grad_()
    y = m(xg)
    assert y.grad_fn is not None and torch.equal(y, y0)    # the no_grad forward, bit for bit
    y.sum().backward()
    assert xg.grad is not None and xg.grad.dtype == x.dtype and xg.grad.shape == x.shape
    ones = torch.ones(M, N, dtype=x.dtype, device=device)
    assert torch.equal(xg.grad, G.quant_matmul_t(ones, qw, s, z, bits, gs, perm=perm))
    ref, T = R.ref_dx64(np.ones((M, N)), c.qweight, c.scales, c.zeros, bits, gs,
                        None if perm is None else perm.cpu().numpy(), "f16")
    err = np.abs(xg.grad.double().cpu().numpy() - ref)
    assert (err <= R.derived_bar(ref, T, N, "f16")).all(), float(err.max())
    # quant_matmul itself routes the same way
    xg2 = x.clone().requires_grad_()
    y2 = G.quant_matmul(xg2, qw, s, z, bits, gs, bias=m.bias, perm=perm)
    assert torch.equal(y2, y0)
    (y2 * 2).sum().backward()
    assert torch.equal(xg2.grad, G.quant_matmul_t(2 * ones, qw, s, z, bits, gs, perm=perm))


@pytest.mark.parametrize("kind", ["row", "group", "act"])
@pytest.mark.parametrize("shape", [(64,), (1, 64), (1, 1, 64)])
def test_single_token_inputs_get_a_grad(G, device, kind, shape):
    m, (qw, s, z, bits, gs), perm, c = _module(G, device, kind)
    N = 40
    x = torch.from_numpy(np.random.default_rng(10).standard_normal(shape).astype(np.float32)).to(device).half()
    with torch.no_grad():
        y0 = m(x)
    xg = x.clone().requires_grad_()
    y = m(xg)
    assert torch.equal(y, y0) and y.shape == y0.shape       # the mat-vec path, as without autograd
    w = torch.from_numpy(np.random.default_rng(11).integers(-4, 5, N).astype(np.float32)).to(device).half()
    (y * w).sum().backward()
    assert xg.grad.shape == x.shape and xg.grad.dtype == x.dtype
    want = G.quant_matmul_t(w, qw, s, z, bits, gs, perm=perm)
    assert want.shape == (64,)
    assert torch.equal(xg.grad.reshape(-1), want)
    ref, T = R.ref_dx64(w.double().cpu().numpy().reshape(1, N), c.qweight, c.scales, c.zeros, bits, gs,
                        None if perm is None else perm.cpu().numpy(), "f16")
    err = np.abs(xg.grad.double().cpu().numpy().reshape(1, -1) - ref)
    assert (err <= R.derived_bar(ref, T, N, "f16")).all()


def test_fp32_activations_that_require_grad_raise(G, device):
    for kind in ("row", "group"):
        m = _module(G, device, kind)[0]
        for shape in ((64,), (3, 64)):
            x = torch.zeros(shape, device=device, requires_grad=True)
            with pytest.raises(ValueError, match="backward through packed Linears needs fp16/bf16 activations"):
                m(x)
        y = m(torch.zeros(64, device=device))               # without autograd fp32 single tokens work as before
        assert y.dtype == torch.float32 and y.grad_fn is None


def test_adapter_training_step_leaves_the_packed_buffers_alone(G, device):
    m, _, _, _ = _module(G, device, "act")
    K, N, r = 64, 40, 4
    torch.manual_seed(0)
    A = torch.nn.Linear(K, r, bias=False).to(device).half()
    B = torch.nn.Linear(r, N, bias=False).to(device).half()
    emb = torch.nn.Parameter(torch.randn(6, K, device=device).half())    # an upstream trainable: needs grad THROUGH the packed Linear
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert not list(m.parameters())
    h = emb * 1.0
    y = m(h) + B(A(h))
    y.float().pow(2).mean().backward()
    for g in (A.weight.grad, B.weight.grad, emb.grad):
        assert g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any())
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    # the packed path contributes to emb.grad: without it the gradient differs
    emb2 = torch.nn.Parameter(emb.detach().clone())
    h2 = emb2 * 1.0
    A.weight.grad = B.weight.grad = None
    (m(h2.detach()) + B(A(h2))).float().pow(2).mean().backward()
    assert not torch.equal(emb.grad, emb2.grad)
