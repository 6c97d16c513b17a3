"""The int8-activation packed GEMM on the GPU (quantize_activations, quant_matmul_a8, set_act_bits): the activation
quantization is bit-exact against the CPU formula, the GEMM EQUALS the fp64 reference on the exact-case table of
packed_a8_ref and stays inside a derived bar on realistic inputs, and the modules route exactly as documented."""
import io

import numpy as np
import pytest
import torch

import packed_a8_ref as A8
import packed_ref as R0

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def G():
    import gptq_amd
    return gptq_amd


# ------------------------------------------------------------------------------------------------ raw C ABI helpers
def _guarded(n, dtype, dev, off, fill):
    """A buffer of n elements at an element offset `off` inside a larger sentinel-filled one: (whole, view)."""
    whole = torch.full((n + off + 64,), fill, dtype=dtype, device=dev)
    return whole, whole[off:off + n]


def _outside_untouched(whole, off, n, fill, rows=None, ld=None, width=None):
    keep = torch.ones(whole.numel(), dtype=torch.bool, device=whole.device)
    if rows is None:
        keep[off:off + n] = False
    else:
        for r in range(rows):
            keep[off + r * ld:off + r * ld + width] = False
    return bool((whole[keep] == fill).all())


def raw_quant(x2, M, K, ldx, perm, ldq, q_off):
    """gptq_quant_act_rows on a strided x view; returns xq [M, K], sx [M] and whether every byte outside them kept its
    sentinel."""
    from gptq_amd import _lib
    dev = x2.device
    qwhole, qv = _guarded(M * ldq, torch.int8, dev, q_off, 77)
    swhole, sv = _guarded(M, torch.float32, dev, 1, -5.0)
    _lib.call("gptq_quant_act_rows", x2.data_ptr(), _lib.dtype_code(x2), ldx, M, K, _lib.ptr(perm), qv.data_ptr(), ldq,
              sv.data_ptr(), _lib.stream(dev))
    torch.cuda.synchronize()
    ok = _outside_untouched(qwhole, q_off, M * ldq, 77, rows=M, ld=ldq, width=K) and _outside_untouched(swhole, 1, M, -5.0)
    return qv.view(M, ldq)[:, :K].clone(), sv.clone(), ok


def special_rows(M, K, dtype):
    """[M, K] CPU activations: randn * 3 with an all-zero row, a row holding the largest finite value, a row of fp16 subnormals (bf16: 2^-100),
    a row with -0.0 and a row whose x / sx lands exactly on k + 0.5 (sx = 2^-3), as far as M has rows for them."""
    g = torch.Generator().manual_seed(1000 * M + K)
    x = (torch.randn(M, K, generator=g) * 3).to(dtype)
    big = 65504.0 if dtype == torch.float16 else 3.3895313892515355e38
    tiny = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -100          # fp16: its smallest subnormal
    rows = []
    z = torch.zeros(K, dtype=dtype)
    rows.append(z.clone())
    r = x[0].clone(); r[K // 2] = big; rows.append(r)
    rows.append((torch.arange(K) % 7 - 3).to(dtype) * tiny)
    r = x[0].clone(); r[::3] = -0.0; rows.append(r)
    r = z.clone(); r[0] = 127 * 0.125; r[1:12] = (torch.arange(-5, 6).to(torch.float32) + 0.5).to(dtype) * 0.125; rows.append(r)
    for i, r in enumerate(rows[:max(0, M - 1)]):                          # (row 0 of x stays random)
        x[1 + i] = r
    return x


# ------------------------------------------------------------------------------------------------ 1. act quant
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("K", [32, 96, 4128, 8224])                       # 8224: past the rows a thread keeps in registers
@pytest.mark.parametrize("M", [1, 3, 65])
def test_act_quant_bit_exact(G, hip_device, M, K, dtype):
    x = special_rows(M, K, dtype)
    wq, ws = A8.quantize_ref(x)
    xq, sx = G.quantize_activations(x.to(hip_device))
    assert xq.dtype == torch.int8 and sx.dtype == torch.float32 and xq.shape == (M, K) and sx.shape == (M,)
    assert torch.equal(sx.cpu(), ws) and torch.equal(xq.cpu(), wq)
    # ldx > K, a base pointer that is only 2-byte aligned, ldq > K at an odd byte offset; sentinels stay
    ldx = K + 24
    buf = torch.zeros(M * ldx + 8, dtype=dtype, device=hip_device)
    xv = buf[1:1 + M * ldx].view(M, ldx)
    xv[:, :K] = x.to(hip_device)
    xv[:, K:] = 1e4                                                        # must not leak into the row maximum
    rq, rs, ok = raw_quant(xv, M, K, ldx, None, K + 16, 3)
    assert ok and torch.equal(rs.cpu(), ws) and torch.equal(rq.cpu(), wq)
    # perm: equals the call on x[:, perm]
    p = torch.randperm(K, generator=torch.Generator().manual_seed(K)).to(torch.int32)
    wqp, wsp = A8.quantize_ref(x[:, p.long()])
    pq, ps = G.quantize_activations(x.to(hip_device), perm=p.to(hip_device))
    assert torch.equal(ps.cpu(), wsp) and torch.equal(pq.cpu(), wqp)
    gq, gs_ = G.quantize_activations(x[:, p.long()].contiguous().to(hip_device))
    assert torch.equal(pq, gq) and torch.equal(ps, gs_)
    if M == 3:                                                             # leading dimensions of x are kept
        q3, s3 = G.quantize_activations(x.to(hip_device).reshape(1, M, K))
        assert q3.shape == (1, M, K) and s3.shape == (1, M) and torch.equal(q3.reshape(M, K).cpu(), wq)


# ------------------------------------------------------------------------------------------------ 2. exact GEMM
@pytest.mark.parametrize("bits", A8.BITS)
@pytest.mark.parametrize("row", A8.GEMM_EXACT, ids=A8.case_id)
def test_gemm_exact_on_dyadic_inputs(G, hip_device, row, bits):
    K, N, gs, Ms, odt, with_bias, form, j = row
    c = A8.dyadic_case(bits, K, N, gs, max(Ms), j=j, perm=False, seed=3)
    qw, s, z, b, _ = R0.dev_tensors(c, hip_device)
    ref = torch.from_numpy(c.ref if with_bias else c.ref - c.bias.astype(np.float64)[None, :]).to(hip_device)
    for m in Ms:
        tag = f"{bits}-bit {K}x{N} g{gs} M={m} {odt} {form}"
        if form == "x":
            xin = c.x[:m].to(hip_device)
        else:
            xin = (torch.from_numpy(c.xq[:m]).to(hip_device), torch.from_numpy(c.sx[:m]).to(hip_device))
        y = G.quant_matmul_a8(xin, qw, s, z, bits, gs, bias=b if with_bias else None, out_dtype=DT[odt])
        assert y.dtype == DT[odt] and y.shape == (m, N)
        A8.assert_equal_bits(y, ref[:m].float().to(DT[odt]), tag)
        y2 = G.quant_matmul_a8(xin, qw, s, z, bits, gs, bias=b if with_bias else None, out_dtype=DT[odt])
        A8.assert_equal_bits(y2, y, tag + " second call")
        if form == "x":                                                    # default output type: x's
            yd = G.quant_matmul_a8(xin, qw, s, z, bits, gs, bias=b if with_bias else None)
            A8.assert_equal_bits(yd, ref[:m].float().to(xin.dtype), tag + " default dtype")


RAW = [(1056, 257, -1, 17), (1056, 257, -1, 1), (1056, 520, 32, 1), (160, 7, 160, 129), (1056, 7, 96, 65), (96, 64, 32, 33)]


@pytest.mark.parametrize("bits", A8.BITS)
@pytest.mark.parametrize("shape", RAW, ids=lambda t: "x".join(map(str, t)))
def test_gemm_raw_abi_strides_alignment_and_sentinels(hip_device, shape, bits):
    """ldq > K, ldy > N, xq / qweight / y at misaligned addresses, a workspace of exactly the queried size: y equals the
    reference and every sentinel round y, xq, sx and the workspace is untouched."""
    from gptq_amd import _lib
    K, N, gs, M = shape
    dev = hip_device
    c = A8.dyadic_case(bits, K, N, gs, M, j=3, seed=9)
    _, s, z, b, _ = R0.dev_tensors(c, dev)
    ldq, ldy = K + 48, N + 5
    qwhole, qv = _guarded(M * ldq, torch.int8, dev, 5, 99)
    qv.view(M, ldq)[:, :K] = torch.from_numpy(c.xq).to(dev)
    swhole, sv = _guarded(M, torch.float32, dev, 1, -7.0)
    sv.copy_(torch.from_numpy(c.sx))
    wwhole, wv = _guarded(c.qweight.size, torch.int32, dev, 1, 0x5a5a5a5a)  # 4-byte aligned only: no 16-byte loads
    wv.copy_(torch.from_numpy(c.qweight).reshape(-1))
    ywhole, yv = _guarded(M * ldy, torch.float32, dev, 1, -123.0)
    nbytes = _lib.load().gptq_quant_gemm_a8_workspace_bytes(M, K, N, bits, gs)
    kwhole, kv = _guarded(nbytes // 4, torch.int32, dev, 4, 0x3c3c3c3c)
    q0, s0, w0 = qwhole.clone(), swhole.clone(), wwhole.clone()
    _lib.call("gptq_quant_gemm_a8", qv.data_ptr(), ldq, sv.data_ptr(), M, wv.data_ptr(), _lib.ptr(s), _lib.ptr(z),
              _lib.ptr(b), K, N, bits, gs, yv.data_ptr(), _lib.F32, ldy, kv.data_ptr() if nbytes else 0, nbytes,
              _lib.stream(dev))
    torch.cuda.synchronize()
    A8.assert_equal_bits(yv.view(M, ldy)[:, :N], torch.from_numpy(c.ref).float().to(dev), f"raw {bits}-bit {shape}")
    assert _outside_untouched(ywhole, 1, M * ldy, -123.0, rows=M, ld=ldy, width=N)
    assert torch.equal(qwhole, q0) and torch.equal(swhole, s0) and torch.equal(wwhole, w0)
    assert _outside_untouched(kwhole, 4, nbytes // 4, 0x3c3c3c3c)


# ------------------------------------------------------------------------------------------------ 3. magnitude guard
def test_magnitude_guard_exact_and_refused_past_it(G, hip_device):
    from gptq_amd import _lib
    dev = hip_device
    K, N, M = 65536, 64, 16
    qw = torch.full((K // 4, N), -1, dtype=torch.int32, device=dev)        # every code 255
    xq = torch.full((M, K), -127, dtype=torch.int8, device=dev)
    sx = torch.ones(M, device=dev)
    s, z = torch.full((N,), 2.0 ** -8, device=dev), torch.zeros(N, device=dev)
    y = G.quant_matmul_a8((xq, sx), qw, s, z, 8, out_dtype=torch.float32)
    want = float(-32385 * 2 ** 16) * 2.0 ** -8                             # I = -32385 * 2^16 is an fp32 number
    assert float(np.float32(-32385 * 2 ** 16)) == -32385 * 2 ** 16
    A8.assert_equal_bits(y, torch.full((M, N), want, device=dev), "K = 65536, all codes 255, all xq -127")
    K2 = 65568
    qw2 = torch.zeros((K2 // 4, N), dtype=torch.int32, device=dev)
    xq2 = torch.zeros((M, K2), dtype=torch.int8, device=dev)
    with pytest.raises(ValueError):
        G.quant_matmul_a8((xq2, sx), qw2, s, z, 8)
    with pytest.raises(ValueError):
        G.quant_matmul_a8(torch.zeros((M, K2), dtype=torch.float16, device=dev), qw2, s, z, 8)
    yb = torch.full((M, N), -3.0, device=dev)
    with pytest.raises(_lib.GptqHipError, match="invalid argument"):        # the C ABI refuses before any launch
        _lib.call("gptq_quant_gemm_a8", xq2.data_ptr(), K2, sx.data_ptr(), M, qw2.data_ptr(), s.data_ptr(), z.data_ptr(), 0,
                  K2, N, 8, -1, yb.data_ptr(), _lib.F32, N, 0, 0, _lib.stream(dev))
    torch.cuda.synchronize()
    assert bool((yb == -3.0).all())


# ------------------------------------------------------------------------------------------------ 4. realistic inputs
@pytest.mark.parametrize("kind", A8.REALISTIC_KINDS)
@pytest.mark.parametrize("bits,gs", [(4, 128), (3, 32), (8, -1)], ids=["4g128", "3g32", "8row"])
def test_gemm_realistic_inside_the_derived_bar(G, hip_device, bits, gs, kind):
    """|y - ref| <= c T + u |ref| against the fp64 formula on the kernel's own (xq, sx); c = (4 G + 4) 2^-24 counts the
    fp32 operations of the contract (packed_a8_ref.realistic_bar), u = 2^-24 for the fp32 output.  Not a measured bar."""
    K, N, M = 4096, 520, 33
    c = A8.realistic_case(kind, bits, K, N, gs, M, seed=2)
    qw, s, z, b, _ = R0.dev_tensors(c, hip_device)
    x = c.x.to(hip_device)
    xq, sx = G.quantize_activations(x)
    wq, ws = A8.quantize_ref(c.x)
    assert torch.equal(sx.cpu(), ws) and torch.equal(xq.cpu(), wq)
    ref, bar = A8.realistic_bar(c, xq.cpu().numpy(), sx.cpu().numpy(), 2.0 ** -24)
    y = G.quant_matmul_a8((xq, sx), qw, s, z, bits, gs, bias=b, out_dtype=torch.float32)
    err = np.abs(y.double().cpu().numpy() - ref)
    worst = float((err / bar).max())
    print(f"a8 realistic {bits}-bit g{gs} {kind}: worst error / bar = {worst:.3f}")
    assert worst <= 1.0
    y2 = G.quant_matmul_a8(x, qw, s, z, bits, gs, bias=b, out_dtype=torch.float32)
    assert torch.equal(y2, y)                                              # the tensor form is the pair form


# ------------------------------------------------------------------------------------------------ 5. act-order
@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("gs", [32, 128])
def test_act_order_equals_the_gathered_call(G, hip_device, gs, bits):
    K, N = 256, 72
    c = A8.realistic_case("mean3", bits, K, N, gs, 130, seed=4)
    qw, s, z, b, _ = R0.dev_tensors(c, hip_device)
    p = torch.randperm(K, generator=torch.Generator().manual_seed(gs)).to(torch.int32).to(hip_device)
    for m in (1, 17, 130):
        x = c.x[:m].to(hip_device)
        y = G.quant_matmul_a8(x, qw, s, z, bits, gs, bias=b, perm=p)
        yg = G.quant_matmul_a8(x[:, p.long()].contiguous(), qw, s, z, bits, gs, bias=b)
        assert torch.equal(y, yg), (gs, bits, m)


# ------------------------------------------------------------------------------------------------ 6. modules
def _stack(G, dev, multi_token=True):
    """A per-row 4-bit Linear 128 -> 96 and an act-order 3-bit g32 QuantGroupLinear 96 -> 40, filled from reference-side
    packed buffers."""
    c1 = A8.realistic_case("randn", 4, 128, 96, -1, 1, seed=11)
    c2 = A8.realistic_case("randn", 3, 96, 40, 32, 1, seed=12)
    l1 = G.Quant4Linear(128, 96, multi_token=multi_token)
    l2 = G.QuantGroupLinear(3, 32, 96, 40, multi_token=multi_token, act_order=True)
    l1.qweight = torch.from_numpy(c1.qweight)
    l1.scales, l1.zeros = torch.from_numpy(c1.scales).reshape(-1, 1), torch.from_numpy(c1.zeros).reshape(-1, 1)
    l1.bias = torch.from_numpy(c1.bias)
    l2.qweight = torch.from_numpy(c2.qweight)
    l2.scales, l2.zeros, l2.bias = torch.from_numpy(c2.scales), torch.from_numpy(c2.zeros), torch.from_numpy(c2.bias)
    l2.perm = torch.randperm(96, generator=torch.Generator().manual_seed(5)).to(torch.int32)
    return torch.nn.Sequential(l1, l2).to(dev)


def test_modules_route_int8_activations_only_where_documented(G, hip_device):
    dev = hip_device
    model = _stack(G, dev)
    l1, l2 = model
    keys = sorted(model.state_dict())
    g = torch.Generator().manual_seed(6)
    x = torch.randn(5, 128, generator=g).to(torch.float16).to(dev)
    x1 = x[:1].clone()
    with torch.no_grad():
        base, base1 = model(x), model(x1)                                  # today's outputs
    xg = x.clone().requires_grad_()
    base_g = model(xg)
    assert G.set_act_bits(model, 8) == 2
    with torch.no_grad():
        y = model(x)
        h = G.quant_matmul_a8(x, l1.qweight, l1.scales, l1.zeros, 4, -1, l1.bias)
        want = G.quant_matmul_a8(h, l2.qweight, l2.scales, l2.zeros, 3, 32, l2.bias, perm=l2.perm)
        assert torch.equal(y, want)
        assert not torch.equal(y, base)                                    # the int8 route really is taken
        rel = float((y.float() - base.float()).norm() / base.float().norm())
        assert rel < 0.05, rel                                             # ... and it is the same layer
        assert torch.equal(model(x1), base1)                               # a single token stays on the mat-vec
        y3 = model(x.reshape(1, 5, 128))
        assert y3.shape == (1, 5, 40) and torch.equal(y3.reshape(5, 40), y)
    yg = model(xg)                                                         # under autograd: today's fp16 path
    assert yg.grad_fn is not None and torch.equal(yg.detach(), base_g.detach())
    assert sorted(model.state_dict()) == keys
    # save / reload: act_bits is no state; a reloaded skeleton switched on scores bit-identically
    buf = io.BytesIO()
    torch.save(model.state_dict(), buf)
    buf.seek(0)
    fresh = _stack(G, dev, multi_token=False)
    for mod in fresh:
        mod.qweight.zero_()
    fresh.load_state_dict(torch.load(buf))
    assert G.set_multi_token(fresh) == 2 and all(m.act_bits is None for m in fresh)
    with torch.no_grad():
        assert torch.equal(fresh(x), base)
        G.set_act_bits(fresh, 8)
        assert torch.equal(fresh(x), y)
    assert G.set_act_bits(model, None) == 2
    with torch.no_grad():
        assert torch.equal(model(x), base) and torch.equal(model(x1), base1)
    assert torch.equal(model(xg).detach(), base_g.detach())


# ------------------------------------------------------------------------------------------------ 7. argument errors
def test_argument_errors_before_any_launch(G, hip_device):
    dev = hip_device
    K, N = 64, 16
    x = torch.zeros(3, K, dtype=torch.float16, device=dev)
    qw = torch.zeros(K // 32 * 4, N, dtype=torch.int32, device=dev)
    s, z = torch.ones(N, device=dev), torch.zeros(N, device=dev)
    sg, zg = torch.ones(2, N, device=dev), torch.zeros(2, N, device=dev)
    xq, sx = torch.zeros(3, K, dtype=torch.int8, device=dev), torch.ones(3, device=dev)
    p = torch.arange(K, dtype=torch.int32, device=dev)
    bad = [
        lambda: G.quant_matmul_a8(x.float(), qw, s, z, 4),                               # wrong dtypes
        lambda: G.quant_matmul_a8((xq.to(torch.int16), sx), qw, s, z, 4),
        lambda: G.quant_matmul_a8((xq, sx.double()), qw, s, z, 4),
        lambda: G.quant_matmul_a8(x, qw.to(torch.int64), s, z, 4),
        lambda: G.quant_matmul_a8(x, qw, s, z, 4, out_dtype=torch.float64),
        lambda: G.quant_matmul_a8(x, qw, s, z, 5),
        lambda: G.quantize_activations(x.float()),
        lambda: G.quantize_activations(torch.zeros(3, 48, dtype=torch.float16, device=dev)),   # K % 32
        lambda: G.quant_matmul_a8(torch.zeros(3, 48, dtype=torch.float16, device=dev),
                                  torch.zeros(6, N, dtype=torch.int32, device=dev), s, z, 4),
        lambda: G.quant_matmul_a8((xq, sx[:2]), qw, s, z, 4),                            # mismatched (xq, sx)
        lambda: G.quant_matmul_a8((xq, sx.reshape(3, 1)), qw, s, z, 4),
        lambda: G.quant_matmul_a8(x, qw, s, z, 4, perm=p),                               # perm with per-row grids
        lambda: G.quant_matmul_a8((xq, sx), qw, sg, zg, 4, 32, perm=p),                  # perm with the pair
        lambda: G.quant_matmul_a8(x, qw, sg, zg, 4, 32, perm=p[:32]),
        lambda: G.quant_matmul_a8(x, qw, sg, zg, 4, 48),                                 # groupsize
        lambda: G.quant_matmul_a8(x, qw, s[:8], z[:8], 4),
        lambda: G.quant_matmul_a8(x, qw, s, z, 4, bias=torch.zeros(N + 1, device=dev)),
        lambda: G.quant_matmul_a8(x.clone().requires_grad_(), qw, s, z, 4),              # requires_grad
        lambda: G.quant_matmul_a8(x, qw, s.clone().requires_grad_(), z, 4),
        lambda: G.quant_matmul_a8(x, qw, s, z, 4, bias=torch.zeros(N, device=dev).requires_grad_()),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} did not raise")
    with torch.no_grad():                                                  # a grad-requiring x is fine without grad mode
        G.quant_matmul_a8(x.clone().requires_grad_(), qw, s, z, 4)
    assert G.quant_matmul_a8(torch.zeros(0, K, dtype=torch.float16, device=dev), qw, s, z, 4).shape == (0, N)
