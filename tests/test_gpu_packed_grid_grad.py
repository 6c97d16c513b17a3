"""The grid gradients of the packed Linears on the GPU: gptq_quant_gemm_grid_grad / quant_grid_grad against
tests/packed_grid_ref.py (bit for bit on dyadic inputs, within the derived bar on realistic ones), autograd for `scales`,
`zeros` and `bias` through the modules, and `trainable_grids` / `frozen_grids`."""
import functools

import numpy as np
import pytest
import torch

import packed_grid_ref as R

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
def _dyadic(bits, K, N, gs, perm=False):
    """One case per (row, width), shared by both 16-bit types: its values are exact in either."""
    return R.dyadic_grid_case(bits, K, N, gs, max(R.GRID_MS), perm=perm, seed=2 if perm else 1)


@functools.lru_cache(maxsize=None)
def _dyadic_ref(bits, K, N, gs, perm, m):
    c = _dyadic(bits, K, N, gs, perm)
    return R.ref_grid_grad64(c.x[:m], c.dy[:m], c.qweight, bits, gs, c.perm)[:3]


def _f32(a, device):
    return torch.from_numpy(np.asarray(a, dtype=np.float64).astype(np.float32)).to(device)


def _check_exact(got, want, device, what):
    for name, g, w in zip(("dscales", "dzeros", "dbias"), got, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == w.shape, (what, name, tuple(g.shape), w.shape)
        R.assert_equal_bits(g, _f32(w, device), f"{name} {what}")


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("dtype", R.GRID_DT)
@pytest.mark.parametrize("bits", R.BITS)
@pytest.mark.parametrize("row", R.GRID_EXACT, ids=[R.grid_case_id(r) for r in R.GRID_EXACT])
def test_grid_grads_equal_the_reference_on_dyadic_inputs(G, device, row, bits, dtype):
    K, N, gs = row
    c = _dyadic(bits, K, N, gs)
    qw = R.dev(c.qweight, device)
    x, dy = c.x.to(device=device, dtype=DT[dtype]), c.dy.to(device=device, dtype=DT[dtype])
    for m in R.GRID_MS:
        got = G.quant_grid_grad(x[:m], dy[:m], qw, bits, gs)
        _check_exact(got, _dyadic_ref(bits, K, N, gs, False, m), device, f"{bits}-bit {K}x{N} g{gs} M={m} {dtype}")
    ds, dz, db = G.quant_grid_grad(x[:3], dy[:3], qw, bits, gs, bias=False)
    assert db is None
    _check_exact((ds, dz), _dyadic_ref(bits, K, N, gs, False, 3)[:2], device, f"no bias {bits}-bit {K}x{N} g{gs}")


def test_the_table_reaches_the_split_path():
    from gptq_amd import _lib
    q = _lib.load().gptq_quant_gemm_grid_grad_workspace_bytes
    for bits in R.BITS:
        sizes = {(K, N, gs, m): q(m, K, N, bits, gs) for K, N, gs in R.GRID_EXACT for m in R.GRID_MS}
        assert any(v == 0 for v in sizes.values()) and any(v > 0 for v in sizes.values()), bits
        # one pass: a group is one segment of its K tile and the tokens are one chunk
        assert sizes[(256, 264, 64, 17)] == 0 and sizes[(256, 40, 128, 17)] == 0 and sizes[(160, 100, 32, 1)] == 0
        # reduced over K tiles / segments: per-row grids, and a grouped grid of 3 segments per group (two arrays of
        # partials, each rounded up to 256 bytes)
        for key, partials in (((256, 264, -1, 17), 256 // 128), ((192, 24, 96, 17), 192 // 32)):
            one = partials * key[1] * 4
            assert 2 * one <= sizes[key] < 2 * one + 512, (key, sizes[key])
        # reduced over token chunks: M = 130 is two chunks (dscales, dzeros and dbias partials)
        one = 2 * (256 // 64) * 264 * 4
        assert 2 * one + 2 * 264 * 4 <= sizes[(256, 264, 64, 130)] < 2 * one + 2 * 264 * 4 + 768


# ------------------------------------------------------------------------------------------------ perm
@pytest.mark.parametrize("bits", R.BITS)
@pytest.mark.parametrize("row", R.GRID_PERM, ids=R.grid_case_id)
def test_perm_equals_the_plain_call_on_gathered_x(G, device, row, bits):
    K, N, gs = row
    c = _dyadic(bits, K, N, gs, True)
    dtype = "bf16" if bits & 1 else "f16"
    qw, perm = R.dev(c.qweight, device), R.dev(c.perm, device)
    x, dy = c.x.to(device=device, dtype=DT[dtype]), c.dy.to(device=device, dtype=DT[dtype])
    for m in R.GRID_MS:
        got = G.quant_grid_grad(x[:m], dy[:m], qw, bits, gs, perm=perm)
        plain = G.quant_grid_grad(x[:m][:, perm.long()], dy[:m], qw, bits, gs)
        for a, b in zip(got, plain):
            assert torch.equal(a, b), (bits, row, m)
        _check_exact(got, _dyadic_ref(bits, K, N, gs, True, m), device, f"perm {bits}-bit {K}x{N} g{gs} M={m}")


# ------------------------------------------------------------------------------------------------ tolerance
@pytest.mark.parametrize("dtype", R.GRID_DT)
@pytest.mark.parametrize("M", [1, 64])
@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("gs", [64, -1])
@pytest.mark.parametrize("kind", R.GRID_KINDS)
def test_realistic_inputs_stay_within_the_derived_bar(G, device, kind, gs, bits, M, dtype):
    K, N = 256, 264
    c = R.realistic_grid_case(kind, bits, K, N, gs, M, seed=5, dtype=dtype)
    got = G.quant_grid_grad(c.x.to(device), c.dy.to(device), R.dev(c.qweight, device), bits, gs)
    worst = 0.0
    for name, g, ref, bar in zip(("dS", "dZ", "dB"), got, (c.dS, c.dZ, c.dB), (c.bar_S, c.bar_Z, c.bar_B)):
        g = g.double().cpu().numpy()
        assert g.shape == ref.shape and np.isfinite(g).all(), name
        err = np.abs(g - ref)
        ratio = float((err / np.maximum(bar, 1e-300)).max())
        print(f"{kind} {bits}-bit g{gs} M={M} {dtype} {name}: worst err / bar = {ratio:.3g}")
        worst = max(worst, ratio)
        assert (err <= bar).all(), (name, ratio)
    print(f"{kind} {bits}-bit g{gs} M={M} {dtype}: worst err / bar = {worst:.3g}")


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("M", [1, 130])
def test_two_calls_give_the_same_bits(G, device, M):
    for bits, dtype, gs in ((3, "f16", 64), (4, "bf16", -1)):
        c = R.realistic_grid_case("randn", bits, 256, 264, gs, M, seed=6, dtype=dtype)
        x, dy, qw = c.x.to(device), c.dy.to(device), R.dev(c.qweight, device)
        a = G.quant_grid_grad(x, dy, qw, bits, gs)
        b = G.quant_grid_grad(x, dy, qw, bits, gs)
        for u, v in zip(a, b):
            assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_return_before_any_launch(G, device):
    from gptq_amd import _lib
    K, N, bits, gs, M = 256, 264, 4, -1, 3
    c = _dyadic(bits, K, N, gs)
    qw = R.dev(c.qweight, device)
    x, dy = c.x[:M].to(device), c.dy[:M].to(device)
    perm = torch.arange(K, dtype=torch.int32, device=device)
    ds, dz = torch.full((N,), 7.0, device=device), torch.full((N,), 7.0, device=device)
    db = torch.full((N,), 7.0, device=device)
    nbytes = _lib.load().gptq_quant_gemm_grid_grad_workspace_bytes(M, K, N, bits, gs)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)

    def call(x_ptr=_lib.ptr(x), x_dtype=_lib.F16, ldx=K, dy_ptr=_lib.ptr(dy), lddy=N, qw_ptr=_lib.ptr(qw), perm_ptr=0, k=K,
             b=bits, g=gs, ds_ptr=_lib.ptr(ds), dz_ptr=_lib.ptr(dz), ws_ptr=_lib.ptr(ws), ws_bytes=nbytes):
        _lib.call("gptq_quant_gemm_grid_grad", x_ptr, x_dtype, ldx, dy_ptr, lddy, M, qw_ptr, perm_ptr, k, N, b, g, ds_ptr,
                  dz_ptr, _lib.ptr(db), ws_ptr, ws_bytes, _lib.stream(device))

    bad = [dict(x_ptr=0), dict(dy_ptr=0), dict(qw_ptr=0), dict(ds_ptr=0), dict(dz_ptr=0), dict(x_dtype=_lib.F32),
           dict(x_dtype=5), dict(ldx=K - 1), dict(lddy=N - 1), dict(k=K + 16), dict(g=48), dict(g=96), dict(b=5),
           dict(perm_ptr=_lib.ptr(perm)), dict(ws_bytes=nbytes - 1), dict(ws_ptr=0)]
    for kw in bad:
        with pytest.raises(_lib.GptqHipError, match="invalid argument"):
            call(**kw)
    torch.cuda.synchronize()
    for t in (ds, dz, db):
        assert bool((t == 7.0).all())                      # nothing ran
    with pytest.raises(ValueError):
        G.quant_grid_grad(x.float(), dy.float(), qw, bits, gs)
    with pytest.raises(ValueError):
        G.quant_grid_grad(x, dy.bfloat16(), qw, bits, gs)
    with pytest.raises(ValueError):
        G.quant_grid_grad(x, dy, qw, bits, gs, perm=perm)
    call()                                                 # and the good call runs
    _check_exact((ds, dz, db), _dyadic_ref(bits, K, N, gs, False, M), device, "raw call")


def test_no_tokens_give_zero_gradients(G, device):
    qw = torch.zeros((64 // 32 * 4, 40), dtype=torch.int32, device=device)
    x, dy = torch.zeros(0, 64, dtype=torch.float16, device=device), torch.zeros(0, 40, dtype=torch.float16, device=device)
    ds, dz, db = G.quant_grid_grad(x, dy, qw, 4, 32)
    assert ds.shape == (2, 40) and dz.shape == (2, 40) and db.shape == (40,)
    assert not ds.any() and not dz.any() and not db.any()
    x3, dy3 = torch.ones(2, 3, 64, dtype=torch.float16, device=device), torch.ones(2, 3, 40, dtype=torch.float16, device=device)
    ds, dz, db = G.quant_grid_grad(x3, dy3, qw, 4, -1)     # leading dimensions are flattened
    assert ds.shape == (40,) and bool((dz == -6.0 * 64).all()) and bool((db == 6.0).all()) and not ds.any()


# ------------------------------------------------------------------------------------------------ autograd
KINDS = ["row", "group", "act"]


def _module(G, device, kind):
    """A 64 -> 40 packed Linear with realistic 4-bit weights and what quant_grid_grad / the reference need."""
    K, N = 64, 40
    gs = -1 if kind == "row" else 32
    c = R.realistic_grid_case("randn", 4, K, N, gs, 1, seed=7)
    qw, s, z, bias = (R.dev(a, device) for a in (c.qweight, c.scales, c.zeros, c.bias))
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
    return m, gs, perm, c


def _tokens(shape, seed, device):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).to(device).half()


def _check_module_grads(G, m, x, w, gs, perm, c, x_grad):
    """loss = sum(y * w): the grads of the three grid tensors equal quant_grid_grad(x, w) in bits and lie within the derived
    bar of the fp64 reference; x.grad (where asked for) is quant_matmul_t(w) as before."""
    K, N = 64, 40
    with torch.no_grad():
        y0 = m(x)
    assert y0.grad_fn is None
    xin = x.clone().requires_grad_() if x_grad else x
    y = m(xin)
    assert y.grad_fn is not None and torch.equal(y, y0) and y.shape == y0.shape    # the no-grad forward, bit for bit
    (y * w).sum().backward()
    ds, dz, db = G.quant_grid_grad(x, w.expand_as(y).contiguous(), m.qweight, 4, gs, perm=perm)
    M = x.numel() // K
    ref = R.ref_grid_grad64(x.reshape(M, K).cpu(), w.expand_as(y).reshape(M, N).cpu(), c.qweight, 4, gs,
                            None if perm is None else perm.cpu().numpy())
    bars = R.grid_bars(ref[3], ref[4], w.expand_as(y).reshape(M, N).cpu(), M, K, gs)
    for p, g, r64, bar in zip((m.scales, m.zeros, m.bias), (ds, dz, db), ref[:3], bars):
        assert p.grad is not None and p.grad.dtype == torch.float32 and p.grad.shape == p.shape
        assert torch.equal(p.grad, g.reshape(p.shape))
        assert (np.abs(p.grad.double().cpu().numpy().reshape(r64.shape) - r64) <= bar).all()
    if x_grad:
        per_row = gs <= 0
        want = G.quant_matmul_t(w.expand_as(y).contiguous(), m.qweight, m.scales.detach().reshape(-1) if per_row else m.scales.detach(),
                                m.zeros.detach().reshape(-1) if per_row else m.zeros.detach(), 4, gs, perm=perm)
        assert xin.grad is not None and xin.grad.dtype == x.dtype and torch.equal(xin.grad, want.reshape(x.shape))


@pytest.mark.parametrize("x_grad", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_grid_grads_through_a_packed_linear(G, device, kind, x_grad):
    m, gs, perm, c = _module(G, device, kind)
    assert not list(m.parameters())
    params = G.trainable_grids(m)
    assert len(params) == 3 and len(list(m.parameters())) == 3
    x = _tokens((5, 64), 9, device)
    w = torch.from_numpy(np.random.default_rng(11).integers(-4, 5, (5, 40)).astype(np.float32)).to(device).half()
    _check_module_grads(G, m, x, w, gs, perm, c, x_grad)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(64,), (1, 64), (1, 1, 64)])
def test_single_token_inputs_get_grid_grads(G, device, kind, shape):
    m, gs, perm, c = _module(G, device, kind)
    G.trainable_grids(m)
    x = _tokens(shape, 10, device)
    w = torch.from_numpy(np.random.default_rng(11).integers(-4, 5, 40).astype(np.float32)).to(device).half()
    _check_module_grads(G, m, x, w, gs, perm, c, x_grad=False)
    for p in m.parameters():
        p.grad = None
    _check_module_grads(G, m, x, w, gs, perm, c, x_grad=True)


@pytest.mark.parametrize("kind", KINDS)
def test_quant_matmul_routes_grid_grads_too(G, device, kind):
    m, gs, perm, c = _module(G, device, kind)
    x = _tokens((5, 64), 9, device)
    s = m.scales.reshape(-1).clone().requires_grad_() if gs <= 0 else m.scales.clone().requires_grad_()
    z = m.zeros.reshape(-1).clone() if gs <= 0 else m.zeros.clone()
    b = m.bias.clone().requires_grad_()
    with torch.no_grad():
        y0 = G.quant_matmul(x, m.qweight, s, z, 4, gs, bias=b, out_dtype=torch.float32, perm=perm)
    y = G.quant_matmul(x, m.qweight, s, z, 4, gs, bias=b, out_dtype=torch.float32, perm=perm)
    assert torch.equal(y, y0) and y.dtype == torch.float32
    (2 * y).sum().backward()                                 # an fp32 grad: cast to x's type
    ds, dz, db = G.quant_grid_grad(x, torch.full((5, 40), 2.0, dtype=x.dtype, device=device), m.qweight, 4, gs, perm=perm)
    assert torch.equal(s.grad, ds) and torch.equal(b.grad, db) and z.grad is None


def test_fp32_activations_with_trainable_grids_raise(G, device):
    m = _module(G, device, "group")[0]
    G.trainable_grids(m)
    with pytest.raises(ValueError, match="backward through packed Linears needs fp16/bf16 activations"):
        m(torch.zeros(64, device=device))
    with torch.no_grad():
        y = m(torch.zeros(64, device=device))                # without autograd fp32 single tokens work as before
    assert y.dtype == torch.float32 and y.grad_fn is None


@pytest.mark.parametrize("kind", KINDS)
def test_parameters_state_and_one_sgd_step(G, device, kind):
    m, gs, perm, c = _module(G, device, kind)
    assert not list(m.parameters())                          # opt-in: nothing trains without the call
    keys = sorted(m.state_dict())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    params = G.trainable_grids(m)
    assert sorted(m.state_dict()) == keys and torch.equal(m.qweight, before["qweight"])
    assert sorted(n for n, _ in m.named_parameters()) == ["bias", "scales", "zeros"]
    x = _tokens((6, 64), 12, device)
    with torch.no_grad():
        y0 = m(x)
    opt = torch.optim.SGD(params, lr=1e-4)
    m(x).float().pow(2).sum().backward()
    opt.step()
    assert not torch.equal(m.scales.detach(), before["scales"]) and torch.equal(m.qweight, before["qweight"])
    with torch.no_grad():
        y1 = m(x)
    assert not torch.equal(y1, y0)
    trained = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert G.frozen_grids(m) == 3 and not list(m.parameters())
    assert sorted(m.state_dict()) == keys
    for k, v in m.state_dict().items():
        assert torch.equal(v, trained[k]), k
    assert m(x).grad_fn is None and torch.equal(m(x), y1)


def test_a_small_fit_recovers_perturbed_scales(G, device):
    """Scales of a grouped 4-bit module off by 10 %: 20 Adam steps on `scales` alone, against the outputs of the
    unperturbed module, bring the loss below a tenth of where it started."""
    m, gs, perm, c = _module(G, device, "group")
    x = _tokens((64, 64), 13, device)
    with torch.no_grad():
        target = m(x).float()
    m.scales = m.scales * 1.1
    params = G.trainable_grids(m, zeros=False, bias=False)
    assert len(params) == 1 and params[0] is m.scales
    opt = torch.optim.Adam(params, lr=float(m.scales.detach().mean()) * 0.005)   # 20 steps span the 10 %
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = (m(x).float() - target).pow(2).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float((m(x).float() - target).pow(2).sum()))
    print("fit: loss", " ".join(f"{v:.4g}" for v in losses))
    assert losses[-1] < 0.1 * losses[0], losses
