"""Non-plain activations and gradients through the packed matmul wrappers: a row-padded, a transposed and an expanded
(stride 0) input give the bits of the same call on a contiguous copy, for `quant_matmul`, `quant_matmul_a8`,
`quant_matmul_t`, `quant_grid_grad` and `quantize_activations`.

Both sides of those comparisons run the wrappers, so the contiguous `quant_matmul` / `quant_matmul_t` results are also
held against `dequant_packed` in fp64 with the bar of test_gpu_quant_gemm.check_bar.  The grids are dyadic (scales a
power of two, integer zero points): scale * (code - zero), as `dequant_packed` forms a weight, and scale * code - zeros,
as the GEMMs do, are then the same exact fp32 value, which fp16 holds too, so the dense weights are exactly the ones
both kernels multiply by.  M = 3, K = 64, N = 40: N is no multiple of 64, the column masks are live."""
import pytest
import torch

from test_gpu_quant_gemm import check_bar

pytestmark = pytest.mark.gpu

M, K, N, PAD = 3, 64, 40, 8
GRIDS = {"row": -1, "g32-perm": 32}


@pytest.fixture(scope="module")
def G():
    import gptq_amd
    from gptq_amd import _lib
    _lib.load()
    return gptq_amd


def make_case(dev, bits, groupsize, seed):
    from gptq_amd.quant import dequant_packed, pack_codes
    gen = torch.Generator(device=dev).manual_seed(seed)
    codes = torch.randint(0, 2 ** bits, (N, K), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
    ng = K // groupsize if groupsize > 0 else 1
    scales = torch.exp2(-torch.randint(4, 8, (ng, N), device=dev, generator=gen).float())
    zint = torch.randint(0, 2 ** bits, (ng, N), device=dev, generator=gen).float()
    perm = torch.randperm(K, device=dev, generator=gen).to(torch.int32) if groupsize > 0 else None
    qw = pack_codes(codes, bits)
    wdeq = dequant_packed(qw, scales, zint, bits, groupsize, torch.float32, perm=perm).double().t()     # [K, N]
    s, z = (scales, zint * scales) if groupsize > 0 else (scales[0], (zint * scales)[0])
    bias = torch.randn(N, device=dev, generator=gen)
    x = torch.randn(M, K, device=dev, generator=gen).half()
    grad = torch.randn(M, N, device=dev, generator=gen).half()
    return qw, s, z, bias, perm, wdeq, x, grad


def padded(t):
    buf = torch.full((t.shape[0], t.shape[1] + PAD), 1000.0, dtype=torch.float32, device=t.device).to(t.dtype)
    buf[:, :t.shape[1]] = t
    v = buf[:, :t.shape[1]]
    assert v.stride(0) == t.shape[1] + PAD and torch.equal(v, t)
    return v


def transposed(t):
    v = t.t().contiguous().t()
    assert v.stride(-1) != 1 and torch.equal(v, t)
    return v


def expanded(t):
    v = t[:1].expand(t.shape[0], -1)
    assert v.stride(0) == 0
    return v


def same(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return len(a) == len(b) and all(same(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("bits", [3, 4])
def test_views_give_the_bits_of_contiguous_copies(G, hip_device, bits, grid):
    gs = GRIDS[grid]
    qw, s, z, bias, perm, wdeq, x, grad = make_case(hip_device, bits, gs, seed=10 * bits + max(gs, 0))

    def fwd(v):
        return G.quant_matmul(v, qw, s, z, bits, gs, bias=bias, perm=perm)

    def a8(v):
        return G.quant_matmul_a8(v, qw, s, z, bits, gs, bias=bias, perm=perm)

    def bwd(v):
        return G.quant_matmul_t(v, qw, s, z, bits, gs, perm=perm)

    def grids(vx, vg):
        return G.quant_grid_grad(vx, vg, qw, bits, gs, perm)

    def act(v):
        return G.quantize_activations(v, perm)

    # the anchors: the contiguous results against the dense fp64 weights
    y, dx = fwd(x), bwd(grad)
    assert y.shape == (M, N) and dx.shape == (M, K) and y.dtype == dx.dtype == torch.float16
    print(f"{bits}-bit {grid}: forward {check_bar(y, x, wdeq, bias, torch.float16):.3g} x the bar, "
          f"backward {check_bar(dx, grad, wdeq.t(), None, torch.float16):.3g} x the bar")

    for view in (padded, transposed, expanded):
        vx, vg = view(x), view(grad)
        cx, cg = vx.contiguous(), vg.contiguous()
        assert same(fwd(vx), fwd(cx)), f"quant_matmul, {view.__name__} x"
        assert same(bwd(vg), bwd(cg)), f"quant_matmul_t, {view.__name__} grad"
        assert same(grids(vx, vg), grids(cx, cg)), f"quant_grid_grad, {view.__name__} x and grad"
        assert same(grids(x, vg), grids(x, cg)), f"quant_grid_grad, {view.__name__} grad"
        assert same(act(vx), act(cx)), f"quantize_activations, {view.__name__} x"
        assert same(a8(vx), a8(cx)), f"quant_matmul_a8, {view.__name__} x"
    # the pair form takes row-padded codes as they are (`perm` went into the quantization)
    xq, sx = act(x)
    vq = torch.zeros(M, K + PAD, dtype=torch.int8, device=hip_device)
    vq[:, :K] = xq
    pair = G.quant_matmul_a8((vq[:, :K], sx), qw, s, z, bits, gs, bias=bias)
    assert same(pair, G.quant_matmul_a8((xq, sx), qw, s, z, bits, gs, bias=bias)) and same(pair, a8(x))
