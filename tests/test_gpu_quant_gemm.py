"""The packed dequant GEMM (csrc/qgemm.hip, gptq_amd.quant_matmul) and the multi-token forward of the packed Linears:
kernel against an fp64 formula, determinism and edges, the modules against dense fake-quantized Linears, and packed
models scored by eval_ppl."""
import pytest
import torch

pytestmark = pytest.mark.gpu

U = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


@pytest.fixture(scope="module")
def G():
    import gptq_amd
    from gptq_amd import _lib
    _lib.load()
    return gptq_amd


def make_case(dev, bits, K, N, groupsize, seed):
    """Random codes packed by pack_codes, random grids (zeros = zero*scale), bias; the dense fp64 weights [K, N]."""
    from gptq_amd.quant import pack_codes
    gen = torch.Generator(device=dev).manual_seed(seed)
    codes = torch.randint(0, 2 ** bits, (N, K), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
    ng = K // groupsize if groupsize > 0 else 1
    scales = torch.rand(ng, N, device=dev, generator=gen) * 0.02 + 0.001
    zeros = torch.randint(0, 2 ** bits, (ng, N), device=dev, generator=gen).float() * scales
    bias = torch.randn(N, device=dev, generator=gen)
    grp = (torch.arange(K, device=dev) // groupsize) if groupsize > 0 else torch.zeros(K, dtype=torch.long, device=dev)
    wdeq = codes.t().double() * scales[grp].double() - zeros[grp].double()          # [K, N]
    if groupsize <= 0:
        scales, zeros = scales[0], zeros[0]
    return pack_codes(codes, bits), scales, zeros, bias, wdeq


def check_bar(y, x, wdeq, bias, out_dtype):
    """|y - ref| <= 5e-5 (|x| @ |Wdeq| + |bias|) + u |ref| per element."""
    xd = x.reshape(-1, x.shape[-1]).double()
    ref = xd @ wdeq + (bias.double() if bias is not None else 0.0)
    mag = xd.abs() @ wdeq.abs() + (bias.double().abs() if bias is not None else 0.0)
    err = (y.reshape(ref.shape).double() - ref).abs()
    bar = 5e-5 * mag + U[out_dtype] * ref.abs()
    worst = float((err / bar).max())
    assert worst <= 1.0, f"error {worst:.3g} x the bar"
    return worst


GRIDS = {"row": -1, "g32": 32, "g128": 128}
SHAPES = [(32, 16), (256, 80), (1024, 1000), (2048, 4096)]


CASES = [(K, N, grid) for K, N in SHAPES for grid in GRIDS if GRIDS[grid] <= K]     # groupsize <= K


@pytest.mark.parametrize("xdtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("K,N,grid", CASES, ids=[f"{k}x{n}-{g}" for k, n, g in CASES])
def test_gemm_vs_fp64_formula(G, hip_device, bits, grid, xdtype, K, N):
    gs = GRIDS[grid]
    qw, s, z, b, wdeq = make_case(hip_device, bits, K, N, gs, seed=K + N + bits + max(gs, 0))
    gen = torch.Generator(device=hip_device).manual_seed(7)
    for M in (1, 2, 7, 16, 33, 100, 257):
        x = torch.randn(M, K, device=hip_device, generator=gen).to(xdtype)
        y = G.quant_matmul(x, qw, s, z, bits, gs, bias=b, out_dtype=torch.float32)
        assert y.shape == (M, N) and y.dtype == torch.float32
        check_bar(y, x, wdeq, b, torch.float32)
        # rounded outputs: one rounding of the same fp32 value
        yo = G.quant_matmul(x, qw, s, z, bits, gs, bias=b)
        assert yo.dtype == xdtype
        check_bar(yo, x, wdeq, b, xdtype)


def test_gemm_llama_shape_m2048(G, hip_device):
    K, N, gs = 4096, 11008, 128
    qw, s, z, b, wdeq = make_case(hip_device, 4, K, N, gs, seed=11)
    x = torch.randn(2048, K, device=hip_device).half()
    y = G.quant_matmul(x, qw, s, z, 4, gs, bias=b, out_dtype=torch.float32)
    check_bar(y, x, wdeq, b, torch.float32)


@pytest.mark.parametrize("M,K,N,bits,gs", [(2, 2048, 4096, 4, 128), (16, 4096, 1000, 3, -1), (300, 1024, 4096, 4, -1)])
def test_gemm_is_deterministic(G, hip_device, M, K, N, bits, gs):
    from gptq_amd import _lib
    assert M > 200 or _lib.load().gptq_quant_gemm_workspace_bytes(M, K, N, bits, gs) > 0   # the split-K path runs
    qw, s, z, b, _ = make_case(hip_device, bits, K, N, gs, seed=3)
    x = torch.randn(M, K, device=hip_device).bfloat16()
    y1 = G.quant_matmul(x, qw, s, z, bits, gs, bias=b, out_dtype=torch.float32)
    y2 = G.quant_matmul(x, qw, s, z, bits, gs, bias=b, out_dtype=torch.float32)
    assert torch.equal(y1, y2)


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("gs", [-1, 128])
def test_gemm_m1_agrees_with_matvec(G, hip_device, bits, gs):
    from gptq_amd import quant_cuda
    K, N = 1024, 1000
    qw, s, z, b, wdeq = make_case(hip_device, bits, K, N, gs, seed=21)
    x = torch.randn(1, K, device=hip_device).half()
    y = G.quant_matmul(x, qw, s, z, bits, gs, bias=b, out_dtype=torch.float32)
    mv = b.clone()
    if gs > 0:
        quant_cuda.vecquant_matmul_grouped(x.reshape(-1), qw, mv, s, z, bits, gs)
    elif bits == 3:
        quant_cuda.vecquant3matmul_faster(x.reshape(-1), qw, mv, s.reshape(-1, 1), z.reshape(-1, 1))
    else:
        quant_cuda.vecquant4matmul(x.reshape(-1), qw, mv, s.reshape(-1, 1), z.reshape(-1, 1))
    mag = x.double().abs() @ wdeq.abs() + b.double().abs()
    assert float(((y.double() - mv.double()).abs() / (5e-5 * mag)).max()) <= 1.0


@pytest.mark.parametrize("pad", [64, 24])      # 64: 16-byte rows; 24: rows that are not (element loads)
def test_gemm_strided_x(G, hip_device, pad):
    K, N = 1024, 1000
    qw, s, z, b, wdeq = make_case(hip_device, 4, K, N, 128, seed=5)
    big = torch.randn(37, K + pad, device=hip_device).half()
    x = big[:, :K]
    assert x.stride(0) == K + pad
    y = G.quant_matmul(x, qw, s, z, 4, 128, bias=b, out_dtype=torch.float32)
    yc = G.quant_matmul(x.contiguous(), qw, s, z, 4, 128, bias=b, out_dtype=torch.float32)
    assert torch.equal(y, yc)
    check_bar(y, x, wdeq, b, torch.float32)


def test_gemm_rejects_bad_arguments(G, hip_device):
    qw, s, z, b, _ = make_case(hip_device, 4, 256, 80, 128, seed=1)
    x = torch.randn(3, 256, device=hip_device)
    with pytest.raises(ValueError):
        G.quant_matmul(x, qw, s, z, 4, 128)                      # fp32 x
    with pytest.raises(ValueError):
        G.quant_matmul(x.half(), qw, s, z, 8, 128)               # bits
    with pytest.raises(ValueError):
        G.quant_matmul(x.half(), qw, s, z, 4, 64)                # table of another groupsize
    with pytest.raises(ValueError):
        G.quant_matmul(x.half()[:, :224], qw, s, z, 4, 128)      # K mismatch


# ------------------------------------------------------------------------------------------ the packed modules
def _per_row_module(G, dev, cls_name, faster, K=512, N=384, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    bits = 3 if cls_name == "Quant3Linear" else 4
    W = torch.randn(N, K, device=dev, generator=gen) * 0.02
    q = G.Quantizer()
    q.configure(bits, perchannel=True, sym=False, mse=False)
    q.find_params(W, weight=True)
    Wq = G.quantize(W, q.scale, q.zero, q.maxq)
    lin = torch.nn.Linear(K, N, device=dev)
    lin.weight.data = Wq.clone()
    lin.bias.data = torch.randn(N, device=dev, generator=gen) * 0.1
    m = getattr(G, cls_name)(K, N, faster=faster, multi_token=True)
    m.pack(lin, q.scale, q.zero)
    dense = torch.nn.Linear(K, N, device=dev, dtype=torch.float16)
    dense.weight.data = Wq.half()
    dense.bias.data = lin.bias.data.half()
    wdeq = Wq.t().double()
    return m, dense, wdeq, lin.bias.data.float(), K


def _grouped_module(G, dev):
    gen = torch.Generator(device=dev).manual_seed(5)
    R, C = 384, 512
    lin = torch.nn.Linear(C, R, bias=True, device=dev, dtype=torch.float16)
    lin.weight.data = (torch.randn(R, C, device=dev, generator=gen) * 0.02).half()
    gp = G.GPTQ(lin)
    gp.quantizer = G.Quantizer()
    gp.quantizer.configure(4, perchannel=True, sym=False, mse=False)
    chan = (1 + torch.arange(C, device=dev) % 7).half()
    for _ in range(2):
        gp.add_batch(torch.randn(1, 1024, C, device=dev, generator=gen).half() * chan, None)
    gp.fasterquant(groupsize=128, actorder=True, static_groups=True)
    m = G.QuantGroupLinear.from_gptq(gp, 4, multi_token=True).to(dev)
    grp = torch.arange(C, device=dev) // 128
    Wq = gp.group_scale[:, grp] * (gp.codes.float() - gp.group_zero[:, grp])     # exact grid values [R, C]
    dense = torch.nn.Linear(C, R, device=dev, dtype=torch.float16)
    dense.weight.data = lin.weight.data.clone()
    dense.bias.data = lin.bias.data.clone()
    return m, dense, Wq.t().double(), lin.bias.data.float(), C


MODULES = ["Quant3Linear", "Quant3Linear-faster", "Quant4Linear", "QuantGroupLinear"]


@pytest.mark.parametrize("kind", MODULES)
def test_module_multi_token_forward(G, hip_device, kind):
    if kind == "QuantGroupLinear":
        m, dense, wdeq, bias, K = _grouped_module(G, hip_device)
        default = G.QuantGroupLinear(m.bits, m.groupsize, K, m.qweight.shape[1]).to(hip_device)
    else:
        cls = kind.split("-")[0]
        m, dense, wdeq, bias, K = _per_row_module(G, hip_device, cls, kind.endswith("faster"))
        default = getattr(G, cls)(K, m.qweight.shape[1])
    keys = sorted(m.state_dict())
    default.load_state_dict(m.state_dict())
    assert sorted(default.state_dict()) == keys           # the flag is no state: same keys with and without it
    default = default.to(hip_device)

    x = torch.randn(2, 37, K, device=hip_device).half()
    y = m(x)
    assert y.shape == (2, 37, dense.out_features) and y.dtype == torch.float16
    ref = dense(x)
    rel = float((y.double() - ref.double()).norm() / ref.double().norm())
    assert rel <= 2e-3, rel
    # every token agrees with its single-token (mat-vec) call within the kernel bar (+ fp16 output rounding)
    singles = torch.stack([m(x[i, j].reshape(1, 1, K)).reshape(-1) for i in range(2) for j in range(37)])
    mag = x.reshape(-1, K).double().abs() @ wdeq.abs() + bias.double().abs()
    exact = x.reshape(-1, K).double() @ wdeq + bias.double()
    diff = (y.reshape(-1, y.shape[-1]).double() - singles.double()).abs()
    assert bool((diff <= 5e-5 * mag + 2 * 2.0 ** -11 * exact.abs() + 1e-7).all()), float(diff.max())
    # bf16 in -> bf16 out
    yb = m(x.bfloat16())
    assert yb.dtype == torch.bfloat16
    relb = float((yb.double() - ref.double()).norm() / ref.double().norm())
    assert relb <= 2e-2, relb
    # the default keeps the reference's guard
    with pytest.raises(ValueError):
        default(x)
    G.set_multi_token(default)
    assert torch.equal(default(x), y)


# ------------------------------------------------------------------------------------------ end to end
def _tiny_opt(seed=0):
    from transformers import OPTConfig, OPTForCausalLM
    cfg = OPTConfig(vocab_size=256, hidden_size=128, ffn_dim=512, num_hidden_layers=2, num_attention_heads=4,
                    max_position_embeddings=128, word_embed_proj_dim=128, do_layer_norm_before=True,
                    dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, layerdrop=0.0)
    torch.manual_seed(seed)
    m = OPTForCausalLM(cfg).half().eval()
    m.seqlen = 128
    return m


def _tiny_llama(seed=0):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=256, hidden_size=128, intermediate_size=352, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=4, max_position_embeddings=256)
    torch.manual_seed(seed)
    m = LlamaForCausalLM(cfg).half().eval()
    m.seqlen = 256
    return m


@pytest.mark.parametrize("family,bits", [("opt", 3), ("opt", 4), ("llama", 4)])
def test_packed_model_eval_ppl(G, hip_device, tmp_path, family, bits):
    import gptq_amd.gptq as gmod
    from gptq_amd.sequential import QuantArgs, eval_ppl, llama_sequential, make_packed_skeleton, opt_sequential, pack_model
    gmod.VERBOSE = False
    build = _tiny_opt if family == "opt" else _tiny_llama
    model = build()
    S = model.seqlen
    gen = torch.Generator().manual_seed(2)
    calib = [(torch.randint(0, 256, (1, S), generator=gen), None) for _ in range(4)]
    test = torch.randint(0, 256, (1, 4 * S), generator=gen)
    if family == "opt":
        quantizers = opt_sequential(model, calib, hip_device, QuantArgs(wbits=bits, nsamples=4, static_groups=True))
    else:
        quantizers = llama_sequential(model, calib, hip_device,
                                      QuantArgs(wbits=bits, nsamples=4, act_order=True, true_sequential=True))
    ppl_dense = eval_ppl(model, test, hip_device)

    pack_model(model, quantizers, bits=bits, multi_token=True)
    ppl_packed = eval_ppl(model, test, hip_device)
    print(f"{family} {bits}-bit: PPL dense {ppl_dense:.5f} packed {ppl_packed:.5f} |dPPL| {abs(ppl_packed - ppl_dense):.2e} "
          f"({abs(ppl_packed - ppl_dense) / ppl_dense:.2e} relative)")
    assert abs(ppl_packed - ppl_dense) <= 5e-3 * ppl_dense

    path = tmp_path / "packed.pt"
    torch.save(model.state_dict(), path)
    fresh = build(seed=1)
    make_packed_skeleton(fresh, list(quantizers), bits=bits, multi_token=True)
    fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)
    assert eval_ppl(fresh, test, hip_device) == ppl_packed
