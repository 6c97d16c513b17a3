"""Grouped and act-order packed Linears end to end: the grouped pack (gptq_pack_grouped), the mat-vec and the dequant
GEMM on the act-order format (storage row j = input column perm[j]), QuantGroupLinear.from_gptq for act-order with
dynamic groups, and grouped models through pack_model / save / make_packed_skeleton / load / eval_ppl."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gptq_amd
    from gptq_amd import _lib
    _lib.load()
    return gptq_amd


def random_perm(K, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return torch.randperm(K, device=dev, generator=gen).to(torch.int32)


def grouped_case(dev, bits, K, N, gs, perm, seed):
    """Random codes [N, K] (original column order), grids [G, N] of the STORAGE groups (zeros = zero*scale) and the fp32
    weights on those grids: column perm[j] lies on the grid of group j // gs."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    codes = torch.randint(0, 2 ** bits, (N, K), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
    ng = K // gs
    scales = torch.rand(ng, N, device=dev, generator=gen) * 0.02 + 0.001
    zero = torch.randint(0, 2 ** bits, (ng, N), device=dev, generator=gen).float()
    gcol = torch.arange(K, device=dev) // gs                                 # group of storage row j
    if perm is not None:
        g = torch.empty_like(gcol)
        g[perm.long()] = gcol                                                  # group of input column i
        gcol = g
    W = scales.t()[:, gcol] * (codes.float() - zero.t()[:, gcol])             # [N, K]
    return codes, scales, zero, W


def storage_wdeq(codes, scales, zeros, gs, perm):
    """fp64 dense weights in STORAGE order [K, N]: row j = scale[j/gs] * q[perm[j]] - zeros[j/gs]."""
    K = codes.shape[1]
    c = codes if perm is None else codes[:, perm.long()]
    grp = torch.arange(K, device=codes.device) // gs
    return c.t().double() * scales[grp].double() - zeros[grp].double()


# ------------------------------------------------------------------------------------------ 1. grouped pack
@pytest.mark.parametrize("wdtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("with_perm", [False, True], ids=["noperm", "perm"])
@pytest.mark.parametrize("K", [1024, 1408])
@pytest.mark.parametrize("gs", [32, 128])
@pytest.mark.parametrize("bits", [3, 4])
def test_grouped_pack_is_bit_identical_to_pack_codes(G, hip_device, bits, gs, K, with_perm, wdtype):
    N = 200
    perm = random_perm(K, hip_device, K + gs) if with_perm else None
    codes, scales, zero, W = grouped_case(hip_device, bits, K, N, gs, perm, seed=bits * K + gs)
    qw = G.pack_grouped(W.to(wdtype), scales, zero * scales, gs, bits, perm)
    want = G.pack_codes(codes if perm is None else codes[:, perm.long()].contiguous(), bits)
    assert qw.shape == (K // 32 * bits, N)
    assert torch.equal(qw, want)


# ------------------------------------------------------------------------------------------ 2. mat-vec with perm
@pytest.mark.parametrize("K,N,gs", [(1024, 520, 32), (4096, 1024, 128), (1408, 130, 128)])
@pytest.mark.parametrize("bits", [3, 4])
def test_matvec_perm_vs_fp64_formula(G, hip_device, bits, K, N, gs):
    from gptq_amd import quant_cuda
    perm = random_perm(K, hip_device, K + N)
    codes, scales, zero, _ = grouped_case(hip_device, bits, K, N, gs, perm, seed=K * bits + N)
    zeros = zero * scales
    qw = G.pack_codes(codes[:, perm.long()].contiguous(), bits)
    wdeq = storage_wdeq(codes, scales, zeros, gs, perm)                      # [K, N]
    gen = torch.Generator(device=hip_device).manual_seed(3)
    bias = torch.randn(N, device=hip_device, generator=gen)
    x = torch.randn(K, device=hip_device, generator=gen)
    ref = bias.double() + x.double()[perm.long()] @ wdeq
    for xt, tol in ((x, 1e-5), (x.half(), 1e-2)):
        y = bias.clone()
        quant_cuda.vecquant_matmul_grouped(xt, qw, y, scales, zeros, bits, gs, perm=perm)
        r = bias.double() + xt.double()[perm.long()] @ wdeq
        assert float((y.double() - r).abs().max()) <= tol * float(ref.abs().max())


# ------------------------------------------------------------------------------------------ 3. GEMM with perm
def check_bar(y, xg, wdeq, bias):
    """|y - ref| <= 5e-5 (|x| @ |Wdeq| + |bias|) per element (fp32 output), ref over the GATHERED x."""
    xd = xg.reshape(-1, xg.shape[-1]).double()
    ref = xd @ wdeq + bias.double()
    mag = xd.abs() @ wdeq.abs() + bias.double().abs()
    worst = float(((y.reshape(ref.shape).double() - ref).abs() / (5e-5 * mag)).max())
    assert worst <= 1.0, f"error {worst:.3g} x the bar"


@pytest.mark.parametrize("xdtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("bits,K,N,gs", [(4, 1024, 1000, 128), (3, 2048, 512, 32), (4, 4096, 4096, 128)])
def test_gemm_perm_bit_identical_to_gathered_x(G, hip_device, bits, K, N, gs, xdtype):
    perm = random_perm(K, hip_device, K + bits)
    codes, scales, zero, _ = grouped_case(hip_device, bits, K, N, gs, perm, seed=K + N + bits)
    zeros = zero * scales
    qw = G.pack_codes(codes[:, perm.long()].contiguous(), bits)
    wdeq = storage_wdeq(codes, scales, zeros, gs, perm)
    gen = torch.Generator(device=hip_device).manual_seed(9)
    bias = torch.randn(N, device=hip_device, generator=gen)
    for M in (1, 2, 5, 16, 17, 64, 333, 2048):
        x = torch.randn(M, K, device=hip_device, generator=gen).to(xdtype)
        xg = x[:, perm.long()].contiguous()
        y = G.quant_matmul(x, qw, scales, zeros, bits, gs, bias=bias, out_dtype=torch.float32, perm=perm)
        y0 = G.quant_matmul(xg, qw, scales, zeros, bits, gs, bias=bias, out_dtype=torch.float32)
        assert torch.equal(y, y0), M
        check_bar(y, xg, wdeq, bias)
        # the same call twice: bit-identical
        assert torch.equal(G.quant_matmul(x, qw, scales, zeros, bits, gs, bias=bias, out_dtype=torch.float32,
                                          perm=perm), y), M
        # rounded output: the same single rounding
        yo = G.quant_matmul(x, qw, scales, zeros, bits, gs, bias=bias, perm=perm)
        assert yo.dtype == xdtype and torch.equal(yo, G.quant_matmul(xg, qw, scales, zeros, bits, gs, bias=bias))


@pytest.mark.parametrize("pad", [64, 24])      # 64: 16-byte rows; 24: rows that are not
def test_gemm_perm_strided_x(G, hip_device, pad):
    K, N, gs = 1024, 1000, 128
    perm = random_perm(K, hip_device, 17)
    codes, scales, zero, _ = grouped_case(hip_device, 4, K, N, gs, perm, seed=5)
    qw = G.pack_codes(codes[:, perm.long()].contiguous(), 4)
    zeros = zero * scales
    for M in (3, 5, 300):                  # fused gather (M <= 4) and pre-pass
        big = torch.randn(M, K + pad, device=hip_device).half()
        x = big[:, :K]
        assert x.stride(0) == K + pad
        y = G.quant_matmul(x, qw, scales, zeros, 4, gs, out_dtype=torch.float32, perm=perm)
        y0 = G.quant_matmul(x[:, perm.long()].contiguous(), qw, scales, zeros, 4, gs, out_dtype=torch.float32)
        assert torch.equal(y, y0)


def test_perm_arguments_are_checked(G, hip_device):
    from gptq_amd import quant_cuda
    K, N = 256, 80
    perm = random_perm(K, hip_device, 1)
    codes, scales, zero, _ = grouped_case(hip_device, 4, K, N, 128, perm, seed=1)
    qw = G.pack_codes(codes, 4)
    x = torch.randn(3, K, device=hip_device).half()
    for bad in (perm.long(), perm[:-32], perm.cpu()):
        with pytest.raises(ValueError):
            G.quant_matmul(x, qw, scales, zero * scales, 4, 128, perm=bad)
        with pytest.raises(ValueError):
            quant_cuda.vecquant_matmul_grouped(x[0], qw, torch.zeros(N, device=hip_device), scales, zero * scales, 4, 128,
                                               perm=bad)
    with pytest.raises(ValueError):                       # the act-order format has grouped grids
        G.quant_matmul(x, qw, scales[0], (zero * scales)[0], 4, -1, perm=perm)


# ------------------------------------------------------------------------------------------ 4. from_gptq
def _act_order_solver(G, dev, R=512, C=1024, gs=128):
    gen = torch.Generator(device=dev).manual_seed(5)
    lin = torch.nn.Linear(C, R, bias=True, device=dev, dtype=torch.float16)
    lin.weight.data = (torch.randn(R, C, device=dev, generator=gen) * 0.02).half()
    gp = G.GPTQ(lin)
    gp.quantizer = G.Quantizer()
    gp.quantizer.configure(4, perchannel=True, sym=False, mse=False)
    # uneven channel scales, in no particular column order: the act-order permutation is far from the identity
    chan = (1 + torch.randperm(C, device=dev, generator=gen) % 13).half()
    for _ in range(3):
        gp.add_batch(torch.randn(1, 2048, C, device=dev, generator=gen).half() * chan, None)
    gp.fasterquant(groupsize=gs, actorder=True, static_groups=False)
    return gp, lin


def test_from_gptq_act_order_dynamic_groups(G, hip_device):
    from gptq_amd.quant import dequant_packed
    R, C, gs = 512, 1024, 128
    gp, lin = _act_order_solver(G, hip_device, R, C, gs)
    perm = gp.perm
    assert perm is not None and not gp.static_groups
    assert int((perm.long() != torch.arange(C, device=hip_device)).sum()) > C // 2
    m = G.QuantGroupLinear.from_gptq(gp, 4, multi_token=True).to(hip_device)
    assert m.act_order and "perm" in m.state_dict() and m.perm.dtype == torch.int32
    assert m.qweight.shape == (C // 8, R) and m.scales.shape == (C // gs, R)
    # the packed layer dequantizes to the fake-quantized weight, bit for bit
    W = dequant_packed(m.qweight, gp.group_scale.t().contiguous(), gp.group_zero.t().contiguous(), 4, gs,
                       dtype=lin.weight.dtype, perm=m.perm)
    assert torch.equal(W, lin.weight.data)
    # g_idx: input column perm[j] is in group j // gs
    g_idx = m.g_idx
    assert g_idx.dtype == torch.int32 and g_idx.shape == (C,)
    assert torch.equal(g_idx[perm.long()], (torch.arange(C, device=hip_device) // gs).int())
    # forward, one token and several, against fp64 on the fake-quantized weight
    wq = lin.weight.data.double()
    bias = lin.bias.data.double()
    gen = torch.Generator(device=hip_device).manual_seed(8)
    for M in (1, 7):
        x = torch.randn(M, C, device=hip_device, generator=gen).half()
        y = m(x.reshape(1, M, C))
        assert y.shape == (1, M, R) and y.dtype == torch.float16
        ref = x.double() @ wq.t() + bias
        mag = x.double().abs() @ wq.abs().t() + bias.abs()
        err = (y.reshape(M, R).double() - ref).abs()
        assert bool((err <= 5e-5 * mag + 2 * 2.0 ** -11 * ref.abs() + 1e-6).all()), float(err.max())
    # plain grouped modules keep k // gs
    plain = G.QuantGroupLinear(4, gs, C, R)
    assert torch.equal(plain.g_idx, (torch.arange(C) // gs).int())


# ------------------------------------------------------------------------------------------ 5. driver end to end
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


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_grouped_model_pack_save_load(G, hip_device, tmp_path, family):
    import gptq_amd.gptq as gmod
    from gptq_amd.modelutils import find_layers
    from gptq_amd.quant import dequant_packed
    from gptq_amd.sequential import (QuantArgs, benchmark, eval_ppl, llama_sequential, make_packed_skeleton,
                                     opt_sequential, pack_model)
    gmod.VERBOSE = False
    bits, gs = 4, 32
    build = _tiny_opt if family == "opt" else _tiny_llama
    model = build()
    S = model.seqlen
    gen = torch.Generator().manual_seed(2)
    calib = [(torch.randint(0, 256, (1, S), generator=gen), None) for _ in range(4)]
    test = torch.randint(0, 256, (1, 4 * S), generator=gen)
    prompt = torch.randint(0, 256, (1, 32), generator=gen)
    if family == "opt":       # act-order with static groups: the plain grouped format
        quantizers = opt_sequential(model, calib, hip_device, QuantArgs(wbits=bits, nsamples=4, groupsize=gs,
                                                                         act_order=True, static_groups=True))
        act = False
    else:                     # act-order with dynamic groups (the LLaMA driver's default): the perm format
        quantizers = llama_sequential(model, calib, hip_device, QuantArgs(wbits=bits, nsamples=4, groupsize=gs,
                                                                           act_order=True, true_sequential=True))
        act = True
    for q in quantizers.values():
        assert q.groupsize == gs and q.static_groups == (family == "opt")
        assert q.group_scale is not None and q.group_zero is not None and q.perm is not None
        assert q.group_scale.shape[1] == q.group_zero.shape[1]
    layers = find_layers(model)
    fake = {n: layers[n].weight.data.clone() for n in quantizers}
    ppl_dense = eval_ppl(model, test, hip_device)
    _, ppl_gen_dense = benchmark(model.to(hip_device), prompt, hip_device, check=True, warmup=1)
    model.cpu()

    pack_model(model, quantizers, bits=bits, multi_token=True)
    packed_layers = {n: m for n, m in model.named_modules() if n in quantizers}
    for n, q in quantizers.items():
        m = packed_layers[n]
        assert isinstance(m, G.QuantGroupLinear) and m.act_order == act and ("perm" in m.state_dict()) == act
        W = dequant_packed(m.qweight.to(hip_device), q.group_scale.t().contiguous(), q.group_zero.t().contiguous(), bits,
                           gs, dtype=fake[n].dtype, perm=m.perm.to(hip_device) if act else None)
        assert torch.equal(W.cpu(), fake[n].cpu()), n
    ppl_packed = eval_ppl(model, test, hip_device)
    print(f"{family} g{gs}: PPL dense {ppl_dense:.5f} packed {ppl_packed:.5f} "
          f"({abs(ppl_packed - ppl_dense) / ppl_dense:.2e} relative)")
    assert abs(ppl_packed - ppl_dense) <= 5e-3 * ppl_dense

    path = tmp_path / "packed.pt"
    torch.save(model.state_dict(), path)
    fresh = build(seed=1)
    make_packed_skeleton(fresh, list(quantizers), bits=bits, multi_token=True, groupsize=gs, act_order=act)
    fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)
    assert eval_ppl(fresh, test, hip_device) == ppl_packed

    # token-by-token generation: every Linear call is the single-token mat-vec
    _, ppl_gen = benchmark(fresh.to(hip_device), prompt, hip_device, check=True, warmup=1)
    print(f"{family} g{gs} generation: PPL dense {ppl_gen_dense:.4f} packed {ppl_gen:.4f}")
    assert abs(ppl_gen - ppl_gen_dense) <= 2e-2 * ppl_gen_dense
