"""The grouped / act-order packed format without a GPU: module buffers and state_dict keys, the load-side skeleton,
argument checks that run before any launch, the new C entry points declared and bound, and no CPU fallback."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gptq_pack_grouped", "gptq_dequant_packed_perm", "gptq_vecquant_matmul_grouped_perm",
               "gptq_quant_gemm_perm", "gptq_quant_gemm_perm_workspace_bytes"]


def test_perm_buffer_only_with_act_order():
    import gptq_amd
    plain = gptq_amd.QuantGroupLinear(4, 128, 512, 96)
    assert sorted(plain.state_dict()) == ["bias", "qweight", "scales", "zeros"]
    assert not plain.act_order
    act = gptq_amd.QuantGroupLinear(3, 32, 512, 96, act_order=True)
    assert sorted(act.state_dict()) == ["bias", "perm", "qweight", "scales", "zeros"]
    assert act.perm.dtype == torch.int32 and act.perm.shape == (512,)
    assert act.qweight.shape == (512 // 32 * 3, 96) and act.scales.shape == (16, 96) and act.zeros.shape == (16, 96)
    assert gptq_amd.set_multi_token(torch.nn.Sequential(plain, act)) == 2 and act.multi_token


def test_g_idx_property():
    import gptq_amd
    plain = gptq_amd.QuantGroupLinear(4, 32, 128, 8)
    assert torch.equal(plain.g_idx, (torch.arange(128) // 32).int())
    act = gptq_amd.QuantGroupLinear(4, 32, 128, 8, act_order=True)
    perm = torch.randperm(128, generator=torch.Generator().manual_seed(0)).int()
    act.perm.copy_(perm)
    g = act.g_idx
    assert g.dtype == torch.int32
    assert torch.equal(g[perm.long()], (torch.arange(128) // 32).int())
    assert "g_idx" not in act.state_dict()


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=64, hidden_size=64, intermediate_size=352, num_hidden_layers=1,
                      num_attention_heads=2, num_key_value_heads=2, max_position_embeddings=64)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).eval()


@pytest.mark.parametrize("act_order", [False, True])
def test_skeleton_builds_grouped_modules(act_order):
    import gptq_amd
    from gptq_amd.modelutils import find_layers
    from gptq_amd.sequential import make_packed_skeleton
    model = _tiny_llama()
    names = [n for n in find_layers(model) if n.startswith("model.layers.")]
    shapes = {n: (m.in_features, m.out_features) for n, m in find_layers(model).items() if n in names}
    make_packed_skeleton(model, names, bits=4, multi_token=True, groupsize=32, act_order=act_order)
    mods = dict(model.named_modules())
    for n in names:
        m = mods[n]
        K, N = shapes[n]
        assert isinstance(m, gptq_amd.QuantGroupLinear) and m.multi_token and m.act_order == act_order
        sd = m.state_dict()
        assert sd["qweight"].shape == (K // 8, N) and sd["scales"].shape == (K // 32, N)
        assert ("perm" in sd) == act_order
        if act_order:
            assert sd["perm"].shape == (K,) and sd["perm"].dtype == torch.int32
    # a skeleton's state_dict loads into another skeleton of the same kind, strictly
    other = _tiny_llama()
    make_packed_skeleton(other, names, bits=4, groupsize=32, act_order=act_order)
    other.load_state_dict(model.state_dict(), strict=True)


def test_skeleton_without_groupsize_is_unchanged():
    import gptq_amd
    from gptq_amd.sequential import make_packed_skeleton
    model = _tiny_llama()
    make_packed_skeleton(model, ["model.layers.0.mlp.down_proj"], bits=3)
    assert isinstance(model.model.layers[0].mlp.down_proj, gptq_amd.Quant3Linear)


def test_bad_perm_raises_value_error_before_launch():
    import gptq_amd
    from gptq_amd import quant_cuda
    from gptq_amd.quant import dequant_packed, pack_grouped
    K, N = 256, 16
    x = torch.zeros(3, K, dtype=torch.float16)
    qw = torch.zeros(K // 32 * 4, N, dtype=torch.int32)
    s, z = torch.ones(K // 128, N), torch.zeros(K // 128, N)
    good = torch.arange(K, dtype=torch.int32)
    for bad in (good.long(), good.float(), good[:-1], torch.arange(K + 32, dtype=torch.int32), good.reshape(2, -1)):
        with pytest.raises(ValueError):
            gptq_amd.quant_matmul(x, qw, s, z, 4, 128, perm=bad)
        with pytest.raises(ValueError):
            quant_cuda.vecquant_matmul_grouped(x[0], qw, torch.zeros(N), s, z, 4, 128, perm=bad)
        with pytest.raises(ValueError):
            pack_grouped(torch.zeros(N, K), s, z, 128, 4, perm=bad)
        with pytest.raises(ValueError):
            dequant_packed(qw, s, z, 4, 128, perm=bad)
    with pytest.raises(ValueError):                           # per-row grids have no act-order format
        gptq_amd.quant_matmul(x, qw, s[0], z[0], 4, -1, perm=good)


def test_new_entry_points_fail_loudly_without_gpu():
    import gptq_amd
    from gptq_amd import _lib, quant_cuda
    from gptq_amd.quant import dequant_packed, pack_grouped
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    K, N = 256, 16
    perm = torch.arange(K, dtype=torch.int32)
    qw = torch.zeros(K // 32 * 4, N, dtype=torch.int32)
    s, z = torch.ones(K // 128, N), torch.zeros(K // 128, N)
    with pytest.raises(_lib.GptqHipError):
        gptq_amd.quant_matmul(torch.zeros(3, K, dtype=torch.float16), qw, s, z, 4, 128, perm=perm)
    with pytest.raises(_lib.GptqHipError):
        quant_cuda.vecquant_matmul_grouped(torch.zeros(K), qw, torch.zeros(N), s, z, 4, 128, perm=perm)
    with pytest.raises(_lib.GptqHipError):
        pack_grouped(torch.zeros(N, K), s, z, 128, 4, perm=perm)
    with pytest.raises(_lib.GptqHipError):
        dequant_packed(qw, s, z, 4, 128, perm=perm)
    m = gptq_amd.QuantGroupLinear(4, 128, K, N, act_order=True)
    with pytest.raises(_lib.GptqHipError):
        m(torch.zeros(1, 1, K))


def test_new_symbols_declared_bound_and_exported():
    from gptq_amd import _lib
    from gptq_amd.build import build_library
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gptq_hip.h")).read(), flags=re.S)
    build_library(verbose=False)
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert re.search(rf"\b{n}\s*\(", text), n
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    # the act-order GEMM's workspace query is a pure function of the shape, at least the plain GEMM's
    for M in (1, 16, 17, 2048):
        a = lib.gptq_quant_gemm_workspace_bytes(M, 4096, 11008, 4, 128)
        b = lib.gptq_quant_gemm_perm_workspace_bytes(M, 4096, 11008, 4, 128)
        assert b >= a
    assert lib.gptq_quant_gemm_perm_workspace_bytes(2, 4096, 4096, 5, 128) == 0
