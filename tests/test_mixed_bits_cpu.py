"""Mixed-width options of the driver without a device: `wbits_for`, the validation that precedes all GPU work, the
per-width skeletons and the new C entry in the binding table."""
import pytest
import torch

from gptq_amd.sequential import (QuantArgs, check_wbits, make_packed_skeleton, pack_model, packed_wbits,
                                 quantize_sequential, wbits_for)

TABLE = {"k_proj": 4, "q_proj": 4, "v_proj": 3, "out_proj": 3, "fc1": 4, "fc2": 3}
OPT_LINEARS = ["self_attn.k_proj", "self_attn.v_proj", "self_attn.q_proj", "self_attn.out_proj", "fc1", "fc2"]


def test_wbits_for_all_three_modes():
    assert wbits_for(QuantArgs(wbits=3), 1, "self_attn.q_proj") == 3
    a = QuantArgs(wbits=2, layer_wbits=[4, 3])
    assert [wbits_for(a, i, n) for i in (0, 1) for n in ("fc1", "self_attn.v_proj")] == [4, 4, 3, 3]
    a = QuantArgs(wbits=2, linear_wbits=dict(TABLE))
    assert [wbits_for(a, 5, n) for n in OPT_LINEARS] == [4, 3, 4, 3, 4, 3]
    assert wbits_for(a, 0, "model.decoder.layers.0.self_attn.v_proj") == 3      # the last component names the Linear
    got = check_wbits(a, [OPT_LINEARS, OPT_LINEARS])
    assert got[(1, "fc2")] == 3 and len(got) == 12


@pytest.mark.parametrize("kw", [
    dict(layer_wbits=[4, 3], linear_wbits=dict(TABLE)),                           # both options
    dict(layer_wbits=[4, 3, 4]),                                                  # wrong length
    dict(layer_wbits=[4]),
    dict(linear_wbits={k: v for k, v in TABLE.items() if k != "fc2"}),           # a Linear with no entry
    dict(layer_wbits=[4, 9]),                                                     # a width outside 1..8
    dict(layer_wbits=[0, 4]),
    dict(linear_wbits=dict(TABLE, fc1=16)),
    dict(linear_wbits=dict(TABLE, fc1=3.5)),
    dict(sweep_wbits=(3, 12)),
], ids=["both", "too_long", "too_short", "no_entry", "width_9", "width_0", "width_16", "width_float", "sweep_12"])
def test_bad_width_options_raise_before_any_gpu_work(kw):
    args = QuantArgs(nsamples=2, **kw)
    with pytest.raises(ValueError):
        check_wbits(args, [OPT_LINEARS, OPT_LINEARS])
    # the driver itself, on a model that never leaves the host: the error comes before the first device call
    from transformers import OPTConfig, OPTForCausalLM
    cfg = OPTConfig(vocab_size=64, hidden_size=32, ffn_dim=64, num_hidden_layers=2, num_attention_heads=2,
                    max_position_embeddings=32, word_embed_proj_dim=32)
    model = OPTForCausalLM(cfg).eval()
    model.seqlen = 16
    calib = [(torch.zeros((1, 16), dtype=torch.long), None)] * 2
    with pytest.raises(ValueError):
        quantize_sequential(model, calib, torch.device("cuda:0"), args)


def test_wbits_for_raises_on_its_own():
    with pytest.raises(ValueError):
        wbits_for(QuantArgs(layer_wbits=[4], linear_wbits={"fc1": 4}), 0, "fc1")
    with pytest.raises(ValueError):
        wbits_for(QuantArgs(layer_wbits=[4, 3]), 2, "fc1")
    with pytest.raises(ValueError):
        wbits_for(QuantArgs(linear_wbits={"fc1": 4}), 0, "fc2")
    with pytest.raises(ValueError):
        wbits_for(QuantArgs(linear_wbits={"fc1": 12}), 0, "fc1")


def test_skeleton_takes_a_width_per_name_and_reads_back():
    import gptq_amd
    net = torch.nn.Sequential()
    net.add_module("a", torch.nn.Linear(64, 32))
    net.add_module("b", torch.nn.Linear(64, 32))
    net.add_module("c", torch.nn.Linear(64, 32))
    make_packed_skeleton(net, ["a", "b"], {"a": 4, "b": 3}, multi_token=True)
    assert type(net.a) is gptq_amd.Quant4Linear and type(net.b) is gptq_amd.Quant3Linear
    assert isinstance(net.c, torch.nn.Linear)
    assert packed_wbits(net) == {"a": 4, "b": 3}
    grouped = torch.nn.Sequential()
    grouped.add_module("a", torch.nn.Linear(64, 32))
    grouped.add_module("b", torch.nn.Linear(64, 32))
    make_packed_skeleton(grouped, ["a", "b"], {"a": 8, "b": 2}, groupsize=32)
    assert packed_wbits(grouped) == {"a": 8, "b": 2}
    assert type(grouped.a) is gptq_amd.QuantGroupLinear and grouped.b.qweight.shape == (64 // 32 * 2, 32)
    with pytest.raises(ValueError):
        make_packed_skeleton(torch.nn.Sequential(torch.nn.Linear(64, 32)), ["0"], {})            # no width for "0"
    with pytest.raises(ValueError):
        make_packed_skeleton(torch.nn.Sequential(torch.nn.Linear(64, 32)), ["0"], {"0": 5})


def test_pack_model_rejects_unpackable_own_widths_before_packing():
    import gptq_amd
    net = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.Linear(64, 32))
    qs = {}
    for name, bits in (("0", 4), ("1", 5)):
        qs[name] = gptq_amd.Quantizer()
        qs[name].configure(bits, perchannel=True, sym=False)
    with pytest.raises(ValueError):
        pack_model(net, qs)                                  # bits=None: every Linear at its own quantizer.wbits
    assert isinstance(net[0], torch.nn.Linear)               # nothing was replaced


def test_new_entry_is_bound():
    from gptq_amd import _lib
    assert "gptq_fasterquant_rows_mixed" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "gptq_fasterquant_rows_mixed")
    res, argtypes = _lib._SIGNATURES["gptq_fasterquant_rows_mixed"]
    assert len(argtypes) == len(_lib._SIGNATURES["gptq_fasterquant_rows"][1]) + 1
    assert lib.gptq_hip_abi_version() == 2
