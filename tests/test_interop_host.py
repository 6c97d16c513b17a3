"""The host side of the GPTQ-checkpoint interop (gptq_amd/interop.py) and its numpy reference (tests/interop_ref.py):
everything here runs without a GPU.  The reference is checked against itself and against tests/packed_ref.py; the argument
validation of `from_gptq_tensors` must raise on CPU tensors before anything touches a device."""
import numpy as np
import pytest
import torch

import interop_ref as IR
import packed_ref as R


# ================================================================================================ the reference itself
@pytest.mark.parametrize("bits", IR.BITS)
def test_reference_pack_roundtrip_along_k_and_n(bits):
    rng = np.random.default_rng(bits)
    for K, N in ((32, 1), (96, 5), (256, 33)):
        codes = rng.integers(0, 2 ** bits, (K, N), dtype=np.uint8)
        codes[:, 0] = 2 ** bits - 1                                                 # every field full: no spill
        q = IR.pack_rows(codes, bits)
        assert q.shape == (K // 32 * bits, N) and q.dtype == np.int32
        assert np.array_equal(IR.unpack_rows(q, bits), codes)
    for G, N in ((1, 32), (3, 96), (8, 160)):
        v = rng.integers(0, 2 ** bits, (G, N))
        v[0] = 2 ** bits - 1
        qz = IR.pack_qzeros(v, bits)
        assert qz.shape == (G, N // 32 * bits) and qz.dtype == np.int32
        assert np.array_equal(IR.unpack_qzeros(qz, bits), v)
        # the definition, element by element: value of column n at bit bits*(n%32) of the stream starting at word (n/32)*bits
        words = qz.view(np.uint32).astype(object)
        for n in (0, 9, 10, 11, 21, 31, N - 1):
            bit = bits * (n % 32)
            stream = sum(int(words[G - 1, (n // 32) * bits + k]) << (32 * k) for k in range(bits))
            assert (stream >> bit) & (2 ** bits - 1) == v[G - 1, n]


def test_reference_qweight_equals_packed_ref():
    rng = np.random.default_rng(0)
    for bits, pack in ((3, R.pack3), (4, R.pack4)):
        codes = rng.integers(0, 2 ** bits, (160, 37), dtype=np.uint8)
        assert np.array_equal(IR.pack_rows(codes, bits), pack(codes))
        assert np.array_equal(IR.unpack_rows(pack(codes), bits), codes)


def test_reference_g_idx_and_perm_rules():
    rng = np.random.default_rng(1)
    K, gs = 96, 32
    g_idx = rng.permutation(np.repeat(np.arange(K // gs), gs)).astype(np.int32)
    perm = IR.perm_of(g_idx)
    assert sorted(perm.tolist()) == list(range(K))
    assert np.array_equal(g_idx[perm], np.arange(K) // gs)                          # storage row j is on the grid of j // gs
    assert all(perm[j] < perm[j + 1] for j in range(K - 1) if (j + 1) % gs)         # stable: ascending inside a group
    assert np.array_equal(IR.g_idx_of(K, gs, perm), g_idx)
    assert np.array_equal(IR.g_idx_of(K, gs), np.arange(K) // gs)
    assert not IR.g_idx_of(K, -1).any()


def test_reference_dense_weight_formula():
    rng = np.random.default_rng(2)
    bits, K, N, gs = 3, 64, 32, 32
    codes = rng.integers(0, 8, (K, N), dtype=np.uint8)
    s = rng.integers(1, 100, (2, N)).astype(np.float16) / np.float16(64)
    z = rng.integers(1, 8, (2, N))
    g_idx = rng.permutation(np.repeat(np.arange(2), gs))
    for fmt in ("gptq", "gptq_v2"):
        t = IR.foreign_tensors(codes, s, z, g_idx, bits, fmt)
        W = IR.dense_weight(t, bits, fmt)
        k, n = 17, 5
        assert W[n, k] == np.float32(s[g_idx[k], n]) * np.float32(int(codes[k, n]) - int(z[g_idx[k], n]))
    full = IR.foreign_tensors(codes, s, np.full((2, N), 8), g_idx, bits, "gptq")    # stored 7 under 'gptq': z = 8, unmasked
    assert (IR.zero_points(full["qzeros"], bits, "gptq") == 8).all()


# ================================================================================================ validation, no device
def _valid(bits=4, K=64, N=32, gs=32, seed=0):
    rng = np.random.default_rng(seed)
    G = K // gs if gs > 0 else 1
    g_idx = IR.g_idx_of(K, gs)
    t = IR.foreign_tensors(rng.integers(0, 2 ** bits, (K, N), dtype=np.uint8), np.ones((G, N), dtype=np.float16),
                           rng.integers(1, 2 ** bits, (G, N)), g_idx, bits, "gptq", bias=np.ones(N))
    return {k: torch.from_numpy(v) for k, v in t.items()}


BAD_INPUTS = {
    "qweight-int64": (lambda t: t.update(qweight=t["qweight"].long()), 32, "qweight must be torch.int32"),
    "scales-fp32": (lambda t: t.update(scales=t["scales"].float()), 32, "scales must be torch.float16"),
    "g_idx-float": (lambda t: t.update(g_idx=t["g_idx"].float()), 32, "g_idx must be int32 or int64"),
    "qzeros-width": (lambda t: t.update(qzeros=t["qzeros"][:, :-1].contiguous()), 32, "qzeros must be"),
    "group_size-48": (lambda t: None, 48, "group_size must be -1 or a positive multiple of 32"),
    "group-over-full": (lambda t: t["g_idx"].__setitem__(0, 1), 32, "every group must hold exactly 32 columns"),
    "g_idx-out-of-range": (lambda t: t["g_idx"].__setitem__(0, 2), 32, "g_idx values must lie in"),
    "g_idx-negative": (lambda t: t["g_idx"].__setitem__(0, -1), 32, "g_idx values must lie in"),
    "scales-shape": (lambda t: t.update(scales=t["scales"][:1].contiguous()), 32, "scales must be"),
    "bias-shape": (lambda t: t.update(bias=t["bias"][:-1].contiguous()), 32, "bias must be"),
    "unknown-key": (lambda t: t.update(zeros=t["scales"]), 32, "unknown entries"),
    "missing-qzeros": (lambda t: t.pop("qzeros"), 32, "lacks 'qzeros'"),
}


@pytest.mark.parametrize("case", list(BAD_INPUTS))
def test_from_gptq_tensors_validates_before_any_device(case, monkeypatch):
    import gptq_amd
    from gptq_amd import _lib, interop
    def no_device(*a, **k):
        raise AssertionError("validation must come before any library call")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(interop, "_stage", no_device)
    edit, gs, msg = BAD_INPUTS[case]
    t = _valid()
    edit(t)
    with pytest.raises(ValueError, match=msg):
        gptq_amd.from_gptq_tensors(t, 4, gs)


def test_from_gptq_tensors_per_row_needs_zero_g_idx(monkeypatch):
    import gptq_amd
    from gptq_amd import interop
    monkeypatch.setattr(interop, "_stage", lambda home: (_ for _ in ()).throw(AssertionError("touched a device")))
    t = _valid(gs=-1)
    t["g_idx"][3] = 1
    with pytest.raises(ValueError, match="g_idx must be absent or all zero"):
        gptq_amd.from_gptq_tensors(t, 4, -1)
    with pytest.raises(ValueError, match="bits must be 2, 3, 4 or 8"):
        gptq_amd.from_gptq_tensors(_valid(), 5, 32)
    with pytest.raises(ValueError, match="checkpoint_format must be"):
        gptq_amd.from_gptq_tensors(_valid(), 4, 32, checkpoint_format="marlin")


def test_valid_tensors_pass_validation_and_then_need_a_gpu():
    """The same tensors unedited get through every check; without a GPU the conversion then fails loudly."""
    import gptq_amd
    from gptq_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.GptqHipError):
        gptq_amd.from_gptq_tensors(_valid(), 4, 32)
    with pytest.raises(_lib.GptqHipError):
        gptq_amd.to_gptq_tensors(gptq_amd.Quant4Linear(32, 32))


# ================================================================================================ model level, no device
def _toy():
    import gptq_amd
    return torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.ReLU(), gptq_amd.QuantGroupLinear(4, 32, 32, 64, act_order=True),
                               torch.nn.LayerNorm(64), gptq_amd.QuantGroupLinear(4, 32, 64, 32))


def test_export_refuses_mixed_widths_and_group_sizes():
    import gptq_amd
    mixed = torch.nn.Sequential(gptq_amd.Quant3Linear(32, 32), gptq_amd.Quant4Linear(32, 32))
    with pytest.raises(ValueError, match=r"'0' has bits=3, group_size=-1 and '1' has bits=4, group_size=-1"):
        gptq_amd.export_gptq_state_dict(mixed)
    groups = torch.nn.Sequential(gptq_amd.QuantGroupLinear(4, 32, 64, 32), gptq_amd.QuantGroupLinear(4, 64, 64, 32))
    with pytest.raises(ValueError, match=r"'0' has bits=4, group_size=32 and '1' has bits=4, group_size=64"):
        gptq_amd.export_gptq_state_dict(groups)
    with pytest.raises(ValueError, match="no packed Linear"):
        gptq_amd.export_gptq_state_dict(torch.nn.Linear(4, 4))
    with pytest.raises(ValueError, match="checkpoint_format must be"):
        gptq_amd.export_gptq_state_dict(mixed, checkpoint_format="awq")


def test_key_mapping_of_a_small_sequential():
    import gptq_amd
    model = _toy()
    assert sorted(model.state_dict()) == sorted(
        ["0.weight", "0.bias", "3.weight", "3.bias"] + [f"2.{k}" for k in ("qweight", "scales", "zeros", "bias", "perm")]
        + [f"4.{k}" for k in ("qweight", "scales", "zeros", "bias")])
    foreign = ["qweight", "qzeros", "scales", "g_idx"]
    assert sorted(gptq_amd.gptq_checkpoint_keys(model)) == sorted(
        ["0.weight", "0.bias", "3.weight", "3.bias"] + [f"2.{k}" for k in foreign] + [f"4.{k}" for k in foreign])
    model[4].bias[3] = 0.5                                                          # a bias with an entry: exported
    assert sorted(gptq_amd.gptq_checkpoint_keys(model)) == sorted(
        ["0.weight", "0.bias", "3.weight", "3.bias"] + [f"2.{k}" for k in foreign] + [f"4.{k}" for k in foreign + ["bias"]])


def test_load_refuses_a_foreign_config_and_a_shape_mismatch(monkeypatch):
    import gptq_amd
    from gptq_amd import interop
    monkeypatch.setattr(interop, "_stage", lambda home: (_ for _ in ()).throw(AssertionError("touched a device")))
    model = torch.nn.Sequential(torch.nn.Linear(64, 32))
    sd = {f"0.{k}": v for k, v in _valid().items()}
    with pytest.raises(ValueError, match="quant_method must be 'gptq'"):
        gptq_amd.load_gptq_state_dict(model, sd, {"bits": 4, "group_size": 32, "quant_method": "awq"})
    with pytest.raises(ValueError, match="lacks 'group_size'"):
        gptq_amd.load_gptq_state_dict(model, sd, {"bits": 4})
    wrong = torch.nn.Sequential(torch.nn.Linear(128, 32))
    with pytest.raises(ValueError, match="is a 128 -> 32 Linear"):
        gptq_amd.load_gptq_state_dict(wrong, sd, {"bits": 4, "group_size": 32})
