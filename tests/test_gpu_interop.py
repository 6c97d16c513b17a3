"""Import and export of the other GPTQ tools' checkpoint layout (gptq_amd/interop.py, csrc/interop.hip) against its
definition as tests/interop_ref.py writes it in numpy.  Every comparison is on integers or on single-operation fp32 /
fp16 results: exact equality, no tolerance (the fp64 dense-product test uses the contract bar of tests/packed_ref.py).

Shapes: K in {32, 96, 256}, N in {32, 96, 160} (one qzeros stream; N no multiple of a 64- or 256-wide workgroup),
group_size in {-1, 32, K}, all four widths, crossed.  Interoperability is checked against the format's definition, not
against the other tools themselves."""
import itertools
import types

import numpy as np
import pytest
import torch

import interop_ref as IR
import packed_ref as R

pytestmark = pytest.mark.gpu

KS, NS = (32, 96, 256), (32, 96, 160)
FORMATS = ("gptq", "gptq_v2")
SENT32 = 0x7FC5A5A5


@pytest.fixture(scope="module")
def G():
    import gptq_amd
    from gptq_amd import _lib
    _lib.load()
    return gptq_amd


def shapes():
    for K, N in itertools.product(KS, NS):
        for gs in sorted({-1, 32, K}):
            yield K, N, gs


def assert_same_tensors(got, want, what):
    assert sorted(got) == sorted(want), f"{what}: keys {sorted(got)} != {sorted(want)}"
    for k in want:
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        w = want[k].cpu().numpy() if isinstance(want[k], torch.Tensor) else want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {k} is {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
        assert np.array_equal(g, w), f"{what}: {k} differs in {int((g != w).sum())} of {g.size} entries"


def make_case(bits, K, N, gs, perm_kind=None, seed=0, zero_min=1, dyadic=False, bias=True):
    """Random codes (storage order), fp16-exact positive scales, integer zero points in [zero_min, 2^bits - 1] with both
    ends present in every group row, an fp16-exact bias.  perm_kind: None, 'random', 'reverse' or 'stable' (a perm that
    is the stable argsort of its own g_idx)."""
    rng = np.random.default_rng([seed, bits, K, N, max(gs, 0), {None: 0, "random": 1, "reverse": 2, "stable": 3}[perm_kind]])
    maxq = 2 ** bits - 1
    Gn = K // gs if gs > 0 else 1
    c = types.SimpleNamespace(bits=bits, K=K, N=N, gs=gs)
    c.codes = rng.integers(0, maxq + 1, (K, N), dtype=np.uint8)
    if dyadic:
        c.scales = np.ldexp(1.0, -rng.integers(6, 9, (Gn, N))).astype(np.float32)
    else:
        c.scales = (rng.integers(1, 2048, (Gn, N)) / 4096.0).astype(np.float16).astype(np.float32)
    c.zint = rng.integers(zero_min, maxq + 1, (Gn, N))
    c.zint[:, 0::7] = zero_min
    c.zint[:, 3::7] = maxq
    c.zeros = c.zint.astype(np.float32) * c.scales                                   # exact: < 9 bits times 11 bits
    c.bias = (rng.integers(-512, 513, N) / 256.0).astype(np.float32) if bias else np.zeros(N, dtype=np.float32)
    if perm_kind is None:
        c.perm = None
    elif perm_kind == "random":
        c.perm = rng.permutation(K).astype(np.int32)
    elif perm_kind == "reverse":
        c.perm = np.arange(K - 1, -1, -1, dtype=np.int32)
    else:
        c.perm = IR.perm_of(rng.permutation(np.repeat(np.arange(Gn), gs)))
    return c


def build_module(G, dev, c, multi_token=True):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if c.gs > 0:
        m = G.QuantGroupLinear(c.bits, c.gs, c.K, c.N, multi_token=multi_token, act_order=c.perm is not None)
        m.scales, m.zeros = t(c.scales), t(c.zeros)
        if c.perm is not None:
            m.perm = t(c.perm)
    else:
        from gptq_amd.quant import PACKED_LINEAR
        m = PACKED_LINEAR[c.bits](c.K, c.N, multi_token=multi_token)
        m.scales, m.zeros = t(c.scales.reshape(c.N, 1)), t(c.zeros.reshape(c.N, 1))
    m.qweight = G.pack_codes(t(c.codes.T), c.bits)
    m.bias = t(c.bias)
    return m.to(dev)


def buffers(m):
    return {k: v.detach() for k, v in m.state_dict().items()}


def perm_kinds(gs):
    return (None, "random", "reverse", "stable") if gs > 0 else (None,)


# ================================================================================================ 1. export
@pytest.mark.parametrize("bits", IR.BITS)
def test_export_equals_the_definition(G, hip_device, bits):
    n = 0
    for K, N, gs in shapes():
        for kind in perm_kinds(gs):
            c = make_case(bits, K, N, gs, kind, seed=1, bias=(K + N) % 64 != 0)
            m = build_module(G, hip_device, c)
            assert np.array_equal(m.qweight.cpu().numpy(), IR.pack_rows(c.codes, bits))      # the input is what we think
            before = {k: v.clone() for k, v in buffers(m).items()}
            for fmt in FORMATS:
                got = G.to_gptq_tensors(m, fmt)
                want = IR.own_to_foreign(c.codes, c.scales, c.zint, gs, bits, fmt, c.perm, c.bias)
                assert_same_tensors(got, want, f"{bits}-bit {K}x{N} g{gs} {kind} {fmt}")
                assert all(v.device == m.qweight.device for v in got.values())
                n += 1
            if gs > 0:
                assert np.array_equal(got["g_idx"].cpu().numpy(), m.g_idx.cpu().numpy())
            assert_same_tensors(buffers(m), before, "the module after exporting")
    assert n == 2 * 3 * (5 + 9 + 9)                                  # K = 32 has two group sizes, 96 and 256 three


def test_export_of_a_host_module_stages_on_the_gpu(G, hip_device):
    c = make_case(3, 96, 96, 32, "random", seed=2)
    m = build_module(G, hip_device, c).cpu()
    got = G.to_gptq_tensors(m, "gptq_v2", strict=True)
    assert all(v.device.type == "cpu" for v in got.values())
    assert_same_tensors(got, IR.own_to_foreign(c.codes, c.scales, c.zint, 32, 3, "gptq_v2", c.perm, c.bias), "host module")


# ================================================================================================ 2. import
def make_foreign(bits, K, N, gs, fmt, seed=0, g_idx_kind="random", bias=True):
    """numpy-made foreign tensors with a random valid g_idx, and what they mean."""
    rng = np.random.default_rng([seed, bits, K, N, max(gs, 0), FORMATS.index(fmt)])
    maxq = 2 ** bits - 1
    Gn = K // gs if gs > 0 else 1
    off = IR.ZERO_OFFSET[fmt]
    f = types.SimpleNamespace(bits=bits, K=K, N=N, gs=gs, fmt=fmt)
    f.codes = rng.integers(0, maxq + 1, (K, N), dtype=np.uint8)                       # original column order
    f.scales16 = (rng.integers(1, 2048, (Gn, N)) / 4096.0).astype(np.float16)
    f.zint = rng.integers(off, maxq + off + 1, (Gn, N))                             # every storable value ...
    f.zint[:, 1::5] = maxq + off                                                    # ... 2^bits under 'gptq' among them
    f.zint[:, 2::5] = off
    if gs <= 0:
        f.g_idx = np.zeros(K, dtype=np.int32)
    elif g_idx_kind == "random":
        f.g_idx = rng.permutation(np.repeat(np.arange(Gn), gs)).astype(np.int32)
    else:
        f.g_idx = (np.arange(K) // gs).astype(np.int32)
    f.bias = (rng.integers(-512, 513, N) / 256.0).astype(np.float16) if bias else None
    f.t = IR.foreign_tensors(f.codes, f.scales16, f.zint, f.g_idx, bits, fmt, f.bias)
    f.perm = IR.perm_of(f.g_idx)
    return f


def torch_tensors(t, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in t.items()}


@pytest.mark.parametrize("bits", IR.BITS)
def test_import_equals_the_definition(G, hip_device, bits):
    from gptq_amd.quant import PACKED_LINEAR, dequant_packed
    dev = hip_device
    for (K, N, gs), fmt in itertools.product(shapes(), FORMATS):
        f = make_foreign(bits, K, N, gs, fmt, seed=3)
        if fmt == "gptq":
            assert (f.zint == 2 ** bits).any() and (IR.unpack_qzeros(f.t["qzeros"], bits) == 2 ** bits - 1).any()
        tt = torch_tensors(f.t, dev)
        if (K + N) % 64 == 0:
            tt["g_idx"] = tt["g_idx"].long()                                        # int64 g_idx is accepted too
        m = G.from_gptq_tensors(tt, bits, gs, fmt, multi_token=True)
        what = f"{bits}-bit {K}x{N} g{gs} {fmt}"
        s32 = f.scales16.astype(np.float32)
        z32 = f.zint.astype(np.float32) * s32                                       # one fp32 multiplication
        trivial = gs <= 0 or np.array_equal(f.g_idx, np.arange(K) // gs)
        want = {"qweight": IR.pack_rows(f.codes if trivial else f.codes[f.perm], bits), "bias": f.bias.astype(np.float32),
                "scales": s32.reshape(N, 1) if gs <= 0 else s32, "zeros": z32.reshape(N, 1) if gs <= 0 else z32}
        if gs <= 0:
            assert type(m) is PACKED_LINEAR[bits]
        else:
            assert type(m) is G.QuantGroupLinear and m.act_order == (not trivial) and m.groupsize == gs and m.bits == bits
            if not trivial:
                want["perm"] = f.perm
        assert m.multi_token and m.qweight.device == dev
        assert_same_tensors(buffers(m), want, what)
        W = dequant_packed(m.qweight, m.scales.reshape(-1, N), torch.from_numpy(f.zint.astype(np.float32)).to(dev), bits,
                           gs, dtype=torch.float32, perm=m.perm if gs > 0 and m.act_order else None)
        assert np.array_equal(W.cpu().numpy(), IR.dense_weight(f.t, bits, fmt)), what + ": dense weight"


def test_import_without_g_idx_or_bias_and_onto_the_host(G, hip_device):
    f = make_foreign(4, 96, 32, 32, "gptq", seed=4, g_idx_kind="trivial", bias=False)
    t = torch_tensors(f.t, hip_device)
    with_g = G.from_gptq_tensors(t, 4, 32)
    assert not with_g.act_order and not with_g.bias.any() and not with_g.multi_token
    del t["g_idx"]
    assert_same_tensors(buffers(G.from_gptq_tensors(t, 4, 32)), buffers(with_g), "g_idx absent")
    host = G.from_gptq_tensors({k: v.cpu() for k, v in t.items()}, 4, 32)          # host tensors: staged, module on the host
    assert all(v.device.type == "cpu" for v in buffers(host).values())
    assert_same_tensors(buffers(host), buffers(with_g), "host tensors")
    on_dev = G.from_gptq_tensors({k: v.cpu() for k, v in t.items()}, 4, 32, device=hip_device)
    assert on_dev.qweight.device == hip_device


# ================================================================================================ 3. round trips
@pytest.mark.parametrize("bits", IR.BITS)
def test_round_trips(G, hip_device, bits):
    dev = hip_device
    for K, N, gs in shapes():
        for kind in perm_kinds(gs):
            c = make_case(bits, K, N, gs, kind, seed=5, dyadic=True)
            m = build_module(G, dev, c)
            what = f"{bits}-bit {K}x{N} g{gs} {kind}"
            # exact arithmetic (dyadic scales, x a small integer / 4: tests/packed_ref.py), so the forward does not depend
            # on the order of the rows inside a group and an equivalent module must give the same bits
            x = torch.from_numpy(np.random.default_rng(K + N).integers(-2, 3, (5, K)) / 4.0).to(dev).half()
            y = m(x)
            for fmt in FORMATS:
                t = G.to_gptq_tensors(m, fmt)
                m2 = G.from_gptq_tensors(t, bits, gs, fmt, multi_token=True)
                if kind is None or (kind == "stable" and gs != K):              # perm is the stable argsort of g_idx
                    assert_same_tensors(buffers(m2), buffers(m), what + " module -> tensors -> module")
                else:
                    assert m2.act_order == (gs != K)                                # one group: g_idx is k // K again
                assert_same_tensors(G.to_gptq_tensors(m2, fmt), t, what + " re-export")
                assert torch.equal(m2(x), y), what + ": multi-token forward of the re-imported module"
                assert torch.equal(m2(x[:1]), m(x[:1])), what + ": single-token forward of the re-imported module"
    # tensors -> module -> tensors
    for (K, N, gs), fmt in itertools.product(shapes(), FORMATS):
        f = make_foreign(bits, K, N, gs, fmt, seed=6)
        if fmt == "gptq":
            f.zint = np.minimum(f.zint, 2 ** bits - 1)                                  # (2^bits cannot be written back)
            f.t = IR.foreign_tensors(f.codes, f.scales16, f.zint, f.g_idx, bits, fmt, f.bias)
        t = torch_tensors(f.t, dev)
        back = G.to_gptq_tensors(G.from_gptq_tensors(t, bits, gs, fmt), fmt, strict=True)
        assert_same_tensors(back, f.t, f"{bits}-bit {K}x{N} g{gs} {fmt} tensors -> module -> tensors")


def test_stored_full_field_under_gptq_is_two_to_the_bits(G, hip_device):
    """A stored 2^bits - 1 under 'gptq' imports as z = 2^bits (no masking), which the classic format cannot write back."""
    for bits in IR.BITS:
        f = make_foreign(bits, 32, 32, -1, "gptq", seed=7)
        f.zint[:] = 2 ** bits
        f.t = IR.foreign_tensors(f.codes, f.scales16, f.zint, f.g_idx, bits, "gptq", f.bias)
        assert (f.t["qzeros"] == -1).all()                                          # every field full
        m = G.from_gptq_tensors(torch_tensors(f.t, hip_device), bits, -1, "gptq")
        want = (np.float32(2 ** bits) * f.scales16.astype(np.float32)).reshape(32, 1)
        assert np.array_equal(m.zeros.cpu().numpy(), want)
        with pytest.raises(ValueError, match="zero point lies outside"):
            G.to_gptq_tensors(m, "gptq")


def test_model_round_trip_through_a_checkpoint_directory(G, hip_device, tmp_path):
    pytest.importorskip("safetensors")
    import json
    dev = hip_device
    ca = make_case(4, 64, 96, 32, "random", seed=8, dyadic=True)
    cb = make_case(4, 96, 32, 32, None, seed=9, dyadic=True, bias=False)
    model = torch.nn.Sequential(build_module(G, dev, ca), torch.nn.LayerNorm(96).to(dev).half(), build_module(G, dev, cb))
    sd, cfg = G.export_gptq_state_dict(model)
    assert sorted(sd) == sorted(G.gptq_checkpoint_keys(model))
    assert cfg == {"bits": 4, "group_size": 32, "desc_act": True, "static_groups": False, "sym": False,
                   "checkpoint_format": "gptq", "quant_method": "gptq", "damp_percent": 0.01, "true_sequential": True}
    assert_same_tensors({k[2:]: v for k, v in sd.items() if k.startswith("0.")},
                        IR.own_to_foreign(ca.codes, ca.scales, ca.zint, 32, 4, "gptq", ca.perm, ca.bias), "state_dict[0.*]")
    assert torch.equal(sd["1.weight"], model[1].weight) and "2.bias" not in sd
    config = G.save_gptq_checkpoint(model, str(tmp_path / "ckpt"), checkpoint_format="gptq_v2")
    assert json.load(open(tmp_path / "ckpt" / "quantize_config.json")) == config and config["checkpoint_format"] == "gptq_v2"
    skeleton = torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.LayerNorm(96), torch.nn.Linear(96, 32)).to(dev).half()
    res = G.load_gptq_checkpoint(skeleton, str(tmp_path / "ckpt"), multi_token=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert type(skeleton[0]) is G.QuantGroupLinear and skeleton[0].act_order and not skeleton[2].act_order
    x = torch.from_numpy(np.random.default_rng(0).integers(-2, 3, (3, 64)) / 4.0).to(dev).half()
    assert torch.equal(skeleton(x), model(x))
    sd2, cfg2 = G.export_gptq_state_dict(skeleton, "gptq_v2")
    assert cfg2 == config
    assert_same_tensors(sd2, G.export_gptq_state_dict(model, "gptq_v2")[0], "re-export of the loaded model")
    # a symmetric grid is reported as such
    sym = make_case(4, 32, 32, -1, seed=10)
    sym.zint[:] = 8
    sym.zeros = sym.zint.astype(np.float32) * sym.scales
    assert G.export_gptq_state_dict(torch.nn.Sequential(build_module(G, dev, sym)))[1]["sym"] is True


# ================================================================================================ 4. fp64 dense product
U_F16 = 2.0 ** -11
ETA_F16 = 2.0 ** -25


def _coef(n_chain):
    return min(1.1 * n_chain * 2.0 ** -24, 5e-5)                                    # tests/test_gpu_packed_exact.py


@pytest.mark.parametrize("bits,gs", [(4, 32), (3, -1)], ids=["4bit-act-order", "3bit-per-row"])
def test_imported_module_against_fp64_dense_product(G, hip_device, bits, gs):
    """|y - x W^T| <= c T + u_out |ref| + eta_out with the contract magnitude and the coefficients of
    tests/test_gpu_packed_exact.py (GEMM chain: group + groups + S + 2; mat-vec: K + groups + 8 against T_mv)."""
    from gptq_amd import _lib
    dev = hip_device
    K, N, M = 256, 160, 5
    f = make_foreign(bits, K, N, gs, "gptq", seed=11)
    m = G.from_gptq_tensors(torch_tensors(f.t, dev), bits, gs, "gptq", multi_token=True)
    assert gs < 0 or m.act_order
    rng = np.random.default_rng(12)
    x = torch.from_numpy(rng.standard_normal((M, K)) + 1.0).half()
    W = IR.dense_weight(f.t, bits, "gptq").astype(np.float64)                       # [N, K], original column order
    bias = f.bias.astype(np.float64)
    ref = x.double().numpy() @ W.T + bias
    storage = f.codes[f.perm] if gs > 0 else f.codes
    xg = x.double().numpy()[:, f.perm] if gs > 0 else x.double().numpy()
    s32 = f.scales16.astype(np.float32)
    z32 = f.zint.astype(np.float32) * s32
    tabs = (s32, z32) if gs > 0 else (s32[0], z32[0])
    ref2, T, Tmv = R.reference_and_magnitude(storage, tabs[0], tabs[1], gs, xg, bias)
    assert np.abs(ref2 - ref).max() <= 1e-9 * np.abs(T).max()                       # the two fp64 routes agree
    ngroups = K // gs if gs > 0 else 1
    nbytes = _lib.load().gptq_quant_gemm_workspace_bytes(M, K, N, bits, gs)
    S = nbytes // (4 * M * N) if nbytes else 1
    y = m(x.to(dev)).double().cpu().numpy()
    bar = _coef((gs if gs > 0 else K) + ngroups + S + 2) * T + U_F16 * np.abs(ref) + ETA_F16
    print(f"GEMM worst err / bar {float((np.abs(y - ref) / bar).max()):.3e}")
    assert (np.abs(y - ref) <= bar).all()
    y1 = m(x[:1].to(dev)).double().cpu().numpy()
    bar1 = _coef(K + ngroups + 8) * Tmv[:1] + U_F16 * np.abs(ref[:1]) + ETA_F16
    print(f"mat-vec worst err / bar {float((np.abs(y1 - ref[:1]) / bar1).max()):.3e}")
    assert (np.abs(y1 - ref[:1]) <= bar1).all()


# ================================================================================================ 5. refusals
def test_refusals(G, hip_device):
    dev = hip_device
    # a trained grid is no longer integer
    m = build_module(G, dev, make_case(4, 64, 32, 32, seed=13))
    G.trainable_grids(m)
    with torch.no_grad():
        m.zeros[1, 5] += 1e-3
    with pytest.raises(ValueError, match="off the integer lattice.*trainable_grids"):
        G.to_gptq_tensors(m)
    with torch.no_grad():
        m.zeros[1, 5] -= 1e-3
    # a zero point of 0: not under 'gptq', fine under 'gptq_v2'
    c = make_case(4, 64, 32, 32, "random", seed=14, zero_min=0)
    assert (c.zint == 0).any()
    m = build_module(G, dev, c)
    with pytest.raises(ValueError, match="zero point lies outside.*gptq_v2"):
        G.to_gptq_tensors(m, "gptq")
    assert_same_tensors(G.to_gptq_tensors(m, "gptq_v2"),
                        IR.own_to_foreign(c.codes, c.scales, c.zint, 32, 4, "gptq_v2", c.perm, c.bias), "zero point 0, v2")
    c.zint[0, 1] = 16                                                               # above the range in either format
    m.zeros = torch.from_numpy(c.zint.astype(np.float32) * c.scales).to(dev)
    with pytest.raises(ValueError, match=r"zero point lies outside \[0, 15\]$"):
        G.to_gptq_tensors(m, "gptq_v2")
    # out_features no multiple of 32
    with pytest.raises(ValueError, match="out_features = 40 is not a multiple of 32"):
        G.to_gptq_tensors(G.QuantGroupLinear(4, 32, 32, 40).to(dev))
    # scales that fp16 cannot hold, or only rounded
    for bad, msg in ((1e-9, "0, inf or nan in fp16"), (1e6, "0, inf or nan in fp16"), (0.0, "0, inf or nan in fp16")):
        c = make_case(4, 64, 32, 32, seed=15)
        c.scales[1, 7] = bad
        c.zeros = c.zint.astype(np.float32) * c.scales
        with pytest.raises(ValueError, match=msg):
            G.to_gptq_tensors(build_module(G, dev, c))
    c = make_case(4, 64, 32, 32, seed=16)
    c.scales[1, 7] = np.float32(0.1)
    c.zeros = c.zint.astype(np.float32) * c.scales
    m = build_module(G, dev, c)
    with pytest.raises(ValueError, match="strict=True.*not exactly representable in fp16"):
        G.to_gptq_tensors(m, strict=True)
    t = G.to_gptq_tensors(m)                                                        # without strict: rounded once
    assert_same_tensors(t, IR.own_to_foreign(c.codes, c.scales, c.zint, 32, 4, "gptq", None, c.bias), "rounded scale")
    assert t["scales"][1, 7].item() == np.float16(np.float32(0.1))
    # repack_rows
    qw = m.qweight
    ident = torch.arange(64, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="must not alias"):
        G.repack_rows(qw, ident, 4, out=qw)
    with pytest.raises(ValueError, match="must not alias"):
        G.repack_rows(qw[:4], ident[:32], 4, out=qw.view(-1)[32:32 + 4 * 32].view(4, 32))        # a partial overlap
    with pytest.raises(ValueError, match="perm must hold 64 entries"):
        G.repack_rows(qw, ident[:32], 4)
    with pytest.raises(ValueError, match="perm must be int32"):
        G.repack_rows(qw, ident.long(), 4)
    with pytest.raises(ValueError, match="not a permutation"):
        m2 = build_module(G, dev, make_case(4, 64, 32, 32, "random", seed=17))
        m2.perm[0] = m2.perm[1]
        G.to_gptq_tensors(m2)
    assert torch.equal(G.repack_rows(qw, ident, 4), qw)


# ================================================================================================ 6. C ABI
def sentinel(shape, dev):
    return torch.full(shape, SENT32, dtype=torch.int32, device=dev)


def test_c_abi_status_codes(hip_device):
    from gptq_amd import _lib
    dev = hip_device
    qw = torch.zeros((8, 64), dtype=torch.int32, device=dev)
    out = torch.zeros_like(qw)
    src = torch.arange(64, dtype=torch.int32, device=dev)
    s = torch.ones((2, 64), device=dev)
    z = torch.ones((2, 64), device=dev)
    qz = torch.zeros((2, 8), dtype=torch.int32, device=dev)
    s16 = torch.ones((2, 64), dtype=torch.float16, device=dev)
    fl = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _lib.stream(dev)
    P = _lib.ptr
    ok = {"gptq_repack_rows": [P(qw), P(src), 64, 64, 4, P(out), st],
          "gptq_qzeros_pack": [P(s), P(z), 2, 64, 4, 1, P(qz), P(s16), P(fl), st],
          "gptq_qzeros_unpack": [P(qz), P(s16), 2, 64, 4, 1, P(s), P(z), st]}
    bad = {"gptq_repack_rows": {"bits must be 2, 3, 4 or 8": (4, 5), "in_features must be a multiple of 32": (2, 40),
                                "null pointer": (1, 0), "null pointer ": (5, 0), "must not overlap": (5, P(qw)),
                                "bad sizes": (3, 0)},
           "gptq_qzeros_pack": {"bits must be 2, 3, 4 or 8": (4, 5), "N must be a multiple of 32": (3, 40),
                                "null pointer": (8, 0), "null pointer ": (0, 0), "zero_offset must be": (5, 2),
                                "bad sizes": (2, 0)},
           "gptq_qzeros_unpack": {"bits must be 2, 3, 4 or 8": (4, 5), "N must be a multiple of 32": (3, 40),
                                  "null pointer": (1, 0), "null pointer ": (7, 0), "zero_offset must be": (5, -1),
                                  "bad sizes": (3, -32)}}
    lib = _lib.load()
    with torch.cuda.device(dev):
        for name, args in ok.items():
            for msg, (i, v) in bad[name].items():
                a = list(args)
                a[i] = v
                assert getattr(lib, name)(*a) == 1, f"{name} with argument {i} = {v}"
                with pytest.raises(_lib.GptqHipError, match=f"{name}: invalid argument: {name}: .*{msg.strip()}"):
                    _lib.call(name, *a)
            _lib.call(name, *args)                                                  # and the unedited call is fine
    torch.cuda.synchronize()
    assert lib.gptq_hip_abi_version() == 2


@pytest.mark.parametrize("bits", IR.BITS)
def test_kernels_write_only_their_outputs(hip_device, bits):
    """The three kernels through the C ABI into the middle of sentinel-filled buffers, at N = 160 (the last workgroup
    of the repack is ragged, the last wave of the zero-point kernels has 5 live lanes): the bytes before and after stay."""
    from gptq_amd import _lib
    dev = hip_device
    K, N, Gn = 96, 160, 3
    rows, zw = K // 32 * bits, N // 32 * bits
    rng = np.random.default_rng(bits)
    codes = rng.integers(0, 2 ** bits, (K, N), dtype=np.uint8)
    src = rng.permutation(K).astype(np.int32)
    qw = torch.from_numpy(IR.pack_rows(codes, bits)).to(dev)
    buf = sentinel((rows + 2, N), dev)
    with torch.cuda.device(dev):
        _lib.call("gptq_repack_rows", _lib.ptr(qw), _lib.ptr(torch.from_numpy(src).to(dev)), K, N, bits, _lib.ptr(buf[1:]),
                  _lib.stream(dev))
    torch.cuda.synchronize()
    assert np.array_equal(buf[1:rows + 1].cpu().numpy(), IR.pack_rows(codes[src], bits))
    assert (buf[0] == SENT32).all() and (buf[rows + 1] == SENT32).all()
    # an entry outside 0..K-1 packs code 0 and reads nothing
    src_bad = src.copy()
    src_bad[[0, 37]] = (-1, K)
    want = codes[np.clip(src_bad, 0, K - 1)]
    want[[0, 37]] = 0
    with torch.cuda.device(dev):
        _lib.call("gptq_repack_rows", _lib.ptr(qw), _lib.ptr(torch.from_numpy(src_bad).to(dev)), K, N, bits,
                  _lib.ptr(buf[1:]), _lib.stream(dev))
    torch.cuda.synchronize()
    assert np.array_equal(buf[1:rows + 1].cpu().numpy(), IR.pack_rows(want, bits))
    s = torch.from_numpy((rng.integers(1, 2048, (Gn, N)) / 4096.0).astype(np.float32)).to(dev)
    zint = rng.integers(1, 2 ** bits, (Gn, N))
    z = torch.from_numpy(zint.astype(np.float32)).to(dev) * s
    qz = sentinel((Gn + 2, zw), dev)
    s16 = torch.full((Gn + 2, N), float("nan"), dtype=torch.float16, device=dev)
    fl = sentinel((3,), dev)
    fl[1] = 0
    with torch.cuda.device(dev):
        _lib.call("gptq_qzeros_pack", _lib.ptr(s), _lib.ptr(z), Gn, N, bits, 1, _lib.ptr(qz[1:]), _lib.ptr(s16[1:]),
                  _lib.ptr(fl[1:]), _lib.stream(dev))
    torch.cuda.synchronize()
    assert np.array_equal(qz[1:Gn + 1].cpu().numpy(), IR.pack_qzeros(zint - 1, bits))
    assert (qz[0] == SENT32).all() and (qz[Gn + 1] == SENT32).all()
    assert torch.equal(s16[1:Gn + 1], s.half()) and s16[0].isnan().all() and s16[Gn + 1].isnan().all()
    assert fl.tolist() == [SENT32, 16 if (zint != 2 ** (bits - 1)).any() else 0, SENT32]
    so = torch.full((Gn + 2, N), float("nan"), device=dev)
    zo = torch.full((Gn + 2, N), float("nan"), device=dev)
    with torch.cuda.device(dev):
        _lib.call("gptq_qzeros_unpack", _lib.ptr(qz[1:]), _lib.ptr(s16[1:]), Gn, N, bits, 1, _lib.ptr(so[1:]),
                  _lib.ptr(zo[1:]), _lib.stream(dev))
    torch.cuda.synchronize()
    assert torch.equal(so[1:Gn + 1], s) and torch.equal(zo[1:Gn + 1], z)
    for t in (so, zo):
        assert t[0].isnan().all() and t[Gn + 1].isnan().all()


def test_flag_bits(hip_device):
    """Each flag of gptq_qzeros_pack on its own, one entry of a [2, 64] table at a time."""
    from gptq_amd import interop
    dev = hip_device
    bits = 4
    base_s = torch.full((2, 64), 0.5, device=dev)
    base_z = torch.full((2, 64), 8.0, device=dev) * base_s
    assert interop._qzeros_pack(base_s, base_z, bits, 1)[2] == 0                    # symmetric, exact, in range
    def flags(ds=None, dz=None, off=1):
        s, z = base_s.clone(), base_z.clone()
        if ds is not None:
            s[1, 33] = ds
            z[1, 33] = 8.0 * s[1, 33]
        if dz is not None:
            z[1, 33] = dz
        return interop._qzeros_pack(s, z, bits, off)[2]
    assert flags(dz=3.0 * 0.5) == 16
    assert flags(dz=3.25 * 0.5) == 16 | 1
    assert flags(dz=0.0) == 16 | 2 and flags(dz=0.0, off=0) == 16
    assert flags(dz=16 * 0.5) == 16 | 2 and flags(dz=15 * 0.5) == 16
    assert flags(ds=0.1) == 8
    assert flags(ds=1e-9) == 4 | 8
    assert flags(ds=float("inf")) & 4 and flags(ds=float("nan")) & 4 and flags(ds=0.0) & 4
