"""Mixed-width solves: a width per row in one solve (gptq_fasterquant_rows_mixed), GPTQ.sensitivity, and the driver's
layer_wbits / linear_wbits / sweep_wbits with per-Linear packs.

The reference for a mixed solve is this project's own uniform-width solve of the same rows (pinned to the reference-made
goldens elsewhere): rows are independent problems given H, so the two agree BIT FOR BIT; per-object `error` values are
fp32 sums in another order and are held to 1e-5 relative, the bar of
test_gpu_parity.py::test_joint_solve_of_shared_hessian_objects_matches_separate_solves."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# the width table of the reference fork's quant_bit/linearwise.json
TABLE = {"k_proj": 4, "q_proj": 4, "v_proj": 3, "out_proj": 3, "fc1": 4, "fc2": 3}


@pytest.fixture(scope="module")
def G():
    import gptq_amd
    from gptq_amd import _lib
    _lib.load()
    gptq_amd.gptq.VERBOSE = False
    return gptq_amd


def make_linear(w):
    lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=False, device=w.device, dtype=w.dtype)
    lin.weight.data = w.clone()
    return lin


def _quantizer(G, bits, sym=False):
    q = G.Quantizer()
    q.configure(bits, perchannel=True, sym=sym, mse=False)
    return q


# ------------------------------------------------------------------------------- 1. joint mixed == separate
HEIGHTS, WIDTHS = (40, 24, 72, 56), (4, 3, 2, 8)      # no width boundary on a 16- / 32-row workgroup or MFMA-tile boundary

CASES = [
    pytest.param(640, {}, False, None, id="c640_per_row"),                 # one 512-column super-block + a second launch, far update
    pytest.param(640, dict(groupsize=128, static_groups=True), False, None, id="c640_g128_static"),
    pytest.param(640, dict(groupsize=128, actorder=True), False, None, id="c640_g128_actorder"),
    pytest.param(512, dict(groupsize=64), False, None, id="c512_g64_dynamic"),   # per-block path, stale-column quirk
    pytest.param(320, {}, False, None, id="c320_inverse_form_tail64"),
    pytest.param(640, {}, True, None, id="c640_per_row_sym"),
    pytest.param(640, {}, False, "8", id="c640_per_row_lanes8"),
    pytest.param(640, {}, False, "0", id="c640_per_row_per_block_path"),
]


def _solve_four(G, C, kw, sym, joint):
    gm = G.gptq
    gm.JOINT_SOLVE = joint
    gen = torch.Generator().manual_seed(21)
    objs = []
    for R, bits in zip(HEIGHTS, WIDTHS):
        gp = G.GPTQ(make_linear((torch.randn(R, C, generator=gen) * 0.02).half().cuda()))
        gp.quantizer = _quantizer(G, bits, sym)
        objs.append(gp)
    for _ in range(4):
        x = (torch.randn(1, 300, C, generator=gen) * (1 + torch.arange(C) % 5)).half().cuda()
        for gp in objs:
            gp.add_batch(x, None)
    G.fasterquant_many(objs, blocksize=128, percdamp=0.01, **kw)
    opt = lambda t: None if t is None else t.clone()
    return [dict(codes=o.codes.clone(), weight=o.layer.weight.data.clone(), scale=o.quantizer.scale.clone(),
                 zero=o.quantizer.zero.clone(), perm=opt(o.perm), group_scale=opt(o.group_scale),
                 group_zero=opt(o.group_zero), error=o.error, joint_rows=o.joint_rows, maxq=int(o.quantizer.maxq))
            for o in objs]


@pytest.mark.parametrize("C,kw,sym,lanes", CASES)
def test_joint_mixed_solve_equals_separate_solves(G, monkeypatch, C, kw, sym, lanes):
    """Four objects of widths 4 / 3 / 2 / 8 that share one Hessian: solved as ONE problem with a width per row they come
    out bit for bit as from four uniform solves."""
    if lanes is not None:
        monkeypatch.setenv("GPTQ_QS_LANES", lanes)         # the library reads it per call
    gm = G.gptq
    old = (gm.HESSIAN_DEFER, gm.JOINT_SOLVE)
    gm.HESSIAN_DEFER = 2                                    # (objects share a running Hessian only while updates are deferred)
    try:
        sep = _solve_four(G, C, kw, sym, joint=False)
        one = _solve_four(G, C, kw, sym, joint=True)
    finally:
        gm.HESSIAN_DEFER, gm.JOINT_SOLVE = old
    for a, b, R, bits in zip(sep, one, HEIGHTS, WIDTHS):
        for key in ("codes", "weight", "scale", "zero", "perm", "group_scale", "group_zero"):
            assert (a[key] is None) == (b[key] is None), key
            if a[key] is not None:
                assert torch.equal(a[key], b[key]), (key, bits)
        assert abs(a["error"] - b["error"]) <= 1e-5 * abs(a["error"]), (a["error"], b["error"])
        assert a["maxq"] == b["maxq"] == 2 ** bits - 1
        assert int(b["codes"].max()) <= 2 ** bits - 1
        assert a["joint_rows"] == R
        assert b["joint_rows"] == sum(HEIGHTS) == 192


# ------------------------------------------------------------------------------- 2. uniform row_bits == the old entry
def _problem(R, C, seed):
    gen = torch.Generator().manual_seed(seed)
    W = (torch.randn(R, C, generator=gen) * 0.02).cuda()
    X = (torch.randn(1200, C, generator=gen) * (1 + torch.arange(C) % 5)).cuda()
    H = (2.0 / 1200) * (X.t() @ X)
    return W, H


@pytest.mark.parametrize("kw", [dict(groupsize=-1, actorder=False, static_groups=False),
                                dict(groupsize=128, actorder=True, static_groups=True)], ids=["per_row", "g128_static_act"])
def test_uniform_row_bits_equal_the_uniform_entry(G, hip_device, kw):
    W, H = _problem(96, 512, 5)
    q = _quantizer(G, 4)
    out = []
    for row_bits in (None, [4] * 96):
        st = G.gptq._enqueue_rows(hip_device, W.clone(), H.clone(), q, None, 128, 0.01, kw["groupsize"], kw["actorder"],
                                  kw["static_groups"], row_bits=row_bits)
        G.gptq._check_solved(st)
        out.append(st)
    for key in ("W", "H", "scale", "zero", "gscale", "gzero", "perm", "codes", "stat", "row_loss"):
        a, b = out[0][key], out[1][key]
        assert (a is None) == (b is None), key
        if a is not None:
            assert torch.equal(a, b), key


def test_row_bits_are_validated_on_the_host(G, hip_device):
    W, H = _problem(8, 128, 6)
    q = _quantizer(G, 4)
    for bad in ([4] * 7, [4] * 7 + [0], [4] * 7 + [9], [4.0] * 8):
        with pytest.raises(ValueError):
            G.gptq._enqueue_rows(hip_device, W.clone(), H.clone(), q, None, 128, 0.01, -1, False, False, row_bits=bad)


# ------------------------------------------------------------------------------- 3. sensitivity
def _calibrated(G, W, xs, bits):
    gp = G.GPTQ(make_linear(W))
    gp.quantizer = _quantizer(G, bits)
    for x in xs:
        gp.add_batch(x, None)
    return gp


def test_sensitivity_is_one_solve_and_leaves_no_trace(G, hip_device):
    gen = torch.Generator().manual_seed(9)
    W = (torch.randn(64, 512, generator=gen) * 0.02).half().cuda()
    xs = [(torch.randn(1, 300, 512, generator=gen) * (1 + torch.arange(512) % 5)).half().cuda() for _ in range(2)]
    widths = (2, 3, 4, 8)
    want = {}
    for bits in widths:                                     # fasterquant's `error` on a clone at that width
        ref = _calibrated(G, W, xs, bits)
        ref.fasterquant(blocksize=128, percdamp=0.01)
        want[bits] = ref.error
    untouched = _calibrated(G, W, xs, 4)
    gp = _calibrated(G, W, xs, 4)
    before = (gp.layer.weight.data.clone(), gp.H.clone(), gp.quantizer.scale.clone(), gp.nsamples)
    got = gp.sensitivity(wbits=widths, blocksize=128, percdamp=0.01)
    assert sorted(got) == sorted(widths)
    for bits in widths:
        assert abs(got[bits] - want[bits]) <= 1e-5 * abs(want[bits]), (bits, got[bits], want[bits])
    assert got[2] > got[3] > got[4] > got[8] > 0
    assert torch.equal(gp.layer.weight.data, before[0])
    assert torch.equal(gp.H, before[1])
    assert torch.equal(gp.quantizer.scale, before[2])
    assert gp.nsamples == before[3]
    gp.fasterquant(blocksize=128, percdamp=0.01)
    untouched.fasterquant(blocksize=128, percdamp=0.01)
    assert torch.equal(gp.codes, untouched.codes)
    assert torch.equal(gp.layer.weight.data, untouched.layer.weight.data)
    assert torch.equal(gp.quantizer.scale, untouched.quantizer.scale)
    assert torch.equal(gp.quantizer.zero, untouched.quantizer.zero)
    assert gp.error == untouched.error
    assert gp.joint_rows == 64


def test_sensitivity_keeps_raising_out_of_scope(G, hip_device):
    gp = G.GPTQ(make_linear(torch.zeros(4, 32, device=hip_device)))
    gp.quantizer = G.Quantizer()
    gp.quantizer.configure(4, perchannel=True, sym=False, trits=True)
    with pytest.raises(NotImplementedError):
        gp.sensitivity()
    gp.quantizer = _quantizer(G, 4)
    for kw in ({"lut_quant": True}, {"non_linear_quant": True}, {"columnwise": True}):
        with pytest.raises(NotImplementedError):
            gp.sensitivity(**kw)
    with pytest.raises(ValueError):
        gp.sensitivity(wbits=(4, 9))


# ------------------------------------------------------------------------------- 4. driver
S = 64


def _tiny_opt(seed=0):
    from transformers import OPTConfig, OPTForCausalLM
    cfg = OPTConfig(vocab_size=256, hidden_size=128, ffn_dim=512, num_hidden_layers=2, num_attention_heads=4,
                    max_position_embeddings=128, word_embed_proj_dim=128, do_layer_norm_before=True,
                    dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, layerdrop=0.0)
    torch.manual_seed(seed)
    m = OPTForCausalLM(cfg).half().eval()
    m.seqlen = S
    return m


def _tokens():
    gen = torch.Generator().manual_seed(2)
    calib = [(torch.randint(0, 256, (1, S), generator=gen), None) for _ in range(4)]
    test = torch.randint(0, 256, (1, 4 * S), generator=gen)
    return calib, test


def _run(dev, **kw):
    from gptq_amd.sequential import QuantArgs, opt_sequential, quantize_sequential
    model = _tiny_opt()
    quantizers = opt_sequential(model, _tokens()[0], dev, QuantArgs(nsamples=4, static_groups=True, **kw))
    return model, quantizers, list(quantize_sequential.last_records)


@pytest.fixture(scope="module")
def table_run(G, hip_device):
    """The fork's table, with a sweep at 3 and 4 bits (shared, read-only: packing tests work on copies)."""
    return _run(hip_device, linear_wbits=dict(TABLE), sweep_wbits=(3, 4))


def test_driver_runs_a_linear_width_table(G, table_run):
    model, quantizers, records = table_run
    sd = model.state_dict()
    assert len(quantizers) == 12
    for name, q in quantizers.items():
        w = TABLE[name.split(".")[-1]]
        assert q.wbits == w and int(q.maxq) == 2 ** w - 1
        weight = sd[name + ".weight"].float()
        assert max(len(torch.unique(row)) for row in weight) <= 2 ** w, name
    by_name = {r["name"]: r for r in records}
    for r in records:
        assert r["wbits"] == TABLE[r["name"].split(".")[-1]]
    for i in range(2):
        qkv = [by_name[f"model.decoder.layers.{i}.self_attn.{n}"]["joint_rows"] for n in ("q_proj", "k_proj", "v_proj")]
        assert qkv == [384, 384, 384]                      # 4 / 4 / 3 bits, one solve
        assert by_name[f"model.decoder.layers.{i}.fc1"]["joint_rows"] == 512


def test_driver_sweep_reports_errors_by_width(G, table_run):
    _, _, records = table_run
    for r in records:
        sweep = r["errors_by_wbits"]
        assert sorted(sweep) == [3, 4]
        assert sweep[3] > sweep[4] > 0
        assert abs(sweep[r["wbits"]] - r["error"]) <= 1e-5 * abs(r["error"]), (r["name"], sweep, r["error"])


def test_driver_uniform_table_equals_wbits(G, hip_device):
    a, qa, ra = _run(hip_device, wbits=4)
    b, qb, rb = _run(hip_device, wbits=2, linear_wbits={k: 4 for k in TABLE})
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for n in qa:
        assert torch.equal(qa[n].scale, qb[n].scale) and torch.equal(qa[n].zero, qb[n].zero)
    assert [r["error"] for r in ra] == [r["error"] for r in rb]


def test_driver_layer_widths(G, hip_device):
    model, quantizers, records = _run(hip_device, layer_wbits=[4, 3])
    sd = model.state_dict()
    for name, q in quantizers.items():
        w = 4 if ".layers.0." in name else 3
        assert q.wbits == w
        assert max(len(torch.unique(row)) for row in sd[name + ".weight"].float()) <= 2 ** w
    assert [r["wbits"] for r in records] == [4] * 6 + [3] * 6


def test_mixed_model_packs_scores_and_reloads(G, hip_device, table_run, tmp_path):
    import copy
    from gptq_amd.sequential import eval_ppl, make_packed_skeleton, pack_model, packed_wbits
    dense, quantizers, _ = table_run
    test = _tokens()[1]
    model = copy.deepcopy(dense)
    ppl_dense = eval_ppl(model, test, hip_device)
    pack_model(model, quantizers, bits=None, multi_token=True)
    layer = model.model.decoder.layers[1]
    assert type(layer.self_attn.q_proj) is G.Quant4Linear and type(layer.self_attn.k_proj) is G.Quant4Linear
    assert type(layer.self_attn.v_proj) is G.Quant3Linear and type(layer.self_attn.out_proj) is G.Quant3Linear
    assert type(layer.fc1) is G.Quant4Linear and type(layer.fc2) is G.Quant3Linear
    widths = packed_wbits(model)
    assert widths == {n: TABLE[n.split(".")[-1]] for n in quantizers}
    ppl_packed = eval_ppl(model, test, hip_device)
    print(f"mixed table: PPL dense {ppl_dense:.5f} packed {ppl_packed:.5f}")
    assert abs(ppl_packed - ppl_dense) <= 2e-2 * ppl_dense      # test_gpu_driver.py's bar for a uniform packed model

    path = tmp_path / "mixed.pt"
    torch.save(model.state_dict(), path)
    fresh = _tiny_opt(seed=1)
    make_packed_skeleton(fresh, list(widths), bits=widths, multi_token=True)
    fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)
    assert packed_wbits(fresh) == widths
    assert eval_ppl(fresh, test, hip_device) == ppl_packed


def test_mixed_grouped_model_packs_per_width(G, hip_device):
    from gptq_amd.sequential import make_packed_skeleton, pack_model, packed_wbits
    model, quantizers, _ = _run(hip_device, linear_wbits=dict(TABLE), groupsize=32)
    dense = {n: model.state_dict()[n + ".weight"].clone() for n in quantizers}
    pack_model(model, quantizers, multi_token=True)
    mods = dict(model.named_modules())
    for n in quantizers:
        m = mods[n]
        assert type(m) is G.QuantGroupLinear and m.bits == TABLE[n.split(".")[-1]] and m.groupsize == 32
        W = G.quant.dequant_packed(m.qweight.to(hip_device), m.scales.to(hip_device),
                                   quantizers[n].group_zero.t().contiguous().to(hip_device), m.bits, 32, dtype=torch.float32)
        assert torch.equal(W.half().cpu(), dense[n].cpu()), n
    widths = packed_wbits(model)
    fresh = _tiny_opt(seed=1)
    make_packed_skeleton(fresh, list(widths), bits=widths, groupsize=32)
    fresh.load_state_dict(model.state_dict(), strict=True)
