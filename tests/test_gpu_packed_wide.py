"""2- and 8-bit packing end to end on the GPU: pack, dequant, mat-vec and dequant GEMM against tests/packed_ref_wide.py.

Exact part: dyadic inputs for which every fp32 operation is exact (packed_ref_wide's docstring; tests/
test_packed_wide_cpu.py proves it for every table row on the CPU), so a kernel's output must EQUAL the fp64 reference --
`torch.equal`, no tolerance.  Sentinels round every output buffer stand in for a sanitizer.  Float part: one realistic
case per width against the bar of the 3-/4-bit GEMM tests, 5e-5 (|x| @ |Wdeq| + |bias|).  End to end: a tiny LLaMA at 2
bits (groupsize 32, act-order, dynamic groups) and a tiny OPT at 8 bits per row through the driver, pack_model, save and
load.
"""
import numpy as np
import pytest
import torch

import packed_ref_wide as R

pytestmark = pytest.mark.gpu

BITS = list(R.WIDE_BITS)
SENT32 = 0x7FC5A5A5                                                                 # a quiet-NaN bit pattern
SENT16 = 0x7E5A                                                                    # fp16 / bf16 NaN bit pattern


@pytest.fixture(scope="module")
def G():
    import gptq_amd
    from gptq_amd import _lib
    _lib.load()
    return gptq_amd


@pytest.fixture(scope="module")
def Q():
    from gptq_amd import quant_cuda
    return quant_cuda


def sentinel(shape, dtype, dev):
    t = torch.empty(shape, dtype=dtype, device=dev)
    if t.element_size() == 4:
        t.view(torch.int32).fill_(SENT32)
    elif t.element_size() == 2:
        t.view(torch.int16).fill_(SENT16)
    else:
        t.fill_(0xA5)
    return t


def bits_of(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def assert_untouched(t, what):
    want = sentinel(t.shape, t.dtype, t.device)
    assert torch.equal(bits_of(t.contiguous()), bits_of(want)), f"stray write into {what}"


# ================================================================================================ GEMM, exact
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("row", R.GEMM_EXACT, ids=[R.case_id(r) for r in R.GEMM_EXACT])
def test_gemm_exact(G, hip_device, bits, row):
    """fp32 output == reference, a second call gives the same bits, the rounded output is one rounding of the exact
    value, bias=None as well (packed_ref.run_gemm_exact), for every M of the row."""
    K, N, gs, Ms, xd, perm = row
    c = R.dyadic_case(bits, K, N, gs, max(Ms), perm=perm, seed=1, x_dtype=xd)
    assert c.headroom_mv < 1.0
    R.run_gemm_exact(G, hip_device, c, Ms)


@pytest.mark.parametrize("bits", BITS)
def test_gemm_chunk_boundary_inside_group(hip_device, bits):
    """K = 1408 is 44 k-steps; the K split must cut them into chunks that are no multiple of the 4 steps of a 128-group
    (test_gemm_exact's 1408 rows then cross it)."""
    from gptq_amd import _lib
    lib = _lib.load()
    K, N, gs = 1408, 1001, 128
    for m in (1, 3, 16, 17):
        nbytes = lib.gptq_quant_gemm_workspace_bytes(m, K, N, bits, gs)
        assert nbytes > 0 and nbytes % (4 * m * N) == 0
        S = nbytes // (4 * m * N)
        chunk_steps = -(-(K // 32) // S)
        assert S > 1 and (chunk_steps * 32) % gs != 0, (m, S, chunk_steps)


@pytest.mark.parametrize("ydt", [torch.float32, torch.float16], ids=["y32", "y16"])
@pytest.mark.parametrize("perm", [False, True], ids=["plain", "perm"])
@pytest.mark.parametrize("bits", BITS)
def test_gemm_strides_and_sentinels(hip_device, bits, perm, ydt):
    """ldx = K + 24 and ldy = N + 5 through the C ABI (x rows that are not 16-byte aligned: element loads): the body equals
    the reference; the padding columns of y, the 4096 bytes after the reported workspace size and qweight keep their
    bits.  K = 1408 splits K at small M, K = 96 never does."""
    from gptq_amd import _lib
    lib = _lib.load()
    dev = hip_device
    for K, gs in ((1408, 128), (96, 32)):
        for N in (3, 257):
            Ms = (1, 17, 129)
            c = R.dyadic_case(bits, K, N, gs, max(Ms), perm=perm, seed=47, x_dtype="f16")
            qw, s, z, b, p = R.dev_tensors(c, dev)
            qw_before = qw.clone()
            ref = torch.from_numpy(c.ref).to(dev).float().to(ydt)
            for m in Ms:
                xbig = sentinel((m, K + 24), torch.float16, dev)
                xbig[:, :K] = c.x[:m].to(dev)
                query = lib.gptq_quant_gemm_perm_workspace_bytes if perm else lib.gptq_quant_gemm_workspace_bytes
                nbytes = query(m, K, N, bits, gs)
                ws = sentinel((nbytes + 4096,), torch.uint8, dev)
                y = sentinel((m, N + 5), ydt, dev)
                args = [_lib.ptr(xbig), _lib.dtype_code(xbig), K + 24, m, _lib.ptr(qw), _lib.ptr(s), _lib.ptr(z)]
                if perm:
                    args.append(_lib.ptr(p))
                args += [_lib.ptr(b), K, N, bits, gs, _lib.ptr(y), _lib.dtype_code(y), N + 5, _lib.ptr(ws), nbytes,
                         _lib.stream(dev)]
                with torch.cuda.device(dev):
                    _lib.call("gptq_quant_gemm_perm" if perm else "gptq_quant_gemm", *args)
                torch.cuda.synchronize()
                R.assert_equal_bits(y[:, :N].contiguous(), ref[:m], f"ldx, ldy padded, {bits}-bit K={K} N={N} M={m}")
                assert_untouched(y[:, N:], f"the padding columns of y (N={N}, M={m})")
                assert_untouched(ws[nbytes:], f"the bytes after the workspace (N={N}, M={m}, {nbytes} bytes)")
                assert_untouched(xbig[:, K:], "the padding columns of x")
            assert torch.equal(qw, qw_before), "qweight was written"


# ================================================================================================ mat-vec, exact
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("row", R.MATVEC_EXACT, ids=[R.case_id(r) for r in R.MATVEC_EXACT])
def test_matvec_exact(Q, hip_device, bits, row):
    """Per-row entries and the grouped entry (with and without perm), fp32 and fp16 x, `mul` preloaded with the bias:
    every add is exact, so the order of the cross-workgroup atomics does not matter and the result is bit-equal."""
    K, N, gs = row
    for perm in ((False, True) if gs > 0 else (False,)):
        c = R.dyadic_case(bits, K, N, gs, 1, perm=perm, seed=2, x_dtype="f16")
        assert c.headroom_mv < 1.0
        for entry in R.matvec_entries(gs):
            R.run_matvec_exact(Q, hip_device, c, entry)
            R.run_matvec_exact(Q, hip_device, c, entry, "second call")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("width", [1, 130, 1000])
def test_matvec_sentinels_and_misaligned_mat(Q, hip_device, bits, width):
    """`mul` is a slice of a sentinel-filled buffer: its neighbours keep their bits, and so does `mat`.  width 1000 also
    runs with `mat` only 4-byte aligned: the one-column-per-thread kernel at a width % 4 == 0."""
    K = 1408
    for gs in (-1, 128):
        for perm in ((False, True) if gs > 0 else (False,)):
            c = R.dyadic_case(bits, K, width, gs, 1, perm=perm, seed=53, x_dtype="f16")
            qw, s, z, b, p = R.dev_tensors(c, hip_device)
            mats = [qw]
            if width == 1000:
                flat = torch.zeros(qw.numel() + 4, dtype=torch.int32, device=hip_device)
                flat[1:1 + qw.numel()] = qw.reshape(-1)
                off = flat[1:1 + qw.numel()].view(qw.shape)
                assert off.data_ptr() % 16 == 4 and off.is_contiguous()
                mats.append(off)
            ref = torch.from_numpy(c.ref[0]).to(hip_device).float()
            for mat in mats:
                before = mat.clone()
                for entry in R.matvec_entries(gs):
                    buf = sentinel((256 + width + 256,), torch.float32, hip_device)
                    mul = buf[256:256 + width]
                    mul.copy_(b)
                    x = c.x[0].to(hip_device).to(torch.float16 if entry.endswith("h") else torch.float32)
                    if gs > 0:
                        Q.vecquant_matmul_grouped(x, mat, mul, s, z, bits, gs, perm=p)
                    else:
                        fn = {2: Q.vecquant2matmul, 8: Q.vecquant8matmul}[bits]
                        fn(x, mat, mul, s.reshape(-1, 1), z.reshape(-1, 1))
                    torch.cuda.synchronize()
                    R.assert_equal_bits(mul.clone(), ref, f"mat-vec into a slice, {entry} width {width} g{gs}")
                    assert_untouched(buf[:256], f"the 256 floats before mul ({entry}, width {width})")
                    assert_untouched(buf[256 + width:], f"the 256 floats after mul ({entry}, width {width})")
                assert torch.equal(mat, before), "mat was written"


# ================================================================================================ modules, exact
@pytest.mark.parametrize("kind", ["Quant2Linear", "Quant8Linear", "QuantGroupLinear-2", "QuantGroupLinear-8",
                                  "QuantGroupLinear-2-act", "QuantGroupLinear-8-act"])
def test_modules_exact(G, hip_device, kind):
    """A 1-token forward equals row 0 of the multi-token forward bit for bit, and both equal the reference."""
    parts = kind.split("-")
    M = 5
    if parts[0] == "QuantGroupLinear":
        bits, act = int(parts[1]), parts[-1] == "act"
        K, N, gs = 1056, 130, 96
        c = R.dyadic_case(bits, K, N, gs, M, perm=act, seed=41, x_dtype="f16")
        m = G.QuantGroupLinear(bits, gs, K, N, multi_token=True, act_order=act)
    else:
        bits = 2 if parts[0] == "Quant2Linear" else 8
        K, N, gs = 416, 257, -1
        c = R.dyadic_case(bits, K, N, gs, M, seed=43, x_dtype="f16")
        m = getattr(G, parts[0])(K, N, multi_token=True)
    qw, s, z, b, perm = R.dev_tensors(c, hip_device)
    m = m.to(hip_device)
    m.qweight, m.bias = qw, b
    m.scales, m.zeros = (s, z) if gs > 0 else (s.reshape(-1, 1), z.reshape(-1, 1))
    if perm is not None:
        m.perm = perm
    for xd in (torch.float16, torch.bfloat16):
        x = c.x.to(hip_device).to(xd).reshape(1, M, K)
        want = torch.from_numpy(c.ref).to(hip_device).float().to(xd)
        multi = m(x)
        assert multi.shape == (1, M, N) and multi.dtype == xd
        R.assert_equal_bits(multi[0], want, f"{kind} multi-token {xd}")
        one = m(x[:, :1])
        assert one.shape == (1, 1, N) and one.dtype == xd
        R.assert_equal_bits(one[0, 0], multi[0, 0], f"{kind} 1-token against row 0 of the multi-token forward {xd}")
        R.assert_equal_bits(one[0, 0], want[0], f"{kind} 1-token {xd}")


# ================================================================================================ pack / dequant
def _pack_wrapping(codes_i64, bits):
    """The pack rule on codes outside [0, 2^bits - 1], as the 4-bit kernel treats them: each code as a uint32, shifted
    and OR-ed unmasked."""
    K, N = codes_i64.shape
    cpw = 32 // bits
    c = (codes_i64.reshape(K // cpw, cpw, N) & 0xFFFFFFFF).astype(np.uint64)
    words = np.zeros((K // cpw, N), dtype=np.uint64)
    for j in range(cpw):
        words |= (c[:, j] << np.uint64(bits * j)) & np.uint64(0xFFFFFFFF)
    return words.astype(np.uint32).view(np.int32)


@pytest.mark.parametrize("bits", BITS)
def test_pack_equals_the_numpy_layout(hip_device, bits):
    """pack_codes (wide tiles for 16-byte-aligned code rows, narrow tiles otherwise, both through the C ABI with sentinel
    rows round qweight), _pack and pack_grouped (with and without perm) on out in {1, 63, 513} x in in {32, 96, 1056}."""
    from gptq_amd import _lib
    from gptq_amd.quant import _pack, pack_codes, pack_grouped
    dev = hip_device
    maxq = 2 ** bits - 1
    for n_out in R.PACK_OUT:
        for K in R.PACK_IN:
            rng = np.random.default_rng([bits, n_out, K])
            rows = K // 32 * bits
            codes = rng.integers(0, maxq + 1, (K, n_out), dtype=np.uint8)                   # [in, out]
            want = torch.from_numpy(R.pack(codes, bits)).to(dev)
            ct = torch.from_numpy(codes.T.copy()).to(dev)                                   # [out, in]
            assert torch.equal(pack_codes(ct, bits), want), f"pack_codes {n_out}x{K}"
            for ld in (K, K + 3):            # K: 16-byte-aligned rows -> the wide-tile kernel; K + 3: the narrow one
                cbuf = torch.zeros((n_out, ld), dtype=torch.uint8, device=dev)
                cbuf[:, :K] = ct
                assert (ld % 16 == 0 and cbuf.data_ptr() % 16 == 0) == (ld == K)
                buf = sentinel((rows + 2, n_out), torch.int32, dev)
                with torch.cuda.device(dev):
                    _lib.call("gptq_pack_codes", _lib.ptr(cbuf), ld, n_out, K, bits, _lib.ptr(buf[1:]), _lib.stream(dev))
                torch.cuda.synchronize()
                assert torch.equal(buf[1:rows + 1], want), f"gptq_pack_codes {n_out}x{K} ld={ld}"
                assert_untouched(buf[:1], "the row before qweight (pack_codes)")
                assert_untouched(buf[rows + 1:], "the row after qweight (pack_codes)")
            # per-row grids: weights exactly on a dyadic grid, in every weight type
            sc = np.ldexp(1.0, -rng.integers(6, 9, n_out))
            zint = rng.integers(0, maxq + 1, n_out)
            w = (sc[None, :] * (codes.astype(np.float64) - zint[None, :])).T.copy()         # [out, in]
            s_t = torch.from_numpy(sc.astype(np.float32)).to(dev)
            zs_t = torch.from_numpy((zint * sc).astype(np.float32)).to(dev)
            for wdt in (torch.float32, torch.float16, torch.bfloat16):
                wt = torch.from_numpy(w).to(wdt).to(dev)
                assert torch.equal(wt.double().cpu(), torch.from_numpy(w))                  # representable
                assert torch.equal(_pack(wt, s_t, zs_t, bits), want), f"_pack {n_out}x{K} {wdt}"
            # grouped grids, with and without perm
            gs = 32
            for perm in (False, True):
                c = R.dyadic_case(bits, K, n_out, gs, 1, perm=perm, seed=59)
                grp = np.arange(K) // gs
                wst = c.scales[grp].astype(np.float64) * c.codes - c.zeros[grp]            # on the grid, storage order
                wg = np.empty_like(wst)
                wg[c.perm if perm else np.arange(K)] = wst
                wt = torch.from_numpy(wg.T.copy()).float().to(dev).contiguous()
                _, s, z, _, p = R.dev_tensors(c, dev)
                got = pack_grouped(wt, s, z, gs, bits, p)
                assert torch.equal(got, torch.from_numpy(c.qweight).to(dev)), f"pack_grouped {n_out}x{K} perm={perm}"


@pytest.mark.parametrize("bits", BITS)
def test_pack_out_of_range_behaves_like_4_bits(hip_device, bits):
    """_pack does not clamp: a weight that lands on code -1 or 2^bits is shifted and OR-ed as a uint32, like the 4-bit
    kernel; pack_codes ORs codes above 2^bits - 1 into their neighbours; pack_grouped clamps."""
    from gptq_amd.quant import _pack, pack_codes, pack_grouped
    dev = hip_device
    K, n_out = 96, 63
    maxq = 2 ** bits - 1
    rng = np.random.default_rng([bits, 5])
    codes = rng.integers(-1, maxq + 2, (K, n_out)).astype(np.int64)                        # -1 and maxq + 1 included
    assert codes.min() == -1 and codes.max() == maxq + 1
    s = torch.full((n_out,), 2.0 ** -6, device=dev)
    z = torch.zeros(n_out, device=dev)
    wt = torch.from_numpy((codes * 2.0 ** -6).T.copy()).float().to(dev)
    assert torch.equal(_pack(wt, s, z, bits).cpu(), torch.from_numpy(_pack_wrapping(codes, bits)))
    big = rng.integers(0, 256, (K, n_out)).astype(np.int64)
    got = pack_codes(torch.from_numpy(big.T.copy().astype(np.uint8)).to(dev), bits)
    assert torch.equal(got.cpu(), torch.from_numpy(_pack_wrapping(big, bits)))
    gq = pack_grouped(wt, s.reshape(1, -1).expand(K // 32, -1).contiguous(), torch.zeros(K // 32, n_out, device=dev), 32,
                      bits)
    assert np.array_equal(R.unpack(gq.cpu().numpy(), bits), np.clip(codes, 0, maxq).astype(np.uint8))


@pytest.mark.parametrize("gs", [-1, 32, 96])
@pytest.mark.parametrize("bits", BITS)
def test_dequant_packed_exact(hip_device, bits, gs):
    """dequant_packed with and without perm == scale * (code - zero) in fp32, rounded once to the output type."""
    from gptq_amd.quant import dequant_packed
    K, N = 1056, 63
    g = gs if gs > 0 else K
    rng = np.random.default_rng([bits, g, 11])
    codes = rng.integers(0, 2 ** bits, (K, N), dtype=np.uint8)
    qw = torch.from_numpy(R.pack(codes, bits)).to(hip_device)
    sc = torch.from_numpy(rng.uniform(1e-3, 2e-2, (K // g, N)).astype(np.float32))
    zint = torch.from_numpy(rng.integers(0, 2 ** bits, (K // g, N)).astype(np.float32))
    grp = torch.arange(K) // g
    dense = (sc[grp] * (torch.from_numpy(R.unpack(qw.cpu().numpy(), bits)).float() - zint[grp])).t().contiguous()  # [N, K]
    p = torch.from_numpy(rng.permutation(K).astype(np.int32))
    scattered = torch.empty_like(dense)
    scattered[:, p.long()] = dense                          # storage row j -> input column perm[j]
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        W = dequant_packed(qw, sc.to(hip_device), zint.to(hip_device), bits, gs, dtype=dt)
        R.assert_equal_bits(W.cpu(), dense.to(dt), f"dequant {bits}-bit g{gs} {dt}")
        W = dequant_packed(qw, sc.to(hip_device), zint.to(hip_device), bits, gs, dtype=dt, perm=p.to(hip_device))
        R.assert_equal_bits(W.cpu(), scattered.to(dt), f"dequant perm {bits}-bit g{gs} {dt}")


# ================================================================================================ float bar
@pytest.mark.parametrize("bits", BITS)
def test_realistic_case_within_the_float_bar(G, Q, hip_device, bits):
    """Real min/max grids against activations with a mean: the GEMM stays within 5e-5 (|x| @ |Wdeq| + |bias|) of the fp64
    reference per element (the bar of the 3-/4-bit GEMM tests), and its M = 1 row and the mat-vec agree under the same
    bar."""
    K, N, gs, M = 1024, 260, 128, 33
    dev = hip_device
    for xd in ("f16", "bf16"):
        c = R.realistic_case(bits, K, N, gs, M, seed=6, x_dtype=xd)
        qw, s, z, b, _ = R.dev_tensors(c, dev)
        bar = 5e-5 * (np.abs(c.xg) @ np.abs(c.Wdeq) + np.abs(c.bias.astype(np.float64)))
        y = G.quant_matmul(c.x.to(dev), qw, s, z, bits, gs, bias=b, out_dtype=torch.float32)
        err = np.abs(y.double().cpu().numpy() - c.ref)
        print(f"{bits}-bit {xd}: GEMM worst err / bar {float((err / bar).max()):.3e}")
        assert (err <= bar).all(), float((err / bar).max())
        y1 = G.quant_matmul(c.x[:1].to(dev), qw, s, z, bits, gs, bias=b, out_dtype=torch.float32)
        if xd == "f16":
            mul = b.clone()
            Q.vecquant_matmul_grouped(c.x[0].to(dev), qw, mul, s, z, bits, gs)
            d = np.abs(mul.double().cpu().numpy() - y1[0].double().cpu().numpy())
            print(f"{bits}-bit: mat-vec against the GEMM's M = 1 row, worst difference / bar {float((d / bar[0]).max()):.3e}")
            assert (d <= bar[0]).all(), float((d / bar[0]).max())
            assert (np.abs(mul.double().cpu().numpy() - c.ref[0]) <= bar[0]).all()


# ================================================================================================ driver end to end
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


@pytest.mark.parametrize("family,bits", [("llama", 2), ("opt", 8)])
def test_model_pack_save_load(G, hip_device, tmp_path, family, bits):
    """LLaMA: wbits 2, groupsize 32, act-order with dynamic groups (the perm format).  OPT: wbits 8, per-row grids.
    Every packed layer dequantizes to exactly its fake-quantized weight; eval_ppl through the packed forward stays within
    the relative bar of the 4-bit grouped test (5e-3); a saved and reloaded checkpoint scores bit-identically."""
    import gptq_amd.gptq as gmod
    from gptq_amd.modelutils import find_layers
    from gptq_amd.quant import dequant_packed
    from gptq_amd.sequential import (QuantArgs, eval_ppl, llama_sequential, make_packed_skeleton, opt_sequential,
                                     pack_model)
    gmod.VERBOSE = False
    build = _tiny_opt if family == "opt" else _tiny_llama
    model = build()
    S = model.seqlen
    gen = torch.Generator().manual_seed(2)
    calib = [(torch.randint(0, 256, (1, S), generator=gen), None) for _ in range(4)]
    test = torch.randint(0, 256, (1, 4 * S), generator=gen)
    if family == "opt":
        gs, act = -1, False
        quantizers = opt_sequential(model, calib, hip_device, QuantArgs(wbits=bits, nsamples=4, static_groups=True))
    else:
        gs, act = 32, True
        quantizers = llama_sequential(model, calib, hip_device, QuantArgs(wbits=bits, nsamples=4, groupsize=gs,
                                                                           act_order=True, true_sequential=True))
        for q in quantizers.values():
            assert q.groupsize == gs and not q.static_groups and q.perm is not None and q.group_scale is not None
    layers = find_layers(model)
    fake = {n: layers[n].weight.data.clone() for n in quantizers}
    ppl_dense = eval_ppl(model, test, hip_device)
    model.cpu()

    pack_model(model, quantizers, bits=bits, multi_token=True)
    packed_layers = {n: m for n, m in model.named_modules() if n in quantizers}
    for n, q in quantizers.items():
        m = packed_layers[n]
        K = fake[n].shape[1]
        assert m.qweight.shape == (K // 32 * bits, fake[n].shape[0]) and m.multi_token
        if family == "opt":
            assert isinstance(m, G.Quant8Linear)
            W = dequant_packed(m.qweight.to(hip_device), q.scale.float().reshape(1, -1).to(hip_device),
                               q.zero.float().reshape(1, -1).to(hip_device), bits, -1, dtype=fake[n].dtype)
        else:
            assert isinstance(m, G.QuantGroupLinear) and m.bits == 2 and m.act_order and "perm" in m.state_dict()
            W = dequant_packed(m.qweight.to(hip_device), q.group_scale.t().contiguous(), q.group_zero.t().contiguous(),
                               bits, gs, dtype=fake[n].dtype, perm=m.perm.to(hip_device))
        assert torch.equal(W.cpu(), fake[n].cpu()), n
    ppl_packed = eval_ppl(model, test, hip_device)
    print(f"{family} {bits}-bit: PPL dense {ppl_dense:.5f} packed {ppl_packed:.5f} "
          f"({abs(ppl_packed - ppl_dense) / ppl_dense:.2e} relative)")
    assert abs(ppl_packed - ppl_dense) <= 5e-3 * ppl_dense

    path = tmp_path / "packed.pt"
    torch.save(model.state_dict(), path)
    fresh = build(seed=1)
    make_packed_skeleton(fresh, list(quantizers), bits=bits, multi_token=True, groupsize=gs, act_order=act)
    fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)
    assert eval_ppl(fresh, test, hip_device) == ppl_packed
