"""The packed forward kernels (csrc/qgemm.hip, csrc/matvec.hip) and the pack / dequant kernels against tests/packed_ref.py.

Exact part: dyadic inputs for which every fp32 operation is exact (packed_ref's docstring; tests/test_packed_ref_cpu.py
proves it for every table entry on the CPU), so a kernel's output must EQUAL the fp64 reference -- `torch.equal`, no
tolerance -- and any indexing slip (group row, ragged tail, partial column quad, perm entry, lost or doubled k-step)
fails.  Canaries round every output buffer stand in for a sanitizer.  Float part: activations that are not zero-mean randn
against a bar proportional to the contract magnitude T.

Where each path is covered:
  odd N, scalar packed-word path, partial column quads ....... test_gemm_exact (N = 1, 3, 5, 63, 65, 130, 255, 257, 1001)
  qweight / x only 4- / 2-byte aligned, padded x rows ........ test_gemm_misaligned_views
  mat only 4-byte aligned (VW = 1 at a width % 4 == 0) ....... test_matvec_misaligned_mat
  groupsize 64 / 96 / 256 / 512 / K, ragged last X tile ....... test_gemm_exact, test_matvec_exact
  split-K chunk boundary inside a group ...................... test_gemm_chunk_boundary_inside_group
  ldy > N, workspace tail .................................... test_gemm_canaries
  plan boundaries in M (16/17, 32/33, 64/65, 128/129) ......... test_gemm_exact
  mat-vec groups longer than a workgroup, ragged workgroup ... test_matvec_exact (in_f 416, groupsize 256 / 512 / in_f)
  off-grid / tie / out-of-range pack ......................... test_pack_grouped_off_grid
  3-bit perm dequant ......................................... test_dequant_packed_perm_exact
  fused-gather GEMM at M > 4, mat-vec workgroup sizes ........ test_variants_on_diagnostic_library
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import packed_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("row", R.GEMM_EXACT, ids=[R.case_id(r) for r in R.GEMM_EXACT])
def test_gemm_exact(G, hip_device, bits, row):
    K, N, gs, Ms, xd, perm = row
    c = R.dyadic_case(bits, K, N, gs, max(Ms), perm=perm, seed=1, x_dtype=xd)
    assert c.headroom_mv < 1.0
    R.run_gemm_exact(G, hip_device, c, Ms)


@pytest.mark.parametrize("bits", [3, 4])
def test_gemm_chunk_boundary_inside_group(G, hip_device, bits):
    """K = 1408 is 44 k-steps; the K split cuts them into chunks of 9, 11 or 15 steps, none a multiple of the 4 steps of
    a 128-group: a chunk closes a partial group at its end (`ks + 1 == kend`) and the next one starts inside it."""
    from gptq_amd import _lib
    K, N, gs = 1408, 1001, 128
    lib = _lib.load()
    Ms = (1, 3, 16, 17)
    for perm in (False, True):
        c = R.dyadic_case(bits, K, N, gs, max(Ms), perm=perm, seed=23, x_dtype="f16")
        for m in Ms:
            nbytes = lib.gptq_quant_gemm_workspace_bytes(m, K, N, bits, gs)
            assert nbytes > 0 and nbytes % (4 * m * N) == 0
            S = nbytes // (4 * m * N)
            chunk_steps = -(-(K // 32) // S)
            assert S > 1 and (chunk_steps * 32) % gs != 0, (m, S, chunk_steps)
        R.run_gemm_exact(G, hip_device, c, Ms, "chunk boundary")


@pytest.mark.parametrize("bits", [3, 4])
def test_gemm_misaligned_views(G, hip_device, bits):
    """N % 4 == 0 with a qweight that is only 4-byte aligned (the scalar packed-word path), x at a 2-byte offset and x
    with padded rows (16-byte rows: vector loads; 48-byte-off rows: element loads)."""
    K, N, gs = 1056, 1000, 32
    Ms = (1, 17, 129)
    c = R.dyadic_case(bits, K, N, gs, max(Ms), perm=False, seed=29, x_dtype="f16")
    qw, s, z, b, _ = R.dev_tensors(c, hip_device)
    ref = torch.from_numpy(c.ref).to(hip_device).float()
    flat = torch.zeros(qw.numel() + 4, dtype=torch.int32, device=hip_device)
    flat[1:1 + qw.numel()] = qw.reshape(-1)
    qw_off = flat[1:1 + qw.numel()].view(qw.shape)
    assert qw_off.is_contiguous() and qw_off.data_ptr() % 16 == 4
    for m in Ms:
        x = c.x[:m].to(hip_device)
        y = G.quant_matmul(x, qw_off, s, z, bits, gs, bias=b, out_dtype=torch.float32)
        R.assert_equal_bits(y, ref[:m], f"qweight at a 4-byte offset, M={m}")
        xf = torch.zeros(m * K + 8, dtype=x.dtype, device=hip_device)
        xf[1:1 + m * K] = x.reshape(-1)
        x_off = xf[1:1 + m * K].view(m, K)
        assert x_off.data_ptr() % 16 == 2
        y = G.quant_matmul(x_off, qw, s, z, bits, gs, bias=b, out_dtype=torch.float32)
        R.assert_equal_bits(y, ref[:m], f"x at a 2-byte offset, M={m}")
        y = G.quant_matmul(x_off, qw_off, s, z, bits, gs, bias=b)
        R.assert_equal_bits(y, ref[:m].half(), f"both misaligned, fp16 output, M={m}")
        for pad in (64, 24):
            big = sentinel((m, K + pad), x.dtype, hip_device)
            big[:, :K] = x
            xs = big[:, :K]
            assert xs.stride(0) == K + pad
            y = G.quant_matmul(xs, qw, s, z, bits, gs, bias=b, out_dtype=torch.float32)
            R.assert_equal_bits(y, ref[:m], f"x rows padded by {pad}, M={m}")
    # act-order on the same misaligned operands (gather pre-pass at M = 17, fused gather at M = 1)
    cp = R.dyadic_case(bits, K, N, gs, 17, perm=True, seed=31, x_dtype="bf16")
    qw, s, z, b, perm = R.dev_tensors(cp, hip_device)
    flat[1:1 + qw.numel()] = qw.reshape(-1)
    refp = torch.from_numpy(cp.ref).to(hip_device).float()
    for m in (1, 17):
        xf = torch.zeros(m * K + 8, dtype=torch.bfloat16, device=hip_device)
        xf[1:1 + m * K] = cp.x[:m].to(hip_device).reshape(-1)
        y = G.quant_matmul(xf[1:1 + m * K].view(m, K), qw_off, s, z, bits, gs, bias=b, out_dtype=torch.float32, perm=perm)
        R.assert_equal_bits(y, refp[:m], f"perm, misaligned x and qweight, M={m}")


# ================================================================================================ mat-vec, exact
@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("row", R.MATVEC_EXACT, ids=[R.case_id(r) for r in R.MATVEC_EXACT])
def test_matvec_exact(Q, hip_device, bits, row):
    """All entry points, fp32 and fp16 x, `mul` preloaded with the bias: every add is exact, so the order of the
    cross-workgroup atomics does not matter and the result is bit-equal."""
    K, N, gs = row
    for perm in ((False, True) if gs > 0 else (False,)):
        c = R.dyadic_case(bits, K, N, gs, 1, perm=perm, seed=2, x_dtype="f16")
        assert c.headroom_mv < 1.0
        for entry in R.matvec_entries(bits, gs):
            R.run_matvec_exact(Q, hip_device, c, entry)
            R.run_matvec_exact(Q, hip_device, c, entry, "second call")


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("gs", [-1, 128])
def test_matvec_misaligned_mat(Q, hip_device, bits, gs):
    """width % 4 == 0 but `mat` only 4-byte aligned: the one-column-per-thread kernel."""
    K, N = 1408, 1000
    for perm in ((False, True) if gs > 0 else (False,)):
        c = R.dyadic_case(bits, K, N, gs, 1, perm=perm, seed=37, x_dtype="f16")
        flat = torch.zeros(c.qweight.size + 4, dtype=torch.int32, device=hip_device)
        flat[1:1 + c.qweight.size] = torch.from_numpy(c.qweight).to(hip_device).reshape(-1)
        c.qweight_dev = flat[1:1 + c.qweight.size].view(c.qweight.shape)
        assert c.qweight_dev.data_ptr() % 16 == 4 and c.qweight_dev.is_contiguous()
        _, s, z, b, p = R.dev_tensors(c, hip_device)
        ref = torch.from_numpy(c.ref[0]).to(hip_device).float()
        for half in (False, True):
            x = c.x[0].to(hip_device).to(torch.float16 if half else torch.float32)
            mul = b.clone()
            if gs > 0:
                Q.vecquant_matmul_grouped(x, c.qweight_dev, mul, s, z, bits, gs, perm=p)
            elif bits == 4:
                Q.vecquant4matmul(x, c.qweight_dev, mul, s.reshape(-1, 1), z.reshape(-1, 1))
            elif half:
                Q.vecquant3matmul_faster(x, c.qweight_dev, mul, s.reshape(-1, 1), z.reshape(-1, 1))
            else:
                Q.vecquant3matmul(x, c.qweight_dev, mul, s.reshape(-1, 1), z.reshape(-1, 1))
            R.assert_equal_bits(mul, ref, f"misaligned mat, {bits}-bit g{gs} half={half} perm={perm}")


# ================================================================================================ modules, exact
@pytest.mark.parametrize("kind", ["Quant3Linear", "Quant3Linear-faster", "Quant4Linear", "QuantGroupLinear-3",
                                  "QuantGroupLinear-4", "QuantGroupLinear-3-act", "QuantGroupLinear-4-act"])
def test_modules_exact(G, hip_device, kind):
    """A 1-token forward equals row 0 of the multi-token forward bit for bit, and both equal the reference."""
    parts = kind.split("-")
    M = 5
    if parts[0] == "QuantGroupLinear":
        bits, act = int(parts[1]), parts[-1] == "act"
        K, N, gs = 1152, 130, 96
        c = R.dyadic_case(bits, K, N, gs, M, perm=act, seed=41, x_dtype="f16")
        m = G.QuantGroupLinear(bits, gs, K, N, multi_token=True, act_order=act)
    else:
        bits = 3 if parts[0] == "Quant3Linear" else 4
        K, N, gs = 416, 257, -1
        c = R.dyadic_case(bits, K, N, gs, M, seed=43, x_dtype="f16")
        m = getattr(G, parts[0])(K, N, faster=parts[-1] == "faster", multi_token=True)
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
def _half_even(v):
    return np.round(v)                                       # numpy rounds half to even, like torch.round and rintf


@pytest.mark.parametrize("perm", [False, True], ids=["plain", "perm"])
@pytest.mark.parametrize("wdtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("bits", [3, 4])
def test_pack_grouped_off_grid(G, hip_device, bits, wdtype, perm):
    """Off-grid weights s (q - z + d), d in {0, -0.49, 0.49}, exact ties d = -0.5 / 0.5 on a dyadic grid (representable in
    every weight type), and weights far outside the grid.  Reference: clamp(round((w + zeros) / scales), 0, maxq) in fp32
    torch on the same fp32 operands; ties go to the even code (torch.round, the reference project's pack, rintf)."""
    from gptq_amd.quant import pack_grouped
    K, N, gs = 1152, 130, 96
    maxq = 2 ** bits - 1
    rng = np.random.default_rng([bits, int(perm), 7])
    for dyadic in (True, False):
        G_ = K // gs
        sc = np.ldexp(1.0, -rng.integers(6, 9, (G_, N))) if dyadic else rng.uniform(1e-3, 2e-2, (G_, N))
        sc = sc.astype(np.float32)
        zint = rng.integers(0, maxq + 1, (G_, N)).astype(np.float64)
        zr = (zint * sc).astype(np.float32)
        q = rng.integers(0, maxq + 1, (K, N)).astype(np.float64)
        d = rng.choice(np.array([0.0, -0.49, 0.49, -0.5, 0.5] if dyadic else [0.0, -0.49, 0.49]), (K, N))
        far = rng.random((K, N)) < 0.05
        grp = np.arange(K) // gs
        wst = sc[grp].astype(np.float64) * (q - zint[grp] + d)                      # storage order [K, N]
        wst[far] = rng.choice(np.array([-10.0, 10.0, -0.9, 0.9]), int(far.sum()))
        p = rng.permutation(K).astype(np.int32) if perm else None
        w_orig = np.empty_like(wst)
        w_orig[p if perm else np.arange(K)] = wst                                   # storage row j = input column perm[j]
        w = torch.from_numpy(w_orig.T.copy()).to(wdtype)                            # [out, in], rounded to the weight type
        wf = w.float().t()[torch.from_numpy(p).long()] if perm else w.float().t()   # storage order again, fp32
        s_t, z_t = torch.from_numpy(sc), torch.from_numpy(zr)
        g_t = torch.from_numpy(grp)
        want = torch.clamp(torch.round((wf + z_t[g_t]) / s_t[g_t]), 0, maxq).numpy().astype(np.uint8)
        if dyadic and wdtype == torch.float32:
            near = ~far
            assert np.array_equal(want[near], np.clip(_half_even(q + d), 0, maxq)[near].astype(np.uint8))
            assert (np.abs(d[near]) == 0.5).sum() > 1000                            # the ties are really there
        qw = pack_grouped(w.to(hip_device), s_t.to(hip_device), z_t.to(hip_device), gs, bits,
                          None if p is None else torch.from_numpy(p).to(hip_device))
        got = R.unpack(qw.cpu().numpy(), bits)
        bad = got != want
        assert not bad.any(), (f"{int(bad.sum())} codes differ (dyadic={dyadic}); first {tuple(np.argwhere(bad)[0])}: "
                               f"got {got[bad][0]}, want {want[bad][0]}")
        assert np.array_equal(qw.cpu().numpy(), R.pack(want, bits))
        assert want.min() == 0 and want.max() == maxq


@pytest.mark.parametrize("gs", [32, 96, 1152])
@pytest.mark.parametrize("bits", [3, 4])
def test_dequant_packed_perm_exact(G, hip_device, bits, gs):
    """dequant_packed with and without perm == scale * (code - zero) in fp32, rounded once to the output type."""
    from gptq_amd.quant import dequant_packed
    K, N = 1152, 130
    rng = np.random.default_rng([bits, gs, 11])
    codes = rng.integers(0, 2 ** bits, (K, N), dtype=np.uint8)
    qw = torch.from_numpy(R.pack(codes, bits)).to(hip_device)
    sc = torch.from_numpy(rng.uniform(1e-3, 2e-2, (K // gs, N)).astype(np.float32))
    zint = torch.from_numpy(rng.integers(0, 2 ** bits, (K // gs, N)).astype(np.float32))
    grp = torch.arange(K) // gs
    dense = (sc[grp] * (torch.from_numpy(R.unpack(qw.cpu().numpy(), bits)).float() - zint[grp])).t().contiguous()  # [N, K]
    p = torch.from_numpy(rng.permutation(K).astype(np.int32))
    scattered = torch.empty_like(dense)
    scattered[:, p.long()] = dense                          # storage row j -> input column perm[j]
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        W = dequant_packed(qw, sc.to(hip_device), zint.to(hip_device), bits, gs, dtype=dt)
        R.assert_equal_bits(W.cpu(), dense.to(dt), f"dequant {bits}-bit g{gs} {dt}")
        W = dequant_packed(qw, sc.to(hip_device), zint.to(hip_device), bits, gs, dtype=dt, perm=p.to(hip_device))
        R.assert_equal_bits(W.cpu(), scattered.to(dt), f"dequant perm {bits}-bit g{gs} {dt}")


# ================================================================================================ canaries
@pytest.mark.parametrize("ydt", [torch.float32, torch.float16], ids=["y32", "y16"])
@pytest.mark.parametrize("perm", [False, True], ids=["plain", "perm"])
@pytest.mark.parametrize("K,gs", [(1408, 128), (96, 32)], ids=["splitK", "nosplit"])
@pytest.mark.parametrize("bits", [3, 4])
def test_gemm_canaries(hip_device, bits, K, gs, perm, ydt):
    """ldy = N + 5 through the C ABI: the body equals the reference, the 5 padding columns of every row and the 4096
    bytes after the reported workspace size keep their sentinel bits (the pre-pass's gathered X lives in the workspace)."""
    from gptq_amd import _lib
    lib = _lib.load()
    dev = hip_device
    split_seen = False
    for N in (3, 130, 257):
        Ms = (1, 17, 129)
        c = R.dyadic_case(bits, K, N, gs, max(Ms), perm=perm, seed=47, x_dtype="f16")
        qw, s, z, b, p = R.dev_tensors(c, dev)
        ref = torch.from_numpy(c.ref).to(dev).float().to(ydt)
        for m in Ms:
            x = c.x[:m].to(dev).contiguous()
            query = lib.gptq_quant_gemm_perm_workspace_bytes if perm else lib.gptq_quant_gemm_workspace_bytes
            nbytes = query(m, K, N, bits, gs)
            split_seen |= lib.gptq_quant_gemm_workspace_bytes(m, K, N, bits, gs) > 0
            ws = sentinel((nbytes + 4096,), torch.uint8, dev)
            y = sentinel((m, N + 5), ydt, dev)
            args = [_lib.ptr(x), _lib.dtype_code(x), K, m, _lib.ptr(qw), _lib.ptr(s), _lib.ptr(z)]
            if perm:
                args.append(_lib.ptr(p))
            args += [_lib.ptr(b), K, N, bits, gs, _lib.ptr(y), _lib.dtype_code(y), N + 5, _lib.ptr(ws), nbytes,
                     _lib.stream(dev)]
            with torch.cuda.device(dev):
                _lib.call("gptq_quant_gemm_perm" if perm else "gptq_quant_gemm", *args)
            torch.cuda.synchronize()
            R.assert_equal_bits(y[:, :N].contiguous(), ref[:m], f"ldy = N + 5, {bits}-bit K={K} N={N} M={m}")
            assert_untouched(y[:, N:], f"the padding columns of y (N={N}, M={m})")
            assert_untouched(ws[nbytes:], f"the bytes after the workspace (N={N}, M={m}, {nbytes} bytes)")
    assert split_seen == (K == 1408)                     # one parametrisation splits K, the other never does


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("width", [1, 130, 257, 1000])
def test_matvec_canaries(Q, hip_device, bits, width):
    """`mul` is a slice of a sentinel-filled buffer: its neighbours on both sides keep their bits."""
    K = 1408
    for gs in (-1, 128):
        for perm in ((False, True) if gs > 0 else (False,)):
            c = R.dyadic_case(bits, K, width, gs, 1, perm=perm, seed=53, x_dtype="f16")
            qw, s, z, b, p = R.dev_tensors(c, hip_device)
            ref = torch.from_numpy(c.ref[0]).to(hip_device).float()
            for entry in R.matvec_entries(bits, gs):
                buf = sentinel((256 + width + 256,), torch.float32, hip_device)
                mul = buf[256:256 + width]
                mul.copy_(b)
                half = entry in ("3faster", "4h", "groupedh")
                x = c.x[0].to(hip_device).to(torch.float16 if half else torch.float32)
                if gs > 0:
                    Q.vecquant_matmul_grouped(x, qw, mul, s, z, bits, gs, perm=p)
                elif bits == 4:
                    Q.vecquant4matmul(x, qw, mul, s.reshape(-1, 1), z.reshape(-1, 1))
                elif half:
                    Q.vecquant3matmul_faster(x, qw, mul, s.reshape(-1, 1), z.reshape(-1, 1))
                else:
                    Q.vecquant3matmul(x, qw, mul, s.reshape(-1, 1), z.reshape(-1, 1))
                torch.cuda.synchronize()
                R.assert_equal_bits(mul.clone(), ref, f"mat-vec into a slice, {entry} width {width}")
                assert_untouched(buf[:256], f"the 256 floats before mul ({entry}, width {width})")
                assert_untouched(buf[256 + width:], f"the 256 floats after mul ({entry}, width {width})")


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("n_out", [1, 130, 257])
def test_pack_canaries(hip_device, bits, n_out):
    """gptq_pack_codes (both kernels: 16-byte-aligned code rows and not) and gptq_pack_grouped write exactly the
    [in/32*bits, out] words: a sentinel row before and after them keeps its bits."""
    from gptq_amd import _lib
    dev = hip_device
    K, gs = 416, 32
    rows = K // 32 * bits
    rng = np.random.default_rng([bits, n_out])
    codes = rng.integers(0, 2 ** bits, (K, n_out), dtype=np.uint8)
    want = torch.from_numpy(R.pack(codes, bits)).to(dev)
    for ld in (K, K + 3):                                    # K + 3: rows not 16-byte aligned -> the narrow kernel
        cbuf = torch.zeros((n_out, ld), dtype=torch.uint8, device=dev)
        cbuf[:, :K] = torch.from_numpy(codes.T.copy()).to(dev)
        buf = sentinel((rows + 2, n_out), torch.int32, dev)
        with torch.cuda.device(dev):
            _lib.call("gptq_pack_codes", _lib.ptr(cbuf), ld, n_out, K, bits, _lib.ptr(buf[1:]), _lib.stream(dev))
        torch.cuda.synchronize()
        assert torch.equal(buf[1:rows + 1], want), f"pack_codes ld={ld}"
        assert_untouched(buf[:1], "the row before qweight (pack_codes)")
        assert_untouched(buf[rows + 1:], "the row after qweight (pack_codes)")
    for perm in (False, True):
        c = R.dyadic_case(bits, K, n_out, gs, 1, perm=perm, seed=59)
        grp = np.arange(K) // gs
        wst = c.scales[grp].astype(np.float64) * c.codes - c.zeros[grp]            # on the grid, storage order
        w = np.empty_like(wst)
        w[c.perm if perm else np.arange(K)] = wst
        wt = torch.from_numpy(w.T.copy()).float().to(dev).contiguous()
        _, s, z, _, p = R.dev_tensors(c, dev)
        buf = sentinel((rows + 2, n_out), torch.int32, dev)
        with torch.cuda.device(dev):
            _lib.call("gptq_pack_grouped", _lib.ptr(wt), _lib.dtype_code(wt), K, n_out, K, _lib.ptr(s), _lib.ptr(z), gs,
                      _lib.ptr(p), bits, _lib.ptr(buf[1:]), _lib.stream(dev))
        torch.cuda.synchronize()
        assert torch.equal(buf[1:rows + 1], torch.from_numpy(c.qweight).to(dev)), f"pack_grouped perm={perm}"
        assert_untouched(buf[:1], "the row before qweight (pack_grouped)")
        assert_untouched(buf[rows + 1:], "the row after qweight (pack_grouped)")


# ================================================================================================ row isolation
@pytest.mark.parametrize("perm", [False, True], ids=["plain", "perm"])
@pytest.mark.parametrize("bits", [3, 4])
def test_gemm_row_isolation(G, hip_device, bits, perm):
    """One NaN / +inf in row r of x: every other row keeps its bits, every element of row r is non-finite."""
    K, N, gs = 1152, 130, 96
    c = R.dyadic_case(bits, K, N, gs, 129, perm=perm, seed=61, x_dtype="f16")
    qw, s, z, b, p = R.dev_tensors(c, hip_device)
    for M in (5, 33, 129):
        x = c.x[:M].to(hip_device)
        base = G.quant_matmul(x, qw, s, z, bits, gs, bias=b, out_dtype=torch.float32, perm=p)
        R.assert_equal_bits(base, torch.from_numpy(c.ref[:M]).to(hip_device).float(), f"row isolation base M={M}")
        for r in (0, M - 1):                              # first and last row tile
            for bad in (float("nan"), float("inf")):
                xb = x.clone()
                xb[r, (7 * r + 401) % K] = bad
                y = G.quant_matmul(xb, qw, s, z, bits, gs, bias=b, out_dtype=torch.float32, perm=p)
                keep = torch.arange(M, device=hip_device) != r
                R.assert_equal_bits(y[keep], base[keep], f"rows other than {r} (M={M}, {bad})")
                assert not bool(torch.isfinite(y[r]).any()), f"finite outputs in the poisoned row {r} (M={M}, {bad})"


# ================================================================================================ diagnostic library
@pytest.mark.parametrize("sweep,env", [("gemm-perm", {"GPTQ_QG_PERM_FUSED_M": "100000"}),
                                       ("matvec", {"GPTQ_MV_KGROUPS": "1"}),
                                       ("matvec", {"GPTQ_MV_KGROUPS": "3"}),
                                       ("matvec", {"GPTQ_MV_KGROUPS": "128"})],
                         ids=["fused-perm-gemm", "mv-kg1", "mv-kg3", "mv-kg128"])
def test_variants_on_diagnostic_library(hip_device, sweep, env):
    """Kernels the product's fixed knobs never select -- the fused-gather GEMM at M = 17 ... 129 (MSUB 2 / 4, WM 2) and
    the mat-vec at other workgroup sizes -- run the exact sweep in a child process on the diagnostic library, which reads
    the knobs from the environment once per process."""
    diag = os.path.join(ROOT, "gptq_amd", "libgptq_hip_diag.so")
    if not os.path.exists(diag):
        pytest.skip("diagnostic library not built (python -m gptq_amd.build --diag)")
    e = dict(os.environ, GPTQ_HIP_LIB=diag, **env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "packed_ref.py"), "--exact-sweep", sweep], env=e,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert f"exact sweep {sweep}:" in r.stdout and "bit-equal" in r.stdout


# ================================================================================================ float bars
BARS = {}
U_OUT = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
# half the spacing of the output type's subnormals: the absolute term of the standard rounding model, which only the
# `subnormal` kind's fp16 outputs (around 1e-6) ever reach
ETA_OUT = {torch.float32: 0.0, torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}
FLOAT_K, FLOAT_N = 4096, 520
FLOAT_GRIDS = {"row": -1, "g32": 32, "g128": 128}


def _coef(n_chain):
    return min(1.1 * n_chain * 2.0 ** -24, 5e-5)


def _ratio(y, ref, T, coef, dtype):
    err = (y.double().cpu().numpy() - ref)
    bar = coef * T + U_OUT[dtype] * np.abs(ref) + ETA_OUT[dtype]
    return float((np.abs(err) / bar).max()) if np.isfinite(err).all() else float("inf")


def _record(kernel, kind, ratio):
    BARS.setdefault(kernel, {})
    BARS[kernel][kind] = max(BARS[kernel].get(kind, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _write_bars():
    yield
    if not BARS:
        return
    for kernel in sorted(BARS):
        print(f"\nworst err / bar, {kernel}: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(BARS[kernel].items())))
    out = os.environ.get("GPTQ_TEST_RECORD_DIR")          # where to keep the record (profiles/packed_forward_bars.json)
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "packed_forward_bars.json"), "w") as f:
            json.dump({"bar": "|y - ref| <= min(1.1 n_chain 2^-24, 5e-5) T + u_out |ref|", "K": FLOAT_K, "N": FLOAT_N,
                       "worst_err_over_bar": BARS}, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.mark.parametrize("grid", list(FLOAT_GRIDS))
@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("kind", R.REALISTIC_KINDS)
def test_realistic_activations_within_contract_bar(G, Q, hip_device, kind, bits, grid):
    """|y - ref| <= c T + u_out |ref| per element, c = min(1.1 n_chain 2^-24, 5e-5): n_chain is the longest fp32 add chain
    (GEMM: group (or K) + number of groups + S + 2; mat-vec: K + number of groups + 8), T the contract magnitude
    sum (s q + z)|x| + |bias| (mat-vec: q + 32), the only magnitude the error of s sum(q x) - z sum(x) is proportional to
    when x has one sign.  1.1 n 2^-24 is the first-order worst case of recursive fp32 summation in any order; 5e-5 is the
    coefficient of the older GEMM tests and caps the long per-row chains.  The `subnormal` kind also shows that fp16
    subnormals are not flushed, neither in the MFMA operand nor in the fp32 sum of x: a flush in one of them breaks the
    cancellation of s acc - z sx and misses the bar by orders of magnitude."""
    from gptq_amd import _lib
    lib = _lib.load()
    K, N, gs = FLOAT_K, FLOAT_N, FLOAT_GRIDS[grid]
    ngroups = K // gs if gs > 0 else 1
    dev = hip_device
    worst = {}
    # ---- mat-vec, fp32 and fp16 x
    for xd in ("f32", "f16"):
        c = R.realistic_case(kind, bits, K, N, gs, 1, seed=5, x_dtype=xd)
        qw, s, z, b, _ = R.dev_tensors(c, dev)
        mul = b.clone()
        x = c.x[0].to(dev)
        if gs > 0:
            Q.vecquant_matmul_grouped(x, qw, mul, s, z, bits, gs)
        elif bits == 4:
            Q.vecquant4matmul(x, qw, mul, s.reshape(-1, 1), z.reshape(-1, 1))
        elif xd == "f16":
            Q.vecquant3matmul_faster(x, qw, mul, s.reshape(-1, 1), z.reshape(-1, 1))
        else:
            Q.vecquant3matmul(x, qw, mul, s.reshape(-1, 1), z.reshape(-1, 1))
        worst[f"matvec-{xd}"] = _ratio(mul, c.ref[0], c.T_mv[0], _coef(K + ngroups + 8), torch.float32)
    # ---- GEMM, fp16 and bf16 x, fp32 and rounded outputs
    for xd in ("f16", "bf16"):
        c = R.realistic_case(kind, bits, K, N, gs, 129, seed=6, x_dtype=xd)
        qw, s, z, b, _ = R.dev_tensors(c, dev)
        dt = R.torch_dtype(xd)
        for m in (1, 7, 129):
            nbytes = lib.gptq_quant_gemm_workspace_bytes(m, K, N, bits, gs)
            S = nbytes // (4 * m * N) if nbytes else 1
            coef = _coef((gs if gs > 0 else K) + ngroups + S + 2)
            x = c.x[:m].to(dev)
            y32 = G.quant_matmul(x, qw, s, z, bits, gs, bias=b, out_dtype=torch.float32)
            yo = G.quant_matmul(x, qw, s, z, bits, gs, bias=b)
            R.assert_equal_bits(yo, y32.to(dt), f"rounded output is one rounding of the fp32 value ({xd}, M={m})")
            worst[f"gemm-{xd}"] = max(worst.get(f"gemm-{xd}", 0.0), _ratio(y32, c.ref[:m], c.T[:m], coef, torch.float32))
            # (close to 1 by nature: the output rounding alone uses up to u_out |ref| of the bar)
            worst[f"gemm-{xd}-rounded"] = max(worst.get(f"gemm-{xd}-rounded", 0.0),
                                              _ratio(yo, c.ref[:m], c.T[:m], coef, dt))
    for k, v in worst.items():
        _record(f"{k}-{bits}bit-{grid}", kind, v)
    print(f"{kind} {bits}-bit {grid}: worst err / bar " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
