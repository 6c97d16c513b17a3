"""The int8-activation packed GEMM without a GPU: the exact-case table of packed_a8_ref really is exact (so the GPU test
may demand equality), the C ABI is declared, exported and bound, nothing falls back to the CPU, `act_bits` is opt-in and
no state, and every kernel of csrc/qgemm_a8.hip compiles for gfx950 without scratch."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import packed_a8_ref as A8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
NEW = ("gptq_quant_act_rows", "gptq_quant_gemm_a8", "gptq_quant_gemm_a8_workspace_bytes")


@pytest.mark.parametrize("bits", A8.BITS)
@pytest.mark.parametrize("row", A8.GEMM_EXACT, ids=A8.case_id)
def test_exact_table_is_exact(row, bits):
    """Every entry stays under the 2^24-lsb bound, its integers convert exactly, and an fp32 evaluation of the contract in
    two different group orders equals the fp64 reference bit for bit."""
    K, N, gs, Ms, _, _, _, j = row
    c = A8.dyadic_case(bits, K, N, gs, max(Ms), j=j, perm=False, seed=3)
    assert c.headroom < 1.0
    I, X = A8.group_sums(c.unpacked, c.xq, gs)
    assert np.abs(I).max() < 2 ** 24 and np.abs(X).max() < 2 ** 24
    assert np.abs(c.xq).max() == 127 and (np.abs(c.xq).max(axis=1) == 127).all()
    want = c.ref.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), c.ref)               # the reference itself is an fp32 number
    for order in ("forward", "reverse", "shuffled"):
        assert np.array_equal(A8.emulate_fp32(c, order, seed=5), want), order


def test_table_covers_every_axis_and_plan():
    rows = A8.GEMM_EXACT
    assert {A8.grid_kind(r[0], r[2]) for r in rows} == {"row", "g32", "g64", "g96", "g128", "gK"}
    assert {32, 96, 160, 1056} <= {r[0] for r in rows}
    assert {m for r in rows for m in r[3]} == {1, 15, 16, 17, 33, 65, 129}
    assert {r[1] for r in rows} == {1, 7, 64, 257, 520}
    assert {r[4] for r in rows} == {A8.F32, A8.F16, A8.BF16}
    assert {r[5] for r in rows} == {True, False} and {r[6] for r in rows} == {"x", "pair"}
    for kind in ("row", "g32", "g96", "gK"):                            # a K % 64 == 32 tail with ragged M and N tiles
        assert any(A8.grid_kind(r[0], r[2]) == kind and r[0] % 64 == 32 and r[1] % 64 and any(m % 16 for m in r[3])
                   for r in rows), kind
    for kind in ("g64", "g128"):                                        # (K % 64 == 0 there): a ragged last xq tile
        assert any(A8.grid_kind(r[0], r[2]) == kind and r[0] % 256 and r[1] % 64 and any(m % 16 for m in r[3])
                   for r in rows), kind
    # the K-split plans: no split, int32 partials (per-row grids), fp32 partials (grouped grids)
    from gptq_amd import _lib
    from gptq_amd.build import build_library
    build_library(verbose=False)
    q = _lib.load().gptq_quant_gemm_a8_workspace_bytes
    plans = set()
    for K, N, gs, Ms, *_ in rows:
        for m in Ms:
            for bits in A8.BITS:
                plans.add(("none" if q(m, K, N, bits, gs) == 0 else "int" if gs <= 0 else "fp32"))
    assert plans == {"none", "int", "fp32"}


def test_quantize_ref_rounds_half_even_and_handles_zero_rows():
    import torch
    x = torch.zeros(3, 32, dtype=torch.float16)
    x[1, 0], x[1, 1:6] = 127.0, torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5])   # sx = 1: ties
    x[2, 3] = 65504.0
    xq, sx = A8.quantize_ref(x)
    assert sx[0] == 1.0 and not xq[0].any()
    assert sx[1] == 1.0 and xq[1, :6].tolist() == [127, 0, 2, 2, 0, -2]
    assert xq[2, 3] == 127 and sx[2] == np.float32(65504.0) / np.float32(127.0)


def _header():
    text = open(os.path.join(ROOT, "include", "gptq_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_export_and_binding_agree():
    from gptq_amd import _lib
    from gptq_amd.build import build_library
    build_library(verbose=False)
    text = _header()
    assert re.search(r"\bint\s+gptq_quant_act_rows\s*\(", text)
    assert re.search(r"\bint\s+gptq_quant_gemm_a8\s*\(", text)
    assert re.search(r"\bsize_t\s+gptq_quant_gemm_a8_workspace_bytes\s*\(", text)
    lib = _lib.load()
    for n in NEW:
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert lib.gptq_hip_abi_version() == 2
    q = lib.gptq_quant_gemm_a8_workspace_bytes                          # a pure function of the shape: no device
    assert q(2048, 4096, 11008, 4, 128) == 0
    assert q(2, 4096, 4096, 4, -1) > 0 and q(2, 4096, 4096, 4, 128) % (2 * 4096 * 4) == 0
    assert q(2, 4096, 4096, 4, 128) == q(2, 4096, 4096, 4, 128)
    assert q(2, 4096, 4096, 5, -1) == 0 and q(2, 65568, 64, 8, -1) == 0 and q(2, 4096, 64, 4, 48) == 0


def test_without_gpu_is_a_loud_failure():
    import torch
    import gptq_amd
    from gptq_amd import _lib
    x = torch.zeros(3, 64, dtype=torch.float16)
    qw = torch.zeros(64 // 32 * 4, 16, dtype=torch.int32)
    s, z = torch.ones(16), torch.zeros(16)
    with pytest.raises(ValueError):                       # fp16 / bf16 activations only
        gptq_amd.quant_matmul_a8(x.float(), qw, s, z, 4)
    with pytest.raises(ValueError):
        gptq_amd.quantize_activations(x.float())
    with pytest.raises(ValueError):                       # K % 32
        gptq_amd.quantize_activations(torch.zeros(3, 48, dtype=torch.float16))
    with pytest.raises(ValueError):                       # qweight of another K
        gptq_amd.quant_matmul_a8(torch.zeros(3, 96, dtype=torch.float16), qw, s, z, 4)
    with pytest.raises(ValueError):                       # mismatched pair
        gptq_amd.quant_matmul_a8((torch.zeros(3, 64, dtype=torch.int8), torch.ones(2)), qw, s, z, 4)
    with pytest.raises(ValueError):                       # perm needs grouped grids
        gptq_amd.quant_matmul_a8(x, qw, s, z, 4, perm=torch.arange(64, dtype=torch.int32))
    with pytest.raises(ValueError):                       # inference only
        gptq_amd.quant_matmul_a8(x.clone().requires_grad_(), qw, s, z, 4)
    with pytest.raises(ValueError):
        gptq_amd.quant_matmul_a8(x, qw, s.clone().requires_grad_(), z, 4)
    big = torch.zeros(1, 65568, dtype=torch.float16)
    with pytest.raises(ValueError):                       # K > 65536
        gptq_amd.quant_matmul_a8(big, torch.zeros(65568 // 32 * 8, 4, dtype=torch.int32), torch.ones(4), torch.zeros(4), 8)
    if torch.cuda.is_available():
        return
    with pytest.raises(_lib.GptqHipError):
        gptq_amd.quantize_activations(x)
    with pytest.raises(_lib.GptqHipError):
        gptq_amd.quant_matmul_a8(x, qw, s, z, 4)
    with pytest.raises(_lib.GptqHipError):
        gptq_amd.quant_matmul_a8((torch.zeros(3, 64, dtype=torch.int8), torch.ones(3)), qw, s, z, 4)


def test_act_bits_is_opt_in_and_not_state():
    import torch
    import gptq_amd
    m = gptq_amd.Quant4Linear(64, 16, multi_token=True)
    g = gptq_amd.QuantGroupLinear(4, 32, 64, 16, multi_token=True, act_order=True)
    assert m.act_bits is None and g.act_bits is None
    model = torch.nn.Sequential(gptq_amd.Quant3Linear(64, 16), gptq_amd.Quant2Linear(64, 16), gptq_amd.Quant8Linear(64, 16),
                                g, m, torch.nn.Linear(16, 16))
    keys = sorted(model.state_dict())
    assert gptq_amd.set_act_bits(model, 8) == 5
    assert all(mod.act_bits == 8 for mod in list(model)[:5]) and not hasattr(model[5], "act_bits")
    assert sorted(model.state_dict()) == keys
    assert gptq_amd.set_act_bits(model, None) == 5 and m.act_bits is None and g.act_bits is None
    with pytest.raises(ValueError):
        gptq_amd.set_act_bits(model, 4)


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_a8_kernels_use_no_scratch(tmp_path):
    from gptq_amd import build
    src = os.path.join(ROOT, "gptq_amd", "csrc", "qgemm_a8.hip")
    assert "qgemm_a8.hip" in build.SOURCES
    r = subprocess.run([HIPCC] + build.FLAGS + build.PER_FILE_FLAGS.get("qgemm_a8.hip", [])
                       + ["-c", src, "-o", str(tmp_path / "qgemm_a8.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            usage[name] = int(m.group(1))
    assert sum("qgemm_a8_kernel" in k for k in usage) == 16 and sum("act_quant_kernel" in k for k in usage) == 4, sorted(usage)
    assert len(usage) >= 22
    assert all(v == 0 for v in usage.values()), {k: v for k, v in usage.items() if v}
