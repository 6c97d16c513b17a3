"""The packed dequant GEMM (gptq_quant_gemm) without a GPU: declared, bound and exported; no CPU fallback; and every
GEMM kernel of csrc/qgemm.hip compiles for gfx950 without scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def test_header_declares_the_gemm():
    text = open(os.path.join(ROOT, "include", "gptq_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+gptq_quant_gemm\s*\(", text)
    assert re.search(r"\bsize_t\s+gptq_quant_gemm_workspace_bytes\s*\(", text)


def test_gemm_is_bound_and_exported():
    from gptq_amd import _lib
    from gptq_amd.build import build_library
    build_library(verbose=False)
    assert "gptq_quant_gemm" in _lib.EXPORTS and "gptq_quant_gemm_workspace_bytes" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "gptq_quant_gemm")
    # the workspace query is a pure function of the shape: no device needed
    assert lib.gptq_quant_gemm_workspace_bytes(2048, 4096, 11008, 4, 128) == 0          # enough tiles: no split
    small = lib.gptq_quant_gemm_workspace_bytes(2, 4096, 4096, 4, -1)
    assert small > 0 and small % (2 * 4096 * 4) == 0                                    # S chunks of M x N fp32
    assert lib.gptq_quant_gemm_workspace_bytes(2, 4096, 4096, 5, -1) == 0               # invalid shapes: 0


def test_quant_matmul_without_gpu_is_a_loud_failure():
    import torch
    import gptq_amd
    from gptq_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x = torch.zeros(3, 64, dtype=torch.float16)
    qw = torch.zeros(64 // 32 * 4, 16, dtype=torch.int32)
    s, z = torch.ones(16), torch.zeros(16)
    with pytest.raises(_lib.GptqHipError):
        gptq_amd.quant_matmul(x, qw, s, z, 4)
    with pytest.raises(ValueError):                       # fp16 / bf16 activations only
        gptq_amd.quant_matmul(x.float(), qw, s, z, 4)
    with pytest.raises(ValueError):
        gptq_amd.quant_matmul(x, qw, s, z, 2)
    with pytest.raises(ValueError):                       # qweight of another K
        gptq_amd.quant_matmul(torch.zeros(3, 96, dtype=torch.float16), qw, s, z, 4)


def test_multi_token_flag_is_opt_in_and_not_state():
    import torch
    import gptq_amd
    m = gptq_amd.Quant4Linear(64, 16)
    assert m.multi_token is False
    keys = sorted(m.state_dict())
    with pytest.raises(ValueError):
        m(torch.zeros(2, 64, dtype=torch.float16))       # the reference's guard stays the default
    model = torch.nn.Sequential(gptq_amd.Quant3Linear(64, 16), gptq_amd.QuantGroupLinear(4, 32, 64, 16), m)
    assert gptq_amd.set_multi_token(model) == 3
    assert all(mod.multi_token for mod in model)
    assert sorted(m.state_dict()) == keys


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_gemm_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "gptq_amd", "csrc", "qgemm.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-c", src,
                        "-o", str(tmp_path / "qgemm.o"), "-Rpass-analysis=kernel-resource-usage"],
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
    gemm = {k: v for k, v in usage.items() if "qgemm" in k}
    assert len(gemm) >= 48, sorted(usage)
    assert all(v == 0 for v in gemm.values()), {k: v for k, v in gemm.items() if v}
