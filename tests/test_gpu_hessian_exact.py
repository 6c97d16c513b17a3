"""The Hessian kernels (csrc/hessian.hip) through the C ABI against tests/hessian_ref.py, bit for bit.

The inputs make X^T X exact in fp32 in any order and under any K split (hessian_ref's docstring; test_hessian_ref_cpu.py
proves it for every table row), so every kernel path must produce exactly `expected`: every assertion compares the 32-bit
patterns of the WHOLE H buffer -- upper triangle against the reference; strict lower triangle, pad columns (ldh > C) and
one guard row on each side against what was there before.  X slabs sit in allocations whose pad channels (ldx > C) and
guard rows hold NaN.  No tolerance anywhere in this file.

Where each path is covered:
  hessian_kernel<float>, vector and element loads ............. test_ragged_and_scalar_paths[f32-*]
  hessian16_kernel, vector and element loads, ragged C/tokens .. test_ragged_and_scalar_paths[f16-* / bf16-*],
                                                                test_aligned_128_path[C384-t96-*]
  hessian16_dma_kernel, > 16 slabs, > 8 problems ............... test_aligned_128_path
  hessian16_big16_kernel + fixup: no split, equal runs, odd chunk rounded up, heads + tails over 2 and 3 tiles,
    > 8 problems, 17 slabs, bf16, widths sharing launches ..... test_big_256_path
  launches by rounds at the device's CU count ................. test_big_256_path[device], [widths-nx17]
  eligible + refused problems in one call, `rest` regrouping .. test_mixed_call_with_refused_problems
  the same under GPTQ_HESS_BIG = 0 / 2 / 3, a CU budget, the 32x32x16 twin .. test_kernel_variants_in_child_process
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hessian_ref as R
from conftest import record_parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = {}                                                  # 256 x 256 case -> plan labels at the device's CU count


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from gptq_amd import _lib
    _lib.load()
    yield
    if LABELS:
        record_parity("hessian_exact_big_plans", **LABELS)
        for k in sorted(LABELS):
            print(f"\n256x256 plan, {k}: " + " | ".join(LABELS[k]))


def _device_cus(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


# ================================================================================================ ragged / scalar
@pytest.mark.parametrize("row", R.RAGGED, ids=[R.ragged_id(r) for r in R.RAGGED])
@pytest.mark.parametrize("dtype", R.X_DTYPES)
def test_ragged_and_scalar_paths(hip_device, dtype, row):
    c = R.upload(R.ragged_case(row, dtype), hip_device)
    path = R.kernel_path(c.Cs[0], c.tokens, c.ldx[0], c.offset[0], dtype)
    R.call_group(c, hip_device)
    want = R.assert_case_exact(c, f"{dtype} {R.ragged_id(row)} ({path})")
    R.reset_h(c, hip_device)
    R.call_mixed(c, hip_device)                              # the mixed entry sends it down the same path
    R.assert_case_exact(c, f"{dtype} {R.ragged_id(row)} ({path}) via _mixed", want)


# ================================================================================================ 128 x 128 DMA path
@pytest.mark.parametrize("row", R.ALIGNED, ids=[R.aligned_id(r) for r in R.ALIGNED])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_aligned_128_path(hip_device, dtype, row):
    """hessian16_dma_kernel: slabs in chunks of 16 (alpha = 1 after the first), problems in chunks of 8, a different
    nsamples_before per problem, ldx > C and ldh > C.  The tokens = 96 row is the shape of the row before it and must
    fall to the ragged kernel."""
    c = R.upload(R.aligned_case(row, dtype), hip_device)
    R.call_group(c, hip_device)
    R.assert_case_exact(c, f"{dtype} {R.aligned_id(row)}")


# ================================================================================================ 256 x 256 path
@pytest.mark.parametrize("name", list(R.BIG))
def test_big_256_path(hip_device, name):
    """gptq_hessian_accum_mixed with >= 100 eligible tiles in the default environment; n_cu steers the plan (the branch
    each row reaches at its budget is checked on the CPU, tests/test_hessian_ref_cpu.py::test_plan_coverage)."""
    widths, tokens, n_x, dtype, n_cu, family, branch = R.BIG[name]
    cus = _device_cus(hip_device)
    eff = cus if n_cu == 0 else max(8, min(cus, n_cu))
    LABELS[name] = [p.label for p in R.big_plans(widths, tokens, n_x, eff)]
    c = R.upload(R.big_case(name), hip_device)
    R.call_mixed(c, hip_device, n_cu)
    R.assert_case_exact(c, f"{name}: " + " | ".join(LABELS[name]))


def test_mixed_call_with_refused_problems(hip_device):
    """Seven eligible problems (105 tiles) in one call with three of C = 320 and one whose slabs are misaligned: the
    eligible ones share the 256 x 256 launches, the others are regrouped by (C, ldx, ldh).  With and without a budget."""
    for n_cu in (0, 29):
        c = R.upload(R.mixed_rest_case(), hip_device)
        R.call_mixed(c, hip_device, n_cu)
        R.assert_case_exact(c, f"eligible + refused problems, n_cu={n_cu}")


def test_split_round_is_deterministic_and_equals_the_group_entry(hip_device):
    """The heads + tails case twice: identical bits; and the same data through gptq_hessian_accum_group (no budget:
    another plan) gives the same bits again."""
    c = R.upload(R.big_case("heads2-cu29"), hip_device)
    R.call_mixed(c, hip_device, 29)
    want = R.assert_case_exact(c, "heads + tails, first call")
    first = [b.clone() for b in c.dHbuf]
    R.reset_h(c, hip_device)
    R.call_mixed(c, hip_device, 29)
    for a, b in zip(first, c.dHbuf):
        assert R.bits_equal(a, b), "the same split-round call twice gave different bits"
    # the group entry wants one (C, ldx, ldh): the same X values in a uniform layout
    u = R.exact_case(c.Cs, c.tokens, c.n_x, c.n_prob, c.dtype, nsamples_before=c.nb, batch_total=c.batch, seed=3,
                     ldx_pad=8, ldh_pad=5)
    for p in range(c.n_prob):
        for i in range(c.n_x):
            assert np.array_equal(u.Xs[p][i], c.Xs[p][i])
        assert np.array_equal(u.H0[p], c.H0[p])
    R.upload(u, hip_device)
    R.call_group(u, hip_device)
    R.assert_case_exact(u, "the same data through gptq_hessian_accum_group")
    for p in range(c.n_prob):
        C = c.Cs[p]
        assert R.bits_equal(u.dH[p][:, :C].contiguous(), first[p][1:C + 1, :C].contiguous())
        assert np.array_equal(want[p][:, :C].view(np.int32), u.dH[p][:, :C].cpu().numpy().view(np.int32))


# ================================================================================================ refused inputs
def test_invalid_arguments_are_refused(hip_device):
    from gptq_amd import _lib
    c = R.upload(R.exact_case(64, 16, 1, 1, "f16", **R.SINGLE), hip_device)
    before = [b.clone() for b in c.dHbuf]
    for field, value in (("ldh", [63]), ("ldx", [63]), ("Cs", [0]), ("tokens", 0), ("batch", 0), ("nb", [-1])):
        old = getattr(c, field)
        setattr(c, field, value)
        try:
            with pytest.raises(_lib.GptqHipError, match="invalid argument"):
                R.call_mixed(c, hip_device)
            with pytest.raises(_lib.GptqHipError, match="invalid argument"):
                R.call_group(c, hip_device)
        finally:
            setattr(c, field, old)
    with pytest.raises(_lib.GptqHipError, match="invalid argument"):
        R.call_mixed(c, hip_device, n_cu=-1)
    assert all(R.bits_equal(a, b) for a, b in zip(before, c.dHbuf))


# ================================================================================================ child processes
VARIANTS = [("big0", {"GPTQ_HESS_BIG": "0"}, [], False),
            ("big2", {"GPTQ_HESS_BIG": "2"}, [], False),
            ("big3", {"GPTQ_HESS_BIG": "3"}, [], False),
            ("big2-cu24", {"GPTQ_HESS_BIG": "2"}, ["--n-cu", "24"], False),
            ("big2-shape32", {"GPTQ_HESS_BIG": "2", "GPTQ_HESS_SHAPE": "32"}, [], True)]
_child_failed = []


@pytest.mark.parametrize("name,env,args,diag", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_kernel_variants_in_child_process(hip_device, name, env, args, diag):
    """The library reads its kernel-selection knobs once per process: the exact sweep of hessian_ref.py in a child per
    setting, one after the other, each under its own time limit.  After a child that failed or timed out no further
    child is started."""
    if _child_failed:
        pytest.fail(f"not started: the child '{_child_failed[0]}' failed before")
    e = dict(os.environ, **env)
    if diag:                                                 # the 32x32x16 twin lives in the diagnostic library only
        lib = os.path.join(ROOT, "gptq_amd", "libgptq_hip_diag.so")
        if not os.path.exists(lib):
            pytest.skip("diagnostic library not built (python -m gptq_amd.build --diag)")
        e["GPTQ_HIP_LIB"] = lib
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "hessian_ref.py"), "--exact-sweep"]
    try:
        r = subprocess.run(cmd + args, env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _child_failed.append(name)
        raise
    if r.returncode != 0:
        _child_failed.append(name)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("exact: ")]
    assert len(lines) == len(R._sweep_cases()) and all(l.endswith(" OK") for l in lines), r.stdout[-4000:]


# ================================================================================================ gptq_symmetrize
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 130, 1000])
def test_symmetrize(hip_device, n, pad):
    """Lower triangle = upper transposed; upper triangle, diagonal, pad columns and the guard rows keep their bits."""
    from gptq_amd import _lib
    lda = n + pad
    rng = np.random.default_rng([n, pad])
    A = rng.standard_normal((n, n)).astype(np.float32)
    A[rng.random((n, n)) < 0.02] = -0.0
    full = np.full((n + 2, lda), R.SENT32, dtype=np.uint32).view(np.float32)
    full[1:n + 1, :n] = A
    want = full.copy()
    low = np.tril(np.ones((n, n), dtype=bool), -1)
    want[1:n + 1, :n][low] = A.T[low]
    buf = torch.from_numpy(full).to(hip_device)
    with torch.cuda.device(hip_device):
        _lib.call("gptq_symmetrize", buf[1:].data_ptr(), lda, n, _lib.stream(hip_device))
    torch.cuda.synchronize()
    assert R.bits_equal(buf.cpu(), torch.from_numpy(want)), f"gptq_symmetrize n={n} lda={lda}"
    with pytest.raises(_lib.GptqHipError, match="invalid argument"):
        _lib.call("gptq_symmetrize", buf[1:].data_ptr(), n - 1, n, _lib.stream(hip_device))


# ================================================================================================ Python layer
def test_add_batch_is_exact_per_recorded_flush(hip_device):
    """GPTQ.add_batch with 2-D and 3-D exact inputs at HESSIAN_DEFER = 1, flushing per call (STAGE_INPUTS = 1) and with
    the default staging.  The grouping is read from FLUSH_EVENTS; `expected` applied once per recorded flush must give
    gp.H bit for bit on the upper triangle, and gp.H must be symmetric."""
    import gptq_amd
    gm = gptq_amd.gptq
    C = 256
    a = R.exact_case(C, 128, 3, 1, "f16", seed=21, **R.family_args("single", 1, 3))
    b = R.exact_case(C, 192, 2, 1, "f16", seed=22, **R.family_args("single", 1, 2))
    # (input tensor, its [tokens, C] slab): three 2-D inputs [128, C], then two 3-D inputs [2, 96, C]
    inputs = [(torch.from_numpy(x).half(), x) for x in a.Xs[0]]
    inputs += [(torch.from_numpy(x).half().reshape(2, 96, C), x) for x in b.Xs[0]]
    assert gm.HESSIAN_DEFER == 1
    old = (gm.STAGE_INPUTS, gm.FLUSH_EVENTS)
    try:
        for stage in (1, old[0]):
            gm.STAGE_INPUTS = stage
            gm.FLUSH_EVENTS = []
            lin = torch.nn.Linear(C, 4, bias=False, device=hip_device, dtype=torch.float16)
            gp = gptq_amd.GPTQ(lin)
            for t, _ in inputs:
                gp.add_batch(t.to(hip_device), None)
            H = gp.H.clone()
            torch.cuda.synchronize()
            events = list(gm.FLUSH_EVENTS)
            assert sum(e[1] for e in events) == len(inputs) and all(e[0] == [C] for e in events)
            if stage == 1:
                assert [e[1] for e in events] == [1] * len(inputs)
            want = np.zeros((C, C), dtype=np.float32)
            n, at = 0, 0
            for _, n_x, _, _ in events:
                group = inputs[at:at + n_x]
                batch = sum(1 if t.dim() == 2 else t.shape[0] for t, _ in group)
                assert len({x.shape for _, x in group}) == 1
                want = R.expected(want, [x for _, x in group], n, batch)
                n += batch
                at += n_x
            assert n == gp.nsamples == 7
            got = H.cpu()
            up = torch.triu(torch.ones(C, C, dtype=torch.bool))
            assert R.bits_equal(got[up], torch.from_numpy(want)[up]), f"gp.H differs from the reference (STAGE_INPUTS={stage})"
            assert R.bits_equal(got, got.t().contiguous()), "gp.H is not symmetric"
            gp.free()
    finally:
        gm.STAGE_INPUTS, gm.FLUSH_EVENTS = old
