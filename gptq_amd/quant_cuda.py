"""Packed dequant mat-vec entry points.

The reference loads a torch extension module literally named `quant_cuda`
(quant.py:134-137, setup_cuda.py:5-7) exporting `vecquant3matmul` and
`vecquant3matmul_faster` (quant_cuda.cpp:51-54).  The name is API, so it is kept;
the implementation is the gfx950 kernel in csrc/matvec.hip behind the C ABI.
`vecquant4matmul` is what zeroShot/models/quant.py:193 calls but the reference never
implemented.

All functions accumulate IN PLACE into `mul` (which the caller pre-loads with the
bias, quant.py:192) and return None.
"""
from __future__ import annotations

import torch

from . import _lib
from ._packed import _check_bits, _f32, _launch
from ._packed import check_perm as _check_perm


def _run(symbol, bits, vec, mat, mul, scales, zeros, vec_dtypes, who=None, groupsize=None, perm=None):
    """Check the operands of one mat-vec and launch it: per-row grids of `width` values, or (with `groupsize`) grouped
    ones [in/groupsize, out] behind the two extra arguments of the grouped symbols."""
    who = who or symbol
    for name, t in (("vec", vec), ("mat", mat), ("mul", mul), ("scales", scales), ("zeros", zeros)):
        _lib.require_gpu(t, name)
    if vec.dtype not in vec_dtypes:
        raise TypeError(f"{who}: vec must be {' or '.join(str(d) for d in vec_dtypes)}, got {vec.dtype}")
    if mat.dtype != torch.int32 or mat.dim() != 2 or not mat.is_contiguous():
        raise TypeError(f"{who}: mat must be a contiguous int32 [in/32*{bits}, out] tensor")
    if mul.dtype != torch.float32 or not mul.is_contiguous():
        raise TypeError(f"{who}: mul must be contiguous fp32")
    height, width = mat.shape
    n_in = height // bits * 32
    if vec.numel() != n_in:
        raise ValueError(f"{who}: vec has {vec.numel()} elements, mat implies {n_in}")
    if groupsize is None:
        if mul.numel() != width or scales.numel() != width or zeros.numel() != width:
            raise ValueError(f"{who}: mul/scales/zeros must have {width} elements")
        extra = ()
    else:
        want = (n_in // groupsize, width)
        if mul.numel() != width or tuple(scales.shape) != want or tuple(zeros.shape) != want:
            raise ValueError(f"{who}: shape mismatch: mul must have {width} elements, scales / zeros must be {want}")
        extra = (bits, groupsize)
    _launch(symbol, vec.device, vec.reshape(-1).contiguous(), _lib.dtype_code(vec), mat, mul, _f32(scales), _f32(zeros),
            *(() if perm is None else (perm,)), height, width, *extra)


_F16_OR_F32 = (torch.float32, torch.float16)


def vecquant3matmul(vec, mat, mul, scales, zeros):
    """Single-token 3-bit mat-vec (quant_cuda.cpp:15-21).  fp32 operands run as they are.  The reference also
    dispatches fp64 (AT_DISPATCH_FLOATING_TYPES, quant_cuda_kernel.cu:47): fp64 `vec/mul/scales/zeros` are accepted
    too -- the kernel computes in fp32 (gfx950 has no fp64 matrix path worth a second kernel for a test-only dtype)
    and the sum is added into `mul` in fp64, so the result agrees with the reference's to fp32 rounding (~1e-7
    relative), not to fp64 rounding."""
    if vec.dtype == torch.float64:
        for name, t in (("mul", mul), ("scales", scales), ("zeros", zeros)):
            if t.dtype != torch.float64:
                raise TypeError(f"vecquant3matmul: {name} must be fp64 like vec (the reference dispatches on vec's type)")
        acc = torch.zeros(mul.shape, dtype=torch.float32, device=mul.device)
        _run("gptq_vecquant3matmul", 3, vec.float(), mat, acc, scales.float(), zeros.float(), (torch.float32,))
        mul += acc.double()
        return
    _run("gptq_vecquant3matmul", 3, vec, mat, mul, scales, zeros, (torch.float32,))


def vecquant3matmul_faster(vec, mat, mul, scales, zeros):
    """fp16-input form (quant_cuda.cpp:23-29); accumulates in fp32 here."""
    _run("gptq_vecquant3matmul", 3, vec, mat, mul, scales, zeros, (torch.float16,))


def vecquant4matmul(vec, mat, mul, scales, zeros):
    """4-bit analogue on the zeroShot/models/quant.py:185 layout; vec fp32 or fp16."""
    _run("gptq_vecquant4matmul", 4, vec, mat, mul, scales, zeros, _F16_OR_F32)


def vecquant2matmul(vec, mat, mul, scales, zeros):
    """2-bit analogue (code i of a column in word i // 16 at bit 2 * (i % 16)); vec fp32 or fp16."""
    _run("gptq_vecquant2matmul", 2, vec, mat, mul, scales, zeros, _F16_OR_F32)


def vecquant8matmul(vec, mat, mul, scales, zeros):
    """8-bit analogue (code i of a column in byte i % 4 of word i // 4); vec fp32 or fp16."""
    _run("gptq_vecquant8matmul", 8, vec, mat, mul, scales, zeros, _F16_OR_F32)


def vecquant_matmul_grouped(vec, mat, mul, scales, zeros, bits, groupsize, perm=None):
    """Grouped-grid mat-vec: scales / zeros are [in/groupsize, out], zeros = zero*scale.  `perm` (int32
    [in]): the act-order format, packed row k multiplies vec[perm[k]] (gptq_vecquant_matmul_grouped_perm)."""
    bits, groupsize = _check_bits(bits, "vecquant_matmul_grouped"), int(groupsize)
    if groupsize <= 0 or groupsize % 32:
        raise ValueError("vecquant_matmul_grouped: groupsize must be a positive multiple of 32")
    if perm is not None:
        perm = _check_perm(perm, mat.shape[0] // bits * 32, vec, "vecquant_matmul_grouped")
    _run("gptq_vecquant_matmul_grouped" if perm is None else "gptq_vecquant_matmul_grouped_perm", bits, vec, mat, mul,
         scales, zeros, _F16_OR_F32, "vecquant_matmul_grouped", groupsize, perm)
