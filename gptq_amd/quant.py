"""Affine weight quantizer and packed 2/3/4/8-bit Linear modules on MI355X.

Mirrors the reference's `quant.py` surface (`quantize`, `Quantizer`, `Quant3Linear`,
`make_quant3`) plus the int4 module whose layout the reference pins in
zeroShot/models/quant.py:172-209, and 2- and 8-bit modules on the same rule (the other
widths the drivers' `--wbits` offers): code i of a column in word i // (32/bits) at bit
bits * (i % (32/bits)).  All arithmetic on the hot path runs in libgptq_hip.so; torch
only owns memory.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from . import quant_cuda  # noqa: F401  (the extension-module name is part of the reference API)
from ._packed import PACKED_BITS, _check_bits, _check_operands, _f32, _launch, _on_gpu, _rows, check_perm  # noqa: F401


def _dev_of(t: torch.Tensor) -> torch.device:
    _lib.require_gpu(t, "tensor")
    return t.device


def quantize(x, scale, zero, maxq):
    """scale * (clamp(round(x / scale) + zero, 0, maxq) - zero)   (reference quant.py:6-10).

    Fast path: x [R, C] with per-row grids scale/zero [R, 1] -> one HIP pass.  Other
    broadcast shapes are elementwise torch on the tensors' own device.
    """
    maxq_i = int(maxq)
    if maxq_i < 0:
        raise NotImplementedError("trits (maxq < 0) are outside the MI355X hot-path scope")
    def per_row(t):   # [R, 1] -- or [R] against a single column -- broadcasts along rows exactly like quant.py:9-10
        return tuple(t.shape) == (x.shape[0], 1) or (t.dim() == 1 and t.numel() == x.shape[0] and x.shape[1] == 1)
    if (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and per_row(scale) and per_row(zero)
            and ((maxq_i + 1) & maxq_i) == 0 and 0 < maxq_i <= 255):
        out = x.contiguous().clone()
        s = scale.reshape(-1).to(torch.float32).contiguous()
        z = zero.reshape(-1).to(torch.float32).contiguous()
        bits = (maxq_i + 1).bit_length() - 1
        with torch.cuda.device(x.device):
            _lib.call("gptq_quantize_rows", _lib.ptr(out), out.stride(0), out.shape[0], out.shape[1],
                      _lib.ptr(s), _lib.ptr(z), bits, _lib.stream(x.device))
        return out
    q = torch.clamp(torch.round(x / scale) + zero, 0, maxq_i)
    return scale * (q - zero)


class Quantizer(nn.Module):
    """Per-output-channel min/max affine grid (reference quant.py:12-131)."""

    def __init__(self, shape=1):
        super().__init__()
        self.register_buffer('maxq', torch.tensor(0))
        self.register_buffer('scale', torch.zeros(shape))
        self.register_buffer('zero', torch.zeros(shape))

    def configure(self, bits, perchannel=False, sym=True, mse=False, norm=2.4, grid=100, maxshrink=.8,
                  trits=False):
        self.wbits = bits
        self.maxq = torch.tensor(2 ** bits - 1)
        self.perchannel = perchannel
        self.sym = sym
        self.mse = mse
        self.norm = norm
        self.grid = grid
        self.maxshrink = maxshrink
        if trits:
            self.maxq = torch.tensor(-1)

    def find_params(self, x, weight=True):
        """Row-wise grid of a weight matrix (quant.py:37-77,105-109) via gptq_find_params."""
        if int(self.maxq) < 0:
            raise NotImplementedError("trits are outside the MI355X hot-path scope")
        if self.mse:
            raise NotImplementedError("mse grid search is outside the MI355X hot-path scope (never enabled by the drivers)")
        if not (self.perchannel and weight):
            raise NotImplementedError("only perchannel=True, weight=True grids are in the MI355X hot-path scope")
        dev = _dev_of(x)
        self.maxq = self.maxq.to(dev)
        w = x.flatten(1)
        if w.dtype != torch.float32 or w.stride(1) != 1:
            w = w.float().contiguous()
        R, C = w.shape
        scale = torch.empty(R, device=dev, dtype=torch.float32)
        zero = torch.empty(R, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.call("gptq_find_params", _lib.ptr(w), w.stride(0), R, 0, C, C, int(self.wbits), int(bool(self.sym)),
                      _lib.ptr(scale), _lib.ptr(zero), 1, 0, _lib.stream(dev))
        shape = [-1] + [1] * (x.dim() - 1)
        self.scale = scale.reshape(shape)
        self.zero = zero.reshape(shape)

    def quantize(self, x):
        if self.ready():
            return quantize(x, self.scale, self.zero, self.maxq)
        return x

    def enabled(self):
        return self.maxq > 0

    def ready(self):
        return torch.all(self.scale != 0)


def _pack(weight, scales, zeros_scaled, bits):
    """[out, in] weights on the grid -> int32 [in/32*bits, out] (quant.py:158-186 / zeroShot quant.py:176-185)."""
    bits = _check_bits(bits, "_pack")
    if weight.dim() != 2 or weight.shape[1] % 32:
        raise ValueError("_pack: weight must be [out, in] with in a multiple of 32")
    dev = _dev_of(weight)
    w = weight if weight.stride(-1) == 1 else weight.contiguous()
    n_out, n_in = w.shape
    s = scales.reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
    z = zeros_scaled.reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
    qweight = torch.empty((n_in // 32 * bits, n_out), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("gptq_pack_weights", _lib.ptr(w), _lib.dtype_code(w), w.stride(0), n_out, n_in,
                  _lib.ptr(s), _lib.ptr(z), bits, _lib.ptr(qweight), _lib.stream(dev))
    return qweight


def pack_codes(codes, bits):
    """uint8 integer codes [out, in] -> int32 [in/32*bits, out]; same layouts as `_pack`."""
    bits = _check_bits(bits, "pack_codes")
    if codes.dim() != 2 or codes.shape[1] % 32 or codes.dtype != torch.uint8:
        raise ValueError("pack_codes: codes must be uint8 [out, in] with in a multiple of 32")
    dev = _dev_of(codes)
    c = codes.contiguous()
    n_out, n_in = c.shape
    qweight = torch.empty((n_in // 32 * bits, n_out), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("gptq_pack_codes", _lib.ptr(c), c.stride(0), n_out, n_in, bits, _lib.ptr(qweight), _lib.stream(dev))
    return qweight


def dequant_packed(qweight, scale, zero, bits, groupsize, dtype=torch.float16, perm=None):
    """int32 [in/32*bits, out] + grids [G, out] (`zero` = integer zero point) -> dense [out, in] weights,
    computed as scale * (code - zero) like the solver itself (quant.py:10).  `perm` (int32 [in]): the act-order format,
    storage row j is written back to input column perm[j]."""
    bits = _check_bits(bits, "dequant_packed")
    if qweight.dim() != 2 or qweight.dtype != torch.int32 or qweight.shape[0] % bits:
        raise ValueError(f"dequant_packed: qweight must be int32 [in/32*{bits}, out]")
    n_out = qweight.shape[1]
    n_in = qweight.shape[0] // bits * 32
    if perm is not None:
        perm = check_perm(perm, n_in, qweight, "dequant_packed")
    dev = _dev_of(qweight)
    W = torch.empty((n_out, n_in), dtype=dtype, device=dev)
    symbol, extra = ("gptq_dequant_packed", ()) if perm is None else ("gptq_dequant_packed_perm", (perm,))
    _launch(symbol, dev, qweight.contiguous(), _f32(scale), _f32(zero), *extra, n_out, n_in, bits, int(groupsize),
            W, _lib.dtype_code(W), W.stride(0))
    return W


def pack_grouped(weight, scales, zeros, groupsize, bits, perm=None):
    """[out, in] weights on grouped grids -> int32 [in/32*bits, out] (gptq_pack_grouped).  scales / zeros: [in/groupsize,
    out] (zeros = zero*scale).  With `perm` (int32 [in]) storage row j holds input column perm[j] on the grid of group
    j // groupsize: the act-order format.  Each code is clamp(round((w + zeros) / scales), 0, 2^bits - 1)."""
    bits, groupsize = _check_bits(bits, "pack_grouped"), int(groupsize)
    w = weight if weight.stride(-1) == 1 else weight.contiguous()
    n_out, n_in = w.shape
    if groupsize <= 0 or groupsize % 32 or n_in % groupsize:
        raise ValueError("pack_grouped: groupsize must be a positive multiple of 32 that divides in_features")
    want = (n_in // groupsize, n_out)
    if tuple(scales.shape) != want or tuple(zeros.shape) != want:
        raise ValueError(f"pack_grouped: scales / zeros must be {want}")
    if perm is not None:
        perm = check_perm(perm, n_in, w, "pack_grouped")
    dev = _dev_of(w)
    s = scales.to(device=dev, dtype=torch.float32).contiguous()
    z = zeros.to(device=dev, dtype=torch.float32).contiguous()
    qweight = torch.empty((n_in // 32 * bits, n_out), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("gptq_pack_grouped", _lib.ptr(w), _lib.dtype_code(w), w.stride(0), n_out, n_in, _lib.ptr(s),
                  _lib.ptr(z), groupsize, _lib.ptr(perm), bits, _lib.ptr(qweight), _lib.stream(dev))
    return qweight


def quant_matmul(x, qweight, scales, zeros, bits, groupsize=-1, bias=None, out_dtype=None, perm=None):
    """x [..., K] (fp16 / bf16) times the packed weights -> [..., N] in `out_dtype` (default x.dtype), through the
    dequant GEMM of libgptq_hip.so (gptq_quant_gemm): the multi-token forward of the packed Linears.

    qweight int32 [K/32*bits, N] (the modules' layouts); scales / zeros (zeros = zero*scale) hold N values for per-row
    grids (groupsize <= 0) or [K/groupsize, N] for grouped ones; bias [N] or None.  fp32 accumulation, one rounding.
    `perm` (int32 [K], grouped grids only): the act-order format, packed row k multiplies x[..., perm[k]]
    (gptq_quant_gemm_perm); the result is bit-identical to quant_matmul(x[..., perm], ...) without it.

    Under autograd (`torch.is_grad_enabled() and x.requires_grad`) the same call runs inside `_PackedLinearFn`: the
    output has the same bits and a `grad_fn` whose backward is `quant_matmul_t`.  The checks below then run inside
    the Function's forward (still `ValueError`), and an x that is not fp16 / bf16 raises "backward through packed
    Linears needs fp16/bf16 activations" instead of "x must be fp16 or bf16".  Where `scales`, `zeros` or `bias`
    require grad the call runs inside `_PackedGridFn` (same forward bits), whose backward adds `quant_grid_grad`."""
    if torch.is_grad_enabled() and (x.requires_grad or _grids_need_grad(scales, zeros, bias)):
        return _apply_packed(x, _GemmForward(qweight, scales, zeros, bits, groupsize, bias, out_dtype, perm))
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"quant_matmul: x must be fp16 or bf16, got {x.dtype}")
    if out_dtype is None:
        out_dtype = x.dtype
    if out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"quant_matmul: out_dtype must be fp32, fp16 or bf16, got {out_dtype}")
    K, N, bits, groupsize, perm = _check_operands("quant_matmul", qweight, bits, groupsize, scales, zeros, bias, perm,
                                                  ref=x, K=x.shape[-1])
    _on_gpu(("x", x), ("qweight", qweight), ("scales", scales), ("zeros", zeros), ("bias", bias))
    x2, ldx = _rows(x, K)
    M = x2.shape[0]
    y = torch.empty((M, N), dtype=out_dtype, device=x.device)
    if M:
        symbol, extra = ("gptq_quant_gemm", ()) if perm is None else ("gptq_quant_gemm_perm", (perm,))
        _launch(symbol, x.device, x2, _lib.dtype_code(x2), ldx, M, qweight.contiguous(), _f32(scales), _f32(zeros), *extra,
                _f32(bias), K, N, bits, groupsize, y, _lib.dtype_code(y), y.stride(0), ws_dims=(M, K, N, bits, groupsize))
    return y.reshape(list(x.shape[:-1]) + [N])


A8_MAX_K = 65536          # 255 * 127 * K must stay below 2^31 (the int32 sums of gptq_quant_gemm_a8)


def quantize_activations(x, perm=None):
    """x [..., K] (fp16 / bf16) -> (xq int8 [..., K], sx fp32 [...]): one symmetric int8 grid per token row
    (gptq_quant_act_rows).  With a = max_k |x[m][k]| in fp32,

        sx[m] = a / 127 (IEEE fp32 division; 1.0 when a == 0),   xq[m][k] = clamp(rint(x[m][k] / sx[m]), -127, 127)

    with a true division and round-half-even.  `perm` (int32 [K]): the act-order gather fused in, xq[m][k] is the code of
    x[m][perm[k]] (the row maximum does not depend on the order), so the result equals the call on x[..., perm].
    K must be a multiple of 32.  Non-finite activations (inf, nan) are outside the contract: their codes and scales are
    unspecified."""
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"quantize_activations: x must be an fp16 or bf16 tensor, got {getattr(x, 'dtype', type(x))}")
    if x.dim() == 0:
        raise ValueError("quantize_activations: x must have at least one dimension")
    K = x.shape[-1]
    if K == 0 or K % 32:
        raise ValueError(f"quantize_activations: the last dimension must be a positive multiple of 32, got {K}")
    if perm is not None:
        perm = check_perm(perm, K, x, "quantize_activations")
    return _quant_act_rows(x, K, perm)


def _quant_act_rows(x, K, perm):
    """`quantize_activations` behind its checks."""
    _lib.require_gpu(x, "x")
    x2, ldx = _rows(x.detach(), K)
    M = x2.shape[0]
    xq = torch.empty((M, K), dtype=torch.int8, device=x.device)
    sx = torch.empty(M, dtype=torch.float32, device=x.device)
    if M:
        _launch("gptq_quant_act_rows", x.device, x2, _lib.dtype_code(x2), ldx, M, K, perm, xq, K, sx)
    return xq.reshape(x.shape), sx.reshape(x.shape[:-1])


def quant_matmul_a8(x, qweight, scales, zeros, bits, groupsize=-1, bias=None, out_dtype=None, perm=None):
    """`quant_matmul` on int8 activations (gptq_quant_gemm_a8): an opt-in serving mode, INFERENCE ONLY.

    `x` is either an fp16 / bf16 tensor [..., K], quantized inside by `quantize_activations(x, perm)`, or the pair
    `(xq, sx)` that call returns (int8 [..., K] and fp32 [...]; already in storage order, so `perm` must be None).  The
    other operands and their checks are those of `quant_matmul`; `out_dtype` defaults to x.dtype (fp16 for the pair).  Per
    output and per group g of K (per-row grids: one group), with exact int32 sums on the integer-MFMA units,

        I_g = sum q[k][n] xq[m][k],  X_g = sum xq[m][k],  y[m][n] = sx[m] * sum_g (s[g][n] I_g - z[g][n] X_g) + bias[n]

    in fp32 with one rounding to `out_dtype`; the same call gives the same bits.  The result differs from `quant_matmul`
    by the int8 rounding of the activations (about 2^-8 of each row's largest value per element).  K <= 65536.  There is
    no backward: with grad enabled and an `x`, `scales`, `zeros` or `bias` that requires grad this raises ValueError."""
    who = "quant_matmul_a8"
    pair = isinstance(x, (tuple, list))
    if pair:
        if len(x) != 2 or not all(isinstance(t, torch.Tensor) for t in x):
            raise ValueError(f"{who}: x must be a tensor or the pair (xq, sx)")
        xq, sx = x
        if xq.dtype != torch.int8 or sx.dtype != torch.float32:
            raise ValueError(f"{who}: the pair must be (int8 xq, fp32 sx), got ({xq.dtype}, {sx.dtype})")
        if xq.dim() == 0 or tuple(sx.shape) != tuple(xq.shape[:-1]):
            raise ValueError(f"{who}: sx {tuple(sx.shape)} must have the shape of xq {tuple(xq.shape)} without its last "
                             "dimension")
        if perm is not None:
            raise ValueError(f"{who}: perm belongs to the activation quantization; the pair (xq, sx) is in storage order")
        shape, default_dtype = xq.shape, torch.float16
    else:
        if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"{who}: x must be fp16 or bf16 (or the pair (xq, sx)), got {getattr(x, 'dtype', type(x))}")
        if x.dim() == 0:
            raise ValueError(f"{who}: x must have at least one dimension")
        shape, default_dtype = x.shape, x.dtype
    if torch.is_grad_enabled() and ((not pair and x.requires_grad) or (pair and sx.requires_grad)
                                    or _grids_need_grad(scales, zeros, bias)):
        raise ValueError(f"{who}: inference only -- no backward through int8 activations (use quant_matmul, or "
                         "torch.no_grad())")
    if out_dtype is None:
        out_dtype = default_dtype
    if out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"{who}: out_dtype must be fp32, fp16 or bf16, got {out_dtype}")
    K, N, bits, groupsize, perm = _check_operands(who, qweight, bits, groupsize, scales, zeros, bias, perm, ref=x,
                                                  K=shape[-1], max_k=A8_MAX_K)
    if not pair:
        xq, sx = _quant_act_rows(x, K, perm)                  # (the first step that needs the GPU)
    _on_gpu(("xq", xq), ("sx", sx), ("qweight", qweight), ("scales", scales), ("zeros", zeros), ("bias", bias))
    xq2, ldx = _rows(xq, K)
    M = xq2.shape[0]
    y = torch.empty((M, N), dtype=out_dtype, device=xq.device)
    if M:
        _launch("gptq_quant_gemm_a8", xq.device, xq2, ldx, sx.reshape(-1).contiguous(), M, qweight.contiguous(),
                _f32(scales), _f32(zeros), _f32(bias), K, N, bits, groupsize, y, _lib.dtype_code(y), y.stride(0),
                ws_dims=(M, K, N, bits, groupsize))
    return y.reshape(list(shape[:-1]) + [N])


def quant_matmul_t(grad, qweight, scales, zeros, bits, groupsize=-1, out_dtype=None, perm=None):
    """grad [..., N] (fp16 / bf16) times the TRANSPOSED packed weights -> [..., K] in `out_dtype` (default grad.dtype),
    through the transposed dequant GEMM of libgptq_hip.so (gptq_quant_gemm_t): the gradient of `quant_matmul` and of the
    packed Linears with respect to their input.

    Operands as in `quant_matmul`.  Each weight is formed in fp32 as scale * code - zeros and rounded once to grad's
    dtype; fp32 accumulation over N, one rounding.  `perm` (int32 [K], grouped grids only): the act-order format,
    packed row k lands in column perm[k] of the result."""
    if grad.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"quant_matmul_t: grad must be fp16 or bf16, got {grad.dtype}")
    if out_dtype is None:
        out_dtype = grad.dtype
    if out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"quant_matmul_t: out_dtype must be fp32, fp16 or bf16, got {out_dtype}")
    K, N, bits, groupsize, perm = _check_operands("quant_matmul_t", qweight, bits, groupsize, scales, zeros, perm=perm,
                                                  ref=grad, N=grad.shape[-1])
    _on_gpu(("grad", grad), ("qweight", qweight), ("scales", scales), ("zeros", zeros))
    g2, ldg = _rows(grad, N)
    M = g2.shape[0]
    dx = torch.empty((M, K), dtype=out_dtype, device=grad.device)
    if M:
        _launch("gptq_quant_gemm_t", grad.device, g2, _lib.dtype_code(g2), ldg, M, qweight.contiguous(), _f32(scales),
                _f32(zeros), perm, K, N, bits, groupsize, dx, _lib.dtype_code(dx), dx.stride(0),
                ws_dims=(M, K, N, bits, groupsize))
    return dx.reshape(list(grad.shape[:-1]) + [K])


def quant_grid_grad(x, grad, qweight, bits, groupsize=-1, perm=None, bias=True):
    """The gradients of `quant_matmul` with respect to its grids, with the integer codes frozen
    (gptq_quant_gemm_grid_grad): x [..., K] and grad [..., N] (the same fp16 / bf16 type, the same leading dimensions)
    -> (dscales, dzeros, dbias), fp32.  With A = x[..., c(k)]^T grad (never stored; c(k) = perm[k] or k),

        dscales[g][n] = sum_{k in g} q[k][n] A[k][n],   dzeros[g][n] = -sum_{k in g} A[k][n],   dbias[n] = sum_m grad[m][n]

    i.e. the gradients with respect to the STORED tensors (`zeros` = zero*scale).  dscales / dzeros are [K/groupsize, N]
    for grouped grids and [N] for per-row ones; dbias is [N], or None with `bias=False`.  fp32 accumulation, nothing is
    rounded to 16 bits, no atomics (the same call gives the same bits)."""
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"quant_grid_grad: x must be fp16 or bf16, got {x.dtype}")
    if grad.dtype != x.dtype:
        raise ValueError(f"quant_grid_grad: grad must have x's dtype {x.dtype}, got {grad.dtype}")
    K, N, bits, groupsize, perm = _check_operands("quant_grid_grad", qweight, bits, groupsize, perm=perm, ref=x,
                                                  K=x.shape[-1], N=grad.shape[-1])
    if x.numel() // K != grad.numel() // N:
        raise ValueError(f"quant_grid_grad: x {tuple(x.shape)} and grad {tuple(grad.shape)} hold different numbers of tokens")
    _on_gpu(("x", x), ("grad", grad), ("qweight", qweight))
    dev = x.device
    (x2, ldx), (g2, ldg) = _rows(x, K), _rows(grad, N)
    M = x2.shape[0]
    shape = (K // groupsize, N) if groupsize > 0 else (N,)
    if M == 0:
        return (torch.zeros(shape, device=dev), torch.zeros(shape, device=dev),
                torch.zeros(N, device=dev) if bias else None)
    ds = torch.empty(shape, dtype=torch.float32, device=dev)
    dz = torch.empty(shape, dtype=torch.float32, device=dev)
    db = torch.empty(N, dtype=torch.float32, device=dev) if bias else None
    _launch("gptq_quant_gemm_grid_grad", dev, x2, _lib.dtype_code(x2), ldx, g2, ldg, M, qweight.contiguous(), perm,
            K, N, bits, groupsize, ds, dz, db, ws_dims=(M, K, N, bits, groupsize),
            ws_symbol=None if perm is None else "gptq_quant_gemm_grid_grad_perm")
    return ds, dz, db


def _grids_need_grad(scales, zeros, bias):
    return scales.requires_grad or zeros.requires_grad or (bias is not None and bias.requires_grad)


def _apply_packed(x, op):
    """The autograd route of one packed forward: `_PackedGridFn` where a grid tensor requires grad, the x-only
    `_PackedLinearFn` otherwise."""
    if _grids_need_grad(op.scales, op.zeros, op.bias):
        return _PackedGridFn.apply(x, op.scales, op.zeros, op.bias, op)
    return _PackedLinearFn.apply(x, op)


class _GemmForward:
    """The operands of one packed forward as `_PackedLinearFn` carries them: `forward(x)` is the module's own path
    (run without grad, so the same bits), the rest is what `quant_matmul_t` needs."""

    def __init__(self, qweight, scales, zeros, bits, groupsize, bias=None, out_dtype=None, perm=None, forward=None):
        self.qweight, self.scales, self.zeros, self.perm, self.bias = qweight, scales, zeros, perm, bias
        self.bits, self.groupsize = int(bits), int(groupsize)
        self.forward = forward if forward is not None else (
            lambda x: quant_matmul(x, qweight, scales, zeros, bits, groupsize, bias, out_dtype, perm))


def _packed_forward(ctx, x, op):
    """The forward of both Functions: the path taken without autograd, run without grad (so the same bits)."""
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"backward through packed Linears needs fp16/bf16 activations, got {x.dtype}")
    ctx.op = op
    ctx.x_dtype = x.dtype
    with torch.no_grad():
        return op.forward(x.detach())


def _grad_input(ctx, grad):
    """The start of both backwards: (grad in x's dtype, which the weights round to -- it differs under an fp32
    `out_dtype`; dx = `quant_matmul_t` of it, or None where x needs no gradient)."""
    op = ctx.op
    if grad.dtype != ctx.x_dtype:
        grad = grad.to(ctx.x_dtype)
    if not ctx.needs_input_grad[0]:
        return grad, None
    return grad, quant_matmul_t(grad, op.qweight, op.scales.detach(), op.zeros.detach(), op.bits, op.groupsize,
                                ctx.x_dtype, op.perm)


class _PackedLinearFn(torch.autograd.Function):
    """y = packed(x) with a gradient for x only (no grid tensor requires grad; see `_PackedGridFn`).  Forward: exactly the path taken
    without autograd -- the dequant GEMM for several tokens, the mat-vec for one.  Backward: `quant_matmul_t`."""

    @staticmethod
    def forward(ctx, x, op):
        return _packed_forward(ctx, x, op)

    @staticmethod
    def backward(ctx, grad):
        return _grad_input(ctx, grad)[1], None


class _PackedGridFn(torch.autograd.Function):
    """y = packed(x) with gradients for x and for the grids (`scales`, `zeros`, `bias` as tensor inputs; the codes stay
    frozen).  Forward: exactly the path taken without autograd.  Backward: `quant_matmul_t` for x where it needs one,
    `quant_grid_grad` for the grids, reshaped to the tensors' own shapes ([out, 1] in the per-row modules).  x is saved
    only where a grid tensor requires grad."""

    @staticmethod
    def forward(ctx, x, scales, zeros, bias, op):
        if any(ctx.needs_input_grad[1:4]):
            ctx.save_for_backward(x)
        return _packed_forward(ctx, x, op)

    @staticmethod
    def backward(ctx, grad):
        op = ctx.op
        grad, dx = _grad_input(ctx, grad)
        ds = dz = db = None
        if any(ctx.needs_input_grad[1:4]):
            x, = ctx.saved_tensors
            gs, gz, gb = quant_grid_grad(x, grad, op.qweight, op.bits, op.groupsize, op.perm,
                                         bias=bool(ctx.needs_input_grad[3]))
            if ctx.needs_input_grad[1]:
                ds = gs.reshape(op.scales.shape).to(op.scales.dtype)
            if ctx.needs_input_grad[2]:
                dz = gz.reshape(op.zeros.shape).to(op.zeros.dtype)
            if ctx.needs_input_grad[3]:
                db = gb.reshape(op.bias.shape).to(op.bias.dtype)
        return dx, ds, dz, db, None


GRID_NAMES = ("scales", "zeros", "bias")


def _packed_modules(model, named=False):
    """Every packed Linear of `model` (per-row and grouped modules alike); with `named`, as (name, module) pairs."""
    found = [(name, m) for name, m in model.named_modules() if isinstance(m, _PackedLinear)]
    return found if named else [m for _, m in found]


def trainable_grids(model, scales=True, zeros=True, bias=True):
    """Opt in to training the grids of every packed Linear in `model`: the chosen buffers (`scales`, `zeros` = zero*scale,
    `bias`) become fp32 `nn.Parameter`s under the same names, so `state_dict` keys do not change and checkpoints load
    both ways; `qweight` (and `perm`) stay buffers, the integer codes stay frozen.  Call it after the modules are packed
    or loaded.  Returns the new parameters (hand them to an optimizer); `frozen_grids` turns them back into buffers."""
    params = []
    for m in _packed_modules(model):
        for name, on in zip(GRID_NAMES, (scales, zeros, bias)):
            if on and name in m._buffers:
                p = nn.Parameter(m._buffers.pop(name).detach().float(), requires_grad=True)
                m.register_parameter(name, p)
                params.append(p)
    return params


def frozen_grids(model):
    """Undo `trainable_grids`: every grid parameter of a packed Linear becomes a buffer again, holding its current
    (trained) values.  Returns the number of tensors turned back."""
    n = 0
    for m in _packed_modules(model):
        for name in GRID_NAMES:
            if name in m._parameters:
                p = m._parameters.pop(name)
                m.register_buffer(name, p.detach())
                n += 1
    return n


class _PackedLinear(nn.Module):
    """What the five packed Linears share: the route of `forward` (autograd, int8 activations, `_forward`) and the
    single-token / multi-token split of `_forward`.  A subclass supplies `_operands`, `_vec` and `_matvec`."""
    act_bits = None    # 8: multi-token inputs outside autograd take quant_matmul_a8 (a plain attribute; set_act_bits)
    multi_token = False

    @staticmethod
    def _staging_device(home):
        """Where `pack` runs for a Linear on `home`: there if it is a GPU, else on the current one."""
        if home.type == 'cuda':
            return home
        if torch.cuda.is_available():
            return torch.device('cuda', torch.cuda.current_device())
        raise _lib.GptqHipError("packing needs an MI355X device; gptq_amd has no CPU path")

    def forward(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or _grids_need_grad(self.scales, self.zeros, self.bias)):
            return _apply_packed(x, _GemmForward(*self._operands(), forward=self._forward))
        if self.act_bits == 8 and self.multi_token and x.shape[-1] != x.numel():
            return quant_matmul_a8(x, *self._operands())
        return self._forward(x)

    def _forward(self, x):
        if x.shape[-1] == x.numel():
            y = self.bias.clone().float()
            self._matvec(self._vec(x), y)
            return y.to(x.dtype).reshape(list(x.shape[:-1]) + [self.bias.numel()])
        if self.multi_token:
            return quant_matmul(x, *self._operands())
        raise ValueError('Only supports a single token currently.')


class _QuantLinearBase(_PackedLinear):
    """Packed Linear with one (scale, zero) per output row.  The constructor accepts either (infeatures, outfeatures)
    like Quant3Linear or the reference's (linear, scales, zeros) form (zeroShot/models/quant.py:172)."""
    bits = 0
    faster = False

    def __init__(self, infeatures, outfeatures=None, zeros=None, faster=False, multi_token=False):
        super().__init__()
        self.faster = faster
        self.multi_token = multi_token   # inputs of several tokens -> quant_matmul (a plain attribute: no state_dict key)
        linear = infeatures if isinstance(infeatures, nn.Module) else None
        n_in, n_out = (linear.in_features, linear.out_features) if linear is not None else (infeatures, outfeatures)
        self.register_buffer('zeros', torch.zeros((n_out, 1)))
        self.register_buffer('scales', torch.zeros((n_out, 1)))
        self.register_buffer('bias', torch.zeros(n_out))
        self.register_buffer('qweight', torch.zeros((n_in // 32 * self.bits, n_out), dtype=torch.int))
        if linear is not None:
            self.pack(linear, outfeatures, zeros)

    def pack(self, linear, scales, zeros):
        """Same contract as Quant3Linear.pack (quant.py:152-187): `zeros` is the integer zero point.

        Tensors may live on the host (the reference packs on the CPU, opt.py:370); they are
        staged on the GPU, packed there and the buffers return to the source device.
        """
        home = linear.weight.device
        dev = self._staging_device(home)
        scales = scales.to(dev)
        self.zeros = (zeros.to(dev) * scales).to(home)
        self.scales = scales.clone().to(home)
        if linear.bias is not None:
            self.bias = linear.bias.detach().clone()
        qweight = _pack(linear.weight.data.to(dev), scales, self.zeros.to(dev), self.bits)
        self.qweight = qweight.to(home)

    def _operands(self):
        return self.qweight, self.scales, self.zeros, self.bits, -1, self.bias

    def _vec(self, x):
        return x.half() if self.faster else x.float()


class Quant3Linear(_QuantLinearBase):
    """3-bit packed Linear (reference quant.py:139-203).  Single-token inputs take the mat-vec; with
    `multi_token=True`, inputs of several tokens take the dequant GEMM (`quant_matmul`), otherwise they raise like
    the reference."""
    bits = 3

    def __init__(self, infeatures, outfeatures, faster=False, multi_token=False):
        super().__init__(infeatures, outfeatures, faster=faster, multi_token=multi_token)

    def _matvec(self, x, y):
        if self.faster:
            quant_cuda.vecquant3matmul_faster(x, self.qweight, y, self.scales, self.zeros)
        else:
            quant_cuda.vecquant3matmul(x, self.qweight, y, self.scales, self.zeros)


class Quant4Linear(_QuantLinearBase):
    """4-bit packed Linear; buffer layout of zeroShot/models/quant.py:172-197 (nibble i%8 of word i//8).

    The reference only defines the layout (its `vecquant4matmul` kernel does not exist); the
    constructor accepts either (infeatures, outfeatures) like Quant3Linear or the reference's
    (linear, scales, zeros) form.
    """
    bits = 4

    def _matvec(self, x, y):
        quant_cuda.vecquant4matmul(x, self.qweight, y, self.scales, self.zeros)


class Quant2Linear(_QuantLinearBase):
    """2-bit packed Linear: code i of a column in word i // 16 at bit 2 * (i % 16).  The 4-bit module's rule with 16
    codes per word; same constructor forms and buffers as Quant4Linear."""
    bits = 2

    def _matvec(self, x, y):
        quant_cuda.vecquant2matmul(x, self.qweight, y, self.scales, self.zeros)


class Quant8Linear(_QuantLinearBase):
    """8-bit packed Linear: code i of a column in byte i % 4 of word i // 4.  The 4-bit module's rule with 4 codes per
    word; same constructor forms and buffers as Quant4Linear."""
    bits = 8

    def _matvec(self, x, y):
        quant_cuda.vecquant8matmul(x, self.qweight, y, self.scales, self.zeros)


class QuantGroupLinear(_PackedLinear):
    """Packed Linear with one (scale, zero) per `groupsize` input columns.

    The reference cannot pack grouped models (Quant3Linear keeps per-row scalars, quant.py:144-145, and
    fasterquant leaves only the LAST group's grid in the quantizer).  Buffers: `qweight` int32
    [in/32*bits, out] (same bit layouts as the per-row modules), `scales` / `zeros` fp32 [in/groupsize, out]
    (`zeros` = zero*scale), `bias`.  Runs without act-order and runs with static groups store the codes in original
    column order.  `act_order=True` is the format of act-order runs with dynamic groups, whose groups are consecutive
    positions of the permuted column order: storage row j holds input column perm[j] on the grid of group j // groupsize,
    and an int32 buffer `perm` [in] is added ("Grouped and act-order checkpoints").
    """

    def __init__(self, bits, groupsize, infeatures, outfeatures, multi_token=False, act_order=False):
        super().__init__()
        self.multi_token = multi_token
        if bits not in PACKED_BITS or groupsize <= 0 or groupsize % 32 or infeatures % groupsize:
            raise ValueError("QuantGroupLinear: bits in {2,3,4,8}, groupsize % 32 == 0, in_features % groupsize == 0")
        self.bits, self.groupsize = bits, groupsize
        self.act_order = bool(act_order)
        self.register_buffer('qweight', torch.zeros((infeatures // 32 * bits, outfeatures), dtype=torch.int))
        self.register_buffer('scales', torch.zeros((infeatures // groupsize, outfeatures)))
        self.register_buffer('zeros', torch.zeros((infeatures // groupsize, outfeatures)))
        self.register_buffer('bias', torch.zeros(outfeatures))
        if self.act_order:
            self.register_buffer('perm', torch.arange(infeatures, dtype=torch.int32))

    @classmethod
    def from_gptq(cls, solver, bits, multi_token=False):
        """Build from a `GPTQ` object after `fasterquant(groupsize=g, ...)`.  Act-order with dynamic groups gives an
        `act_order=True` module (codes packed in the permuted order); every other grouped run today's format."""
        gs, gz = solver.group_scale, solver.group_zero          # [out, G]
        if gs is None:
            raise ValueError("QuantGroupLinear.from_gptq: the solver ran without groups")
        act = solver.perm is not None and not getattr(solver, "static_groups", False)
        n_out, n_in = solver.codes.shape
        m = cls(bits, n_in // gs.shape[1], n_in, n_out, multi_token=multi_token, act_order=act)
        if act:
            perm = solver.perm.to(torch.int32)
            m.qweight = pack_codes(solver.codes.index_select(1, perm.long()), bits)
            m.perm = perm.contiguous().clone()
        else:
            m.qweight = pack_codes(solver.codes, bits)
        m.scales = gs.t().contiguous()
        m.zeros = (gz * gs).t().contiguous()
        bias = getattr(solver.layer, "bias", None)
        m.bias = bias.detach().clone().float() if bias is not None else torch.zeros(n_out, device=gs.device)
        return m

    def pack(self, linear, group_scale, group_zero, perm=None):
        """Fill the buffers from a Linear holding fake-quantized weights and its grids `group_scale` / `group_zero`
        [out, G] (`group_zero` = the integer zero point), as the driver's quantizers carry them.  `perm` (act-order
        modules only): the solver's permutation.  Like the per-row modules' `pack`, the packing runs on the GPU and the
        buffers go back to the Linear's device."""
        if (perm is not None) != self.act_order:
            raise ValueError("QuantGroupLinear.pack: perm is needed exactly for act_order=True modules")
        home = linear.weight.device
        dev = self._staging_device(home)
        gs = group_scale.to(device=dev, dtype=torch.float32)
        scales = gs.t().contiguous()
        zeros = (group_zero.to(device=dev, dtype=torch.float32) * gs).t().contiguous()
        p = perm.to(device=dev, dtype=torch.int32) if perm is not None else None
        qweight = pack_grouped(linear.weight.data.to(dev), scales, zeros, self.groupsize, self.bits, p)
        self.qweight = qweight.to(home)
        self.scales = scales.to(home)
        self.zeros = zeros.to(home)
        if linear.bias is not None:
            self.bias = linear.bias.detach().float().clone().to(home)
        if p is not None:
            self.perm = p.clone().to(home)

    @property
    def g_idx(self):
        """Group index of every ORIGINAL input column (int32 [in]), what other GPTQ tools call g_idx:
        g_idx[perm[j]] = j // groupsize for act-order modules, k // groupsize otherwise.  Derived, not stored."""
        n_in = self.qweight.shape[0] // self.bits * 32
        grp = torch.arange(n_in, dtype=torch.int32, device=self.qweight.device) // self.groupsize
        if not self.act_order:
            return grp
        g = torch.empty_like(grp)
        g[self.perm.long()] = grp
        return g

    def _operands(self):
        return (self.qweight, self.scales, self.zeros, self.bits, self.groupsize, self.bias, None,
                self.perm if self.act_order else None)

    def _vec(self, x):
        return x if x.dtype in (torch.float16, torch.float32) else x.float()

    def _matvec(self, x, y):
        quant_cuda.vecquant_matmul_grouped(x, self.qweight, y, self.scales, self.zeros, self.bits, self.groupsize,
                                           perm=self.perm if self.act_order else None)


def make_quant3(module, names, name='', faster=False, multi_token=False):
    """Replace the named Linears by empty Quant3Linear modules (reference quant.py:205-216)."""
    _make_quant(module, names, name, Quant3Linear, faster, multi_token)


def make_quant4(module, names, name='', faster=False, multi_token=False):
    _make_quant(module, names, name, Quant4Linear, faster, multi_token)


def make_quant2(module, names, name='', faster=False, multi_token=False):
    _make_quant(module, names, name, Quant2Linear, faster, multi_token)


def make_quant8(module, names, name='', faster=False, multi_token=False):
    _make_quant(module, names, name, Quant8Linear, faster, multi_token)


PACKED_LINEAR = {2: Quant2Linear, 3: Quant3Linear, 4: Quant4Linear, 8: Quant8Linear}   # per-row module of each width


def _make_quant(module, names, name, cls, faster, multi_token=False):
    if isinstance(module, _QuantLinearBase):
        return
    for attr in dir(module):
        tmp = getattr(module, attr)
        full = name + '.' + attr if name != '' else attr
        if full in names:
            setattr(module, attr, cls(tmp.in_features, tmp.out_features, faster=faster, multi_token=multi_token))
    for child_name, child in module.named_children():
        _make_quant(child, names, name + '.' + child_name if name != '' else child_name, cls, faster, multi_token)


def set_multi_token(model, enabled=True):
    """Switch the multi-token forward (`quant_matmul`) of every packed Linear in `model` on or off, e.g. after
    loading a checkpoint into a skeleton built without it.  Returns the number of modules switched."""
    n = 0
    for m in _packed_modules(model):
        m.multi_token = bool(enabled)
        n += 1
    return n


def set_act_bits(model, bits=8):
    """Switch every packed Linear in `model` to int8 activations (`bits=8`) or back (`bits=None`).  With `multi_token` on
    and `act_bits == 8`, an input of several tokens that needs no gradient takes `quant_matmul_a8`; single tokens stay on
    the mat-vec (decode is bound by the weight bytes) and any input under autograd stays on the fp16 path, so a model's
    training-time forward and its int8 serving forward differ by the activations' int8 rounding.  `act_bits` is a plain
    attribute: no `state_dict` key, off by default, and with it off every output is bit-identical to before.  Returns the
    number of modules switched."""
    if bits not in (8, None):
        raise ValueError(f"set_act_bits: act_bits must be 8 or None, got {bits!r}")
    n = 0
    for m in _packed_modules(model):
        m.act_bits = bits
        n += 1
    return n
