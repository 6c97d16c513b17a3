"""What every host wrapper of a packed kernel does before it launches: one check of the packed operands, one 2-D view
rule for activations and gradients, one launch.  `quant.py` (which re-exports the public names) and `quant_cuda.py`
both build on it."""
from __future__ import annotations

import torch

from . import _lib

PACKED_BITS = (2, 3, 4, 8)


def _check_bits(bits, who):
    bits = int(bits)
    if bits not in PACKED_BITS:
        raise ValueError(f"{who}: bits must be 2, 3, 4 or 8, got {bits}")
    return bits


def check_perm(perm, n_in, ref, who):
    """The act-order permutation as the kernels take it: int32 [n_in] on `ref`'s device, contiguous and 16-byte aligned.
    Raises ValueError before any launch."""
    if perm.dtype != torch.int32:
        raise ValueError(f"{who}: perm must be int32, got {perm.dtype}")
    if perm.dim() != 1 or perm.numel() != n_in:
        raise ValueError(f"{who}: perm must hold {n_in} entries (one per input feature), got shape {tuple(perm.shape)}")
    if perm.device != ref.device:
        raise ValueError(f"{who}: perm is on {perm.device}, the operands on {ref.device}")
    p = perm.contiguous()
    return p if p.data_ptr() % 16 == 0 else p.clone()


def _check_operands(who, qweight, bits, groupsize, scales=None, zeros=None, bias=None, perm=None, ref=None, K=None,
                    N=None, max_k=None):
    """The packed operands of one matmul, checked once on the host: returns (K, N, bits, groupsize, perm), perm as
    `check_perm` leaves it.  `K` / `N`: the input / output features the activation / gradient tensor `ref` implies
    (without `K` it follows from qweight).  `scales` / `zeros` / `bias` are checked where given."""
    bits, groupsize = _check_bits(bits, who), int(groupsize)
    if qweight.dtype != torch.int32 or qweight.dim() != 2:
        raise ValueError(f"{who}: qweight must be an int32 [K/32*bits, N] tensor")
    height, width = qweight.shape
    if K is None:
        if height % bits or height == 0:
            raise ValueError(f"{who}: qweight {tuple(qweight.shape)} is no [K/32*{bits}, N] buffer "
                             "(K must be a multiple of 32)")
        K = height // bits * 32
    elif K == 0 or K % 32 or height != K // 32 * bits:
        raise ValueError(f"{who}: x has {K} input features, qweight {tuple(qweight.shape)} implies "
                         f"{height // bits * 32} (and K must be a multiple of 32)")
    if N is not None and N != width:
        raise ValueError(f"{who}: grad has {N} output features, qweight {tuple(qweight.shape)} implies {width}")
    N = width
    if max_k is not None and K > max_k:
        raise ValueError(f"{who}: K = {K} exceeds {max_k}, the bound that keeps the int32 sums exact")
    if groupsize > 0:
        if groupsize % 32 or K % groupsize:
            raise ValueError(f"{who}: groupsize must be a multiple of 32 that divides K")
        want = (K // groupsize, N)
        if scales is not None and (tuple(scales.shape) != want or tuple(zeros.shape) != want):
            raise ValueError(f"{who}: grouped scales / zeros must be {want}")
    elif scales is not None and (scales.numel() != N or zeros.numel() != N):
        raise ValueError(f"{who}: per-row scales / zeros must hold {N} values")
    if bias is not None and bias.numel() != N:
        raise ValueError(f"{who}: bias must hold {N} values")
    if perm is not None:
        if groupsize <= 0:
            raise ValueError(f"{who}: perm (the act-order format) needs grouped grids")
        perm = check_perm(perm, K, ref, who)
    return K, N, bits, groupsize, perm


def _on_gpu(*named):
    for name, t in named:
        if t is not None and not t.is_cuda:
            _lib.require_gpu(t, name)


def _rows(t, width):
    """t [..., width] as the kernels read a matrix: (a [rows, width] view, its leading dimension).  Row-padded inputs
    go as they are; a copy is made only where the elements of a row are not adjacent or rows overlap (expanded
    gradients, e.g. of sum(), have stride 0)."""
    t2 = t.reshape(-1, width)
    if t2.stride(-1) != 1 or (t2.shape[0] > 1 and t2.stride(0) < width):
        t2 = t2.contiguous()
    return t2, max(t2.stride(0), width)


def _f32(t):
    """A grid or bias tensor as the kernels read it: fp32, contiguous (None stays None)."""
    if t is None or (t.dtype is torch.float32 and t.is_contiguous()):
        return t
    return t.to(torch.float32).contiguous()


def _launch(symbol, dev, *args, ws_dims=None, ws_symbol=None):
    """One library call on `dev`'s current stream.  `args`: the symbol's arguments in order, tensors (or None) standing
    for their device pointers -- they stay alive until the call is enqueued.  With `ws_dims` (M, K, N, bits, groupsize) the
    workspace `<ws_symbol or symbol>_workspace_bytes` asks for is allocated and passed with its size, then the stream."""
    tail = ()
    if ws_dims is not None:
        nbytes = getattr(_lib.load(), (ws_symbol or symbol) + "_workspace_bytes")(*ws_dims)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        tail = (_lib.ptr(ws), nbytes)
    with torch.cuda.device(dev):
        _lib.call(symbol, *[a if type(a) is int else _lib.ptr(a) for a in args], *tail, _lib.stream(dev))
