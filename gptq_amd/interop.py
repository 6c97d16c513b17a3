"""Checkpoints of other GPTQ tools: the `qweight` / `qzeros` / `scales` / `g_idx` layout that AutoGPTQ, GPTQ-for-LLaMa,
GPTQModel and the `gptq` loaders of transformers and vLLM read and write ("Checkpoints of other GPTQ
tools"; the format is spelled out in include/gptq_hip.h).

The bit layout of `qweight` is the packed Linears' own.  Three things differ and are converted on the GPU
(csrc/interop.hip): the order of the code rows (original column order + `g_idx` there, permuted order + `perm` here),
the zero points (integers bit-packed along N, minus one in the classic format, against fp32 zero*scale) and the scales
(fp16 against fp32).  Like `pack`, the conversions stage host tensors on the GPU; without one they raise `GptqHipError`.
"""
from __future__ import annotations

import json
import os

import torch
import torch.nn as nn

from . import _lib
from .quant import PACKED_LINEAR, QuantGroupLinear, _check_bits, _packed_modules, _QuantLinearBase, check_perm

CHECKPOINT_FORMATS = {"gptq": 1, "gptq_v2": 0}          # -> zero_offset: stored value = zero point - zero_offset
FLAG_OFF_GRID, FLAG_ZERO_RANGE, FLAG_SCALE_F16, FLAG_SCALE_INEXACT, FLAG_ASYM = 1, 2, 4, 8, 16
OWN_KEYS = ("qweight", "scales", "zeros", "bias", "perm")
FOREIGN_KEYS = ("qweight", "qzeros", "scales", "g_idx", "bias")
WEIGHTS_NAME, CONFIG_NAME = "model.safetensors", "quantize_config.json"


def _zero_offset(checkpoint_format, who):
    try:
        return CHECKPOINT_FORMATS[checkpoint_format]
    except (KeyError, TypeError):
        raise ValueError(f"{who}: checkpoint_format must be 'gptq' or 'gptq_v2', got {checkpoint_format!r}") from None


def _stage(home):
    """The GPU a conversion of tensors living on `home` runs on."""
    if home.type == "cuda":
        return home
    if not torch.cuda.is_available():
        raise _lib.GptqHipError("converting GPTQ checkpoints needs an MI355X device; gptq_amd has no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def repack_rows(qweight, row_src, bits, out=None):
    """int32 [K/32*bits, N] -> the same buffer with code row j taken from code row row_src[j] (gptq_repack_rows).
    `row_src` is an int32 permutation [K] on qweight's device; its VALUES are the caller's to validate (an entry outside
    0..K-1 packs code 0).  Returns a new tensor, or `out` (contiguous int32 of qweight's shape, no memory shared with
    qweight: the rows move between positions)."""
    bits = _check_bits(bits, "repack_rows")
    if qweight.dtype != torch.int32 or qweight.dim() != 2 or qweight.shape[0] == 0 or qweight.shape[0] % bits:
        raise ValueError(f"repack_rows: qweight must be int32 [K/32*{bits}, N]")
    K, N = qweight.shape[0] // bits * 32, qweight.shape[1]
    row_src = check_perm(row_src, K, qweight, "repack_rows")
    qw = qweight.contiguous()
    if out is None:
        out = torch.empty_like(qw)
    else:
        if out.shape != qw.shape or out.dtype != torch.int32 or not out.is_contiguous() or out.device != qw.device:
            raise ValueError("repack_rows: out must be a contiguous int32 tensor of qweight's shape on its device")
        nbytes = qw.numel() * 4
        if out.data_ptr() < qw.data_ptr() + nbytes and qw.data_ptr() < out.data_ptr() + nbytes:
            raise ValueError("repack_rows: out must not alias qweight (the rows move between positions)")
    _lib.require_gpu(qw, "qweight")
    dev = qw.device
    with torch.cuda.device(dev):
        _lib.call("gptq_repack_rows", _lib.ptr(qw), _lib.ptr(row_src), K, N, bits, _lib.ptr(out), _lib.stream(dev))
    return out


def _as_perm(perm, K, who):
    """perm checked as a permutation of 0..K-1 (ValueError otherwise) -> (perm, inverse), both int32."""
    p = perm.long()
    if p.numel() != K or int(p.min()) < 0 or int(p.max()) >= K or int(torch.bincount(p, minlength=K).max()) != 1:
        raise ValueError(f"{who}: perm is not a permutation of 0..{K - 1}")
    inv = torch.empty_like(p)
    inv[p] = torch.arange(K, device=p.device)
    return perm.to(torch.int32), inv.to(torch.int32)


def _qzeros_pack(scales, zeros, bits, zero_offset):
    """fp32 [G, N] tables (zeros = zero*scale) on the GPU -> (qzeros int32 [G, N/32*bits], scales fp16 [G, N], flags)."""
    G, N = scales.shape
    dev = scales.device
    s = scales.to(torch.float32).contiguous()
    z = zeros.to(torch.float32).contiguous()
    qzeros = torch.empty((G, N // 32 * bits), dtype=torch.int32, device=dev)
    s16 = torch.empty((G, N), dtype=torch.float16, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("gptq_qzeros_pack", _lib.ptr(s), _lib.ptr(z), G, N, bits, zero_offset, _lib.ptr(qzeros), _lib.ptr(s16),
                  _lib.ptr(flags), _lib.stream(dev))
    return qzeros, s16, int(flags.item())


def _qzeros_unpack(qzeros, scales16, bits, zero_offset):
    """The inverse of `_qzeros_pack`: (scales, zeros) fp32 [G, N]."""
    G, N = scales16.shape
    dev = scales16.device
    qz, s16 = qzeros.contiguous(), scales16.contiguous()
    scales = torch.empty((G, N), dtype=torch.float32, device=dev)
    zeros = torch.empty((G, N), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("gptq_qzeros_unpack", _lib.ptr(qz), _lib.ptr(s16), G, N, bits, zero_offset, _lib.ptr(scales),
                  _lib.ptr(zeros), _lib.stream(dev))
    return scales, zeros


def _describe(module, who):
    """(bits, group_size, act_order) of one packed module; group_size -1 for the per-row modules."""
    if isinstance(module, QuantGroupLinear):
        return int(module.bits), int(module.groupsize), bool(module.act_order)
    if isinstance(module, _QuantLinearBase):
        return int(module.bits), -1, False
    raise ValueError(f"{who}: {type(module).__name__} is not a packed Linear")


def _export_module(module, checkpoint_format, strict, who):
    zero_offset = _zero_offset(checkpoint_format, who)
    bits, group_size, act_order = _describe(module, who)
    qweight = module.qweight
    K, N = qweight.shape[0] // bits * 32, qweight.shape[1]
    if N % 32:
        raise ValueError(f"{who}: out_features = {N} is not a multiple of 32; the zero points of the format are packed "
                         "32 columns at a time (qzeros [G, N/32*bits])")
    home = qweight.device
    dev = _stage(home)
    G = K // group_size if group_size > 0 else 1
    scales = module.scales.detach().to(dev).reshape(G, N)           # (the per-row modules keep [N, 1])
    zeros = module.zeros.detach().to(dev).reshape(G, N)
    qzeros, scales16, flags = _qzeros_pack(scales, zeros, bits, zero_offset)
    if flags & FLAG_SCALE_F16:
        raise ValueError(f"{who}: a scale becomes 0, inf or nan in fp16, the format's scale type")
    if flags & FLAG_OFF_GRID:
        raise ValueError(f"{who}: the grid is off the integer lattice: zeros is no longer an integer zero point times "
                         "scales (e.g. after training with trainable_grids), and the format stores integer zero points")
    if flags & FLAG_ZERO_RANGE:
        hint = ("; the classic 'gptq' format stores zero point - 1 and cannot hold a zero point of 0: export with "
                "checkpoint_format='gptq_v2'") if zero_offset else ""
        raise ValueError(f"{who}: a zero point lies outside [{zero_offset}, {2 ** bits - 1}]{hint}")
    if strict and flags & FLAG_SCALE_INEXACT:
        raise ValueError(f"{who}: strict=True and a scale is not exactly representable in fp16 (the checkpoint would hold "
                         "rounded scales)")
    if act_order:
        inv = _as_perm(module.perm.to(dev), K, who)[1]
        qw = repack_rows(qweight.to(dev), inv, bits)
    else:
        qw = qweight.to(dev).contiguous().clone()
    g_idx = module.g_idx.to(dev) if group_size > 0 else torch.zeros(K, dtype=torch.int32, device=dev)
    out = {"qweight": qw, "qzeros": qzeros, "scales": scales16, "g_idx": g_idx}
    bias = module.bias.detach()
    if bool((bias != 0).any()):
        out["bias"] = bias.to(dev).to(torch.float16)
    return {k: v.to(home) for k, v in out.items()}, flags


def to_gptq_tensors(module, checkpoint_format="gptq", strict=False):
    """One packed module -> {'qweight', 'qzeros', 'scales', 'g_idx'[, 'bias']} in the other tools' layout, on the
    module's device.  Per-row modules export as group_size -1 (scales [1, N], g_idx all zero); act-order modules get their
    code rows moved back to original column order.  `bias` is present iff it has a non-zero entry.

    Raises ValueError where the format cannot hold the module: a grid that is no longer integer (after
    `trainable_grids` training), a zero point outside the storable range (0 under 'gptq': use 'gptq_v2'), a scale that is
    0 / inf / nan in fp16, out_features % 32 != 0, and with strict=True any scale that fp16 would round."""
    return _export_module(module, checkpoint_format, strict, "to_gptq_tensors")[0]


def from_gptq_tensors(tensors, bits, group_size, checkpoint_format="gptq", multi_token=False, device=None):
    """{'qweight', 'qzeros', 'scales'[, 'g_idx'][, 'bias']} -> a packed module on `device` (default: qweight's device).
    group_size -1 gives the per-row module of the width; a `g_idx` that is absent or k // group_size a
    `QuantGroupLinear`; any other `g_idx` an act-order one with perm = argsort(g_idx, stable).  Under 'gptq' the zero
    point is the stored value + 1 without masking.  Everything is validated (ValueError) before the first launch."""
    who = "from_gptq_tensors"
    zero_offset = _zero_offset(checkpoint_format, who)
    bits, group_size = _check_bits(bits, who), int(group_size)
    for key in ("qweight", "qzeros", "scales"):
        if key not in tensors:
            raise ValueError(f"{who}: tensors lacks {key!r}")
    unknown = set(tensors) - set(FOREIGN_KEYS)
    if unknown:
        raise ValueError(f"{who}: unknown entries {sorted(unknown)}")
    qweight, qzeros, scales = tensors["qweight"], tensors["qzeros"], tensors["scales"]
    g_idx, bias = tensors.get("g_idx"), tensors.get("bias")
    for name, t, dt in (("qweight", qweight, torch.int32), ("qzeros", qzeros, torch.int32), ("scales", scales, torch.float16)):
        if t.dtype != dt:
            raise ValueError(f"{who}: {name} must be {dt}, got {t.dtype}")
    if qweight.dim() != 2 or qweight.shape[0] == 0 or qweight.shape[0] % bits:
        raise ValueError(f"{who}: qweight {tuple(qweight.shape)} is no [K/32*{bits}, N] buffer")
    K, N = qweight.shape[0] // bits * 32, qweight.shape[1]
    if N == 0 or N % 32:
        raise ValueError(f"{who}: out_features = {N} must be a positive multiple of 32")
    if group_size != -1 and (group_size <= 0 or group_size % 32 or K % group_size):
        raise ValueError(f"{who}: group_size must be -1 or a positive multiple of 32 that divides K = {K}, got {group_size}")
    G = K // group_size if group_size > 0 else 1
    if tuple(scales.shape) != (G, N):
        raise ValueError(f"{who}: scales must be {(G, N)}, got {tuple(scales.shape)}")
    if tuple(qzeros.shape) != (G, N // 32 * bits):
        raise ValueError(f"{who}: qzeros must be {(G, N // 32 * bits)}, got {tuple(qzeros.shape)}")
    if bias is not None and (bias.dtype not in (torch.float16, torch.float32) or tuple(bias.shape) != (N,)):
        raise ValueError(f"{who}: bias must be fp16 (or fp32) [{N}], got {bias.dtype} {tuple(bias.shape)}")
    act_order = False
    if g_idx is not None:
        if g_idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{who}: g_idx must be int32 or int64, got {g_idx.dtype}")
        if tuple(g_idx.shape) != (K,):
            raise ValueError(f"{who}: g_idx must hold {K} entries, got shape {tuple(g_idx.shape)}")
        gl = g_idx.long()
        if int(gl.min()) < 0 or int(gl.max()) >= G:
            if group_size == -1:
                raise ValueError(f"{who}: group_size -1 is one group: g_idx must be absent or all zero")
            raise ValueError(f"{who}: g_idx values must lie in [0, {G}), got {int(gl.min())}..{int(gl.max())}")
        if group_size > 0:
            counts = torch.bincount(gl, minlength=G)
            if bool((counts != group_size).any()):
                g = int((counts != group_size).nonzero()[0])
                raise ValueError(f"{who}: every group must hold exactly {group_size} columns; group {g} holds "
                                 f"{int(counts[g])}")
            act_order = not torch.equal(gl, torch.arange(K, device=gl.device) // group_size)
    home = torch.device(device) if device is not None else qweight.device
    dev = _stage(home)
    s, z = _qzeros_unpack(qzeros.to(dev), scales.to(dev), bits, zero_offset)
    qw = qweight.to(dev).contiguous()
    if group_size == -1:
        m = PACKED_LINEAR[bits](K, N, multi_token=multi_token)
        m.scales, m.zeros = s.reshape(N, 1), z.reshape(N, 1)
    else:
        m = QuantGroupLinear(bits, group_size, K, N, multi_token=multi_token, act_order=act_order)
        m.scales, m.zeros = s, z
        if act_order:
            perm = torch.argsort(g_idx.to(dev).long(), stable=True).to(torch.int32)
            qw = repack_rows(qw, perm, bits)
            m.perm = perm
    m.qweight = qw if qw.data_ptr() != qweight.data_ptr() else qw.clone()
    m.bias = bias.to(dev, torch.float32, copy=True) if bias is not None else torch.zeros(N, device=dev)
    return m.to(home)


def _uniform_config(packed, who):
    """(bits, group_size) shared by every packed Linear; ValueError naming two that differ."""
    if not packed:
        raise ValueError(f"{who}: the model holds no packed Linear")
    name0, m0 = packed[0]
    bits, group_size, _ = _describe(m0, who)
    for name, m in packed[1:]:
        b, g, _ = _describe(m, who)
        if (b, g) != (bits, group_size):
            raise ValueError(f"{who}: one quantize_config covers the whole checkpoint, but {name0!r} has bits={bits}, "
                             f"group_size={group_size} and {name!r} has bits={b}, group_size={g} (mixed checkpoints are "
                             "out of scope)")
    return bits, group_size


def gptq_checkpoint_keys(model):
    """The keys `export_gptq_state_dict(model)[0]` has, without converting anything (no GPU needed): under every packed
    Linear's prefix the foreign keys replace the module's own (`bias` only where it has a non-zero entry); every other
    entry keeps its key."""
    packed = dict(_packed_modules(model, named=True))
    own = {f"{p}.{k}" if p else k for p in packed for k in OWN_KEYS}
    keys = [k for k in model.state_dict() if k not in own]
    for p, m in packed.items():
        for k in FOREIGN_KEYS:
            if k != "bias" or bool((m.bias != 0).any()):
                keys.append(f"{p}.{k}" if p else k)
    return keys


def export_gptq_state_dict(model, checkpoint_format="gptq", strict=False):
    """(state_dict, quantize_config) of `model` in the other tools' layout: every packed Linear's keys are replaced by
    `to_gptq_tensors` of it under the same prefix, every other entry passes through untouched.  All packed Linears must
    share bits and group_size (ValueError naming two that do not)."""
    who = "export_gptq_state_dict"
    _zero_offset(checkpoint_format, who)
    packed = _packed_modules(model, named=True)
    bits, group_size = _uniform_config(packed, who)
    own = {f"{p}.{k}" if p else k for p, _ in packed for k in OWN_KEYS}
    sd = {k: v for k, v in model.state_dict().items() if k not in own}
    flags = 0
    for p, m in packed:
        tensors, f = _export_module(m, checkpoint_format, strict, f"{who}({p!r})")
        flags |= f
        for k, v in tensors.items():
            sd[f"{p}.{k}" if p else k] = v
    config = {"bits": bits, "group_size": group_size, "desc_act": any(_describe(m, who)[2] for _, m in packed),
              "static_groups": False, "sym": not flags & FLAG_ASYM, "checkpoint_format": checkpoint_format,
              "quant_method": "gptq", "damp_percent": 0.01, "true_sequential": True}
    return sd, config


def _read_config(quantize_config, who):
    for key in ("bits", "group_size"):
        if key not in quantize_config:
            raise ValueError(f"{who}: quantize_config lacks {key!r}")
    method = quantize_config.get("quant_method", "gptq")
    if method != "gptq":
        raise ValueError(f"{who}: quant_method must be 'gptq', got {method!r}")
    return int(quantize_config["bits"]), int(quantize_config["group_size"]), quantize_config.get("checkpoint_format", "gptq")


def load_gptq_state_dict(model, state_dict, quantize_config, multi_token=False):
    """Load a checkpoint of the other tools' layout into `model`: every `nn.Linear` named p with p + '.qweight' in
    `state_dict` is replaced by `from_gptq_tensors` of its entries (on the Linear's device); the remaining keys go through
    `model.load_state_dict(rest, strict=False)`, whose result is returned (its `missing_keys` without the buffers of the
    modules built here: the checkpoint did supply them)."""
    who = "load_gptq_state_dict"
    bits, group_size, fmt = _read_config(quantize_config, who)
    rest = dict(state_dict)
    built = []
    for name, lin in [(n, m) for n, m in model.named_modules() if isinstance(m, nn.Linear)]:
        if not name or f"{name}.qweight" not in rest:
            continue
        rows, n_out = rest[f"{name}.qweight"].shape[0], rest[f"{name}.qweight"].shape[-1]
        if (rows * 32, n_out) != (lin.in_features * bits, lin.out_features):
            raise ValueError(f"{who}: {name!r} is a {lin.in_features} -> {lin.out_features} Linear, the checkpoint's "
                             f"qweight {tuple(rest[name + '.qweight'].shape)} is not [{lin.in_features}/32*{bits}, "
                             f"{lin.out_features}]")
        tensors = {k: rest.pop(f"{name}.{k}") for k in FOREIGN_KEYS if f"{name}.{k}" in rest}
        m = from_gptq_tensors(tensors, bits, group_size, fmt, multi_token=multi_token, device=lin.weight.device)
        parent_name, _, attr = name.rpartition(".")
        setattr(model.get_submodule(parent_name) if parent_name else model, attr, m)
        built.append(name)
    result = model.load_state_dict(rest, strict=False)
    result.missing_keys[:] = [k for k in result.missing_keys if k.rpartition(".")[0] not in built]
    return result


def _safetensors():
    try:
        import safetensors.torch as st
    except ImportError as e:
        raise ImportError("save_gptq_checkpoint / load_gptq_checkpoint read and write model.safetensors and need the "
                          "`safetensors` package, which cannot be imported here; use export_gptq_state_dict / "
                          "load_gptq_state_dict with a serializer of your own") from e
    return st


def save_gptq_checkpoint(model, directory, checkpoint_format="gptq", strict=False):
    """Write `model` as model.safetensors + quantize_config.json in `directory` (created if missing).  Returns the
    quantize_config."""
    st = _safetensors()
    sd, config = export_gptq_state_dict(model, checkpoint_format, strict)
    os.makedirs(directory, exist_ok=True)
    st.save_file({k: v.detach().cpu().contiguous() for k, v in sd.items()}, os.path.join(directory, WEIGHTS_NAME),
                 metadata={"format": "pt"})
    with open(os.path.join(directory, CONFIG_NAME), "w") as f:
        json.dump(config, f, indent=2)
    return config


def load_gptq_checkpoint(model, directory, multi_token=False):
    """Read model.safetensors + quantize_config.json from `directory` into `model` (`load_gptq_state_dict`)."""
    st = _safetensors()
    with open(os.path.join(directory, CONFIG_NAME)) as f:
        config = json.load(f)
    return load_gptq_state_dict(model, st.load_file(os.path.join(directory, WEIGHTS_NAME)), config, multi_token=multi_token)
