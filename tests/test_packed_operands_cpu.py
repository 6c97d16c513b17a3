"""The host side of the packed matmul wrappers without a GPU: the one operand check behind `quant_matmul`,
`quant_matmul_a8` (tensor and pair form), `quant_matmul_t` and `quant_grid_grad` refuses every malformed call with a
`ValueError` that names the wrapper, before anything needs a device; the five packed modules keep their `state_dict`
keys and their bases; and the 2-D view rule copies exactly the inputs the kernels cannot read in place."""
import pytest
import torch

import gptq_amd
from gptq_amd import _lib
from gptq_amd.quant import A8_MAX_K, _packed_modules, _QuantLinearBase, _rows

K, N, M, BITS = 64, 40, 3, 4


def operands(K=K, groupsize=-1):
    """Valid host operands: per-row grids, or [K/groupsize, N] ones."""
    shape = (K // groupsize, N) if groupsize > 0 else (N,)
    return dict(x=torch.zeros(M, K, dtype=torch.float16), grad=torch.zeros(M, N, dtype=torch.float16),
                qweight=torch.zeros(K // 32 * BITS, N, dtype=torch.int32), scales=torch.ones(shape),
                zeros=torch.zeros(shape), bits=BITS, groupsize=groupsize, bias=torch.zeros(N), perm=None)


def call_matmul(o):
    return gptq_amd.quant_matmul(o["x"], o["qweight"], o["scales"], o["zeros"], o["bits"], o["groupsize"], o["bias"],
                                 perm=o["perm"])


def call_a8(o):
    return gptq_amd.quant_matmul_a8(o["x"], o["qweight"], o["scales"], o["zeros"], o["bits"], o["groupsize"], o["bias"],
                                    perm=o["perm"])


def call_a8_pair(o):
    pair = (o["x"].to(torch.int8), torch.ones(o["x"].shape[:-1]))
    return gptq_amd.quant_matmul_a8(pair, o["qweight"], o["scales"], o["zeros"], o["bits"], o["groupsize"], o["bias"],
                                    perm=o["perm"])


def call_t(o):
    return gptq_amd.quant_matmul_t(o["grad"], o["qweight"], o["scales"], o["zeros"], o["bits"], o["groupsize"],
                                   perm=o["perm"])


def call_grid_grad(o):
    return gptq_amd.quant_grid_grad(o["x"], o["grad"], o["qweight"], o["bits"], o["groupsize"], o["perm"])


WRAPPERS = {"quant_matmul": call_matmul, "quant_matmul_a8": call_a8, "quant_matmul_a8/pair": call_a8_pair,
            "quant_matmul_t": call_t, "quant_grid_grad": call_grid_grad}
TAKES_X = ("quant_matmul", "quant_matmul_a8", "quant_matmul_a8/pair", "quant_grid_grad")
TAKES_GRAD = ("quant_matmul_t", "quant_grid_grad")
TAKES_GRIDS = ("quant_matmul", "quant_matmul_a8", "quant_matmul_a8/pair", "quant_matmul_t")
TAKES_BIAS = ("quant_matmul", "quant_matmul_a8", "quant_matmul_a8/pair")
PAIR_PERM = "perm belongs to the activation quantization"     # the pair form refuses every perm with this text


def defects(name):
    """(id, operands with one defect, fragment of the message) for one wrapper."""
    out = [("bits", dict(operands(), bits=5), "bits must be")]
    other = torch.zeros(K // 32 * 3, N, dtype=torch.int32)                  # the height of a 3-bit buffer
    out.append(("qweight-height", dict(operands(), qweight=other),
                "input features" if name in TAKES_X else r"is no \[K/32\*4, N\] buffer"))
    if name in TAKES_X:
        out.append(("K-mismatch", dict(operands(), x=torch.zeros(M, K + 32, dtype=torch.float16)), "input features"))
    if name in TAKES_GRAD:
        out.append(("N-mismatch", dict(operands(), grad=torch.zeros(M, N + 8, dtype=torch.float16)), "output features"))
    out.append(("groupsize-48", dict(operands(), groupsize=48), "groupsize must be a multiple of 32 that divides K"))
    if name in TAKES_GRIDS:
        wrong = torch.zeros(K // 32 + 1, N)
        out.append(("grouped-grids", dict(operands(groupsize=32), scales=wrong, zeros=wrong),
                    r"grouped scales / zeros must be \(2, 40\)"))
        out.append(("per-row-grids", dict(operands(), scales=torch.ones(N + 1), zeros=torch.zeros(N + 1)),
                    "per-row scales / zeros must hold 40 values"))
    if name in TAKES_BIAS:
        out.append(("bias", dict(operands(), bias=torch.zeros(N + 1)), "bias must hold 40 values"))
    pair = name == "quant_matmul_a8/pair"
    perm = torch.arange(K, dtype=torch.int32)
    out.append(("perm-per-row", dict(operands(), perm=perm), PAIR_PERM if pair else "perm .* needs grouped grids"))
    out.append(("perm-int64", dict(operands(groupsize=32), perm=perm.long()), PAIR_PERM if pair else "perm must be int32"))
    out.append(("perm-length", dict(operands(groupsize=32), perm=perm[:-1]),
                PAIR_PERM if pair else "perm must hold 64 entries"))
    if name.startswith("quant_matmul_a8"):
        out.append(("K-above-bound", operands(K=A8_MAX_K + 32), f"exceeds {A8_MAX_K}"))
    return out


CASES = [pytest.param(name, o, fragment, id=f"{name}-{what}") for name in WRAPPERS for what, o, fragment in defects(name)]


@pytest.mark.parametrize("name,o,fragment", CASES)
def test_one_defect_is_a_value_error_naming_the_wrapper(name, o, fragment):
    who = name.split("/")[0]
    with pytest.raises(ValueError, match=f"^{who}: .*{fragment}"):
        WRAPPERS[name](o)


@pytest.mark.parametrize("name", WRAPPERS)
@pytest.mark.parametrize("groupsize,act_order", [(-1, False), (32, False), (32, True)])
def test_valid_host_operands_pass_the_checks_and_then_need_the_gpu(name, groupsize, act_order):
    o = operands(groupsize=groupsize)
    if act_order and name != "quant_matmul_a8/pair":
        o["perm"] = torch.arange(K, dtype=torch.int32)
    with pytest.raises(_lib.GptqHipError, match="must live on an MI355X device"):
        WRAPPERS[name](o)


PER_ROW_KEYS = ["zeros", "scales", "bias", "qweight"]
GROUPED_KEYS = ["qweight", "scales", "zeros", "bias"]


def test_state_dict_keys_bases_and_module_lookup():
    per_row = [gptq_amd.Quant2Linear(K, N), gptq_amd.Quant3Linear(K, N), gptq_amd.Quant4Linear(K, N),
               gptq_amd.Quant8Linear(K, N)]
    grouped = [gptq_amd.QuantGroupLinear(BITS, 32, K, N), gptq_amd.QuantGroupLinear(3, 32, K, N, act_order=True)]
    for m in per_row:
        assert list(m.state_dict()) == PER_ROW_KEYS and isinstance(m, _QuantLinearBase)
        assert tuple(m.qweight.shape) == (K // 32 * m.bits, N) and m.qweight.dtype == torch.int32
        assert tuple(m.scales.shape) == tuple(m.zeros.shape) == (N, 1) and tuple(m.bias.shape) == (N,)
        assert m.faster is False and m.multi_token is False and m.act_bits is None
    assert list(grouped[0].state_dict()) == GROUPED_KEYS
    assert list(grouped[1].state_dict()) == GROUPED_KEYS + ["perm"]
    for m in grouped:
        assert not isinstance(m, _QuantLinearBase)
        assert tuple(m.scales.shape) == tuple(m.zeros.shape) == (K // 32, N) and m.groupsize == 32
        assert m.multi_token is False and m.act_bits is None
    assert grouped[1].act_order and grouped[1].perm.dtype == torch.int32 and not grouped[0].act_order
    model = torch.nn.Sequential(*per_row, torch.nn.Linear(N, N), torch.nn.Sequential(*grouped))
    assert _packed_modules(model) == per_row + grouped
    assert _packed_modules(model, named=True) == [(str(i), m) for i, m in enumerate(per_row)] + [
        (f"5.{i}", m) for i, m in enumerate(grouped)]
    assert gptq_amd.set_multi_token(model) == 6 and all(m.multi_token for m in per_row + grouped)
    assert gptq_amd.packed_wbits(model) == {"0": 2, "1": 3, "2": 4, "3": 8, "5.0": 4, "5.1": 3}


def test_rows_copies_only_what_the_kernels_cannot_read_in_place():
    base = torch.arange(M * (K + 8), dtype=torch.float16).reshape(M, K + 8)
    padded = base[:, :K]
    t2, ld = _rows(padded, K)
    assert t2.data_ptr() == padded.data_ptr() and ld == padded.stride(0) == K + 8      # row-padded: no copy
    plain = torch.zeros(2, M, K)
    t2, ld = _rows(plain, K)
    assert t2.data_ptr() == plain.data_ptr() and tuple(t2.shape) == (2 * M, K) and ld == K
    one = base[1:2, :K]                                                              # one row: any stride(0) is fine
    t2, ld = _rows(one, K)
    assert t2.data_ptr() == one.data_ptr() and ld >= K
    transposed = torch.arange(K * M, dtype=torch.float16).reshape(K, M).t()            # stride(-1) != 1
    expanded = torch.arange(K, dtype=torch.float16).reshape(1, K).expand(M, K)         # stride(0) == 0
    for t in (transposed, expanded):
        t2, ld = _rows(t, K)
        assert t2.is_contiguous() and ld == K and t2.data_ptr() != t.data_ptr() and torch.equal(t2, t)
