"""gptq_amd -- MI355X-native GPTQ hot path (Hessian, damped inverse factor, column loop, pack, dequant mat-vec).

Importing the package does not touch the GPU or load libgptq_hip.so; the first kernel
call does, and fails loudly if the library was not built (`python -m gptq_amd.build`).
"""
from .gptq import GPTQ, fasterquant_many, flush_pending  # noqa: F401
from .modelutils import DEV, find_layers  # noqa: F401
from .quant import (Quant2Linear, Quant3Linear, Quant4Linear, Quant8Linear, QuantGroupLinear,  # noqa: F401
                    Quantizer, frozen_grids, make_quant2, make_quant3, make_quant4, make_quant8, pack_codes,
                    pack_grouped, quant_grid_grad, quant_matmul, quant_matmul_a8, quant_matmul_t, quantize,
                    quantize_activations, set_act_bits, set_multi_token, trainable_grids)
from .interop import (export_gptq_state_dict, from_gptq_tensors, gptq_checkpoint_keys, load_gptq_checkpoint,  # noqa: F401
                      load_gptq_state_dict, repack_rows, save_gptq_checkpoint, to_gptq_tensors)

from .sequential import QuantArgs, check_wbits, packed_wbits, wbits_for  # noqa: F401

__version__ = "0.1.0"
