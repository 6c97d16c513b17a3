"""A data-parallel solve at 2 bits: 2 ranks on one card exchange PACKED rows (gptq_amd.parallel.fasterquant_sharded needs
pack_codes and dequant_packed of the width) and must end with the single-process result.  The ranks are child processes
of this file (`--worker`), each under its own timeout."""
import os
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = 2


def _case():
    gen = torch.Generator().manual_seed(13)
    R, C = 130, 256
    W = (torch.randn(R, C, generator=gen) * 0.02).half().float()
    X = torch.randn(2 * C, C, generator=gen) * (1 + torch.arange(C) % 5)
    return W, ((X.t() @ X) * (2.0 / X.shape[0])).float()


def _solver(dev, nsamples):
    import gptq_amd
    import gptq_amd.gptq as gmod
    gmod.VERBOSE = False
    W, H = _case()
    lin = torch.nn.Linear(W.shape[1], W.shape[0], bias=False, device=dev, dtype=torch.float16)
    lin.weight.data = W.half().to(dev)
    gp = gptq_amd.GPTQ(lin)
    gp.quantizer = gptq_amd.Quantizer()
    gp.quantizer.configure(BITS, perchannel=True, sym=False, mse=False)
    gp.H = H.clone().to(dev)
    gp.nsamples = nsamples
    return lin, gp


def _worker(rank, port, out_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)        # both ranks share the one card
    try:
        from gptq_amd import parallel as par
        lin, gp = _solver(torch.device("cuda:0"), 1)                # two ranks x the same H: the all-reduced mean IS H
        (qw, stab, ztab), = par.fasterquant_sharded([gp], bits=BITS, actorder=True)
        torch.cuda.synchronize()
        torch.save({"w": lin.weight.data.cpu(), "error": gp.error, "perm": gp.perm.cpu(), "qw": qw.cpu(),
                    "scale": stab.cpu(), "zero": ztab.cpu()}, f"{out_path}.{rank}")
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_at_2_bits_match_single_process(hip_device, tmp_path):
    import gptq_amd
    lin, gp = _solver(hip_device, 2)
    gp.fasterquant(blocksize=128, percdamp=0.01, actorder=True)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "shard2.pt")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    procs = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "--worker",
                               str(rank), str(port), out], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for rank in range(2)]
    logs = [p.communicate()[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(f"rank {i} exit {p.returncode}:\n{l[-3000:]}"
                                                             for i, (p, l) in enumerate(zip(procs, logs)))
    want_qw = gptq_amd.pack_codes(gp.codes, BITS).cpu()
    assert want_qw.shape == (256 // 32 * BITS, 130)
    for rank in range(2):
        got = torch.load(f"{out}.{rank}", weights_only=True)
        assert torch.equal(got["perm"], gp.perm.cpu())
        assert torch.equal(got["qw"], want_qw), f"rank {rank}: packed rows differ"
        assert torch.equal(got["w"], lin.weight.data.cpu()), f"rank {rank}: rebuilt weights differ"
        assert abs(got["error"] - gp.error) <= 1e-6 * abs(gp.error)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--worker":
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        _worker(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    else:
        raise SystemExit("usage: test_gpu_packed_wide_sharded.py --worker RANK PORT OUT")
