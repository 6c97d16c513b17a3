"""Packed dequant GEMM (gptq_amd.quant_matmul) against dense fp16 torch.nn.functional.linear on the Llama-7B Linears.

    python tools/bench_qgemm.py [--iters 30] [--json out.json]

Shapes 4096->4096, 4096->11008, 11008->4096; M in {2, 8, 16, 64, 256, 2048}; 3-bit per-row and 4-bit g128 grids.  The
two are timed alternately in one process with device events after a warm-up, each as a graph of 20 back-to-back
calls (per-call host launch cost would otherwise set a ~20 us floor on both); reported: median time, TFLOP/s, GB/s of
the packed weight bytes, and the share of the roof that bounds the case (2.5 PF fp16 MFMA, 8 TB/s HBM; the bytes
counted are weights + activations + output)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FLOPS, PEAK_BW = 2.5e15, 8e12
SHAPES = [(4096, 4096), (4096, 11008), (11008, 4096)]
MS = [2, 8, 16, 64, 256, 2048]
GRIDS = [(3, -1), (4, 128)]


def graphed(fn, reps):
    """`reps` back-to-back calls of fn captured in one graph: replays time the kernels, not the host launch path."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    return g


def timed(g, reps, rounds):
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from gptq_amd.build import ensure_built
    ensure_built()
    import gptq_amd
    from gptq_amd import _lib
    from gptq_amd.quant import pack_codes
    lib = _lib.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for K, N in SHAPES:
        Wd = (torch.randn(N, K, device=dev, generator=gen) * 0.02).half()
        for bits, gs in GRIDS:
            codes = torch.randint(0, 2 ** bits, (N, K), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
            qw = pack_codes(codes, bits)
            ng = K // gs if gs > 0 else 1
            s = torch.rand(ng, N, device=dev, generator=gen) * 0.01 + 1e-3
            z = s * 2 ** (bits - 1)
            if gs <= 0:
                s, z = s[0].contiguous(), z[0].contiguous()
            packed_bytes = qw.numel() * 4 + 2 * s.numel() * 4
            for M in MS:
                x = torch.randn(M, K, device=dev, generator=gen).half()
                # preallocated outputs / workspace and the C entry point: the kernels, not the wrapper, are timed
                # (gptq_amd.quant_matmul adds its host-side checks and allocations to every call)
                y = torch.empty(M, N, device=dev, dtype=torch.float16)
                yd = torch.empty(M, N, device=dev, dtype=torch.float16)
                nb = lib.gptq_quant_gemm_workspace_bytes(M, K, N, bits, gs)
                ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
                sp, zp = s.contiguous(), z.contiguous()
                q = lambda: _lib.call("gptq_quant_gemm", x.data_ptr(), _lib.F16, K, M, qw.data_ptr(), sp.data_ptr(),  # noqa: E731
                                      zp.data_ptr(), None, K, N, bits, gs, y.data_ptr(), _lib.F16, N, ws.data_ptr(), nb,
                                      _lib.stream(dev))
                d = lambda: torch.matmul(x, Wd.t(), out=yd)                        # noqa: E731
                ref = gptq_amd.quant_matmul(x, qw, s, z, bits, gs)
                q()
                assert torch.equal(y, ref)
                reps = 20
                gq, gd = graphed(q, reps), graphed(d, reps)
                for _ in range(args.warmup):
                    gq.replay(); gd.replay()
                tq, td = [], []
                for _ in range(args.iters):                                          # alternate the two
                    tq += timed(gq, reps, 1)
                    td += timed(gd, reps, 1)
                t_q, t_d = statistics.median(tq), statistics.median(td)
                flops = 2.0 * M * K * N
                io = M * K * 2 + M * N * 2
                floor_c, floor_m = flops / PEAK_FLOPS, (packed_bytes + io) / PEAK_BW
                bound = "mfma" if floor_c >= floor_m else "hbm"
                r = dict(K=K, N=N, M=M, bits=bits, groupsize=gs, qgemm_us=t_q * 1e6, dense_fp16_us=t_d * 1e6,
                         ratio=t_q / t_d, tflops=flops / t_q / 1e12, packed_gbs=packed_bytes / t_q / 1e9, bound=bound,
                         roof_share=max(floor_c, floor_m) / t_q,
                         dense_roof_share=max(floor_c, (K * N * 2 + io) / PEAK_BW) / t_d)
                rows.append(r)
                print(f"{K:>5}->{N:<5} {bits}b g{gs:<4} M={M:<5} qgemm {r['qgemm_us']:8.1f} us  dense {r['dense_fp16_us']:8.1f} us"
                      f"  ratio {r['ratio']:5.2f}  {r['tflops']:7.1f} TF/s  {r['packed_gbs']:7.0f} GB/s packed"
                      f"  {100 * r['roof_share']:5.1f}% of {bound} roof", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
