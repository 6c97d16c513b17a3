#!/usr/bin/env python3
"""Time of the GPTQ-checkpoint conversion kernels on one Linear (default: Llama-7B down_proj, 11008 -> 4096, 4-bit,
groups of 128, act-order with a random permutation).

    python tools/bench_interop.py [--in 11008 --out 4096 --bits 4 --groupsize 128 --iters 200]

Reports microseconds per call of `repack_rows` (device events round `iters` calls, after a warm-up) next to the bytes the
conversion has to move -- the packed words read once and written once -- over the MI355X's 8 TB/s, and the same for the
zero-point tables.  `repack_rows` fetches every source word once per code it holds (32 / bits times), from L2 after the
first; the yardstick counts it once.  An observation for DESIGN.md, not a bar.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gptq_amd
from gptq_amd import interop

PEAK = 8000.0   # GB/s


def timeit(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--in", dest="n_in", type=int, default=11008)
    ap.add_argument("--out", dest="n_out", type=int, default=4096)
    ap.add_argument("--bits", type=int, choices=(2, 3, 4, 8), default=4)
    ap.add_argument("--groupsize", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    K, N, G = a.n_in, a.n_out, a.n_in // a.groupsize
    codes = torch.randint(0, 2 ** a.bits, (N, K), device=dev, generator=gen, dtype=torch.uint8)
    qw = gptq_amd.pack_codes(codes, a.bits)
    perm = torch.randperm(K, device=dev, generator=gen).to(torch.int32)
    out = torch.empty_like(qw)
    res = {"in": K, "out": N, "bits": a.bits, "groupsize": a.groupsize}
    for tag, src in (("random_perm", perm), ("identity", torch.arange(K, device=dev, dtype=torch.int32))):
        t = timeit(lambda: gptq_amd.repack_rows(qw, src, a.bits, out=out), a.iters)
        nbytes = 2 * qw.numel() * 4
        res[f"repack_rows_{tag}"] = {"us": round(t, 2), "bytes": nbytes, "GBps": round(nbytes / t / 1e3, 1),
                                     "us_at_8TBps": round(nbytes / PEAK / 1e3, 2)}
    scales = torch.rand(G, N, device=dev, generator=gen) * 0.01 + 1e-3
    zeros = torch.randint(1, 2 ** a.bits, (G, N), device=dev, generator=gen).float() * scales
    t = timeit(lambda: interop._qzeros_pack(scales, zeros, a.bits, 1), a.iters)      # (includes reading the flags back)
    nbytes = G * N * (4 + 4 + 2) + G * N // 32 * a.bits * 4
    res["qzeros_pack_with_flag_readback"] = {"us": round(t, 2), "bytes": nbytes, "us_at_8TBps": round(nbytes / PEAK / 1e3, 3)}
    qz, s16, _ = interop._qzeros_pack(scales, zeros, a.bits, 1)
    t = timeit(lambda: interop._qzeros_unpack(qz, s16, a.bits, 1), a.iters)
    res["qzeros_unpack"] = {"us": round(t, 2), "bytes": nbytes, "us_at_8TBps": round(nbytes / PEAK / 1e3, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
