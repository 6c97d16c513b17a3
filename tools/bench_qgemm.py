"""Packed dequant GEMM (gptq_amd.quant_matmul) against dense fp16 torch.nn.functional.linear on the Llama-7B Linears.

    python tools/bench_qgemm.py [--iters 30] [--json out.json] [--perm] [--bits 2 4 8] [--ms 1 16 2048]

Shapes 4096->4096, 4096->11008, 11008->4096; M in {2, 8, 16, 64, 256, 2048}; 3-bit per-row and 4-bit g128 grids.  The
two are timed alternately in one process with device events after a warm-up, each as a graph of 20 back-to-back
calls (per-call host launch cost would otherwise set a ~20 us floor on both); reported: median time, TFLOP/s, GB/s of
the packed weight bytes, and the share of the roof that bounds the case (2.5 PF fp16 MFMA, 8 TB/s HBM; the bytes
counted are weights + activations + output).  --bits: these packed widths (any of 2, 3, 4, 8), all on g128 grids, so
that the widths compare on one grid; --ms: these M instead.

--perm: the act-order format instead (4-bit g128, storage row k = input column perm[k], a random permutation): the
grouped GEMM with perm (gptq_quant_gemm_perm) against the same GEMM without it on the same packed weights, M in
{1, 4, 16, 128, 2048}, plus the grouped mat-vec with and without perm on the FC2 shape 36864 -> 9216.  Which gather the
GEMM used (fused into the X staging, or a pre-pass into the workspace) is read off the workspace query.  With the
diagnostic library (GPTQ_HIP_LIB=gptq_amd/libgptq_hip_diag.so) GPTQ_QG_PERM_FUSED_M moves the switch between the two.

--backward: the transposed dequant GEMM (gptq_quant_gemm_t, dx = dy . Wdeq^T: the backward of the packed Linears) on the
same Linears, 4-bit per-row, 4-bit g128 and 4-bit g128 with perm, M in {1, 16, 2048}, beside the route that needs no
such kernel, in the same process: gptq_dequant_packed(_perm) to a dense fp16 matrix, then torch.matmul(dy, W).  Both
times and their ratio go to profiles/qgemm_backward.json (or --json).

--grid-grad: the grid gradients (gptq_quant_gemm_grid_grad: dscales, dzeros, dbias from x and dy, the codes frozen) on the
same Linears at M = 2048 and M = 16, 4-bit per-row, 4-bit g128, 4-bit g128 with perm and 2-bit g128, beside the dense route
it replaces, in the same process: A = x.t() @ dy in fp32 (a [K, N] tensor), A times the unpacked codes, both summed per
group, and dy summed over the tokens (the codes are unpacked once, outside the timed region).  Reported: both times,
their ratio, the TFLOP/s of 2 M K N over the call and its share of the roof that bounds it, and the peak device memory
each route adds on top of its operands (torch.cuda.max_memory_allocated around one eager call).  Results go to
profiles/qgemm_grid_grad.json (or --json).

--a8: the GEMM on int8 activations (gptq_quant_act_rows + gptq_quant_gemm_a8, the opt-in prefill path) on the same Linears
at M = 16, 256, 2048 for 4-bit g128, 3-bit per-row and 8-bit g128, in one process beside today's gptq_quant_gemm and dense
fp16 torch.matmul.  Five graphs are replayed in turn: the a8 call with the activation quantization included, the a8 GEMM
alone on a pre-quantized (xq, sx), the fp16 dequant GEMM twice (two interleaved series of the same code: their medians'
spread is the A/A noise of the comparison) and the dense product.  Also recorded, without a gate: the relative error of the
a8 output against the fp16 path's on randn activations.  Results go to profiles/qgemm_a8.json (or --json)."""
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


def alternate(fa, fb, reps, warmup, iters):
    """Median seconds per call of fa and fb, graphed and timed alternately."""
    ga, gb = graphed(fa, reps), graphed(fb, reps)
    for _ in range(warmup):
        ga.replay(); gb.replay()
    ta, tb = [], []
    for _ in range(iters):
        ta += timed(ga, reps, 1)
        tb += timed(gb, reps, 1)
    return statistics.median(ta), statistics.median(tb)


PERM_MS = [1, 4, 16, 128, 2048]


def main_perm(args):
    import gptq_amd
    from gptq_amd import _lib
    from gptq_amd.quant import pack_codes
    lib = _lib.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    bits, gs, reps = 4, 128, 20
    rows = []

    def grouped(K, N):
        codes = torch.randint(0, 2 ** bits, (N, K), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
        s = torch.rand(K // gs, N, device=dev, generator=gen) * 0.01 + 1e-3
        perm = torch.randperm(K, device=dev, generator=gen).to(torch.int32)
        return pack_codes(codes, bits), s, s * 2 ** (bits - 1), perm

    for K, N in SHAPES:
        qw, s, z, perm = grouped(K, N)
        for M in PERM_MS:
            x = torch.randn(M, K, device=dev, generator=gen).half()
            y0 = torch.empty(M, N, device=dev, dtype=torch.float16)
            y1 = torch.empty(M, N, device=dev, dtype=torch.float16)
            nb0 = lib.gptq_quant_gemm_workspace_bytes(M, K, N, bits, gs)
            nb1 = lib.gptq_quant_gemm_perm_workspace_bytes(M, K, N, bits, gs)
            ws0 = torch.empty(max(nb0, 1), dtype=torch.uint8, device=dev)
            ws1 = torch.empty(max(nb1, 1), dtype=torch.uint8, device=dev)
            plain = lambda: _lib.call("gptq_quant_gemm", x.data_ptr(), _lib.F16, K, M, qw.data_ptr(), s.data_ptr(),  # noqa: E731
                                      z.data_ptr(), None, K, N, bits, gs, y0.data_ptr(), _lib.F16, N, ws0.data_ptr(), nb0,
                                      _lib.stream(dev))
            withp = lambda: _lib.call("gptq_quant_gemm_perm", x.data_ptr(), _lib.F16, K, M, qw.data_ptr(),  # noqa: E731
                                      s.data_ptr(), z.data_ptr(), perm.data_ptr(), None, K, N, bits, gs, y1.data_ptr(),
                                      _lib.F16, N, ws1.data_ptr(), nb1, _lib.stream(dev))
            withp()
            assert torch.equal(y1, gptq_amd.quant_matmul(x[:, perm.long()].contiguous(), qw, s, z, bits, gs))
            t0, t1 = alternate(plain, withp, reps, args.warmup, args.iters)
            gather = "prepass" if nb1 > nb0 else "fused"
            r = dict(kind="gemm", K=K, N=N, M=M, bits=bits, groupsize=gs, gather=gather, noperm_us=t0 * 1e6,
                     perm_us=t1 * 1e6, ratio=t1 / t0, target=1.10, met=t1 / t0 <= 1.10)
            rows.append(r)
            print(f"gemm {K:>5}->{N:<5} M={M:<5} no perm {r['noperm_us']:8.1f} us  perm ({gather:7}) {r['perm_us']:8.1f} us"
                  f"  ratio {r['ratio']:5.3f}", flush=True)
    K, N = 36864, 9216                                      # FC2 shape of the mat-vec
    from gptq_amd import quant_cuda  # noqa: F401  (the wrapper's checks are not timed: the C entry points are)
    qw, s, z, perm = grouped(K, N)
    for xdt, code in ((torch.float16, _lib.F16), (torch.float32, _lib.F32)):
        x = torch.randn(K, device=dev, generator=gen).to(xdt)
        y = torch.zeros(N, device=dev)
        h = qw.shape[0]
        plain = lambda: _lib.call("gptq_vecquant_matmul_grouped", x.data_ptr(), code, qw.data_ptr(), y.data_ptr(),  # noqa: E731
                                  s.data_ptr(), z.data_ptr(), h, N, bits, gs, _lib.stream(dev))
        withp = lambda: _lib.call("gptq_vecquant_matmul_grouped_perm", x.data_ptr(), code, qw.data_ptr(),  # noqa: E731
                                  y.data_ptr(), s.data_ptr(), z.data_ptr(), perm.data_ptr(), h, N, bits, gs,
                                  _lib.stream(dev))
        t0, t1 = alternate(plain, withp, reps, args.warmup, args.iters)
        r = dict(kind="matvec", K=K, N=N, M=1, bits=bits, groupsize=gs, x_dtype=str(xdt).split(".")[-1],
                 noperm_us=t0 * 1e6, perm_us=t1 * 1e6, ratio=t1 / t0, target=1.10, met=t1 / t0 <= 1.10)
        rows.append(r)
        print(f"matvec {K}->{N} x {r['x_dtype']}: no perm {r['noperm_us']:7.2f} us  perm {r['perm_us']:7.2f} us"
              f"  ratio {r['ratio']:5.3f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "library": _lib.LIB_PATH,
                       "GPTQ_QG_PERM_FUSED_M": os.environ.get("GPTQ_QG_PERM_FUSED_M"), "rows": rows}, f, indent=1)


BWD_MS = [1, 16, 2048]
BWD_GRIDS = [(4, -1, False), (4, 128, False), (4, 128, True)]


def main_backward(args):
    import gptq_amd
    from gptq_amd import _lib
    from gptq_amd.quant import dequant_packed, pack_codes
    lib = _lib.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    reps = 20
    rows = []
    for K, N in SHAPES:
        for bits, gs, with_perm in BWD_GRIDS:
            codes = torch.randint(0, 2 ** bits, (N, K), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
            qw = pack_codes(codes, bits)
            ng = K // gs if gs > 0 else 1
            s = (torch.rand(ng, N, device=dev, generator=gen) * 0.01 + 1e-3).contiguous()
            zint = torch.full_like(s, float(2 ** (bits - 1)))
            z = (s * zint).contiguous()
            perm = torch.randperm(K, device=dev, generator=gen).to(torch.int32) if with_perm else None
            W = torch.empty(N, K, device=dev, dtype=torch.float16)
            for M in (args.ms or BWD_MS):
                dy = (torch.randn(M, N, device=dev, generator=gen) * 0.1).half()
                dx = torch.empty(M, K, device=dev, dtype=torch.float16)
                dxb = torch.empty(M, K, device=dev, dtype=torch.float16)
                nb = lib.gptq_quant_gemm_t_workspace_bytes(M, K, N, bits, gs)
                ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
                kern = lambda: _lib.call("gptq_quant_gemm_t", dy.data_ptr(), _lib.F16, N, M, qw.data_ptr(),  # noqa: E731
                                         s.data_ptr(), z.data_ptr(), _lib.ptr(perm), K, N, bits, gs, dx.data_ptr(), _lib.F16,
                                         K, ws.data_ptr(), nb, _lib.stream(dev))

                def base():
                    if perm is None:
                        _lib.call("gptq_dequant_packed", qw.data_ptr(), s.data_ptr(), zint.data_ptr(), N, K, bits, gs,
                                  W.data_ptr(), _lib.F16, K, _lib.stream(dev))
                    else:
                        _lib.call("gptq_dequant_packed_perm", qw.data_ptr(), s.data_ptr(), zint.data_ptr(), perm.data_ptr(),
                                  N, K, bits, gs, W.data_ptr(), _lib.F16, K, _lib.stream(dev))
                    torch.matmul(dy, W, out=dxb)

                kern()
                base()
                torch.cuda.synchronize()
                assert torch.equal(dx, gptq_amd.quant_matmul_t(dy, qw, s if gs > 0 else s[0], z if gs > 0 else z[0], bits, gs,
                                                               perm=perm))
                assert torch.equal(W, dequant_packed(qw, s, zint, bits, gs, torch.float16, perm=perm))
                diff = float((dx.float() - dxb.float()).abs().max()) / max(float(dxb.float().abs().max()), 1e-30)
                assert diff < 2e-2, diff                                             # the same product, two routes
                t_k, t_b = alternate(kern, base, reps, args.warmup, args.iters)
                r = dict(K=K, N=N, M=M, bits=bits, groupsize=gs, perm=with_perm, qgemm_t_us=t_k * 1e6,
                         dequant_matmul_us=t_b * 1e6, ratio=t_k / t_b, split=nb > 0, max_rel_diff=diff)
                rows.append(r)
                print(f"{K:>5}->{N:<5} {bits}b g{gs:<4}{' perm' if with_perm else '     '} M={M:<5} qgemm_t {r['qgemm_t_us']:9.1f} us"
                      f"  dequant+matmul {r['dequant_matmul_us']:9.1f} us  ratio {r['ratio']:5.2f}", flush=True)
    out = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                    "qgemm_backward.json")
    with open(out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(dev), "reps_per_graph": reps, "iters": args.iters,
                   "warmup": args.warmup, "rows": rows}, f, indent=1)


GRID_MS = [2048, 16]
GRID_GRIDS = [(4, -1, False), (4, 128, False), (4, 128, True), (2, 128, False)]


def peak_extra(fn, dev):
    """Peak device bytes that one eager call of fn allocates on top of what is live before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return peak


def main_grid_grad(args):
    import gptq_amd
    from gptq_amd import _lib
    from gptq_amd.quant import pack_codes
    lib = _lib.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for K, N in SHAPES:
        for bits, gs, with_perm in GRID_GRIDS:
            codes = torch.randint(0, 2 ** bits, (N, K), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
            qw = pack_codes(codes, bits)
            codes_kn = codes.t().contiguous()                                         # [K, N] in storage order, for the dense route
            del codes
            G = K // gs if gs > 0 else 1
            rows_g = gs if gs > 0 else K
            perm = torch.randperm(K, device=dev, generator=gen).to(torch.int32) if with_perm else None
            plong = perm.long() if with_perm else None
            packed_bytes = qw.numel() * 4
            for M in (args.ms or GRID_MS):
                x = torch.randn(M, K, device=dev, generator=gen).half()
                dy = (torch.randn(M, N, device=dev, generator=gen) * 0.1).half()
                ds = torch.empty(G, N, device=dev)
                dz = torch.empty(G, N, device=dev)
                db = torch.empty(N, device=dev)
                query = lib.gptq_quant_gemm_grid_grad_perm_workspace_bytes if with_perm else lib.gptq_quant_gemm_grid_grad_workspace_bytes
                nb = query(M, K, N, bits, gs)
                ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
                kern = lambda: _lib.call("gptq_quant_gemm_grid_grad", x.data_ptr(), _lib.F16, K, dy.data_ptr(), N, M,  # noqa: E731
                                         qw.data_ptr(), _lib.ptr(perm), K, N, bits, gs, ds.data_ptr(), dz.data_ptr(),
                                         db.data_ptr(), ws.data_ptr(), nb, _lib.stream(dev))

                def dense():
                    xs = x[:, plong] if with_perm else x
                    A = torch.matmul(xs.float().t(), dy.float())                      # [K, N] fp32
                    return ((A * codes_kn).view(G, rows_g, N).sum(1), -A.view(G, rows_g, N).sum(1), dy.float().sum(0))

                kern()
                want = dense()
                torch.cuda.synchronize()
                got = gptq_amd.quant_grid_grad(x, dy, qw, bits, gs, perm=perm)
                diff = 0.0
                for a, b, w in zip((ds, dz, db), got, want):
                    assert torch.equal(a.reshape(-1), b.reshape(-1))                  # the wrapper runs the timed call
                    diff = max(diff, float((a.reshape(-1) - w.reshape(-1)).abs().max()) / max(float(w.abs().max()), 1e-30))
                assert diff < 1e-3, diff                                             # the same sums, two routes
                del want, got
                mem_k = peak_extra(lambda: gptq_amd.quant_grid_grad(x, dy, qw, bits, gs, perm=perm), dev)
                mem_d = peak_extra(dense, dev)
                reps = 20 if M <= 256 else 5
                t_k, t_d = alternate(kern, dense, reps, args.warmup, args.iters)
                flops = 2.0 * M * K * N
                floor_c, floor_m = flops / PEAK_FLOPS, (packed_bytes + (M * K + M * N) * 2 + 2 * G * N * 4) / PEAK_BW
                bound = "mfma" if floor_c >= floor_m else "hbm"
                r = dict(K=K, N=N, M=M, bits=bits, groupsize=gs, perm=with_perm, grid_grad_us=t_k * 1e6, dense_us=t_d * 1e6,
                         ratio=t_k / t_d, tflops=flops / t_k / 1e12, bound=bound, roof_share=max(floor_c, floor_m) / t_k,
                         workspace_bytes=nb, grid_grad_peak_bytes=mem_k, dense_peak_bytes=mem_d, max_rel_diff=diff)
                rows.append(r)
                print(f"{K:>5}->{N:<5} {bits}b g{gs:<4}{' perm' if with_perm else '     '} M={M:<5} grid_grad {r['grid_grad_us']:9.1f} us"
                      f"  dense {r['dense_us']:9.1f} us  ratio {r['ratio']:5.2f}  {r['tflops']:6.1f} TF/s {100 * r['roof_share']:5.1f}% of"
                      f" {bound} roof  peak {mem_k / 2 ** 20:7.1f} MiB vs {mem_d / 2 ** 20:7.1f} MiB", flush=True)
                del x, dy, ds, dz, db, ws
            del qw, codes_kn
    out = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                    "qgemm_grid_grad.json")
    with open(out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(dev), "iters": args.iters, "warmup": args.warmup,
                   "reps_per_graph": {"M<=256": 20, "M>256": 5}, "rows": rows}, f, indent=1)


A8_MS = [16, 256, 2048]
A8_GRIDS = [(4, 128), (3, -1), (8, 128)]


def main_a8(args):
    import gptq_amd
    from gptq_amd import _lib
    from gptq_amd.quant import pack_codes
    lib = _lib.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for K, N in SHAPES:
        Wd = (torch.randn(N, K, device=dev, generator=gen) * 0.02).half()
        for bits, gs in A8_GRIDS:
            codes = torch.randint(0, 2 ** bits, (N, K), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
            qw = pack_codes(codes, bits)
            del codes
            ng = K // gs if gs > 0 else 1
            s = (torch.rand(ng, N, device=dev, generator=gen) * 0.01 + 1e-3).contiguous()
            z = (s * 2 ** (bits - 1)).contiguous()
            if gs <= 0:
                s, z = s[0].contiguous(), z[0].contiguous()
            for M in (args.ms or A8_MS):
                x = torch.randn(M, K, device=dev, generator=gen).half()
                y8 = torch.empty(M, N, device=dev, dtype=torch.float16)
                y8p = torch.empty(M, N, device=dev, dtype=torch.float16)
                y16 = torch.empty(M, N, device=dev, dtype=torch.float16)
                yd = torch.empty(M, N, device=dev, dtype=torch.float16)
                xq = torch.empty(M, K, device=dev, dtype=torch.int8)
                sx = torch.empty(M, device=dev)
                nb8 = lib.gptq_quant_gemm_a8_workspace_bytes(M, K, N, bits, gs)
                nb16 = lib.gptq_quant_gemm_workspace_bytes(M, K, N, bits, gs)
                ws8 = torch.empty(max(nb8, 1), dtype=torch.uint8, device=dev)
                ws16 = torch.empty(max(nb16, 1), dtype=torch.uint8, device=dev)
                st = _lib.stream

                def quant():
                    _lib.call("gptq_quant_act_rows", x.data_ptr(), _lib.F16, K, M, K, None, xq.data_ptr(), K, sx.data_ptr(),
                              st(dev))

                def gemm8(out):
                    _lib.call("gptq_quant_gemm_a8", xq.data_ptr(), K, sx.data_ptr(), M, qw.data_ptr(), s.data_ptr(),
                              z.data_ptr(), None, K, N, bits, gs, out.data_ptr(), _lib.F16, N, ws8.data_ptr(), nb8, st(dev))

                def full8():
                    quant()
                    gemm8(y8)

                pre8 = lambda: gemm8(y8p)                                              # noqa: E731
                f16 = lambda: _lib.call("gptq_quant_gemm", x.data_ptr(), _lib.F16, K, M, qw.data_ptr(), s.data_ptr(),  # noqa: E731
                                        z.data_ptr(), None, K, N, bits, gs, y16.data_ptr(), _lib.F16, N, ws16.data_ptr(), nb16,
                                        st(dev))
                dense = lambda: torch.matmul(x, Wd.t(), out=yd)                        # noqa: E731
                full8(); pre8(); f16()
                torch.cuda.synchronize()
                assert torch.equal(y8, gptq_amd.quant_matmul_a8(x, qw, s, z, bits, gs)) and torch.equal(y8, y8p)
                assert torch.equal(y16, gptq_amd.quant_matmul(x, qw, s, z, bits, gs))
                rel = float((y8.float() - y16.float()).norm() / y16.float().norm())
                reps = 20 if M <= 256 else 5
                graphs = [graphed(f, reps) for f in (full8, pre8, f16, f16, dense)]
                for _ in range(args.warmup):
                    for g in graphs:
                        g.replay()
                t = [[] for _ in graphs]
                for _ in range(args.iters):                                            # the five in turn
                    for i, g in enumerate(graphs):
                        t[i] += timed(g, reps, 1)
                t_full, t_pre, t_a, t_b, t_d = (statistics.median(v) for v in t)
                t16 = 0.5 * (t_a + t_b)
                aa = abs(t_a - t_b) / t16
                flops = 2.0 * M * K * N
                r = dict(K=K, N=N, M=M, bits=bits, groupsize=gs, a8_full_us=t_full * 1e6, a8_gemm_us=t_pre * 1e6,
                         fp16_path_us=t16 * 1e6, fp16_path_series_us=[t_a * 1e6, t_b * 1e6], aa_spread=aa,
                         dense_fp16_us=t_d * 1e6, full_over_fp16_path=t_full / t16, full_over_dense=t_full / t_d,
                         fp16_path_over_dense=t16 / t_d, a8_gemm_tflops=flops / t_pre / 1e12,
                         faster_than_fp16_path_beyond_aa=t_full < min(t_a, t_b) * (1 - aa), rel_err_vs_fp16_path=rel,
                         a8_workspace_bytes=nb8)
                rows.append(r)
                print(f"{K:>5}->{N:<5} {bits}b g{gs:<4} M={M:<5} a8 full {r['a8_full_us']:8.1f} us  gemm {r['a8_gemm_us']:8.1f} us"
                      f"  fp16 path {r['fp16_path_us']:8.1f} us (A/A {100 * aa:4.1f}%)  dense {r['dense_fp16_us']:8.1f} us"
                      f"  full/fp16 {r['full_over_fp16_path']:5.2f}  full/dense {r['full_over_dense']:5.2f}"
                      f"  {r['a8_gemm_tflops']:6.1f} TOP/s  rel err {rel:.2e}", flush=True)
                del graphs
    out = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "qgemm_a8.json")
    with open(out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(dev), "iters": args.iters, "warmup": args.warmup,
                   "reps_per_graph": {"M<=256": 20, "M>256": 5}, "rows": rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a8", action="store_true",
                    help="the GEMM on int8 activations beside the fp16 dequant GEMM and dense fp16")
    ap.add_argument("--grid-grad", action="store_true",
                    help="the grid gradients (dscales, dzeros, dbias) against the dense x.t() @ dy route")
    ap.add_argument("--backward", action="store_true",
                    help="the transposed dequant GEMM against dequant_packed + torch.matmul")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--perm", action="store_true", help="the act-order format: GEMM and mat-vec with / without perm")
    ap.add_argument("--bits", type=int, nargs="+", choices=(2, 3, 4, 8), default=None,
                    help="packed widths, each on a g128 grid (default: 3-bit per-row and 4-bit g128)")
    ap.add_argument("--ms", type=int, nargs="+", default=None, help=f"the M to run (default {MS})")
    args = ap.parse_args()
    from gptq_amd.build import ensure_built
    ensure_built()
    if args.a8:
        return main_a8(args)
    if args.perm:
        return main_perm(args)
    if args.backward:
        return main_backward(args)
    if args.grid_grad:
        return main_grid_grad(args)
    import gptq_amd
    from gptq_amd import _lib
    from gptq_amd.quant import pack_codes
    lib = _lib.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for K, N in SHAPES:
        Wd = (torch.randn(N, K, device=dev, generator=gen) * 0.02).half()
        for bits, gs in ([(b, 128) for b in args.bits] if args.bits else GRIDS):
            codes = torch.randint(0, 2 ** bits, (N, K), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
            qw = pack_codes(codes, bits)
            ng = K // gs if gs > 0 else 1
            s = torch.rand(ng, N, device=dev, generator=gen) * 0.01 + 1e-3
            z = s * 2 ** (bits - 1)
            if gs <= 0:
                s, z = s[0].contiguous(), z[0].contiguous()
            packed_bytes = qw.numel() * 4 + 2 * s.numel() * 4
            for M in (args.ms or MS):
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
