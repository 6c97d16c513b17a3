"""Mixed-width solves against what they replace, on the Llama-7B q/k/v Linears (three 4096 x 4096 that share one Hessian;
4-bit per-row grids with act-order, the benchmark's llama7b configuration).

    python tools/bench_mixed.py [--iters 7] [--warmup 2] [--json profiles/mixed_bits_bench.json]

(a) widths 4 / 4 / 3 (the reference's linearwise table) through fasterquant_many: ONE joint solve with a width per row
    (gptq.JOINT_SOLVE = True) against three separate solves on concurrent streams (JOINT_SOLVE = False).
(b) GPTQ.sensitivity((2, 3, 4, 8)) -- one solve of the weights stacked four times -- against four separate solves of the
    same Linear, one per width: one after the other (`fasterquant` x 4, what a sweep costs without it) and on concurrent
    streams (`fasterquant_many`).
Every sample builds fresh solver objects whose Hessian is folded BEFORE the clock starts; the two sides of a comparison
are timed alternately in one process with device events around the call (the calls end with the solver's own
synchronisation, so host time is inside both).  Reported: median and min / max milliseconds."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

R = C = 4096
KW = dict(blocksize=128, percdamp=0.01, groupsize=-1, actorder=True, static_groups=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from gptq_amd.build import ensure_built
    ensure_built()
    import gptq_amd
    from gptq_amd import gptq as gm
    gm.VERBOSE = False
    gm.HESSIAN_DEFER = 2                                   # objects share a running Hessian only while updates are deferred
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    Ws = [(torch.randn(R, C, device=dev, generator=gen) * 0.02).half() for _ in range(3)]
    X = (torch.randn(1, 2048, C, device=dev, generator=gen) * (1 + torch.arange(C, device=dev) % 7)).half()

    def solver(W, bits):
        lin = torch.nn.Linear(C, R, bias=False, device=dev, dtype=torch.float16)
        lin.weight.data = W.clone()
        g = gptq_amd.GPTQ(lin)
        g.quantizer = gptq_amd.Quantizer()
        g.quantizer.configure(bits, perchannel=True, sym=False, mse=False)
        return g

    def calibrated(specs):
        objs = [solver(W, bits) for W, bits in specs]
        for g in objs:
            g.add_batch(X, None)
        gm.flush_pending()                                 # H is folded (and shared) before the clock starts
        return objs

    def clocked(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    def qkv(joint):
        objs = calibrated(list(zip(Ws, (4, 4, 3))))
        gm.JOINT_SOLVE = joint
        ms, _ = clocked(lambda: gptq_amd.fasterquant_many(objs, **KW))
        assert [o.joint_rows for o in objs] == ([3 * R] * 3 if joint else [R] * 3)
        res = [(o.codes, o.error) for o in objs]
        for o in objs:
            o.free()
        return ms, res

    widths = (2, 3, 4, 8)

    def sweep(mode):
        if mode == "sensitivity":
            g, = calibrated([(Ws[0], 4)])
            ms, errs = clocked(lambda: g.sensitivity(wbits=widths, **KW))
            g.free()
            return ms, errs
        objs = calibrated([(Ws[0], b) for b in widths])
        gm.JOINT_SOLVE = False
        if mode == "serial":
            ms, _ = clocked(lambda: [o.fasterquant(**KW) for o in objs])
        else:
            ms, _ = clocked(lambda: gptq_amd.fasterquant_many(objs, **KW))
        errs = {b: o.error for b, o in zip(widths, objs)}
        for o in objs:
            o.free()
        return ms, errs

    def stats(ts):
        return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), samples=ts)

    t = {k: [] for k in ("qkv_joint_mixed", "qkv_separate", "sweep_sensitivity", "sweep_serial", "sweep_streams")}
    for it in range(args.warmup + args.iters):
        keep = it >= args.warmup
        a, ra = qkv(True)
        b, rb = qkv(False)
        for (ca, ea), (cb, eb) in zip(ra, rb):             # the two sides computed the same thing
            assert torch.equal(ca, cb) and abs(ea - eb) <= 1e-5 * abs(eb)
        c, ec = sweep("sensitivity")
        d, ed = sweep("serial")
        e, ee = sweep("streams")
        for w in widths:
            assert abs(ec[w] - ed[w]) <= 1e-5 * abs(ed[w]) and abs(ee[w] - ed[w]) <= 1e-5 * abs(ed[w])
        if keep:
            for k, v in zip(t, (a, b, c, d, e)):
                t[k].append(v)
    gm.JOINT_SOLVE = True
    out = {k: stats(v) for k, v in t.items()}
    med = {k: v["median_ms"] for k, v in out.items()}
    print(f"(a) q/k/v 4/4/3 bits: joint mixed {med['qkv_joint_mixed']:.2f} ms, separate (3 streams) {med['qkv_separate']:.2f} ms"
          f"  -> x{med['qkv_separate'] / med['qkv_joint_mixed']:.2f}")
    print(f"(b) sweep 2/3/4/8 bits: sensitivity {med['sweep_sensitivity']:.2f} ms, four solves in turn {med['sweep_serial']:.2f} ms"
          f" (x{med['sweep_serial'] / med['sweep_sensitivity']:.2f}), on streams {med['sweep_streams']:.2f} ms"
          f" (x{med['sweep_streams'] / med['sweep_sensitivity']:.2f})")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "shape": [R, C], "options": KW, "iters": args.iters,
                       "warmup": args.warmup, "results": out}, f, indent=1)


if __name__ == "__main__":
    main()
