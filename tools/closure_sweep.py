#!/usr/bin/env python3
"""Semiring closure (mm_closure_enqueue: blocked Floyd-Warshall in place) against repeated squaring with the accumulating
product (addmm_ / baddbmm_ on a copy, ceil(log2 n) rounds), and against its own step-3 launches alone (the T seeded rank-B
updates it runs: mm_gemm_batched_accumulate_enqueue, or mm_gemm_argreduce_enqueue with witnesses, on (n, B, n)), so that the
cost of the diagonal and panel phases shows.  HIP events around each form, warm-up first, best of N; dense random graphs
with integer weights in [1, 100] (diagonal 0), filled on the device.

    python tools/closure_sweep.py [--reps 3] [--out-dir profiles]

Writes <out-dir>/closure_sweep_mi355x.txt and .json.  TOp/s counts 2 n^3 operations per graph (map and reduce per (i, j, v)).
"""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemm_hls_amd as g  # noqa: E402

# (label, dtype, batch, n, witness)
CASES = [
    ("minplus_f32_4096", "float", 1, 4096, False),
    ("minplus_f32_8192", "float", 1, 8192, False),
    ("minplus_f32_16384", "float", 1, 16384, False),
    ("minplus_i32_8192", "int", 1, 8192, False),
    ("minplus_f64_8192", "double", 1, 8192, False),
    ("minplus_f32_8192_witness", "float", 1, 8192, True),
    ("minplus_f32_4096x64", "float", 4096, 64, False),
    ("minplus_f32_1024x128", "float", 1024, 128, False),
    # one graph of one block: exactly one diagonal launch, the step whose latency chains T times in a blocked closure
    ("diag_latency_f32_B256", "float", 1, 256, False),
    ("diag_latency_f32_B128_witness", "float", 1, 128, True),
]


def _timed(fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e-3


def _graphs(dtype, batch, n):
    import torch
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    d = torch.randint(1, 101, (batch, n, n), device="cuda:0", generator=gen).to(g.torch_dtype(dtype))
    d.diagonal(dim1=1, dim2=2).zero_()
    return d if batch > 1 else d[0]


def measure(dtype, batch, n, witness, reps=3):
    import torch
    L = g.lib()
    cfg = g.make_config(dtype, "Add", "Min")
    src = _graphs(dtype, batch, n)
    d = src.clone()
    w = torch.empty(d.shape, dtype=torch.int32, device=d.device) if witness else None
    block = g.get_tuning("closure_block")
    block = block if block > 0 else (256 if not witness and g.lib().mm_dtype_size(g.DTYPES[dtype]) <= 4 else 128)

    def closure():
        d.copy_(src)
        g.closure_(d, w, dtype)

    # step 3 alone: T seeded rank-B updates of every graph, on snapshots of the closure's shapes
    rounds = [(k0, min(block, n - k0)) for k0 in range(0, n, block)] if n > block else []
    tdt = g.torch_dtype(dtype)
    cc = torch.ones(batch * n * block, dtype=tdt, device=d.device)
    rc = torch.ones(batch * n * block, dtype=tdt, device=d.device)
    d3 = src.clone()
    w3 = torch.full(d.shape, -1, dtype=torch.int32, device=d.device)

    def step3():
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for k0, bt in rounds:
            if witness:
                r = L.mm_gemm_argreduce_enqueue(stream, ctypes.byref(cfg), cc.data_ptr(), rc.data_ptr(), d3.data_ptr(),
                                                w3.data_ptr(), n, bt, n, batch, n * bt, n * bt, n * n, k0, 1)
            else:
                r = L.mm_gemm_batched_accumulate_enqueue(stream, ctypes.byref(cfg), cc.data_ptr(), rc.data_ptr(),
                                                         d3.data_ptr(), n, bt, n, batch, n * bt, n * bt, n * n)
            assert r == 0, L.mm_last_error().decode()

    sq = src.clone()
    steps = math.ceil(math.log2(n))

    def squaring():
        sq.copy_(src)
        for _ in range(steps):
            prev = sq.clone()
            if batch > 1:
                g.baddbmm_(sq, prev, prev, dtype, "Add", "Min")
            else:
                g.addmm_(sq, prev, prev, dtype, "Add", "Min")

    out = {}
    for name, fn in (("closure", closure), ("step3", step3), ("squaring", squaring)):
        if name == "step3" and not rounds:
            out[name] = 0.0
            continue
        fn()   # warm-up (and the workspace pool)
        out[name] = min(_timed(fn) for _ in range(reps))
    # the copies inside the timed closure and squaring are n^2 element moves, noted rather than subtracted
    closure()
    squaring()
    out["agrees_with_squaring"] = bool(torch.equal(d, sq)) if not witness else None
    out["kernel"] = g.kernel_name_closure(cfg, n, batch, witness)
    out["block"] = block
    out["step3_kernel"] = (g.kernel_name_argreduce(cfg, n, block, n, batch) if witness
                           else g.kernel_name_batched(cfg, n, block, n, batch)) if rounds else None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--cases", default="", help="comma-separated labels (default: all)")
    args = ap.parse_args()
    import torch
    rows, lines = [], []
    hdr = (f"{'case':28s} {'kernel':16s} {'B':>4s} {'closure ms':>11s} {'TOp/s':>7s} {'step3 ms':>9s} {'1+2 over 3':>10s} "
           f"{'squaring ms':>12s} {'speedup':>8s}  step-3 kernel")
    lines.append(hdr)
    print(hdr, flush=True)
    for label, dtype, batch, n, witness in CASES:
        if args.cases and label not in args.cases.split(","):
            continue
        r = measure(dtype, batch, n, witness, args.reps)
        tops = 2.0 * batch * n ** 3 / r["closure"] / 1e12
        over = (r["closure"] - r["step3"]) / r["step3"] if r["step3"] else None
        row = dict(case=label, dtype=dtype, batch=batch, n=n, witness=witness, closure_s=r["closure"], step3_s=r["step3"],
                   squaring_s=r["squaring"], tops=tops, overhead_steps12=over, speedup_vs_squaring=r["squaring"] / r["closure"],
                   kernel=r["kernel"], block=r["block"], step3_kernel=r["step3_kernel"],
                   agrees_with_squaring=r["agrees_with_squaring"])
        rows.append(row)
        line = (f"{label:28s} {r['kernel']:16s} {r['block']:4d} {r['closure'] * 1e3:11.3f} {tops:7.2f} "
                f"{r['step3'] * 1e3:9.3f} {('%9.1f%%' % (100 * over)) if over is not None else '         -':>10s} "
                f"{r['squaring'] * 1e3:12.3f} {row['speedup_vs_squaring']:7.2f}x  {r['step3_kernel'] or '-'}")
        lines.append(line)
        print(line, flush=True)
        torch.cuda.empty_cache()
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "closure_sweep_mi355x.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(args.out_dir, "closure_sweep_mi355x.json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
