#!/usr/bin/env python3
"""Accumulating launch (mm_gemm_batched_accumulate_enqueue, C <- C (+) A (x) B) against the plain batched launch
(mm_gemm_batched_enqueue) of the same problem: the cost of reading C once more.  HIP events around each launch, warm-up
first, the two forms alternating, best of N; operands filled on the device.

    python tools/accumulate_sweep.py [--reps 7] [--json out.json]

Prints one line per case: the kernel (the same for both forms), plain and seeded time, their ratio, and -- for the rank-k
updates -- the budget "plain + one read of C at the copy bandwidth measured in the same run" (a device-to-device copy of
a buffer the size of C: bandwidth = bytes read + bytes written over its time).
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemm_hls_amd as g  # noqa: E402

# (label, dtype, map, reduce, batch, n, k, m, rank-k update)
CASES = [
    ("f32_8192^3", "float", "Multiply", "Add", 1, 8192, 8192, 8192, False),
    ("f32_16384^3", "float", "Multiply", "Add", 1, 16384, 16384, 16384, False),
    ("f64_8192^3", "double", "Multiply", "Add", 1, 8192, 8192, 8192, False),
    ("half_16384^3", "half", "Multiply", "Add", 1, 16384, 16384, 16384, False),
    ("uint8_16384^3", "uint8_t", "Multiply", "Add", 1, 16384, 16384, 16384, False),
] + [(f"minplus_8192x{k}x8192", "float", "Add", "Min", 1, 8192, k, 8192, True) for k in (128, 256, 1024)] + [
    (f"f32_8192x{k}x8192", "float", "Multiply", "Add", 1, 8192, k, 8192, True) for k in (128, 256, 1024)] + [
    ("f32_1024x256^3", "float", "Multiply", "Add", 1024, 256, 256, 256, False),
]


def _timed(stream, fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(stream)
    fn()
    e.record(stream)
    e.synchronize()
    return s.elapsed_time(e) * 1e-3


def measure(dtype, mp, rd, batch, n, k, m, reps=7, warmup=2):
    """(plain seconds, seeded seconds, copy seconds of a C-sized buffer), each the best of `reps` after `warmup`."""
    import torch
    L = g.lib()
    tdt = g.torch_dtype(dtype)
    dev = torch.device("cuda:0")
    a = torch.empty(batch * n * k, dtype=tdt, device=dev)
    b = torch.empty(batch * k * m, dtype=tdt, device=dev)
    c = torch.empty(batch * n * m, dtype=tdt, device=dev)
    for t, seed in ((a, 1), (b, 2), (c, 3)):
        rc = L.mm_fill_device(0, g.DTYPES[dtype], ctypes.c_void_p(t.data_ptr()), t.numel(), seed)
        assert rc == 0, L.mm_last_error().decode()
    c2 = torch.empty_like(c)
    cfg = g.make_config(dtype, mp, rd)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    args = (a.data_ptr(), b.data_ptr(), c.data_ptr(), n, k, m, batch, n * k, k * m, n * m)

    def plain():
        rc = L.mm_gemm_batched_enqueue(sp, ctypes.byref(cfg), *args)
        assert rc == 0, L.mm_last_error().decode()

    def seeded():
        rc = L.mm_gemm_batched_accumulate_enqueue(sp, ctypes.byref(cfg), *args)
        assert rc == 0, L.mm_last_error().decode()

    def copy():
        c2.copy_(c)

    for _ in range(warmup):
        plain()
        seeded()
        copy()
    torch.cuda.synchronize()
    tp, ts, tc = [], [], []
    for _ in range(reps):   # alternating, so that clocks and temperature drift hit both forms alike
        tp.append(_timed(stream, plain))
        ts.append(_timed(stream, seeded))
        tc.append(_timed(stream, copy))
    return min(tp), min(ts), min(tc), c.numel() * c.element_size()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None, help="also write the results as JSON")
    args = ap.parse_args()
    rows = []
    print(f"{'case':24s} {'kernel':40s} {'plain ms':>9s} {'seeded ms':>9s} {'ratio':>6s} {'copy GB/s':>9s} "
          f"{'budget ms':>9s} {'within':>6s}", flush=True)
    for label, dtype, mp, rd, batch, n, k, m, rank_k in CASES:
        kname = g.kernel_name_batched(g.make_config(dtype, mp, rd), n, k, m, batch)
        tp, ts, tc, cbytes = measure(dtype, mp, rd, batch, n, k, m, reps=args.reps)
        bw = 2.0 * cbytes / tc
        budget = tp + cbytes / bw if rank_k else 1.03 * tp
        r = dict(case=label, dtype=dtype, map=mp, reduce=rd, batch=batch, n=n, k=k, m=m, kernel=kname, plain_s=tp,
                 seeded_s=ts, ratio=ts / tp, copy_s=tc, copy_gbps=bw / 1e9, c_bytes=cbytes,
                 target="plain + C read" if rank_k else "1.03 x plain", budget_s=budget, within_target=ts <= budget)
        rows.append(r)
        print(f"{label:24s} {kname:40s} {tp * 1e3:9.3f} {ts * 1e3:9.3f} {ts / tp:6.3f} {bw / 1e9:9.0f} {budget * 1e3:9.3f} "
              f"{'yes' if r['within_target'] else 'NO':>6s}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
