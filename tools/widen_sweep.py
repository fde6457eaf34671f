#!/usr/bin/env python3
"""Widening launch (mm_gemm_widen_enqueue: int8_t operands to an int C, half operands to a float C) against the narrow
batched launch (mm_gemm_batched_enqueue) of the same operands: the cost of storing -- and, accumulating, of reading -- four
bytes per output instead of one or two, on the same kernel and schedule.  torch.cuda.Event around each launch, warm-up
first, the forms alternating, best of N; operands filled on the device.

    python tools/widen_sweep.py [--reps 7] [--out profiles/widen_sweep_mi355x.txt]

Prints one line per case: the wide kernel, narrow / wide / wide-accumulating time, and the ratio of wide to narrow
THROUGHPUT (narrow time / wide time) with the floor tests/test_gpu_widen.py derives from it (0.93 x the ratio: the 6-7 %
box-to-box spread of VERDICT.md).
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemm_hls_amd as g  # noqa: E402

# (label, dtype, n, k, m, K x N A)
CASES = [
    ("int8_16384^3", "int8_t", 16384, 16384, 16384, False),
    ("int8_32768^3", "int8_t", 32768, 32768, 32768, False),
    ("half_16384^3", "half", 16384, 16384, 16384, False),
    ("half_32768^3", "half", 32768, 32768, 32768, False),
    ("int8_8192x512x8192", "int8_t", 8192, 512, 8192, False),     # a rank-k update: the output dominates
    ("half_8192x256x8192", "half", 8192, 256, 8192, False),
    ("int8_4097x4096x4096", "int8_t", 4097, 4096, 4096, False),   # ragged N
    ("half_4096x4112x4096", "half", 4096, 4112, 4096, False),     # K % 16 == 0 only: slab64
    ("half_KxN_4096^3", "half", 4096, 4096, 4096, True),          # K x N A served where it lies
    ("half_KxN_2048x2048x8192", "half", 2048, 2048, 8192, True),  # K x N A the narrow single launch would transpose first: widen_ordered
]
SPREAD = 0.93


def _timed(stream, fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(stream)
    fn()
    e.record(stream)
    e.synchronize()
    return s.elapsed_time(e) * 1e-3


def measure(dtype, n, k, m, reps=7, warmup=2, transposed_a=False):
    """(narrow seconds, wide seconds, wide accumulating seconds), each the best of `reps` after `warmup`."""
    import torch
    L = g.lib()
    tdt, wdt = g.torch_dtype(dtype), g.torch_dtype(g.widen_dtype(dtype))
    dev = torch.device("cuda:0")
    a = torch.empty(n * k, dtype=tdt, device=dev)
    b = torch.empty(k * m, dtype=tdt, device=dev)
    for t, seed in ((a, 1), (b, 2)):
        rc = L.mm_fill_device(0, g.DTYPES[dtype], ctypes.c_void_p(t.data_ptr()), t.numel(), seed)
        assert rc == 0, L.mm_last_error().decode()
    c = torch.empty(n * m, dtype=tdt, device=dev)
    cw = torch.zeros(n * m, dtype=wdt, device=dev)
    cfg = g.make_config(dtype, transposed_a=transposed_a)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)

    def narrow():
        rc = L.mm_gemm_batched_enqueue(sp, ctypes.byref(cfg), a.data_ptr(), b.data_ptr(), c.data_ptr(), n, k, m, 1, 0, 0, 0)
        assert rc == 0, L.mm_last_error().decode()

    def wide(acc=0):
        rc = L.mm_gemm_widen_enqueue(sp, ctypes.byref(cfg), a.data_ptr(), b.data_ptr(), cw.data_ptr(), n, k, m, 1, 0, 0, 0, acc)
        assert rc == 0, L.mm_last_error().decode()

    for _ in range(warmup):
        narrow()
        wide()
        wide(1)
    torch.cuda.synchronize()
    tn, tw, ta = [], [], []
    for _ in range(reps):   # alternating, so that clocks and temperature drift hit every form alike
        tn.append(_timed(stream, narrow))
        tw.append(_timed(stream, wide))
        ta.append(_timed(stream, lambda: wide(1)))
    return min(tn), min(tw), min(ta)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    lines = ["# widen sweep (MI355X, best of %d, events around each launch); ratio = wide / narrow throughput = narrow time / "
             "wide time; floor = %.2f x ratio" % (args.reps, SPREAD),
             f"{'case':22s} {'kernel':42s} {'narrow ms':>9s} {'wide ms':>9s} {'wide+= ms':>9s} {'TOp/s wide':>10s} {'ratio':>6s} "
             f"{'ratio+=':>7s} {'floor':>6s}"]
    print("\n".join(lines), flush=True)
    for label, dtype, n, k, m, kxn in CASES:
        kname = g.kernel_name_widen(g.make_config(dtype, transposed_a=kxn), n, k, m)
        tn, tw, ta = measure(dtype, n, k, m, reps=args.reps, transposed_a=kxn)
        lines.append(f"{label:22s} {kname:42s} {tn * 1e3:9.3f} {tw * 1e3:9.3f} {ta * 1e3:9.3f} {2.0 * n * k * m / tw / 1e12:10.1f} "
                     f"{tn / tw:6.3f} {tn / ta:7.3f} {SPREAD * tn / tw:6.3f}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
