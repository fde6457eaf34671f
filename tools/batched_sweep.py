#!/usr/bin/env python3
"""One strided-batched launch (mm_gemm_batched_enqueue) against a loop of mm_gemm_enqueue calls over the same elements on
one stream.  HIP events around each form, warm-up first, best of N repetitions; operands filled on the device.

    python tools/batched_sweep.py [--reps 10] [--json out.json]

Prints one line per case: kernel the batched call resolves to, batched and loop time, throughput of each, and the ratio.
The loop is driven from Python (ctypes, one mm_gemm_enqueue per element): for small elements its time is mostly host-side
call overhead (tens of microseconds per call), so the ratio there is what a Python caller gains, not the device-side
launch cost alone.  For large elements (the 4096^3 rows) the device time dominates both forms.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemm_hls_amd as g  # noqa: E402

# (label, dtype, map, reduce, batch, n, k, m, broadcast_b)
CASES = [
    ("minplus_4096x128^3", "float", "Add", "Min", 4096, 128, 128, 128, False),
    ("maxplus_bcastB_4096x64x128x128", "float", "Add", "Max", 4096, 64, 128, 128, True),
    ("f32_1024x256^3", "float", "Multiply", "Add", 1024, 256, 256, 256, False),
    ("half_1024x256^3", "half", "Multiply", "Add", 1024, 256, 256, 256, False),
    ("f32_8x4096^3", "float", "Multiply", "Add", 8, 4096, 4096, 4096, False),
    ("half_8x4096^3", "half", "Multiply", "Add", 8, 4096, 4096, 4096, False),
    ("double_1024x256^3", "double", "Multiply", "Add", 1024, 256, 256, 256, False),
    ("double_8x4096^3", "double", "Multiply", "Add", 8, 4096, 4096, 4096, False),
    ("uint8_1024x256^3", "uint8_t", "Multiply", "Add", 1024, 256, 256, 256, False),
    ("uint8_8x4096^3", "uint8_t", "Multiply", "Add", 8, 4096, 4096, 4096, False),
]


def measure(dtype, mp, rd, batch, n, k, m, bcast_b, reps=10, warmup=3):
    """(batched seconds, loop seconds), each the best of `reps` event-timed runs after `warmup` untimed ones."""
    import torch
    L = g.lib()
    tdt = g.torch_dtype(dtype)
    dev = torch.device("cuda:0")
    a = torch.empty(batch * n * k, dtype=tdt, device=dev)
    b = torch.empty((1 if bcast_b else batch) * k * m, dtype=tdt, device=dev)
    c = torch.empty(batch * n * m, dtype=tdt, device=dev)
    for t, seed in ((a, 1), (b, 2)):
        rc = L.mm_fill_device(0, g.DTYPES[dtype], ctypes.c_void_p(t.data_ptr()), t.numel(), seed)
        assert rc == 0, L.mm_last_error().decode()
    cfg = g.make_config(dtype, mp, rd)
    es = a.element_size()
    sa, sb, sc = n * k, (0 if bcast_b else k * m), n * m
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)

    def batched():
        rc = L.mm_gemm_batched_enqueue(sp, ctypes.byref(cfg), a.data_ptr(), b.data_ptr(), c.data_ptr(), n, k, m, batch, sa, sb, sc)
        assert rc == 0, L.mm_last_error().decode()

    def loop():
        for e in range(batch):
            rc = L.mm_gemm_enqueue(sp, ctypes.byref(cfg), a.data_ptr() + e * sa * es, b.data_ptr() + e * sb * es,
                                   c.data_ptr() + e * sc * es, n, k, m)
            assert rc == 0, L.mm_last_error().decode()

    def best(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(stream)
            fn()
            e.record(stream)
            e.synchronize()
            times.append(s.elapsed_time(e) * 1e-3)
        return min(times)

    return best(batched), best(loop)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None, help="also write the results as JSON")
    args = ap.parse_args()
    rows = []
    print(f"{'case':34s} {'batched kernel':36s} {'batched ms':>10s} {'loop ms':>9s} {'batched TOp/s':>13s} "
          f"{'loop TOp/s':>10s} {'speedup':>8s}", flush=True)
    for label, dtype, mp, rd, batch, n, k, m, bb in CASES:
        kname = g.kernel_name_batched(g.make_config(dtype, mp, rd), n, k, m, batch)
        tb, tl = measure(dtype, mp, rd, batch, n, k, m, bb, reps=args.reps)
        ops = 2.0 * batch * n * k * m
        rows.append(dict(case=label, dtype=dtype, map=mp, reduce=rd, batch=batch, n=n, k=k, m=m, broadcast_b=bb,
                         kernel=kname, batched_s=tb, loop_s=tl, batched_tops=ops / tb / 1e12, loop_tops=ops / tl / 1e12,
                         speedup=tl / tb))
        r = rows[-1]
        print(f"{label:34s} {kname:36s} {tb * 1e3:10.3f} {tl * 1e3:9.3f} {r['batched_tops']:13.2f} {r['loop_tops']:10.2f} "
              f"{r['speedup']:7.2f}x", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
