#!/usr/bin/env python3
"""A x B^T forms of argmin / argmax and of the log semiring (mm_gemm_argreduce_nt_enqueue, mm_gemm_logsumexp_nt_enqueue, Bt
stored M x K) against the row-major launch of the same product on a materialised transpose, on the same box in the same run:

  * argreduce_tile_nt against argreduce_tile and lse_hybrid_nt against lse_hybrid (the row-major launch on Bt^T, the
    transposition NOT timed): the cost, or gain, of staging Bt's slab like A's, or of expanding EB from Bt as it lies;
  * both against what a caller does today, torch's bt.mT.contiguous() followed by the row-major launch, both timed.

torch.cuda.Event around each form, warm-up first, the forms alternating, best of N; operands filled on the device.  The
spread column is (max - min) / min over the row-major launch's own N timings: what "the same speed" can mean in this run.

    python tools/nt_products_sweep.py [--reps 5] [--out profiles/nt_products_sweep_mi355x.txt]
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemm_hls_amd as g  # noqa: E402

# (label, product, dtype, reduce, n, k, m, accumulate); the map is Add throughout (min-plus, log semiring)
CASES = [
    ("argreduce_float_minplus_4096^3", "argreduce", "float", "Min", 4096, 4096, 4096, False),
    ("argreduce_float_minplus_8192^3", "argreduce", "float", "Min", 8192, 8192, 8192, False),
    ("argreduce_int_minplus_8192^3", "argreduce", "int", "Min", 8192, 8192, 8192, False),
    ("argreduce_float_acc_8192x256x8192", "argreduce", "float", "Min", 8192, 256, 8192, True),
    ("logsumexp_float_4096^3", "logsumexp", "float", "Max", 4096, 4096, 4096, False),
    ("logsumexp_float_8192^3", "logsumexp", "float", "Max", 8192, 8192, 8192, False),
]


def _timed(stream, fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(stream)
    fn()
    e.record(stream)
    e.synchronize()
    return s.elapsed_time(e) * 1e-3


def measure(product, dtype, rd, n, k, m, accumulate, reps=5, warmup=2):
    """(row-major timings, torch transpose + row-major timings, A x B^T timings): `reps` seconds each, after `warmup`."""
    import torch
    L = g.lib()
    tdt = g.torch_dtype(dtype)
    dev = torch.device("cuda:0")
    a = torch.empty((n, k), dtype=tdt, device=dev)
    bt = torch.empty((m, k), dtype=tdt, device=dev)
    c = torch.empty((n, m), dtype=tdt, device=dev)
    for t, seed in ((a, 1), (bt, 2), (c, 3)):
        rc = L.mm_fill_device(0, g.DTYPES[dtype], ctypes.c_void_p(t.data_ptr()), t.numel(), seed)
        assert rc == 0, L.mm_last_error().decode()
    b = bt.mT.contiguous()
    idx = torch.full((n, m), -1, dtype=torch.int32, device=dev)
    cfg = g.make_config(dtype, "Add", rd)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    acc = int(accumulate)

    def call(nt, bp):
        if product == "argreduce":
            fn = L.mm_gemm_argreduce_nt_enqueue if nt else L.mm_gemm_argreduce_enqueue
            rc = fn(sp, ctypes.byref(cfg), a.data_ptr(), bp.data_ptr(), c.data_ptr(), idx.data_ptr(), n, k, m, 1, 0, 0, 0, 0, acc)
        else:
            fn = L.mm_gemm_logsumexp_nt_enqueue if nt else L.mm_gemm_logsumexp_enqueue
            rc = fn(sp, ctypes.byref(cfg), a.data_ptr(), bp.data_ptr(), c.data_ptr(), n, k, m, 1, 0, 0, 0, acc)
        assert rc == 0, L.mm_last_error().decode()

    forms = (lambda: call(False, b), lambda: call(False, bt.mT.contiguous()), lambda: call(True, bt))
    for _ in range(warmup):
        for f in forms:
            f()
    torch.cuda.synchronize()
    times = ([], [], [])
    for _ in range(reps):   # alternating, so that clocks and temperature drift hit every form alike
        for ts, f in zip(times, forms):
            ts.append(_timed(stream, f))
    return times


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    lines = ["# A x B^T argreduce / logsumexp sweep (MI355X, best of %d, events around each form); NN = the row-major launch on a "
             "materialised transpose (transposition not timed); torch+NN = bt.mT.contiguous() + that launch; NN spread = (max - min) "
             "/ min of NN's own timings; ratios are throughput ratios = time ratios inverted" % args.reps,
             f"{'case':36s} {'NT kernel':18s} {'NN kernel':15s} {'NN ms':>9s} {'NN spread':>9s} {'torch+NN ms':>11s} {'NT ms':>9s} "
             f"{'TOp/s NT':>9s} {'NT/NN':>6s} {'NT/torch+NN':>11s}"]
    print("\n".join(lines), flush=True)
    for label, product, dtype, rd, n, k, m, accumulate in CASES:
        cfg = g.make_config(dtype, "Add", rd)
        names = ((g.kernel_name_argreduce_nt, g.kernel_name_argreduce) if product == "argreduce"
                 else (g.kernel_name_logsumexp_nt, g.kernel_name_logsumexp))
        nn, tr, nt = measure(product, dtype, rd, n, k, m, accumulate, reps=args.reps)
        t_nn, t_tr, t_nt = min(nn), min(tr), min(nt)
        lines.append(f"{label:36s} {names[0](cfg, n, k, m):18s} {names[1](cfg, n, k, m):15s} {t_nn * 1e3:9.3f} "
                     f"{(max(nn) - t_nn) / t_nn:9.3f} {t_tr * 1e3:11.3f} {t_nt * 1e3:9.3f} {2.0 * n * k * m / t_nt / 1e12:9.1f} "
                     f"{t_nn / t_nt:6.3f} {t_tr / t_nt:11.3f}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
