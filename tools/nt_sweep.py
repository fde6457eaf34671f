#!/usr/bin/env python3
"""A x B^T launch (mm_gemm_nt_enqueue, Bt stored M x K) against the row-major launch on a materialised transpose, on the same
box in the same run:

  * valu_tile_nt against valu_tile (mm_gemm_batched_enqueue on Bt^T, the transposition NOT timed): the cost, or gain, of
    staging Bt's slab like A's and storing C element by element;
  * nt_prepass against what a caller does today, torch's bt.mT.contiguous() followed by the row-major launch, both timed;
    the row-major launch alone is the floor either route could reach.

torch.cuda.Event around each form, warm-up first, the forms alternating, best of N; operands filled on the device.

    python tools/nt_sweep.py [--reps 7] [--out profiles/nt_sweep_mi355x.txt]
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemm_hls_amd as g  # noqa: E402

# (label, dtype, map, reduce, n = k = m)
CASES = [
    ("float_minplus_4096^3", "float", "Add", "Min", 4096),
    ("float_minplus_8192^3", "float", "Add", "Min", 8192),
    ("half_minplus_4096^3", "half", "Add", "Min", 4096),
    ("half_minplus_8192^3", "half", "Add", "Min", 8192),
    ("double_minplus_4096^3", "double", "Add", "Min", 4096),
    ("float_gemm_4096^3", "float", "Multiply", "Add", 4096),
    ("float_gemm_8192^3", "float", "Multiply", "Add", 8192),
    ("half_gemm_4096^3", "half", "Multiply", "Add", 4096),
    ("half_gemm_8192^3", "half", "Multiply", "Add", 8192),
]


def _timed(stream, fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(stream)
    fn()
    e.record(stream)
    e.synchronize()
    return s.elapsed_time(e) * 1e-3


def measure(dtype, mp, rd, n, reps=7, warmup=2):
    """(row-major seconds, torch transpose + row-major seconds, A x B^T seconds), each the best of `reps` after `warmup`."""
    import torch
    L = g.lib()
    tdt = g.torch_dtype(dtype)
    dev = torch.device("cuda:0")
    a = torch.empty((n, n), dtype=tdt, device=dev)
    bt = torch.empty((n, n), dtype=tdt, device=dev)
    for t, seed in ((a, 1), (bt, 2)):
        rc = L.mm_fill_device(0, g.DTYPES[dtype], ctypes.c_void_p(t.data_ptr()), t.numel(), seed)
        assert rc == 0, L.mm_last_error().decode()
    b = bt.mT.contiguous()
    c = torch.empty((n, n), dtype=tdt, device=dev)
    cfg = g.make_config(dtype, mp, rd)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)

    def nn(bp=None):
        rc = L.mm_gemm_batched_enqueue(sp, ctypes.byref(cfg), a.data_ptr(), (b if bp is None else bp).data_ptr(), c.data_ptr(),
                                       n, n, n, 1, 0, 0, 0)
        assert rc == 0, L.mm_last_error().decode()

    def torch_then_nn():
        nn(bt.mT.contiguous())

    def nt():
        rc = L.mm_gemm_nt_enqueue(sp, ctypes.byref(cfg), a.data_ptr(), bt.data_ptr(), c.data_ptr(), n, n, n, 1, 0, 0, 0, 0)
        assert rc == 0, L.mm_last_error().decode()

    for _ in range(warmup):
        nn()
        torch_then_nn()
        nt()
    torch.cuda.synchronize()
    t_nn, t_tr, t_nt = [], [], []
    for _ in range(reps):   # alternating, so that clocks and temperature drift hit every form alike
        t_nn.append(_timed(stream, nn))
        t_tr.append(_timed(stream, torch_then_nn))
        t_nt.append(_timed(stream, nt))
    return min(t_nn), min(t_tr), min(t_nt)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    lines = ["# A x B^T sweep (MI355X, best of %d, events around each form); NN = the row-major launch on a materialised transpose "
             "(transposition not timed); torch+NN = bt.mT.contiguous() + that launch; ratios are throughput ratios = time ratios "
             "inverted" % args.reps,
             f"{'case':24s} {'NT kernel':14s} {'NN kernel':40s} {'NN ms':>9s} {'torch+NN ms':>11s} {'NT ms':>9s} {'TOp/s NT':>9s} "
             f"{'NT/NN':>6s} {'NT/torch+NN':>11s}"]
    print("\n".join(lines), flush=True)
    for label, dtype, mp, rd, n in CASES:
        cfg = g.make_config(dtype, mp, rd)
        t_nn, t_tr, t_nt = measure(dtype, mp, rd, n, reps=args.reps)
        lines.append(f"{label:24s} {g.kernel_name_nt(cfg, n, n, n):14s} {g.kernel_name_batched(cfg, n, n, n, 1):40s} {t_nn * 1e3:9.3f} "
                     f"{t_tr * 1e3:11.3f} {t_nt * 1e3:9.3f} {2.0 * n ** 3 / t_nt / 1e12:9.1f} {t_nn / t_nt:6.3f} {t_tr / t_nt:11.3f}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
