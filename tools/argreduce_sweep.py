#!/usr/bin/env python3
"""Argmin / argmax launch (mm_gemm_argreduce_enqueue: values and the winning k) against the value-only launch of the same
problem (mm_gemm_batched_enqueue / _accumulate_enqueue: valu_tile under MM_PATH_AUTO), and MM_PATH_AUTO's argreduce kernel
(argreduce_tile where it serves; the 8-byte types run argreduce) against MM_PATH_ORDERED's (always argreduce, the
predicated kernel).  HIP events around each launch, warm-up first, the forms alternating, best of N; operands filled on
the device.  Each case also checks that the two argreduce launches return the same values and indices.

    python tools/argreduce_sweep.py [--reps 5] [--out-dir profiles]

Writes <out-dir>/argreduce_sweep_mi355x.txt and .json.  TOp/s counts two operations (map, reduce) per (output, k).
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemm_hls_amd as g  # noqa: E402

# (label, dtype, map, reduce, batch, n, k, m, accumulate, broadcast B)
CASES = [
    ("minplus_f32_8192^3", "float", "Add", "Min", 1, 8192, 8192, 8192, False, False),
    ("minplus_f64_8192^3", "double", "Add", "Min", 1, 8192, 8192, 8192, False, False),
    ("minplus_i32_8192^3", "int", "Add", "Min", 1, 8192, 8192, 8192, False, False),
    ("maxplus_f32_8192^3", "float", "Add", "Max", 1, 8192, 8192, 8192, False, False),
    ("apsp_relax_f32_8192x256x8192_acc", "float", "Add", "Min", 1, 8192, 256, 8192, True, False),
    ("minplus_f32_4096x128^3_bcastB", "float", "Add", "Min", 4096, 128, 128, 128, False, True),
]


def _timed(stream, fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(stream)
    fn()
    e.record(stream)
    e.synchronize()
    return s.elapsed_time(e) * 1e-3


def measure(dtype, mp, rd, batch, n, k, m, acc, bcast_b, reps=5, warmup=1):
    """{form: best seconds} for value_only (valu_tile), auto (argreduce_tile where it serves) and ordered (argreduce), the
    kernel names, and whether the two argreduce launches agreed bit for bit."""
    import torch
    L = g.lib()
    tdt = g.torch_dtype(dtype)
    dev = torch.device("cuda:0")
    a = torch.empty(batch * n * k, dtype=tdt, device=dev)
    b = torch.empty((1 if bcast_b else batch) * k * m, dtype=tdt, device=dev)
    c0 = torch.empty(batch * n * m, dtype=tdt, device=dev)
    for t, seed in ((a, 1), (b, 2), (c0, 3)):
        rc = L.mm_fill_device(0, g.DTYPES[dtype], ctypes.c_void_p(t.data_ptr()), t.numel(), seed)
        assert rc == 0, L.mm_last_error().decode()
    i0 = torch.full((batch * n * m,), -1, dtype=torch.int32, device=dev)
    sa, sb, sc = n * k, (0 if bcast_b else k * m), n * m
    outs = {f: (torch.empty_like(c0), torch.empty_like(i0)) for f in ("auto", "ordered")}
    c_val = torch.empty_like(c0)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    auto, ordered = g.make_config(dtype, mp, rd), g.make_config(dtype, mp, rd, g.PATH_ORDERED)
    names = {"value_only": g.kernel_name_batched(auto, n, k, m, batch),
             "auto": g.kernel_name_argreduce(auto, n, k, m, batch),
             "ordered": g.kernel_name_argreduce(ordered, n, k, m, batch)}

    def value_only():
        if acc:
            c_val.copy_(c0)
            return _timed(stream, lambda: g._check(L.mm_gemm_batched_accumulate_enqueue(
                sp, ctypes.byref(auto), a.data_ptr(), b.data_ptr(), c_val.data_ptr(), n, k, m, batch, sa, sb, sc)))
        return _timed(stream, lambda: g._check(L.mm_gemm_batched_enqueue(
            sp, ctypes.byref(auto), a.data_ptr(), b.data_ptr(), c_val.data_ptr(), n, k, m, batch, sa, sb, sc)))

    def arg(form):
        cfg = auto if form == "auto" else ordered
        c, i = outs[form]
        if acc:
            c.copy_(c0)
            i.copy_(i0)
        return _timed(stream, lambda: g._check(L.mm_gemm_argreduce_enqueue(
            sp, ctypes.byref(cfg), a.data_ptr(), b.data_ptr(), c.data_ptr(), i.data_ptr(), n, k, m, batch, sa, sb, sc, 0,
            int(acc))))

    forms = {"value_only": value_only, "auto": lambda: arg("auto"), "ordered": lambda: arg("ordered")}
    best = {f: float("inf") for f in forms}
    for r in range(warmup + reps):
        for f, fn in forms.items():
            t = fn()
            if r >= warmup:
                best[f] = min(best[f], t)
    same = bool(torch.equal(outs["auto"][1], outs["ordered"][1]) and
                torch.equal(outs["auto"][0].view(torch.uint8), outs["ordered"][0].view(torch.uint8)))
    return best, names, same


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import torch
    rows, lines = [], []
    hdr = (f"{'case':36s} {'value_only':>22s} {'argreduce AUTO':>22s} {'argreduce ORDERED':>22s} {'auto/value':>10s} "
           f"{'ordrd/auto':>10s} same")
    print(hdr)
    lines.append(hdr)
    for label, dtype, mp, rd, batch, n, k, m, acc, bcast_b in CASES:
        best, names, same = measure(dtype, mp, rd, batch, n, k, m, acc, bcast_b, args.reps)
        ops = 2.0 * batch * n * k * m
        tops = {f: ops / t / 1e12 for f, t in best.items()}
        row = {"case": label, "dtype": dtype, "map": mp, "reduce": rd, "batch": batch, "n": n, "k": k, "m": m,
               "accumulate": acc, "broadcast_b": bcast_b, "kernels": names, "seconds": best, "TOps": tops,
               "auto_over_value_time": best["auto"] / best["value_only"],
               "ordered_over_auto_time": best["ordered"] / best["auto"], "auto_equals_ordered": same}
        rows.append(row)
        cell = lambda f: f"{best[f] * 1e3:9.2f}ms {tops[f]:6.2f}TOp/s"  # noqa: E731
        ln = (f"{label:36s} {cell('value_only'):>22s} {cell('auto'):>22s} {cell('ordered'):>22s} "
              f"{row['auto_over_value_time']:9.2f}x {row['ordered_over_auto_time']:9.2f}x {'yes' if same else 'NO'}")
        print(ln, flush=True)
        lines.append(ln)
        lines.append(f"    kernels: {names}")
    lines.append(f"# device: {torch.cuda.get_device_name(0)}; best of {args.reps} after 1 warm-up; HIP events; "
                 "TOp/s = 2 * batch * N * K * M / time; auto/value = the AUTO argreduce time over the value-only launch's; "
                 "ordrd/auto = the ORDERED (predicated argreduce) time over the AUTO one's")
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "argreduce_sweep_mi355x.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(args.out_dir, "argreduce_sweep_mi355x.json"), "w") as f:
        json.dump(rows, f, indent=1)
    if not all(r["auto_equals_ordered"] for r in rows):
        sys.exit("the AUTO and ORDERED argreduce launches disagree")


if __name__ == "__main__":
    main()
