#!/usr/bin/env python3
"""Bit-packed Boolean product and transitive closure (mm_bits_gemm_enqueue, mm_bits_closure_enqueue) against the byte forms
the library already had: bmm / baddbmm_ and closure_ with (And, Max) on 0 / 1 uint8_t, on the unpacked operands, same logical
shape, same process, interleaved rounds.  HIP events around each form, one warm-up, best of N, and the spread of the N
((max - min) / min) next to every figure.

    python tools/bits_sweep.py [--reps 5] [--out-dir profiles]

Writes <out-dir>/bits_sweep_mi355x.txt and .json.  The packed product skips the k no row of a wavefront has set, so its time
depends on the data: every product shape runs at the tests' density sqrt(ln 2 / K) (half the outputs set) and at density 0.5
(nothing to skip).  "of peak" = n k ceil(m / 32) lane-operations -- one acc |= mask & b per lane per 32 outputs -- over the
time, against 256 CUs x 128 lanes x 2.4 GHz.
"""
import math

from _bits_sweep import PEAK_LANE_OPS, _interleaved, _random_bits, g, sweep_main

# (label, n, k, m, density or None for sqrt(ln 2 / k), accumulate)
PRODUCTS = [
    ("product_4096_half_set", 4096, 4096, 4096, None, False),
    ("product_4096_dense", 4096, 4096, 4096, 0.5, False),
    ("product_16384_half_set", 16384, 16384, 16384, None, False),
    ("product_16384_dense", 16384, 16384, 16384, 0.5, False),
    ("rank64_accumulate_16384", 16384, 64, 16384, None, True),
    ("rank64_accumulate_16384_dense", 16384, 64, 16384, 0.5, True),
]
# (label, n, byte form too)
CLOSURES = [("closure_4096", 4096, True), ("closure_16384", 16384, True), ("closure_65536", 65536, False)]


def product(n, k, m, density, accumulate, reps):
    import torch
    p = density if density is not None else min(1.0, math.sqrt(math.log(2.0) / k))
    a8, ap = _random_bits(n, k, p, 1)
    b8, bp = _random_bits(k, m, p, 2)
    c8, cp = _random_bits(n, m, 0.1, 3) if accumulate else (torch.empty((n, m), dtype=torch.uint8, device="cuda:0"), None)
    if cp is None:
        cp = torch.empty((n, g.bits_words(m)), dtype=torch.int32, device="cuda:0")
    if accumulate:   # C only gains bits, so repeated rounds do the same work
        forms = {"packed": lambda: g.bits_addmm_(cp, ap, bp, k, m),
                 "byte": lambda: g.addmm_(c8, a8, b8, "uint8_t", "And", "Max")}
    else:
        forms = {"packed": lambda: g.bits_matmul(ap, bp, k, m, out=cp),
                 "byte": lambda: g.matmul(a8, b8, "uint8_t", "And", "Max", out=c8)}
    t = _interleaved(forms, reps)
    agree = bool(torch.equal(g.unpack_bits(cp, m, dtype=torch.uint8), c8))
    cfg = g.make_config("uint8_t", "And", "Max")
    return dict(density=p, packed_s=t["packed"][0], packed_spread=t["packed"][1], byte_s=t["byte"][0], byte_spread=t["byte"][1],
                ratio=t["byte"][0] / t["packed"][0], of_peak=n * k * g.bits_words(m) / t["packed"][0] / PEAK_LANE_OPS,
                output_density=float(c8.float().mean()), agree=agree, kernel=g.kernel_name_bits_gemm(n, k, m),
                byte_kernel=g.kernel_name_batched(cfg, n, k, m, 1) if accumulate else g.kernel_name(cfg, n, k, m))


def closure(n, with_byte, reps):
    import torch
    src8, srcp = _random_bits(n, n, 1.5 / n, 4)
    dp = srcp.clone()

    def packed():
        dp.copy_(srcp)
        g.bits_closure_(dp)
    forms = {"packed": packed}
    if with_byte:
        d8 = src8.clone()

        def byte():
            d8.copy_(src8)
            g.closure_(d8, None, "uint8_t", "And", "Max")
        forms["byte"] = byte
    t = _interleaved(forms, reps)
    out = dict(packed_s=t["packed"][0], packed_spread=t["packed"][1], kernel=g.kernel_name_bits_closure(n),
               closure_density=float(g.unpack_bits(dp[:4096], n, dtype=torch.uint8).float().mean()))
    if with_byte:
        out.update(byte_s=t["byte"][0], byte_spread=t["byte"][1], ratio=t["byte"][0] / t["packed"][0],
                   agree=bool(torch.equal(g.unpack_bits(dp, n, dtype=torch.uint8), d8)),
                   byte_kernel=g.kernel_name_closure(g.make_config("uint8_t", "And", "Max"), n))
    return out


def cases(reps, wanted, emit, rows):
    import torch
    emit(f"best of {reps}, interleaved; spread = (max - min) / min of the {reps}; the timed closures include one copy of their input")
    emit(f"{'case':30s} {'density':>8s} {'packed ms':>10s} {'spread':>7s} {'byte ms':>10s} {'spread':>7s} {'byte/packed':>11s} "
         f"{'of peak':>8s} {'out dens':>8s} {'same':>5s}  kernels")
    for label, n, k, m, density, accumulate in PRODUCTS:
        if not wanted(label):
            continue
        r = product(n, k, m, density, accumulate, reps)
        rows.append(dict(case=label, n=n, k=k, m=m, accumulate=accumulate, **r))
        emit(f"{label:30s} {r['density']:8.4f} {r['packed_s'] * 1e3:10.3f} {r['packed_spread']:6.1%} {r['byte_s'] * 1e3:10.3f} "
             f"{r['byte_spread']:6.1%} {r['ratio']:10.1f}x {r['of_peak']:7.1%} {r['output_density']:8.3f} {str(r['agree']):>5s}  "
             f"{r['kernel']} / {r['byte_kernel']}")
        torch.cuda.empty_cache()
    for label, n, with_byte in CLOSURES:
        if not wanted(label):
            continue
        r = closure(n, with_byte, reps)
        rows.append(dict(case=label, n=n, **r))
        byte = (f"{r['byte_s'] * 1e3:10.3f} {r['byte_spread']:6.1%} {r['ratio']:10.1f}x" if with_byte else f"{'-':>10s} {'-':>7s} {'-':>11s}")
        emit(f"{label:30s} {1.5 / n:8.6f} {r['packed_s'] * 1e3:10.3f} {r['packed_spread']:6.1%} {byte} {'-':>8s} "
             f"{r['closure_density']:8.3f} {str(r.get('agree', '-')):>5s}  {r['kernel']} / {r.get('byte_kernel', '-')}")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    sweep_main(__doc__, "bits_sweep_mi355x", cases)
