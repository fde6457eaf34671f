#!/usr/bin/env python3
"""Bit-packed product over GF(2) (mm_bits_gf2_enqueue: C = XOR_k (A AND B), packed in and packed out): its two kernels against
each other and against two yardsticks the library already had, on the same operands, in the same process, in interleaved
rounds.  Whole calls between HIP events, one warm-up, best of N, and the spread of the N ((max - min) / min) next to every
figure.

    python tools/bits_gf2_sweep.py [--reps 5] [--out-dir profiles] [--cases a,b]

Writes <out-dir>/bits_gf2_sweep_mi355x.txt and .json.  Forms per case: "tile" and "plain" are bits_gf2_tile and
bits_gf2_plain forced by the knob bits_gf2_variant; "or" is the Boolean product bits_matmul / bits_addmm_ on the same operands
(at density 0.5 nothing of it can be skipped); "route" is what a user did before this call: unpack_bits of both operands,
matmul_wide(int8_t) to int32 on the matrix cores, & 1, pack_bits (and ^ into C when accumulating), all inside the timed
region.  Operands have density 0.5; the row strides are the rows' own word counts (multiples of 4 here, so both kernels
serve).  Every packed result is compared with the route's.  "lds bound" = N K / 4 ceil(M / 4096) ds_read_b64 wave instructions (64 lanes x 64 columns each)
at 2 LDS cycles each over 256 CUs at the clock mm_kernel_info reports (2.4 GHz); "of lds" is that bound over the tile kernel's time.
"bytes" is device memory the form needs beyond the packed operands and result: nothing for the packed call, the two unpacked
operands and the int32 product for the route (its & 1 and pack temporaries not counted)."""
from _bits_sweep import _interleaved, _random_bits, g, sweep_main

# (label, n, k, m, accumulate)
PRODUCTS = [("gf2_4096_cubed", 4096, 4096, 4096, False), ("gf2_16384_cubed", 16384, 16384, 16384, False),
            ("rank64_accumulate_16384", 16384, 64, 16384, True)]
PRODUCTS += [(f"rule_{n}_k4096", n, 4096, n, False) for n in (128, 256, 512, 1024, 2048, 8192, 16384)]


def _with_variant(v, fn):
    def run():
        g.set_tuning("bits_gf2_variant", v)
        try:
            fn()
        finally:
            g.set_tuning("bits_gf2_variant", -1)
    return run


def product(n, k, m, accumulate, reps):
    import torch
    _, ap = _random_bits(n, k, 0.5, 1)
    _, bp = _random_bits(k, m, 0.5, 2)
    mw = g.bits_words(m)
    new = lambda: torch.empty((n, mw), dtype=torch.int32, device="cuda:0")
    c_gf2, c_or, c_route = new(), new(), new()
    wide = torch.empty((n, m), dtype=torch.int32, device="cuda:0")
    if accumulate:
        seed = _random_bits(n, m, 0.5, 3)[1]
        for c in (c_gf2, c_or, c_route):
            c.copy_(seed)

    def route(dst, acc):
        x = g.unpack_bits(ap, k, dtype=torch.uint8).view(torch.int8)
        y = g.unpack_bits(bp, m, dtype=torch.uint8).view(torch.int8)
        g.matmul_wide(x, y, "int8_t", out=wide)
        p = g.pack_bits((wide & 1).to(torch.uint8))
        if acc:
            dst.bitwise_xor_(p)
        else:
            dst.copy_(p)

    if accumulate:   # C ^= A B toggles between two values, C |= A B only gains bits: every round does the same work
        packed, boolean = (lambda: g.bits_addmm_gf2_(c_gf2, ap, bp, k, m)), (lambda: g.bits_addmm_(c_or, ap, bp, k, m))
    else:
        packed, boolean = (lambda: g.bits_matmul_gf2(ap, bp, k, m, out=c_gf2)), (lambda: g.bits_matmul(ap, bp, k, m, out=c_or))
    forms = {"tile": _with_variant(1, packed), "plain": _with_variant(0, packed), "or": boolean,
             "route": lambda: route(c_route, accumulate)}
    t = _interleaved(forms, reps)
    route(c_route, False)   # every kernel's product, not accumulated, against the route's
    agree = {}
    for name, v in (("tile", 1), ("plain", 0)):
        _with_variant(v, lambda: g.bits_matmul_gf2(ap, bp, k, m, out=c_gf2))()
        agree[name] = bool(torch.equal(c_gf2, c_route))
        c_gf2.zero_()
    clock = g.kernel_info(g.make_config("int8_t"), n, k, m).max_clock_mhz * 1e6
    lds = n * (k / 4.0) * ((m + 4095) // 4096) * 2.0 / (256 * clock)
    out = dict(lds_bound_s=lds, of_lds=lds / t["tile"][0], clock_hz=clock, agree=agree["tile"] and agree["plain"],
               plain_over_tile=t["plain"][0] / t["tile"][0], or_over_tile=t["or"][0] / t["tile"][0],
               route_over_tile=t["route"][0] / t["tile"][0], kernel=g.kernel_name_bits_gf2(n, k, m),
               or_kernel=g.kernel_name_bits_gemm(n, k, m), int8_kernel=g.kernel_name_widen(g.make_config("int8_t"), n, k, m, 1),
               packed_bytes=4 * (n * g.bits_words(k) + k * mw + n * mw), route_extra_bytes=n * k + k * m + 4 * n * m)
    for name, (best_s, spread) in t.items():
        out[name + "_s"], out[name + "_spread"] = best_s, spread
    return out


def cases(reps, wanted, emit, rows):
    import torch
    emit(f"best of {reps}, interleaved; spread = (max - min) / min of the {reps}; density 0.5; ms")
    emit(f"{'case':26s} {'tile':>9s} {'spread':>7s} {'plain':>9s} {'spread':>7s} {'or':>9s} {'spread':>7s} {'route':>9s} {'spread':>7s} "
         f"{'plain/tile':>10s} {'route/tile':>10s} {'lds bd':>8s} {'of lds':>7s} {'packed MiB':>10s} {'route +MiB':>10s} {'same':>5s}  "
         f"rule's kernel / or kernel / int8 kernel")
    for label, n, k, m, accumulate in PRODUCTS:
        if not wanted(label):
            continue
        r = product(n, k, m, accumulate, reps)
        rows.append(dict(case=label, n=n, k=k, m=m, accumulate=accumulate, **r))
        emit(f"{label:26s} " + " ".join(f"{r[f + '_s'] * 1e3:9.3f} {r[f + '_spread']:6.1%}" for f in ("tile", "plain", "or", "route")) +
             f" {r['plain_over_tile']:9.2f}x {r['route_over_tile']:9.2f}x {r['lds_bound_s'] * 1e3:8.3f} {r['of_lds']:6.1%} "
             f"{r['packed_bytes'] / 2**20:10.1f} {r['route_extra_bytes'] / 2**20:10.1f} {str(r['agree']):>5s}  "
             f"{r['kernel']} / {r['or_kernel']} / {r['int8_kernel']}")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    sweep_main(__doc__, "bits_gf2_sweep_mi355x", cases)
