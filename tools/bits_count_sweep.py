#!/usr/bin/env python3
"""Packed counting products (mm_bits_count_enqueue: popcount AND / XOR to int32, A x B^T) and the packed transpose against
what a user of this library did before them: unpack both operands to bytes, materialise a transpose of the second, and call
matmul_wide(..., "int8_t") on the matrix cores.  Same logical shape, same process, interleaved rounds; HIP events around each
form, one warm-up, best of N, and the spread of the N ((max - min) / min) next to every figure.

    python tools/bits_count_sweep.py [--reps 5] [--out-dir profiles] [--cases a,b]

Writes <out-dir>/bits_count_sweep_mi355x.txt and .json.  Forms per case: "tile" and "plain" are the two kernels forced by the
knob bits_count_variant (operands with row strides that are multiples of 4 words / elements, so that both serve); "int8" is
the byte product alone on operands unpacked beforehand, "route" the same with both unpacks and the transpose inside the timed
region.  Bounds: "valu" = 2 lane-operations (one AND / XOR, one population count) per output and 32 k against 256 CUs x 128
lanes x 2.4 GHz; "store" = the 4 N M bytes of C against 8 TB/s.  "of bound" is the larger of the two bounds over the best
packed time.  Every packed result is compared with the byte route's (XOR through pop(a) + pop(bt) - 2 and)."""
from _bits_sweep import PEAK_LANE_OPS, _interleaved, _random_packed, _up4, g, sweep_main

HBM_BYTES_PER_S = 8e12

# (label, batch, n, k, m, op)
PRODUCTS = [(f"count_16384_k{k}_{op.lower()}", 1, 16384, k, 16384, op) for k in (64, 256, 1024, 16384) for op in ("And", "Xor")]
PRODUCTS += [("count_4096_cubed_and", 1, 4096, 4096, 4096, "And")]
PRODUCTS += [(f"rule_{n}_k1024_and", 1, n, 1024, n, "And") for n in (1024, 2048, 4096)]      # 64, 256, 1024 tiles of 128 x 128
PRODUCTS += [("batch16_1024_k1024_xor", 16, 1024, 1024, 1024, "Xor")]
TRANSPOSES = [("transpose_16384", 16384, 16384)]


def _with_variant(v, fn):
    def run():
        g.set_tuning("bits_count_variant", v)
        try:
            fn()
        finally:
            g.set_tuning("bits_count_variant", -1)
    return run


def product(batch, n, k, m, op, reps):
    import torch
    ap, btp = _random_packed(batch, n, k, 1), _random_packed(batch, m, k, 2)
    c = torch.empty((batch, n, _up4(m)), dtype=torch.int32, device="cuda:0")[:, :, :m]
    ref = torch.empty((batch, n, m), dtype=torch.int32, device="cuda:0")
    a8 = g.unpack_bits(ap, k, dtype=torch.uint8).view(torch.int8)
    b8 = g.unpack_bits(btp, k, dtype=torch.uint8).view(torch.int8).mT.contiguous()

    def route():
        x = g.unpack_bits(ap, k, dtype=torch.uint8).view(torch.int8)
        y = g.unpack_bits(btp, k, dtype=torch.uint8).view(torch.int8).mT.contiguous()
        g.matmul_wide(x, y, "int8_t", out=ref)
    forms = {"tile": _with_variant(1, lambda: g.bits_matmul_count(ap, btp, k, op, out=c)),
             "plain": _with_variant(0, lambda: g.bits_matmul_count(ap, btp, k, op, out=c)),
             "int8": lambda: g.matmul_wide(a8, b8, "int8_t", out=ref),
             "route": route}
    t = _interleaved(forms, reps)
    want = ref
    if op == "Xor":
        pa, pb = a8.sum(-1, dtype=torch.int32), b8.sum(-2, dtype=torch.int32)
        want = pa[:, :, None] + pb[:, None, :] - 2 * ref
    agree = {}
    for name, v in (("tile", 1), ("plain", 0)):
        c.zero_()
        _with_variant(v, lambda: g.bits_matmul_count(ap, btp, k, op, out=c))()
        agree[name] = bool(torch.equal(c, want))
    valu = 2.0 * batch * n * m * g.bits_words(k) / PEAK_LANE_OPS
    store = 4.0 * batch * n * m / HBM_BYTES_PER_S
    best = min(t["tile"][0], t["plain"][0])
    out = dict(valu_bound_s=valu, store_bound_s=store, of_bound=max(valu, store) / best, of_valu=valu / best, of_store=store / best,
               int8_over_packed=t["int8"][0] / best, route_over_packed=t["route"][0] / best, agree=agree["tile"] and agree["plain"],
               kernel=g.kernel_name_bits_count(n, k, m, ap.stride(-2), btp.stride(-2), c.stride(-2), batch),
               int8_kernel=g.kernel_name_widen(g.make_config("int8_t"), n, k, m, batch),
               packed_operand_bytes=4 * batch * (n + m) * g.bits_words(k), byte_operand_bytes=batch * (n + m) * k)
    for name, (best_s, spread) in t.items():
        out[name + "_s"], out[name + "_spread"] = best_s, spread
    return out


def transposed(rows, cols, reps):
    import torch
    p = _random_packed(1, rows, cols, 3)[0]
    out = torch.empty((cols, g.bits_words(rows)), dtype=torch.int32, device="cuda:0")
    t = _interleaved({"packed": lambda: g.transpose_bits(p, cols, out=out),
                      "route": lambda: g.pack_bits(g.unpack_bits(p, cols, dtype=torch.uint8).mT)}, reps)
    agree = bool(torch.equal(out, g.pack_bits(g.unpack_bits(p, cols, dtype=torch.uint8).mT)))
    moved = 4.0 * (rows * g.bits_words(cols) + cols * g.bits_words(rows))
    return dict(packed_s=t["packed"][0], packed_spread=t["packed"][1], route_s=t["route"][0], route_spread=t["route"][1],
                bytes_per_s=moved / t["packed"][0], agree=agree)


def cases(reps, wanted, emit, rows):
    import torch
    emit(f"best of {reps}, interleaved; spread = (max - min) / min of the {reps}; density 0.5; ms")
    emit(f"{'case':28s} {'tile':>9s} {'spread':>7s} {'plain':>9s} {'spread':>7s} {'int8':>9s} {'spread':>7s} {'route':>9s} {'spread':>7s} "
         f"{'valu bd':>8s} {'store bd':>8s} {'of bound':>8s} {'int8/pk':>8s} {'route/pk':>8s} {'same':>5s}  rule's kernel / int8 kernel")
    for label, batch, n, k, m, op in PRODUCTS:
        if not wanted(label):
            continue
        r = product(batch, n, k, m, op, reps)
        rows.append(dict(case=label, batch=batch, n=n, k=k, m=m, op=op, **r))
        emit(f"{label:28s} " + " ".join(f"{r[f + '_s'] * 1e3:9.3f} {r[f + '_spread']:6.1%}" for f in ("tile", "plain", "int8", "route")) +
             f" {r['valu_bound_s'] * 1e3:8.3f} {r['store_bound_s'] * 1e3:8.3f} {r['of_bound']:7.1%} {r['int8_over_packed']:7.2f}x "
             f"{r['route_over_packed']:7.2f}x {str(r['agree']):>5s}  {r['kernel']} / {r['int8_kernel']}")
        torch.cuda.empty_cache()
    for label, nrows, ncols in TRANSPOSES:
        if not wanted(label):
            continue
        r = transposed(nrows, ncols, reps)
        rows.append(dict(case=label, rows=nrows, cols=ncols, **r))
        emit(f"{label:28s} packed {r['packed_s'] * 1e3:.3f} ms ({r['packed_spread']:.1%}), {r['bytes_per_s'] / 1e12:.3f} TB/s read + written; "
             f"unpack + transposed pack {r['route_s'] * 1e3:.3f} ms ({r['route_spread']:.1%}); same {r['agree']}")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    sweep_main(__doc__, "bits_count_sweep_mi355x", cases)
