#!/usr/bin/env python3
"""Log-semiring product (mm_gemm_logsumexp_*): the hybrid (prepass, fp32 / fp64 matrix-core product, epilogue, fallback)
and the exact VALU kernel, next to the plain (Multiply, Add) GEMM of the same shape (mm_gemm_launch) and torch's shifted
log(exp(A - a_max) @ exp(B - b_max)) pipeline (fast, not robust); the all-fallback cross-check (lse_variant = 2); and an
HMM forward pass (64 sequences, 512 states, T = 50) against the same torch pipeline.  HIP events around each form, one
warm-up, best of --reps with the forms of a case alternating; uniform [-4, 4] data.

    python tools/logsumexp_sweep.py [--reps 5] [--out-dir profiles] [--only hybrid_f32_8192]

Writes <out-dir>/logsumexp_sweep_mi355x.txt and .json (not with --only).  TOp/s counts 2 N K M.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemm_hls_amd as g  # noqa: E402


def _ms(fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def _shifted(a, b):
    import torch
    am, bm = a.max(dim=1, keepdim=True).values, b.max(dim=0, keepdim=True).values
    return torch.log(torch.exp(a - am) @ torch.exp(b - bm)) + am + bm


def _variant(v):
    return lambda: g.set_tuning("lse_variant", v)


def case(dtype, n, reps, forms):
    import torch
    tdt = g.torch_dtype(dtype)
    gen = torch.Generator(device="cuda").manual_seed(1)
    a = (torch.rand((n, n), generator=gen, device="cuda", dtype=torch.float32) * 8 - 4).to(tdt)
    b = (torch.rand((n, n), generator=gen, device="cuda", dtype=torch.float32) * 8 - 4).to(tdt)
    c = torch.empty((n, n), dtype=tdt, device="cuda")
    gemm_cfg = g.make_config("float" if dtype == "half" else dtype)
    fns = {
        "hybrid": (_variant(-1), lambda: g.matmul_logsumexp(a, b, dtype, out=c)),
        "exact": (_variant(0), lambda: g.matmul_logsumexp(a, b, dtype, out=c)),
        "all_fallback": (_variant(2), lambda: g.matmul_logsumexp(a, b, dtype, out=c)),
        "gemm": (_variant(-1), None),
        "torch_shifted": (_variant(-1), lambda: _shifted(a, b)),
    }
    if "gemm" in forms:
        af, bf = a.float(), b.float()
        cf = torch.empty((n, n), dtype=torch.float32 if dtype != "double" else torch.float64, device="cuda")
        ad, bd = (af, bf) if dtype != "double" else (a, b)
        fns["gemm"] = (_variant(-1), lambda: g.matmul(ad, bd, "float" if dtype != "double" else "double", out=cf))
        del gemm_cfg
    best = {f: float("inf") for f in forms}
    for f in forms:   # warm-up
        fns[f][0]()
        fns[f][1]()
    torch.cuda.synchronize()
    for _ in range(reps):
        for f in forms:
            fns[f][0]()
            best[f] = min(best[f], _ms(fns[f][1]))
    g.set_tuning("lse_variant", -1)
    ops = 2.0 * n ** 3
    return {f: {"ms": round(best[f], 4), "tops": round(ops / best[f] / 1e9, 2)} for f in forms}


def hmm(reps):
    import torch
    seqs, states, steps = 64, 512, 50
    gen = torch.Generator(device="cuda").manual_seed(2)
    lt = torch.log_softmax(torch.randn((states, states), generator=gen, device="cuda"), dim=1)
    em = torch.log_softmax(torch.randn((seqs, steps, states), generator=gen, device="cuda"), dim=2)
    alpha0 = em[:, 0].contiguous()

    def ours():
        al = alpha0
        for t in range(1, steps):
            al = g.matmul_logsumexp(al, lt) + em[:, t]
        return al

    def shifted():
        al = alpha0
        for t in range(1, steps):
            al = _shifted(al, lt) + em[:, t]
        return al
    best = {"hybrid": float("inf"), "torch_shifted": float("inf")}
    ours(), shifted()
    torch.cuda.synchronize()
    for _ in range(reps):
        best["hybrid"] = min(best["hybrid"], _ms(ours))
        best["torch_shifted"] = min(best["torch_shifted"], _ms(shifted))
    return {f: {"ms": round(v, 4)} for f, v in best.items()}


CASES = [   # (label, dtype, n, forms)
    ("f32_4096", "float", 4096, ["hybrid", "exact", "gemm", "torch_shifted", "all_fallback"]),
    ("f32_8192", "float", 8192, ["hybrid", "exact", "gemm", "torch_shifted", "all_fallback"]),
    ("f16_4096", "half", 4096, ["hybrid", "exact", "torch_shifted"]),
    ("f16_8192", "half", 8192, ["hybrid", "exact", "torch_shifted"]),
    ("f64_4096", "double", 4096, ["hybrid", "exact", "gemm", "torch_shifted"]),
    ("f64_8192", "double", 8192, ["hybrid", "exact", "gemm"]),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--only", default=None, help="one form of one case, e.g. hybrid_f32_8192 (for rocprofv3)")
    args = ap.parse_args()
    if args.only:
        form, label = args.only.split("_", 1)
        for lab, dt, n, _ in CASES:
            if lab == label:
                print(json.dumps(case(dt, n, args.reps, [form])))
        return
    res = {}
    lines = ["# logsumexp sweep (MI355X, best of %d, uniform [-4, 4]); TOp/s = 2 N K M / time" % args.reps]
    for label, dt, n, forms in CASES:
        r = case(dt, n, args.reps, forms)
        res[label] = r
        line = f"{label:10s} " + "  ".join(f"{f} {v['ms']:.3f} ms ({v['tops']:.1f} TOp/s)" for f, v in r.items())
        print(line, flush=True)
        lines.append(line)
    res["hmm_forward_64x512_T50"] = hmm(args.reps)
    line = "hmm_forward_64x512_T50 " + "  ".join(f"{f} {v['ms']:.3f} ms" for f, v in res["hmm_forward_64x512_T50"].items())
    print(line, flush=True)
    lines.append(line)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "logsumexp_sweep_mi355x.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out_dir, "logsumexp_sweep_mi355x.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
