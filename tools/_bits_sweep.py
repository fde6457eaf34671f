"""What tools/bits_sweep.py and tools/bits_count_sweep.py share: HIP-event timing in interleaved rounds, random packed
operands, and the command line that writes <out-dir>/<stem>.txt and .json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemm_hls_amd as g  # noqa: E402

PEAK_LANE_OPS = 256 * 128 * 2.4e9


def _timed(fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e-3


def _interleaved(forms, reps):
    """{name: (best, spread)} of callables timed in interleaved rounds after one warm-up each."""
    for fn in forms.values():
        fn()
    times = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            times[name].append(_timed(fn))
    return {name: (min(t), (max(t) - min(t)) / min(t)) for name, t in times.items()}


def _up4(x):
    return (x + 3) // 4 * 4


def _random_bits(rows, cols, p, seed):
    """(bytes or None, packed) of a rows x cols Boolean matrix of density p, drawn on the device 4096 rows at a time."""
    import torch
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    packed = torch.empty((rows, g.bits_words(cols)), dtype=torch.int32, device="cuda:0")
    keep = rows * cols <= 1 << 28
    byte = torch.empty((rows, cols), dtype=torch.uint8, device="cuda:0") if keep else None
    for r0 in range(0, rows, 4096):
        r1 = min(rows, r0 + 4096)
        x = (torch.rand((r1 - r0, cols), device="cuda:0", generator=gen) < p).to(torch.uint8)
        packed[r0:r1] = g.pack_bits(x)
        if keep:
            byte[r0:r1] = x
    return byte, packed


def _random_packed(batch, rows, cols, seed):
    """(batch, rows, words) packed bits of density 0.5 inside a tensor whose rows are a multiple of 4 words apart; the
    padding bits are random too."""
    import torch
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    w = g.bits_words(cols)
    full = torch.randint(-(1 << 31), 1 << 31, (batch, rows, _up4(w)), dtype=torch.int64, device="cuda:0", generator=gen).to(torch.int32)
    return full[:, :, :w]


def sweep_main(doc, stem, cases):
    """The command line of a sweep: cases(reps, wanted, emit, rows) prints its lines through emit(line) and appends a dict per
    case to rows, for the cases whose label wanted(label) accepts; both go to <out-dir>/<stem>.txt and .json."""
    ap = argparse.ArgumentParser(description=doc.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--cases", default="", help="comma-separated labels (default: all)")
    args = ap.parse_args()
    import torch
    want = set(args.cases.split(",")) if args.cases else None
    rows, lines = [], []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    cases(args.reps, lambda label: not want or label in want, emit, rows)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, stem + ".txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(args.out_dir, stem + ".json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}, f, indent=1)
