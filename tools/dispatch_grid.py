#!/usr/bin/env python3
"""Every dispatch answer of a built tree over a fixed grid, one line each.  CPU only (no device is touched): diff the output
of two trees to see whether a host-side change moved any kernel choice or description.

    python tools/dispatch_grid.py [TREE] > answers.txt        # TREE: a built checkout (default: this one)

Per line: the knob setting, the configuration, the shape and batch, then mm_kernel_name, mm_kernel_name_batched,
mm_kernel_name_widen and every field of mm_kernel_info.  Knobs vary one at a time over their documented values
(include/mm_gemm.h) plus one value the library does not have.
"""
import os
import sys

tree = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
import gemm_hls_amd as g  # noqa: E402

INVALID = 99
KNOBS = [("f32_variant", [33, 8, 35, 64, 0, 3, INVALID]), ("f64_variant", [0, 1, 2, 3, 4, INVALID]),
         ("f16_variant", [200, 100, 11, 0, 4, 5, INVALID]), ("i8_variant", [200, 100, 10, 5, 0, INVALID])]
SHAPES = [(s, s, s) for s in (64, 200, 256, 512, 1024, 4096, 16384)] + [(256, k, 256) for k in (48, 96, 128, 256)]
OP_PAIRS = [("Multiply", "Add"), ("Add", "Min")]


def main():
    assert os.path.dirname(os.path.abspath(g.__file__)) == os.path.join(tree, "gemm_hls_amd"), g.__file__
    for knob, value in [(None, -1)] + [(k, v) for k, values in KNOBS for v in values]:
        for k, _ in KNOBS:
            g.set_tuning(k, value if k == knob else -1)
        for dtype in g.DTYPES:
            for mp, rd in OP_PAIRS:
                for transposed in (False, True):
                    for path in (g.PATH_AUTO, g.PATH_ORDERED, g.PATH_SPLIT):
                        cfg = g.make_config(dtype, mp, rd, path, transposed)
                        for n, kk, m in SHAPES:
                            i = g.kernel_info(cfg, n, kk, m)
                            info = " ".join(f"{f}={getattr(i, f)}" for f, _ in g.KernelInfo._fields_)
                            single = g.kernel_name(cfg, n, kk, m)
                            for batch in (1, 64):
                                print(f"{knob}={value} {dtype} {mp},{rd} {'KxN' if transposed else 'NxK'} path={path} "
                                      f"{n}x{kk}x{m} batch={batch}: {single} | {g.kernel_name_batched(cfg, n, kk, m, batch)} | "
                                      f"{g.kernel_name_widen(cfg, n, kk, m, batch)} | {info}")


if __name__ == "__main__":
    main()
