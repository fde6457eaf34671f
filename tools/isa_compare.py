#!/usr/bin/env python3
"""Are the gfx950 kernels of two source trees the same machine code?  CPU only: hipcc cross-compiles each unit of both trees
to assembly with the flags the product is built with (build.COMMON without --offload-compress, plus build.EXTRA[unit]).

    python tools/isa_compare.py OLD_TREE NEW_TREE [unit ...]        # default: the nine units whose kernels take a Form
    python tools/isa_compare.py --same-naming OLD_TREE NEW_TREE [unit ...]   # default: every .hip unit of NEW_TREE's csrc
    python tools/isa_compare.py --flag-added OLD_TREE NEW_TREE [unit ...]    # default: every .hip unit of OLD_TREE's csrc

Without --same-naming, OLD_TREE names a kernel's form in its symbol (`*_batched`, `*_batched_seeded`), NEW_TREE in a template argument
(`(mm::Form)N`; mfma_f32_batched_kernel: a trailing `bool SEED`).  Kernels are paired by (base name, form, the remaining
template arguments).  A pair is identical when the instruction streams are equal line for line -- comments, assembler
directives and blank lines dropped, local labels (.LBB<n>_<m>) renumbered in order of appearance -- and the .amdhsa_
resource lines are equal (registers, LDS, private segment, user SGPRs).  A differing pair's line also says whether the
instruction count, the opcode multiset (first token of each line) and the .amdhsa_ lines are equal; a pair with all three
equal is counted as "reordered" in its unit's line.  Only .amdhsa_kernarg_size of a Form::Single
kernel may differ: it gained the batch arguments it never loads.  Prints one line per unit; exit status 1 on any
difference, unpaired kernel or changed kernel count.

--same-naming: both trees name a kernel's form in a template argument (a host-side refactor, say).  Kernels are paired by
their whole demangled name and nothing may differ, .amdhsa_kernarg_size included.

--flag-added: --same-naming, where NEW_TREE gave some kernels one more trailing `bool` template parameter.  A NEW kernel
whose name is not OLD's pairs with the OLD kernel of that name without a trailing `, false`; the `true` instantiations are
new kernels, counted and not compared.  Every OLD kernel must be paired and identical.
"""
import concurrent.futures
import os
import re
import runpy
import subprocess
import sys

UNITS = ["mm_ordered.hip", "mm_valu_tile_fp.hip", "mm_valu_tile_fp_exact.hip", "mm_valu_tile_int_narrow.hip",
         "mm_valu_tile_int_wide.hip", "mm_mfma_f64.hip", "mm_mfma_f16.hip", "mm_mfma_i8.hip", "mm_mfma_f32.hip"]
FORMS = ("Single", "Batched", "Seeded")


def assembly(tree, unit):
    b = runpy.run_path(os.path.join(tree, "gemm_hls_amd", "build.py"))
    flags = [f for f in b["COMMON"] if f != "--offload-compress"] + b["EXTRA"].get(unit, [])
    src = os.path.join(tree, "gemm_hls_amd", "csrc", unit)
    r = subprocess.run([b["HIPCC"], *flags, "-S", "--cuda-device-only", src, "-o", "-"], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{src}: hipcc failed\n{r.stderr[-3000:]}")
    return r.stdout


def kernels(asm):
    """{symbol: (instruction stream, .amdhsa_ lines)} -- the parser of tests/test_isa_contract.py, labels kept"""
    out, name, body = {}, None, []
    for ln in asm.split("\n"):
        m = re.match(r"^(_Z\w+):\s*; @", ln)
        if m:
            name, body = m.group(1), []
            continue
        t = ln.split(";")[0].strip()
        if name is None or not t or ln.lstrip().startswith(";;#ASM"):
            continue
        if not t.startswith(".") or re.match(r"\.LBB\d+_\d+:", t):
            body.append(t)
        if t.startswith(".Lfunc_end"):                                  # not the first s_endpgm: a kernel may have several
            labels = {}
            for lab in re.findall(r"\.LBB\d+_\d+", "\n".join(body)):
                labels.setdefault(lab, f".L{len(labels)}")
            out[name] = ([re.sub(r"\.LBB\d+_\d+", lambda x: labels[x.group(0)], t) for t in body], None)
            name = None
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S):
        out[m.group(1)] = (out[m.group(1)][0], [t.strip() for t in m.group(2).strip().split("\n")])
    return out


def keyed(kerns, new, same_naming=False, known=None):
    """{(base name, form, other template arguments): symbol}; same_naming: {(demangled name, "", ""): symbol}, a name
    not in `known` (given) taken without its trailing `, false` template argument where that is in `known`"""
    # _Float16 (DF16_) is newer than some c++filt; a builtin type takes no substitution slot, so `Dh` (half) stands in
    names = subprocess.run(["c++filt"], input="\n".join(k.replace("DF16_", "Dh") for k in kerns), capture_output=True,
                           text=True, check=True).stdout.split("\n")
    out = {}
    for sym, d in zip(kerns, names):
        if same_naming:
            if known is not None and d not in known and d.replace(", false>(", ">(", 1) in known:
                d = d.replace(", false>(", ">(", 1)
            assert (d, "", "") not in out, d
            out[(d, "", "")] = sym
            continue
        m = re.match(r"(?:void )?(?:[\w:]|\(anonymous namespace\))*?(\w+)(?:<(.*)>)?\((?:[^()]|\(anonymous namespace\))*\)$", d)
        assert m, d
        base, args, form = m.group(1), m.group(2) or "", 0
        if not new:
            form = 2 if "_batched_seeded" in base else 1 if "_batched" in base else 0
            base = base.replace("_batched_seeded", "").replace("_batched", "")
        elif args.startswith("(mm::Form)"):
            form, args = int(args[10]), args[11:].lstrip(", ")
        elif "_batched" in base:                                        # <..., bool SEED>
            args, seed = args.rsplit(", ", 1)
            form, base = 2 if seed == "true" else 1, base.replace("_batched", "")
        key = (base, FORMS[form], args)
        assert key not in out, key
        out[key] = sym
    return out


def compare(old_tree, new_tree, unit, same_naming=False, flag_added=False):
    old, new = kernels(assembly(old_tree, unit)), kernels(assembly(new_tree, unit))
    ko = keyed(old, False, same_naming)
    kn = keyed(new, True, same_naming, {k[0] for k in ko} if flag_added else None)
    notes, same, reordered = [], 0, 0
    for key in sorted(ko.keys() & kn.keys()):
        (bo, ro), (bn, rn) = old[ko[key]], new[kn[key]]
        skip = ".amdhsa_kernarg_size" if key[1] == "Single" else "\0"
        ro, rn = [t for t in ro if not t.startswith(skip)], [t for t in rn if not t.startswith(skip)]
        diff = next((f"line {i}: {a!r} != {b!r}" for i, (a, b) in enumerate(zip(bo + ro, bn + rn)) if a != b),
                    None if (len(bo), len(ro)) == (len(bn), len(rn)) else f"{len(bo)} != {len(bn)} instructions")
        same += diff is None
        if diff:
            # a pair that differs only in scheduling and register naming: the same opcodes, as many of each, the same resources
            eq = (len(bo) == len(bn), sorted(t.split()[0] for t in bo) == sorted(t.split()[0] for t in bn), ro == rn)
            reordered += all(eq)
            notes.append(f"  differs: {key}: {diff} [instruction count {'=' if eq[0] else '!'}= opcode multiset "
                         f"{'=' if eq[1] else '!'}= .amdhsa_ {'=' if eq[2] else '!'}=]")
    notes += [f"  only in OLD: {k}" for k in sorted(ko.keys() - kn.keys())]
    added = sorted(kn.keys() - ko.keys())
    if not flag_added:
        notes += [f"  only in NEW: {k}" for k in added]
    paired = len(ko.keys() & kn.keys())
    line = f"{unit}: kernels {len(old)} -> {len(new)}, paired {paired}, identical {same}, differing {paired - same}"
    if paired - same:
        line += f" ({reordered} reordered: equal instruction count, opcode multiset and .amdhsa_ lines)"
    if flag_added:
        line += f", new {len(added)}"
    return "\n".join([line] + notes), not notes and (flag_added or len(old) == len(new))


def main():
    argv = [a for a in sys.argv[1:] if a not in ("--same-naming", "--flag-added")]
    flag_added = "--flag-added" in sys.argv[1:]
    same_naming = flag_added or "--same-naming" in sys.argv[1:]
    if len(argv) < 2:
        raise SystemExit(__doc__)
    every = sorted(f for f in os.listdir(os.path.join(argv[0 if flag_added else 1], "gemm_hls_amd", "csrc")) if f.endswith(".hip"))
    units = argv[2:] or (every if same_naming else UNITS)
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4) // 2 or 1) as ex:
        results = list(ex.map(lambda u: compare(argv[0], argv[1], u, same_naming, flag_added), units))
    for text, _ in results:
        print(text)
    return 0 if all(ok for _, ok in results) else 1


if __name__ == "__main__":
    sys.exit(main())
