"""The reference's OWN host programs -- /root/reference/host/RunHardware.cpp, test/TestSimulation.cpp and
src/PrintSpecifications.cpp, compiled UNMODIFIED from where they lie by oracle/build_ref_hosts.py against
include/compat (hlslib::ocl over include/mm_gemm.h) and this repository's libraries -- run on the MI355X.

This is the drop-in claim in its strongest form: not a re-written runner that prints the same lines, but
the reference's callers themselves, generating the seeded inputs, driving Context / MakeBuffer / CopyFromHost /
MakeKernel / ExecuteTask / CopyToHost (host/RunHardware.cpp:114-190) or calling MatrixMultiplicationKernel directly
(test/TestSimulation.cpp:61-92), and verifying the device's result with THEIR reference implementation and THEIR
tolerance rule (1e-3 relative for float / double, exact for integers and for half).  The binaries are built where
/root/reference exists (build()) into oracle/_ref/ref_hosts and travel with oracle/_ref; nothing here reads /root/reference at run time."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTS = os.path.join(ROOT, "oracle", "_ref", "ref_hosts")
STATIC = "float_static_528x512x560"
# the reference's benchmark parser (scripts/build_manager.py:601)
PERF = re.compile(r"([\d\.]+) seconds[^\d]+([\d\.]+) GOp/s")


def _exe(config, name):
    path = os.path.join(HOSTS, config, name)
    if not os.path.exists(path):
        pytest.skip(f"{os.path.relpath(path, ROOT)} not built (oracle/build_ref_hosts.py needs /root/reference)")
    return path


def _run(config, name, *args, env=None, timeout=900):
    full_env = dict(os.environ)
    full_env.pop("XCL_EMULATION_MODE", None)
    full_env.update(env or {})
    r = subprocess.run([_exe(config, name)] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout,
                       cwd=ROOT, env=full_env)
    if config.endswith("_blas") and r.returncode == 127 and "error while loading shared libraries" in r.stderr:
        # the *_blas builds link the image's CBLAS (/opt/conda/lib/libmkl_rt.so) dynamically: a box without it cannot start them
        pytest.skip(f"{config}: the BLAS library the build was linked against is not on this box: {r.stderr.strip()[-160:]}")
    return r


# ---- CPU: what can be said without a device -------------------------------------------------------------------------
def test_reference_hosts_fail_loudly_without_a_device_and_keep_their_argument_checks():
    """The reference's argv contract is the reference's code; the adapter's part is the error path: no device -> the
    Context throws, the reference's catch block prints it and returns 1 (host/RunHardware.cpp:192-196)."""
    r = _run("float", "RunHardware.exe", 513, 520, 528)
    assert r.returncode == 1 and "K (520) must be divisable by the memory width in K (16)." in r.stderr
    r = _run("float", "RunHardware.exe")
    assert r.returncode == 1 and "Usage: ./RunHardware.exe N K M" in r.stderr
    r = _run(STATIC, "RunHardware.exe", "hw", "on", "extra")
    assert r.returncode == 1 and "Usage: ./RunHardware.exe <mode [hw/hw_emu]>" in r.stderr
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        r = _run("float", "RunHardware.exe", 513, 528, 528, "hw", "on")
        assert r.returncode == 1 and 'Execution failed with error: "no usable device' in r.stderr and "no CPU fallback" in r.stderr


def test_reference_print_specifications_builds_against_the_compat_headers():
    """src/PrintSpecifications.cpp needs include/Memory.h's dataflow declarations (arrays of hlslib::Stream) to parse;
    its output is the reference's FPGA model, unchanged."""
    r = _run("float", "PrintSpecifications.exe", 16384, 16384, 16384)
    assert r.returncode == 0 and "Number of operations: 8796093022208" in r.stdout and "Memory tile size: 256x256" in r.stdout


# ---- GPU ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["hw", "hw_emu"])
def test_reference_run_hardware_verifies_its_ctest_shape(mode):
    """`RunHardware.exe 513 528 528 <mode> on`: the CTest shape of the default build (CMakeLists.txt:155-159).
    hw -> the fast path, hw_emu -> the k-ordered kernel (XCL_EMULATION_MODE, set by the reference itself)."""
    r = _run("float", "RunHardware.exe", 513, 528, 528, mode, "on")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for line in ("Initializing OpenCL context...", "Programming device...", "Copying memory to device...", "Creating kernel...",
                 "Executing kernel...", "Copying back result...", "Running reference implementation...", "Verifying result...",
                 "Successfully verified."):
        assert line in r.stdout, line
    assert PERF.search(r.stdout)


@pytest.mark.gpu
def test_reference_run_hardware_times_the_baseline_shape():
    """`RunHardware.exe 16384 16384 16384 hw off` (BASELINE configs[1]): the reference's own line, parsed with the
    reference's own regex, says what the MI355X kernel does."""
    r = _run("float", "RunHardware.exe", 16384, 16384, 16384, "hw", "off")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    mo = PERF.search(r.stdout)
    assert mo, r.stdout
    seconds, gops = float(mo.group(1)), float(mo.group(2))
    assert abs(gops - 1e-9 * 2 * 16384.0 ** 3 / seconds) / gops < 2e-2     # their arithmetic (float operation count), their print precision
    assert gops > 0.80 * 157.3e3, r.stdout                                  # north_star: >= 80 % of the fp32 MFMA peak
    assert "Successfully verified." not in r.stdout and "Copying back result" not in r.stdout


@pytest.mark.gpu
def test_reference_test_simulation_verifies_on_the_device():
    """test/TestSimulation.cpp calls MatrixMultiplicationKernel(aKernel.data(), bKernel.data(), cKernel.data(), N, K, M)
    with its DataPack arrays; bin/libmmkernel.so stands where the reference's `mmkernel` library stood."""
    r = _run("float", "TestSimulation.exe", 513, 528, 528)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Running simulation..." in r.stdout and "Matrix-matrix multiplication successfully verified." in r.stdout
    r = _run("float", "TestSimulation.exe", 513, 520, 528)
    assert r.returncode == 1 and "K must be divisable by memory width." in r.stderr


@pytest.mark.gpu
def test_reference_hosts_half_build_is_exact():
    """MM_DATA_TYPE=half (-DMM_HALF_PRECISION, CMakeLists.txt:110-112).  The reference compares half results EXACTLY
    (its `half` is not std::is_floating_point) with a Naive that accumulates in binary16: the k-ordered kernel matches it bit
    for bit (hw_emu; TestSimulation linked against the ordered kernel library).  `hw` runs the matrix-core kernel, which
    accumulates in fp32 and rounds once -- more accurate, hence not equal: timed, not verified (the reference-contract knob
    below is the way to have both)."""
    r = _run("half", "RunHardware.exe", 513, 544, 544, "hw_emu", "on")     # the half build's CTest shape: 64-byte bus = 32 elements
    assert r.returncode == 0 and "Successfully verified." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = _run("half", "TestSimulation.exe", 513, 544, 544)
    assert r.returncode == 0 and "successfully verified" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = _run("half", "RunHardware.exe", 8192, 8192, 8192, "hw", "off")
    # (above 1e6 GOp/s the reference's `std::cout << perf` prints 1.3e+06, which its own parser's [\d\.]+ cannot read:
    # a limit of the reference's print statement, left as it is -- this repository's runner prints fixed notation there)
    mo = re.search(r"performance of ([\d\.e\+]+) GOp/s", r.stdout)
    assert r.returncode == 0 and mo, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(mo.group(1)) > 500e3       # matrix cores, not the ordered kernel


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(513, 528, 528), (512, 528, 528)], ids=lambda s: "x".join(map(str, s)))
def test_reference_hosts_transposed_a_build(shape):
    """-DMM_TRANSPOSED_A (CMakeLists.txt:30,100-103): their generator's N*K draws ARE the K x N matrix, their Naive indexes
    a[k * N + n] (include/Utility.h:31-35); N = 513 is not a multiple of 4, so the generic family serves it."""
    r = _run("float_transposedA", "RunHardware.exe", *shape, "hw", "on")
    assert r.returncode == 0 and "Successfully verified." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = _run("float_transposedA", "TestSimulation.exe", *shape)
    assert r.returncode == 0 and "successfully verified" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_reference_hosts_static_size_build():
    """MM_DYNAMIC_SIZES=OFF (CMakeLists.txt:21-24): sizes from Config.h, `RunHardware.exe [mode] [verify]`, the 3-argument
    MakeKernel and the 3-pointer MatrixMultiplicationKernel (include/MatrixMultiplication.h:155-171)."""
    r = _run(STATIC, "RunHardware.exe", "hw", "on")
    assert r.returncode == 0 and "Successfully verified." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = _run(STATIC, "RunHardware.exe")
    assert r.returncode == 0 and "Successfully verified." in r.stdout
    r = _run(STATIC, "TestSimulation.exe")
    assert r.returncode == 0 and "successfully verified" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["float_Add_Min", "int", "double"])
def test_reference_run_hardware_other_build_configurations(config):
    """MM_MAP_OP / MM_REDUCE_OP / MM_DATA_TYPE choices of the reference's build (CMakeLists.txt:16-34) through the same
    unmodified host: min-plus on the VALU family, int32 exact, double on the fp64 matrix cores."""
    r = _run(config, "RunHardware.exe", 513, 528, 528, "hw", "on")
    assert r.returncode == 0 and "Successfully verified." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["environment", "build_flag"])
def test_reference_half_host_verifies_under_hw_with_the_reference_half_contract(how):
    """VERDICT r5 next 1.  The reference compares half results EXACTLY with a Naive that accumulates in binary16
    (test/TestSimulation.cpp:80-85, host/RunHardware.cpp:214-218, include/Utility.h:29-37) == what kernel/Compute.cpp:129-133
    computes.  Under MM_HALF_CONTRACT=reference (or a build of the compat adapter with -DMM_HALF_CONTRACT_REFERENCE) `hw` --
    MM_PATH_AUTO -- keeps that arithmetic on the register-tiled k-ordered kernel: the reference's own unmodified half host is
    timed AND verified on the same kernel; without the knob `hw` is the matrix cores' f32 accumulation and its exact check fails."""
    config, env = ("half", {"MM_HALF_CONTRACT": "reference"}) if how == "environment" else ("half_reference_contract", {})
    r = _run(config, "RunHardware.exe", 513, 544, 544, "hw", "on", env=env)      # the half build's CTest shape
    assert r.returncode == 0 and "Successfully verified." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = _run(config, "RunHardware.exe", 512, 2048, 512, "hw", "on", env=env)     # K = 2048 on [1,10): sums pass 65504 -> inf == inf
    assert r.returncode == 0 and "Successfully verified." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    if how == "environment":
        r = _run("half", "RunHardware.exe", 513, 544, 544, "hw", "on")
        assert r.returncode == 1 and "Mismatch at" in r.stderr, "default half contract (f32 accumulate) is not the reference's bits"
    # and it is a fast kernel, not the 64 x 64 anchor (27 TOp/s): 8192^3 measured 74.4 TOp/s (v_pk_mul_f16 + v_pk_add_f16 issue limit:
    # 78.6); the bar here only tells the two kernels apart on any box
    r = _run(config, "RunHardware.exe", 8192, 8192, 8192, "hw", "off", env=env)
    mo = PERF.search(r.stdout)
    assert r.returncode == 0 and mo, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(mo.group(2)) > 40e3, r.stdout


@pytest.mark.gpu
def test_reference_hw_emu_float_8192_takes_seconds():
    """`hw_emu` (XCL_EMULATION_MODE, set by the reference's host itself) -> MM_PATH_ORDERED -> the k-ordered TILE kernel where
    it serves: float 8192^3 in the unfused k-ascending contract in 18 ms (60 TOp/s; the 64 x 64 anchor kernel: 49)."""
    r = _run("float", "RunHardware.exe", 8192, 8192, 8192, "hw_emu", "off")
    mo = PERF.search(r.stdout)
    assert r.returncode == 0 and mo, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(mo.group(1)) < 0.08 and float(mo.group(2)) > 25e3, r.stdout


# ---- the reference's hosts WITH the reference's BLAS oracle (-DMM_HAS_BLAS, CMakeLists.txt:75-85) ---------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("config", ["float_blas", "double_blas"])
def test_reference_hosts_blas_build_ctest_shape(config):
    """include/Utility.h:76-103: with MM_HAS_BLAS the reference's ReferenceImplementation is cblas_sgemm / cblas_dgemm
    (row-major, lda = size_k) instead of the Naive fall-back; both its hosts verify the device against it."""
    r = _run(config, "RunHardware.exe", 513, 528, 528, "hw", "on")
    assert r.returncode == 0 and "Running BLAS..." in r.stdout and "Successfully verified." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "WARNING: BLAS not available" not in r.stdout
    r = _run(config, "TestSimulation.exe", 513, 528, 528)
    assert r.returncode == 0 and "Running BLAS..." in r.stdout and "successfully verified" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("config,floor", [("float_blas", 0.80 * 157.3e3), ("double_blas", 0.80 * 78.6e3)])
def test_reference_run_hardware_verifies_the_baseline_shape_against_blas(config, floor):
    """BASELINE C2 / C4 through the reference's OWN runner, end to end: `RunHardware.exe 16384 16384 16384 hw on` -- its seeded
    generator, its copies, the MI355X kernel timed by its ExecuteTask(), its BLAS reference, its comparison of all 2^28
    elements (north_star: "matching the repo's TestSimulation/BLAS reference")."""
    r = _run(config, "RunHardware.exe", 16384, 16384, 16384, "hw", "on", timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Running BLAS..." in r.stdout and "Successfully verified." in r.stdout, r.stdout[-2000:]
    mo = re.search(r"performance of ([\d\.e\+]+) GOp/s", r.stdout)
    assert mo and float(mo.group(1)) > floor, r.stdout
    out_dir = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out_dir):     # kept as evidence next to the GPU test log
        with open(os.path.join(out_dir, f"reference_runhardware_{config}_16384_hw_on.log"), "w") as f:
            f.write(r.stdout + r.stderr)


def test_reference_hosts_no_transposed_blas_build():
    """The one combination that is NOT built: -DMM_TRANSPOSED_A with -DMM_HAS_BLAS.  The reference's BLAS call passes
    lda = size_k with CblasTrans (include/Utility.h:86-87,99-100), which is the leading dimension of a K x N matrix only when
    N == K -- for any other shape its oracle reads the wrong elements.  Kept as a written-down skip, not a build."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import build_ref_hosts
    assert not any(name.endswith("_blas") and cfg[3] for name, cfg in build_ref_hosts.CONFIGS.items())


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["float", "float_blas"])
def test_reference_test_simulation_at_baseline_c1_size(config):
    """BASELINE configs[0] is `float 1024x1024x1024 via ... TestSimulation`: the reference's own test/TestSimulation.cpp, unmodified,
    at that size, with MatrixMultiplicationKernel bound to the MI355X kernel library instead of the hlslib simulation -- verified by
    its own ReferenceImplementation (the Naive fall-back in the plain build, cblas_sgemm in the -DMM_HAS_BLAS build) and its own rule."""
    r = _run(config, "TestSimulation.exe", 1024, 1024, 1024)
    assert r.returncode == 0 and "Matrix-matrix multiplication successfully verified." in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert ("Running BLAS..." in r.stdout) == (config == "float_blas")
