"""CPU tests of the strided-batched entry points (mm_gemm_batched_enqueue / _launch, mm_kernel_name_batched): the header,
the binding and EXPORTS agree, bad arguments are refused before any device is touched, the batched resolver names the
family each shape runs (never a kernel that needs workspace), and the batch_chunk knob round-trips."""
import ctypes
import os
import re

import pytest

import gemm_hls_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mm_gemm.h")).read()
BATCHED = ("mm_gemm_batched_enqueue", "mm_gemm_batched_launch", "mm_kernel_name_batched")


def test_batched_symbols_declared_exported_and_bound():
    for sym in BATCHED:
        assert re.search(rf"^(?:int|const char \*)\s*{sym}\(", HEADER, flags=re.M), sym
        assert sym in g.EXPORTS
        assert getattr(g.lib(), sym).argtypes is not None
    assert "batch_chunk" in HEADER and "MM_BATCH_CHUNK" in open(os.path.join(ROOT, "gemm_hls_amd", "csrc", "mm_common.h")).read()


def _enqueue(cfg, a=16, b=16, c=16, n=64, k=64, m=64, batch=4, sa=64 * 64, sb=64 * 64, sc=64 * 64):
    return g.lib().mm_gemm_batched_enqueue(None, ctypes.byref(cfg), a, b, c, n, k, m, batch, sa, sb, sc)


def _launch(cfg, a=16, b=16, c=16, n=64, k=64, m=64, batch=4, sa=64 * 64, sb=64 * 64, sc=64 * 64):
    return g.lib().mm_gemm_batched_launch(0, ctypes.byref(cfg), a, b, c, n, k, m, batch, sa, sb, sc, None)


@pytest.mark.parametrize("call", [_enqueue, _launch], ids=["enqueue", "launch"])
def test_batched_bad_arguments_refused_without_a_device(call):
    f32 = g.make_config("float")
    # overlapping outputs
    assert call(f32, sc=64 * 64 - 1) == 2
    assert "overlap" in g.lib().mm_last_error().decode()
    # a null pointer
    assert call(f32, b=0) == 2
    # K == 0
    assert call(f32, k=0) == 2
    # an unknown enum
    assert call(g.Config(99, 1, 0, 0, 0)) == 2
    assert call(g.Config(0, 1, 0, 7, 0)) == 2
    # element-misaligned strides on the fast path (float: 16 B = 4 elements)
    assert call(f32, sa=64 * 64 + 1) == 2
    assert "16-byte" in g.lib().mm_last_error().decode()
    # MM_PATH_SPLIT has no batched form
    assert call(g.make_config("float", path=g.PATH_SPLIT)) == 3


def test_batched_empty_calls_are_no_ops_without_a_device():
    f32 = g.make_config("float")
    assert _enqueue(f32, batch=0) == 0
    assert _enqueue(f32, n=0) == 0
    assert _enqueue(f32, m=0) == 0
    assert _enqueue(f32, batch=0, a=0, b=0, c=0) == 0
    assert _launch(f32, batch=0) == 0


@pytest.mark.parametrize("batch,sa,sb,sc", [(1, 64 * 64, 64 * 64, 0), (4, 0, 64 * 64, 64 * 64), (4, 64 * 64, 0, 64 * 64)],
                         ids=["one_element_stride_c_0", "broadcast_A", "broadcast_B"])
def test_batched_one_element_and_broadcast_strides_pass_the_argument_checks(batch, sa, sb, sc):
    # device -1 is refused only AFTER every argument check (no device is touched, nothing is launched): a call that got
    # that far was not refused as overlapping or misaligned
    rc = g.lib().mm_gemm_batched_launch(-1, ctypes.byref(g.make_config("float")), 16, 16, 16, 64, 64, 64, batch, sa, sb, sc,
                                        None)
    msg = g.lib().mm_last_error().decode()
    assert rc in (1, 2) and "overlap" not in msg and "aligned" not in msg, (rc, msg)


WORKSPACE_KERNELS = ("splitk", "streamk", "split_bf16")


@pytest.mark.parametrize("dtype,mp,rd,ta,shape,batch,want", [
    ("float", "Add", "Min", False, (128, 128, 128), 4096, "valu_tile"),
    ("float", "Multiply", "Add", False, (256, 256, 256), 1024, "mfma_f32_"),
    ("float", "Multiply", "Add", False, (1024, 1024, 1024), 1, "mfma_f32_"),     # split-K / 64 x 64 when single
    ("float", "Multiply", "Add", False, (2304, 2304, 2304), 1, "mfma_f32_"),     # stream-K when single
    ("float", "Multiply", "Add", True, (1024, 1024, 1024), 4, "mfma_f32_256x256x16"),   # K x N: direct kernel, no pre-pass
    ("half", "Multiply", "Add", False, (256, 256, 256), 64, "mfma_f16_256x256_pingpong_16x16x32"),
    ("half", "Multiply", "Add", False, (4096, 4096, 4096), 8, "mfma_f16_256x256_pingpong_16x16x32"),
    ("half", "Multiply", "Add", True, (512, 512, 8192), 2, "mfma_f16_256x256_pingpong_k32_KxN"),
    ("half", "Multiply", "Add", True, (132, 256, 136), 3, "ordered_wide_f16"),                # N % 8 != 0
    ("half", "Multiply", "Add", False, (256, 256, 260), 8, "ordered_wide_f16"),               # M % 8 != 0
    ("double", "Multiply", "Add", False, (256, 256, 256), 16, "mfma_f64_"),
    ("double", "Multiply", "Add", True, (256, 256, 256), 16, "mfma_f64_"),
    ("int8_t", "Multiply", "Add", True, (512, 512, 8192), 2, "mfma_i8_256x256_pingpong_k64_KxN"),
    ("uint8_t", "Multiply", "Add", False, (256, 256, 256), 8, "mfma_i8_"),
    ("uint8_t", "Multiply", "Add", False, (4096, 4096, 4096), 8, "mfma_i8_256x256_pingpong_16x16x64"),
    ("int", "Multiply", "Multiply", False, (64, 64, 64), 8, "ordered"),
    ("float", "Multiply", "Add", False, (30, 30, 30), 8, "ordered"),
], ids=lambda x: str(x))
def test_kernel_name_batched_names_a_workspace_free_family(dtype, mp, rd, ta, shape, batch, want):
    cfg = g.make_config(dtype, mp, rd, transposed_a=ta)
    name = g.kernel_name_batched(cfg, *shape, batch)
    assert name.startswith(want), name
    assert not any(w in name for w in WORKSPACE_KERNELS), name


def test_kernel_name_batched_ordered_and_split_paths():
    assert g.kernel_name_batched(g.make_config("float", "Add", "Min", g.PATH_ORDERED), 128, 128, 128, 8) == "ordered_tile"
    assert g.kernel_name_batched(g.make_config("float", "Add", "Min", g.PATH_ORDERED), 130, 130, 130, 8) == "ordered"
    assert g.kernel_name_batched(g.make_config("float", path=g.PATH_SPLIT), 128, 128, 128, 8) == "unsupported"
    assert g.kernel_name_batched(g.Config(99, 1, 0, 0, 0), 128, 128, 128, 8) == "invalid"


def test_kernel_name_batched_picks_the_tile_on_the_whole_batch():
    cfg = g.make_config("float")
    # one 256^3 element is 4 tiles of 128 x 128; a batch of 1024 fills rounds of the bigger tiles
    small, big = g.kernel_name_batched(cfg, 256, 256, 256, 1), g.kernel_name_batched(cfg, 256, 256, 256, 1024)
    assert small.startswith("mfma_f32_128x128x32") and big.startswith("mfma_f32_128x256x16"), (small, big)
    # the other matrix-core families pick their tiles the same way
    assert g.kernel_name_batched(g.make_config("half"), 128, 96, 256, 1).startswith("mfma_f16_64x256")
    assert g.kernel_name_batched(g.make_config("double"), 512, 512, 512, 1).startswith("mfma_f64_64x64")
    assert g.kernel_name_batched(g.make_config("double"), 512, 512, 512, 64).startswith("mfma_f64_256x128")


def test_batch_chunk_knob_round_trips():
    old = g.get_tuning("batch_chunk")
    try:
        g.set_tuning("batch_chunk", 3)
        assert g.get_tuning("batch_chunk") == 3
        g.set_tuning("batch_chunk", -1)
        assert g.get_tuning("batch_chunk") == -1
    finally:
        g.set_tuning("batch_chunk", old)
