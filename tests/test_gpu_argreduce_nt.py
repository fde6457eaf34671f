"""GPU tests of argmin / argmax over an M x K B (mm_gemm_argreduce_nt_*, matmul_argreduce_nt / addmm_argreduce_nt_).  The
oracle is the contract's loop in numpy -- test_gpu_argreduce.oracle applied to bt.T:
    acc = seed or identity; idx = seed index or -1
    for k ascending: s = Map(a[i,k], bt[j,k]); if (Min: s < acc / Max: acc < s): acc = s; idx = index_base + k
and, beside it, the row-major call on a materialised transpose, which must agree bit for bit."""
import ctypes
import zlib

import numpy as np
import pytest

import _semiring_ref as sr
import gemm_hls_amd as g
import test_gpu_argreduce as ar

pytestmark = pytest.mark.gpu

GUARD = ar.GUARD
TILED, PLAIN = (200, 68, 132), (67, 37, 61)   # 68 = 4 slabs of 16 + a last slab of 4; 200 and 132 leave ragged tile edges
EDGE = (65, 17, 67)   # the 64 x 64 kernel: two tiles each way, a one-line last tile, a one-k last slab


def launch(cfg, a, b, n, k, m, batch=1, sa=0, sb=0, sc=None, c0=None, i0=None, index_base=0, a_offset=0, nt=True):
    """The blocking launch on host arrays, C and I inside guarded buffers (checked); returns (C flat, I flat).  nt: b is
    M x K per element and the A x B^T call runs, else the row-major call on b as it is.  a_offset moves A's base by that
    many elements (a pointer that is not 16-byte aligned)."""
    t = a.dtype
    sc = n * m if sc is None else sc
    size = (batch - 1) * sc + n * m
    c = np.zeros(size, dtype=t) if c0 is None else np.asarray(c0, dtype=t).reshape(-1)
    i = np.full(size, 7, dtype=np.int32) if i0 is None else np.asarray(i0, dtype=np.int32).reshape(-1)
    cbuf, cpat = ar._guarded(c)
    ibuf, ipat = ar._guarded(i)
    da = ar._dev(np.concatenate([np.zeros(a_offset, dtype=t), a.reshape(-1)]))
    db, dc, di = ar._dev(b), ar._dev(cbuf), ar._dev(ibuf)
    fn = g.lib().mm_gemm_argreduce_nt_launch if nt else g.lib().mm_gemm_argreduce_launch
    rc = fn(0, ctypes.byref(cfg), da.data_ptr() + a_offset * t.itemsize, db.data_ptr(), dc.data_ptr() + GUARD * t.itemsize,
            di.data_ptr() + GUARD * 4, n, k, m, batch, sa, sb, sc, index_base, int(c0 is not None), None)
    assert rc == 0, (rc, g.lib().mm_last_error().decode())
    cout, iout = dc.cpu().numpy().view(t), di.cpu().numpy().view(np.int32)
    for out, pat in ((cout, cpat), (iout, ipat)):
        assert out[:GUARD].tobytes() == pat.tobytes() and out[-GUARD:].tobytes() == pat.tobytes(), "guard overwritten"
    return cout[GUARD:-GUARD], iout[GUARD:-GUARD]


def operands_nt(dtype, mp, rd, n, k, m, rng):
    """(a, bt, b): test_gpu_argreduce.operands' pair with B stored M x K, and B itself for the oracle."""
    a, b = ar.operands(dtype, mp, rd, n, k, m, rng)
    return a, np.ascontiguousarray(b.T), b


@pytest.mark.parametrize("dtype,mp,rd", ar.ARG_CONFIGS, ids=["-".join(c) for c in ar.ARG_CONFIGS])
def test_argreduce_nt_every_config_both_paths(dtype, mp, rd):
    rng = np.random.default_rng(zlib.crc32(f"nt/{dtype}/{mp}/{rd}".encode()))
    for n, k, m in (TILED, PLAIN, EDGE):
        a, bt, b = operands_nt(dtype, mp, rd, n, k, m, rng)
        want_c, want_i = ar.oracle(dtype, mp, rd, a, b)
        if (n, k, m) == TILED and (mp, rd) != ("And", "Max"):
            # the indices say something: many distinct winners, some of them in the last slab ((And, Max) outputs are 0 / 1
            # and win at k < 16 by nature)
            assert len(np.unique(want_i[want_i >= 0])) >= 8 and (want_i >= 64).any(), np.unique(want_i)
        for path in (g.PATH_AUTO, g.PATH_ORDERED):
            cfg = g.make_config(dtype, mp, rd, path)
            c, i = launch(cfg, a, bt, n, k, m)
            ar.check(c.reshape(n, m), i.reshape(n, m), want_c, want_i, (n, k, m, path, g.kernel_name_argreduce_nt(cfg, n, k, m)))
        # accumulating, seeded with random values (NaN, +-inf, +-0 among them) and random indices
        c0, i0 = ar.seeds(dtype, (n, m), rng), rng.integers(-1, 1000, size=(n, m)).astype(np.int32)
        want_c, want_i = ar.oracle(dtype, mp, rd, a, b, c0, i0, index_base=5)
        for path in (g.PATH_AUTO, g.PATH_ORDERED):
            c, i = launch(g.make_config(dtype, mp, rd, path), a, bt, n, k, m, c0=c0, i0=i0, index_base=5)
            ar.check(c.reshape(n, m), i.reshape(n, m), want_c, want_i, (n, k, m, path, "seeded"))


def test_argreduce_nt_serving_rule_on_the_tested_shapes():
    for dtype, mp, rd in ar.ARG_CONFIGS:
        tile = np.dtype(sr.NP_DTYPES[dtype]).itemsize <= 4 and mp != "And"
        assert g.kernel_name_argreduce_nt(g.make_config(dtype, mp, rd), *TILED) == ("argreduce_tile_nt" if tile else "argreduce_nt")
        assert g.kernel_name_argreduce_nt(g.make_config(dtype, mp, rd), *PLAIN) == "argreduce_nt"
        assert g.kernel_name_argreduce_nt(g.make_config(dtype, mp, rd), *EDGE) == "argreduce_nt"
        assert g.kernel_name_argreduce_nt(g.make_config(dtype, mp, rd, g.PATH_ORDERED), *TILED) == "argreduce_nt"


@pytest.mark.parametrize("mp,rd", [("Add", "Min"), ("Multiply", "Max")])
@pytest.mark.parametrize("dtype", ["float", "half", "int8_t", "int", "double"])
def test_argreduce_nt_equals_the_row_major_call_on_a_materialised_transpose(dtype, mp, rd):
    rng = np.random.default_rng(zlib.crc32(f"nt-eq/{dtype}/{mp}/{rd}".encode()))
    for n, k, m in (TILED, PLAIN):
        a, bt, b = operands_nt(dtype, mp, rd, n, k, m, rng)
        c0, i0 = ar.seeds(dtype, (n, m), rng), rng.integers(-1, 1000, size=(n, m)).astype(np.int32)
        for path in (g.PATH_AUTO, g.PATH_ORDERED):
            cfg = g.make_config(dtype, mp, rd, path)
            for kw in ({}, {"c0": c0, "i0": i0, "index_base": 9}):
                c, i = launch(cfg, a, bt, n, k, m, **kw)
                rc, ri = launch(cfg, a, b, n, k, m, nt=False, **kw)
                ar.check(c, i, rc, ri, (dtype, n, k, m, path, sorted(kw)))


@pytest.mark.parametrize("dtype,rd", [("float", "Min"), ("int", "Max"), ("half", "Min"), ("double", "Max")])
def test_argreduce_nt_planted_ties_and_planted_winner(dtype, rd):
    t = sr.NP_DTYPES[dtype]
    for n, k, m in (TILED, PLAIN):
        for path in (g.PATH_AUTO, g.PATH_ORDERED):
            cfg = g.make_config(dtype, "Add", rd, path)
            a, bt = np.full((n, k), 3, dtype=t), np.full((m, k), 2, dtype=t)
            c, i = launch(cfg, a, bt, n, k, m, index_base=11)        # every k ties: the first one stays
            assert (i == 11).all() and (c == t(5)).all(), (np.unique(i), np.unique(c))
            bt[:, k - 1] = 1 if rd == "Min" else 4                    # one strictly better k per output, the last
            c, i = launch(cfg, a, bt, n, k, m, index_base=11)
            assert (i == 11 + k - 1).all() and (c == t(4 if rd == "Min" else 7)).all(), (np.unique(i), np.unique(c))


@pytest.mark.parametrize("shape", [(64, 32, 128), (33, 30, 45)], ids=["tile", "plain"])
def test_argreduce_nt_batches_broadcast_padded_and_chunked(shape):
    n, k, m = shape
    batch, sc = 3, n * m + 12
    rng = np.random.default_rng(17)
    dtype, mp, rd = "float", "Add", "Min"
    a = np.stack([ar.operands(dtype, mp, rd, n, k, m, rng)[0] for _ in range(batch)])
    _, bt, b = operands_nt(dtype, mp, rd, n, k, m, rng)
    cfg = g.make_config(dtype, mp, rd)
    assert g.kernel_name_argreduce_nt(cfg, n, k, m, batch) == ("argreduce_tile_nt" if k % 4 == 0 and m % 4 == 0 else "argreduce_nt")
    old = g.get_tuning("batch_chunk")
    try:
        runs = []
        for chunk in (-1, 2):
            g.set_tuning("batch_chunk", chunk)
            c, i = launch(cfg, a, bt, n, k, m, batch, n * k, 0, sc)          # a broadcast Bt: stride_b = 0
            runs.append((c.copy(), i.copy()))
            for e in range(batch):
                want_c, want_i = ar.oracle(dtype, mp, rd, a[e], b)
                ar.check(c[e * sc:e * sc + n * m].reshape(n, m), i[e * sc:e * sc + n * m].reshape(n, m), want_c, want_i, (chunk, e))
                if e < batch - 1:   # the gap between elements is not written
                    assert (i[e * sc + n * m:(e + 1) * sc] == 7).all() and (c[e * sc + n * m:(e + 1) * sc] == 0).all()
        ar.check(*runs[1], *runs[0], "batch_chunk = 2 against one launch")
    finally:
        g.set_tuning("batch_chunk", old)


@pytest.mark.parametrize("n,k", [(128, 64), (61, 37)], ids=["tile", "plain"])
def test_argreduce_nt_a_and_bt_one_buffer(n, k):
    """Min-plus A (x) A^T from ONE device buffer: the call takes the same pointer twice."""
    import torch
    rng = np.random.default_rng(19)
    a = ar.operands("float", "Add", "Min", n, k, n, rng)[0]
    da = torch.from_numpy(a).to("cuda:0")
    vals, idx = g.matmul_argreduce_nt(da, da)
    torch.cuda.synchronize()
    ar.check(vals.cpu().numpy(), idx.cpu().numpy(), *ar.oracle("float", "Add", "Min", a, a.T), (n, k))


@pytest.mark.parametrize("dtype", ["float", "half", "uint8_t"])
def test_argreduce_nt_misaligned_a_is_demoted_with_the_same_bits(dtype):
    n, k, m = 128, 64, 128
    rng = np.random.default_rng(23)
    a, bt, b = operands_nt(dtype, "Add", "Min", n, k, m, rng)
    cfg = g.make_config(dtype, "Add", "Min")
    assert g.kernel_name_argreduce_nt(cfg, n, k, m) == "argreduce_tile_nt"    # the name is the shape's, not the pointer's
    want = ar.oracle(dtype, "Add", "Min", a, b)
    aligned = launch(cfg, a, bt, n, k, m)
    moved = launch(cfg, a, bt, n, k, m, a_offset=1)
    ar.check(aligned[0].reshape(n, m), aligned[1].reshape(n, m), *want, "aligned")
    ar.check(*moved, *aligned, "A's base moved by one element")


def test_argreduce_nt_torch_binding():
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    for n, k, m in ((256, 128, 132), (67, 37, 61)):
        a, bt, b = operands_nt("float", "Add", "Min", n, k, m, rng)
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(bt).to(dev)
        vals, idx = g.matmul_argreduce_nt(ta, tb)
        assert idx.dtype == torch.int32 and vals.dtype == torch.float32 and tuple(vals.shape) == (n, m)
        ar.check(vals.cpu().numpy(), idx.cpu().numpy(), *ar.oracle("float", "Add", "Min", a, b), (n, "2-D"))
    # 3-D and expanded operands, out= / out_index=, and the in-place form on a batch
    a3 = torch.from_numpy(rng.uniform(-1, 1, size=(3, 64, 32)).astype(np.float32)).to(dev)
    b2 = torch.from_numpy(rng.uniform(-1, 1, size=(68, 32)).astype(np.float32)).to(dev)
    out = torch.empty(3, 64, 68, device=dev)
    out_i = torch.empty(3, 64, 68, dtype=torch.int32, device=dev)
    vals, idx = g.matmul_argreduce_nt(a3, b2.expand(3, 68, 32), reduce_op="Max", out=out, out_index=out_i)
    assert vals is out and idx is out_i
    rv, ri = g.matmul_argreduce(a3, b2.mT.contiguous(), reduce_op="Max")
    assert torch.equal(vals, rv) and torch.equal(idx, ri)
    c, ci = vals.clone(), idx.clone()
    g.addmm_argreduce_nt_(c, ci, a3 - 0.5, b2, reduce_op="Max", index_base=32)
    for e in range(3):
        want_c, want_i = ar.oracle("float", "Add", "Max", (a3[e] - 0.5).cpu().numpy(), b2.cpu().numpy().T,
                                   vals[e].cpu().numpy(), idx[e].cpu().numpy(), index_base=32)
        ar.check(c[e].cpu().numpy(), ci[e].cpu().numpy(), want_c, want_i, ("addmm_argreduce_nt_", e))
    with pytest.raises(g.MMError, match="Min or Max"):
        g.matmul_argreduce_nt(a3, b2, reduce_op="Add")
    with pytest.raises(g.MMError, match="inner dimensions"):
        g.matmul_argreduce_nt(a3, b2.mT.contiguous())
