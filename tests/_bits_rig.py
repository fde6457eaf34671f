"""What the tests of the packed calls (mm_bits_*) share.  GPU side: device buffers between guard words, operands laid out with
row and batch strides inside fill words, poisoned padding bits, the first difference of an exact comparison.  CPU side: the
last error's text, the enqueue / launch parametrisation, a kernel knob set for the duration of a with-block."""
import numpy as np
import pytest

import gemm_hls_amd as g

GUARD = 8   # words of pattern in front of and behind every device buffer (32 bytes: the 16-byte alignment survives)


def _pattern(count, salt=0):
    return ((np.arange(count, dtype=np.uint64) * 2654435761 + 0x9E3779B9 + salt) & 0xFFFFFFFF).astype(np.uint32)


class Dev:
    """A host array of words on the device behind GUARD (+ shift) words of pattern; fetch() checks the guards."""
    def __init__(self, words, shift=0):
        import torch
        self.shape, self.lead = words.shape, GUARD + shift
        flat = np.concatenate([_pattern(self.lead, 1), words.reshape(-1).astype(np.uint32), _pattern(GUARD, 2)])
        self.t = torch.from_numpy(flat.view(np.int32)).to("cuda:0")
        self.ptr = self.t.data_ptr() + 4 * self.lead

    def fetch(self):
        out = self.t.cpu().numpy().view(np.uint32)
        assert np.array_equal(out[:self.lead], _pattern(self.lead, 1)) and np.array_equal(out[-GUARD:], _pattern(GUARD, 2)), "guard overwritten"
        return out[self.lead:-GUARD].reshape(self.shape)


def _layout(rows_, ld, stride, fill):
    """(batch, rows, w) words laid out with row stride ld and batch stride `stride` inside `fill`-valued words."""
    batch, rows, w = rows_.shape
    out = fill[:batch * stride].reshape(batch, stride).copy()
    for r in range(rows):
        out[:, r * ld:r * ld + w] = rows_[:, r]
    return out


def _rows_of(buf, rows, w, ld):
    return np.stack([buf[:, r * ld:r * ld + w] for r in range(rows)], axis=1)


def _poison_padding(packed, cols):
    if cols % 32:
        packed[..., -1] |= np.uint32((0xFFFFFFFF << (cols % 32)) & 0xFFFFFFFF)
    return packed


def _first_difference(got, want, unit, fmt):
    """unit: what differs ("words", "elements"); fmt: how one is printed ("#x", "")."""
    idx = np.argwhere(got != want)
    return (f"{len(idx)} {unit} differ, the first at {idx[0]}: got {got[tuple(idx[0])]:{fmt}}, want {want[tuple(idx[0])]:{fmt}}"
            if len(idx) else "")


def _err():
    return g.lib().mm_last_error().decode()


LAUNCH = pytest.mark.parametrize("launch", [False, True], ids=["enqueue", "launch"])


class _Variant:
    """The tuning knob `name` set to `value` for the duration of a with-block."""
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = g.get_tuning(self.name)
        g.set_tuning(self.name, self.value)

    def __exit__(self, *exc):
        g.set_tuning(self.name, self.old)
