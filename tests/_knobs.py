"""The set-and-restore fixture of the library's tuning knobs; a test file imports it under the name its tests use."""
import pytest

import gemm_hls_amd as g


@pytest.fixture
def knob():
    """set(name, value) on the library's tuning knobs; every knob that was set gets its earlier value back."""
    old = {}

    def set_(name, value):
        old.setdefault(name, g.get_tuning(name))
        g.set_tuning(name, value)
    yield set_
    for name, value in old.items():
        g.set_tuning(name, value)
