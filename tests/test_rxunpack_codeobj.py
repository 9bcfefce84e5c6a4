"""vp_rx_unpack's kernels (vp_rxunpack.hip) keep nothing in scratch memory:
their kernel descriptors in the gfx950 code object that ships in
vigor_amd/libvigpath.so have a private segment of 0 bytes (read as
test_codeobj reads them). CPU only."""
import pytest

from test_codeobj import _find, _private_segments


@pytest.fixture(scope="module")
def segs():
    return _private_segments()


@pytest.mark.parametrize("kernel", ["rxu_sizes", "rxu_scatter"])
def test_rxunpack_kernels_have_no_private_segment(segs, kernel):
    for name, size in _find(segs, kernel).items():
        assert size == 0, "%s keeps %d bytes per lane in scratch memory" % (name, size)


def test_every_rxu_kernel_is_covered(segs):
    names = {n for n in segs if "rxu_" in n}
    assert names and all("rxu_sizes" in n or "rxu_scatter" in n for n in names), names
