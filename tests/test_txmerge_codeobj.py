"""vp_tx_merge's kernels (vp_txmerge.hip) keep nothing in scratch memory:
their kernel descriptors in the gfx950 code object that ships in
vigor_amd/libvigpath.so have a private segment of 0 bytes (read as
test_codeobj reads them). CPU only."""
import pytest

from test_codeobj import _find, _private_segments


@pytest.fixture(scope="module")
def segs():
    return _private_segments()


@pytest.mark.parametrize("kernel", ["txm_rank", "txm_gather"])
def test_txm_kernels_have_no_private_segment(segs, kernel):
    found = _find(segs, kernel)
    assert found
    for name, size in found.items():
        assert size == 0, "%s keeps %d bytes per lane in scratch memory" % (name, size)
