"""vp_tx_rebatch's kernel (vp_txbatch.hip) keeps nothing in scratch memory:
its kernel descriptor in the gfx950 code object that ships in
vigor_amd/libvigpath.so has a private segment of 0 bytes (read as
test_codeobj reads them). CPU only."""
import pytest

from test_codeobj import _find, _private_segments


@pytest.fixture(scope="module")
def segs():
    return _private_segments()


def test_txr_gather_has_no_private_segment(segs):
    found = _find(segs, "txr_gather")
    assert found
    for name, size in found.items():
        assert size == 0, "%s keeps %d bytes per lane in scratch memory" % (name, size)
