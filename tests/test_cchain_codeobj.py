"""The chain's one kernel (chn_compose, vp_chain.hip) keeps nothing in scratch
memory: its kernel descriptor in the gfx950 code object that ships in
vigor_amd/libvigpath.so has a private segment of 0 bytes (read as
test_codeobj reads them). CPU only."""
import pytest

from test_codeobj import _find, _private_segments


@pytest.fixture(scope="module")
def segs():
    return _private_segments()


def test_chn_compose_has_no_private_segment(segs):
    found = _find(segs, "chn_compose")
    assert found
    for name, size in found.items():
        assert size == 0, "%s keeps %d bytes per lane in scratch memory" % (name, size)
