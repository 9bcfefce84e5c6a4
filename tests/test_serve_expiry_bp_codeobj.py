"""vigbridge's and vigpol's resident kernels are templates on whether the
kernel expires from the touch journal: the gfx950 code object
in vigor_amd/libvigpath.so holds two instances of each, the one without the
journal for a context that has met no due expiry, and neither keeps anything
in scratch memory (test_codeobj). CPU only."""
import pytest
from test_codeobj import _find, _private_segments


@pytest.fixture(scope="module")
def segs():
    return _private_segments()


@pytest.mark.parametrize("kernel", ["bridge_serve", "pol_serve"])
def test_two_instances_without_a_private_segment(segs, kernel):
    hits = _find(segs, kernel)
    assert len(hits) == 2, "%s: %d instances %s" % (kernel, len(hits), sorted(hits))
    for name, size in hits.items():
        assert size == 0, "%s keeps %d bytes per lane in scratch memory" % (name, size)
