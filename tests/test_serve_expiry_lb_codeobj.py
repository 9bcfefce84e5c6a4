"""viglb's resident kernel is a template on whether it expires from the touch
journals: the gfx950 code object in vigor_amd/libvigpath.so
holds two instances of lb_serve, the one without the journals for a context
that has met no due expiry, and neither keeps anything in scratch memory
(test_codeobj) -- with two journals' control words in registers as well. CPU
only."""
from test_codeobj import _find, _private_segments


def test_two_instances_without_a_private_segment():
    hits = _find(_private_segments(), "lb_serve")
    assert len(hits) == 2, "lb_serve: %d instances %s" % (len(hits), sorted(hits))
    for name, size in hits.items():
        assert size == 0, "%s keeps %d bytes per lane in scratch memory" % (name, size)
