"""vigpol's resident kernel pol_serve is in the gfx950 code object that ships in
vigor_amd/libvigpath.so and keeps nothing in scratch memory: it polls and
answers per packet, and a private segment would put register spills or a
dynamically indexed array of the ordered bucket replay on that path
(test_codeobj). CPU only."""
from test_codeobj import _find, _private_segments


def test_pol_serve_has_no_private_segment():
    for name, size in _find(_private_segments(), "pol_serve").items():
        assert size == 0, "%s keeps %d bytes per lane in scratch memory" % (name, size)
