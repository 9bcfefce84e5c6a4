"""viglb's resident kernel lb_serve is in the gfx950 code object that ships in
vigor_amd/libvigpath.so and keeps nothing in scratch memory: it polls and
answers per packet, and a private segment would put register spills, a copy
of its arguments or a dynamically indexed frame word on that path
(test_codeobj). CPU only."""
from test_codeobj import _find, _private_segments


def test_lb_serve_has_no_private_segment():
    for name, size in _find(_private_segments(), "lb_serve").items():
        assert size == 0, "%s keeps %d bytes per lane in scratch memory" % (name, size)
