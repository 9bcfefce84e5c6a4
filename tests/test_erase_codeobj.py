"""The kernels of vp_table_erase / vp_table_free (vp_erase.hip) keep nothing
in scratch memory: each one's kernel descriptor in the gfx950 code object that
ships in vigor_amd/libvigpath.so has a private segment of 0 bytes (read as
test_codeobj reads them). CPU only."""
import pytest

from test_codeobj import _find, _private_segments

KERNELS = ["er_by_key", "er_by_index", "er_rank", "er_apply", "er_commit"]


@pytest.fixture(scope="module")
def segs():
    return _private_segments()


@pytest.mark.parametrize("kernel", KERNELS)
def test_erase_kernel_has_no_private_segment(segs, kernel):
    found = _find(segs, kernel)
    assert found
    for name, size in found.items():
        assert size == 0, "%s keeps %d bytes per lane in scratch memory" % (name, size)
