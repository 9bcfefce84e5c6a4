"""vp_tx_return's kernel (vp_txreturn.hip) keeps nothing in scratch memory and
uses no LDS: its kernel descriptor in the gfx950 code object that ships in
vigor_amd/libvigpath.so has a private segment and a group segment of 0 bytes
(the code objects found as test_codeobj finds them). CPU only."""
import os
import re
import subprocess
import tempfile

import pytest

from test_codeobj import LLVM, _code_objects, _find


def _segments(field):
    """{mangled kernel name: bytes of `field`} over every code object."""
    sizes = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in _code_objects(tmp):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co],
                                   check=True, capture_output=True, text=True).stdout
            # a kernel's metadata lists both segment sizes before its .symbol
            pending = None
            for line in notes.splitlines():
                m = re.match(r"\s+(?:- )?\.%s:\s+(\d+)" % field, line)
                if m:
                    pending = int(m.group(1))
                m = re.match(r"\s+\.symbol:\s+(\S+)\.kd", line)
                if m and pending is not None:
                    sizes[m.group(1)] = pending
                    pending = None
    return sizes


@pytest.mark.parametrize("field", ["private_segment_fixed_size", "group_segment_fixed_size"])
def test_txt_scatter_has_no_private_segment_and_no_lds(field):
    hits = _find(_segments(field), "txt_scatter")
    for name, size in hits.items():
        assert size == 0, "%s: %s is %d bytes" % (name, field, size)
