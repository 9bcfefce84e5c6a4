"""vp_serve_expiry_stats (include/vigpath.h) and its ctypes mirror
vigor_amd.ServeExpiryStatsC: 40 bytes, the header's fields in the header's
order at the header's offsets, compiled here with gcc against the header (CPU
only, in the manner of test_serve_stats_abi.py); the symbol and VP_EINVAL."""
import ctypes as C
import os
import re
import subprocess

import vigor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["seeds", "expired", "walks", "handed", "splits"]


def header_fields():
    src = open(os.path.join(ROOT, "include", "vigpath.h")).read()
    body = re.search(r"typedef struct vp_serve_expiry_stats \{(.*?)\} vp_serve_expiry_stats;",
                     src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"uint64_t\s+(\w+)\s*;", body)


def test_serve_expiry_stats_layout(tmp_path):
    py = vigor_amd.ServeExpiryStatsC
    assert [f for f, _ in py._fields_] == header_fields() == FIELDS
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vigpath.h"',
             "int main(void) {", '  printf("size %zu\\n", sizeof(vp_serve_expiry_stats));',
             '  printf("serve %zu\\n", sizeof(vp_serve_stats));']
    for f in FIELDS:
        lines.append('  printf("%s %%zu\\n", offsetof(vp_serve_expiry_stats, %s));' % (f, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict((a, int(b)) for a, b in (x.split() for x in out.splitlines()))
    assert got["size"] == 40 == C.sizeof(py)
    assert got["serve"] == 40  # (vp_serve_stats did not grow)
    for i, f in enumerate(FIELDS):
        assert getattr(py, f).offset == got[f] == 8 * i, f


def test_serve_expiry_stats_prototype():
    """The library exports the symbol, the package declares its arguments, and
    NULL is VP_EINVAL."""
    assert "vp_serve_expiry_stats_get" in vigor_amd.EXPORTS
    L = vigor_amd.lib()
    assert L.vp_serve_expiry_stats_get.argtypes == \
        [C.c_void_p, C.POINTER(vigor_amd.ServeExpiryStatsC)]
    st = vigor_amd.ServeExpiryStatsC()
    assert L.vp_serve_expiry_stats_get(None, C.byref(st)) == vigor_amd.VP_EINVAL
    assert L.vp_serve_expiry_stats_get(None, None) == vigor_amd.VP_EINVAL
    assert hasattr(vigor_amd.NfBase, "serve_expiry_stats")
