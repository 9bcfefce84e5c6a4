"""vp_serve_stats (include/vigpath.h) and its ctypes mirror
vigor_amd.ServeStatsC: 40 bytes, the header's fields in the header's order at
the header's offsets, compiled here with gcc against the header (CPU only, in
the manner of test_abi_layout.py)."""
import ctypes as C
import os
import re
import subprocess

import vigor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["packets_one", "bursts", "burst_packets", "declined", "launches"]


def header_fields():
    src = open(os.path.join(ROOT, "include", "vigpath.h")).read()
    body = re.search(r"typedef struct vp_serve_stats \{(.*?)\} vp_serve_stats;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"uint64_t\s+(\w+)\s*;", body)


def test_serve_stats_layout(tmp_path):
    py = vigor_amd.ServeStatsC
    assert [f for f, _ in py._fields_] == header_fields() == FIELDS
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vigpath.h"',
             "int main(void) {", '  printf("size %zu\\n", sizeof(vp_serve_stats));']
    for f in FIELDS:
        lines.append('  printf("%s %%zu\\n", offsetof(vp_serve_stats, %s));' % (f, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict((a, int(b)) for a, b in (x.split() for x in out.splitlines()))
    assert got["size"] == 40 == C.sizeof(py)
    for f in FIELDS:
        assert getattr(py, f).offset == got[f], f


def test_serve_stats_prototype():
    """The library exports the symbol and the package declares its arguments."""
    assert "vp_serve_stats_get" in vigor_amd.EXPORTS
    L = vigor_amd.lib()
    assert L.vp_serve_stats_get.argtypes == [C.c_void_p, C.POINTER(vigor_amd.ServeStatsC)]
    assert L.vp_serve_stats_get(None, None) == vigor_amd.VP_EINVAL
