"""The incremental state images' boundary without a GPU: the library exports
the five calls and the binding declares them, the ctypes mirror of
vp_state_mark_t has the header's C layout (compiled here with gcc, as
test_rxmerge_abi.py does for its struct), the magic and version constants are
the header's, and every NF class shares NfBase's four methods."""
import ctypes as C
import os
import subprocess

import pytest

import deltaref as DR
import vigor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"vp_state_mark": 2, "vp_state_delta_size": 3, "vp_state_delta_save": 6,
         "vp_state_follow": 2, "vp_state_delta_apply": 3}


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("statedeltaabi")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vigpath.h"',
             "int main(void) {", '  printf("magic %u\\n", VP_STATE_DELTA_MAGIC);',
             '  printf("version %u\\n", VP_STATE_DELTA_VERSION);',
             '  printf("size %zu\\n", sizeof(vp_state_mark_t));']
    for fname, _ in vigor_amd.StateMarkC._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(vp_state_mark_t, %s));' % (fname, fname))
    lines += ["  return 0;", "}"]
    src = d / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = d / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {a: int(v) for a, v in (line.split() for line in out.splitlines())}


def test_ctypes_mirror_and_constants_match_header(c_layout):
    py = vigor_amd.StateMarkC
    assert [f for f, _ in py._fields_] == ["seq", "epoch"]
    assert C.sizeof(py) == c_layout["size"] == 16
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == c_layout[fname], fname
    assert vigor_amd.STATE_DELTA_MAGIC == c_layout["magic"] == DR.MAGIC
    assert c_layout["magic"].to_bytes(4, "little") == b"VPSD"
    assert vigor_amd.STATE_DELTA_VERSION == c_layout["version"] == DR.VERSION == 1


@pytest.mark.parametrize("name", sorted(CALLS))
def test_library_exports_and_binding(name):
    assert name in vigor_amd.EXPORTS
    L = C.CDLL(os.path.join(ROOT, "vigor_amd", "libvigpath.so"))
    assert hasattr(L, name)
    fn = getattr(vigor_amd.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == CALLS[name]


def test_nfbase_has_the_methods():
    from vigor_amd.nf import NfBase
    for m in ("state_mark", "save_delta", "follow", "apply_delta"):
        assert callable(getattr(NfBase, m))
        for cls in (vigor_amd.Nat, vigor_amd.Bridge, vigor_amd.Lb, vigor_amd.Fw, vigor_amd.Pol):
            assert getattr(cls, m) is getattr(NfBase, m)
