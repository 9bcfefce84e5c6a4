"""The table lookups' boundary without a GPU: the library exports the three
calls and the binding declares them, the ctypes mirror of vp_lookup_out has
the header's C layout (compiled here with gcc, as test_state_delta_abi.py
does for its struct), VP_LOOKUP_MISS is the header's, every NF class shares
NfBase's methods, and a NULL context is refused before any GPU is touched."""
import ctypes as C
import os
import subprocess

import pytest

import lookupref as LR
import vigor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"vp_table_lookup": 6, "vp_table_entries": 6, "vp_table_value_size": 3}
EINVAL = -22


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("lookupabi")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vigpath.h"',
             "int main(void) {", '  printf("miss %u\\n", VP_LOOKUP_MISS);',
             '  printf("size %zu\\n", sizeof(vp_lookup_out));']
    for fname, _ in vigor_amd.VpLookupOutC._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(vp_lookup_out, %s));' % (fname, fname))
    lines += ["  return 0;", "}"]
    src = d / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = d / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {a: int(v) for a, v in (line.split() for line in out.splitlines())}


def test_ctypes_mirror_and_constant_match_header(c_layout):
    py = vigor_amd.VpLookupOutC
    assert [f for f, _ in py._fields_] == ["index", "ts", "key", "value"]
    assert C.sizeof(py) == c_layout["size"] == 32
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == c_layout[fname], fname
    assert vigor_amd.LOOKUP_MISS == c_layout["miss"] == LR.MISS == 0xFFFFFFFF


@pytest.mark.parametrize("name", sorted(CALLS))
def test_library_exports_and_binding(name):
    assert name in vigor_amd.EXPORTS
    L = C.CDLL(os.path.join(ROOT, "vigor_amd", "libvigpath.so"))
    assert hasattr(L, name)
    fn = getattr(vigor_amd.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == CALLS[name]


def test_nfbase_has_the_methods():
    from vigor_amd.nf import NfBase
    for m in ("lookup_device", "entries_device", "value_size", "lookup", "entries"):
        assert callable(getattr(NfBase, m))
        for cls in (vigor_amd.Nat, vigor_amd.Bridge, vigor_amd.Lb, vigor_amd.Fw, vigor_amd.Pol):
            assert getattr(cls, m) is getattr(NfBase, m)


def test_null_context_is_refused_without_a_gpu():
    L = vigor_amd.lib()
    out = vigor_amd.VpLookupOutC()
    n = C.c_uint32(7)
    calls = (("vp_table_lookup", lambda: L.vp_table_lookup(None, 0, 0, None, C.byref(out), None)),
             ("vp_table_entries", lambda: L.vp_table_entries(None, 0, 0, None, C.byref(out), None)),
             ("vp_table_value_size", lambda: L.vp_table_value_size(None, 0, C.byref(n))))
    for name, call in calls:
        assert call() == EINVAL, name
        assert L.vp_last_error().decode() == "%s: ctx is NULL" % name
    assert n.value == 7
