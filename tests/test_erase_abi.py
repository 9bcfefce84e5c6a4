"""The table erase calls' boundary without a GPU: the library exports both
with seven arguments and the binding declares them, the header states the
loop they stand for, every NF class shares NfBase's methods, and a NULL
context is refused before any GPU is touched."""
import ctypes as C
import os
import re

import pytest

import vigor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"vp_table_erase": 7, "vp_table_free": 7}
EINVAL = -22


def header():
    with open(os.path.join(ROOT, "include", "vigpath.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(CALLS))
def test_library_exports_and_binding(name):
    assert name in vigor_amd.EXPORTS
    L = C.CDLL(os.path.join(ROOT, "vigor_amd", "libvigpath.so"))
    assert hasattr(L, name)
    fn = getattr(vigor_amd.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == CALLS[name]


@pytest.mark.parametrize("name", sorted(CALLS))
def test_header_declares_seven_arguments(name):
    m = re.search(r"^int %s\s*\(([^;]*)\);" % name, header(), re.M)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    assert len(args) == CALLS[name]
    assert "vp_lookup_out" in args[4] and "n_erased" in args[5] and "stream" in args[6]


def test_header_states_the_loop_and_the_free_order():
    text = " ".join(re.sub(r"^\s*\*", " ", line) for line in header().splitlines())
    text = re.sub(r"\s+", " ", text)
    for phrase in ("for q = 0 .. n-1 in order: if the query names a live entry, map_erase its key "
                   "and dchain_free_index its index",
                   "hands out the index of the last erasing query first",
                   "in reverse query order",
                   "ends a vp_state_follow",
                   "advances the context's sequence by one",
                   "n == 0 is VP_OK, launches nothing and writes *n_erased = 0"):
        assert phrase in text, phrase


def test_nfbase_has_the_methods():
    from vigor_amd.nf import NfBase
    for m in ("erase_device", "free_device", "erase", "free"):
        assert callable(getattr(NfBase, m))
        for cls in (vigor_amd.Nat, vigor_amd.Bridge, vigor_amd.Lb, vigor_amd.Fw, vigor_amd.Pol):
            assert getattr(cls, m) is getattr(NfBase, m)


def test_null_context_is_refused_without_a_gpu():
    L = vigor_amd.lib()
    out = vigor_amd.VpLookupOutC()
    for name in sorted(CALLS):
        k = C.c_uint32(7)
        assert getattr(L, name)(None, 0, 0, None, C.byref(out), C.byref(k), None) == EINVAL, name
        assert L.vp_last_error().decode() == "%s: ctx is NULL" % name
        assert k.value == 7
