"""The chain object's boundary without a GPU: the ctypes mirrors of
vp_chain_link, vp_chain_exit, vp_chain_config and vp_chain_view have the
header's C layout, compiled here with gcc as test_txreturn_abi.py does for its
structs; the three constants are the header's; the library exports the five
calls and the binding declares them; vp_chain_create refuses, before it reads
a context, everything its contract lists that needs none; the other calls
refuse a NULL chain, and vp_chain_destroy(NULL) does nothing."""
import ctypes as C
import os
import subprocess

import pytest

import vigor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"vp_chain_link": "ChainLinkC", "vp_chain_exit": "ChainExitC",
           "vp_chain_config": "ChainConfigC", "vp_chain_view": "ChainViewC"}
CALLS = {"vp_chain_create": 2, "vp_chain_destroy": 1, "vp_chain_run": 3, "vp_chain_view_get": 3,
         "vp_chain_process_device": 4}


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("cchainabi")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vigpath.h"',
             "int main(void) {",
             '  printf("VP_CHAIN_MAX_STAGES %u\\n", (unsigned)VP_CHAIN_MAX_STAGES);',
             '  printf("VP_CABLE_SLOTS %u\\n", (unsigned)VP_CABLE_SLOTS);',
             '  printf("VP_CABLE_STREAM %u\\n", (unsigned)VP_CABLE_STREAM);']
    for cname, pyname in STRUCTS.items():
        lines.append('  printf("%s.size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in getattr(vigor_amd, pyname)._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname,
                                                                          fname))
    lines += ["  return 0;", "}"]
    src = d / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = d / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {a: int(v) for a, v in (line.split() for line in out.splitlines())}


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_ctypes_mirror_matches_header(c_layout, cname):
    py = getattr(vigor_amd, STRUCTS[cname])
    assert C.sizeof(py) == c_layout[cname + ".size"]
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == c_layout["%s.%s" % (cname, fname)], fname


def test_field_names_and_constants(c_layout):
    assert [f for f, _ in vigor_amd.ChainLinkC._fields_] == ["from", "out_port", "to", "in_port"]
    assert [f for f, _ in vigor_amd.ChainExitC._fields_] == ["stage", "port", "ext_port"]
    assert [f for f, _ in vigor_amd.ChainConfigC._fields_] == [
        "stages", "n_stages", "links", "n_links", "exits", "n_exits", "cable"]
    assert [f for f, _ in vigor_amd.ChainViewC._fields_] == [
        "n", "slot", "frames", "len", "out_dev", "in_dev", "in_port", "now", "origin"]
    assert vigor_amd.CHAIN_MAX_STAGES == c_layout["VP_CHAIN_MAX_STAGES"] == 16
    assert vigor_amd.CABLE_SLOTS == c_layout["VP_CABLE_SLOTS"] == 0
    assert vigor_amd.CABLE_STREAM == c_layout["VP_CABLE_STREAM"] == 1


def test_library_exports_and_binding():
    raw = C.CDLL(os.path.join(ROOT, "vigor_amd", "libvigpath.so"))
    for name, n_args in CALLS.items():
        assert name in vigor_amd.EXPORTS
        assert hasattr(raw, name)
        fn = getattr(vigor_amd.lib(), name)
        assert len(fn.argtypes) == n_args, name
        assert fn.restype is (None if name == "vp_chain_destroy" else C.c_int), name
    for name in ("run", "process_device", "close"):
        assert callable(getattr(vigor_amd.CChain, name))


def test_create_refuses_before_any_context_is_read():
    """The stages stand for contexts (memory of ours, never real ones) and are
    not dereferenced on any of these paths: the NULL and count checks and the
    cable come first. The graph checks, which read n_devices, are in the GPU
    test."""
    L = vigor_amd.lib()
    E = vigor_amd.VP_EINVAL
    mem = (C.c_uint8 * 4096)()
    fake = C.addressof(mem)
    stages = (C.c_void_p * 17)(*[fake] * 17)
    links = (vigor_amd.ChainLinkC * 1)(vigor_amd.ChainLinkC(0, 1, 1, 0))

    def cfg(**kw):
        a = dict(stages=stages, n_stages=2, links=links, n_links=1, exits=None, n_exits=0,
                 cable=vigor_amd.CABLE_SLOTS)
        a.update(kw)
        return vigor_amd.ChainConfigC(**a)

    def rc(c, want_out=True):
        out = C.c_void_p(0x1234)
        got = L.vp_chain_create(C.byref(c) if c is not None else None,
                                C.byref(out) if want_out else None)
        assert out.value == 0x1234  # (a refusal writes no handle)
        return got

    assert rc(None) == E
    assert rc(cfg(), want_out=False) == E
    assert rc(cfg(n_stages=0)) == E
    assert rc(cfg(n_stages=17)) == E
    assert rc(cfg(stages=None)) == E
    holed = (C.c_void_p * 2)(fake, None)
    assert rc(cfg(stages=holed)) == E
    assert rc(cfg(stages=(C.c_void_p * 2)(None, fake))) == E
    assert rc(cfg(cable=2)) == E
    assert rc(cfg(cable=0xFFFFFFFF)) == E
    # an array that is missing although its count says otherwise
    assert rc(cfg(links=None)) == E
    assert rc(cfg(exits=None, n_exits=1)) == E


def test_null_chain():
    L = vigor_amd.lib()
    E = vigor_amd.VP_EINVAL
    b = vigor_amd.DevBatchC(n=0, slot=64)
    view = vigor_amd.ChainViewC()
    stats = vigor_amd.TxReturnStatsC()
    assert L.vp_chain_run(None, C.byref(b), None) == E
    assert L.vp_chain_view_get(None, 0, C.byref(view)) == E
    assert L.vp_chain_process_device(None, C.byref(b), C.byref(stats), None) == E
    assert L.vp_chain_process_device(None, C.byref(b), None, None) == E
    assert L.vp_chain_destroy(None) is None


def test_mirror_refuses_a_bad_cable_and_no_stage():
    with pytest.raises(ValueError):
        vigor_amd.CChain([], [])
    with pytest.raises(ValueError):
        vigor_amd.CChain([object()], [], cable="wire")
