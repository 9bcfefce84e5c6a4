"""vp_tx_merge's boundary without a GPU: the ctypes mirrors of vp_tx_source and
vp_tx_merged have the header's C layout (compiled here with gcc, as
test_txbatch_abi.py does for its struct), the library exports the call and the
binding declares it, the call refuses what it can refuse before it touches a
context, and the numpy reference the GPU tests compare against (txmergeref.py)
gives the contract's order and bytes on a hand-written example with ties."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vigor_amd
from test_abi import declared
from txmergeref import merge_reference, source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = [("vp_tx_source", "TxSourceC"), ("vp_tx_merged", "TxMergedC")]


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("txmergeabi")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vigpath.h"',
             "int main(void) {", '  printf("max %d\\n", VP_TX_MERGE_MAX);']
    for cname, pyname in STRUCTS:
        lines.append('  printf("%s.size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in getattr(vigor_amd, pyname)._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));'
                         % (cname, fname, cname, fname))
    lines += ["  return 0;", "}"]
    src = d / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = d / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {a: int(v) for a, v in (line.split() for line in out.splitlines())}


def test_ctypes_mirrors_match_header(c_layout):
    assert c_layout["max"] == vigor_amd.TX_MERGE_MAX == 8
    for cname, pyname in STRUCTS:
        py = getattr(vigor_amd, pyname)
        assert C.sizeof(py) == c_layout[cname + ".size"]
        for fname, _ in py._fields_:
            assert getattr(py, fname).offset == c_layout["%s.%s" % (cname, fname)], fname
    assert [f for f, _ in vigor_amd.TxSourceC._fields_] == [
        "ctx", "batch", "lists", "port", "in_port", "key"]
    assert [f for f, _ in vigor_amd.TxMergedC._fields_] == [
        "frames", "slot", "cap", "len", "now", "in_dev", "key", "src", "which", "count"]


def test_library_exports_and_binding():
    assert "vp_tx_merge" in vigor_amd.EXPORTS
    assert "vp_tx_merge" in declared("vigpath.h")
    L = C.CDLL(os.path.join(ROOT, "vigor_amd", "libvigpath.so"))
    assert hasattr(L, "vp_tx_merge")
    fn = vigor_amd.lib().vp_tx_merge
    assert fn.restype is C.c_int and len(fn.argtypes) == 5
    assert fn.argtypes[2] is C.c_uint32


def test_nfbase_has_tx_merge():
    from vigor_amd.nf import NfBase
    assert callable(NfBase.tx_merge)
    for cls in (vigor_amd.Nat, vigor_amd.Bridge, vigor_amd.Pol):
        assert cls.tx_merge is NfBase.tx_merge


def test_einval_before_any_context_is_read():
    """Every refusal the call makes before it reads a context: `ctx` stands
    for one (memory of ours, never a real context) and is not dereferenced on
    any of these paths; the refusals that need a real context (a port beyond
    n_devices, another GPU, overlapping slot arrays) are in the GPU test."""
    L = vigor_amd.lib()
    E = vigor_amd.VP_EINVAL
    mem = (C.c_uint8 * 4096)()
    base = (C.addressof(mem) + 15) & ~15
    ctx = C.c_void_p(base)

    def batch(**kw):
        b = dict(frames=base, slot=64, n=4, len=base)
        b.update(kw)
        return vigor_amd.DevBatchC(**b)

    def lists(**kw):
        a = dict(idx=base, cap=4, offset=base, stats=None)
        a.update(kw)
        return vigor_amd.TxListsC(**a)

    def merged(**kw):
        a = dict(frames=base, slot=64, cap=4, len=base, now=None, in_dev=None, key=None,
                 src=base, which=base, count=base)
        a.update(kw)
        return vigor_amd.TxMergedC(**a)

    keep = []

    def srcs(n=1, b=None, a=None, **kw):
        arr = (vigor_amd.TxSourceC * max(n, 1))()
        for s in arr:
            bb, ll = b or batch(), a or lists()
            keep.extend([bb, ll])
            s.ctx, s.batch, s.lists = base, C.addressof(bb), C.addressof(ll)
            s.port, s.in_port, s.key = 0, 0, None
            for k, v in kw.items():
                setattr(s, k, v)
        return arr

    def rc(h, arr, n, o):
        return L.vp_tx_merge(h, arr, n, C.byref(o) if o is not None else None, None)

    assert rc(None, srcs(), 1, merged()) == E
    assert rc(ctx, None, 1, merged()) == E
    assert rc(ctx, srcs(), 1, None) == E
    assert rc(ctx, srcs(), 1, merged(count=None)) == E
    assert rc(ctx, srcs(), 0, merged()) == E
    assert rc(ctx, srcs(9), 9, merged()) == E
    assert rc(ctx, srcs(), 0xFFFFFFFF, merged()) == E
    for bad_slot in (0, 48, 72, 1000):
        assert rc(ctx, srcs(), 1, merged(slot=bad_slot)) == E
        assert rc(ctx, srcs(b=batch(slot=bad_slot)), 1, merged()) == E
    assert rc(ctx, srcs(), 1, merged(frames=base + 8)) == E
    assert rc(ctx, srcs(b=batch(frames=base + 8)), 1, merged()) == E
    for missing in ("frames", "len", "src", "which"):
        assert rc(ctx, srcs(), 1, merged(**{missing: None})) == E
    assert rc(ctx, srcs(ctx=None), 1, merged()) == E
    assert rc(ctx, srcs(batch=None), 1, merged()) == E
    assert rc(ctx, srcs(lists=None), 1, merged()) == E
    assert rc(ctx, srcs(a=lists(offset=None)), 1, merged()) == E
    assert rc(ctx, srcs(a=lists(idx=None)), 1, merged()) == E
    assert rc(ctx, srcs(in_port=0x10000), 1, merged()) == E
    assert rc(ctx, srcs(in_port=0xFFFFFFFF), 1, merged()) == E
    # the second source is checked like the first
    two = srcs(2)
    two[1].in_port = 0x10000
    assert rc(ctx, two, 2, merged()) == E
    assert not any(mem)


def _example():
    """Three sources with ties. Source 0 and 1 are ports 0 and 1 of one
    6-packet batch in 64-byte slots (packets 1 and 4 stand in both lists: a
    flood), keyed by index; source 2 is port 0 of a 4-packet batch in 128-byte
    slots with a key array that repeats, and an entry outside its batch."""
    fa = (np.arange(6 * 64) % 251 + 1).astype(np.uint8)
    la = [17, 0, 1518, 33, 64, 60]
    idx_a, off_a = [1, 4, 5, 0, 1, 2, 4], [0, 3, 7]
    fb = (np.arange(4 * 128) % 241 + 3).astype(np.uint8)
    lb = [100, 128, 7, 90]
    idx_b, off_b = [0, 1, 2, 3, 9], [0, 5, 5]
    key_b = [1, 1, 4, 6]
    a0 = source(fa, 64, la, idx_a, off_a, 2, 0, in_port=3, now0=1000, now_step=10)
    a1 = source(fa, 64, la, idx_a, off_a, 2, 1, in_port=4, now0=1000, now_step=10)
    b0 = source(fb, 128, lb, idx_b, off_b, 2, 0, in_port=5, key=key_b,
                now=np.array([1010, 1011, 1040, 1060], np.int64))
    return fa.reshape(6, 64), fb.reshape(4, 128), [a0, a1, b0]


def test_reference_hand_written_example_with_ties():
    fa, fb, srcs = _example()
    o = merge_reference(srcs, 128, 64)
    # keys: source 0: 1 4 5; source 1: 0 1 2 4; source 2: 1 1 4 6 9
    assert o.count == 12
    assert o.key.tolist() == [0, 1, 1, 1, 1, 2, 4, 4, 4, 5, 6, 9]
    assert o.which.tolist() == [1, 0, 1, 2, 2, 1, 0, 1, 2, 0, 2, 2]
    assert o.src.tolist() == [0, 1, 1, 0, 1, 2, 4, 4, 2, 5, 3, 9]
    assert o.in_dev.tolist() == [4, 3, 4, 5, 5, 4, 3, 4, 5, 3, 5, 5]
    assert o.len.tolist() == [17, 0, 0, 100, 128, 1518, 64, 64, 7, 60, 90, 0]
    assert o.now.tolist() == [1000, 1010, 1010, 1010, 1011, 1020, 1040, 1040, 1040, 1050, 1060, 0]
    g = o.frames.reshape(12, 128)
    assert g[0, :64].tobytes() == fa[0].tobytes() and not g[0, 64:].any()
    assert g[3].tobytes() == fb[0].tobytes() and g[8].tobytes() == fb[2].tobytes()
    assert not g[11].any()  # the entry outside its batch
    assert o.key.dtype == np.uint32 and o.which.dtype == np.uint8 and o.in_dev.dtype == np.uint16
    # a narrow output that holds five entries; the wide source is cut to 64 bytes
    o = merge_reference(srcs, 64, 5)
    assert o.count == 12 and o.frames.size == 5 * 64 and o.len.tolist() == [17, 0, 0, 100, 128]
    assert o.frames.reshape(5, 64)[4].tobytes() == fb[1, :64].tobytes()
    # lists clipped by their capacity: source 1 keeps one entry of its four
    srcs[1].lists_cap = 4
    srcs[0].lists_cap = 4
    o = merge_reference(srcs, 64, 64)
    assert o.count == 9 and o.which.tolist() == [1, 0, 2, 2, 0, 2, 0, 2, 2]
