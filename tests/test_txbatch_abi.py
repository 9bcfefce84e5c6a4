"""vp_tx_rebatch's boundary without a GPU: the ctypes mirror of vp_tx_next has
the header's C layout (compiled here with gcc, as test_txpack_abi.py does for
its struct), the library exports the call and the binding declares it, the
numpy reference the GPU tests compare against (txbatchref.py) gives the
contract's bytes on a hand-computed example, and Chain refuses the link sets
it does not support."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import vigor_amd
from test_abi import declared
from txbatchref import rebatch_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    py = vigor_amd.TxNextC
    d = tmp_path_factory.mktemp("txbatchabi")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vigpath.h"',
             "int main(void) {",
             '  printf("size %zu\\n", sizeof(vp_tx_next));']
    for fname, _ in py._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(vp_tx_next, %s));' % (fname, fname))
    lines += ["  return 0;", "}"]
    src = d / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = d / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {a: int(v) for a, v in (line.split() for line in out.splitlines())}


def test_ctypes_mirror_matches_header(c_layout):
    py = vigor_amd.TxNextC
    assert C.sizeof(py) == c_layout["size"]
    assert [f for f, _ in py._fields_] == ["frames", "slot", "cap", "len", "now", "src", "count"]
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == c_layout[fname], fname


def test_library_exports_and_binding():
    assert "vp_tx_rebatch" in vigor_amd.EXPORTS
    assert "vp_tx_rebatch" in declared("vigpath.h")
    L = C.CDLL(os.path.join(ROOT, "vigor_amd", "libvigpath.so"))
    assert hasattr(L, "vp_tx_rebatch")
    fn = vigor_amd.lib().vp_tx_rebatch
    assert fn.restype is C.c_int and len(fn.argtypes) == 6
    assert fn.argtypes[3] is C.c_uint32


def test_nfbase_has_tx_rebatch():
    from vigor_amd.nf import NfBase
    assert callable(NfBase.tx_rebatch)
    for cls in (vigor_amd.Nat, vigor_amd.Bridge, vigor_amd.Pol):
        assert cls.tx_rebatch is NfBase.tx_rebatch


def _example():
    """5 packets in 64-byte slots, two ports; port 1's list is packets 0, 2, 4
    and an entry outside the batch."""
    slot = 64
    frames = (np.arange(5 * slot) % 251 + 1).astype(np.uint8)  # no zero byte
    lens = [17, 0, 1518, 33, 64]
    idx = [1, 3, 0, 2, 4, 9]
    offset = [0, 2, 6]
    return frames, slot, lens, idx, offset


def test_reference_hand_computed_example():
    frames, slot, lens, idx, offset = _example()
    f = frames.reshape(5, slot)
    count, o_f, o_l, o_n, o_s = rebatch_reference(frames, slot, lens, idx, offset, 6, 2, 1, 128,
                                                  8, now0=1000, now_step=10)
    assert count == 4 and o_f.size == 4 * 128
    g = o_f.reshape(4, 128)
    for k, i in enumerate([0, 2, 4]):
        assert g[k, :64].tobytes() == f[i].tobytes() and not g[k, 64:].any()
    assert not g[3].any()
    assert o_l.tolist() == [17, 1518, 64, 0] and o_l.dtype == np.uint16
    assert o_n.tolist() == [1000, 1020, 1040, 0] and o_n.dtype == np.int64
    assert o_s.tolist() == [0, 2, 4, 9] and o_s.dtype == np.uint32
    # port 0, a time array, a narrow output that holds one entry of the two
    now = np.array([5, 6, 7, 8, 9], np.int64)
    count, o_f, o_l, o_n, o_s = rebatch_reference(frames, slot, lens, idx, offset, 6, 2, 0, 64,
                                                  1, now=now)
    assert count == 2 and o_f.tobytes() == f[1].tobytes()
    assert o_l.tolist() == [0] and o_n.tolist() == [6] and o_s.tolist() == [1]


def test_reference_clipped_lists_and_wrapping_time():
    frames, slot, lens, idx, offset = _example()
    # the lists' capacity ends inside port 1's list, and before it
    assert rebatch_reference(frames, slot, lens, idx, offset, 3, 2, 1, 64, 8)[0] == 1
    count, o_f, *_ = rebatch_reference(frames, slot, lens, idx, offset, 1, 2, 1, 64, 8)
    assert count == 0 and o_f.size == 0
    # the affine time is a 64-bit product and sum
    *_, o_n, _ = rebatch_reference(frames, slot, lens, idx, offset, 6, 2, 1, 64, 8,
                                   now0=(1 << 62), now_step=(1 << 61))
    # packets 0, 2, 4: 2^62, 2^63 and 3 * 2^62 modulo 2^64, read as signed
    assert o_n.tolist() == [1 << 62, -(1 << 63), -(1 << 62), 0]


def _stage(nd=2):
    return SimpleNamespace(cfg=SimpleNamespace(n_devices=nd))


def test_chain_accepts_a_line_and_a_tree():
    c = vigor_amd.Chain([_stage(), _stage(), _stage()], [(0, 1, 1, 0), (1, 1, 2, 0)])
    assert c.inbound == [None, (0, 1, 0), (1, 1, 0)]
    vigor_amd.Chain([_stage(4), _stage(), _stage()], [(0, 1, 1, 0), (0, 3, 2, 1)])
    vigor_amd.Chain([_stage()], [])


@pytest.mark.parametrize("links", [
    [(1, 0, 0, 0)],                               # backward
    [(0, 1, 1, 0), (2, 0, 1, 1)],                 # backward, into a linked stage
    [(0, 1, 0, 0)],                               # onto itself
    [(0, 0, 2, 0), (0, 1, 2, 0), (0, 1, 1, 0)],   # two inbound links
    [(0, 1, 2, 0)],                               # stage 1 has none
    [],                                           # neither stage has one
    [(0, 1, 1, 0), (1, 1, 3, 0)],                 # a stage outside the chain
    [(0, 2, 1, 0), (1, 1, 2, 0)],                 # a port the stage does not have
])
def test_chain_rejects(links):
    with pytest.raises(ValueError):
        vigor_amd.Chain([_stage(), _stage(), _stage()], links)
