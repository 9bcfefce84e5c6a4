"""vp_rx_merge's boundary without a GPU: the ctypes mirror of vp_rx_queue has
the header's C layout (compiled here with gcc, as test_rxunpack_abi.py does for
its struct) and the constant is the header's, the library exports the call and
the binding declares it, every NF class shares NfBase.rx_merge, and the numpy
reference the GPU tests compare against (rxmergeref.py) gives the contract's
bytes on a hand-computed example."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vigor_amd
from rxmergeref import I64_MAX, merge_reference, queue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    py = vigor_amd.RxQueueC
    d = tmp_path_factory.mktemp("rxmergeabi")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vigpath.h"',
             "int main(void) {", '  printf("max %d\\n", VP_RX_MERGE_MAX);',
             '  printf("size %zu\\n", sizeof(vp_rx_queue));',
             '  printf("inner %zu\\n", sizeof(vp_rx_stream));']
    for fname, _ in py._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(vp_rx_queue, %s));' % (fname, fname))
    lines += ["  return 0;", "}"]
    src = d / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = d / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {a: int(v) for a, v in (line.split() for line in out.splitlines())}


def test_ctypes_mirror_matches_header(c_layout):
    py = vigor_amd.RxQueueC
    assert vigor_amd.RX_MERGE_MAX == c_layout["max"] == 8
    assert C.sizeof(py) == c_layout["size"]
    assert C.sizeof(vigor_amd.RxStreamC) == c_layout["inner"]
    assert [f for f, _ in py._fields_] == ["stream", "in_port"]
    assert py._fields_[0][1] is vigor_amd.RxStreamC
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == c_layout[fname], fname


def test_library_exports_and_binding():
    assert "vp_rx_merge" in vigor_amd.EXPORTS
    L = C.CDLL(os.path.join(ROOT, "vigor_amd", "libvigpath.so"))
    assert hasattr(L, "vp_rx_merge")
    fn = vigor_amd.lib().vp_rx_merge
    assert fn.restype is C.c_int and len(fn.argtypes) == 5


def test_nfbase_has_rx_merge():
    from vigor_amd.nf import NfBase
    assert callable(NfBase.rx_merge)
    for cls in (vigor_amd.Nat, vigor_amd.Bridge, vigor_amd.Lb, vigor_amd.Fw, vigor_amd.Pol):
        assert cls.rx_merge is NfBase.rx_merge


def _example():
    """Queue 0 on port 3: frames of 60 and 20 bytes at 0 and 64, times 10 and
    30. Queue 1 on port 7: frames of 17, 9 and 33 bytes at 0, 40 (misaligned:
    not readable) and 32, times 5, 10 and 40. The padding holds 0xEE."""
    a = (np.arange(60) + 1).astype(np.uint8)
    b = (np.arange(20) + 101).astype(np.uint8)
    d0 = np.full(96, 0xEE, np.uint8)
    d0[0:60], d0[64:84] = a, b
    c = (np.arange(17) + 151).astype(np.uint8)
    d = (np.arange(33) + 201).astype(np.uint8)
    d1 = np.full(80, 0xEE, np.uint8)
    d1[0:17], d1[32:65] = c, d
    q0 = queue(d0, [60, 20], 3, pos=[0, 64], now=[10, 30])
    q1 = queue(d1, [17, 9, 33], 7, pos=[0, 40, 32], now=[5, 10, 40])
    return q0, q1, (a, b, c, d)


def test_reference_hand_computed_example():
    q0, q1, (a, b, c, d) = _example()
    count, fr, ln, nw, ind, sr, wh = merge_reference([q0, q1], 64, 8)
    # by time; the tie at 10 goes to queue 0; the broken frame keeps its time
    assert count == 5 and fr.size == 5 * 64 and fr.dtype == np.uint8
    assert wh.tolist() == [1, 0, 1, 0, 1] and wh.dtype == np.uint8
    assert sr.tolist() == [0, 0, 1, 1, 2] and sr.dtype == np.uint32
    assert nw.tolist() == [5, 10, 10, 30, 40] and nw.dtype == np.int64
    assert ln.tolist() == [17, 60, 0, 20, 33] and ln.dtype == np.uint16
    assert ind.tolist() == [7, 3, 7, 3, 7] and ind.dtype == np.uint16
    s = fr.reshape(5, 64)
    assert s[0, :17].tobytes() == c.tobytes() and not s[0, 17:].any()  # (0xEE cleared)
    assert s[1, :60].tobytes() == a.tobytes() and not s[1, 60:].any()
    assert not s[2].any()
    assert s[3, :20].tobytes() == b.tobytes() and not s[3, 20:].any()
    assert s[4, :33].tobytes() == d.tobytes() and not s[4, 33:].any()


def test_reference_truncation_keys_and_signed_times():
    q0, q1, _ = _example()
    full = merge_reference([q0, q1], 64, 8)
    # the capacity cuts the arrays, not the count
    cut = merge_reference([q0, q1], 64, 3)
    assert cut[0] == 5 and cut[2].size == 3 and cut[1].size == 3 * 64
    assert all(x.tobytes() == y[:x.size].tobytes() for x, y in zip(cut[1:], full[1:]))
    assert merge_reference([q0, q1], 64, 0)[0] == 5
    # an index beyond len[] has the key INT64_MAX: it goes last, with that time
    q2 = queue(q1["data"], [17, 9, 33], 1, pos=[0, 0], sel=[9, 0], now=[5, 10, 40])
    count, fr, ln, nw, ind, sr, wh = merge_reference([q0, q2], 64, 8)
    # (queue 2's own times go back here; the reference still sorts all entries)
    assert nw.tolist() == [5, 10, 30, I64_MAX] and sr.tolist() == [0, 0, 1, 9]
    assert ln.tolist() == [17, 60, 20, 0]
    # all 64 bits, signed: -1 before 0 before 2^32, an affine time against an array
    z = np.zeros(64, np.uint8)
    qa = queue(z, [1, 1], 0, now0=-1, now_step=(1 << 32) + 1)  # -1, 2^32
    qb = queue(z, [1, 1], 1, pos=[0, 16], now=[0, 1 << 32])
    count, fr, ln, nw, ind, sr, wh = merge_reference([qa, qb], 64, 4)
    assert nw.tolist() == [-1, 0, 1 << 32, 1 << 32] and wh.tolist() == [0, 1, 0, 1]
