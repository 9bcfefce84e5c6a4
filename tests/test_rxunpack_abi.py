"""vp_rx_unpack's boundary without a GPU: the ctypes mirror of vp_rx_stream has
the header's C layout (compiled here with gcc, as test_txpack_abi.py does for
its struct), the library exports the call and the binding declares it, every NF
class shares NfBase.rx_unpack, Chain rejects an unknown cable, and the numpy
reference the GPU tests compare against (rxunpackref.py) gives the contract's
bytes on a hand-computed example."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vigor_amd
from rxunpackref import unpack_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    py = vigor_amd.RxStreamC
    d = tmp_path_factory.mktemp("rxunpackabi")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vigpath.h"',
             "int main(void) {",
             '  printf("size %zu\\n", sizeof(vp_rx_stream));']
    for fname, _ in py._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(vp_rx_stream, %s));' % (fname, fname))
    lines += ["  return 0;", "}"]
    src = d / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = d / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {a: int(v) for a, v in (line.split() for line in out.splitlines())}


def test_ctypes_mirror_matches_header(c_layout):
    py = vigor_amd.RxStreamC
    assert C.sizeof(py) == c_layout["size"]
    assert [f for f, _ in py._fields_] == ["data", "bytes", "n", "pos", "sel", "meta_n", "len",
                                           "now", "now0", "now_step"]
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == c_layout[fname], fname


def test_library_exports_and_binding():
    assert "vp_rx_unpack" in vigor_amd.EXPORTS
    L = C.CDLL(os.path.join(ROOT, "vigor_amd", "libvigpath.so"))
    assert hasattr(L, "vp_rx_unpack")
    fn = vigor_amd.lib().vp_rx_unpack
    assert fn.restype is C.c_int and len(fn.argtypes) == 4


def test_nfbase_has_rx_unpack():
    from vigor_amd.nf import NfBase
    assert callable(NfBase.rx_unpack)
    for cls in (vigor_amd.Nat, vigor_amd.Bridge, vigor_amd.Lb, vigor_amd.Fw, vigor_amd.Pol):
        assert cls.rx_unpack is NfBase.rx_unpack


def test_chain_rejects_an_unknown_cable():
    class Stage:  # (the cable is checked before anything of a stage is used)
        class cfg:
            n_devices = 2

    with pytest.raises(ValueError):
        vigor_amd.Chain([Stage(), Stage()], [(0, 1, 1, 0)], cable="bogus")
    for cable in ("slots", "stream"):
        assert vigor_amd.Chain([Stage(), Stage()], [(0, 1, 1, 0)], cable=cable).cable == cable
    assert vigor_amd.Chain([Stage(), Stage()], [(0, 1, 1, 0)]).cable == "slots"


def _example():
    """Three frames of 60, 17 and 0 bytes at 0, 64 and 96 of a 96-byte stream
    whose padding holds 0xEE, not zero."""
    f0 = (np.arange(60) + 1).astype(np.uint8)
    f1 = (np.arange(17) + 101).astype(np.uint8)
    data = np.full(96, 0xEE, np.uint8)
    data[0:60] = f0
    data[64:81] = f1
    return data, [60, 17, 0], f0, f1


def test_reference_hand_computed_example():
    data, lens, f0, f1 = _example()
    # five entries: the three frames, frame 1 again at a misaligned position,
    # and an entry whose sel is beyond len[]
    count, fr, ln, nw, sr = unpack_reference(data, 96, 5, lens, 64, 8, pos=[0, 64, 96, 72, 0],
                                             sel=[0, 1, 2, 1, 7], now=[1000, 2000, 3000])
    assert count == 5 and fr.size == 5 * 64 and fr.dtype == np.uint8
    assert ln.tolist() == [60, 17, 0, 0, 0] and ln.dtype == np.uint16
    assert nw.tolist() == [1000, 2000, 3000, 0, 0] and nw.dtype == np.int64
    assert sr.tolist() == [0, 1, 2, 1, 7] and sr.dtype == np.uint32
    s = fr.reshape(5, 64)
    assert s[0, :60].tobytes() == f0.tobytes() and not s[0, 60:].any()
    assert s[1, :17].tobytes() == f1.tobytes() and not s[1, 17:].any()  # (0xEE cleared)
    assert not s[2:].any()


def test_reference_self_describing_positions_and_clamps():
    data, lens, f0, f1 = _example()
    # without pos: 0, 64, 96 are the running sums of the padded lengths
    a = unpack_reference(data, 96, 3, lens, 64, 3, now0=5, now_step=1 << 40)
    b = unpack_reference(data, 96, 3, lens, 64, 3, pos=[0, 64, 96], now0=5, now_step=1 << 40)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
    assert a[3].tolist() == [5, 5 + (1 << 40), 5 + (2 << 40)]
    # one byte short of frame 1's padded end: it is not readable, frame 2 (no
    # bytes) at 96 is not either, frame 0 still is
    count, fr, ln, nw, sr = unpack_reference(data, 95, 3, lens, 64, 3, now0=5, now_step=1)
    assert ln.tolist() == [60, 0, 0] and nw.tolist() == [5, 0, 0] and not fr[64:].any()
    # the capacity cuts the arrays, not the count; a wider slot is zero-filled
    count, fr, ln, nw, sr = unpack_reference(data, 96, 3, lens, 128, 2)
    assert count == 3 and ln.tolist() == [60, 17] and fr.size == 256 and not fr[60:128].any()
    # a position near 2^64 does not wrap into the stream
    count, fr, ln, nw, sr = unpack_reference(data, 96, 1, lens, 64, 1, pos=[(1 << 64) - 16])
    assert ln.tolist() == [0] and not fr.any()
    # a length beyond the slot keeps its value and gives the slot's bytes
    big = np.arange(256, dtype=np.uint8)
    count, fr, ln, nw, sr = unpack_reference(big, 256, 1, [200], 64, 1)
    assert ln.tolist() == [200] and fr.tobytes() == big[:64].tobytes()
    count, fr, ln, nw, sr = unpack_reference(big, 256, 0, [200], 64, 4)
    assert count == 0 and fr.size == 0 and ln.size == 0
