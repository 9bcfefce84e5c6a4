"""vp_tx_pack's boundary without a GPU: the ctypes mirror of vp_tx_frames has
the header's C layout (compiled here with gcc, as test_tx_abi.py does for its
structs), the library exports the call and the binding declares it, and the
numpy reference the GPU tests compare against (txpackref.py) gives the
contract's bytes on a hand-computed example."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vigor_amd
from txpackref import pack_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    py = vigor_amd.TxFramesC
    d = tmp_path_factory.mktemp("txpackabi")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vigpath.h"',
             "int main(void) {",
             '  printf("size %zu\\n", sizeof(vp_tx_frames));']
    for fname, _ in py._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(vp_tx_frames, %s));' % (fname, fname))
    lines += ["  return 0;", "}"]
    src = d / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = d / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {a: int(v) for a, v in (line.split() for line in out.splitlines())}


def test_ctypes_mirror_matches_header(c_layout):
    py = vigor_amd.TxFramesC
    assert C.sizeof(py) == c_layout["size"]
    assert [f for f, _ in py._fields_] == ["data", "cap_bytes", "port_off", "pos"]
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == c_layout[fname], fname


def test_library_exports_and_binding():
    assert "vp_tx_pack" in vigor_amd.EXPORTS
    L = C.CDLL(os.path.join(ROOT, "vigor_amd", "libvigpath.so"))
    assert hasattr(L, "vp_tx_pack")
    fn = vigor_amd.lib().vp_tx_pack
    assert fn.restype is C.c_int and len(fn.argtypes) == 5


def test_nfbase_has_tx_pack():
    from vigor_amd.nf import NfBase
    assert callable(NfBase.tx_pack)
    for cls in (vigor_amd.Nat, vigor_amd.Bridge):
        assert cls.tx_pack is NfBase.tx_pack


def _example():
    """4 packets in 64-byte slots; packet 2 is flooded to both ports. Port 0
    sends packets 1 (length 0) and 2, port 1 packets 0 (length 17), 2 and 3."""
    slot = 64
    frames = (np.arange(4 * slot) % 251 + 1).astype(np.uint8)  # no zero byte
    lens = [17, 0, 64, 33]
    idx = [1, 2, 0, 2, 3]
    offset = [0, 2, 5]
    return frames, slot, lens, idx, offset


def test_reference_hand_computed_example():
    frames, slot, lens, idx, offset = _example()
    data, port_off, pos = pack_reference(frames, slot, lens, idx, offset, 5, 2, 1 << 20)
    # pads: 0, 64, 32, 64, 48
    assert pos.tolist() == [0, 0, 64, 96, 160] and pos.dtype == np.uint64
    assert port_off.tolist() == [0, 64, 208] and port_off.dtype == np.uint64
    assert data.size == 208 and data.dtype == np.uint8
    f = frames.reshape(4, slot)
    want = np.concatenate([f[2], f[0][:17], np.zeros(15, np.uint8), f[2], f[3][:33],
                           np.zeros(15, np.uint8)])
    assert data.tobytes() == want.tobytes()


def test_reference_capacity_clamp_and_guard():
    frames, slot, lens, idx, offset = _example()
    # 150 bytes: entries 0..2 fit (they end at 96), entry 3 would end at 160
    data, port_off, pos = pack_reference(frames, slot, lens, idx, offset, 5, 2, 150,
                                         canary=0xA5)
    assert port_off.tolist() == [0, 64, 208] and pos.tolist() == [0, 0, 64, 96, 160]
    assert data.size == 150 and (data[96:] == 0xA5).all()
    f = frames.reshape(4, slot)
    assert data[:64].tobytes() == f[2].tobytes() and data[64:81].tobytes() == f[0][:17].tobytes()
    assert not data[81:96].any()
    # an overflowed list: only the first cap entries, later bounds at pos(cap)
    data, port_off, pos = pack_reference(frames, slot, lens, idx, offset, 3, 2, 1 << 20)
    assert pos.tolist() == [0, 0, 64] and port_off.tolist() == [0, 64, 96] and data.size == 96
    # an index outside the batch occupies nothing; a length beyond the slot is cut
    data, port_off, pos = pack_reference(frames, slot, [17, 0, 100, 33], [2, 4, 7, 0], [0, 1, 4],
                                         4, 2, 1 << 20)
    assert pos.tolist() == [0, 64, 64, 64] and port_off.tolist() == [0, 64, 96]
    assert data[:64].tobytes() == f[2].tobytes()
    # nothing to send
    data, port_off, pos = pack_reference(frames, slot, lens, [], [0, 0, 0], 0, 2, 64)
    assert data.size == 0 and pos.size == 0 and port_off.tolist() == [0, 0, 0]
