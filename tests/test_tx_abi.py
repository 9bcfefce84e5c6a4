"""vp_tx_build's boundary without a GPU: the ctypes mirrors of vp_tx_stats and
vp_tx_lists have the header's C layout (compiled here with gcc, as
test_abi_layout.py does for the older structs), the binding is declared, and
the numpy reference the GPU tests compare against (txref.py) gives nf.c's
transmit decisions on hand-written cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vigor_amd
from txref import MAX_DEV, STATS_WORDS, tx_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 0xFFFF


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    pairs = {"vp_tx_stats": vigor_amd.TxStatsC, "vp_tx_lists": vigor_amd.TxListsC}
    d = tmp_path_factory.mktemp("txabi")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vigpath.h"',
             "int main(void) {"]
    for cname, py in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in py._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));'
                         % (cname, fname, cname, fname))
    lines += ["  return 0;", "}"]
    src = d / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = d / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        a, b, v = line.split()
        got[(a, b)] = int(v)
    return pairs, got


@pytest.mark.parametrize("cname", ["vp_tx_lists", "vp_tx_stats"])
def test_ctypes_mirror_matches_header(c_layout, cname):
    pairs, got = c_layout
    py = pairs[cname]
    assert C.sizeof(py) == got[(cname, "size")], cname
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == got[(cname, fname)], (cname, fname)


def test_stats_words_are_the_struct():
    assert C.sizeof(vigor_amd.TxStatsC) == 8 * STATS_WORDS
    assert vigor_amd.TxStatsC.bytes.offset == 8 * MAX_DEV
    assert vigor_amd.TxStatsC.dropped.offset == 16 * MAX_DEV
    assert MAX_DEV == vigor_amd.MAX_DEV


def test_binding_is_declared():
    assert "vp_tx_build" in vigor_amd.EXPORTS
    assert vigor_amd.TX_BLOCK_PACKETS > 0 and vigor_amd.TX_BLOCK_PACKETS % 64 == 0


def _stats(packets, nbytes, dropped, flooded, bad):
    s = np.zeros(STATS_WORDS, np.uint64)
    s[:len(packets)] = packets
    s[MAX_DEV:MAX_DEV + len(nbytes)] = nbytes
    s[2 * MAX_DEV:] = (dropped, flooded, bad)
    return s


def test_reference_nf_loop_sequence():
    """drop, flood, tx, tx, flood, drop on three ports: host/nf_loop.c prints
    "packets 6 tx 2 drop 2 flood 2" and its tx masks are the lists' columns."""
    out = [0, F, 2, 0, F, 1]
    ins = [0, 1, 0, 2, 2, 1]
    lens = [60, 100, 64, 1500, 70, 61]
    idx, off, st = tx_reference(out, ins, lens, 3, 100)
    # port 0: flood(1), tx(3), flood(4); port 1: flood(4); port 2: flood(1), tx(2)
    assert idx.tolist() == [1, 3, 4, 4, 1, 2]
    assert off.tolist() == [0, 3, 4, 6]
    assert np.array_equal(st, _stats([3, 1, 2], [1670, 70, 164], 2, 2, 0))
    unicast = int(st[:MAX_DEV].sum()) - sum(
        sum(1 for d in range(3) if d != i) for o, i in zip(out, ins) if o == F and o != i)
    assert (unicast, int(st[2 * MAX_DEV]), int(st[2 * MAX_DEV + 1])) == (2, 2, 2)


def test_reference_rule_order_and_bad_ports():
    # out == in wins over flood and over a bad port; 3 and 0xFFFE are bad on 3 ports
    out = [F, 7, 3, 0xFFFE, 2]
    ins = [F, 7, 0, 0, 0]
    idx, off, st = tx_reference(out, ins, [10, 20, 30, 40, 50], 3, 10)
    assert idx.tolist() == [4] and off.tolist() == [0, 0, 0, 1]
    assert np.array_equal(st, _stats([0, 0, 1], [0, 0, 50], 2, 0, 2))


def test_reference_flood_edges():
    # one device: a flood from port 0 goes nowhere, and is still a flood
    idx, off, st = tx_reference([F, F], 0, [64, 64], 1, 10)
    assert idx.size == 0 and off.tolist() == [0, 0]
    assert np.array_equal(st, _stats([0], [0], 0, 2, 0))
    # an input port >= n_devices skips no port
    idx, off, st = tx_reference([F], [9], [64], 2, 10)
    assert idx.tolist() == [0, 0] and off.tolist() == [0, 1, 2]
    assert np.array_equal(st, _stats([1, 1], [64, 64], 0, 1, 0))


def test_reference_capacity_keeps_true_offsets():
    out, ins, lens = [1, 0, 1, 1], [0, 1, 0, 0], [1, 2, 3, 4]
    full, off, st = tx_reference(out, ins, lens, 2, 4)
    assert full.tolist() == [1, 0, 2, 3] and off.tolist() == [0, 1, 4]
    cut, off2, st2 = tx_reference(out, ins, lens, 2, 3)
    assert cut.tolist() == [1, 0, 2]
    assert np.array_equal(off, off2) and np.array_equal(st, st2)
    none, off3, _ = tx_reference(out, ins, lens, 2, 0)
    assert none.size == 0 and np.array_equal(off, off3)
    empty, off4, st4 = tx_reference([], [], [], 2, 5)
    assert empty.size == 0 and off4.tolist() == [0, 0, 0] and not st4.any()
