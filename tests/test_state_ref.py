"""tests/stateref.py against itself: unpack(pack(x)) == x on hand-made states,
the tail normalisation, and the byte layout include/vigpath.h describes (sizes,
alignment, zero pads). CPU only."""
import struct

import pytest

import stateref as SR


def _table(cap, lru, freed, fresh, vsz=0, t0=100):
    return {"capacity": cap, "fresh_next": fresh, "value_size": vsz, "lru": list(lru),
            "freed": list(freed), "ts": [t0 + j // 2 for j in range(len(lru))],
            "key": [bytes([i & 0xFF, i >> 8]) + bytes(14) for i in lru],
            "value": [bytes([7] * vsz) for _ in lru]}


CAP = 8
STATES = {
    "empty": {"kind": "nat", "last_now": -1, "tables": [_table(CAP, [], [], 0)]},
    "one": {"kind": "nat", "last_now": 100, "tables": [_table(CAP, [0], [], 1)]},
    "full": {"kind": "nat", "last_now": 104,
             "tables": [_table(CAP, [3, 1, 2, 0, 7, 6, 5, 4], [], CAP)]},
    "stack": {"kind": "fw", "last_now": 101,
              "tables": [_table(CAP, [4, 0, 2], [1, 3], 5, vsz=4)]},
    "two_tables": {"kind": "lb", "last_now": 101,
                   "tables": [_table(CAP, [1, 0, 3], [2], 4, vsz=4),
                              _table(4, [0, 1, 2], [], 3, vsz=8)]},
    "pol": {"kind": "pol", "last_now": 100, "tables": [_table(CAP, [5], [0, 1, 2, 3, 4], 6, 16)]},
}


@pytest.mark.parametrize("name", sorted(STATES))
def test_roundtrip(name):
    s = STATES[name]
    blob = SR.pack(s)
    assert SR.unpack(blob) == s
    assert SR.pack(SR.unpack(blob)) == blob


@pytest.mark.parametrize("name", sorted(STATES))
def test_layout(name):
    s = STATES[name]
    blob = SR.pack(s)
    magic, version, kind, nt, total, last_now = struct.unpack_from("<IIIIQq", blob, 0)
    assert blob[:4] == b"VPST" and magic == SR.MAGIC and version == 1
    assert kind == SR.KINDS[s["kind"]] and nt == len(s["tables"])
    assert total == len(blob) and total % 16 == 0 and last_now == s["last_now"]
    at = 32
    for t in s["tables"]:
        cap, n, fresh, vsz, nf, r0, r1, r2 = struct.unpack_from("<8I", blob, at)
        assert (cap, n, fresh, vsz, nf) == (t["capacity"], len(t["lru"]), t["fresh_next"],
                                            t["value_size"], len(t["freed"]))
        assert r0 == r1 == r2 == 0
        assert n + nf + (cap - fresh) == cap
        at += 32
        for width, count in ((4, n), (4, nf), (8, n), (16, n), (vsz, n)):
            assert at % 16 == 0
            size = width * count
            pad = -size % 16
            assert blob[at + size:at + size + pad] == bytes(pad)
            at += size + pad
    assert at == len(blob)
    # size follows the entries, not the capacity
    big = dict(s, tables=[dict(t, capacity=t["capacity"] + 1000) for t in s["tables"]])
    assert len(SR.pack(big, canon=False)) == len(blob)


def test_tail_normalisation():
    """A freed fresh_next - 1 at the bottom of the stack (the end of freed[])
    belongs to the never-used tail, and so does the run below it."""
    raw = _table(CAP, [0, 1], [3, 5, 4, 2], 6)  # hand-out order 3 5 4 2 6 7
    # 2 does not continue the run 6 7 downwards, so nothing moves
    assert SR.normalise(raw)["freed"] == [3, 5, 4, 2]
    raw = _table(CAP, [0, 1], [3, 2, 4, 5], 6)  # hand-out order 3 2 4 5 6 7
    n = SR.normalise(raw)
    assert n["freed"] == [3, 2] and n["fresh_next"] == 4
    a = SR.pack({"kind": "nat", "last_now": 101, "tables": [raw]})
    b = SR.pack({"kind": "nat", "last_now": 101, "tables": [n]})
    assert a == b
    assert SR.unpack(a)["tables"][0]["freed"] == [3, 2]
    # the whole stack is the tail; a table with nothing free has none
    assert SR.normalise(_table(CAP, [0], [1, 2, 3], 4))["fresh_next"] == 1
    assert SR.normalise(_table(CAP, [0], [1, 2, 3], 4))["freed"] == []
    full = _table(CAP, range(7), [7], CAP)
    assert SR.normalise(full)["fresh_next"] == 7 and SR.normalise(full)["freed"] == []


def test_unpack_rejects_what_it_cannot_walk():
    blob = SR.pack(STATES["stack"])
    for bad in (blob[:-1], blob + b"\0", b"X" + blob[1:], blob[:31]):
        with pytest.raises(ValueError):
            SR.unpack(bad)
    pad_at = 32 + 32 + 12  # behind lru[3]
    assert blob[pad_at] == 0
    with pytest.raises(ValueError):
        SR.unpack(blob[:pad_at] + b"\1" + blob[pad_at + 1:])
