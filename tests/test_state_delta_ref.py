"""tests/deltaref.py against itself and the oracle: apply(s0, diff(s0, s1,
touched)) == s1 for states the oracle reaches along tests/statecases.py's
traces and for hand-made ones with removals and re-used indices, the byte
layout include/vigpath.h describes, and a ValueError for every malformed case
the header lists (tests/deltacases.py). CPU only."""
import struct

import pytest

import deltacases as DC
import deltaref as DR
import statecases as SC
import stateref as SR


CAP = 16
S0, S1, TOUCHED = DC.victim("fw", cap=CAP)


def _oracle_states(kind, cuts=(150, 151, 400, 600)):
    """The oracle's state after each cut of the kind's distinct trace (one
    stamp per packet: a dump's ts order is the LRU order)."""
    tr = SC.distinct_trace(kind)
    o = SC.oracle(kind, expire_us=60_000_000)
    out, at = [], 0
    for c in cuts:
        o.run(tr[0][at * 64:c * 64].copy(), tr[1][at:c], tr[2][at:c], tr[3][at:c], 64)
        out.append(SR.state_from_dump(kind, SC.dump(kind, o), tr[3][c - 1]))
        at = c
    return out


def _touched(s0, s1):
    return [{i for j, i in enumerate(t["lru"]) if t["ts"][j] > s0["last_now"]}
            for t in s1["tables"]]


def test_apply_of_diff_hand_made():
    d = DR.diff(S0, S1, TOUCHED, base=(5, 0), mark=(9, 0))
    assert d["tables"][0]["idx"] == [7, 3, 5, 1, 10, 11] and d["tables"][0]["n_live"] == 10
    assert DR.apply(S0, d) == S1
    assert DR.apply(S0, DR.unpack(DR.pack(d))) == S1
    # the empty delta changes nothing
    e = DR.diff(S0, S0, [set()])
    assert e["tables"][0]["idx"] == [] and DR.apply(S0, e) == S0


@pytest.mark.parametrize("kind", SC.KINDS)
def test_apply_of_diff_along_the_oracle(kind):
    states = _oracle_states(kind)
    for s0, s1 in zip(states[:-1], states[1:]):
        d = DR.diff(s0, s1, _touched(s0, s1))
        assert DR.apply(s0, d) == s1
        assert DR.unpack(DR.pack(d)) == d
    # cumulative: from the first state to the last in one delta
    d = DR.diff(states[0], states[-1], _touched(states[0], states[-1]))
    assert DR.apply(states[0], d) == states[-1]
    assert sum(len(t["idx"]) for t in d["tables"]) > 0


def test_layout():
    d = DR.diff(S0, S1, TOUCHED, base=(5, 2), mark=(9, 2))
    blob = DR.pack(d)
    assert DR.unpack(blob) == d and DR.pack(DR.unpack(blob)) == blob
    magic, version, kind, nt, total, last_now, bs, be, ms, me = struct.unpack_from(
        "<IIIIQqQQQQ", blob, 0)
    assert blob[:4] == b"VPSD" and magic == DR.MAGIC and version == 1
    assert (kind, nt, total, last_now) == (SR.KINDS["fw"], 1, len(blob), 140)
    assert (bs, be, ms, me) == (5, 2, 9, 2)
    cap, n_live, fresh, vsz, nf, n, r0, r1 = struct.unpack_from("<8I", blob, 64)
    assert (cap, n_live, fresh, vsz, nf, n, r0, r1) == (CAP, 10, 12, 4, 2, 6, 0, 0)
    at = 96
    for width, count in ((4, n), (4, nf), (8, n), (16, n), (vsz, n)):
        assert at % 16 == 0
        size = width * count
        assert blob[at + size:at + size + (-size % 16)] == bytes(-size % 16)
        at += size + (-size % 16)
    assert at == len(blob)
    assert struct.unpack_from("<6I", blob, 96) == (7, 3, 5, 1, 10, 11)


def test_unpack_rejects_what_it_cannot_walk():
    blob = DR.pack(DR.diff(S0, S1, TOUCHED))
    for bad in (blob[:-1], blob + b"\0", b"X" + blob[1:], blob[:63]):
        with pytest.raises(ValueError):
            DR.unpack(bad)


def _victim(kind):
    s0, s1, touched = DC.victim(kind)
    d = DR.diff(s0, s1, touched)
    assert DR.apply(s0, d) == s1
    return s0, d


@pytest.mark.parametrize("kind,name", [(k, n) for k in ("fw", "lb") for n in DC.names_for(k)])
def test_malformed_delta_raises(kind, name):
    s0, d = _victim(kind)
    blob = DC.mutations(s0, d)[name]
    with pytest.raises(ValueError):
        DR.apply(s0, DR.unpack(blob))
