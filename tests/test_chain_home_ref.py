"""The composite reference (chainhomeref.py) alone, without a GPU: on a
hand-made chain result it applies the rules of the composite box, and on the
cases the GPU test runs (fw-nat, fw-nat-lb, bridge-pol) it meets the
conditions that test relies on: every stage has the last word on at least 32
input packets, at least 32 packets come home dropped, and at least 32 come
home on each exit."""
from types import SimpleNamespace

import numpy as np
import pytest

import chainhomeref as H
import chainref as CR


def _reference_run(name):
    case, exits, ports = H.cases()[name]
    trace = case.trace()
    orcs = [st.oracle() for st in case.stages]
    for s, mk in (case.prime or {}).items():
        pf, pl, pd, pn = mk()
        orcs[s].run(pf.copy(), pl, pd, pn, CR.SLOT)
    res = CR.chain_reference(orcs, case.links, *trace, CR.SLOT)
    return case, exits, ports, trace, res


@pytest.mark.parametrize("name", H.NAMES)
def test_cases_meet_the_gpu_tests_conditions(name):
    case, exits, ports, (fr, ln, dv, now), res = _reference_run(name)
    assert all(0 <= e < ports for e in exits.values())
    got = H.conditions(case, exits, res, dv, CR.SLOT)
    assert len(got) == len(case.stages) + 1 + len(exits)
    for what, count in got.items():
        assert count >= 32, "%s: %s is %d" % (name, what, count)


def test_rules_on_a_hand_made_result():
    # two stages: 0 has ports 0..2 (port 1 linked to stage 1's port 0, port 0
    # an exit, port 2 nothing), 1 has ports 0..1 (port 1 an exit)
    case = SimpleNamespace(links=[(0, 1, 1, 0)],
                           stages=[SimpleNamespace(n_devices=3), SimpleNamespace(n_devices=2)])
    exits = {(0, 0): 4, (1, 1): 5}
    slot = 64
    in_dev = np.array([2, 2, 0, 1, 2, 2], np.uint16)
    f0 = np.repeat(np.arange(1, 7, dtype=np.uint8), slot)
    # stage 0: sends 0 on (port 1), 1 to the exit, drops 2 (out == in), 3 to
    # port 2 (no cable), floods 4 and 5 (copies reach stage 1)
    r0 = (np.arange(6), np.array([1, 0, 0, 2, 0xFFFF, 0xFFFF], np.uint16), f0,
          np.full(6, 60, np.uint16))
    # stage 1 received 0, 4, 4 (twice: the first counts) and 5: forwards 0,
    # forwards 4 (the second copy, a drop, does not count), drops 5
    f1 = np.repeat(np.array([11, 12, 13, 14], np.uint8), slot)
    r1 = (np.array([0, 4, 4, 5]), np.array([1, 1, 0, 0], np.uint16), f1,
          np.array([60, 20, 20, 60], np.uint16))
    before = np.full(6, 0xABCD, np.uint16)
    fr, out, st, last = H.home_reference(case, exits, [r0, r1], in_dev, slot, before)
    assert out.tolist() == [5, 4, 0, 1, 5, 2]
    assert last.tolist() == [1, 0, 0, 0, 1, 1]
    s = fr.reshape(6, slot)
    assert [int(x[0]) for x in s] == [11, 2, 3, 4, 12, 14]
    assert st == {"returned": 6, "dropped": 3, "skipped": 3, "dup": 1, "bad_home": 0}
    # cable "stream": behind the link the bytes past the length are zero
    fr, out, st, last = H.home_reference(case, exits, [r0, r1], in_dev, slot, before,
                                         stream=True)
    s = fr.reshape(6, slot)
    assert (s[4, :20] == 12).all() and not s[4, 20:].any()
    assert (s[0, :60] == 11).all() and not s[0, 60:].any() and (s[1] == 2).all()
    # a flood nobody takes up keeps the caller's out; its frame is stage 0's
    r1 = (np.array([0]), np.array([1], np.uint16), f1[:slot], np.array([60], np.uint16))
    fr, out, st, last = H.home_reference(case, exits, [r0, r1], in_dev, slot, before)
    assert out.tolist() == [5, 4, 0, 1, 0xABCD, 0xABCD] and last.tolist() == [1, 0, 0, 0, -1, -1]
    assert (fr.reshape(6, slot)[4] == 5).all()
    # every port an exit: the flood is the composite's own
    case1 = SimpleNamespace(links=[], stages=[SimpleNamespace(n_devices=3)])
    fr, out, st, last = H.home_reference(case1, {(0, 0): 0, (0, 1): 1, (0, 2): 2}, [r0], in_dev,
                                         slot, before)
    assert out.tolist() == [1, 0, 0, 2, 0xFFFF, 0xFFFF]
