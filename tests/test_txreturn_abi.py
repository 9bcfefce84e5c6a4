"""vp_tx_return's boundary without a GPU: the ctypes mirrors of
vp_tx_return_stats and vp_tx_way_home (and of vp_dev_batch, which the call
takes twice) have the header's C layout, compiled here with gcc as
test_rxunpack_abi.py does for its struct; the two constants are the header's;
the library exports the call and the binding declares it; every NF class
shares NfBase.tx_return; the call refuses, before it reads a context,
everything its contract lists that needs none; Chain checks `exits`; and the
numpy model the GPU tests compare against (txreturnref.py) gives the
contract's bytes on hand-computed examples."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vigor_amd
from txreturnref import RET_DROP, RET_SKIP, return_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"vp_tx_return_stats": "TxReturnStatsC", "vp_tx_way_home": "TxWayHomeC",
           "vp_dev_batch": "DevBatchC"}


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("txreturnabi")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vigpath.h"',
             "int main(void) {",
             '  printf("VP_RET_SKIP %u\\n", (unsigned)VP_RET_SKIP);',
             '  printf("VP_RET_DROP %u\\n", (unsigned)VP_RET_DROP);']
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
    assert [f for f, _ in vigor_amd.TxReturnStatsC._fields_] == [
        "returned", "dropped", "skipped", "dup", "bad_home"]
    assert [f for f, _ in vigor_amd.TxWayHomeC._fields_] == [
        "home", "port", "on_drop", "on_flood", "on_bad", "stats"]
    assert C.sizeof(vigor_amd.TxReturnStatsC) == 40
    assert vigor_amd.RET_SKIP == c_layout["VP_RET_SKIP"] == RET_SKIP == 0x10000
    assert vigor_amd.RET_DROP == c_layout["VP_RET_DROP"] == RET_DROP == 0x10001


def test_library_exports_and_binding():
    assert "vp_tx_return" in vigor_amd.EXPORTS
    L = C.CDLL(os.path.join(ROOT, "vigor_amd", "libvigpath.so"))
    assert hasattr(L, "vp_tx_return")
    fn = vigor_amd.lib().vp_tx_return
    assert fn.restype is C.c_int and len(fn.argtypes) == 5


def test_nfbase_has_tx_return():
    from vigor_amd.nf import NfBase
    assert callable(NfBase.tx_return)
    for cls in (vigor_amd.Nat, vigor_amd.Bridge, vigor_amd.Lb, vigor_amd.Fw, vigor_amd.Pol):
        assert cls.tx_return is NfBase.tx_return
    assert callable(vigor_amd.Chain.process_device)


def test_einval_before_any_context_is_read():
    """Every refusal the call makes before it reads a context: `ctx` stands
    for one (memory of ours, never a real context) and is not dereferenced on
    any of these paths. The refusals that read n_devices (a bad port[d] below
    it) are in the GPU test."""
    L = vigor_amd.lib()
    E = vigor_amd.VP_EINVAL
    mem = (C.c_uint8 * 8192)()
    base = (C.addressof(mem) + 15) & ~15
    ctx = C.c_void_p(base)

    def batch(**kw):
        b = dict(frames=base, slot=64, n=4, in_dev=None, out_dev=base, in_port=0)
        b.update(kw)
        return vigor_amd.DevBatchC(**b)

    def home(**kw):
        return batch(**dict(dict(frames=base + 4096), **kw))

    def way(**kw):
        a = dict(home=base, on_drop=RET_DROP, on_flood=0xFFFF, on_bad=RET_SKIP, stats=None)
        a.update(kw)
        return vigor_amd.TxWayHomeC(**a)

    def rc(h, f, g, w):
        ref = [C.byref(x) if x is not None else None for x in (f, g, w)]
        return L.vp_tx_return(h, ref[0], ref[1], ref[2], None)

    assert rc(None, batch(), home(), way()) == E
    assert rc(ctx, None, home(), way()) == E
    assert rc(ctx, batch(), None, way()) == E
    assert rc(ctx, batch(), home(), None) == E
    assert rc(ctx, batch(frames=None), home(), way()) == E
    assert rc(ctx, batch(out_dev=None), home(), way()) == E
    assert rc(ctx, batch(), home(frames=None), way()) == E
    assert rc(ctx, batch(), home(out_dev=None), way()) == E
    for bad_slot in (0, 48, 72, 1000):
        assert rc(ctx, batch(slot=bad_slot), home(), way()) == E
        assert rc(ctx, batch(), home(slot=bad_slot), way()) == E
    assert rc(ctx, batch(frames=base + 8), home(), way()) == E
    assert rc(ctx, batch(), home(frames=base + 4096 + 8), way()) == E
    assert rc(ctx, batch(in_port=0x10000), home(), way()) == E
    assert rc(ctx, batch(), home(in_port=0x10000), way()) == E
    for field in ("on_drop", "on_flood", "on_bad"):
        for bad in (0x10002, 0xFFFFFFFF, 0x20000):
            assert rc(ctx, batch(), home(), way(**{field: bad})) == E
    # overlapping slot ranges: partly; wholly with a home array; wholly with
    # another slot -- only the same frames, equal slots and no home array is
    # the in-place form
    assert rc(ctx, batch(), home(frames=base + 64), way()) == E
    assert rc(ctx, batch(), home(frames=base), way()) == E
    assert rc(ctx, batch(slot=128, n=2), home(frames=base), way(home=None)) == E


def _stage(nd=2):
    class Stage:
        class cfg:
            n_devices = nd
    return Stage()


def test_chain_checks_exits():
    links = [(0, 1, 1, 0)]
    c = vigor_amd.Chain([_stage(), _stage(3)], links, exits={(0, 0): 0, (1, 1): 7, (1, 2): 0xFFFF})
    assert c.exits == {(0, 0): 0, (1, 1): 7, (1, 2): 0xFFFF}
    assert vigor_amd.Chain([_stage(), _stage()], links).exits == {}
    for bad in ({(0, 1): 3},       # a linked port
                {(0, 2): 3},       # a port stage 0 does not have
                {(2, 0): 3},       # a stage the chain does not have
                {(1, -1): 3},
                {(1, 1): 0x10000},  # beyond 16 bits
                {(1, 1): -1}):
        with pytest.raises(ValueError):
            vigor_amd.Chain([_stage(), _stage()], links, exits=bad)
    # the actions of each stage: linked -> skip, exit -> its number, else drop
    c = vigor_amd.Chain([_stage(4), _stage()], [(0, 2, 1, 0)], exits={(0, 0): 5, (1, 1): 6})
    assert c.way_home(0) == ([5, RET_DROP, RET_SKIP, RET_DROP], RET_DROP, RET_SKIP, RET_DROP)
    assert c.way_home(1) == ([RET_DROP, 6], RET_DROP, RET_DROP, RET_DROP)
    c = vigor_amd.Chain([_stage()], [], exits={(0, 0): 0, (0, 1): 1})
    assert c.way_home(0) == ([0, 1], RET_DROP, 0xFFFF, RET_DROP)


def _slots(n, slot, first):
    """n slots whose bytes are all different from zero and from one another's
    neighbours: slot k holds first + k in every byte."""
    return np.repeat((np.arange(n) + first).astype(np.uint8), slot)


def test_model_first_of_run_and_each_action():
    # seven entries on a stage with 3 ports, in ports given per entry; home has
    # 6 slots of 64 bytes filled with 0xEE and out 0xBBBB
    out = [1, 2, 0, 0xFFFF, 1, 9, 2]
    inp = [0, 0, 0, 1, 1, 2, 0]
    hom = [0, 0, 1, 2, 3, 4, 9]   # entry 1 repeats home 0; entry 6 is beyond home
    fr = _slots(7, 64, 1)
    hf, ho, st = return_reference(fr, 64, out, inp, np.full(6 * 64, 0xEE, np.uint8), 64,
                                  np.full(6, 0xBBBB, np.uint16), [3, 3, 4, 4, 5, 5], 3,
                                  [RET_SKIP, 7, RET_DROP], RET_DROP, 0xFFFF, 0x1234, home=hom)
    # entry 0: port 1 -> 7. entry 1: not a first. entry 2: out == in -> drop ->
    # home 1's in, 3. entry 3: flood -> 0xFFFF. entry 4: out == in (1) -> drop
    # -> home 3's in, 4. entry 5: port 9 of 3 -> on_bad. entry 6: home 9 >= 6.
    assert ho.tolist() == [7, 3, 0xFFFF, 4, 0x1234, 0xBBBB]
    s = hf.reshape(6, 64)
    assert (s[0] == 1).all() and (s[1] == 3).all() and (s[2] == 4).all() and (s[3] == 5).all()
    assert (s[4] == 6).all() and (s[5] == 0xEE).all()  # slot 5: nobody's home
    assert st == {"returned": 5, "dropped": 2, "skipped": 0, "dup": 1, "bad_home": 1}
    # the same with everything skipped: entry 0 leaves home 0 alone, and entry
    # 1, not a first, does not step in; entry 6 counts as skipped and as bad
    hf, ho, st = return_reference(fr, 64, out, inp, np.full(6 * 64, 0xEE, np.uint8), 64,
                                  np.full(6, 0xBBBB, np.uint16), 3, 3,
                                  [RET_SKIP, RET_SKIP, RET_SKIP], RET_SKIP, RET_SKIP, RET_SKIP,
                                  home=hom)
    assert ho.tolist() == [0xBBBB] * 6 and (hf == 0xEE).all()
    assert st == {"returned": 0, "dropped": 0, "skipped": 6, "dup": 1, "bad_home": 1}


def test_model_clipping_zero_fill_and_untouched_slots():
    fr = _slots(3, 128, 1)
    fr[64:128] = 0x77  # the second half of slot 0
    # 128 -> 64: clipped to the home slot; home NULL: entry k's home is k
    hf, ho, st = return_reference(fr, 128, [1, 1, 1], 0, np.full(4 * 64, 0xEE, np.uint8), 64,
                                  np.full(4, 0xBBBB, np.uint16), 0, 2, [0, 1], RET_DROP, 0, 0)
    s = hf.reshape(4, 64)
    assert (s[0] == 1).all() and (s[1] == 2).all() and (s[2] == 3).all() and (s[3] == 0xEE).all()
    assert ho.tolist() == [1, 1, 1, 0xBBBB] and st["returned"] == 3
    # 64 -> 128: the narrow slot, then zero up to the home slot's end
    hf, ho, st = return_reference(_slots(2, 64, 1), 64, [1, 0], 0,
                                  np.full(3 * 128, 0xEE, np.uint8), 128,
                                  np.full(3, 0xBBBB, np.uint16), 9, 2, [0, 1], RET_DROP, 0, 0,
                                  home=[2, 2])
    s = hf.reshape(3, 128)
    assert (s[:2] == 0xEE).all() and (s[2, :64] == 1).all() and not s[2, 64:].any()
    assert ho.tolist() == [0xBBBB, 0xBBBB, 1] and st["dup"] == 1
    # in place: no frame byte moves, out is translated, drops take the home in
    fr = _slots(3, 64, 1)
    hf, ho, st = return_reference(fr, 64, [1, 0, 0xFFFF], 0, fr, 64, [1, 0, 0xFFFF], 0, 2,
                                  [RET_SKIP, 5], RET_DROP, RET_SKIP, RET_DROP, in_place=True)
    assert hf.tobytes() == fr.tobytes() and ho.tolist() == [5, 0, 0xFFFF]
    assert st == {"returned": 2, "dropped": 1, "skipped": 1, "dup": 0, "bad_home": 0}
    # n == 0: nothing written, the counts zero
    hf, ho, st = return_reference(np.zeros(0, np.uint8), 64, [], 0, fr, 64, [1, 2, 3], 0, 2,
                                  [0, 1], 0, 0, 0)
    assert hf.tobytes() == fr.tobytes() and ho.tolist() == [1, 2, 3] and not any(st.values())
