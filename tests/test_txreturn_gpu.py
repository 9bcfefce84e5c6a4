"""vp_tx_return on the GPU, byte for byte against txreturnref.return_reference
(the contract of include/vigpath.h as a per-entry loop).

Every case fills the home batch -- frames and out_dev -- and the stats with a
canary first, with a canary tail behind each, and compares the buffers whole,
so the slots nobody comes home to, the out ports of skipped packets and the
bytes behind the batch are checked with the rest. The returning frames hold
neither zero nor the canary, so zero fill, moved bytes and untouched bytes
cannot pass for one another. The call reads n_devices, the GPU and the default
stream of its context and nothing else, so a small vigbridge context serves."""
import numpy as np
import pytest
import torch

import vigor_amd
from tracegen import mixed_bridge_trace
from txreturnref import RET_DROP, RET_SKIP, STATS, return_reference

pytestmark = pytest.mark.gpu

F = 0xFFFF
CANARY = 0xA5
TAIL = 64  # canary entries kept behind every buffer
ND = 4
COUNTS = [1, 63, 64, 65, 2047, 2048, 2049, 5000]  # turn, wave and block edges
SLOTS = [(64, 64), (64, 128), (128, 64), (80, 64), (1536, 1536)]
# (ports, on_drop, on_flood, on_bad): between them every kind of action in
# every place
ACTIONS = [([5, RET_SKIP, RET_DROP, F], RET_DROP, 9, RET_SKIP),
           ([RET_SKIP, 6, 0, RET_DROP], RET_SKIP, RET_DROP, 0xFFFE),
           ([1, 2, 3, 0], 0x1234, F, RET_DROP)]
# in ports of (the returning batch, the home batch): arrays, or one port
IN_MODES = [("array", "array"), (2, 1), ("array", 3), (0, "array")]

_ctx = {}


def bridge(nd=ND):
    if nd not in _ctx:
        _ctx[nd] = vigor_amd.Bridge(vigor_amd.bridge_config_from_args([], nd), gpu=0)
    return _ctx[nd]


def dev(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    signed = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed)).to("cuda:0")


def filled(count, width):
    t = torch.full(((count + TAIL) * width,), CANARY, dtype=torch.uint8, device="cuda:0")
    return t if width == 1 else t.view({2: torch.int16, 8: torch.int64}[width])


def homes(rng, n):
    """Home indices that do not decrease, in runs of 1 to 5 equal ones with a
    gap now and then; one run lies across every 64-entry boundary it can reach
    among the first few and across entry 2,048."""
    h = np.zeros(n, np.int64)
    k, cur = 0, int(rng.integers(0, 3))
    while k < n:
        run = int(rng.integers(1, 6))
        h[k:k + run] = cur
        k += run
        cur += int(rng.integers(1, 3))
    for edge in (64, 128, 2048, 4096):
        if edge + 1 <= n:  # entries edge - 2 .. edge share a home
            h[edge - 2:edge + 1] = h[edge - 2]
    return np.maximum.accumulate(h).astype(np.uint32)


def draw(rng, n, fslot, with_home, in_modes):
    """One case's inputs on the host."""
    fr = rng.integers(1, 255, n * fslot + 16).astype(np.uint8)[:n * fslot]
    fr[fr == CANARY] = 0x11
    out = rng.choice([0, 1, 2, 3, F, 7, 0x1234], n).astype(np.uint16)
    home = homes(rng, n) if with_home else None
    top = int(home[-1]) + 1 if with_home and n else n
    # a few homes beyond the home batch where there are enough, else slots
    # behind the last home that stay untouched
    hn = top - 2 if top > 8 else top + 3
    f_in = rng.integers(0, ND, n).astype(np.uint16) if in_modes[0] == "array" else in_modes[0]
    h_in = rng.integers(0, ND, hn).astype(np.uint16) if in_modes[1] == "array" else in_modes[1]
    return fr, out, home, hn, f_in, h_in


class Returned:
    """One vp_tx_return call over a canary-filled home batch, back on the host."""

    def __init__(self, nf, fr, fslot, out, f_in, hslot, hn, h_in, action, home=None,
                 stream=None):
        self.args = (fr, fslot, out, f_in, hslot, hn, h_in, action, home)
        self.hf, self.ho, self.st = filled(hn * hslot, 1), filled(hn, 2), filled(len(STATS), 8)
        ports, on_drop, on_flood, on_bad = action
        torch.cuda.synchronize()
        nf.tx_return(dev(fr, np.uint8), fslot, dev(out, np.uint16),
                     f_in if isinstance(f_in, int) else dev(f_in, np.uint16),
                     self.hf[:hn * hslot], hslot, self.ho[:hn],
                     h_in if isinstance(h_in, int) else dev(h_in, np.uint16),
                     ports, on_drop, on_flood, on_bad,
                     home=dev(home, np.uint32) if home is not None else None,
                     stats=self.st[:len(STATS)], stream=stream)
        torch.cuda.synchronize()

    def check(self):
        fr, fslot, out, f_in, hslot, hn, h_in, action, home = self.args
        ports, on_drop, on_flood, on_bad = action
        ef, eo, est = return_reference(fr, fslot, out, f_in, np.full(hn * hslot, CANARY, np.uint8),
                                       hslot, np.full(hn, CANARY * 0x101, np.uint16), h_in, ND,
                                       ports, on_drop, on_flood, on_bad, home=home)
        gf = self.hf.cpu().numpy()
        go = self.ho.cpu().numpy().view(np.uint16)
        gs = self.st.cpu().numpy().view(np.uint64)
        assert dict(zip(STATS, gs[:len(STATS)].tolist())) == est
        assert (gs[len(STATS):] == int.from_bytes(bytes([CANARY]) * 8, "little")).all()
        bad = np.nonzero(go[:hn] != eo)[0]
        assert bad.size == 0, "out_dev differs at home %s: %s vs %s" % (
            bad[:8], go[bad[:8]], eo[bad[:8]])
        assert (go[hn:] == CANARY * 0x101).all(), "out_dev written behind the home batch"
        g2, e2 = gf[:hn * hslot].reshape(hn, hslot), ef.reshape(hn, hslot)
        badf = np.nonzero((g2 != e2).any(axis=1))[0]
        assert badf.size == 0, "frames differ at home slots %s" % badf[:8]
        assert (gf[hn * hslot:] == CANARY).all(), "frames written behind the home batch"
        return est


def case_id(n, slots, with_home):
    return COUNTS.index(n) * 10 + SLOTS.index(slots) * 2 + int(with_home)


@pytest.mark.parametrize("with_home", [False, True], ids=["homenull", "home"])
@pytest.mark.parametrize("slots", SLOTS, ids=["%dto%d" % s for s in SLOTS])
@pytest.mark.parametrize("n", COUNTS)
def test_matches_the_model(n, slots, with_home):
    c = case_id(n, slots, with_home)
    rng = np.random.default_rng(1000 + c)
    modes, action = IN_MODES[c % len(IN_MODES)], ACTIONS[c % len(ACTIONS)]
    fr, out, home, hn, f_in, h_in = draw(rng, n, slots[0], with_home, modes)
    est = Returned(bridge(), fr, slots[0], out, f_in, slots[1], hn, h_in, action,
                   home=home).check()
    assert est["returned"] + est["dup"] <= n
    if with_home and n >= 2049:  # (the case holds what it is meant to)
        assert est["dup"] > 100 and est["bad_home"] > 0 and home[2046] == home[2048]
        assert home[62] == home[64]


@pytest.mark.parametrize("modes", IN_MODES, ids=["arrays", "ports", "arr-port", "port-arr"])
@pytest.mark.parametrize("a", range(len(ACTIONS)))
def test_every_action_with_in_arrays_and_in_ports(a, modes):
    rng = np.random.default_rng(50 + a)
    n = 700
    fr, out, home, hn, f_in, h_in = draw(rng, n, 64, True, modes)
    est = Returned(bridge(), fr, 64, out, f_in, 64, hn, h_in, ACTIONS[a], home=home).check()
    assert est["returned"] > 50 and est["dup"] > 50
    if a < 2:
        assert est["dropped"] > 10 and est["skipped"] > 10


def test_runs_of_every_length_across_the_boundaries():
    """Runs of 1 to 5 equal homes laid so that each length lies across a
    64-entry boundary and across the 2,048-entry one, at every offset."""
    rng = np.random.default_rng(7)
    n = 2048 + 64 * 30
    home = np.arange(n, dtype=np.int64) * 8  # (room between the homes)
    case = 0
    for length in range(2, 6):
        for offset in range(1, length):
            edge = 64 * (case + 1) if case % 2 else 2048 + 64 * case
            home[edge - offset:edge - offset + length] = home[edge - offset]
            case += 1
    home[2048 - 2:2048 + 3] = home[2046]
    assert (np.diff(home) >= 0).all()
    home = home.astype(np.uint32)
    fr, out, _, _, f_in, _ = draw(rng, n, 64, False, ("array", "array"))
    hn = int(home[-1]) + 1
    h_in = rng.integers(0, ND, hn).astype(np.uint16)
    est = Returned(bridge(), fr, 64, out, f_in, 64, hn, h_in, ACTIONS[2], home=home).check()
    assert est["dup"] == n - np.unique(home).size


def in_place(n, same_out):
    rng = np.random.default_rng(n)
    fr, out, _, _, f_in, _ = draw(rng, n, 64, False, ("array", "array"))
    ports, on_drop, on_flood, on_bad = action = ACTIONS[0]
    fr_t, out_t, in_t = dev(fr, np.uint8), dev(out, np.uint16), dev(f_in, np.uint16)
    ho_t = out_t if same_out else filled(n, 2)
    st = torch.zeros(len(STATS), dtype=torch.int64, device="cuda:0")
    bridge().tx_return(fr_t, 64, out_t, in_t, fr_t, 64, ho_t[:n], in_t, ports, on_drop, on_flood,
                       on_bad, stats=st)
    torch.cuda.synchronize()
    before = out if same_out else np.full(n, CANARY * 0x101, np.uint16)
    ef, eo, est = return_reference(fr, 64, out, f_in, fr, 64, before, f_in, ND, *action,
                                   in_place=True)
    assert fr_t.cpu().numpy().tobytes() == fr.tobytes(), "a frame byte moved"
    assert ho_t.cpu().numpy().view(np.uint16)[:n].tolist() == eo.tolist()
    if not same_out:
        assert out_t.cpu().numpy().view(np.uint16).tolist() == out.tolist()
        assert (ho_t.cpu().numpy().view(np.uint16)[n:] == CANARY * 0x101).all()
    assert dict(zip(STATS, st.cpu().numpy().view(np.uint64).tolist())) == est
    assert est["skipped"] > 0 and est["dropped"] > 0


@pytest.mark.parametrize("same_out", [False, True], ids=["other-out", "same-out"])
def test_the_batch_that_is_its_own_home(same_out):
    in_place(2049, same_out)


def test_no_entries_writes_zero_stats_and_nothing_else():
    r = Returned(bridge(), np.zeros(0, np.uint8), 64, np.zeros(0, np.uint16), 0, 64, 5, 1,
                 ACTIONS[0])
    est = r.check()
    assert not any(est.values())


def test_refusals_that_read_the_context():
    nf, E = bridge(), vigor_amd.VP_EINVAL
    fr, hf = filled(4 * 64, 1), filled(4 * 64, 1)
    out, ho = filled(4, 2), filled(4, 2)

    def rc(ports, home_frames=hf):
        with pytest.raises(vigor_amd.VigpathError) as e:
            nf.tx_return(fr[:256], 64, out[:4], 0, home_frames[:256], 64, ho[:4], 0, ports,
                         RET_DROP, RET_DROP, RET_DROP)
        return e.value.rc

    assert rc([0, 1, 0x10002, 3]) == E       # a bad action below n_devices
    assert rc([0, 1, 2, 3], fr[64:]) == E    # the two slot ranges overlap
    # beyond n_devices port[] is not read
    nf.tx_return(fr[:256], 64, out[:4], 0, hf[:256], 64, ho[:4], 0, [0, 1, 2, 3, 0x10002],
                 RET_DROP, RET_DROP, RET_DROP)
    torch.cuda.synchronize()


def test_on_another_stream_after_a_process_device():
    """process_device and the return of its batch, in place, enqueued on one
    non-default stream with nothing between them: the return sees the out
    ports the NF wrote."""
    rng = np.random.default_rng(3)
    n = 3000
    fr, ln, dv, now = mixed_bridge_trace(rng, n, 200, n_dev=ND)
    nfs = [vigor_amd.Bridge(vigor_amd.bridge_config_from_args([], ND), gpu=0) for _ in range(2)]
    tens = []
    for nf in nfs:
        tens.append((dev(fr, np.uint8), dev(ln, np.uint16), dev(dv, np.uint16),
                     dev(now, np.int64), torch.zeros(n, dtype=torch.int16, device="cuda:0")))
    f_t, l_t, d_t, n_t, o_t = tens[0]
    nfs[0].process_device(f_t, l_t, d_t, o_t, 64, now=n_t)
    torch.cuda.synchronize()
    want_out = o_t.cpu().numpy().view(np.uint16)
    assert len(set(want_out.tolist())) > 2
    f_t, l_t, d_t, n_t, o_t = tens[1]
    ho = filled(n, 2)
    st = filled(len(STATS), 8)
    S = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    action = ([4, 5, RET_SKIP, RET_DROP], RET_DROP, F, RET_DROP)
    nfs[1].process_device(f_t, l_t, d_t, o_t, 64, now=n_t, stream=S)
    nfs[1].tx_return(f_t, 64, o_t, d_t, f_t, 64, ho[:n], d_t, *action, stats=st[:len(STATS)],
                     stream=S)
    S.synchronize()
    _, eo, est = return_reference(tens[0][0].cpu().numpy(), 64, want_out, dv, fr, 64,
                                  np.full(n, CANARY * 0x101, np.uint16), dv, ND, *action,
                                  in_place=True)
    assert ho.cpu().numpy().view(np.uint16)[:n].tolist() == eo.tolist()
    assert dict(zip(STATS, st.cpu().numpy().view(np.uint64)[:len(STATS)].tolist())) == est
    assert f_t.cpu().numpy().tobytes() == tens[0][0].cpu().numpy().tobytes()
    for nf in nfs:
        nf.close()
