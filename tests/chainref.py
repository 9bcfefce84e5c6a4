"""Reference for vigor_amd.Chain and the chains the GPU test runs.

The reference pushes every packet through the whole chain before the next
one, as boxes joined by cables would: one orc.Oracle per stage, called with
n = 1 per packet and stage; between two stages the slot image is copied into a
fresh slot, and every stage sees the packet's own time. Shares no code with
vigor_amd.Chain.

The cases (configurations, links, traces) live here so that the CPU test can
check, without a GPU, that the reference alone meets the conditions the GPU
test relies on: every stage receives at least a quarter of the input, drops
and forwards at least one packet, and expires at least one entry."""
from types import SimpleNamespace

import numpy as np

import orc
import vigor_amd
from tracegen import mixed_bridge_trace, mixed_fw_trace, mixed_pol_trace
from vigor_amd import traces as T

SLOT = 64
DEV_MACS = [T.mac("02:03:04:05:06:07"), T.mac("12:13:14:15:16:17"),
            T.mac("22:23:24:25:26:27")]
END_MACS = [T.mac("01:23:45:67:89:00"), T.mac("01:23:45:67:89:01"),
            T.mac("01:23:45:67:89:02")]
LB_MACS = [bytes([0x10 * d + i for i in range(6)]) for d in range(3)]


class Stage:
    """One stage of a case: how to make its oracle and its GPU object, how to
    read either's table state as [(alloc, columns...)] and its devices."""

    def __init__(self, kind, n_devices, oracle, gpu, o_dump, g_dump):
        self.kind, self.n_devices = kind, n_devices
        self.cfg = SimpleNamespace(n_devices=n_devices)  # (what Chain reads of a stage)
        self.oracle, self.gpu, self.o_dump, self.g_dump = oracle, gpu, o_dump, g_dump


def fw_stage(max_flows, expire_us, n_dev=2, wan=1):
    args = ["--wan", str(wan), "--expire", str(expire_us), "--max-flows", str(max_flows)]
    for d in range(n_dev):
        args += ["--eth-dest", "%d,%s" % (d, END_MACS[d].hex(":"))]
    return Stage(
        "fw", n_dev,
        lambda: orc.Oracle("fw", orc.fw_cfg(wan=wan, expire_us=expire_us, max_flows=max_flows,
                                            device_macs=DEV_MACS[:n_dev],
                                            endpoint_macs=END_MACS[:n_dev], n_devices=n_dev)),
        lambda: vigor_amd.Fw(vigor_amd.fw_config_from_args(args, n_dev, DEV_MACS[:n_dev]), gpu=0),
        lambda o: [o.fw_dump(max_flows)], lambda g: [g.dump()])


def nat_stage(max_flows, expire_us, n_dev=2, wan=1):
    args = ["--wan", str(wan), "--expire", str(expire_us), "--starting-port", "1000",
            "--max-flows", str(max_flows), "--extip", "192.168.4.2"]
    for d in range(n_dev):
        args += ["--eth-dest", "%d,%s" % (d, END_MACS[d].hex(":"))]
    return Stage(
        "nat", n_dev,
        lambda: orc.Oracle("nat", orc.nat_cfg(wan=wan, start_port=1000,
                                              ext_ip=T.ip4(192, 168, 4, 2), expire_us=expire_us,
                                              max_flows=max_flows, device_macs=DEV_MACS[:n_dev],
                                              endpoint_macs=END_MACS[:n_dev], n_devices=n_dev)),
        lambda: vigor_amd.Nat(vigor_amd.nat_config_from_args(args, n_dev, DEV_MACS[:n_dev]),
                              gpu=0),
        lambda o: [o.nat_dump(max_flows)], lambda g: [g.dump()])


def bridge_stage(capacity, expire_us, n_dev=4):
    args = ["--capacity", str(capacity), "--expire", str(expire_us)]
    return Stage(
        "bridge", n_dev,
        lambda: orc.Oracle("bridge", orc.BridgeCfg(expiration_time=expire_us,
                                                   dyn_capacity=capacity, n_devices=n_dev),
                           statics=[]),
        lambda: vigor_amd.Bridge(vigor_amd.bridge_config_from_args(args, n_dev), gpu=0),
        lambda o: [o.bridge_dump(capacity)], lambda g: [g.dump()])


def pol_stage(capacity, rate, burst, n_dev=2, lan=1, wan=0):
    args = ["--lan", str(lan), "--wan", str(wan), "--rate", str(rate), "--burst", str(burst),
            "--capacity", str(capacity)]
    return Stage(
        "pol", n_dev,
        lambda: orc.Oracle("pol", orc.pol_cfg(lan=lan, wan=wan, rate=rate, burst=burst,
                                              capacity=capacity, n_devices=n_dev)),
        lambda: vigor_amd.Pol(vigor_amd.pol_config_from_args(args, n_dev), gpu=0),
        lambda o: [o.pol_dump(capacity)], lambda g: [g.dump()])


def lb_stage(flow_cap, bcap, height, fexp, bexp, n_dev=3, wan=2):
    args = ["--flow-capacity", str(flow_cap), "--backend-capacity", str(bcap),
            "--cht-height", str(height), "--flow-expiration", str(fexp),
            "--backend-expiration", str(bexp), "--wan", str(wan)]

    def oracle():
        c = orc.LbCfg(flow_capacity=flow_cap, flow_expiration_time=fexp, backend_capacity=bcap,
                      cht_height=height, backend_expiration_time=bexp, wan_device=wan,
                      n_devices=n_dev)
        for d in range(n_dev):
            c.device_macs[d][:] = list(LB_MACS[d])
        return orc.Oracle("lb", c)

    return Stage(
        "lb", n_dev, oracle,
        lambda: vigor_amd.Lb(vigor_amd.lb_config_from_args(args, n_dev, LB_MACS[:n_dev]), gpu=0),
        lambda o: list(o.lb_dump(flow_cap, bcap)), lambda g: list(g.dump()))


class Case:
    def __init__(self, stages, links, trace, prime=None):
        self.stages, self.links, self.trace, self.prime = stages, links, trace, prime


def _fw_trace(seed, n, n_flows):
    """mixed_fw_trace on two devices (LAN 0, WAN 1), both directions."""
    return mixed_fw_trace(np.random.default_rng(seed), n, n_flows, n_dev=2, wan=1)


def _bridge_ipv4_trace(seed, n, n_stations, n_dsts):
    """mixed_bridge_trace's MACs and ports on 4 devices, carrying
    mixed_pol_trace's IPv4 packets (destination addresses, sizes up to 1400
    bytes in 64-byte slots, gaps that refill buckets and expire entries),
    with half of the frames to a station nobody has seen: floods."""
    rng = np.random.default_rng(seed)
    fb, _, dv, _ = mixed_bridge_trace(rng, n, n_stations, n_dev=4)
    fp, ln, _, now = mixed_pol_trace(rng, n, n_dsts, n_dev=2, gap_ns=1500)
    fb, fp = fb.reshape(n, SLOT).copy(), fp.reshape(n, SLOT)
    fb[:, 12:] = fp[:, 12:]
    unseen = rng.random(n) < 0.5
    fb[unseen, 0:4] = [0x02, 0xEE, 0, 0]
    return fb.reshape(-1), ln, dv, now


def _lb_heartbeats(n_backends):
    """Heartbeats that register viglb's backends before the chain runs: the
    chain's one link into viglb is its WAN port."""
    fr, ln, dv, now = T.lb_heartbeats(n_backends)
    return fr, ln, dv, now


def cases():
    n = 3000
    return {
        # LAN packets pass the firewall to its WAN port and on to the NAT's
        # LAN port; the firewall's accepted WAN replies leave the chain on its
        # port 0. The NAT's table is smaller than the flows in flight.
        "fw-nat": Case([fw_stage(256, 1), nat_stage(64, 1)], [(0, 1, 1, 0)],
                       lambda: _fw_trace(11, n, 400)),
        # what the bridge sends to its port 2 (floods from the other three,
        # and frames to stations learned there) is policed as WAN traffic
        "bridge-pol": Case([bridge_stage(256, 300), pol_stage(64, 10_000_000, 3000)],
                           [(0, 2, 1, 0)], lambda: _bridge_ipv4_trace(12, n, 300, 90)),
        "fw-nat-lb": Case([fw_stage(256, 1), nat_stage(128, 1), lb_stage(64, 16, 17, 1, 3)],
                          [(0, 1, 1, 0), (1, 1, 2, 2)], lambda: _fw_trace(13, n, 400),
                          prime={2: lambda: _lb_heartbeats(8)}),
    }


def chain_reference(oracles, links, frames, lens, in_dev, now, slot, snap=None, every=128):
    """Per stage (origin, out, frames, lens): the packets it received by
    their index in the input, its out ports, and the slots as it left them
    (u8, received x slot). links: (s, out_port, t, in_port), t > s, at most
    one inbound per stage. snap: called as snap(stage) -> state before the
    first packet and after every `every`-th; the snapshots are returned as a
    second value (per stage a list)."""
    k = len(oracles)
    route = {}
    for s, p, t, q in links:
        route.setdefault(s, []).append((p, t, q))
    got = [([], [], [], []) for _ in range(k)]
    shots = [[] for _ in range(k)]
    frames = np.asarray(frames, np.uint8).reshape(-1, slot)
    n = len(lens)

    def shoot():
        for s in range(k):
            shots[s].append(snap(s))

    def push(s, port, buf, length, t, i):
        out = oracles[s].process(port, buf, length=length, cap=slot, now=t)
        origin, outs, slots, ls = got[s]
        origin.append(i)
        outs.append(out)
        slots.append(bytes(buf))
        ls.append(length)
        if out == port:
            return  # dropped (nf.c:159)
        for p, t2, q in route.get(s, []):
            if out == p or (out == vigor_amd.FLOOD_FRAME and port != p):
                push(t2, q, bytearray(buf), length, t, i)  # a fresh slot

    if snap:
        shoot()
    for i in range(n):
        push(0, int(in_dev[i]), bytearray(frames[i].tobytes()), int(lens[i]), int(now[i]), i)
        if snap and (i + 1) % every == 0:
            shoot()
    if snap:
        shoot()
    res = []
    for origin, outs, slots, ls in got:
        res.append((np.array(origin, np.int64), np.array(outs, np.uint16),
                    np.frombuffer(b"".join(slots), np.uint8), np.array(ls, np.uint16)))
    return (res, shots) if snap else res


def expired_between(shots):
    """True where some index that was allocated in one snapshot is free, or
    holds another key, in the next: an entry left the table. shots: per
    snapshot a list of tables (alloc, ts, key, ...)."""
    for a, b in zip(shots[:-1], shots[1:]):
        for ta, tb in zip(a, b):
            was = ta[0] == 1
            ka, kb = np.asarray(ta[2]), np.asarray(tb[2])
            moved = (ka != kb).reshape(ka.shape[0], -1).any(axis=1)
            if (was & ((tb[0] == 0) | moved)).any():
                return True
    return False


def dropped_and_forwarded(origin, out, in_port_of):
    """(dropped, forwarded) packets of one stage: out == the port it came in
    on is a drop (nf.c:159)."""
    ins = np.array([in_port_of(i) for i in origin], np.uint16) if origin.size else \
        np.zeros(0, np.uint16)
    return int((out == ins).sum()), int((out != ins).sum())
