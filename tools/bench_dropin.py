#!/usr/bin/env python3
"""The drop-in boundary, timed for one NF: host/nf_loop_<nf> (nf.c's loop
restated over a trace file, linked against lib<nf>_nf.so) the way bench.py's
per_packet_drop_in times vignat -- `--flows` flows opened by an untimed
warm-up, then `--packets` steady LAN hits round robin, each with its own time
stamp; every packet through nf_process one at a time (batch 0, nf.c:150-176)
and through vp_process_batch in bursts (nf.c:178-215).

  tools/bench_dropin.py --nf fw                      # batch 0 / 32 / 1024
  tools/bench_dropin.py --nf fw --sweep 32,64,128    # burst routing limit
  tools/bench_dropin.py --nf bridge                  # vigbridge: 1,024 stations
  tools/bench_dropin.py --nf pol                     # vigpol: 1,024 policed addresses
  tools/bench_dropin.py --nf lb                      # viglb: 256 backends, 1,024 flows
  tools/bench_dropin.py --nf nat --churn --batches 0,32   # flows expiring all along

--churn (every NF; viglb's trace is below): every 16th timed packet opens a
never-seen flow and the others hit the `--flows` most recent flows round
robin, so the oldest flow goes idle each time; the clock advances 1 us a
packet and `--expire` is four round-robin turns (4 x flows us), so in steady
state about one flow expires every 16 packets while no flow that is still hit
does. The table holds 2 x flows. A vigbridge flow is a src MAC (every frame is
addressed to a MAC that is never learnt and floods); a vigpol flow is a
policed address, and the lifetime burst * 1e9 / rate is set by --rate
1000000000 --burst 4000 x flows (4,096,000 for 1,024 flows: 4.096 ms, and no
bucket of 64-byte packets runs dry). VIGPATH_SERVE_EXPIRE=0 in the environment
gives the path that hands every due expiry to the batch pipeline.

--churn --nf lb: the warm-up announces 16 backends ahead of the flows; flows
churn as above; every 16th timed packet at offset 8 is a heartbeat, round robin
over the backends except one in turn, which stays silent for 5 x flows packets
-- longer than the backend lifetime -- so a backend expires, its flows are
re-pointed, and it comes back, again and again in the run. Both lifetimes are
4 x flows us. The tool prints the CPU oracle's expiry counts per table for the
trace first.

--sweep N,...: each burst size twice in this run, VIGPATH_SERVE_BURST forcing
the resident kernel (a limit above every N) and the batch pipeline (0): the
routing limit (kServeBurstRoute / kFwBurstRoute / kBridgeBurstRoute /
kPolBurstRoute / kLbBurstRoute) is the
largest N at which the served path is the faster one per packet.

--tree DIR: another build of the library (a checkout of another commit with
its own host/ and vigor_amd/), for A/B on one machine in one session.

Prints one JSON line per measurement; --out appends them to a file.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vigor_amd import traces as T  # noqa: E402

SLOT = 64


def wan_port(n, flows):
    """vignat, vigfw: every steady packet is a LAN hit and goes out on the WAN
    port."""
    return np.ones(n, np.uint16)


def bridge_port(n, flows):
    """T.bridge_trace: frame p goes to station dst_k = (p + flows / 2) mod
    flows, learned by the warm-up on port dst_k & 1."""
    p = np.arange(n, dtype=np.int64)
    return (((p + flows // 2) % flows) & 1).astype(np.uint16)


def lan_port(n, flows):
    """vigpol: every steady packet arrives on the WAN device, finds its
    address's bucket full enough and goes out on the LAN device."""
    return np.ones(n, np.uint16)


def churn_trace(n, flows, nf="nat"):
    """--churn: `flows` flows opened by the warm-up, then packet p of the
    timed part opens flow flows + p / 16 when p is a multiple of 16 and else
    hits one of the `flows` newest flows, round robin; 1 us a packet. Flow k
    is a LAN 5-tuple (vignat, vigfw), the src MAC 02:00:00:kk:kk:kk of a frame
    to ff:00:00:00:00:01 on port 0 (vigbridge), or the policed address
    10.0.0.0 + k of a WAN packet (vigpol)."""
    p = np.arange(n - flows, dtype=np.int64)
    newest = flows - 1 + (p // 16 + 1)  # (the newest flow once packet p has been seen)
    hit = newest - flows + 1 + (p - p // 16) % flows
    fl = np.concatenate([np.arange(flows, dtype=np.int64), np.where(p % 16 == 0, newest, hit)])
    z = np.zeros_like(fl)
    if nf == "pol":
        frames, lens = T.udp_frames(np.full_like(fl, T.ip4(192, 168, 0, 1)),
                                    T.ip4(10, 0, 0, 0) + fl, z + 53, z + 80, slot=SLOT)
    else:
        frames, lens = T.udp_frames(T.ip4(10, 0, 0, 0) + (fl >> 16), z, fl & 0xFFFF, z, slot=SLOT)
    if nf == "bridge":
        f = frames.reshape(n, SLOT)
        f[:, 0:6] = np.array([0xFF, 0, 0, 0, 0, 1], np.uint8)
        f[:, 6:9] = np.array([0x02, 0, 0], np.uint8)
        f[:, 9] = (fl >> 16) & 0xFF
        f[:, 10] = (fl >> 8) & 0xFF
        f[:, 11] = fl & 0xFF
    now = T.NOW0 + 1000 * np.arange(n, dtype=np.int64)
    return frames, lens, np.zeros(n, np.uint16), now


def churn_port(nf, n):
    """--churn: every packet's out port -- the WAN port (vignat, vigfw), a
    flood (vigbridge), the LAN port (vigpol)."""
    return np.full(n, 0xFFFF if nf == "bridge" else 1, np.uint16)


LB_BACKENDS = 256
LB_CHURN_BACKENDS = 16


def lb_churn_trace(n, flows):
    """--churn --nf lb: LB_CHURN_BACKENDS heartbeats and `flows` WAN flows for
    the warm-up, then n - flows timed packets, 1 us each: packet p opens flow
    flows + p / 16 when p is a multiple of 16, is a heartbeat when p mod 16 is
    8 -- of backend (p / 16) mod 16, or of the next one while that one is the
    silent backend (p / (5 flows)) mod 16 --, and else hits one of the `flows`
    newest flows, round robin."""
    nb = LB_CHURN_BACKENDS
    p = np.arange(n - flows, dtype=np.int64)
    newest = flows - 1 + (p // 16 + 1)
    hit = newest - flows + 1 + (p - p // 16 - (p + 8) // 16) % flows
    fl = np.concatenate([np.arange(flows, dtype=np.int64), np.where(p % 16 == 0, newest, hit)])
    z = np.zeros_like(fl)
    frames, lens = T.udp_frames(T.ip4(11, 0, 0, 0) + fl, z, z, z, slot=SLOT)
    dv = np.full(n, 2, np.uint16)
    silent = (p // (5 * flows)) % nb
    b = (p // 16) % nb
    b = np.where(b == silent, (b + 1) % nb, b)
    hb = np.nonzero(p % 16 == 8)[0]
    hf, _, hd, _ = T.lb_heartbeats(nb)
    f = frames.reshape(n, SLOT)
    f[flows + hb] = hf.reshape(nb, SLOT)[b[hb]]
    dv[flows + hb] = hd[b[hb]]
    w = T.lb_heartbeats(nb)
    frames = np.concatenate([w[0], f.reshape(-1)])
    lens = np.concatenate([w[1], lens])
    dv = np.concatenate([w[2], dv])
    now = T.NOW0 + 1000 * np.arange(nb + n, dtype=np.int64)
    return frames, lens, dv, now


def lb_churn_oracle(frames, lens, dv, now, flows):
    """The CPU oracle's expiry counts per table over that trace: the entries
    allocated before a packet and stamped below its time less the lifetime."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import orc
    fcap, bcap, e_ns = 2 * flows, LB_CHURN_BACKENDS, 4 * flows * 1000
    cfg = orc.LbCfg(flow_capacity=fcap, flow_expiration_time=4 * flows, backend_capacity=bcap,
                    cht_height=17, backend_expiration_time=4 * flows, wan_device=2, n_devices=3)
    o = orc.Oracle("lb", cfg)
    F = frames.reshape(-1, SLOT).copy()
    nf = nb = 0
    for i in range(F.shape[0]):
        (fa, ft, _, _), (ba, bt, _, _, _) = o.lb_dump(fcap, bcap)
        nf += int(((fa == 1) & (ft < int(now[i]) - e_ns)).sum())
        nb += int(((ba == 1) & (bt < int(now[i]) - e_ns)).sum())
        o.run(F[i], lens[i:i + 1], dv[i:i + 1], now[i:i + 1], SLOT)
    return {"flows_expired": nf, "backends_expired": nb}


def lb_trace(n, flows):
    """viglb: LB_BACKENDS heartbeats announce the backends first, then WAN
    traffic over `flows` flows round robin (n packets of it); nothing expires
    in the run."""
    hb = T.lb_heartbeats(LB_BACKENDS)
    tr = T.lb_traffic(n, flows)
    return tuple(np.concatenate(x) for x in zip(hb, tr))


def lb_port(n, flows):
    """viglb: every steady packet hits its flow and leaves on its backend's
    device, 0 or 1 (which of the two is the CHT's choice): never on the WAN
    device, 2."""
    return None


# per NF: its loop binary, trace, arguments, the option that sizes its table to
# `--flows`, and the out port expected of every steady packet
NF = {
    "nat": dict(loop="nf_loop", trace=T.nat_lan_trace, size="--max-flows", steady=wan_port,
                args=["--expire", "60000000", "--starting-port", "0", "--wan", "1",
                      "--extip", "192.168.4.2", "--eth-dest", "0,90:e2:ba:55:12:20",
                      "--eth-dest", "1,90:e2:ba:55:12:21"]),
    "fw": dict(loop="nf_loop_fw", trace=T.fw_trace, size="--max-flows", steady=wan_port,
               args=["--expire", "60000000", "--wan", "1",
                     "--eth-dest", "0,90:e2:ba:55:12:20",
                     "--eth-dest", "1,90:e2:ba:55:12:21"]),
    "bridge": dict(loop="nf_loop_bridge", trace=T.bridge_trace, size="--capacity",
                   steady=bridge_port, args=["--expire", "60000000"]),
    # 1 B/ns into buckets of 100 MB: entries live 0.1 s of trace time (the
    # trace advances 1 ns a packet, so no expiry is due in a run of up to 1e8
    # packets) and no bucket of 60-byte packets runs dry
    "pol": dict(loop="nf_loop_pol", trace=T.pol_trace, size="--capacity", steady=lan_port,
                args=["--lan", "1", "--wan", "0", "--rate", "1000000000",
                      "--burst", "100000000"]),
    # `warm`: packets ahead of the flows that the warm-up takes too
    "lb": dict(loop="nf_loop_lb", trace=lb_trace, size="--flow-capacity", steady=lb_port,
               warm=LB_BACKENDS, env={"VIGPATH_NB_DEVICES": "3"},  # (WAN = device 2)
               args=["--backend-capacity", str(LB_BACKENDS), "--cht-height", "257",
                     "--flow-expiration", "60000000", "--backend-expiration", "60000000",
                     "--wan", "2"]),
}


def run_loop(tree, nf, tin, tout, flows, batch, env, churn=False):
    """One nf_loop run: us per timed packet (its out ports are left in tout)."""
    cmd = [os.path.join(tree, "host", NF[nf]["loop"]), tin, tout]
    if batch:
        cmd += ["--batch", str(batch)]
    args, size = list(NF[nf]["args"]), flows
    warm = NF[nf].get("warm", 0)
    if churn:  # four round-robin turns of 1 us packets; room for the idle flows
        if nf == "pol":  # (1 B/ns: burst bytes last burst ns)
            args[args.index("--burst") + 1] = str(4000 * flows)
        elif nf == "lb":
            warm = LB_CHURN_BACKENDS
            for k, v in [("--backend-capacity", LB_CHURN_BACKENDS), ("--cht-height", 17),
                         ("--flow-expiration", 4 * flows), ("--backend-expiration", 4 * flows)]:
                args[args.index(k) + 1] = str(v)
        else:
            args[args.index("--expire") + 1] = str(4 * flows)
        size = 2 * flows
    cmd[3:3] = ["--warm", str(flows + warm)]
    cmd += ["--"] + args + [NF[nf]["size"], str(size)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **NF[nf].get("env", {}), **env))
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d): %s" % (cmd[0], r.returncode, r.stderr[-500:]))
    line = [x for x in r.stderr.splitlines() if x.startswith("timed ")][-1]
    return float(line.split(",")[1].split()[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nf", choices=sorted(NF), default="fw")
    ap.add_argument("--packets", type=int, default=20000)
    ap.add_argument("--flows", type=int, default=1024)
    ap.add_argument("--batches", default="0,32,1024")
    ap.add_argument("--sweep", default="", help="burst sizes, each served and through the pipeline")
    ap.add_argument("--repeat", type=int, default=3, help="runs per point (all reported)")
    ap.add_argument("--churn", action="store_true",
                    help="a flow expires about every 16 packets (vigpol: --rate 1000000000 "
                         "--burst 4000 x flows; viglb: a backend falls silent in turn as well)")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = a.flows + a.packets
    if a.churn and a.nf == "lb":
        fr, ln, dv, now = lb_churn_trace(n, a.flows)
        steady = None  # (a backend's device, or a heartbeat's own: 0 or 1, never the WAN's)
        print(json.dumps(dict(lb_churn_oracle(fr, ln, dv, now, a.flows), nf="lb",
                              packets=a.packets, flows=a.flows)), flush=True)
    elif a.churn:
        fr, ln, dv, now = churn_trace(n, a.flows, a.nf)
        steady = churn_port(a.nf, n)
    else:
        fr, ln, dv, now = NF[a.nf]["trace"](n, a.flows)
        steady = NF[a.nf]["steady"](n, a.flows)
    n, warm = len(ln), len(ln) - a.packets  # (viglb: the heartbeats ahead of the flows)
    points = []
    if a.sweep:
        for bt in [int(x) for x in a.sweep.split(",")]:
            points.append((bt, "served", {"VIGPATH_SERVE_BURST": "1000000"}))
            points.append((bt, "pipeline", {"VIGPATH_SERVE_BURST": "0"}))
    else:
        points = [(int(x), "default", {}) for x in a.batches.split(",")]
    with tempfile.TemporaryDirectory() as d:
        tin, tout = os.path.join(d, "t.in"), os.path.join(d, "t.out")
        with open(tin, "wb") as f:
            f.write(b"VPTR" + np.array([n, SLOT], np.uint32).tobytes())
            f.write(dv.astype(np.uint16).tobytes() + ln.astype(np.uint16).tobytes())
            f.write(now.astype(np.int64).tobytes() + fr.tobytes())
        for bt, path, env in points:
            us = []
            for _ in range(a.repeat):
                us.append(run_loop(a.tree, a.nf, tin, tout, a.flows, bt, env, a.churn))
                out = np.frombuffer(open(tout, "rb").read(), np.uint16, n, 12)
                # every steady packet out where expected
                assert (out[warm:] < 2).all() if steady is None else \
                    (out[warm:] == steady[a.flows:]).all()
            rec = {"nf": a.nf, "label": a.label, "batch": bt, "path": path, "churn": a.churn,
                   "packets": a.packets, "flows": a.flows,
                   "us_per_packet": [round(x, 3) for x in us],
                   "us_per_packet_min": round(min(us), 3)}
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
