"""Independent Python reading of the KBRTestApp RPC test (kbrRpcTest) -- test infrastructure only.

A message-level replay of one routed KbrTestCall round trip: the call route, its delivery, the
KbrTestResponse and the ordering of the response against the timeout self-message; then the
statistics KBRTestApp hands to GlobalStatistics.  It never calls the engine.

  call      KBRTestApp.cc:172-189 -> BaseRpc::sendRpcCall (BaseRpc.cc:173-274, timeout rpcKeyTimeout
            202-205, scheduled at send time 257-258) -> BaseOverlay::route / sendToKey (BaseOverlay.cc:1310-1359)
  response  KBRTestApp.cc:230-235 -> BaseApp::internalSendRpcResponse (BaseApp.cc:572-611) ->
            BaseRpc::sendRpcResponse (BaseRpc.cc:531-596): direct UDP (iterative, semi-recursive;
            BaseOverlay.cc:1340-1341, hop count 1 at 751, a message to oneself: no delay, hop count 0) or a
            second full-recursive route to the caller's own key (BaseApp.cc:595-599)
  outcome   KBRTestApp.cc:237-329; finishApp 519-545

Per-hop routing decisions come from elsewhere: `chord_leg` walks refmodel.ChordRing.decide (a converged
ring) and times every message itself; `oracle_leg` takes whole routes from OracleNet.route (Kademlia,
Koorde, large rings).  The response delay, the timeout rule, the hop sum and all statistics are
computed here.
"""
from __future__ import annotations

import math

import numpy as np

import refmodel

NONE = 0xFFFFFFFF
ANSWERED, TIMEOUT = 0, 1
BASEAPPDATA_BYTES = 5      # BASEAPPDATA_L = BASEOVERLAY_L + 2 * COMP_L = 40 bits (CommonMessages.msg:68)
BASEROUTE_BYTES = 53       # BASEROUTE_L = 424 bits (CommonMessages.msg)
UDP_IP_BYTES = 28          # SimpleUDP.cc:291
MIN_MEASURED = 0.1         # GlobalStatistics.cc:32

RPC_DTYPE = np.dtype([("responder", "<u4"), ("hop_count", "<u2"), ("call_hops", "u1"), ("status", "u1"),
                      ("outcome", "u1"), ("resp_status", "u1"), ("pad", "u1", 6), ("rtt_ns", "<i8"),
                      ("call_latency_ns", "<i8")])
FIELDS = tuple(f for f in RPC_DTYPE.names if f != "pad")


def simtime(seconds: float, rnd: bool) -> int:
    """SimTime(double) at scale 1e-9: round half up, or truncate."""
    x = seconds * 1e9
    return math.floor(x + 0.5) if rnd else int(x)


def calc_delay(xy, a: int, b: int, nbytes: int, rnd: bool = True, datarate: float = 10e6, access: float = 0.0) -> int:
    """SimpleNodeEntry::calcDelay with idle queues (SimpleNodeEntry.cc:155-195), ns: the sender's and the
    receiver's serialisation and access delay plus 1 ms per coordinate unit (float distance); a
    message to the same host is delivered at once (SimpleUDP.cc:322)."""
    if a == b:
        return 0
    bw = simtime((nbytes * 8) / datarate, rnd)
    dx = float(xy[a][0]) - float(xy[b][0])
    dy = float(xy[a][1]) - float(xy[b][1])
    dist = float(np.float32(math.sqrt(dx * dx + dy * dy)))
    return 2 * bw + 2 * simtime(access, rnd) + simtime(0.001 * dist, rnd)


def route_bytes(test_msg_size: int) -> int:
    return BASEROUTE_BYTES + BASEAPPDATA_BYTES + test_msg_size + UDP_IP_BYTES


def response_bytes(test_msg_size: int) -> int:
    """The direct KbrTestResponse: setByteLength(call length) in a BaseAppDataMessage over UDP, no
    BaseRouteMessage, and no BASERESPONSE_L (so measureAuthBlock adds nothing)."""
    return test_msg_size + BASEAPPDATA_BYTES + UDP_IP_BYTES


# ---------------------------------------------------------------- call / return legs
def chord_leg(ring: "refmodel.ChordRing", routing_type: int, hop_max: int = 50, test_msg_size: int = 100,
              rpc_udp_timeout: float = 1.5, lookup_timeout: float = 10.0):
    """One-way route of a testMsgSize payload on a converged Chord ring, message by message: decisions
    from ChordRing.decide, times from calc_delay.  Iterative: FindNodeCall (83 B) / FindNodeResponse
    (87 B, one NodeHandle) from the source per hop, then the route message (IterativeLookup.cc:803-921,
    1067-1170; BaseOverlay.cc:1107-1146); recursive: the route message hop by hop (BaseOverlay.cc:869-1005)."""
    rnd, xy, rb = ring.rnd, ring.xy, route_bytes(test_msg_size)

    def fail(status, hops=0):
        return dict(responsible=NONE, hops=hops, status=status, one_way_hops=0, latency_ns=-1)

    def iterative(k, S):
        sib, nxt = ring.decide(S, k)
        if sib:
            return dict(responsible=S, hops=0, status=0, one_way_hops=0, latency_ns=0)
        t, hops, visited, cur = 0, 0, {S}, nxt
        to, lk = simtime(rpc_udp_timeout, rnd), simtime(lookup_timeout, rnd)
        while True:
            rtt = calc_delay(xy, S, cur, 83, rnd) + calc_delay(xy, cur, S, 87, rnd)
            if rtt >= to:
                return fail(1 if t + to > lk else 2, hops)
            t += rtt
            if t > lk:
                return fail(1, hops)
            hops += 1
            visited.add(cur)
            sib, nxt = ring.decide(cur, k)
            if sib:
                return dict(responsible=cur, hops=hops, status=0, one_way_hops=hops + (cur != S),
                            latency_ns=t + calc_delay(xy, S, cur, rb, rnd))
            if hop_max and hops >= hop_max:
                return fail(3, hops)
            if nxt in visited:
                return fail(4, hops)
            cur = nxt

    def recursive(k, S):
        cur, t, hops = S, 0, 0
        while True:
            sib, nxt = ring.decide(cur, k)
            if sib:
                return dict(responsible=cur, hops=hops, status=0, one_way_hops=hops, latency_ns=t)
            if hops >= hop_max:
                return fail(3)
            t += calc_delay(xy, cur, nxt, rb, rnd)
            hops += 1
            cur = nxt

    one = iterative if routing_type == 0 else recursive

    def leg(keys, src):
        rows = [one(refmodel.to_int(k), int(s)) for k, s in zip(keys, src)]
        return {f: np.array([r[f] for r in rows], dtype=np.int64) for f in
                ("responsible", "hops", "status", "one_way_hops", "latency_ns")}

    return leg


def oracle_leg(net):
    """Whole routes from the CPU oracle (tests/oracle_lib.OracleNet) with the network's own parameters."""
    def leg(keys, src):
        r = net.route(keys, src, record_hops=False)
        return {f: np.asarray(r[f]).astype(np.int64) for f in ("responsible", "hops", "status", "one_way_hops", "latency_ns")}
    return leg


# ---------------------------------------------------------------- one batch of RPCs
def rpc_batch(ids, xy, keys, src, leg, routing_type: int, rnd: bool = True, test_msg_size: int = 100,
              rpc_key_timeout: float = 10.0, datarate: float = 10e6, access: float = 0.0) -> np.ndarray:
    """Replay RPC i = KbrTestCall from src[i] to keys[i]; returns RPC_DTYPE records."""
    ids = np.asarray(ids)
    keys = np.asarray(keys)
    src = np.asarray(src).astype(np.int64)
    n = len(src)
    out = np.zeros(n, dtype=RPC_DTYPE)
    call = leg(keys, src.astype(np.uint32))
    limit = simtime(rpc_key_timeout, rnd)
    ret = None
    if routing_type == 2:
        # the response is routed to the caller's key from the responder; calls nobody answered send none
        idx = np.flatnonzero(call["status"] == 0)
        ret = {int(i): j for j, i in enumerate(idx)}
        rleg = leg(ids[src[idx]], call["responsible"][idx].astype(np.uint32)) if len(idx) else None
    rb = response_bytes(test_msg_size)
    for i in range(n):
        o = out[i]
        o["status"] = call["status"][i]
        o["outcome"], o["rtt_ns"], o["responder"], o["call_latency_ns"] = TIMEOUT, -1, NONE, -1
        if call["status"][i] != 0:
            continue                                   # the call was dropped on its way: handleRpcTimeout
        R, S = int(call["responsible"][i]), int(src[i])
        o["responder"], o["call_hops"], o["call_latency_ns"] = R, call["one_way_hops"][i], call["latency_ns"][i]
        if routing_type == 2:
            j = ret[i]
            o["resp_status"] = rleg["status"][j]
            if rleg["status"][j] != 0 or int(rleg["responsible"][j]) != S:
                continue                               # dropped, or delivered where no call is pending
            arrival = int(call["latency_ns"][i]) + int(rleg["latency_ns"][j])
            resp_hops = int(rleg["one_way_hops"][j])
        else:
            arrival = int(call["latency_ns"][i]) + calc_delay(xy, R, S, rb, rnd, datarate, access)
            resp_hops = 0 if R == S else 1             # BaseOverlay.cc:747-751
        # events at one instant run in scheduling order: the timeout was scheduled when the call was sent
        if arrival >= limit:
            continue
        o["outcome"], o["rtt_ns"] = ANSWERED, arrival
        o["hop_count"] = int(call["one_way_hops"][i]) + resp_hops      # KBRTestApp.cc:271-274
    return out


# ---------------------------------------------------------------- statistics
def cstddev(vals) -> dict:
    """cStdDev (OMNeT++ 4.x): count, mean, sample standard deviation, min, max."""
    n = len(vals)
    if n == 0:
        return {"count": 0, "mean": 0.0, "stddev": 0.0, "min": 0.0, "max": 0.0}
    s = math.fsum(vals)
    sq = math.fsum(v * v for v in vals)
    var = (sq - s * s / n) / (n - 1) if n > 1 else 0.0
    return {"count": n, "mean": s / n, "stddev": math.sqrt(max(var, 0.0)), "min": min(vals), "max": max(vals)}


SD_FIELDS = ("delivered_msgs_per_s", "delivered_bytes_per_s", "dropped_msgs_per_s", "dropped_bytes_per_s",
             "delivery_ratio")
INT_FIELDS = ("num_sent", "num_delivered", "num_dropped", "num_timeout", "bytes_sent", "bytes_delivered",
              "bytes_dropped", "hop_count_sum", "success_latency_sum_ns", "hop_count_min", "hop_count_max",
              "success_latency_min_ns", "success_latency_max_ns")


def rpc_stats(out, ids, keys, src, measured_time_s: float, lookup_node_ids: bool = True, failure_latency: float = 10.0,
              test_msg_size: int = 100) -> dict:
    """KBRTestApp::handleRpcResponse / handleRpcTimeout (KBRTestApp.cc:251-314) over the batch and finishApp
    (519-545) over the nodes.  A source that is no node (the engine's device-pointer calls do not check
    them) counts in the sums and in no node's counters, as in the oracle's one-way and lookup statistics."""
    ids, keys = np.asarray(ids), np.asarray(keys)
    nn, n = len(ids), len(out)
    sent, deliv, drop = ([0] * (nn + 1) for _ in range(3))
    hops, lats, timeouts = [], [], 0
    status, hist = [0] * 8, [0] * 64
    for i in range(n):
        o, s = out[i], int(src[i])
        status[int(o["status"]) & 7] += 1
        s = s if s < nn else nn                     # no node: the extra row
        sent[s] += 1
        ok = int(o["outcome"]) == ANSWERED
        timeouts += 0 if ok else 1
        if ok and lookup_node_ids:
            ok = bool(np.array_equal(ids[int(o["responder"])], keys[i]))
        if not ok:
            drop[s] += 1
            continue
        deliv[s] += 1
        hops.append(int(o["hop_count"]))
        lats.append(int(o["rtt_ns"]))
        hist[min(hops[-1], 63)] += 1
    nd, nr, B = len(hops), n - len(hops), test_msg_size
    st = dict(num_sent=n, num_delivered=nd, num_dropped=nr, num_timeout=timeouts, bytes_sent=n * B,
              bytes_delivered=nd * B, bytes_dropped=nr * B, hop_count_sum=sum(hops), success_latency_sum_ns=sum(lats),
              hop_count_min=min(hops, default=0), hop_count_max=max(hops, default=0),
              success_latency_min_ns=min(lats, default=0), success_latency_max_ns=max(lats, default=0),
              hop_count_mean=sum(hops) / nd if nd else 0.0,
              success_latency_mean_s=sum(lats) / nd * 1e-9 if nd else 0.0,
              total_latency_mean_s=(sum(lats) * 1e-9 + nr * failure_latency) / n if n else 0.0,
              status_count=status, hop_hist=hist)
    sent, deliv, drop = sent[:nn], deliv[:nn], drop[:nn]
    T = measured_time_s
    if T >= MIN_MEASURED:
        sd = [[d / T for d in deliv], [d * B / T for d in deliv], [r / T for r in drop], [r * B / T for r in drop],
              [float(np.float32(d) / np.float32(s)) for d, s in zip(deliv, sent) if s > 0]]
    else:
        sd = [[], [], [], [], []]
    for name, vals in zip(SD_FIELDS, sd):
        st[name] = cstddev(vals)
    return st
