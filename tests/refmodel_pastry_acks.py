"""Pastry routes with per-hop acks (routeMsgAcks = true, default.ini:245) and KBRTestApp's RPC test on them,
replayed event by event on top of refmodel_pastry: the checker of k_pastry_route<true> (oversim_amd/csrc/pastry.hip)
and of ovs_pastry_rpc_batch.

Test infrastructure only.  The routing decisions are refmodel_pastry.PastryNet.route's (findNode and the recursive
branch of sendToKey); this file replays the packets of the route it took, with a transmit queue per node:

  sendRouteMessage(dest, msg, ack = true)   BaseOverlay.cc:1107-1146: the route message travels inside a NextHopCall
                                            (1135-1144), sent with sendUdpRpcCall and routeRetries = 0
  nextHopRpc                                BaseOverlay.cc:1971-2000: the receiver sends the NextHopResponse (1997)
                                            and only then handles the decapsulated route message (1999), which
                                            forwards it -- or delivers it, and an RPC's responder answers -- in the
                                            same instant from the same node
  SimpleNodeEntry::calcDelay                SimpleNodeEntry.cc:164-194: tx.finished = max(tx.finished, now) +
                                            bits / bandwidth; the packet leaves when the queue has drained
  the ack's timeout                         BaseRpc.cc:191-211: rpcUdpTimeout from sendUdpRpcCall; the timeout
                                            event was scheduled first, so a response at the same instant is late
  KbrTestResponse                           BaseOverlay.cc:1340-1341: straight back over UDP (refmodel_rpc)

Lengths (CommonMessages.msg): NEXTHOPCALL_L = BASECALL_L (88) = BASERPC_L (71, 69-70) = TYPE_L 8 (30, 59) + NONCE_L
32 (34) + NODEHANDLE_L 208 (52: IPADDR_L 32 + UDPPORT_L 16 + KEY_L 160) + TIER_L 8 (42) = 256 bits = 32 B around the
encapsulated route message; NEXTHOPRESPONSE_L = BASERESPONSE_L (89, 73-76) = BASERPC_L + AUTHBLOCK_L (57: 800 bits
under measureAuthBlock) + no NCS info (ncsType "none") = 32 B or 132 B.  Each packet carries the 28 B UDP/IP header
(SimpleUDP.cc:291), which refmodel_rpc.route_bytes already counts for the route message.

Every lookup starts with all queues idle: the batch rule of DESIGN.md.
"""
from __future__ import annotations

import heapq

import numpy as np

import refmodel_pastry as RP
import refmodel_pastry_iter as RI
import refmodel_rpc as RR
from refmodel import coord_ns, simtime

NONE = RP.NONE
OK = RP.OK
NO_TIMEOUT_HOP = 0xFF
BASERPC_BITS = 8 + 32 + 208 + 8                                 # BASERPC_L (CommonMessages.msg:69-70)
AUTHBLOCK_BITS = 800                                            # SIGNATURE_L + CERT_L + PUBKEY_L (45-47, 57)
UDP_IP_BYTES = 28


def call_bytes(route_bytes: int) -> int:
    """A NextHopCall around a route message of route_bytes (which count the UDP/IP header once)."""
    return BASERPC_BITS // 8 + route_bytes


def ack_bytes(auth: bool = False) -> int:
    """A NextHopResponse on the wire."""
    return (BASERPC_BITS + (AUTHBLOCK_BITS if auth else 0)) // 8 + UDP_IP_BYTES


class Underlay:
    """SimpleUnderlay's delay with a transmit queue per node (SimpleNodeEntry.cc:164-194); times in ns."""

    def __init__(self, xy, rnd=True, datarate=10e6, access=0.0):
        self.xy, self.rnd, self.datarate = xy, rnd, datarate
        self.access = simtime(access, rnd)
        self.tx_finished = {}

    def bw(self, nbytes: int) -> int:
        return simtime((nbytes * 8) / self.datarate, self.rnd)          # simtime_t = double

    def send(self, a: int, b: int, nbytes: int, now: int) -> int:
        """calcDelay for a packet a -> b handed to UDP at `now`: its arrival time."""
        assert a != b
        fin = max(self.tx_finished.get(a, 0), now) + self.bw(nbytes)
        self.tx_finished[a] = fin
        return fin + self.access + coord_ns(self.xy, a, b, self.rnd) + self.bw(nbytes) + self.access


def replay(net, path, acks=True, route_bytes=186, auth=False, rpc_to=1.5, response_bytes=None, datarate=10e6, access=0.0):
    """The packets of one route message that visits path[0] (the source), path[1], ... in event order, all queues
    idle at 0.  response_bytes: the last node of the path answers a KbrTestCall with a message of that length to
    path[0].  -> dict(arrival: when path[-1] got the message, ack_rtt: one round trip per hop in hop order,
    forwards: NextHopCalls sent by a node that had just received one, response_arrival or None)."""
    u = Underlay(net.xy, net.rnd, datarate, access)
    nb = call_bytes(route_bytes) if acks else route_bytes
    ev, seq = [], 0

    def post(t, kind, i):
        nonlocal seq
        heapq.heappush(ev, (t, seq, kind, i))
        seq += 1

    sent = {}                     # hop index -> when its sender called sendUdpRpcCall
    rtt = {}
    arrival = {0: 0}
    forwards = 0
    resp = None
    post(0, "msg", 0)
    while ev:
        t, _, kind, i = heapq.heappop(ev)
        if kind == "ack":
            rtt[i] = t - sent[i]
        elif kind == "resp":
            resp = t
        else:
            arrival[i] = t
            if i > 0 and acks:
                post(u.send(path[i], path[i - 1], ack_bytes(auth), t), "ack", i - 1)        # nextHopRpc: 1997
            if i + 1 < len(path):
                sent[i] = t
                forwards += 1 if (i > 0 and acks) else 0
                post(u.send(path[i], path[i + 1], nb, t), "msg", i + 1)                     # 1999 -> sendRouteMessage
            elif response_bytes is not None:
                if path[i] == path[0]:
                    resp = t                                                                # SimpleUDP.cc:322
                else:
                    post(u.send(path[i], path[0], response_bytes, t), "resp", 0)
    rtts = [rtt[i] for i in range(len(path) - 1)] if acks else []
    limit = simtime(rpc_to, net.rnd)
    late = [i for i, r in enumerate(rtts) if r >= limit]
    return dict(arrival=arrival[len(path) - 1], ack_rtt=rtts, forwards=forwards, response_arrival=resp,
                timeout_hop=late[0] if late else NO_TIMEOUT_HOP)


def route(net, kw, S, acks=True, rec_num_redundant=3, hop_max=50, route_bytes=186, auth=False, rpc_to=1.5, response_bytes=None):
    """One semi-recursive route message under routeMsgAcks = acks: refmodel_pastry's record with the replayed
    latency, the ack record (acks, max_ack_rtt_ns, timeout_hop, ack_rtt, forwards) and response_arrival.  A route
    that fails part-way has sent the NextHopCalls of the hops it took, and they were acknowledged."""
    r = net.route(kw, S, rec_num_redundant, hop_max, route_bytes)
    path = [S] + list(r["hop_seq"])
    ok = r["status"] == OK
    p = replay(net, path, acks, route_bytes, auth, rpc_to, response_bytes if ok else None)
    out = dict(r)
    out["latency_ns"] = p["arrival"] if ok else -1
    out["acks"] = len(p["ack_rtt"])
    out["max_ack_rtt_ns"] = max(p["ack_rtt"], default=-1)
    out["timeout_hop"] = p["timeout_hop"]
    out["ack_rtt"] = p["ack_rtt"]
    out["forwards"] = p["forwards"]
    out["response_arrival"] = p["response_arrival"]
    return out


def _arrays(res, H):
    out = dict(responsible=np.array([r["responsible"] for r in res], dtype=np.uint32),
               hops=np.array([r["hops"] for r in res], dtype=np.uint16),
               status=np.array([r["status"] for r in res], dtype=np.uint8),
               one_way_hops=np.array([r["one_way_hops"] for r in res], dtype=np.uint8),
               latency_ns=np.array([r["latency_ns"] for r in res], dtype=np.int64),
               acks=np.array([r["acks"] for r in res], dtype=np.uint16),
               max_ack_rtt_ns=np.array([r["max_ack_rtt_ns"] for r in res], dtype=np.int64),
               timeout_hop=np.array([r["timeout_hop"] for r in res], dtype=np.uint8),
               hop_seq=np.full((len(res), H), NONE, dtype=np.uint32))
    for i, r in enumerate(res):
        out["hop_seq"][i, :len(r["hop_seq"])] = r["hop_seq"]
    return out


def routes(net, keys, src, **kw):
    """Model routes as arrays, hop_seq padded with NONE to max(hop_max, 1) columns."""
    return _arrays([route(net, k, int(s), **kw) for k, s in zip(keys, src)], max(kw.get("hop_max", 50), 1))


def iterative_route(net, kw, S, acks=True, hop_max=50, rpc_to=1.5, lk_to=10.0, auth=False, route_bytes=186):
    """The one-way message under iterative routing: refmodel_pastry_iter's lookup, then sendRouteMessage to
    getResult()[0] with ack = routeMsgAcks (BaseOverlay.cc:1254-1257): one NextHopCall from the source, whose queue
    the lookup's last FindNodeCall left long ago, and one ack."""
    r = RI.lookup(net, kw, S, 1, hop_max, rpc_to, lk_to, auth)
    out = dict(responsible=NONE, hops=r["hops"], status=r["status"], one_way_hops=0, latency_ns=-1, hop_seq=r["hop_seq"],
               acks=0, max_ack_rtt_ns=-1, timeout_hop=NO_TIMEOUT_HOP)
    if r["status"] != OK:
        return out
    R = r["siblings"][0]
    p = replay(net, [S, R] if R != S else [S], acks, route_bytes, auth, rpc_to)
    out.update(responsible=R, one_way_hops=r["hops"] + int(R != S), latency_ns=r["latency_ns"] + p["arrival"],
               acks=len(p["ack_rtt"]), max_ack_rtt_ns=max(p["ack_rtt"], default=-1), timeout_hop=p["timeout_hop"])
    return out


def iterative_routes(net, keys, src, **kw):
    return _arrays([iterative_route(net, k, int(s), **kw) for k, s in zip(keys, src)], kw.get("hop_max", 50))


def rpc_batch(net, keys, src, acks=True, rpc_key_timeout=10.0, test_msg_size=100, **kw) -> np.ndarray:
    """KbrTestCalls src[i] -> keys[i] (KBRTestApp.cc:172-189, 230-329) as refmodel_rpc.RPC_DTYPE records: the call leg is
    route() above; the responder sends the KbrTestResponse behind its ack, straight to the caller."""
    out = np.zeros(len(src), dtype=RR.RPC_DTYPE)
    limit = simtime(rpc_key_timeout, net.rnd)
    for i, (k, s) in enumerate(zip(keys, src)):
        r = route(net, k, int(s), acks, route_bytes=RR.route_bytes(test_msg_size),
                  response_bytes=RR.response_bytes(test_msg_size), **kw)
        o = out[i]
        o["status"] = r["status"]
        o["outcome"], o["rtt_ns"], o["responder"], o["call_latency_ns"] = RR.TIMEOUT, -1, NONE, -1
        if r["status"] != OK:
            continue
        o["responder"], o["call_hops"], o["call_latency_ns"] = r["responsible"], r["one_way_hops"], r["latency_ns"]
        if r["response_arrival"] >= limit:                     # the timeout was scheduled when the call was sent
            continue
        o["outcome"], o["rtt_ns"] = RR.ANSWERED, r["response_arrival"]
        o["hop_count"] = r["one_way_hops"] + int(r["responsible"] != int(s))
    return out
