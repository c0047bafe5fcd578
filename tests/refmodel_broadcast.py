"""Event-ordered replay of the reference's Chord overlay broadcast, in pure Python.

Test infrastructure only: the independent checker of ovs_chord_broadcast_batch.  It restates

  BroadcastTestApp::initBroadcast / rpcBroadcastRequest   BroadcastTestApp.cc:197-340
  Chord::forwardBroadcast                                  Chord.cc:1410-1445
  SimpleNodeEntry::calcDelay with the transmit queue       SimpleNodeEntry.cc:155-195

as a discrete-event simulation: a heap keyed by (time, sequence), one `receivedFrom` slot and one
`tx_finished` per node, the full 160-position getFinger table plus successor 0 per node.  It knows
nothing of levels: messages are handled in time order, the duplicate branch is kept and counted, so
"every node is reached once" is measured here, not assumed.  The tables come from the oracle
(oracle_lib.OracleNet), the coordinate delay from OracleNet.delay_ns, the queue arithmetic is
restated here in integer ns.
"""
from __future__ import annotations

import heapq
import math

import numpy as np

from refmodel import between, simtime, to_int

NONE = 0xFFFFFFFF
NODE_DTYPE = np.dtype([("arrival_ns", "<i8"), ("parent", "<u4"), ("hops", "<u2"), ("rank", "<u2")])

# CommonMessages.msg:30-52, 59, 68-73, 90-91 (bits)
BASEAPPDATA_L = 8 + 2 * 16
BASERPC_L = 8 + 32 + (32 + 16 + 160) + 8
NODEHANDLE_L = 32 + 16 + 160
AUTHBLOCK_L = 40 * 8 + 40 * 8 + 20 * 8
UDP_IP_BYTES = 28                       # SimpleUDP.cc:291, as the engine's other messages


def request_bits(query_bytes: int) -> int:
    """BROADCASTREQUESTCALL_L: the query's size in bytes is added as bits, as the macro stands."""
    return BASERPC_L + query_bytes + NODEHANDLE_L + 8 + 8


def response_bits(auth: bool) -> int:
    """BROADCASTREQUESTRESPONSE_L = BASERESPONSE_L + REQUESTID_L + 1."""
    return BASERPC_L + (AUTHBLOCK_L if auth else 0) + 8 + 1


def byte_length(bits: int) -> int:
    return (bits + 7) >> 3              # cPacket::getByteLength


class BroadcastReplay:
    def __init__(self, ids, xy, simtimeRound: int = 1, datarate: float = 10e6, accessDelay: float = 0.0,
                 measureAuthBlock: bool = False):
        self.ids = np.ascontiguousarray(ids, dtype=np.uint32)
        self.n = n = len(self.ids)
        self.keys = [to_int(w) for w in self.ids]
        self.rnd = bool(simtimeRound)
        self.datarate = datarate
        self.acc = simtime(accessDelay, self.rnd)
        self.auth = bool(measureAuthBlock)
        if n == 1:
            # the oracle builds rings of two nodes and more.  A lone node's successor list holds the
            # node itself (ChordSuccessorList.cc:72-78) and every getFinger falls back to it
            self.net = None
            self.fingers = [[0] * 160]
            self.succ0 = [0]
        else:
            from oracle_lib import OracleNet, chord_params
            self.net = OracleNet("chord", self.ids, xy, chord_params(simtimeRound=int(simtimeRound), datarate=datarate,
                                                                      accessDelay=accessDelay))
            self.fingers = self.net.chord_fingers().tolist()
            self.succ0 = self.net.chord_lists()[1][:, 0].tolist()

    def coord_ns(self, a: int, b: int) -> int:
        # calcDelay of an empty packet on idle queues = 2 * accessDelay + coordDelay
        return self.net.delay_ns(a, b, 0) - 2 * self.acc

    def forward_broadcast(self, v: int, limit: int) -> list[tuple[int, int]]:
        """Chord::forwardBroadcast at node v for a call whose BroadcastInfo limit is `limit` (the
        initiator passes its own key).  Returns (node, limit) per request in list order.  The
        `finger == lastFinger` test compares addresses; two equal addresses hold one node, which the
        interval test turns away the second time with or without it, so it is left out."""
        keys = self.keys
        vk = keys[v]
        row = self.fingers[v]
        requests = []
        for i in range(159, -2, -1):
            f = self.succ0[v] if i < 0 else row[i]
            fk = keys[f]
            if between(fk, vk, limit):
                requests.append((f, limit))
                limit = fk
        return requests

    def run(self, initiator: int, ttl: int, query_bytes: int = 0):
        """One broadcast.  Returns (records, stats, receptions): NODE_DTYPE records of the first
        reception of each node, the statistics (with `duplicated`) and how often each node received."""
        n, rnd = self.n, self.rnd
        call_len = byte_length(request_bits(query_bytes))
        resp_len = byte_length(response_bits(self.auth))
        call_bw = simtime((byte_length(BASEAPPDATA_L + request_bits(query_bytes)) + UDP_IP_BYTES) * 8 / self.datarate, rnd)
        resp_bw = simtime((resp_len + UDP_IP_BYTES) * 8 / self.datarate, rnd)
        rec = np.zeros(n, dtype=NODE_DTYPE)
        rec["arrival_ns"] = -1
        rec["parent"] = NONE
        receptions = np.zeros(n, dtype=np.int64)
        received_from = [None] * n
        tx_finished = [0] * n
        st = dict(expected=n, actual=0, expired=0, duplicated=0, messages=0, bytes=0, last_arrival_ns=0)
        hops_seen = []
        seq = 0
        # initBroadcast: an internal RPC to the node's own tier 2, now, with the full TTL and no BroadcastInfo
        heap = [(0, seq, initiator, self.keys[initiator], ttl, NONE, 0)]
        while heap:
            t, _, v, limit, tau, parent, rank = heapq.heappop(heap)
            receptions[v] += 1
            if received_from[v] is not None:                       # 233-244
                st["duplicated"] += 1
                st["messages"] += 1
                st["bytes"] += resp_len
                continue
            if rec["arrival_ns"][v] < 0:
                rec[v] = (t, parent, ttl - tau, rank)
            st["last_arrival_ns"] = max(st["last_arrival_ns"], t)
            hops_seen.append(ttl - tau)                            # 259-260
            if tau <= 0:                                           # 290-299: no setBitLength, receivedFrom stays
                st["expired"] += 1
                st["messages"] += 1
                continue
            tau -= 1
            st["actual"] += 1
            for j, (f, lim) in enumerate(self.forward_broadcast(v, limit)):      # 305-327
                st["messages"] += 1
                st["bytes"] += call_len
                # sendRouteRpcCall to a node: UDP, SimpleNodeEntry::calcDelay at the sender
                new_tx = max(tx_finished[v], t) + call_bw
                tx_finished[v] = new_tx
                delay = new_tx - t + self.acc + self.coord_ns(v, f) + call_bw + self.acc
                seq += 1
                heapq.heappush(heap, (t + delay, seq, f, lim, tau, v, j))
            received_from[v] = parent if parent != NONE else v     # 331
            st["messages"] += 1                                    # 333-339
            st["bytes"] += resp_len
            if parent != NONE:                                     # the response leaves through the queue too
                tx_finished[v] = max(tx_finished[v], t) + resp_bw
        cnt = len(hops_seen)
        s, sq = sum(hops_seen), sum(h * h for h in hops_seen)
        var = (float(sq) - float(s) * float(s) / float(cnt)) / float(cnt - 1) if cnt > 1 else 0.0
        st["hop_count"] = dict(count=cnt, mean=float(s) / float(cnt), stddev=math.sqrt(max(var, 0.0)),
                               min=float(min(hops_seen)), max=float(max(hops_seen)))
        return rec, st, receptions

    def run_batch(self, initiators, ttl: int, query_bytes: int = 0):
        recs, stats, rx = zip(*(self.run(int(i), ttl, query_bytes) for i in initiators))
        return np.stack(recs), list(stats), np.stack(rx)


STAT_FIELDS = ("expected", "actual", "expired", "messages", "bytes", "last_arrival_ns")


def stats_equal(engine_stats: dict, ref: dict) -> list[str]:
    """Names of the statistics that differ (bit-exact, the cStdDev doubles included)."""
    bad = [f for f in STAT_FIELDS if int(engine_stats[f]) != int(ref[f])]
    bad += ["hop_count." + f for f in ("count", "mean", "stddev", "min", "max")
            if engine_stats["hop_count"][f] != ref["hop_count"][f]]
    return bad
