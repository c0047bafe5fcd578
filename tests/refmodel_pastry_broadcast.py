"""Event-ordered replay of the reference's Pastry overlay broadcast, in pure Python.

Test infrastructure only: the independent checker of ovs_pastry_broadcast_batch.  It restates

  BroadcastTestApp::initBroadcast / rpcBroadcastRequest   BroadcastTestApp.cc:197-340
  Pastry::forwardAndForget / forwardBroadcast              Pastry.cc:1307-1390
  SimpleNodeEntry::calcDelay with the transmit queue       SimpleNodeEntry.cc:155-195

as a discrete-event simulation over the tables of tests/refmodel_pastry.py (the rule's, or explicit ones): a
heap keyed by (time, sequence), one `receivedFrom` slot, one `started` flag and one `tx_finished` per node.  It
knows nothing of levels: messages are handled in time order and the forwardAndForget, duplicate and extra
branches are kept and counted, so "every node is reached once" is measured here, not assumed.  The outputs are
those of refmodel_broadcast.BroadcastReplay.run (plus `extra`); the message lengths are that module's, since
the PastryBroadcastInfo object is attached with addObject and its length is set on the object, not on the call.
"""
from __future__ import annotations

import heapq
import math

import numpy as np

from refmodel import between_lr, coord_ns, simtime
from refmodel_broadcast import (BASEAPPDATA_L, NODE_DTYPE, NONE, STAT_FIELDS, UDP_IP_BYTES, byte_length, request_bits,  # noqa: F401
                                response_bits, stats_equal)
from refmodel_pastry import PastryNet, shared_prefix_length


def _between_l(x, a, b):
    """OverlayKey::isBetweenL: [a, b)."""
    return x == a or (between_lr(x, a, b) and x != b)


class PastryBroadcastReplay:
    def __init__(self, net: PastryNet, simtimeRound: int = 1, datarate: float = 10e6, accessDelay: float = 0.0,
                 measureAuthBlock: bool = False):
        self.net, self.n = net, net.n
        self.rnd = bool(simtimeRound)
        self.datarate = datarate
        self.acc = simtime(accessDelay, self.rnd)
        self.auth = bool(measureAuthBlock)
        self._rows = {}

    def rows(self, v: int):
        """The routing table of v: the loaded node's, or the rule's for a network built with nodes=[...]."""
        r = self._rows.get(v)
        if r is None:
            nd = self.net.nodes.get(v)
            r = self._rows[v] = nd.rows if nd is not None else self.net.rule_rows(v)
        return r

    def forward_and_forget(self, v: int, info) -> bool:
        """Pastry::forwardAndForget (1307-1341).  forwardBroadcast never sets midpoint, so this is always False;
        the branch behind it is kept as the reference has it."""
        if info is None:
            return False
        if not info["midpoint"]:
            return False
        ids = self.net.ids
        start, end = info["start"], info["end"]
        if _between_l(ids[v], start, end):
            return False
        for x in self.net.nodes[v].leaves:
            if x is not None and _between_l(ids[x], start, end):
                return True
        return False

    def forward_broadcast(self, v: int, info) -> list[tuple[int, dict]]:
        """Pastry::forwardBroadcast (1343-1390) at node v: (node, BroadcastInfo) per request in list order.  The
        second isUnspecified() test (1374-1381) follows a `continue` on the same condition (1367) and never
        holds: the key of a request is always unspecified, midpoint false."""
        limit = 0 if info is None else info["limit"]
        rows = self.rows(v)
        requests = []
        for row in range(limit, len(rows)):                       # getLastRow() = rows.size()
            for finger in rows[row]:
                if finger is not None and finger == v:
                    continue
                if finger is None:
                    continue
                requests.append((finger, dict(limit=row + 1, midpoint=False, start=None, end=None)))
        return requests

    def run(self, initiator: int, ttl: int, query_bytes: int = 0):
        """One broadcast.  Returns (records, stats, receptions) as BroadcastReplay.run does."""
        n, rnd, xy = self.n, self.rnd, self.net.xy
        call_len = byte_length(request_bits(query_bytes))
        resp_len = byte_length(response_bits(self.auth))
        call_bw = simtime((byte_length(BASEAPPDATA_L + request_bits(query_bytes)) + UDP_IP_BYTES) * 8 / self.datarate, rnd)
        resp_bw = simtime((resp_len + UDP_IP_BYTES) * 8 / self.datarate, rnd)
        rec = np.zeros(n, dtype=NODE_DTYPE)
        rec["arrival_ns"] = -1
        rec["parent"] = NONE
        receptions = np.zeros(n, dtype=np.int64)
        received_from = [None] * n
        started = [False] * n                                      # set for broadcasts older than the node: none here
        tx_finished = [0] * n
        st = dict(expected=n, actual=0, expired=0, duplicated=0, extra=0, messages=0, bytes=0, last_arrival_ns=0)
        hops_seen = []
        seq = 0
        # initBroadcast: an internal RPC to the node's own tier 2, now, with the full TTL and no BroadcastInfo
        heap = [(0, seq, initiator, None, ttl, NONE, 0)]
        while heap:
            t, _, v, info, tau, parent, rank = heapq.heappop(heap)
            receptions[v] += 1
            if self.forward_and_forget(v, info):                   # 220-230
                st["messages"] += 1
                st["bytes"] += resp_len
                continue
            if received_from[v] is not None:                       # 233-244
                st["duplicated"] += 1
                st["messages"] += 1
                st["bytes"] += resp_len
                continue
            if started[v]:                                         # 246-257
                st["extra"] += 1
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
            for j, (f, finfo) in enumerate(self.forward_broadcast(v, info)):     # 305-327
                st["messages"] += 1
                st["bytes"] += call_len
                # sendRouteRpcCall to a node: UDP, SimpleNodeEntry::calcDelay at the sender
                new_tx = max(tx_finished[v], t) + call_bw
                tx_finished[v] = new_tx
                delay = new_tx - t + self.acc + coord_ns(xy, v, f, rnd) + call_bw + self.acc
                seq += 1
                heapq.heappush(heap, (t + delay, seq, f, finfo, tau, v, j))
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

    def walk(self, initiator: int, target: int):
        """The direct walk from the initiator to `target`: at every node the slot (shared digits, the target's
        next digit).  Returns the number of hops, or None where the walk meets an empty slot."""
        ids, b = self.net.ids, self.net.b
        v, hops = initiator, 0
        while v != target:
            r = shared_prefix_length(ids[v], ids[target], b)
            rows = self.rows(v)
            if r >= len(rows):
                return None
            v = rows[r][(ids[target] >> (160 - (r + 1) * b)) & ((1 << b) - 1)]
            if v is None:
                return None
            hops += 1
        return hops
