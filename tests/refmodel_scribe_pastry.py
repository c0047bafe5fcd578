"""Scribe on converged Pastry tables: tests/refmodel_scribe.py's event simulation and closed form with Pastry
underneath (tests/refmodel_pastry.py), in pure Python.

Test infrastructure only: the independent checker of ovs_scribe_build / ovs_scribe_multicast_batch on a context
loaded with ovs_pastry_load.  This is the reference's own Scribe configuration ([Config Scribe]: overlayType =
PastryModules, useCommonAPIforward = true), so nothing about forward() is assumed here.  The state is the same:
"every join answered, no timer fired"; routing is semi-recursive (routingType 1) without per-hop acks.

ScribeModel's seams are overridden -- __init__, next_hop, responsible, route, coord_ns -- and simulate_joins,
because a Pastry first hop that is not responsible runs sendToKey's findNode and candidate loop
(BaseOverlay.cc:1443-1521) with last hop = source = the join's sender BEFORE callForward (:1546) lets forward()
absorb the join: a join it cannot forward is dropped unseen.  The event simulation restates that step in full;
the closed form (closure, inherited) does not, and is exact where no first hop ever refuses -- the premise
tests/test_scribe_pastry_model.py asserts on rule-built tables.  Pastry::recursiveRoutingHook (Pastry.cc:562-589)
acts on Pastry's own join messages only and always forwards: it adds nothing.

    next_hop(x, K)   the pick of sendToKey's source step at x: findNode(K, recNumRedundantNodes, 1) and the
                     candidate loop with no last hop and source = x; x itself where it is the sibling for K;
                     None where the step ends without a node (NO_NEXT, BROKEN): the join is dropped
    responsible      isSiblingFor(x, K, 1), what receipt asks before it delivers (:907-918)
    route            PastryNet.route under the message's wire length

refmodel_pastry's delays take the default datarate (10 Mbit/s) and accessDelay (0) only, so this model does too
and refuses other values.
"""
from __future__ import annotations

import heapq

import numpy as np

import refmodel_pastry as RP
from refmodel import coord_ns, simtime, to_int
from refmodel_scribe import JOINCALL_BYTES, JOINRESPONSE_BYTES, ScribeModel, direct_wire, routed_wire


def _int(key) -> int:
    return key if isinstance(key, int) else to_int(key)


class _LazyNodes(dict):
    """PastryNet.nodes filled by the converged-table rule on first use (a forest touches few of 2^14 nodes)."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def __missing__(self, v):
        nd = RP.PastryNode(self.net, v)
        nd.leaves = self.net.rule_leaves(v)
        nd.rows = self.net.rule_rows(v)
        nd.is_full = nd.leaves[0] is not None and nd.leaves[-1] is not None
        self[v] = nd
        return nd


class ScribePastryModel(ScribeModel):
    def __init__(self, ids, xy, hopCountMax: int = 50, simtimeRound: int = 1, datarate: float = 10e6,
                 accessDelay: float = 0.0, bitsPerDigit: int = 4, numberOfLeaves: int = 16, optimizeLookup: bool = False,
                 useRegularNextHop: bool = True, recNumRedundantNodes: int = 3, tables=None):
        if datarate != 10e6 or accessDelay != 0.0:
            raise ValueError("refmodel_pastry models the default datarate and accessDelay only")
        self.ids = np.ascontiguousarray(ids, dtype=np.uint32)
        self.n = len(self.ids)
        self.xy = xy
        self.rnd = bool(simtimeRound)
        self.datarate = datarate
        self.acc = simtime(accessDelay, self.rnd)
        self.rt = 1
        self.hcm = hopCountMax
        self.rnr = recNumRedundantNodes
        self.net = RP.PastryNet(self.ids, xy, bitsPerDigit, numberOfLeaves, bool(optimizeLookup), bool(useRegularNextHop),
                                rnd=self.rnd, tables=tables, nodes=[] if tables is None else None)
        if tables is None:
            self.net.nodes = _LazyNodes(self.net)
        self._nh = {}

    # -- the pieces taken from the Pastry model ---------------------------------------------------
    def coord_ns(self, a: int, b: int) -> int:
        return coord_ns(self.xy, a, b, self.rnd)

    def step(self, cur: int, key, last, S: int):
        """sendToKey's findNode and candidate loop at cur for a message from `last` with source S
        (BaseOverlay.cc:1443-1449, 1507-1521) -> (node or None, status)."""
        k = _int(key)
        nd = self.net.nodes[cur]
        try:
            cands, _ = nd.find_node(k, self.rnr, 1)
        except RP.PastryError:
            return None, RP.BROKEN
        if not cands:
            return None, RP.NO_NEXT
        sib = nd.is_sibling_for(k, 1)[0]
        for c in cands:
            if (last == c and c != cur) or (c == S and cur != S) or (c == cur and not sib):
                continue
            return c, RP.OK
        return None, RP.NO_NEXT

    def next_hop(self, x: int, key):
        k = (x, _int(key))
        if k not in self._nh:
            self._nh[k] = self.step(x, k[1], None, x)[0]
        return self._nh[k]

    def responsible(self, x, key) -> bool:
        if x is None:                     # a join dropped at its source has no first hop: nothing to ask (closure)
            return True
        return self.net.nodes[x].is_sibling_for(_int(key), 1)[0]

    def route(self, x: int, key, wire_bytes: int):
        r = self.net.route(_int(key), x, rec_num_redundant=self.rnr, hop_max=self.hcm, route_bytes=wire_bytes)
        return int(r["status"]), int(r["responsible"]), int(r["latency_ns"]), int(r["one_way_hops"])

    # -- joins as events --------------------------------------------------------------------------
    def simulate_joins(self, group_keys, members, start_times=None, log=None):
        """As ScribeModel.simulate_joins, with the first hop's own sendToKey.  log (a dict) counts what the premise
        is about: joins dropped at the source, dropped by a first hop's candidate loop, and first hops whose pick
        for the sender's join differs from their own source step's."""
        state, txf, heap, seq = {}, {}, [], [0]
        log = log if log is not None else {}
        for f in ("src_drop", "hop_drop", "pick_differs"):
            log.setdefault(f, 0)

        def push(t, *ev):
            seq[0] += 1
            heapq.heappush(heap, (t, seq[0], ev))

        def send_join(t, x, g):
            key = group_keys[g]
            nh, st = self.step(x, key, None, x)               # findNode comes first (:1445-1449), then the hop check
            if nh is None:
                log["src_drop"] += 1
                return
            if self.hcm <= 0:                                 # BaseOverlay.cc:1464: discarded at its source
                return
            push(self.send(txf, t, x, nh, routed_wire(JOINCALL_BYTES)), "join", nh, x, g, int(nh != x))

        def group(y, g):
            new = (g, y) not in state
            return state.setdefault((g, y), dict(parent=None, subscribed=False, children=set())), new

        for i, (g, x) in enumerate(members):
            push(i if start_times is None else start_times[i], "subscribe", int(x), int(g))
        while heap:
            t, _, ev = heapq.heappop(heap)
            if ev[0] == "subscribe":                          # 459-479
                _, x, g = ev
                G, new = group(x, g)
                G["subscribed"] = True
                if new or G["parent"] is None:
                    send_join(t, x, g)
            elif ev[0] == "join":                             # at y from src: forward() / handleJoinCall
                _, y, src, g, hop_count = ev
                key = group_keys[g]
                if y != src and not self.responsible(y, key):
                    # not delivered on receipt (:907-918): sendToKey (:1003) runs findNode, the hop check (:1464) and
                    # the candidate loop with last hop = source = the sender before callForward (:1546)
                    nx, st = self.step(y, key, src, src)
                    if st == RP.OK and hop_count >= self.hcm:
                        continue
                    if nx is None:
                        log["hop_drop"] += 1
                        continue
                    if nx != self.next_hop(y, key):
                        log["pick_differs"] += 1
                am_root = y == src                            # 122: only a node's own join passes forward()
                G, new = group(y, g)
                if not am_root and (new or G["parent"] is None):      # 345-350
                    send_join(t, y, g)
                if src != y:                                  # 492-495
                    G["children"].add(src)
                push(self.send(txf, t, y, src, direct_wire(JOINRESPONSE_BYTES)), "response", src, y, g)   # 369-372
            else:                                             # 410-419
                _, x, frm, g = ev
                if (g, x) in state:
                    state[(g, x)]["parent"] = frm
        return state
