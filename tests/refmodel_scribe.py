"""Scribe on a converged Chord ring: a message-level event simulation and its closed form, in pure Python.

Test infrastructure only: the independent checker of ovs_scribe_build / ovs_scribe_multicast_batch.
It restates, for the state "every join answered, no timer fired yet",

  Scribe::subscribeToGroup                      Scribe.cc:459-479
  Scribe::forward                               Scribe.cc:113-127
  Scribe::handleJoinCall / handleJoinMessage    Scribe.cc:324-373
  Scribe::addChildToGroup                       Scribe.cc:490-513
  Scribe::handleJoinResponse                    Scribe.cc:410-431
  Scribe::deliverALMDataToRoot                  Scribe.cc:624-661
  Scribe::handlePublishCall / Response          Scribe.cc:375-408, 433-448
  Scribe::deliverALMDataToGroup                 Scribe.cc:664-704
  BaseApp::handleCommonAPIMessage               BaseApp.cc:321-395
  BaseOverlay::sendToKey                        BaseOverlay.cc:1367-1583
  SimpleNodeEntry::calcDelay with the tx queue  SimpleNodeEntry.cc:155-195

The per-hop decisions are the oracle's Chord findNode (oracle_lib.OracleNet.find_node), whole routes
the oracle's route (OracleNet.route), the coordinate delay OracleNet.delay_ns; the queue arithmetic
is restated here in integer ns.

What the reference does that is easy to misread:

* forward() runs before EVERY delivery, not only at intermediate hops: KBR_DELIVER calls forward()
  first (BaseApp.cc:334-341) and a ScribeJoinCall from another node is absorbed there (Scribe.cc:
  122-126, handleJoinMessage(msg, false)).  So the node responsible for the group key absorbs a
  join like any forwarder and sends a join of its own (Scribe.cc:345-350), which reaches itself, is
  not absorbed (srcNode == thisNode, :122) and is handled as root (:324-327): its response sets
  parent = itself (:419).  handleJoinCall with amIRoot = true therefore runs for a node's own
  join only, and a responsible node that is no member still becomes the root as soon as one join
  reaches it.  "Wrong Root" (:379-388) is the answer of a responsible node that no join has reached:
  a group without members, or one whose every join was dropped.
* Under semi-recursive routing with useCommonAPIforward = true a join travels one hop: the first node
  after its source absorbs it.  (The reference's [Config Scribe] sets useCommonAPIforward for Pastry only,
  omnetpp.ini:309, and default.ini:391 sets it false elsewhere: for Chord it is this model's assumption.)
  The join leaves its source with hop count 0 -- hopCountMax = 0 discards it there (BaseOverlay.cc:1464)
  -- and arrives with hop count 1 (sendRouteMessage, :1131).  A first hop that is responsible for the key
  delivers it (:915-982, no hop check) and forward() absorbs it on delivery.  Any other first hop passes it
  to sendToKey (:1003), where the hop check (:1464) comes BEFORE callForward (:1546-1551): with
  hopCountMax = 1 the join is discarded unseen, its sender stays without a parent and the first hop joins
  nothing.  hopCountMax >= 2 cuts no join.
  Under iterative routing nobody forwards (BaseOverlay.cc:1434-1442); a join whose lookup fails (hop
  limit) is dropped (SendToKeyListener) and its sender stays without a parent.
* SCRIBE_PUBLISHRESPONSE_L and SCRIBE_JOINRESPONSE_L are built on BASECALL_L (ScribeMessage.msg:
  37, 39), which has no AUTHBLOCK_L: measureAuthBlock changes no Scribe message.
"""
from __future__ import annotations

import heapq

import numpy as np

from refmodel import simtime

NONE = 0xFFFFFFFF
SUBSCRIBER, ROOT, FORWARDER = 1, 2, 4
OK, WRONG_ROOT, ROUTE_FAILED = 0, 1, 2
NODE_DTYPE = np.dtype([("group", "<u4"), ("node", "<u4"), ("parent", "<u4"), ("depth", "<u2"), ("flags", "<u2")])
MSG_FIELDS = ("response_ns", "last_delivery_ns", "receivers", "forwarded", "publish_hops", "depth", "status")
DELIVERY_DTYPE = np.dtype([("msg", "<u4"), ("node", "<u4"), ("hops", "<u4"), ("pad", "<u4"), ("arrival_ns", "<i8")])

# CommonMessages.msg:30-73 (bits), ScribeMessage.msg:32-43
BASECALL_L = 8 + 32 + (32 + 16 + 160) + 8
BASEAPPDATA_BYTES = 5                   # BASEAPPDATA_L 40 bits
BASEROUTE_BYTES = 53                    # BASEROUTE_L 424 bits
UDP_IP_BYTES = 28                       # SimpleUDP.cc:291
JOINCALL_BYTES = BASECALL_L // 8        # SCRIBE_JOINCALL_L
JOINRESPONSE_BYTES = BASECALL_L // 8    # SCRIBE_JOINRESPONSE_L
PUBLISHRESPONSE_BYTES = (BASECALL_L + 8) // 8   # SCRIBE_PUBLISHRESPONSE_L


def data_bytes(payload: int) -> int:
    return (160 + 8) // 8 + payload     # SCRIBE_DATA_L + the encapsulated ALM payload


def publish_bytes(payload: int) -> int:
    return BASECALL_L // 8 + data_bytes(payload)    # SCRIBE_PUBLISHCALL_L + the ScribeDataMessage


def direct_wire(nbytes: int) -> int:
    """A message to a known node: in a BaseAppDataMessage over UDP (BaseOverlay.cc:1340-1341)."""
    return nbytes + BASEAPPDATA_BYTES + UDP_IP_BYTES


def routed_wire(nbytes: int) -> int:
    """A message to a key: BaseAppDataMessage in a BaseRouteMessage (BaseOverlay.cc:1388-1399)."""
    return nbytes + BASEAPPDATA_BYTES + BASEROUTE_BYTES + UDP_IP_BYTES


class ScribeModel:
    def __init__(self, ids, xy, routingType: int = 1, hopCountMax: int = 50, simtimeRound: int = 1, datarate: float = 10e6,
                 accessDelay: float = 0.0, **chord_kw):
        from oracle_lib import OracleNet, chord_params
        self.ids = np.ascontiguousarray(ids, dtype=np.uint32)
        self.n = len(self.ids)
        self.rnd = bool(simtimeRound)
        self.datarate = datarate
        self.acc = simtime(accessDelay, self.rnd)
        self.rt = routingType
        self.hcm = hopCountMax
        self._mk = lambda **kw: OracleNet("chord", self.ids, xy, chord_params(
            simtimeRound=int(simtimeRound), datarate=datarate, accessDelay=accessDelay, routingType=routingType,
            hopCountMax=hopCountMax, **chord_kw, **kw))
        self.net = self._mk()
        self._routes = {}
        self._nh = {}

    # -- the pieces taken from the oracle -------------------------------------------------------
    def bw(self, nbytes: int) -> int:
        return simtime(nbytes * 8 / self.datarate, self.rnd)

    def coord_ns(self, a: int, b: int) -> int:
        return self.net.delay_ns(a, b, 0) - 2 * self.acc

    def next_hop(self, x: int, key) -> int:
        """findNode(key, recNumRedundantNodes, 1)[0] at x (BaseOverlay.cc:1445-1447, 1507-1521: the first
        candidate passes the loop detection on a converged ring); x itself when it is responsible."""
        k = (x, bytes(np.asarray(key, np.uint32)))
        if k not in self._nh:
            nodes, sib = self.net.find_node(x, key, 1, 1)
            self._nh[k] = x if sib else int(nodes[0])
        return self._nh[k]

    def responsible(self, x: int, key) -> bool:
        """isSiblingFor(x, key, 1) (BaseOverlay.cc:917)."""
        return self.next_hop(x, key) == x

    def route(self, x: int, key, wire_bytes: int):
        """The oracle's one-way route of a wire_bytes message from x to key: (status, node, latency, hops)."""
        if wire_bytes not in self._routes:
            self._routes[wire_bytes] = self._mk(routeBytes=wire_bytes)
        r = self._routes[wire_bytes].route(np.asarray(key, np.uint32).reshape(1, 5), [x], record_hops=False)
        return int(r["status"][0]), int(r["responsible"][0]), int(r["latency_ns"][0]), int(r["one_way_hops"][0])

    # -- the transmit queue (SimpleNodeEntry.cc:165-183) ----------------------------------------
    def send(self, txf: dict, t: int, a: int, b: int, wire_bytes: int) -> int:
        if a == b:
            return t                                          # SimpleUDP.cc:322: no delay to the node itself
        bw = self.bw(wire_bytes)
        tx = max(txf.get(a, 0), t) + bw
        txf[a] = tx
        return tx + self.acc + self.coord_ns(a, b) + bw + self.acc

    # -- joins as events ------------------------------------------------------------------------
    def simulate_joins(self, group_keys, members, start_times=None):
        """members: (group, node) pairs in issue order; start_times: when each subscribes (default 0, 1, ...).
        Returns {(group, node): dict(parent, subscribed, children)} once no message is in flight."""
        state, txf, heap, seq = {}, {}, [], [0]

        def push(t, *ev):
            seq[0] += 1
            heapq.heappush(heap, (t, seq[0], ev))

        def send_join(t, x, g):
            key = group_keys[g]
            if self.rt == 0:
                st, R, lat, _ = self.route(x, key, routed_wire(JOINCALL_BYTES))
                if st == 0:                                   # else the lookup failed: the call is dropped
                    push(t + lat, "join", R, x, g, 0)
                return
            if self.hcm <= 0:                                 # BaseOverlay.cc:1464: discarded at its source
                return
            nh = self.next_hop(x, key)
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
                # a routed message at a node that is not responsible goes through sendToKey (:1003), whose
                # hop check (:1464) precedes callForward (:1546): dropped before forward() sees it
                if self.rt != 0 and not self.responsible(y, group_keys[g]) and hop_count >= self.hcm:
                    continue
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

    # -- the closed form ------------------------------------------------------------------------
    def closure(self, group_keys, members):
        """The same state as the closure of the memberships under "next hop towards the group key"."""
        state = {}
        frontier = []
        for g, x in members:
            g, x = int(g), int(x)
            if (g, x) not in state:
                state[(g, x)] = dict(parent=None, subscribed=True, children=set())
                frontier.append((g, x, True))
        while frontier:
            nxt = []
            for g, x, member in frontier:
                if self.rt == 0 and member:
                    st, R, _, _ = self.route(x, group_keys[g], routed_wire(JOINCALL_BYTES))
                    p = R if st == 0 else None
                elif self.rt != 0 and self.hcm <= 0:
                    p = None
                else:
                    p = self.next_hop(x, group_keys[g])
                    if self.rt != 0 and self.hcm == 1 and p != x and not self.responsible(p, group_keys[g]):
                        p = None                              # discarded by the first hop's sendToKey
                state[(g, x)]["parent"] = p
                if p is None or p == x:
                    continue
                if (g, p) not in state:
                    state[(g, p)] = dict(parent=None, subscribed=False, children=set())
                    nxt.append((g, p, False))
                state[(g, p)]["children"].add(x)
            frontier = nxt
        return state

    @staticmethod
    def records(state) -> np.ndarray:
        rec = np.zeros(len(state), dtype=NODE_DTYPE)
        for i, (g, x) in enumerate(sorted(state)):
            S = state[(g, x)]
            d, v = 0, x
            while state[(g, v)]["parent"] not in (None, v):
                v = state[(g, v)]["parent"]
                d += 1
            fl = (SUBSCRIBER if S["subscribed"] else 0) | (ROOT if S["parent"] == x else 0) | (FORWARDER if S["children"] else 0)
            rec[i] = (g, x, NONE if S["parent"] is None else S["parent"], d, fl)
        return rec

    # -- publishes ------------------------------------------------------------------------------
    def _publish_leg(self, state, key, g, s, known, payload):
        """(responsible node or None, arrival, hops) of the ScribePublishCall (624-661)."""
        roots = [x for (gg, x), S in state.items() if gg == g and S["parent"] == x]
        if known and roots:                                   # 652-654: straight to the rendezvous point
            R = roots[0]
            return R, self.send({}, 0, s, R, direct_wire(publish_bytes(payload))), int(R != s)
        st, R, lat, hops = self.route(s, key, routed_wire(publish_bytes(payload)))
        return (R, lat, hops) if st == 0 else (None, -1, 0)

    def publish_events(self, state, group_keys, g, s, known=False, payload=100):
        """One publish as events on idle queues.  Returns (fields dict, [(node, hops, arrival)])."""
        out = dict(response_ns=-1, last_delivery_ns=-1, receivers=0, forwarded=0, publish_hops=0, depth=0, status=ROUTE_FAILED)
        R, t0, hops = self._publish_leg(state, group_keys[g], g, s, known, payload)
        if R is None:
            return out, []
        out["publish_hops"] = hops
        txf, heap, seq, deliveries = {}, [], 0, []
        G = state.get((g, R))
        if G is None or G["parent"] != R:                     # 379-388
            out["status"] = WRONG_ROOT
            out["response_ns"] = self.send(txf, t0, R, s, direct_wire(PUBLISHRESPONSE_BYTES))
            return out, []
        out["status"] = OK
        out["response_ns"] = self.send(txf, t0, R, s, direct_wire(PUBLISHRESPONSE_BYTES))      # 392-395, before 406
        heap.append((t0, 0, R, 0))
        while heap:
            t, _, v, h = heapq.heappop(heap)
            S = state[(g, v)]
            out["depth"] = max(out["depth"], h)
            for c in sorted(S["children"]):                   # 687-692: std::set<NodeHandle> order
                seq += 1
                out["forwarded"] += 1
                heapq.heappush(heap, (self.send(txf, t, v, c, direct_wire(data_bytes(payload))), seq, c, h + 1))
            if S["subscribed"]:                               # 695-701
                deliveries.append((v, h, t))
                out["receivers"] += 1
                out["last_delivery_ns"] = max(out["last_delivery_ns"], t)
        return out, sorted(deliveries)

    def publish_closed(self, state, group_keys, g, s, known=False, payload=100):
        """The same level by level: child k of p hears at t_p + (k + 2) T(data) + 2 T(access) + coord,
        one T(response) later below a root that answers another node."""
        out = dict(response_ns=-1, last_delivery_ns=-1, receivers=0, forwarded=0, publish_hops=0, depth=0, status=ROUTE_FAILED)
        R, t0, hops = self._publish_leg(state, group_keys[g], g, s, known, payload)
        if R is None:
            return out, []
        out["publish_hops"] = hops
        bwr, bwd = self.bw(direct_wire(PUBLISHRESPONSE_BYTES)), self.bw(direct_wire(data_bytes(payload)))
        out["response_ns"] = t0 if R == s else t0 + 2 * bwr + 2 * self.acc + self.coord_ns(R, s)
        G = state.get((g, R))
        if G is None or G["parent"] != R:
            out["status"] = WRONG_ROOT
            return out, []
        out["status"] = OK
        deliveries = []
        level, h = [(R, t0, t0 + (0 if R == s else bwr))], 0
        while level:
            nxt = []
            for v, t, tsend in level:
                S = state[(g, v)]
                if S["subscribed"]:
                    deliveries.append((v, h, t))
                for k, c in enumerate(sorted(S["children"])):
                    tc = tsend + (k + 2) * bwd + 2 * self.acc + self.coord_ns(v, c)
                    nxt.append((c, tc, tc))
            out["forwarded"] += len(nxt)
            if nxt:
                out["depth"] = h + 1
            level, h = nxt, h + 1
        out["receivers"] = len(deliveries)
        out["last_delivery_ns"] = max((t for _, _, t in deliveries), default=-1)
        return out, sorted(deliveries)

    def multicast(self, state, group_keys, msg_group, msg_src, known=None, payload=100, events=False):
        """A batch: (list of field dicts, DELIVERY_DTYPE records sorted by (msg, node))."""
        fn = self.publish_events if events else self.publish_closed
        outs, recs = [], []
        for m, (g, s) in enumerate(zip(msg_group, msg_src)):
            o, d = fn(state, group_keys, int(g), int(s), bool(known[m]) if known is not None else False, payload)
            outs.append(o)
            recs += [(m, v, h, 0, t) for v, h, t in d]
        return outs, np.array(recs, dtype=DELIVERY_DTYPE) if recs else np.zeros(0, DELIVERY_DTYPE)


def msg_mismatches(engine_out, ref_outs) -> list:
    return [(m, f, int(engine_out[f][m]), int(o[f])) for m, o in enumerate(ref_outs) for f in MSG_FIELDS
            if int(engine_out[f][m]) != int(o[f])]
