"""The DHT replay's LookupCall on Pastry -- test infrastructure only, never calls the engine.

tests/refmodel_dht.DhtModel takes its sibling list, hop count and latency from a `lookup` callable.  Two of
them for a Pastry network (refmodel_pastry.PastryNet):

  pastry_lookup           the iterative LookupCall of tests/refmodel_pastry_iter.py with numSiblings = numReplica,
                          as oracle_lookup feeds the replay from the CPU oracle
  pastry_measured_lookup  the same lookup replayed message by message through real per-node transmit queues
                          (SimpleNodeEntry.cc:164-194), the counterpart of refmodel_dht.chord_measured_lookup: it
                          reports src_tx_finished, the source's tx.finished when the lookup completes, which
                          DhtModel.start_queue asserts not to lie beyond the completion time

The exactness premise it measures (DESIGN.md "DHT on Pastry"): with one path and one RPC in flight the lookup
completes on a FindNodeResponse that arrives a full round trip after the source's last FindNodeCall left, or at
t0 with no message at all when the source's own findNode carries the siblings flag; after an RPC timeout the
next start-vector entry is called at the timeout instant, and that call too is a round trip old at completion;
a failed lookup sends no DHT message.

Lengths: FINDNODECALL_L 440 bits and FINDNODERESPONSE_L 264 bits + 208 per NodeHandle, each plus the 224 bits
(28 B) of the PastryFindNodeExtData object (PastryMessage.msg:35; IterativeLookup.cc:385-388,
BaseOverlay.cc:1903-1907), +800 bits (100 B) in every response under measureAuthBlock, + 28 B UDP/IP.
"""
from __future__ import annotations

import numpy as np

import refmodel_pastry_iter as RI
from refmodel import coord_ns, simtime, to_int
from refmodel_pastry import NONE, PastryError

FIELDS = ("siblings", "num_siblings", "hops", "status", "is_valid", "latency_ns")


def pastry_lookup(net, num_replica: int, **kw):
    """LookupCalls with numSiblings = numReplica from refmodel_pastry_iter (kw: hop_max, rpc_to, lk_to, auth)."""
    def lookup(keys, src):
        return RI.lookups(net, keys, src, num_replica, **kw)
    return lookup


def measured_one(net, k: int, S: int, ns: int, hop_max=50, rpc_to=1.5, lk_to=10.0, auth=False, datarate=10e6):
    """One IterativeLookup (one path, one RPC in flight, merge off, visitOnlyOnce) with every FindNodeCall sent
    through the source's transmit queue and every FindNodeResponse through the responder's.
    -> (siblings, hops, status, latency_ns, src_tx_finished)."""
    rnd, xy = net.rnd, net.xy
    T_rpc, T_lk = simtime(rpc_to, rnd), simtime(lk_to, rnd)
    txq: dict[int, int] = {}

    def hop(a, b, nb, now):
        """Arrival at b of an nb-byte packet a sends at `now`: the sender's queue, the wire, the receiver's line."""
        bw = simtime((nb * 8) / datarate, rnd)
        fin = max(txq.get(a, 0), now) + bw
        txq[a] = fin
        return fin + coord_ns(xy, a, b, rnd) + bw

    t = hops = 0

    def done(st, sibs=()):
        return (list(sibs) if st == RI.OK else []), hops, st, (t if st == RI.OK else -1), txq.get(S, 0)

    try:                                                     # IterativeLookup::start (133-244)
        cands, info = net.nodes[S].find_node(k, net.L, ns)
    except PastryError:
        return done(RI.BROKEN)
    if not cands:
        return done(RI.NO_NEXT)
    if info["sib"]:
        return done(RI.OK, cands[:ns])                       # the key is local: no message, the queue never used
    visited, dead, used, after_timeout = {S}, set(), set(), False
    cands = list(cands)
    while True:                                              # IterativePathLookup::sendRpc (1067-1170)
        if hop_max and hops >= hop_max:
            return done(RI.HOPMAX)
        entry = next((i for i, c in enumerate(cands) if i not in used and c not in dead), None)
        if entry is None or cands[entry] in visited:
            return done(RI.RPC_TIMEOUT if after_timeout else RI.NO_NEXT)
        used.add(entry)
        cur = cands[entry]
        try:                                                 # findNodeRpc at cur (BaseOverlay.cc:1857-1914)
            res, rinfo = net.nodes[cur].find_node(k, 1, ns)
        except PastryError:
            return done(RI.BROKEN)
        back = hop(cur, S, RI.resp_bytes(len(res), auth), hop(S, cur, RI.call_bytes(), t))
        if back - t >= T_rpc:                                # handleRpcTimeout (588-654), handleTimeout (935-1023)
            t += T_rpc
            dead.add(cur)
            if t > T_lk:
                return done(RI.TIMEOUT)
            after_timeout = True
            continue
        t = back
        if t > T_lk:                                         # 808-815
            return done(RI.TIMEOUT)
        after_timeout = False
        hops += 1
        visited.add(cur)
        if res:                                              # replace mode (839-843)
            cands, used = list(res), set()
        if rinfo["sib"] and res:                             # 897-905
            return done(RI.OK, res[:ns])


def pastry_measured_lookup(net, num_replica: int, hop_max=50, rpc_to=1.5, lk_to=10.0, auth=False, datarate=10e6):
    """The `lookup` callable of DhtModel with src_tx_finished, relative to the lookup's start."""
    def lookup(keys, src):
        rows = [measured_one(net, to_int(k), int(s), num_replica, hop_max, rpc_to, lk_to, auth, datarate)
                for k, s in zip(keys, src)]
        sibs = np.full((len(rows), max(num_replica, 1)), NONE, dtype=np.uint32)
        for i, r in enumerate(rows):
            sibs[i, :len(r[0])] = r[0]
        return dict(siblings=sibs, num_siblings=np.array([len(r[0]) for r in rows], dtype=np.uint32),
                    hops=np.array([r[1] for r in rows], dtype=np.uint16),
                    status=np.array([r[2] for r in rows], dtype=np.uint8),
                    is_valid=np.array([r[2] == RI.OK for r in rows], dtype=np.uint8),
                    latency_ns=np.array([r[3] for r in rows], dtype=np.int64),
                    src_tx_finished=np.array([r[4] for r in rows], dtype=np.int64))
    return lookup
