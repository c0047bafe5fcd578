"""IterativeLookup on Pastry, restated line by line in pure Python on top of refmodel_pastry: the checker of
k_pastry_iter (oversim_amd/csrc/pastry.hip).

Test infrastructure only.  One path, one RPC in flight: lookupRedundantNodes = lookupParallelPaths =
lookupParallelRpcs = 1, merge off, visitOnlyOnce on, finishOnFirstUnchanged / newRpcOnEveryResponse /
failedNodeRpcs off (default.ini:423-433).

Cites: IterativeLookup.cc:133-244 (start), 359-390 (createFindNodeCall), 406-449 (addSibling), 588-654
(handleRpcTimeout: the target is dead), 803-921 (handleResponse), 935-1023 (handleTimeout), 1067-1182 (sendRpc,
getNextEntry), 1184-1195 (add: push_back with merge off -- the start vector is the source's answer in its own
order and unbounded, whatever comparator the LookupVector was built with); BasePastry.cc:1090-1098, 1212-1239
(createLookup: the PastryFindNodeExtData object); BaseOverlay.cc:1240-1300 (lookupFinished), 1857-1914
(findNodeRpc), 1938-1968 (lookupRpc); PastryMessage.msg:35; CommonMessages.msg (lengths).
"""
from __future__ import annotations

import numpy as np

from refmodel import coord_ns, msg_ns, simtime, to_int
from refmodel_pastry import NONE, PastryError

OK, TIMEOUT, RPC_TIMEOUT, HOPMAX, NO_NEXT, BROKEN = 0, 1, 2, 3, 4, 5

FINDNODECALL_BITS = 440
FINDNODERESPONSE_BITS = 264
NODEHANDLE_BITS = 208
HOPCOUNT_BITS = 16
AUTHBLOCK_BITS = 800
PASTRY_EXT_BITS = NODEHANDLE_BITS + HOPCOUNT_BITS       # PASTRYFINDNODEEXTDATA_L (PastryMessage.msg:35)
UDP_IP_BYTES = 28


def call_bytes() -> int:
    """FINDNODECALL_L plus the extension createFindNodeCall adds (385-388)."""
    return (FINDNODECALL_BITS + PASTRY_EXT_BITS + 7) // 8 + UDP_IP_BYTES


def resp_bytes(nodes: int, auth=False) -> int:
    """FINDNODERESPONSE_L for `nodes` NodeHandles plus the extension findNodeRpc moves over from the call
    (BaseOverlay.cc:1901-1907); measureAuthBlock adds AUTHBLOCK_L to every response."""
    bits = FINDNODERESPONSE_BITS + NODEHANDLE_BITS * nodes + PASTRY_EXT_BITS + (AUTHBLOCK_BITS if auth else 0)
    return (bits + 7) // 8 + UDP_IP_BYTES


def lookup(net, kw, S, num_siblings=1, hop_max=50, rpc_to=1.5, lk_to=10.0, auth=False):
    """One IterativeLookup for key kw at node S with num_siblings >= 1 siblings (lookupRpc passes getMaxNumSiblings()
    for a negative count before it gets here).  -> dict(status, siblings, hops, latency_ns, hop_seq, rpcs, targets):
    hop_seq the responders in order, targets every FindNodeCall's destination in order."""
    assert num_siblings >= 1
    k = kw if isinstance(kw, int) else to_int(kw)
    rnd, xy, ns = net.rnd, net.xy, num_siblings
    T_rpc, T_lk = simtime(rpc_to, rnd), simtime(lk_to, rnd)
    m_call = msg_ns(call_bytes(), rnd)
    t, hops, seq, rpcs, targets = 0, 0, [], 0, []

    def done(st, sibs=()):
        ok = st == OK
        return dict(status=st, siblings=list(sibs) if ok else [], hops=hops, latency_ns=t if ok else -1, hop_seq=seq, rpcs=rpcs,
                    targets=targets)

    # start (133-244): the local findNode asks for getMaxNumRedundantNodes() = numberOfLeaves nodes
    src = net.nodes[S]
    try:
        next_hops, info = src.find_node(k, net.L, ns)
    except PastryError:
        return done(BROKEN)
    visited, dead = {S}, set()                                   # setVisited(thisNode) (164)
    if not next_hops:
        return done(NO_NEXT)                                     # 167-170
    if info["sib"]:                                              # 186-195: isSiblingFor is true only without err
        return done(OK, next_hops[:ns])                          # addSibling fills a NodeVector(numSiblings) (436-440)
    cands, used = list(next_hops), [False] * len(next_hops)      # pathLookup->add: push_back (1192)
    after_timeout = False
    while True:
        # IterativePathLookup::sendRpc (1067-1170) with num = 1: one entry is looked at (redundantNodes = 1)
        if hop_max and hops >= hop_max:
            return done(HOPMAX)
        entry = next((i for i, c in enumerate(cands) if not used[i] and c not in dead), None)    # getNextEntry
        if entry is None:
            return done(RPC_TIMEOUT if after_timeout else NO_NEXT)
        used[entry] = True
        cur = cands[entry]
        if cur in visited:                                       # visitOnlyOnce (1111): no RPC, none pending
            return done(RPC_TIMEOUT if after_timeout else NO_NEXT)
        rpcs += 1
        targets.append(cur)
        # findNodeRpc at cur (BaseOverlay.cc:1857-1914): numRedundantNodes = config.redundantNodes = 1
        try:
            res, rinfo = net.nodes[cur].find_node(k, 1, ns)
        except PastryError:
            return done(BROKEN)
        cd = coord_ns(xy, S, cur, rnd)
        rtt = m_call + cd + msg_ns(resp_bytes(len(res), auth), rnd) + cd
        if rtt >= T_rpc:
            # handleRpcTimeout (588-654): cur is dead; handleTimeout (935-1023) sends one new RPC
            t += T_rpc
            dead.add(cur)
            if t > T_lk:
                return done(TIMEOUT)
            after_timeout = True
            continue
        t += rtt
        if t > T_lk:                                             # 808-815
            return done(TIMEOUT)
        after_timeout = False
        hops += 1                                                # cur is never the source: the source is visited
        visited.add(cur)
        seq.append(cur)
        if res:
            cands, used = list(res), [False] * len(res)          # replace mode (839-843, 851-855)
        # an empty response leaves the next hops as they were: sendRpc(0) tries the remaining ones (1095-1100)
        if rinfo["sib"] and res:                                 # 872-878, 897-905
            return done(OK, res[:ns])


def route(net, kw, S, hop_max=50, rpc_to=1.5, lk_to=10.0, auth=False, route_bytes=186):
    """The KBRTestApp one-way message under iterative routing: the lookup with numSiblings = 1 and
    sendRouteMessage to getResult()[0] (BaseOverlay.cc:1240-1258)."""
    r = lookup(net, kw, S, 1, hop_max, rpc_to, lk_to, auth)
    if r["status"] != OK:
        return dict(responsible=NONE, hops=r["hops"], status=r["status"], one_way_hops=0, latency_ns=-1, hop_seq=r["hop_seq"])
    R = r["siblings"][0]
    lat = r["latency_ns"] + (msg_ns(route_bytes, net.rnd) + coord_ns(net.xy, S, R, net.rnd) if R != S else 0)
    return dict(responsible=R, hops=r["hops"], status=OK, one_way_hops=r["hops"] + int(R != S), latency_ns=lat,
                hop_seq=r["hop_seq"])


def lookups(net, keys, src, num_siblings=1, **kw):
    """Model LookupCalls as arrays: siblings (n, num_siblings) and hop_seq (n, hop_max) NONE padded."""
    res = [lookup(net, k, int(s), num_siblings, **kw) for k, s in zip(keys, src)]
    H = kw.get("hop_max", 50)
    out = dict(num_siblings=np.array([len(r["siblings"]) for r in res], dtype=np.uint32),
               hops=np.array([r["hops"] for r in res], dtype=np.uint16),
               status=np.array([r["status"] for r in res], dtype=np.uint8),
               is_valid=np.array([r["status"] == OK for r in res], dtype=np.uint8),
               latency_ns=np.array([r["latency_ns"] for r in res], dtype=np.int64),
               rpcs=np.array([r["rpcs"] for r in res], dtype=np.uint32),
               siblings=np.full((len(res), num_siblings), NONE, dtype=np.uint32),
               hop_seq=np.full((len(res), H), NONE, dtype=np.uint32))
    for i, r in enumerate(res):
        out["siblings"][i, :len(r["siblings"])] = r["siblings"]
        out["hop_seq"][i, :len(r["hop_seq"])] = r["hop_seq"]
    return out


def routes(net, keys, src, **kw):
    res = [route(net, k, int(s), **kw) for k, s in zip(keys, src)]
    H = kw.get("hop_max", 50)
    out = dict(responsible=np.array([r["responsible"] for r in res], dtype=np.uint32),
               hops=np.array([r["hops"] for r in res], dtype=np.uint16),
               status=np.array([r["status"] for r in res], dtype=np.uint8),
               one_way_hops=np.array([r["one_way_hops"] for r in res], dtype=np.uint8),
               latency_ns=np.array([r["latency_ns"] for r in res], dtype=np.int64),
               hop_seq=np.full((len(res), H), NONE, dtype=np.uint32))
    for i, r in enumerate(res):
        out["hop_seq"][i, :len(r["hop_seq"])] = r["hop_seq"]
    return out
