"""Independent Python reading of the replica-team DHTs (src/applications/dht/SymmetricDHT.cc,
RepeatedHashingDHT.cc over DHT.cc) -- test infrastructure only.  It never calls the engine.

One DHTputCAPICall / DHTgetCAPICall becomes numReplicaTeams copies under derived keys, each with its own
LookupCall for numReplica / T siblings and its own replica RPCs, all started at t0 from one node.  An operation
is an event-heap simulation, ordered by (time, insertion sequence), of ALL its messages with one transmit queue
per node (SimpleNodeEntry.cc:164-194):

  lookup  every FindNodeCall (83 B) and FindNodeResponse (61 B + 26 B per NodeHandle, + 100 B with
          measureAuthBlock) of a team's chain, the chain from refmodel.ChordRing.decide; rpcUdpTimeout per call,
          LOOKUP_TIMEOUT checked on every response, the hop budget and the visited check as
          refmodel_dht.chord_measured_lookup states them (IterativeLookup.cc:803-921, 1067-1170)
  put/get the rules of refmodel_dht.DhtModel (DHT.cc), as event handlers; the store, the lengths and the
          underlay's send() are DhtModel's own
  keys    Python ints and hashlib.sha1 (OverlayKey.cc:60, 163-181, 274-279, 685-701)

A timeout is scheduled when its call is sent (BaseRpc.cc:257-258), before the call itself, so it precedes a
response of the same instant.  A responder answers a call whether or not the caller still waits for it.  The
operation's record is the record of the team that finishes first in event order, success or failure.
"""
from __future__ import annotations

import hashlib
import heapq

import numpy as np

import refmodel
import refmodel_dht as D

SYMMETRIC, REPEATED_HASHING = 0, 1
M160 = 1 << 160


def offset(teams: int) -> int:
    """overlayKeyOffset = OverlayKey::getMax() / numReplicaTeams (mpn_divrem_1)."""
    return (M160 - 1) // teams


def next_key(k: int, mode: int, teams: int) -> int:
    if mode == SYMMETRIC:
        return (k + offset(teams)) % M160
    return int.from_bytes(hashlib.sha1(format(k, "040x").encode()).digest(), "big")


def team_keys_int(k: int, mode: int, teams: int) -> list:
    out = [k]
    for _ in range(teams - 1):
        out.append(next_key(out[-1], mode, teams))
    return out


def words(k: int) -> np.ndarray:
    return np.array([(k >> (32 * i)) & 0xFFFFFFFF for i in range(5)], dtype=np.uint32)


def team_keys(keys, mode: int, teams: int) -> np.ndarray:
    """(n, T, 5) uint32."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    out = np.zeros((len(keys), teams, 5), dtype=np.uint32)
    for i, kw in enumerate(keys):
        for j, k in enumerate(team_keys_int(refmodel.to_int(kw), mode, teams)):
            out[i, j] = words(k)
    return out


def check_params(num_replica: int, teams: int) -> None:
    """SymmetricDHT.cc:40-43."""
    if num_replica % teams:
        raise ValueError("numReplica must be a multiple of numReplicaTeams")


class _Team:
    def __init__(self, j, key, kw, dtype):
        self.j, self.key, self.kw = j, key, kw
        self.o = np.zeros((), dtype=dtype)
        self.done = False
        self.hops, self.visited = 0, set()
        self.m = self.ok = self.bad = 0
        # get
        self.sibs, self.replica, self.resp = [], [], []
        self.value_sent, self.chosen, self.nresp, self.msgs, self.bytes = False, None, 0, 0, 0


class TeamDhtModel:
    def __init__(self, ring, mode, teams, rnd=True, num_replica=8, num_get_requests=4, ratio_identical=0.5,
                 rpc_udp_timeout=1.5, lookup_timeout=10.0, hop_max=50, datarate=10e6, access=0.0, auth=False):
        check_params(num_replica, teams)
        self.ring, self.mode, self.T = ring, mode, teams
        self.r = num_replica // teams
        self.D = D.DhtModel(ring.xy, None, rnd, self.r, num_get_requests, ratio_identical, rpc_udp_timeout, datarate,
                            access, auth)
        self.lk = D.simtime(lookup_timeout, rnd)
        self.hop_max = hop_max
        self.m = min(self.r, 1 + ring.ns)                     # what the responsible node answers
        self.resp_base = 61 + (100 if auth else 0)

    # the store is DhtModel's
    def dump(self, node, now):
        return self.D.dump(node, now)

    def count(self):
        return self.D.count()

    # ------------------------------------------------------------ one operation
    def _run(self, i, kw, S, op, is_put, writes):
        Dm, ring, n = self.D, self.ring, self.ring.n
        t0, to = int(op["t0_ns"]), self.D.to
        heap, seq, txq, order = [], [0], {}, []
        dtype = D.PUT_DTYPE if is_put else D.GET_DTYPE
        teams = [_Team(j, k, words(k), dtype)
                 for j, k in enumerate(team_keys_int(refmodel.to_int(kw), self.mode, self.T))]

        def push(t, fn, *a):
            heapq.heappush(heap, (t, seq[0], fn, a))
            seq[0] += 1

        def rpc_call(tm, target, wire, now, on_arrival, on_response, on_timeout):
            rpc = {"dead": False, "done": False, "target": target}
            push(now + to, timeout, tm, rpc, on_timeout)
            a = Dm.send(txq, S, target, wire, now)
            push(a, on_arrival, tm, rpc, on_response)
            return rpc, a

        def timeout(now, tm, rpc, on_timeout):
            if rpc["done"]:
                return
            rpc["dead"] = True
            if not tm.done:                                   # the team's pending RPCs went with its state
                on_timeout(now, tm, rpc)

        def respond(now, tm, rpc, on_response, wire):
            back = Dm.send(txq, rpc["target"], S, wire, now)
            push(back, response, tm, rpc, on_response)

        def response(now, tm, rpc, on_response):
            if rpc["dead"] or tm.done:
                return
            rpc["done"] = True
            on_response(now, tm, rpc)

        def finish(tm, outcome, now, status=0):
            o = tm.o
            o["outcome"], o["status"] = outcome, status
            o["latency_ns"] = -1 if outcome == D.LOOKUP_FAILED else now - t0
            if outcome == D.LOOKUP_FAILED:
                o["hop_count"] = 0
            tm.done = True
            order.append(tm.j)

        # ---- the LookupCall
        def find_node(tm, cur, now):
            rpc_call(tm, cur, 83, now, fn_arrival, fn_response, fn_timeout)

        def fn_arrival(now, tm, rpc, on_response):
            sib, nxt = ring.decide(rpc["target"], tm.key)
            rpc["sib"], rpc["nxt"] = sib, nxt
            respond(now, tm, rpc, on_response, self.resp_base + 26 * (self.m if sib else 1))

        def fn_timeout(now, tm, rpc):
            finish(tm, D.LOOKUP_FAILED, now, 1 if now > t0 + self.lk else 2)

        def fn_response(now, tm, rpc):
            if now > t0 + self.lk:                            # IterativeLookup.cc:808-815
                return finish(tm, D.LOOKUP_FAILED, now, 1)
            cur = rpc["target"]
            tm.hops += 1
            tm.visited.add(cur)
            if rpc["sib"]:
                return lookup_ok(tm, [(cur + x) % n for x in range(self.m)], now)
            if self.hop_max and tm.hops >= self.hop_max:
                return finish(tm, D.LOOKUP_FAILED, now, 3)
            if rpc["nxt"] in tm.visited:
                return finish(tm, D.LOOKUP_FAILED, now, 4)
            find_node(tm, rpc["nxt"], now)

        def lookup_ok(tm, sibs, now):
            tm.o["hop_count"] = tm.hops                       # DHT.cc:866-867, 929-930
            tm.m = len(sibs)
            (put_start if is_put else get_start)(tm, sibs, now)

        # ---- put (DhtModel.put_batch)
        vlen = int(op["vlen"])
        call_bits = D.BASERPC_BITS + Dm.auth + vlen + D.ENTRY_BITS
        resp_bits = D.BASERPC_BITS + Dm.auth + 8

        def put_start(tm, sibs, now):
            ek = (tm.kw.tobytes(), int(op["kind"]), int(op["id"]))
            for r in sibs:                                    # DHT.cc:876-891, back to back
                _, a = rpc_call(tm, r, D.wire_bytes(call_bits), now, put_arrival, put_response, put_timeout)
                writes.append((a, i, tm.j, r, ek, int(op["token"]), vlen, int(op["ttl"])))
            tm.o["num_sent"], tm.o["messages"] = tm.m, 2 * tm.m
            tm.o["bytes"] = tm.m * (D.nbytes(call_bits) + D.nbytes(resp_bits))

        def put_arrival(now, tm, rpc, on_response):
            respond(now, tm, rpc, on_response, D.wire_bytes(resp_bits))

        def put_response(now, tm, rpc):
            tm.ok += 1                                        # DHT.cc:560-561
            if tm.ok / tm.m > 0.5:                            # DHT.cc:568
                tm.o["num_responses"] = tm.ok
                finish(tm, D.SUCCESS, now)

        def put_timeout(now, tm, rpc):
            tm.bad += 1                                       # DHT.cc:172
            if tm.bad / tm.m >= 0.5:                          # DHT.cc:174
                tm.o["num_responses"] = tm.ok
                finish(tm, D.FAILED, now)

        # ---- get (DhtModel.get_one)
        def get_start(tm, sibs, now):
            tm.ek = (tm.kw.tobytes(), int(op["kind"]), int(op["id"]))
            tm.sibs, tm.replica = sibs, sibs[Dm.G:]           # DHT.cc:947-950
            tm.o["num_sent"] = min(len(sibs), Dm.G)
            for r in sibs[:Dm.G]:                             # DHT.cc:934-946
                get_send(tm, r, True, now)

        def get_send(tm, target, is_hash, now):
            rpc, a = rpc_call(tm, target, D.wire_bytes(D.GETCALL_BITS), now, get_arrival, get_response, get_timeout)
            e = Dm.entry(target, tm.ek, a)                    # DHT.cc:441-443
            if e is None:                                     # DHT.cc:462-464
                bits, h = D.BASERPC_BITS + Dm.auth + 160, (0, 0)
            elif is_hash:                                     # DHT.cc:466-481
                bits, h = D.BASERPC_BITS + Dm.auth + 160 + D.HASH_BITS, (1, e[0])
            else:                                             # DHT.cc:483-487
                bits, h = D.BASERPC_BITS + Dm.auth + 160 + e[1] + D.ENTRY_BITS, (1, e[0])
            rpc.update(is_hash=is_hash, h=h, e=e, bits=bits)
            tm.msgs += 2
            tm.bytes += D.nbytes(D.GETCALL_BITS) + D.nbytes(bits)

        def get_arrival(now, tm, rpc, on_response):
            respond(now, tm, rpc, on_response, D.wire_bytes(rpc["bits"]))

        def sizes(tm):
            c = {}
            for node, h, popped in tm.resp:
                if not popped:
                    c[h] = c.get(h, 0) + 1
            return c

        def majority(tm):
            best, cnt = None, 0
            for h, c in sorted(sizes(tm).items()):
                if c > cnt:
                    best, cnt = h, c
            return best, cnt

        def pop_back(tm, h):
            for r in reversed(tm.resp):
                if r[1] == h and not r[2]:
                    r[2] = True
                    return r[0]
            raise AssertionError

        def get_done(tm, outcome, now, e=None, node=D.NONE):
            o = tm.o
            o["num_responses"], o["messages"], o["bytes"] = tm.nresp, tm.msgs, tm.bytes
            if e is not None:
                o["result_count"], o["value_token"], o["value_len"] = 1, e[0], e[1]
            o["server"] = node if outcome == D.SUCCESS else D.NONE
            finish(tm, outcome, now)

        def value_or_fail(tm, now, mark):
            if tm.chosen is not None and sizes(tm).get(tm.chosen, 0) > 0:
                get_send(tm, pop_back(tm, tm.chosen), False, now)
                if mark:
                    tm.value_sent = True
            else:
                get_done(tm, D.FAILED, now)

        def get_timeout(now, tm, rpc):                        # DHT.cc:184-294
            if tm.value_sent:                                 # 198-221
                value_or_fail(tm, now, False)
            elif tm.replica:                                  # 226-240
                get_send(tm, tm.replica.pop(), True, now)
            else:
                if tm.nresp > 0:                              # 243-259
                    tm.chosen = majority(tm)[0]
                value_or_fail(tm, now, False)                 # 268-290: the state stays

        def get_response(now, tm, rpc):
            if tm.value_sent and not rpc["is_hash"]:          # DHT.cc:585-598
                return get_done(tm, D.SUCCESS, now, rpc["e"], rpc["target"])
            if rpc["is_hash"]:                                # DHT.cc:601-684
                tm.resp.append([rpc["target"], rpc["h"], False])
                tm.nresp += 1
                if tm.value_sent:
                    return                                    # 617-620
                hv, cnt = majority(tm)
                if cnt / tm.m >= Dm.ratio:                    # 635-637
                    tm.chosen = hv
                elif tm.nresp >= Dm.G:                        # 638
                    if tm.replica:                            # 640-653
                        get_send(tm, tm.replica.pop(), True, now)
                    elif hv is None:                          # 654-678
                        return get_done(tm, D.FAILED, now)
                    else:                                     # 679-682
                        tm.chosen = hv
            if not tm.value_sent and tm.chosen is not None:   # DHT.cc:686-714
                value_or_fail(tm, now, True)

        # ---- t0: every team's LookupCall in team order
        for tm in teams:
            if not is_put:
                tm.o["server"] = D.NONE
            sib, nxt = ring.decide(S, tm.key)
            tm.visited.add(S)
            if sib:
                lookup_ok(tm, [(S + x) % n for x in range(self.m)], t0)
            else:
                find_node(tm, nxt, t0)
        while heap:
            now, _, fn, a = heapq.heappop(heap)
            fn(now, *a)
        assert len(order) == self.T, "a team ran out of events before it completed"
        return [tm.o for tm in teams], order[0]

    # ------------------------------------------------------------ batches
    def _batch(self, keys, src, ops, is_put):
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        n = len(src)
        dtype = D.PUT_DTYPE if is_put else D.GET_DTYPE
        out, team, win = np.zeros(n, dtype=dtype), np.zeros((n, self.T), dtype=dtype), np.zeros(n, dtype=np.int32)
        writes = []
        for i in range(n):
            recs, w = self._run(i, keys[i], int(src[i]), ops[i], is_put, writes)
            for j, o in enumerate(recs):
                team[i, j] = o
            out[i], win[i] = team[i, w], w
        # every replica handles its calls in arrival order (DHT.cc:399-419); ties by operation, then team
        Dm = self.D
        for a, i, j, r, ek, token, vlen, ttl in sorted(writes, key=lambda w: (w[0], w[1], w[2])):
            d = Dm.store.setdefault(r, {})
            d.pop(ek, None)
            if vlen > 0:
                Dm.order += 1
                d[ek] = [token, vlen, a + ttl * 10**9 if ttl > 0 else D.NEVER, Dm.order]
        return out, team, win

    def put_batch(self, keys, src, ops):
        return self._batch(keys, src, ops, True)

    def get_batch(self, keys, src, ops):
        return self._batch(keys, src, ops, False)


def team_stats(nnodes, put_out, put_team, put_src, get_out, get_team, get_ops, get_src, expect, measured_time_s) -> dict:
    """ovs_dhttest_team_stats_batch: outcomes, latencies and per-node rates from the out records; the hop-count
    vectors (one sample per team with a valid lookup) and normalMessages / numBytesNormal from the team records."""
    st = D.dhttest_stats(nnodes, put_out, put_src, get_out, get_ops, get_src, expect, measured_time_s)
    for name, team in (("put", put_team), ("get", get_team)):
        t = np.asarray(team).reshape(-1)
        valid = t["outcome"] != D.LOOKUP_FAILED
        st[name + "_hop_count"] = int(valid.sum())
        st[name + "_hop_sum"] = int(t["hop_count"][valid].astype(np.int64).sum())
    allt = [np.asarray(put_team).reshape(-1), np.asarray(get_team).reshape(-1)]
    st["normal_messages"] = int(sum(t["messages"].astype(np.int64).sum() for t in allt))
    st["num_bytes_normal"] = int(sum(t["bytes"].astype(np.int64).sum() for t in allt))
    return st
