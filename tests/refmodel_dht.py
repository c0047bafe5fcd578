"""Independent Python reading of the DHT tier (src/applications/dht/DHT.cc) -- test infrastructure only.

A message-level, time-ordered replay of batched DHT puts and gets on a stable network.  It never
calls the engine.  The LookupCall's sibling list, hop count and latency come from a `lookup`
callable (the CPU oracle's lookup_call, tests/oracle_lib.py); everything after the lookup -- the
replica RPCs through real transmit queues, their timeouts, the arrival-ordered put majority, the get's
hash / value state machine and the per-node storage with TTLs -- is computed here.

  put     DHT.cc:499-516 (LookupCall, numSiblings = numReplica), 832-897 (one DHTPutCall per sibling),
          298-428 (handlePutRequest), 553-575 (handlePutResponse), 157-183 (timeout)
  get     DHT.cc:518-535, 898-957 (hash requests to the first numGetRequests siblings), 430-497
          (handleGetRequest), 577-715 (handleGetResponse), 184-294 (timeout)
  storage DHTDataStorage.cc:155-243
  lengths DHTMessage.msg:30-41, CommonMessages.msg:28-76; a call to a TransportAddress leaves as a
          BaseAppDataMessage straight over UDP (BaseRpc.cc:173-272, BaseApp.cc:241-281, 564-570,
          BaseOverlay.cc:1310-1341), the response likewise (BaseApp.cc:572-611, BaseOverlay.cc:857-866)
  delay   SimpleNodeEntry.cc:155-195 (the sender's transmit queue), SimpleUDP.cc:320-345 (a message to
          the sending host itself: no delay and no queue)

A value is a 64-bit token plus a length in bytes.  The `hashes` map of DHT.cc is ordered by hash value;
here the order is UNSPECIFIED_VALUE (the empty hash) first, then ascending token.
"""
from __future__ import annotations

import math

import numpy as np

NONE = 0xFFFFFFFF
SUCCESS, FAILED, LOOKUP_FAILED = 0, 1, 2
NEVER = (1 << 63) - 1

BASEAPPDATA_BITS = 40      # BASEAPPDATA_L = TYPE_L + 2 * COMP_L (CommonMessages.msg:68)
UDP_IP_BYTES = 28          # SimpleUDP.cc:291
BASERPC_BITS = 256         # BASERPC_L = TYPE_L + NONCE_L + NODEHANDLE_L + TIER_L (CommonMessages.msg:69-70)
AUTHBLOCK_BITS = 800       # SIGNATURE_L + CERT_L + PUBKEY_L (CommonMessages.msg:45-47, 57)
ENTRY_BITS = 608           # KEY_L + KIND_L + ID_L + SEQNO_L + TTL_L + KEY_L + PUBKEY_L (DHTMessage.msg:30-37)
GETCALL_BITS = BASERPC_BITS + 160 + 32 + 32 + 1     # GETCALL_L: sizeof(bool) counts as one bit (DHTMessage.msg:38)
HASH_BITS = 20             # a SHA-1 BinaryValue: size() * sizeof(char) taken as bits (DHTMessage.msg:40)

OP_DTYPE = np.dtype([("t0_ns", "<i8"), ("token", "<u8"), ("kind", "<u4"), ("id", "<u4"), ("vlen", "<u4"),
                     ("ttl", "<i4")])
PUT_DTYPE = np.dtype([("latency_ns", "<i8"), ("bytes", "<u4"), ("hop_count", "<u2"), ("messages", "<u2"),
                      ("outcome", "u1"), ("status", "u1"), ("num_sent", "u1"), ("num_responses", "u1"),
                      ("pad", "u1", 4)])
GET_DTYPE = np.dtype([("latency_ns", "<i8"), ("bytes", "<u4"), ("hop_count", "<u2"), ("messages", "<u2"),
                      ("outcome", "u1"), ("status", "u1"), ("num_sent", "u1"), ("num_responses", "u1"),
                      ("result_count", "<u4"), ("value_token", "<u8"), ("value_len", "<u4"), ("server", "<u4")])
DUMP_DTYPE = np.dtype([("key", "<u4", 5), ("kind", "<u4"), ("id", "<u4"), ("vlen", "<u4"), ("token", "<u8"),
                       ("expiry_ns", "<i8")])
PUT_FIELDS = tuple(f for f in PUT_DTYPE.names if f != "pad")
GET_FIELDS = GET_DTYPE.names


def simtime(seconds: float, rnd: bool) -> int:
    """SimTime(double) at scale 1e-9: round half up, or truncate."""
    x = seconds * 1e9
    return math.floor(x + 0.5) if rnd else int(x)


def nbytes(bits: int) -> int:
    """cPacket::getByteLength(): (bits + 7) / 8."""
    return (bits + 7) // 8


def wire_bytes(bits: int) -> int:
    """The UDP packet of a DHT message in its BaseAppDataMessage: the lengths add up in bits."""
    return nbytes(UDP_IP_BYTES * 8 + BASEAPPDATA_BITS + bits)


class DhtModel:
    def __init__(self, xy, lookup, rnd=True, num_replica=4, num_get_requests=4, ratio_identical=0.5,
                 rpc_udp_timeout=1.5, datarate=10e6, access=0.0, auth=False):
        self.xy, self.lookup, self.rnd = xy, lookup, bool(rnd)
        self.R, self.G, self.ratio = num_replica, num_get_requests, ratio_identical
        self.to = simtime(rpc_udp_timeout, self.rnd)
        self.datarate, self.acc = datarate, simtime(access, self.rnd)
        self.auth = AUTHBLOCK_BITS if auth else 0
        self.store: dict[int, dict] = {}         # node -> {(key bytes, kind, id): [token, vlen, expiry, order]}
        self.order = 0
        self.queue_measured = 0                  # operations whose source queue was measured idle at lookup completion

    def start_queue(self, look, i, S: int, t0: int, t: int) -> dict:
        """The transmit queues at lookup completion.  A lookup that replays its own messages (chord_measured_lookup)
        reports the source's tx.finished; it must not lie beyond the completion time, or the DHT's first message
        would wait behind a FindNodeCall."""
        if "src_tx_finished" not in look:
            return {}
        fin = t0 + int(look["src_tx_finished"][i])
        assert fin <= t, ("the source's transmit queue is busy at lookup completion", i, fin, t)
        self.queue_measured += 1
        return {S: fin}

    # ------------------------------------------------------------ underlay
    def send(self, txq: dict, a: int, b: int, wire: int, now: int) -> int:
        """Arrival time of a `wire`-byte packet sent by a to b at `now` (SimpleNodeEntry.cc:164-194)."""
        if a == b:
            return now                                        # SimpleUDP.cc:322
        bw = simtime((wire * 8) / self.datarate, self.rnd)
        fin = max(txq.get(a, 0), now) + bw                    # the send queue, SimpleNodeEntry.cc:166, 183
        txq[a] = fin
        dx = float(self.xy[a][0]) - float(self.xy[b][0])
        dy = float(self.xy[a][1]) - float(self.xy[b][1])
        dist = float(np.float32(math.sqrt(dx * dx + dy * dy)))
        return now + (fin - now) + self.acc + simtime(0.001 * dist, self.rnd) + bw + self.acc

    # ------------------------------------------------------------ storage
    def entry(self, node: int, ek, now: int):
        """The entry a replica holds at `now`: a TTL timer due at or before `now` has removed it."""
        e = self.store.get(node, {}).get(ek)
        return e if e is not None and e[2] > now else None

    def dump(self, node: int, now: int) -> np.ndarray:
        live = sorted((e[3], ek, e) for ek, e in self.store.get(node, {}).items() if e[2] > now)
        out = np.zeros(len(live), dtype=DUMP_DTYPE)
        for o, (_, ek, e) in zip(out, live):
            o["key"], o["kind"], o["id"] = np.frombuffer(ek[0], dtype=np.uint32), ek[1], ek[2]
            o["token"], o["vlen"], o["expiry_ns"] = e[0], e[1], e[2]
        return out

    def count(self) -> int:
        return sum(len(d) for d in self.store.values())

    # ------------------------------------------------------------ put
    def put_batch(self, keys, src, ops) -> np.ndarray:
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        look = self.lookup(keys, np.asarray(src, dtype=np.uint32))
        out = np.zeros(len(src), dtype=PUT_DTYPE)
        writes = []
        for i in range(len(src)):
            o, op, S = out[i], ops[i], int(src[i])
            o["status"] = look["status"][i]
            m = int(look["num_siblings"][i])
            if not look["is_valid"][i] or m == 0:             # DHT.cc:852-864
                o["outcome"], o["latency_ns"] = LOOKUP_FAILED, -1
                continue
            o["hop_count"] = look["hops"][i]                  # DHT.cc:866-867
            t = int(op["t0_ns"]) + int(look["latency_ns"][i])
            vlen = int(op["vlen"])
            call_bits = BASERPC_BITS + self.auth + vlen + ENTRY_BITS          # PUTCALL_L
            resp_bits = BASERPC_BITS + self.auth + 8                          # PUTRESPONSE_L
            ek = (keys[i].tobytes(), int(op["kind"]), int(op["id"]))
            txq, events = self.start_queue(look, i, S, int(op["t0_ns"]), t), []
            for j in range(m):                                # DHT.cc:876-891, back to back
                r = int(look["siblings"][i][j])
                a = self.send(txq, S, r, wire_bytes(call_bits), t)
                writes.append((a, i, r, ek, int(op["token"]), vlen, int(op["ttl"])))
                back = self.send(txq, r, S, wire_bytes(resp_bits), a)
                # the timeout was scheduled when the call was sent (BaseRpc.cc:257-258): it precedes a
                # response of the same instant
                events.append((t + self.to, j, "T") if back - t >= self.to else (back, j, "R"))
            o["num_sent"], o["messages"] = m, 2 * m
            o["bytes"] = m * (nbytes(call_bits) + nbytes(resp_bits))
            ok = bad = 0
            for when, _, what in sorted(events):
                if what == "R":
                    ok += 1                                   # DHT.cc:560-561
                    if ok / m > 0.5:                          # DHT.cc:568
                        o["outcome"] = SUCCESS
                        break
                else:
                    bad += 1                                  # DHT.cc:172
                    if bad / m >= 0.5:                        # DHT.cc:174
                        o["outcome"] = FAILED
                        break
            o["num_responses"], o["latency_ns"] = ok, when - int(op["t0_ns"])
        # every replica handles its calls in arrival order (DHT.cc:399-419); ties by operation index
        for a, i, r, ek, token, vlen, ttl in sorted(writes, key=lambda w: (w[0], w[1])):
            d = self.store.setdefault(r, {})
            d.pop(ek, None)                                   # removeData
            if vlen > 0:
                self.order += 1
                d[ek] = [token, vlen, a + ttl * 10**9 if ttl > 0 else NEVER, self.order]
        return out

    # ------------------------------------------------------------ get
    def get_batch(self, keys, src, ops) -> np.ndarray:
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        look = self.lookup(keys, np.asarray(src, dtype=np.uint32))
        out = np.zeros(len(src), dtype=GET_DTYPE)
        for i in range(len(src)):
            o, op = out[i], ops[i]
            o["status"], o["server"] = look["status"][i], NONE
            m = int(look["num_siblings"][i])
            if not look["is_valid"][i] or m == 0:             # DHT.cc:910-927
                o["outcome"], o["latency_ns"] = LOOKUP_FAILED, -1
                continue
            o["hop_count"] = look["hops"][i]                  # DHT.cc:929-930
            ek = (keys[i].tobytes(), int(op["kind"]), int(op["id"]))
            t = int(op["t0_ns"]) + int(look["latency_ns"][i])
            self.get_one(o, int(src[i]), [int(x) for x in look["siblings"][i][:m]], t, ek,
                         self.start_queue(look, i, int(src[i]), int(op["t0_ns"]), t))
            o["latency_ns"] += int(look["latency_ns"][i])
        return out

    def get_one(self, o, S: int, sibs: list, t: int, ek, txq=None):
        txq, rpcs, pending = ({} if txq is None else txq), [], []
        replica = sibs[self.G:]                               # DHT.cc:947-950
        resp = []                                             # hash responses in arrival order: [node, hash, popped]
        st = dict(value_sent=False, chosen=None, nresp=0, msgs=0, bytes=0)

        def send(target, is_hash, now):
            a = self.send(txq, S, target, wire_bytes(GETCALL_BITS), now)
            e = self.entry(target, ek, a)                     # DHT.cc:441-443
            if e is None:                                     # DHT.cc:462-464
                bits, h = BASERPC_BITS + self.auth + 160, (0, 0)
            elif is_hash:                                     # DHT.cc:466-481
                bits, h = BASERPC_BITS + self.auth + 160 + HASH_BITS, (1, e[0])
            else:                                             # DHT.cc:483-487; RESULT_L
                bits, h = BASERPC_BITS + self.auth + 160 + e[1] + ENTRY_BITS, (1, e[0])
            back = self.send(txq, target, S, wire_bytes(bits), a)
            st["msgs"] += 2
            st["bytes"] += nbytes(GETCALL_BITS) + nbytes(bits)
            k = len(rpcs)
            rpcs.append((target, is_hash, h, e))
            pending.append((now + self.to, k, "T") if back - now >= self.to else (back, k, "R"))

        def sizes():
            c = {}
            for node, h, popped in resp:
                if not popped:
                    c[h] = c.get(h, 0) + 1
            return c

        def majority():
            """The first hash in map order with the strictly largest vector (DHT.cc:244-254, 623-633)."""
            best, cnt = None, 0
            for h, c in sorted(sizes().items()):
                if c > cnt:
                    best, cnt = h, c
            return best, cnt

        def pop_back(h):
            for r in reversed(resp):
                if r[1] == h and not r[2]:
                    r[2] = True
                    return r[0]
            raise AssertionError

        def done(outcome, now, e=None, node=NONE):
            o["outcome"], o["latency_ns"] = outcome, now - t
            o["num_responses"], o["messages"], o["bytes"] = st["nresp"], st["msgs"], st["bytes"]
            if e is not None:
                o["result_count"], o["value_token"], o["value_len"] = 1, e[0], e[1]
            if outcome == SUCCESS:
                o["server"] = node

        for r in sibs[:self.G]:                               # DHT.cc:934-946
            send(r, True, t)
        o["num_sent"] = min(len(sibs), self.G)
        navail = len(sibs)                                    # DHT.cc:953
        while pending:
            pending.sort()
            now, k, what = pending.pop(0)                     # arrival order, ties by send order
            target, is_hash, h, e = rpcs[k]
            if what == "T":                                   # DHT.cc:184-294
                if st["value_sent"]:
                    if st["chosen"] is not None and sizes().get(st["chosen"], 0) > 0:     # 198-212
                        send(pop_back(st["chosen"]), False, now)
                    else:                                     # 213-221
                        return done(FAILED, now)
                elif replica:                                 # 226-240
                    send(replica.pop(), True, now)
                else:
                    if st["nresp"] > 0:                       # 243-259
                        st["chosen"] = majority()[0]
                    if st["chosen"] is not None and sizes().get(st["chosen"], 0) > 0:     # 268-282: the state stays
                        send(pop_back(st["chosen"]), False, now)
                    else:                                     # 283-290
                        return done(FAILED, now)
                continue
            if st["value_sent"] and not is_hash:              # DHT.cc:585-598: also with an empty result array
                return done(SUCCESS, now, e, target)
            hv = None
            if is_hash:                                       # DHT.cc:601-684
                resp.append([target, h, False])
                st["nresp"] += 1
                if st["value_sent"]:
                    continue                                  # 617-620
                hv, cnt = majority()
                if cnt / navail >= self.ratio:                # 635-637
                    st["chosen"] = hv
                elif st["nresp"] >= self.G:                   # 638
                    if replica:                               # 640-653
                        send(replica.pop(), True, now)
                    elif hv is None:                          # 654-678
                        return done(FAILED, now)
                    else:                                     # 679-682
                        st["chosen"] = hv
            if not st["value_sent"] and st["chosen"] is not None:            # DHT.cc:686-714
                if sizes().get(st["chosen"], 0) > 0:
                    send(pop_back(st["chosen"]), False, now)
                    st["value_sent"] = True
                else:
                    return done(FAILED, now)
        raise AssertionError("a get ran out of events before it completed")


def oracle_lookup(net, num_replica: int):
    """LookupCalls with numSiblings = numReplica from the CPU oracle (tests/oracle_lib.OracleNet)."""
    def lookup(keys, src):
        return net.lookup_call(keys, src, num_replica)
    return lookup


def chord_measured_lookup(ring, num_replica: int, rnd: bool = True, rpc_udp_timeout=1.5, lookup_timeout=10.0,
                          hop_max=50, datarate=10e6, auth=False):
    """LookupCalls on a converged Chord ring (refmodel.ChordRing.decide) replayed message by message through real
    transmit queues: every FindNodeCall (83 B) leaves through the source's queue and every FindNodeResponse
    (61 B + 26 B per NodeHandle, + 100 B with measureAuthBlock) through the responder's
    (IterativeLookup.cc:803-921, 1067-1170; SimpleNodeEntry.cc:164-194).  Besides the oracle's fields it returns
    src_tx_finished: the source's tx.finished when the lookup completes, relative to its start."""
    import refmodel
    n, xy = ring.n, ring.xy
    to, lk = simtime(rpc_udp_timeout, rnd), simtime(lookup_timeout, rnd)
    m = min(num_replica, 1 + ring.ns)
    base = 61 + (100 if auth else 0)

    def hop(txq, a, b, nb, now):
        bw = simtime((nb * 8) / datarate, rnd)
        fin = max(txq.get(a, 0), now) + bw
        txq[a] = fin
        return fin + refmodel.coord_ns(xy, a, b, rnd) + bw

    def one(k, S):
        sib, nxt = ring.decide(S, k)
        if sib:
            return [(S + j) % n for j in range(m)], 0, 0, 0, 0
        t, hops, visited, cur, txq = 0, 0, {S}, nxt, {}
        while True:
            sib, nxt = ring.decide(cur, k)
            back = hop(txq, cur, S, base + 26 * (m if sib else 1), hop(txq, S, cur, 83, t))
            if back - t >= to:
                return [], hops, (1 if t + to > lk else 2), -1, txq.get(S, 0)
            t = back
            if t > lk:
                return [], hops, 1, -1, txq.get(S, 0)
            hops += 1
            visited.add(cur)
            if sib:
                return [(cur + j) % n for j in range(m)], hops, 0, t, txq.get(S, 0)
            if hop_max and hops >= hop_max:
                return [], hops, 3, -1, txq.get(S, 0)
            if nxt in visited:
                return [], hops, 4, -1, txq.get(S, 0)
            cur = nxt

    def lookup(keys, src):
        rows = [one(refmodel.to_int(k), int(s)) for k, s in zip(keys, src)]
        sibs = np.full((len(rows), max(num_replica, 1)), NONE, dtype=np.uint32)
        for i, r in enumerate(rows):
            sibs[i, :len(r[0])] = r[0]
        return dict(siblings=sibs, num_siblings=np.array([len(r[0]) for r in rows], dtype=np.uint32),
                    hops=np.array([r[1] for r in rows], dtype=np.uint16), status=np.array([r[2] for r in rows], dtype=np.uint8),
                    is_valid=np.array([r[2] == 0 for r in rows], dtype=np.uint8),
                    latency_ns=np.array([r[3] for r in rows], dtype=np.int64),
                    src_tx_finished=np.array([r[4] for r in rows], dtype=np.int64))
    return lookup


# ---------------------------------------------------------------- DHTTestApp statistics
EXPECT_DTYPE = np.dtype([("token", "<u8"), ("endtime_ns", "<i8"), ("known", "<u4"), ("pad", "<u4")])
MIN_MEASURED = 0.1         # GlobalStatistics.cc:32
STAT_INTS = ("num_put_success", "num_put_error", "num_get_success", "num_get_error", "put_latency_sum_ns",
             "put_latency_sumsq_lo", "put_latency_sumsq_hi", "get_latency_sum_ns", "get_latency_sumsq_lo",
             "get_latency_sumsq_hi", "put_latency_min_ns", "put_latency_max_ns", "get_latency_min_ns",
             "get_latency_max_ns", "get_latency_count", "put_hop_count", "put_hop_sum", "get_hop_count", "get_hop_sum",
             "normal_messages", "num_bytes_normal")
STAT_SDS = ("put_latency_s", "get_latency_s", "put_success_per_s", "put_error_per_s", "get_success_per_s",
            "get_error_per_s", "get_success_ratio")


def cstddev(vals) -> dict:
    """cStdDev (OMNeT++ 4.x): count, mean, sample standard deviation, min, max."""
    n = len(vals)
    if n == 0:
        return {"count": 0, "mean": 0.0, "stddev": 0.0, "min": 0.0, "max": 0.0}
    s = math.fsum(vals)
    sq = math.fsum(v * v for v in vals)
    var = (sq - s * s / n) / (n - 1) if n > 1 else 0.0
    return {"count": n, "mean": s / n, "stddev": math.sqrt(max(var, 0.0)), "min": min(vals), "max": max(vals)}


def dhttest_stats(nnodes, put_out, put_src, get_out, get_ops, get_src, expect, measured_time_s) -> dict:
    """DHTTestApp::handlePutResponse / handleGetResponse (DHTTestApp.cc:147-234) over the two batches, finishApp
    (439-467) over the nodes, and the DHT's normalMessages / numBytesNormal and hop-count vectors."""
    cnt = [[0] * nnodes for _ in range(4)]
    plat, glat = [], []
    st = dict.fromkeys(STAT_INTS, 0)
    for o, s in zip(put_out, put_src):
        st["normal_messages"] += int(o["messages"])
        st["num_bytes_normal"] += int(o["bytes"])
        if o["outcome"] != LOOKUP_FAILED:                       # DHT.cc:866-867
            st["put_hop_count"] += 1
            st["put_hop_sum"] += int(o["hop_count"])
        if o["outcome"] == SUCCESS:                             # DHTTestApp.cc:161-164
            plat.append(int(o["latency_ns"]))
            cnt[0][int(s)] += 1
        else:                                                   # 165-167
            cnt[1][int(s)] += 1
    for o, op, s, e in zip(get_out, get_ops, get_src, expect):
        st["normal_messages"] += int(o["messages"])
        st["num_bytes_normal"] += int(o["bytes"])
        if o["outcome"] != LOOKUP_FAILED:                       # DHT.cc:929-930
            st["get_hop_count"] += 1
            st["get_hop_sum"] += int(o["hop_count"])
        if o["latency_ns"] >= 0:                                # DHTTestApp.cc:182-183
            glat.append(int(o["latency_ns"]))
        ok = False
        if o["outcome"] == SUCCESS:                             # 185-190
            now = int(op["t0_ns"]) + int(o["latency_ns"])
            if not e["known"]:                                  # 194-200
                ok = False
            elif now > int(e["endtime_ns"]):                    # 202-216
                ok = int(o["result_count"]) == 0
            else:                                               # 219-231
                ok = int(o["result_count"]) > 0 and int(o["value_token"]) == int(e["token"])
        cnt[2 if ok else 3][int(s)] += 1
    st["num_put_success"], st["num_put_error"] = sum(cnt[0]), sum(cnt[1])
    st["num_get_success"], st["num_get_error"] = sum(cnt[2]), sum(cnt[3])
    for name, lat in (("put", plat), ("get", glat)):
        sq = sum(v * v for v in lat)
        st[name + "_latency_sum_ns"] = sum(lat)
        st[name + "_latency_sumsq_lo"], st[name + "_latency_sumsq_hi"] = sq & (2**64 - 1), sq >> 64
        st[name + "_latency_min_ns"], st[name + "_latency_max_ns"] = min(lat, default=0), max(lat, default=0)
        st[name + "_latency_s"] = cstddev([v * 1e-9 for v in lat])
    st["get_latency_count"] = len(glat)
    T = measured_time_s
    on = T >= MIN_MEASURED
    for k, name in enumerate(("put_success_per_s", "put_error_per_s", "get_success_per_s", "get_error_per_s")):
        st[name] = cstddev([c / T for c in cnt[k]] if on else [])
    st["get_success_ratio"] = cstddev([a / (a + b) for a, b in zip(cnt[2], cnt[3]) if a + b > 0] if on else [])
    return st


def make_ops(n, t0_ns=0, token=0, kind=1, id=1, vlen=0, ttl=0) -> np.ndarray:
    ops = np.zeros(n, dtype=OP_DTYPE)
    for f, v in (("t0_ns", t0_ns), ("token", token), ("kind", kind), ("id", id), ("vlen", vlen), ("ttl", ttl)):
        ops[f] = v
    return ops
