"""Crafted Broose networks, key families and the path census shared by the Broose deep tests (CPU:
tests/test_broose_model.py; GPU: tests/test_gpu_broose_deep.py).  Not a conftest: both import it.

Uniform ids of a small network differ within their top 10 to 20 bits, so every 160-bit compare, split bit and
shift of oversim_amd/csrc/broose.hip is decided in the top word.  The rings here put runs of ids under one
(160 - low_bits)-bit prefix: inside a run the XOR distances tie in their top 64 bits, the trie descent of the
snapshot build splits below bit low_bits, rBucket[0] / rBucket[1] of a run member hold run members only (so
longestPrefix, and with it the distance estimate, goes up to 160 - low_bits and beyond 31), and the bBucket range
distance of a run member lies below 2^low_bits.  `census` counts, from the model and the ids alone, how often each
of these is met; it reads nothing the engine reports.

Every model here is built with build="add" (BrooseBucket::add in a shuffled order); the trie descent
(build="fast") restates the kernel's method and serves only as the third party in the CPU comparison.
"""
from __future__ import annotations

import functools
import random

import numpy as np

from oversim_amd import workload as W
from oversim_amd.kbr import Network
import refmodel_broose as RB

M = 1 << 160
LOW_BITS = (96, 64, 40, 33, 32, 31, 5)
# name -> (n, runs, per, low_bits, seed): every low_bits value, both sizes
RUN_RINGS = {
    "lb96": (160, 4, 20, 96, 71), "lb64": (48, 2, 12, 64, 72), "lb40": (160, 4, 20, 40, 73), "lb33": (48, 2, 12, 33, 74),
    "lb32": (160, 4, 20, 32, 75), "lb31": (48, 2, 12, 31, 76), "lb5": (160, 4, 20, 5, 77),
}
RINGS = tuple(RUN_RINGS) + ("edge",)
PAIR_RINGS = ("pair2", "pair3")
DEFAULT_SHAPE = (8, 8, 2, 0)
# (bucketSize, rBucketSize, shiftingBits, userDist)
SHAPES = ((3, 5, 2, 0), (1, 1, 1, 0), (8, 4, 4, 0), (5, 16, 2, 2), (8, 16, 2, 0), (8, 8, 3, 2))
SHAPE_RING = "lb40"                 # the clustered ring every bucket shape runs on
PAIR_SHAPES = tuple((1, 8, sb, ud) for sb in (2, 3) for ud in (0, 2))


def words(vals) -> np.ndarray:
    return np.array([[(int(v) >> (32 * i)) & 0xFFFFFFFF for i in range(5)] for v in vals], dtype=np.uint32).reshape(-1, 5)


def _network(vals, seed) -> Network:
    vals = sorted(set(vals))
    return Network(ids=words(vals), xy=W.coordinates(len(vals), seed))


def run_ring(n: int, runs: int, per: int, low_bits: int, seed: int):
    """(network, runs, feeders): `runs` runs of `per` ids that share all but their low `low_bits` bits, 12 feeders and
    uniform ids for the rest; runs = lists of node indices.  The first two members of a run differ in bit
    low_bits - 1, so the run splits exactly below its prefix.  The first run's prefix starts with four zero bits
    and, for each shiftingBits sb of 1..4, three feeders have the id (member << sb) + sb random low bits: their
    rBucket[0] key (id >> sb) is a run member, the bucket holds run members only, longestPrefix is at least
    160 - low_bits and the distance estimate above 31.  Which other nodes' rBucket keys fall into a run is chance."""
    rnd = random.Random(seed)
    vals, members = set(), []
    for r in range(runs):
        prefix = rnd.getrandbits(160 - low_bits - (4 if r == 0 else 0)) << low_bits
        top = 1 << (low_bits - 1)
        low = {rnd.getrandbits(low_bits - 1), top | rnd.getrandbits(low_bits - 1)}
        while len(low) < per:
            low.add(rnd.getrandbits(low_bits))
        members.append([prefix | x for x in sorted(low)])
        vals.update(members[-1])
    assert len(vals) == runs * per
    feed = []
    for sb in (1, 2, 3, 4):
        for _ in range(3):
            x = next(x for x in iter(lambda: ((rnd.choice(members[0]) << sb) | rnd.getrandbits(sb)) % M, None) if x not in vals)
            feed.append(x)
            vals.add(x)
    assert len(vals) == runs * per + len(feed) <= n
    while len(vals) < n:
        vals.add(rnd.getrandbits(160))
    net = _network(vals, seed)
    pos = {v: i for i, v in enumerate(sorted(vals))}
    return net, [sorted(pos[x] for x in mem) for mem in members], sorted(pos[x] for x in feed)


def edge_ring(seed: int = 78):
    """48 ids that include 0 and 2^160 - 1 and one run of 12 straddling 2^159: six ids just below it, six at and just
    above, so the run's members differ in bit 159 and below bit 8 and nowhere between."""
    rnd = random.Random(seed)
    lows = rnd.sample(range(1, 200), 5)
    run = [(1 << 159) - x for x in rnd.sample(range(1, 200), 6)] + [1 << 159] + [(1 << 159) + x for x in lows]
    vals = {0, M - 1, *run}
    while len(vals) < 48:
        vals.add(rnd.getrandbits(160))
    net = _network(vals, seed)
    pos = {v: i for i, v in enumerate(sorted(vals))}
    return net, [sorted(pos[x] for x in run)], []


def pair_ring(n: int, seed: int = 79):
    """n = 2: the ids X and X ^ 1, so every rBucket holds both, longestPrefix = 159 and the raw distance estimate is
    160 + userDist.  n = 3: X ^ 2 as well (a uniform third id would be the farthest entry of every bucket and end
    the shared prefix in the top bits): X ^ 2 is the closest or the farthest of the three and longestPrefix is 158.  With bucketSize >= n every key is a sibling's
    (keyInRange: size <= maxSize / 7) and findNode never estimates a distance, so the pair rings are loaded with
    bucketSize = 1, where only a node's own key is."""
    rnd = random.Random(seed + n)
    x = rnd.getrandbits(160) & ~1
    x &= ~3
    vals = {x, x ^ 1} | ({x ^ 2} if n == 3 else set())
    net = _network(vals, seed)
    pos = {v: i for i, v in enumerate(sorted(vals))}
    return net, [sorted((pos[x], pos[x ^ 1]))], []


@functools.lru_cache(maxsize=None)
def ring(name: str):
    if name in RUN_RINGS:
        return run_ring(*RUN_RINGS[name])
    if name == "edge":
        return edge_ring()
    return pair_ring(int(name[4:]))


def low_bits_of(name: str) -> int:
    """the number of low bits inside which a run's members differ (edge: 8, beside the top bit)"""
    return RUN_RINGS[name][3] if name in RUN_RINGS else (8 if name == "edge" else 1)


@functools.lru_cache(maxsize=None)
def model(name: str, shape=DEFAULT_SHAPE, build: str = "add") -> RB.BrooseNet:
    net = ring(name)[0]
    k, kr, sb, ud = shape
    return RB.BrooseNet(net.ids, net.xy, bucket_size=k, r_bucket_size=kr, user_dist=ud, shifting_bits=sb, build=build,
                        seed=len(name) + k + kr)


def range_edge_keys(m: RB.BrooseNet, v: int) -> list[int]:
    """the keys at which Broose::isSiblingFor(v, key) turns: key ^ ids[v] equal to the bBucket range distance
    getDist(maxSize / 7 - 1), one above (no sibling) and one below"""
    dist = m.b_bucket(v).dist
    if len(dist) <= m.k:
        return []
    d = dist[m.k - 1]
    return [m.ids[v] ^ x for x in (d, d + 1, d - 1) if 0 <= x < M]


def lookups(name: str, m: RB.BrooseNet, nq: int, seed: int):
    """(keys (nq, 5), src, right) over the key families: uniform keys, node ids, a node id XOR a value below
    2^low_bits (inside a run when the node is a run member), node ids +- 1, and the three range-edge keys of run
    members.  Half of the sources are run members, a quarter feeders, and a run-family key is looked up from its own run."""
    net, runs, feed = ring(name)
    rnd = random.Random(seed)
    lb = low_bits_of(name)
    members = [i for run in runs for i in run]
    keys, src = [], []
    for i in range(nq):
        fam = i % 8
        v = rnd.choice(members) if fam >= 2 else rnd.randrange(m.n)
        s = rnd.choice(members) if i % 2 else (rnd.choice(feed) if feed and i % 4 == 2 else rnd.randrange(m.n))
        if fam == 0:
            k = rnd.getrandbits(160)
        elif fam == 1:
            k = m.ids[v]
        elif fam in (2, 3, 4):
            k = m.ids[v] ^ rnd.getrandbits(lb)
            s = rnd.choice(next(run for run in runs if v in run)) if fam != 4 else s
        elif fam == 5:
            k = (m.ids[v] + rnd.choice((1, -1))) % M
        else:
            edge = range_edge_keys(m, v)
            k = rnd.choice(edge) if edge else m.ids[v]
            s = v if fam == 6 else s
        keys.append(k)
        src.append(s)
    right = np.array([rnd.randrange(2) for _ in range(nq)], dtype=np.uint8)
    return words(keys), np.array(src, dtype=np.uint32), right


def timeout_between(m: RB.BrooseNet) -> float:
    """an rpcUdpTimeout between the smallest and the largest FindNodeCall round trip of the network (the model's own
    delays, IterativeLookup's rtt of a call and a one-node response): the median over all pairs, in seconds"""
    rnd = m.rnd
    fixed = RB.msg_ns(RB.call_bytes(), rnd) + RB.msg_ns(RB.resp_bytes(1), rnd)
    rtt = sorted(fixed + 2 * RB.coord_ns(m.xy, a, b, rnd) for a in range(m.n) for b in range(a + 1, m.n))
    t = round(rtt[len(rtt) // 2] / 1e9, 3)           # whole milliseconds: no round trip equals it to the nanosecond
    assert rtt[0] < t * 1e9 < rtt[-1]
    return t


def _top(x: int, bits: int) -> int:
    return x >> (160 - bits)


def census(m: RB.BrooseNet, keys, src, right, **kw) -> dict:
    """What the lookups (keys, src, right) on model m meet, from the model alone:

    tie_rows      rows with two adjacent entries whose distances to the bucket key agree in their top 64 bits (the
                  `k_lt` fallback of the snapshot's insertion sort);
    split_lt      {128, 96, 64, 32} -> rows whose membership was decided by a split bit below that: the msb of
                  ids[farthest member] ^ ids[closest non-member], the last bit at which the trie descent divides a
                  range (rows that hold every node of the network have none);
    dist_gt31     nodes whose distance estimate is above 31; dist_hist: estimate -> nodes; dist_cap: nodes whose raw
                  estimate was above the key length and got capped;
    sib_top32     isSiblingFor decisions (at the source and at every responder of a route) in bBucket mode 0 where
                  key ^ me and the range distance agree in their top 32 bits; sib_eq / sib_above / sib_below: those
                  at equality and one off;
    status        route finishes by status; retries: first-hop timeouts after which a further candidate of the
                  source was tried; retries_low: those where the two candidates' distances agree in the top 32 bits."""
    ids, n = m.ids, m.n
    out = dict(tie_rows=0, split_lt={128: 0, 96: 0, 64: 0, 32: 0}, dist_gt31=0, dist_hist={}, dist_cap=0, sib_top32=0,
               sib_eq=0, sib_above=0, sib_below=0, status={}, retries=0, retries_low=0)
    for v in range(n):
        for b in m.buckets[v]:
            out["tie_rows"] += any(_top(x, 64) == _top(y, 64) for x, y in zip(b.dist, b.dist[1:]))
            if len(b.dist) < n:
                by_dist = sorted(range(n), key=lambda j: ids[j] ^ b.key)
                assert [b.node[d] for d in b.dist] == by_dist[:len(b.dist)]
                bit = (ids[by_dist[len(b.dist) - 1]] ^ ids[by_dist[len(b.dist)]]).bit_length() - 1
                for lim in out["split_lt"]:
                    out["split_lt"][lim] += bit < lim
        d = m.distance_estimate(v)
        out["dist_hist"][d] = out["dist_hist"].get(d, 0) + 1
        out["dist_gt31"] += d > RB.MAX_LEFT_DIST
        raw = max(m.r_bucket(v, 0).longest_prefix(ids), m.r_bucket(v, 1).longest_prefix(ids)) + 1 + m.user_dist
        out["dist_cap"] += raw + (-raw) % m.sb > RB.KEYLEN

    def sibling_decision(v, k):
        dist = m.b_bucket(v).dist
        if len(dist) <= m.k:
            return
        x, d = k ^ ids[v], dist[m.k - 1]
        out["sib_top32"] += _top(x, 32) == _top(d, 32)
        out["sib_eq"] += x == d
        out["sib_above"] += x == d + 1
        out["sib_below"] += x == d - 1

    for i in range(len(keys)):
        k, s = RB.to_int(keys[i]), int(src[i])
        r = m.lookup(k, s, bool(right[i]), **kw)
        out["status"][r["status"]] = out["status"].get(r["status"], 0) + 1
        for v in [s] + r["hop_seq"]:
            sibling_decision(v, k)
        if r["rpcs"] > r["hops"] + 1:       # two calls unanswered: only the first hop goes on after a timeout
            out["retries"] += 1
            # the source's candidates: its local findNode asked for bucketSize nodes of the scanned row
            msg = {}
            cands = m.find_node(s, k, m.k, 1, msg, bool(right[i]))
            e = msg["ext"]
            tgt = k if e.step == 0 else e.route_key
            out["retries_low"] += _top(ids[cands[0]] ^ tgt, 32) == _top(ids[cands[1]] ^ tgt, 32)
    return out


BIG_STEPS = (32, 33, 34, 64, 66, 96, 128, 159, 160)


def direct_calls(name: str, m: RB.BrooseNet, seed: int):
    """findNode calls (node, key, extension or None, direction) for broose_cases.find_node_calls(direct=...): run
    members asked for keys inside their run, first calls in both directions at every node whose distance estimate
    is above 31 (and at four others), mid-route right-shifting calls whose step is each of BIG_STEPS rounded down to
    a multiple of shiftingBits (the prefix bits are read at 160 - step: across every word boundary), and the three
    range-edge keys of run members."""
    net, runs, feed = ring(name)
    rnd = random.Random(seed)
    lb = low_bits_of(name)
    members = [i for run in runs for i in run]
    inside = lambda v: m.ids[v] ^ rnd.getrandbits(lb)
    out = []
    for v in members:
        out.append((v, inside(v), None, rnd.randrange(2)))
        for k in range_edge_keys(m, v):
            out.append((v, k, None, rnd.randrange(2)))
    far = [v for v in range(m.n) if m.distance_estimate(v) > RB.MAX_LEFT_DIST]
    for v in far + [rnd.randrange(m.n) for _ in range(4)]:
        for k in (m.ids[v] ^ (1 << 158), rnd.getrandbits(160), inside(rnd.choice(members))):
            out += [(v, k, None, 0), (v, k, None, 1)]
    for step in sorted({s - s % m.sb for s in BIG_STEPS}):
        for _ in range(6):
            v = rnd.choice(members + list(range(m.n)))
            rk = rnd.choice((rnd.getrandbits(160), m.ids[rnd.choice(members)] << m.sb & (M - 1), inside(rnd.choice(members))))
            k = rnd.choice((rnd.getrandbits(160), inside(rnd.choice(members))))
            out.append((v, k, RB.Ext(rk, step, True, rnd.randrange(m.n)), 1))
    return out


def key_pool(name: str, m: RB.BrooseNet, seed: int) -> list[int]:
    return [RB.to_int(k) for k in lookups(name, m, 256, seed)[0]]


NQ = 512


@functools.lru_cache(maxsize=None)
def batch(name: str, shape=DEFAULT_SHAPE):
    """the route batch of a ring and shape: (keys, src, right)"""
    return lookups(name, model(name, shape), NQ, 7 + len(name))


@functools.lru_cache(maxsize=None)
def census_of(name: str, shape=DEFAULT_SHAPE, timeout: bool = False, hop_max: int = 50) -> dict:
    m = model(name, shape)
    kw = dict(rpc_to=timeout_between(m)) if timeout else {}
    return census(m, *batch(name, shape), hop_max=hop_max, **kw)


def split_limit(name: str) -> int:
    """the word boundary at or above the ring's low_bits: rows of the ring must split below it"""
    return next(x for x in (32, 64, 96, 128) if x >= low_bits_of(name))
