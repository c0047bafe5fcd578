"""Rings, key families and the code census shared by the Koorde path tests (CPU:
tests/test_refmodel_koorde.py; GPU: tests/test_gpu_koorde_paths.py).  Not a conftest: both import it.

K3's record form (oversim_amd/csrc/koorde.hip) decides every ring compare on a 32-bit code of the
distance -- msb + 1 in the top byte, the 24 bits below the msb -- and reads the exact keys only when
two codes are equal.  Random IDs never tie, so the crafted rings here put runs of adjacent IDs under
one 128-bit prefix, their low words spaced so that some in-run distances are below 2^24 (codes
exact) and others are at or above 2^26 and differ only below the 24-bit mantissa (codes equal,
values unequal).  `census` counts, from the IDs alone, how often the first findNode of a lookup (or
a direct findNode call) meets such a tie in the predecessor test, the successor test and the
successor-list walk; it reads nothing the kernel reports.

Undefined corner, kept out of every ring here: findStartKey runs
`while ((160 - nBits) % shiftingBits != 0) nBits--` from nBits = msb(successor gap).  When
shiftingBits does not divide 160 (3, 6, 7, ...) and the gap is tiny, nBits goes negative and the
shifts that follow are undefined in the reference, the oracle and the kernel alike.  So a ring that
is used with such a shiftingBits keeps every adjacent gap at or above 2^16 (`min_gap`), and gaps of
exactly 1 (the crafted runs, the ring holding 0 and 2^160 - 1) are used only with shiftingBits in
{1, 2, 4, 5, 8}.
"""
from __future__ import annotations

import bisect

import numpy as np

from oversim_amd import workload as W
from oversim_amd.kbr import Network

MOD = 1 << 160
SAFE_SB = (1, 2, 4, 5, 8)          # the shiftingBits values that divide 160: nBits never goes below 0
# gaps between consecutive run members, cycled: below 2^24 (exact codes) and at or above 2^26 with
# low bits that the 24-bit mantissa drops
RUN_GAPS = (1, (1 << 26) + 1, 3, (1 << 26) + 2, (1 << 12) + 1, (1 << 27) + 3, 2, (1 << 26) + 5)
# (first node, length) of the runs; every ring has one run longer than 16: a whole successor list ties
RUNS = {17: [(0, 17)], 40: [(2, 18), (24, 5), (33, 2)],
        1000: [(60, 18), (200, 20), (350, 2), (500, 5), (650, 9), (800, 3)]}


def ints(words) -> list[int]:
    return [sum(int(w) << (32 * i) for i, w in enumerate(row)) for row in np.asarray(words).reshape(-1, 5)]


def words(vals) -> np.ndarray:
    return np.array([[(int(v) >> (32 * i)) & 0xFFFFFFFF for i in range(5)] for v in vals],
                    dtype=np.uint32).reshape(-1, 5)


def code32(v: int) -> int:
    """The kernel's distance code: 0 for 0, else msb + 1 in the top byte and the 24 bits below the msb."""
    if v == 0:
        return 0
    m = v.bit_length() - 1
    mant = (v >> (m - 24)) if m >= 24 else (v << (24 - m))
    return ((m + 1) << 24) | (mant & 0xFFFFFF)


def min_gap(net: Network) -> int:
    v = ints(net.ids)
    return min((b - a) % MOD for a, b in zip(v, v[1:] + v[:1]))


def crafted_ring(n: int, seed: int):
    """(ring, runs): a random population in which each run of RUNS[n] takes the first member's top
    128 bits and low words spaced by RUN_GAPS; runs = lists of node indices."""
    net = W.population(n, seed)
    ids = net.ids.copy()
    rng = np.random.default_rng(seed + 1)
    runs = []
    for s, k in RUNS[n]:
        low = int(rng.integers(1, 1 << 28))
        for j in range(k):
            ids[s + j, 1:] = ids[s, 1:]
            ids[s + j, 0] = low
            low += RUN_GAPS[j % len(RUN_GAPS)]
        assert low < (1 << 32)
        runs.append(list(range(s, s + k)))
    v = ints(ids)
    assert all(a < b for a, b in zip(v, v[1:])), "crafted IDs must stay sorted and distinct"
    return Network(ids=ids, xy=net.xy), runs


def crafted_keys(net: Network, runs, seed: int):
    """[(key, run index or None)]: every run member, member +- 1, the midpoints of adjacent members,
    the lowest and highest 160-bit values under each run's 128-bit prefix, and 20 random keys."""
    v = ints(net.ids)
    out = []
    for r, run in enumerate(runs):
        m = [v[i] for i in run]
        ks = list(m) + [(x + 1) % MOD for x in m] + [(x - 1) % MOD for x in m]
        ks += [(a + b) // 2 for a, b in zip(m, m[1:])]
        ks += [(m[0] >> 32) << 32, m[0] | 0xFFFFFFFF]
        out += [(k, r) for k in ks]
    out += [(k, None) for k in ints(W.random_keys(20, np.random.default_rng(seed)))]
    return out


def crafted_lookups(net: Network, runs, seed: int):
    """(keys, src) of a crafted ring: every node as the source of every key on the small rings; on
    n = 1000 each run's keys from its members and the 20 nodes before it, every key from 2 random
    nodes, and the random keys from every run member."""
    n = len(net.ids)
    kr = crafted_keys(net, runs, seed)
    rng = np.random.default_rng(seed + 1)
    keys, src = [], []
    for k, r in kr:
        if n <= 40:
            s = list(range(n))
        else:
            s = [int(x) for x in rng.integers(0, n, 2)]
            for run in (runs if r is None else [runs[r]]):
                s += run
                if r is not None:
                    s += [(run[0] - j) % n for j in range(1, 21)]
        keys += [k] * len(s)
        src += s
    return words(keys), np.array(src, dtype=np.uint32)


def steered_calls(net: Network, runs, sb: int):
    """Direct findNode calls whose de Bruijn step lands in a run: for a run member t and every
    j < 2^sb, the route key rk = (t >> sb) | (j << (160 - sb)) at the node c with rk in (c, succ(c)],
    looking up key t.  The step shifts rk left by sb and adds sb bits of t: with step = 161 - sb the
    low bits (the route key becomes t itself), with step = 1 the top bits (within 2^sb of t).
    Returns (node, keys, route keys, steps)."""
    v = ints(net.ids)
    n = len(v)
    node, keys, rks, steps = [], [], [], []
    for run in runs:
        for i in run:
            t = v[i]
            for j in range(1 << sb):
                rk = (t >> sb) | (j << (160 - sb))
                c = (bisect.bisect_left(v, rk) - 1) % n          # rk in (c, succ(c)], wrapping
                if rk == v[c]:
                    continue
                node.append(c); keys.append(t); rks.append(rk); steps.append(161 - sb if j % 2 == 0 else 1)
    return np.array(node, dtype=np.uint32), words(keys), words(rks), np.array(steps, dtype=np.int32)


def census(net: Network, sls: int, node, keys, use_other: bool = True) -> dict:
    """How many findNode calls (node[i], keys[i]) meet equal codes of unequal distances: in the
    predecessor test (key - .. - me against pred - .. - me), in the successor test, reached when the
    key is not in (pred, me], and in the successor-list walk, reached when it is not in (me, succ0]
    either.  The exact order decides which tests are reached; nothing here comes from the kernel."""
    v = ints(net.ids)
    n = len(v)
    ns = min(sls, n - 1)
    cnt = dict(pred=0, succ=0, walk=0)
    for c, k in zip([int(x) for x in node], ints(keys)):
        me = v[c]
        dp, dk = (me - v[(c - 1) % n]) % MOD, (me - k) % MOD
        cnt["pred"] += code32(dk) == code32(dp) and dk != dp
        if dk < dp:                                   # key in (pred, me]
            continue
        d, ds = (k - me) % MOD, (v[(c + 1) % n] - me) % MOD
        cnt["succ"] += code32(d) == code32(ds) and d != ds
        if d <= ds or not use_other:                  # key in (me, succ0]
            continue
        sj = [(v[(c + 1 + j) % n] - me) % MOD for j in range(1, ns)]
        cnt["walk"] += any(code32(x) == code32(d) and x != d for x in sj)
    return cnt


def steered_census(net: Network, runs, answers, db_start, db_num, node) -> int:
    """Steered calls (answers = the oracle's next hops) that end at a run member other than the last
    node of the responder's de Bruijn list: decided inside the list, among the tying codes."""
    n = len(net.ids)
    members = {i for run in runs for i in run}
    last = [(int(db_start[c]) + int(db_num[c]) - 1) % n for c in node]
    return sum(1 for h, l in zip(answers, last) if h is not None and h in members and h != l)


def tiny_ring(n: int, seed: int) -> Network:
    return W.population(n, seed)


def edge_ring(seed: int = 40) -> Network:
    """40 nodes whose IDs include 0 and 2^160 - 1 (adjacent across the wrap: a gap of 1)."""
    net = W.population(40, seed)
    ids = net.ids.copy()
    ids[0] = 0
    ids[-1] = 0xFFFFFFFF
    return Network(ids=ids, xy=net.xy)


def edge_lookups(net: Network, seed: int):
    """Every (key, source) pair over: all IDs, IDs +- 1, 0, 2^160 - 1, 2^159 and 10 random keys."""
    v = ints(net.ids)
    n = len(v)
    ks = v + [(x + 1) % MOD for x in v] + [(x - 1) % MOD for x in v] + [0, MOD - 1, 1 << 159]
    ks += ints(W.random_keys(10, np.random.default_rng(seed)))
    return np.repeat(words(ks), n, axis=0), np.tile(np.arange(n, dtype=np.uint32), len(ks))


def mixed_lookups(net: Network, m: int, seed: int):
    k1, s1 = W.lookups(net.ids, m // 2, seed, node_ids=True)
    k2, s2 = W.lookups(net.ids, m - m // 2, seed + 1, node_ids=False)
    return np.concatenate([k1, k2]), np.concatenate([s1, s2])


def chain_inputs(net: Network, m: int, seed: int):
    """findNode chain inputs as test_find_node_chains_match_oracle: random nodes; half random keys,
    half node IDs."""
    rng = np.random.default_rng(seed)
    n = len(net.ids)
    node = rng.integers(0, n, m).astype(np.uint32)
    keys = np.concatenate([W.random_keys(m // 2, rng), net.ids[rng.integers(0, n, m - m // 2)]])
    return node, keys


def past_key_length_inputs(net: Network, m: int, seed: int):
    """Extensions with steps around the key length, half of the route keys just after the node's
    own key -- inside (node, succ0], where the de Bruijn step reads key bits: past bit 0 it throws."""
    rng = np.random.default_rng(seed)
    n = len(net.ids)
    node = rng.integers(0, n, m).astype(np.uint32)
    keys = W.random_keys(m, rng)
    steps = rng.integers(150, 170, m).astype(np.int32)
    rk = net.ids[rng.integers(0, n, m)].copy()
    own = words([(x + 1) % MOD for x in ints(net.ids[node])])
    half = rng.random(m) < 0.5
    rk[half] = own[half]
    return node, keys, rk, steps


# the list-walk form: (successorListSize, deBruijnListSize) above the record's 16, with further
# parameters; shiftingBits 3 only on the random 3000-node ring (gaps far above 2^16)
LIST_WALK = {
    "17_16": dict(successorListSize=17, deBruijnListSize=16),
    "16_17": dict(successorListSize=16, deBruijnListSize=17),
    "40_64": dict(successorListSize=40, deBruijnListSize=64),
    "200_255": dict(successorListSize=200, deBruijnListSize=255),
    "17_16_sb2": dict(successorListSize=17, deBruijnListSize=16, shiftingBits=2),
    "16_17_sb8": dict(successorListSize=16, deBruijnListSize=17, shiftingBits=8),
    "40_64_sb1": dict(successorListSize=40, deBruijnListSize=64, shiftingBits=1),
    "200_255_sb3": dict(successorListSize=200, deBruijnListSize=255, shiftingBits=3),
    "40_64_no_other": dict(successorListSize=40, deBruijnListSize=64, useOtherLookup=0),
    "200_255_no_suc": dict(successorListSize=200, deBruijnListSize=255, useSucList=0),
}
