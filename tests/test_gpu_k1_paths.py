"""Every path of the converged-ring Chord route kernel (k_chord_lanes) against the CPU oracle.

The kernel decides its 160-bit ring compares on the top 64 bits of the distances and takes an exact
branch only on a tie, carries the arrival's coordinate delay to the finish, and writes each result
as one 16 B record.  These cases drive the branches that random keys on a large ring never take:
rings on both sides of the successor-list boundary (ns = min(8, n - 1): n = 2, 3, 9 run the general
instantiation, n = 10 and 1000 the one with successorListSize 8 / hopCountMax 50 folded in), node-ID
keys and their neighbours (exact ties, the "temp == K" finger rule, finishes at the source with no
route delay), and rings in which adjacent IDs share their top 64 bits, where every top-64 compare
ties.  Every field of every lookup must equal the oracle's.
"""
from __future__ import annotations

import numpy as np
import pytest

from oversim_amd import KbrEngine, Params, workload as W
from oversim_amd.kbr import Network
from oracle_lib import OracleNet, chord_params

pytestmark = pytest.mark.gpu
FIELDS = ("responsible", "hops", "status", "one_way_hops", "latency_ns")
LFIELDS = ("num_siblings", "hops", "status", "is_valid", "latency_ns")
OK, TIMEOUT, RPC_TIMEOUT, HOPMAX = 0, 1, 2, 3
RINGS = [2, 3, 9, 10, 1000]
MOD = 1 << 160


def _eq(g: dict, r: dict, label: str, fields=FIELDS):
    for f in fields:
        x, y = np.asarray(g[f]).astype(np.int64), np.asarray(r[f]).astype(np.int64)
        bad = np.nonzero(x != y)[0]
        assert len(bad) == 0, f"{label}: {f} differs at {bad[:8]}: gpu={x[bad[:8]]} ref={y[bad[:8]]}"


def _ints(words: np.ndarray) -> list[int]:
    return [sum(int(w) << (32 * i) for i, w in enumerate(row)) for row in words]


def _words(vals) -> np.ndarray:
    return np.array([[(int(v) >> (32 * i)) & 0xFFFFFFFF for i in range(5)] for v in vals], dtype=np.uint32).reshape(-1, 5)


def _pairs(n: int, keys: np.ndarray, seed: int):
    """(key, source) pairs: every source for every key on the small rings, one random source per key
    (plus the key's own node and its neighbours as sources, for node-derived keys) on the large one."""
    if n <= 10:
        src = np.tile(np.arange(n, dtype=np.uint32), len(keys))
        return np.repeat(keys, n, axis=0), src
    rng = np.random.default_rng(seed)
    return keys, rng.integers(0, n, len(keys)).astype(np.uint32)


def _crafted(n: int, seed: int) -> Network:
    """A ring in which runs of adjacent IDs share their top 64 bits (words 3 and 4) and differ only
    below bit 96: the two smallest rings entirely, the others in runs of 2 to 5 nodes."""
    net = W.population(n, seed)
    ids = net.ids.copy()
    rng = np.random.default_rng(seed + 1)
    runs = [(0, n)] if n <= 3 else ([(1, 4), (6, 2)] if n <= 10 else
                                    [(int(s), int(k)) for s, k in zip(range(5, n - 10, 37), rng.integers(2, 6, n))])
    for s, k in runs:
        ids[s:s + k, 3:] = ids[s, 3:]
        low = sorted(set(_ints(np.concatenate([ids[s:s + k, :3], np.zeros((k, 2), np.uint32)], axis=1))))
        assert len(low) == k
        ids[s:s + k, :3] = _words(low)[:, :3]
    v = _ints(ids)
    assert all(a < b for a, b in zip(v, v[1:])), "crafted IDs must stay sorted and distinct"
    return Network(ids=ids, xy=net.xy)


def _between_keys(ids: np.ndarray, seed: int) -> np.ndarray:
    """Keys between adjacent IDs that share their top 64 bits: just above the lower one, just below
    the upper one, their midpoint and both IDs themselves."""
    v = _ints(ids)
    out = []
    for a, b in zip(v, v[1:] + v[:1]):
        if (a >> 96) == (b >> 96):
            out += [a, (a + 1) % MOD, (a + b) // 2, (b - 1) % MOD, b]
    # and the lowest and highest keys with a run's top 64 bits, which lie outside the run
    for t in sorted({x >> 96 for x in out}):
        out += [t << 96, (t << 96) | ((1 << 96) - 1)]
    return _words(out)


def _keys(family: str, net: Network, n: int, seed: int) -> np.ndarray:
    if family == "random":
        return W.random_keys(40 if n <= 10 else 4000, np.random.default_rng(seed))
    if family == "node_ids":
        return net.ids.copy()
    if family == "node_ids_pm1":
        v = _ints(net.ids)
        return _words([(x + 1) % MOD for x in v] + [(x - 1) % MOD for x in v])
    raise AssertionError(family)


def _route_case(engine: KbrEngine, net: Network, keys, src, label: str, **p):
    engine.set_params(Params.chord().replace(**p))
    engine.chord_load(net.ids, net.xy)
    o = OracleNet("chord", net.ids, net.xy, chord_params(**p))
    g, r = engine.lookup(keys, src), o.route(keys, src, record_hops=False)
    _eq(g, r, label)
    return r


@pytest.mark.parametrize("family", ["random", "node_ids", "node_ids_pm1"])
@pytest.mark.parametrize("n", RINGS)
def test_key_families(engine: KbrEngine, n, family):
    net = W.population(n, 700 + n)
    keys, src = _pairs(n, _keys(family, net, n, 710 + n), 720 + n)
    if n > 10 and family != "random":
        # the key's own node and both neighbours as sources too (R == S finishes, one-hop finishes)
        own = np.tile(np.arange(n, dtype=np.int64), len(keys) // n)
        keys = np.concatenate([keys, keys, keys, keys])
        src = np.concatenate([src, own.astype(np.uint32), ((own + 1) % n).astype(np.uint32), ((own - 1) % n).astype(np.uint32)])
    r = _route_case(engine, net, keys, src, f"n={n} {family}")
    assert (r["status"] == OK).all()
    if family == "node_ids":
        # finishes at the source carry no route delay
        at_src = r["responsible"] == src
        assert at_src.any() and (r["latency_ns"][at_src & (r["hops"] == 0)] == 0).all()


@pytest.mark.parametrize("n", RINGS)
def test_ids_sharing_their_top_64_bits(engine: KbrEngine, n):
    net = _crafted(n, 800 + n)
    bk = _between_keys(net.ids, 810 + n)
    assert len(bk) >= 5
    keys = np.concatenate([bk, net.ids, W.random_keys(20, np.random.default_rng(820 + n))])
    keys, src = _pairs(n, keys, 830 + n)
    if n > 10:
        # sources next to the runs: the window and sibling tests of the run's own members
        rng = np.random.default_rng(840 + n)
        near = (np.repeat(np.arange(5, n - 10, 37), 8) + rng.integers(-9, 6, 8 * len(range(5, n - 10, 37)))) % n
        k2 = bk[rng.integers(0, len(bk), len(near))]
        keys, src = np.concatenate([keys, k2]), np.concatenate([src, near.astype(np.uint32)])
    r = _route_case(engine, net, keys, src, f"crafted n={n}")
    assert (r["status"] == OK).all()


# ------------------------------------------------------------ the 1000-node ring's further rules

def _mixed(net: Network, m: int, seed: int):
    k1, s1 = W.lookups(net.ids, m // 2, seed, node_ids=True)
    k2, s2 = W.lookups(net.ids, m - m // 2, seed + 1, node_ids=False)
    return np.concatenate([k1, k2]), np.concatenate([s1, s2])


@pytest.fixture(scope="module")
def ring1000():
    net = W.population(1000, 900)
    keys, src = _mixed(net, 6000, 901)
    return net, keys, src


@pytest.mark.parametrize("rnd", [0, 1])
def test_simtime_round_rules(engine: KbrEngine, ring1000, rnd):
    net, keys, src = ring1000
    _route_case(engine, net, keys, src, f"simtimeRound={rnd}", simtimeRound=rnd)


def test_hop_limit(engine: KbrEngine, ring1000):
    net, keys, src = ring1000
    r = _route_case(engine, net, keys, src, "hopCountMax=3", hopCountMax=3)
    assert (r["status"] == HOPMAX).any() and (r["status"] == OK).any()


@pytest.mark.parametrize("lookup_timeout", [10.0, 3.0])
def test_rpc_and_lookup_timeouts(engine: KbrEngine, ring1000, lookup_timeout):
    """Coordinates spread over +-450: a coordinate delay reaches 0.75 s, so some RTT reaches
    rpcUdpTimeout (1.5 s); with lookupTimeout 3 s the timed-out call also ends past the lookup's
    own limit, and a run of slow answers passes it."""
    net, keys, src = ring1000
    xy = np.random.default_rng(902).uniform(-450.0, 450.0, size=net.xy.shape)
    wide = Network(ids=net.ids, xy=xy)
    r = _route_case(engine, wide, keys, src, f"wide coordinates, lookupTimeout={lookup_timeout}", lookupTimeout=lookup_timeout)
    assert (r["status"] == OK).any()
    if lookup_timeout == 10.0:
        assert (r["status"] == RPC_TIMEOUT).any()
    else:
        assert (r["status"] == TIMEOUT).any()


def test_recorded_hop_sequences(engine: KbrEngine, ring1000):
    net, keys, src = ring1000
    engine.set_params(Params.chord())
    engine.chord_load(net.ids, net.xy)
    g = engine.lookup(keys, src, record_hops=True)
    r = OracleNet("chord", net.ids, net.xy).route(keys, src, record_hops=True)
    _eq(g, r, "hop_seq request")
    assert np.array_equal(g["hop_seq"], r["hop_seq"])


@pytest.mark.parametrize("hcm", [50, 3])
def test_semi_recursive(engine: KbrEngine, ring1000, hcm):
    net, keys, src = ring1000
    r = _route_case(engine, net, keys, src, f"semi-recursive hopCountMax={hcm}", routingType=1, hopCountMax=hcm)
    assert (r["status"] == OK).any() and (hcm == 50 or (r["status"] != OK).any())


def test_lookup_call_batch(engine: KbrEngine, ring1000):
    net, keys, src = ring1000
    engine.set_params(Params.chord())
    engine.chord_load(net.ids, net.xy)
    g, r = engine.lookupCall(keys, src), OracleNet("chord", net.ids, net.xy).lookup_call(keys, src)
    _eq(g, r, "LookupCall batch", LFIELDS)
    assert np.array_equal(g["siblings"], r["siblings"])


def test_batch_with_dynamic_tail(engine: KbrEngine, ring1000):
    """2^18 lookups: the last 30 % is handed out in chunks from the launch's counter, and lanes are
    refilled from several chunks."""
    net = ring1000[0]
    keys, src = _mixed(net, 1 << 18, 903)
    _route_case(engine, net, keys, src, "2^18 lookups")
