"""The paths of Koorde's K3 (oversim_amd/csrc/koorde.hip) that random IDs on large rings with the
default list sizes never take, bit-exact against the CPU oracle on every field (responsible, hops,
status, one_way_hops, latency_ns, rpcs, hop_seq where requested).  The oracle and the Python
reading agree on all of these inputs first (tests/test_refmodel_koorde.py); the rings, key families
and the census come from tests/koorde_rings.py.

* List-walk form (no KoordeRec: successorListSize or deBruijnListSize above 16; on the 12-node ring
  only deBruijnListSize 32 selects it): state export, findNode chains, routes with and without a
  hop-sequence request (k_koorde_route<false, true> and <false, false>), k_koorde_find_node<false>.
* Record form on crafted rings (n = 17, 40, 1000; ns = 16): runs of adjacent IDs under one 128-bit
  prefix, so that distance codes tie with unequal values -- with a hop-sequence request
  (<true, true>), at the defaults (<true, false, true>, the DEF instantiation) and at shiftingBits 2
  (<true, false>); direct findNode calls steered into the runs (k_koorde_find_node<true>).
  The census (CPU-side facts only) shows that the tie fallbacks were reached.  Counts reached, per
  ring as (predecessor test, successor test, successor-list walk) ties over the lookups' first
  findNode, then the steered calls answered inside a run (shiftingBits 4 / 2):
  n = 17: (91, 90, 834) of 1513 lookups, steered 272 of 272 / 68 of 68;
  n = 40: (133, 132, 2009) of 4920, steered 168 of 400 / 59 of 100;
  n = 1000: (87, 306, 4626) of 9757, steered 149 of 912 / 61 of 228.
  The clustered IDs also make Koorde's de Bruijn walk revisit nodes: on n = 1000 the oracle ends 868
  lookups with NO_NEXT, 38 at the hop limit of 50 and 113 at the lookup timeout, so the visited
  list is scanned at every length up to 50.
* Tiny rings (n = 2, 3, 5, 17; the lists wrap the whole ring) and a 40-node ring holding the IDs 0
  and 2^160 - 1, keys 0, 2^160 - 1 and 2^159 among them.
* Finish statuses on a 1000-node ring: HOPMAX (hopCountMax 1 and 3), RPC_TIMEOUT and TIMEOUT (wide
  coordinates), both simtimeRound rules, and lookups of more than 16 responders without a
  hop-sequence request (the visited list's LDS part and its scratch part).
* hopCountMax = 0 is refused for Koorde and for explicit Chord tables: the hop list is their
  visited set and has hopCountMax entries.
"""
from __future__ import annotations

import numpy as np
import pytest

import koorde_rings as KR
from oversim_amd import KbrEngine, KbrError, Params, workload as W
from oversim_amd.kbr import KOORDE_EXT_DTYPE, Network
from oracle_lib import OracleNet, koorde_params

pytestmark = pytest.mark.gpu
FIELDS = ("responsible", "hops", "status", "one_way_hops", "latency_ns", "rpcs")
OK, TIMEOUT, RPC_TIMEOUT, HOPMAX = 0, 1, 2, 3
NONE = 0xFFFFFFFF


def _load(engine: KbrEngine, net: Network, **kw) -> OracleNet:
    engine.set_params(Params.koorde().replace(**kw))
    engine.koorde_load(net.ids, net.xy)
    return OracleNet("koorde", net.ids, net.xy, koorde_params(**kw))


def _same_state(engine: KbrEngine, o: OracleNet):
    for a, b in zip(engine.koorde_state(), o.koorde_state()):
        assert np.array_equal(a, b)


def _same_routes(engine: KbrEngine, o: OracleNet, keys, src, label: str, record=(True, False)) -> dict:
    r = o.route(keys, src, record_hops=True, count_rpcs=True)
    for rec in record:
        g = engine.lookup(keys, src, record_hops=rec, count_rpcs=True)
        for f in FIELDS:
            x, y = g[f].astype(np.int64), r[f].astype(np.int64)
            bad = np.nonzero(x != y)[0]
            assert len(bad) == 0, f"{label} record_hops={rec}: {f} differs at {bad[:8]}: gpu={x[bad[:8]]} ref={y[bad[:8]]}"
        if rec:
            assert np.array_equal(g["hop_seq"], r["hop_seq"]), f"{label}: hop_seq"
    return r


def _ext(m: int, rks=None, steps=None) -> np.ndarray:
    ext = np.zeros(m, dtype=KOORDE_EXT_DTYPE)
    ext["step"] = 1 if steps is None else steps
    if rks is not None:
        ext["has_route_key"] = 1
        ext["route_key"] = rks
    return ext


def _same_find_node(engine: KbrEngine, o: OracleNet, node, keys, ext, rounds: int = 1) -> list:
    """findNode at node[i] with ext[i] against the oracle: next hop, route key and step; with
    rounds > 1 each answer and the extension its response carries feed the next call."""
    ans = []
    for _ in range(rounds):
        nxt, ext_out = engine.koorde_find_node(node, keys, ext)
        ans = []
        for i in range(len(node)):
            h, rk, st = o.koorde_find_node(int(node[i]), keys[i], ext["route_key"][i] if ext["has_route_key"][i] else None,
                                           int(ext["step"][i]))
            ans.append(h)
            assert int(nxt[i]) == (NONE if h is None else h), i
            if h is None:
                continue
            assert int(ext_out["step"][i]) == st and bool(ext_out["has_route_key"][i]) == (rk is not None), i
            if rk is not None:
                assert np.array_equal(ext_out["route_key"][i], rk), i
        ok = nxt != NONE
        node = np.where(ok, nxt, node).astype(np.uint32)
        ext = np.where(ok, ext_out, ext)
    return ans


# ------------------------------------------------------------------ 1. the list-walk form

@pytest.fixture(scope="module")
def ring3000():
    net = W.population(3000, 30)
    assert KR.min_gap(net) >= 1 << 16          # shiftingBits 3 is used on it
    return net, KR.mixed_lookups(net, 6000, 31)


@pytest.mark.parametrize("variant", list(KR.LIST_WALK))
def test_list_walk_form(engine: KbrEngine, ring3000, variant):
    net, (keys, src) = ring3000
    kw = KR.LIST_WALK[variant]
    assert kw["successorListSize"] > 16 or kw["deBruijnListSize"] > 16      # koorde_build: no KoordeRec
    o = _load(engine, net, **kw)
    _same_state(engine, o)
    _same_routes(engine, o, keys, src, f"list walk {variant}")
    node, fk = KR.chain_inputs(net, 1000, 32)
    _same_find_node(engine, o, node, fk, _ext(len(node)), rounds=5)
    node, fk, rk, steps = KR.past_key_length_inputs(net, 1000, 33)
    assert None in _same_find_node(engine, o, node, fk, _ext(len(node), rk, steps))


def test_list_walk_form_on_a_12_node_ring(engine: KbrEngine):
    """n - 1 = 11 successors: only deBruijnListSize 32 keeps the record form away."""
    net = KR.tiny_ring(12, 34)
    o = _load(engine, net, deBruijnListSize=32)
    _same_state(engine, o)
    keys, src = KR.edge_lookups(net, 35)
    _same_routes(engine, o, keys, src, "n=12 deBruijnListSize=32")
    _same_find_node(engine, o, src, keys, _ext(len(src)), rounds=3)


# ------------------------------------------------------------------ 2., 3. crafted rings, census

@pytest.mark.parametrize("sb", [4, 2])
@pytest.mark.parametrize("n", [17, 40, 1000])
def test_code_ties_on_crafted_rings(engine: KbrEngine, n, sb):
    net, runs = KR.crafted_ring(n, 50 + n)
    o = _load(engine, net, shiftingBits=sb)
    assert o.params.successorListSize == 16 and min(16, n - 1) == 16        # the record form, ns = 16
    _same_state(engine, o)
    keys, src = KR.crafted_lookups(net, runs, 60 + n)
    assert len(keys) <= 10_000
    c = KR.census(net, 16, src, keys)
    assert min(c.values()) > 0, c
    # sb 4: hop sequences (<true, true>) and the defaults (DEF); sb 2: <true, true> and <true, false>
    _same_routes(engine, o, keys, src, f"crafted n={n} shiftingBits={sb}")
    node, sk, rk, steps = KR.steered_calls(net, runs, sb)
    assert 0 < len(node) <= 2000
    ans = _same_find_node(engine, o, node, sk, _ext(len(node), rk, steps))
    _, st, num = o.koorde_state()
    assert KR.steered_census(net, runs, ans, st, num, node) > 0


# ------------------------------------------------------------------ 4. tiny rings and wrap-around

@pytest.mark.parametrize("kw", [{}, dict(successorListSize=4, deBruijnListSize=4, shiftingBits=2)], ids=["default", "4_4_sb2"])
@pytest.mark.parametrize("n", [2, 3, 5, 17, "edge40"])
def test_tiny_rings_and_wrap_around(engine: KbrEngine, n, kw):
    net = KR.edge_ring() if n == "edge40" else KR.tiny_ring(n, 70 + n)
    o = _load(engine, net, **kw)
    _same_state(engine, o)
    keys, src = KR.edge_lookups(net, 80)
    _same_routes(engine, o, keys, src, f"n={n} {kw}", record=(True,))


# ------------------------------------------------------------------ 5. finish statuses, parameters

@pytest.fixture(scope="module")
def ring1000():
    net = W.population(1000, 90)
    return net, KR.mixed_lookups(net, 6000, 91)


@pytest.mark.parametrize("hcm", [1, 3])
def test_hop_limit(engine: KbrEngine, ring1000, hcm):
    net, (keys, src) = ring1000
    r = _same_routes(engine, _load(engine, net, hopCountMax=hcm), keys, src, f"hopCountMax={hcm}")
    assert (r["status"] == HOPMAX).any() and (r["status"] == OK).any()


@pytest.mark.parametrize("rnd", [0, 1])
def test_simtime_round_rules(engine: KbrEngine, ring1000, rnd):
    net, (keys, src) = ring1000
    _same_routes(engine, _load(engine, net, simtimeRound=rnd), keys, src, f"simtimeRound={rnd}")


@pytest.mark.parametrize("lookup_timeout", [10.0, 3.0])
def test_rpc_and_lookup_timeouts(engine: KbrEngine, ring1000, lookup_timeout):
    """Coordinates spread over +-450: some RTT reaches rpcUdpTimeout (1.5 s); with lookupTimeout 3 s
    the timed-out call also ends past the lookup's own limit, and a run of slow answers passes it.
    rpcs counts the lost call."""
    net, (keys, src) = ring1000
    wide = Network(ids=net.ids, xy=np.random.default_rng(902).uniform(-450.0, 450.0, size=net.xy.shape))
    r = _same_routes(engine, _load(engine, wide, lookupTimeout=lookup_timeout), keys, src,
                     f"wide coordinates, lookupTimeout={lookup_timeout}")
    st = RPC_TIMEOUT if lookup_timeout == 10.0 else TIMEOUT
    assert (r["status"] == OK).any() and (r["status"] == st).any()
    assert (r["rpcs"][r["status"] == st] == r["hops"][r["status"] == st] + 1).all()


def test_long_lookups_without_a_hop_sequence_request(engine: KbrEngine, ring1000):
    """shiftingBits 1: lookups of more than KVL = 16 responders keep the first 16 in LDS and the
    later ones in scratch; the visitOnlyOnce scan reads both."""
    net, (keys, src) = ring1000
    r = _same_routes(engine, _load(engine, net, shiftingBits=1), keys, src, "shiftingBits=1", record=(False,))
    assert (r["hops"] > 16).any()


# ------------------------------------------------------------------ 6. hopCountMax = 0

def test_koorde_refuses_hop_count_max_0(engine: KbrEngine, ring1000):
    net, (keys, src) = ring1000
    o = _load(engine, net)
    engine.set_params(Params.koorde().replace(hopCountMax=0))
    for rec in (False, True):
        with pytest.raises(KbrError, match="hopCountMax"):
            engine.lookup(keys[:100], src[:100], record_hops=rec)
    engine.set_params(Params.koorde().replace(hopCountMax=50))
    _same_routes(engine, o, keys[:1000], src[:1000], "after the refusal")


def test_explicit_chord_tables_refuse_hop_count_max_0(engine: KbrEngine):
    """The explicit-table Chord kernel scans the same hop list as its visited set."""
    n = 300
    net = W.population(n, 33)
    engine.set_params(Params.chord())
    engine.chord_load(net.ids, net.xy)
    fingers = engine.chord_fingers()
    pred = ((np.arange(n) - 1) % n).astype(np.uint32)
    succ = np.stack([(np.arange(n) + 1 + j) % n for j in range(8)], axis=1).astype(np.uint32)
    engine.chord_load_tables(net.ids, net.xy, pred, succ, np.full(n, 8, np.uint8), fingers, np.full(n, 160, np.uint8))
    keys, src = W.lookups(net.ids, 200, 34, node_ids=False)
    ok = engine.lookup(keys, src)
    engine.set_params(Params.chord().replace(hopCountMax=0))
    with pytest.raises(KbrError, match="hopCountMax"):
        engine.lookup(keys, src)
    with pytest.raises(KbrError, match="hopCountMax"):
        engine.lookupCall(keys, src, 4)
    engine.set_params(Params.chord())
    again = engine.lookup(keys, src)
    for f in FIELDS[:5]:
        assert np.array_equal(ok[f], again[f]), f
