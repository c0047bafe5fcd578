"""Pastry on the GPU (oversim_amd/csrc/pastry.hip) against the model (tests/refmodel_pastry.py): the converged tables
the device builds, explicit tables, BasePastry::findNode node for node with its flags, whole semi-recursive routes
bit for bit (responsible node, hops, hop sequence, status, int64 latency), the committed golden vectors, a large
ring checked by properties, and the refusals."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from oversim_amd import KbrEngine, KbrError, Params, PastryParams, workload as W
from oversim_amd.kbr import key_from_int
import refmodel_pastry as RP
from pastry_cases import assert_routes as _assert_routes, find_node_want as _find_node_want

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
NONE = 0xFFFFFFFF
FIELDS = ("responsible", "hops", "status", "one_way_hops", "latency_ns")
FN_CASES = [(1, 1), (3, 1), (8, 4), (16, 8)]


def _pp(**kw):
    return PastryParams.default(routeMsgAcks=0, **kw)


def _load(engine, n, seed=81, b=4, L=16, opt=0, reg=1, **pk):
    net = W.population(n, seed)
    engine.set_params(Params.pastry().replace(**pk))
    engine.pastry_load(net.ids, net.xy, _pp(bitsPerDigit=b, numberOfLeaves=L, optimizeLookup=opt, useRegularNextHop=reg))
    m = RP.PastryNet(net.ids, net.xy, b, L, bool(opt), bool(reg), rnd=bool(pk.get("simtimeRound", 1)))
    return net, m


def _batch(net, nq, seed):
    rng = np.random.default_rng(seed)
    keys = W.random_keys(nq, rng)
    keys[::4] = net.ids[rng.integers(0, len(net.ids), len(keys[::4]))]
    return keys, rng.integers(0, len(net.ids), nq).astype(np.uint32)


@pytest.mark.parametrize("n", [2, 3, 9, 17, 40, 1000])
@pytest.mark.parametrize("b", [1, 2, 4])
def test_export_equals_model_tables(engine: KbrEngine, n, b):
    net, m = _load(engine, n, b=b)
    leaf, tab = engine.pastry_export()
    wleaf, wtab = m.tables()
    assert np.array_equal(leaf, wleaf)
    assert tab.shape == wtab.shape and np.array_equal(tab, wtab)


def test_load_tables_round_trips(engine: KbrEngine):
    net, m = _load(engine, 1000)
    keys, src = _batch(net, 512, 82)
    ideal = engine.pastry_lookup(keys, src, record_hops=True)
    leaf, tab = engine.pastry_export()
    engine.pastry_load_tables(net.ids, net.xy, leaf, tab, _pp())
    l2, t2 = engine.pastry_export()
    assert np.array_equal(l2, leaf) and np.array_equal(t2, tab)
    again = engine.pastry_lookup(keys, src, record_hops=True)
    for f in ideal:
        assert np.array_equal(ideal[f], again[f]), f
    # malformed tables are refused and leave the loaded network as it is
    bad = tab.copy()
    bad[5, 0, 3] = 1000
    with pytest.raises(KbrError, match="EINVAL"):
        engine.pastry_load_tables(net.ids, net.xy, leaf, bad, _pp())
    bad = leaf.copy()
    bad[7, 8] = 7
    with pytest.raises(KbrError, match="EINVAL"):
        engine.pastry_load_tables(net.ids, net.xy, bad, tab, _pp())
    assert np.array_equal(engine.pastry_lookup(keys[:32], src[:32])["latency_ns"], ideal["latency_ns"][:32])


def test_find_node_golden_cases(engine: KbrEngine):
    g = np.load(GOLD / "pastry_n1000.npz")
    engine.set_params(Params.pastry())
    engine.pastry_load(g["ids"], g["xy"], _pp())
    for nr, ns in FN_CASES:
        out, cnt, sib, st = engine.pastry_find_node(g["fn_node"], g["fn_keys"], nr, ns, max_out=17)
        assert np.array_equal(st, g[f"fn_{nr}_{ns}_status"]), (nr, ns)
        assert np.array_equal(sib, g[f"fn_{nr}_{ns}_sib"]), (nr, ns)
        assert np.array_equal(cnt, g[f"fn_{nr}_{ns}_count"]), (nr, ns)
        assert np.array_equal(out, g[f"fn_{nr}_{ns}_nodes"]), (nr, ns)


@pytest.mark.parametrize("opt,reg", [(0, 1), (1, 1), (0, 0)])
def test_find_node_ring_of_9(engine: KbrEngine, opt, reg):
    """Every node of a ring of 9 (leaf sets half full) for node ids, keys beside them, the isCloser tie half-way
    between two ids and random keys; every numSiblings from 0, where a full vector is unlimited."""
    net, m = _load(engine, 9, L=8, opt=opt, reg=reg)
    ids = m.ids
    ks = list(ids) + [(k + 1) % RP.M for k in ids] + [(k - 1) % RP.M for k in ids]
    ks += [(ids[i] + ((ids[(i + 1) % 9] - ids[i]) % RP.M) // 2) % RP.M for i in range(9)]
    ks += [RP.to_int(k) for k in W.random_keys(16, np.random.default_rng(83))]
    node = np.repeat(np.arange(9, dtype=np.uint32), len(ks))
    keys = np.array([key_from_int(k) for k in ks] * 9, dtype=np.uint32)
    for nr, ns in [(1, 1), (1, 0), (3, 1), (8, 4), (4, 2), (2, 3)]:
        out, cnt, sib, st = engine.pastry_find_node(node, keys, nr, ns, max_out=10)
        wout, wcnt, wsib, wst = _find_node_want(m, node, keys, nr, ns, 10)
        assert np.array_equal(st, wst), (nr, ns)
        assert np.array_equal(sib, wsib), (nr, ns)
        assert np.array_equal(cnt, wcnt) and np.array_equal(out, wout), (nr, ns)


@pytest.mark.parametrize("rnd", [1, 0])
def test_lookup_equals_golden(engine: KbrEngine, rnd):
    g = np.load(GOLD / "pastry_n1000.npz")
    for rnr in (1, 3):
        engine.set_params(Params.pastry().replace(simtimeRound=rnd, recNumRedundantNodes=rnr))
        engine.pastry_load(g["ids"], g["xy"], _pp())
        got = engine.pastry_lookup(g["keys"], g["src"], record_hops=True)
        for f in FIELDS[:-1]:
            assert np.array_equal(got[f], g[f"r{rnr}_{f}"]), (rnr, f)
        assert np.array_equal(got["latency_ns"], g[f"r{rnr}_latency_ns" + ("" if rnd else "_trunc")]), rnr
        H = g[f"r{rnr}_hop_seq"].shape[1]
        assert np.array_equal(got["hop_seq"][:, :H], g[f"r{rnr}_hop_seq"]) and np.all(got["hop_seq"][:, H:] == NONE)


@pytest.mark.parametrize("kw", [dict(hopCountMax=3), dict(hopCountMax=0), dict(opt=1), dict(reg=0), dict(b=2, L=8),
                                dict(b=1, L=2, recNumRedundantNodes=2), dict(b=3, L=32, recNumRedundantNodes=8)])
def test_route_edge_cases(engine: KbrEngine, kw):
    kw = dict(kw)
    shape = {k: kw.pop(k) for k in ("b", "L", "opt", "reg") if k in kw}
    net, m = _load(engine, 1000, **shape, **kw)
    keys, src = _batch(net, 1024, 84)
    got = engine.pastry_lookup(keys, src, record_hops=True)
    want = RP.routes(m, keys, src, rec_num_redundant=kw.get("recNumRedundantNodes", 3), hop_max=kw.get("hopCountMax", 50))
    _assert_routes(got, want, str(kw))
    if "hopCountMax" in kw:
        assert (want["status"] == RP.HOPMAX).sum() > 0
        if kw["hopCountMax"] == 0:
            assert (want["status"] == RP.HOPMAX).all()


@pytest.mark.parametrize("n", [2, 3, 9])
def test_tiny_networks_every_pair(engine: KbrEngine, n):
    net, m = _load(engine, n)
    ids = m.ids
    fixed = [0, 1, RP.M - 1, 1 << 159, ids[0], ids[n - 1] + 1, (ids[0] + (ids[1] - ids[0]) // 2)]
    keys = np.array([key_from_int(k % RP.M) for k in fixed for _ in range(n)], dtype=np.uint32)
    src = np.array(list(range(n)) * len(fixed), dtype=np.uint32)
    _assert_routes(engine.pastry_lookup(keys, src, record_hops=True), RP.routes(m, keys, src), f"n={n}")


@pytest.mark.parametrize("opt", [0, 1])
def test_thinned_tables_take_the_closer_node_path(engine: KbrEngine, opt):
    net, m = _load(engine, 1000, opt=opt)
    leaf, tab = engine.pastry_export()
    rng = np.random.default_rng(85)
    thin = tab.copy()
    thin[rng.random(tab.shape) < 0.3] = NONE
    engine.pastry_load_tables(net.ids, net.xy, leaf, thin, _pp(optimizeLookup=opt))
    sm = RP.PastryNet(net.ids, net.xy, optimize=bool(opt), tables=(leaf, thin))
    keys, src = _batch(net, 1024, 86)
    for rnr in (1, 3):
        engine.set_params(Params.pastry().replace(recNumRedundantNodes=rnr))
        want = RP.routes(sm, keys, src, rec_num_redundant=rnr)
        _assert_routes(engine.pastry_lookup(keys, src, record_hops=True), want, f"thin rnr={rnr}")
    node = src[:512]
    out, cnt, sib, st = engine.pastry_find_node(node, keys[:512], 3, 1)
    wout, wcnt, wsib, wst = _find_node_want(sm, node, keys[:512], 3, 1, 4)
    assert np.array_equal(out, wout) and np.array_equal(cnt, wcnt) and np.array_equal(sib, wsib) and np.array_equal(st, wst)
    srcs = [sm.nodes[int(v)].find_node(RP.to_int(k), 1, 1)[1]["source"] for v, k in zip(node, keys[:512])]
    assert srcs.count("closer") > 20
    print("thinned: sources", {s: srcs.count(s) for s in set(srcs)}, "status",
          {int(s): int((want["status"] == s).sum()) for s in np.unique(want["status"])})


def test_large_ring_properties(engine: KbrEngine):
    n, nq = 1 << 16, 1 << 17
    net = W.population(n, 87)
    engine.set_params(Params.pastry())
    engine.pastry_load(net.ids, net.xy, _pp())
    rng = np.random.default_rng(88)
    keys = W.random_keys(nq, rng)
    src = rng.integers(0, n, nq).astype(np.uint32)
    r = engine.pastry_lookup(keys, src, record_hops=True)
    assert (r["hops"] <= 50).all() and (r["status"] == 0).mean() > 0.99
    ok = r["status"] == 0
    assert np.array_equal(r["hops"][ok], (r["hop_seq"][ok] != NONE).sum(axis=1))
    assert (r["latency_ns"][ok & (r["hops"] > 0)] > 0).all()
    m = RP.PastryNet(net.ids, net.xy, nodes=[])
    for i in rng.choice(nq, 2000, replace=False):
        if ok[i]:
            assert int(r["responsible"][i]) in m.owner(RP.to_int(keys[i])), i


def test_refusals_leave_the_context_usable(engine: KbrEngine):
    net, m = _load(engine, 1000)
    keys, src = _batch(net, 16, 89)
    base = engine.pastry_lookup(keys, src)

    def refused(fn, reload=None, match="ENOTSUP"):
        with pytest.raises(KbrError, match=match):
            fn()
        engine.set_params(Params.pastry())
        if reload:
            engine.pastry_load(net.ids, net.xy, _pp())
        assert np.array_equal(engine.pastry_lookup(keys, src)["latency_ns"], base["latency_ns"])

    for kw in (dict(routingType=0), dict(routingType=2), dict(routingType=4), dict(numSiblings=2), dict(recNumRedundantNodes=9)):
        engine.set_params(Params.pastry().replace(**kw))
        refused(lambda: engine.pastry_lookup(keys, src))
    # routeMsgAcks: the default, refused at the route with its name
    engine.pastry_load(net.ids, net.xy, PastryParams.default())
    refused(lambda: engine.pastry_lookup(keys, src), reload=True, match="routeMsgAcks")
    for bad in (dict(numberOfNeighbors=4), dict(bitsPerDigit=5), dict(bitsPerDigit=0), dict(numberOfLeaves=7), dict(numberOfLeaves=34)):
        refused(lambda: engine.pastry_load(net.ids, net.xy, _pp(**bad)), reload=True)
    with pytest.raises(KbrError, match="EINVAL"):
        engine.pastry_find_node(src, keys, 17, 1)
    with pytest.raises(KbrError, match="EINVAL"):
        engine.pastry_find_node(src, keys, 1, 9)
    # the generic calls
    refused(lambda: engine.lookup(keys, src), match="Pastry: ovs_pastry_route_batch")
    refused(lambda: engine.lookupCall(keys, src, 1), match="Pastry: ovs_pastry_route_batch")
    refused(lambda: engine.findNode(src, keys, 1, 1), match="Pastry: ovs_pastry_route_batch")
    refused(lambda: engine.rpcCall(keys, src), match="Pastry: ovs_pastry_route_batch")
