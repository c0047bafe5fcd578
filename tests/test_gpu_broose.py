"""Broose on the GPU (oversim_amd/csrc/broose.hip) against the model (tests/refmodel_broose.py): the snapshot the
device builds, Broose::findNode over every class of call, whole routes bit for bit (responsible node, hops, hop
sequence, status, int64 latency, FindNodeCall counts), explicit tables, the KBRTestApp statistics, the refusals
and the committed golden vectors."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from oversim_amd import DHT_OP_DTYPE, ROUTE_OUT_DTYPE, BrooseParams, KbrEngine, KbrError, Params, stats as S, workload as W
from oversim_amd.kbr import BROOSE_EXT_DTYPE, key_from_int, key_to_int
from oracle_lib import OracleNet
import broose_cases as BC
import refmodel_broose as RB

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
NONE = 0xFFFFFFFF


def _load(engine, n, sb=2, user_dist=0, **pk):
    net = BC.network(n)
    engine.set_params(Params.broose().replace(**pk))
    engine.broose_load(net.ids, net.xy, BrooseParams.default(shiftingBits=sb, userDist=user_dist))
    return net, BC.model(n, sb, user_dist)


@pytest.mark.parametrize("n", [2, 3, 9, 1000])
@pytest.mark.parametrize("sb", [1, 2, 3])
def test_export_equals_model_buckets(engine: KbrEngine, n, sb):
    net, m = _load(engine, n, sb)
    off, nodes = engine.broose_export()
    woff, wnodes = m.csr()
    assert np.array_equal(off, np.array(woff, dtype=np.uint64))
    assert np.array_equal(nodes, np.array(wnodes, dtype=np.uint32))
    if n <= 9:
        # buckets not full: n = 2, 3 take the size <= maxSize / 7 branch of keyInRange, n = 9 the getDist branch on a
        # bBucket of 9; longestPrefix from few entries
        assert all(len(m.b_bucket(v).dist) == n for v in range(n))


def test_find_node_batch_equals_model(engine: KbrEngine):
    net, m = _load(engine, 1000)
    calls = BC.find_node_calls(m, 4096, 43)
    classes = {c[4] for c in calls}
    for need in ("sibling", "first_left", "first_right", "mid_left", "mid_right", "brother", "loop"):
        assert need in classes, need
    node = np.array([c[0] for c in calls], dtype=np.uint32)
    keys = np.array([key_from_int(c[1]) for c in calls], dtype=np.uint32)
    ext = np.array([BC.ext_record(c[2]) for c in calls], dtype=BROOSE_EXT_DTYPE)
    right = np.array([c[3] for c in calls], dtype=np.uint8)
    out, cnt, sib, st, eo = engine.broose_find_node(node, keys, right, ext)
    for i, (v, k, e, r, cls, res, e2) in enumerate(calls):
        if cls == "broken":
            assert st[i] == 1 and cnt[i] == 0, i
            continue
        assert st[i] == 0 and cnt[i] == len(res) == 1 and int(out[i, 0]) == res[0], (i, cls)
        assert bool(sib[i]) == (cls == "sibling"), (i, cls)
        if e2 is not None:
            assert (key_to_int(eo["route_key"][i]), int(eo["step"][i]), bool(eo["right_shifting"][i])) == e2.tup(), (i, cls)
            assert eo["has_ext"][i] == 1
            if cls != "sibling":
                assert int(eo["last_node"][i]) == v
        else:
            assert eo["has_ext"][i] == 0
    # several nodes per answer: the source's local call asks for bucketSize nodes, a sibling answers numSiblings
    sel = np.arange(0, 4096, 9)
    out8, cnt8, sib8, st8, _ = engine.broose_find_node(node[sel], keys[sel], right[sel], ext[sel], numRedundantNodes=8,
                                                      numSiblings=4, max_out=8)
    for j, i in enumerate(sel):
        v, k, e, r, cls = calls[i][:5]
        if cls == "broken":
            continue
        res = m.find_node(v, k, 8, 4, {} if e is None else {"ext": e.copy()}, r)
        assert list(out8[j, :cnt8[j]]) == res and np.all(out8[j, cnt8[j]:] == NONE), (i, cls)
    # numSiblings = 0: the exact key
    ek = np.array([key_from_int(m.ids[int(v)]) for v in node[:64]] + list(keys[:64]), dtype=np.uint32)
    en = np.concatenate([node[:64], node[:64]])
    o0, c0, s0, t0, _ = engine.broose_find_node(en, ek, np.ones(128, np.uint8), None, numRedundantNodes=1, numSiblings=0)
    assert s0[:64].all() and np.array_equal(o0[:64, 0], node[:64])
    for j in range(64, 128):
        v, k = int(en[j]), key_to_int(ek[j])
        want_sib = m.ids[v] == k
        assert bool(s0[j]) == want_sib
        assert int(o0[j, 0]) == m.find_node(v, k, 1, 0, {}, True)[0]


@pytest.mark.parametrize("sb", [1, 2, 3])
@pytest.mark.parametrize("user_dist", [0, 2])
def test_routes_equal_model(engine: KbrEngine, sb, user_dist):
    rng = np.random.default_rng(44 + sb)
    nq = 2048
    keys = W.random_keys(nq, rng)
    net = BC.network(1000)
    keys[::16] = net.ids[rng.integers(0, 1000, len(keys[::16]))]      # node ids as keys too
    src = rng.integers(0, 1000, nq).astype(np.uint32)
    right = rng.integers(0, 2, nq).astype(np.uint8)
    # the four (rounding, measureAuthBlock) combinations, a quarter of the batch each
    for q, (rnd, auth) in enumerate([(1, 0), (0, 0), (1, 1), (0, 1)]):
        sl = slice(q * nq // 4, (q + 1) * nq // 4)
        _, m = _load(engine, 1000, sb, user_dist, simtimeRound=rnd, measureAuthBlock=auth)
        got = engine.broose_lookup(keys[sl], src[sl], right[sl], record_hops=True, count_rpcs=True)
        want = BC.model_routes(BC.with_rounding(m, bool(rnd)), keys[sl], src[sl], right[sl], auth=bool(auth))
        BC.assert_routes_equal(got, want, 50)
        assert (want["status"] == 0).sum() > 400


@pytest.mark.parametrize("n", [2, 3, 9])
def test_tiny_networks_every_pair(engine: KbrEngine, n):
    net, m = _load(engine, n)
    fixed = [0, 1, (1 << 160) - 1, 1 << 159, (1 << 159) - 1, 0x5555 << 140, key_to_int(net.ids[0]), key_to_int(net.ids[n - 1]) + 1]
    keys = np.array([key_from_int(k) for k in fixed for _ in range(n)] * 2, dtype=np.uint32)
    src = np.array(list(range(n)) * len(fixed) * 2, dtype=np.uint32)
    right = np.repeat([0, 1], n * len(fixed)).astype(np.uint8)
    got = engine.broose_lookup(keys, src, right, record_hops=True, count_rpcs=True)
    BC.assert_routes_equal(got, BC.model_routes(m, keys, src, right), 50)


def test_rpc_timeouts_and_hop_limit(engine: KbrEngine):
    rng = np.random.default_rng(46)
    nq = 1024
    keys, src = W.random_keys(nq, rng), rng.integers(0, 1000, nq).astype(np.uint32)
    right = rng.integers(0, 2, nq).astype(np.uint8)
    # rpcUdpTimeout below the larger round trips: some FindNodeCalls time out, and at the first hop the source's
    # further candidates are tried
    _, m = _load(engine, 1000, rpcUdpTimeout=0.12, lookupTimeout=0.9)
    got = engine.broose_lookup(keys, src, right, record_hops=True, count_rpcs=True)
    want = BC.model_routes(m, keys, src, right, rpc_to=0.12, lk_to=0.9)
    BC.assert_routes_equal(got, want, 50)
    assert (want["status"] == 2).sum() > 0 and (want["rpcs"] > want["hops"] + 1).sum() > 0
    print("timeouts:", {int(s): int((want["status"] == s).sum()) for s in np.unique(want["status"])})
    _, m = _load(engine, 1000, hopCountMax=3)
    got = engine.broose_lookup(keys, src, right, record_hops=True, count_rpcs=True)
    want = BC.model_routes(m, keys, src, right, hop_max=3)
    BC.assert_routes_equal(got, want, 3)
    assert (want["status"] == 3).sum() > 0


def test_explicit_tables(engine: KbrEngine):
    net, m = _load(engine, 1000)
    rng = np.random.default_rng(47)
    nq = 768
    keys, src = W.random_keys(nq, rng), rng.integers(0, 1000, nq).astype(np.uint32)
    right = rng.integers(0, 2, nq).astype(np.uint8)
    ideal = engine.broose_lookup(keys, src, right, record_hops=True)
    off, nodes = engine.broose_export()
    engine.broose_load_tables(net.ids, net.xy, off, nodes)
    again = engine.broose_lookup(keys, src, right, record_hops=True)
    for f in ideal:
        assert np.array_equal(ideal[f], again[f]), f
    o2, n2 = engine.broose_export()
    assert np.array_equal(o2, off) and np.array_equal(n2, nodes)
    # sparse tables: every second entry of each row dropped
    soff, snodes = [0], []
    for g in range(len(off) - 1):
        snodes.extend(nodes[int(off[g]):int(off[g + 1]):2])
        soff.append(len(snodes))
    engine.broose_load_tables(net.ids, net.xy, soff, snodes)
    sm = RB.BrooseNet(net.ids, net.xy, rows=(soff, snodes))
    got = engine.broose_lookup(keys, src, right, record_hops=True, count_rpcs=True)
    BC.assert_routes_equal(got, BC.model_routes(sm, keys, src, right), 50)
    # malformed tables are refused and leave the loaded network as it is
    bad = np.array(snodes, dtype=np.uint32)
    bad[5] = 1000
    with pytest.raises(KbrError, match="EINVAL"):
        engine.broose_load_tables(net.ids, net.xy, soff, bad)
    assert np.array_equal(engine.broose_lookup(keys[:32], src[:32], right[:32])["latency_ns"], got["latency_ns"][:32])


def test_statistics(engine: KbrEngine):
    net, m = _load(engine, 1000, hopCountMax=4)
    rng = np.random.default_rng(48)
    nq = 1024
    keys, src = W.random_keys(nq, rng), rng.integers(0, 1000, nq).astype(np.uint32)
    right = rng.integers(0, 2, nq).astype(np.uint8)
    want = BC.model_routes(m, keys, src, right, hop_max=4)
    assert 0 < (want["status"] == 0).sum() < nq
    # the reference statistics (the oracle's reading of KBRTestApp.cc:380-520) of the MODEL's records against the
    # device statistics of the device's records, as files: oversim_amd.stats writes both
    rec = np.zeros(nq, dtype=ROUTE_OUT_DTYPE)
    for f in BC.FIELDS:
        rec[f] = want[f] if f != "responsible" else want[f] & 0xFFFFFFFF
    ref = OracleNet("chord", net.ids, net.xy).kbrtest_stats({f: rec[f] for f in BC.FIELDS}, keys, src, 60.0, lookupNodeIds=True,
                                                            testMsgSize=100)
    st = engine.kbrtest_stats(engine.broose_lookup(keys, src, right), keys, src, 60.0, lookupNodeIds=True)
    got = S.summary(st)
    for f in ("num_sent", "num_delivered", "num_dropped", "num_lookup_failed", "hop_count_sum", "latency_sum_ns"):
        assert got[f] == ref[f], f
    assert got["num_sent"] == nq and got["num_delivered"] + got["num_dropped"] > 0
    assert got["num_delivered"] + got["num_dropped"] == (want["status"] == 0).sum()
    assert got["hop_count_mean"] == pytest.approx(ref["hop_count_mean"], rel=1e-15)
    assert got["latency_mean_s"] == pytest.approx(ref["latency_mean_s"], rel=1e-12)
    for f in ("delivered_msgs_per_s", "delivery_ratio"):
        for k in ("count", "mean", "stddev", "min", "max"):
            assert getattr(getattr(st, f), k) == pytest.approx(ref[f][k], rel=1e-12, abs=1e-15), (f, k)


def test_refusals_leave_the_context_usable(engine: KbrEngine):
    net, m = _load(engine, 1000)
    keys, src = W.random_keys(16, np.random.default_rng(49)), np.arange(16, dtype=np.uint32)
    right = np.zeros(16, np.uint8)
    base = engine.broose_lookup(keys, src, right)

    def refused(fn):
        with pytest.raises(KbrError, match="ENOTSUP"):
            fn()
        engine.set_params(Params.broose())
        assert np.array_equal(engine.broose_lookup(keys, src, right)["latency_ns"], base["latency_ns"])

    for kw in (dict(routingType=1), dict(routingType=2), dict(routingType=4), dict(hopCountMax=0), dict(numSiblings=2),
               dict(lookupParallelRpcs=2), dict(lookupRedundantNodes=2), dict(lookupMerge=1)):
        engine.set_params(Params.broose().replace(**kw))
        refused(lambda: engine.broose_lookup(keys, src, right))
    # the other overlays' calls and every application tier
    refused(lambda: engine.lookup(keys, src))
    refused(lambda: engine.lookupCall(keys, src, 1))
    refused(lambda: engine.findNode(src, keys, 1, 1))
    refused(lambda: engine.rpcCall(keys, src))
    refused(lambda: engine.chord_broadcast(src[:2]))
    engine.dht_store_create(1024)
    ops = np.zeros(16, dtype=DHT_OP_DTYPE)
    refused(lambda: engine.dht_put(keys, src, ops))
    refused(lambda: engine.scribe_build(keys[:2], np.zeros(4, np.uint32), src[:4]))
    # parameters outside the implemented ranges
    with pytest.raises(KbrError, match="ENOTSUP"):
        engine.broose_load(net.ids, net.xy, BrooseParams.default(shiftingBits=5))


def test_directions_helper(engine: KbrEngine):
    net, m = _load(engine, 1000)
    rng = np.random.default_rng(50)
    keys = W.random_keys(400, rng)
    src = rng.integers(0, 20, 400).astype(np.uint32)
    keys[::7] = net.ids[src[::7]]                       # lookups whose source is a sibling create no extension
    right, par = engine.broose_directions(keys, src)
    creates = [not m.is_sibling_for(int(s), RB.to_int(k), 1) for s, k in zip(src, keys)]
    want, wpar = RB.directions(src, creates)
    assert list(right.astype(bool)) == want
    assert all(par[v] == c for v, c in wpar.items()) and par.sum() == sum(creates)
    r2, _ = engine.broose_directions(keys, src, par)
    assert list(r2.astype(bool)) == RB.directions(src, creates, par)[0]


def test_golden_reproduces(engine: KbrEngine):
    g = np.load(GOLD / "broose_n1000.npz")
    engine.set_params(Params.broose())
    engine.broose_load(g["ids"], g["xy"])
    off, nodes = engine.broose_export()
    R = 6
    for j, v in enumerate(g["sample_nodes"]):
        want = g["sample_rows"][j]
        for r in range(R):
            row = nodes[int(off[v * R + r]):int(off[v * R + r + 1])]
            assert np.array_equal(row, want[r][want[r] != NONE]), (v, r)
    out, cnt, sib, st, eo = engine.broose_find_node(g["fn_node"], g["fn_keys"], g["fn_right"], g["fn_ext"])
    assert np.array_equal(out[:, 0], g["fn_next"]) and np.array_equal(sib, g["fn_sib"])
    assert np.array_equal(eo["step"], g["fn_ext_out"]["step"]) and np.array_equal(eo["route_key"], g["fn_ext_out"]["route_key"])
    got = engine.broose_lookup(g["keys"], g["src"], g["right"], record_hops=True)
    for f in BC.FIELDS:
        assert np.array_equal(got[f], g[f]), f
    H = g["hop_seq"].shape[1]
    assert np.array_equal(got["hop_seq"][:, :H], g["hop_seq"]) and np.all(got["hop_seq"][:, H:] == NONE)
