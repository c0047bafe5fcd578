"""The DHT tier on a Pastry context on the GPU (ovs_dht_put_batch / ovs_dht_get_batch / ovs_dht_dump_node /
ovs_dhttest_stats_batch over k_pastry_iter and the kernels of oversim_amd/csrc/dht.hip): every out-record field
bit-equal to the message-level replay tests/refmodel_dht.py fed by the Pastry iterative LookupCall of
tests/refmodel_pastry_iter.py (tests/refmodel_dht_pastry.pastry_lookup).  The networks, batches and replays are
those of tests/dht_pastry_cases.py, which tests/test_dht_pastry_model.py checks on the CPU."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest
import torch

import dht_pastry_cases as X
import refmodel_dht as D
from oversim_amd import (DHT_GET_DTYPE, DHT_PUT_DTYPE, DhtParams, DhtTeamParams, KbrEngine, KbrError, Params,
                         PastryParams)
from oversim_amd.kbr import Network

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
SEC = X.SEC
CAP = 1 << 14
SMALLEST = 2                       # ovs_pastry_load: "Pastry needs at least 2 nodes"


def load(engine, n, b=4, L=16, rnd=1, tmo=1.5, auth=0, acks=0, ids=None, xy=None, **pk):
    net = X.population(n) if ids is None else Network(ids=ids, xy=xy)
    engine.set_params(Params.pastry().replace(routingType=0, simtimeRound=rnd, rpcUdpTimeout=tmo, measureAuthBlock=auth, **pk))
    engine.pastry_load(net.ids, net.xy, PastryParams.default(routeMsgAcks=acks, bitsPerDigit=b, numberOfLeaves=L))
    return net


def dparams(R=4, G=4, **kw):
    return DhtParams.default().replace(numReplica=R, numGetRequests=G, **kw)


def same(got, ref, fields, what):
    for f in fields:
        a, b = np.asarray(got[f]).astype(np.int64), np.asarray(ref[f]).astype(np.int64)
        assert np.array_equal(a, b), (what, f, np.flatnonzero(a != b)[:5], a[a != b][:5], b[a != b][:5])


def fields(j):
    return D.PUT_FIELDS if j % 2 == 0 else D.GET_FIELDS


def host_run(engine, b, dp=None):
    keys, src, put, get1, over, sel, get2 = b
    return [engine.dht_put(keys, src, put, dp), engine.dht_get(keys, src, get1, dp),
            engine.dht_put(keys[sel], src[sel], over[sel], dp), engine.dht_get(keys, src, get2, dp)]


def device_run(engine, b, dp=None):
    keys, src, put, get1, over, sel, get2 = b
    res = []
    for is_put, k, s, ops in ((1, keys, src, put), (0, keys, src, get1), (1, keys[sel], src[sel], over[sel]),
                              (0, keys, src, get2)):
        dt = DHT_PUT_DTYPE if is_put else DHT_GET_DTYPE
        dk = torch.from_numpy(np.ascontiguousarray(k).view(np.int32).copy()).cuda()
        ds = torch.from_numpy(np.ascontiguousarray(s).view(np.int32).copy()).cuda()
        dop = torch.from_numpy(np.ascontiguousarray(ops).view(np.uint8).copy()).cuda()
        do = torch.full((len(s) * dt.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
        fn = engine.dht_put_device if is_put else engine.dht_get_device
        fn(dk.data_ptr(), ds.data_ptr(), dop.data_ptr(), len(s), do.data_ptr(), dp)
        torch.cuda.synchronize()
        res.append(do.cpu().numpy().view(dt).copy())
    return res


def check_sequence(engine, b, ref, what, dp=None):
    """The put / get / overwrite / get sequence with host pointers and with device pointers: both the model's."""
    runs = {}
    for mode, run in (("host", host_run), ("device", device_run)):
        engine.dht_store_create(CAP)
        runs[mode] = run(engine, b, dp)
        for j, (g, r) in enumerate(zip(runs[mode], ref)):
            same(g, r, fields(j), (what, mode, j))
            if j % 2 == 0:
                assert not g["pad"].any()
        assert engine.dht_store_count()[1] == 0
    for j, (h, d) in enumerate(zip(runs["host"], runs["device"])):
        assert h.tobytes() == d.tobytes(), (what, "host and device records differ", j)


# n, bitsPerDigit, numberOfLeaves, simtimeRound, numReplica, numGetRequests, rpcUdpTimeout, measureAuthBlock
CASES = [
    (SMALLEST, 4, 16, 1, 4, 4, 1.5, 0), (3, 4, 16, 1, 4, 4, 1.5, 0), (9, 4, 16, 1, 4, 4, 1.5, 0),     # rows shorter than R
    (3, 2, 8, 0, 4, 1, 1.5, 0), (9, 4, 16, 0, 8, 4, 1.5, 0),                                          # (9 nodes, R = 8 too)
    (64, 4, 16, 1, 4, 4, 1.5, 0), (64, 2, 8, 0, 4, 1, 1.5, 0), (64, 4, 16, 1, 4, 4, 1.5, 1),
    (1000, 4, 16, 1, 4, 4, 1.5, 0), (1000, 4, 16, 0, 4, 4, 1.5, 0), (1000, 2, 8, 1, 4, 4, 1.5, 0),
    (1000, 4, 16, 1, 1, 1, 1.5, 0), (1000, 4, 16, 1, 8, 4, 1.5, 0), (1000, 4, 16, 0, 8, 1, 1.5, 0),
    (1000, 4, 16, 1, 4, 4, X.SHORT_TMO, 0), (1000, 2, 8, 0, 4, 1, X.SHORT_TMO, 1),
]


@pytest.mark.parametrize("n,b,L,rnd,R,G,tmo,auth", CASES)
def test_records_equal_the_model(engine: KbrEngine, n, b, L, rnd, R, G, tmo, auth):
    bt, ref, _ = X.reference(n, b, L, rnd, R, G, tmo, bool(auth))
    c = X.census(ref)
    if tmo < 1:
        assert min(c["put_ok"], c["put_failed"], c["put_lookup_failed"], c["get_ok"], c["get_failed"]) > 0, c
    else:
        assert c["put_ok"] > 0 and c["get_value"] > 0, c
    if n < R:
        ok = ref[0]["outcome"] != D.LOOKUP_FAILED
        assert ok.any() and (ref[0]["num_sent"][ok] == n).all()         # the majority counts the real siblings
    load(engine, n, b, L, rnd, tmo, auth)
    check_sequence(engine, bt, ref, (n, b, L, rnd, R, G, tmo, auth), dparams(R, G))


def test_golden_fixture(engine: KbrEngine):
    z = np.load(GOLD / "dht_pastry_n1000.npz")
    h = len(z["over"])
    for tag, tmo in (("d", 1.5), ("s", float(z["short_timeout"]))):
        engine.set_params(Params.pastry().replace(routingType=0, simtimeRound=1, rpcUdpTimeout=tmo))
        engine.pastry_load(z["ids"], z["xy"], PastryParams.default(routeMsgAcks=0))
        engine.dht_store_create(CAP)
        same(engine.dht_put(z["keys"], z["src"], z["put"]), z[f"{tag}_put_out"], D.PUT_FIELDS, (tag, "put"))
        same(engine.dht_get(z["keys"], z["src"], z["get1"]), z[f"{tag}_get1_out"], D.GET_FIELDS, (tag, "get"))
        same(engine.dht_put(z["keys"][:h], z["src"][:h], z["over"]), z[f"{tag}_over_out"], D.PUT_FIELDS, (tag, "overwrite"))
        same(engine.dht_get(z["keys"], z["src"], z["get2"]), z[f"{tag}_get2_out"], D.GET_FIELDS, (tag, "get 2"))
    s = z["s_put_out"]["outcome"]
    assert (s == D.SUCCESS).any() and (s == D.FAILED).any() and (s == D.LOOKUP_FAILED).any()
    assert (z["d_get2_out"]["result_count"] == 0).any() and (z["d_get2_out"]["value_token"] > 10**6).any()


@pytest.mark.parametrize("n", [9, 64])
def test_dump_and_store_count_equal_the_replay_storage(engine: KbrEngine, n):
    bt = X.batches(X.population(n), X.M_OPS, 7 + n)
    keys, src, put, get1, over, sel, get2 = bt
    M = X.model(n)
    load(engine, n)
    engine.dht_store_create(CAP)
    same(engine.dht_put(keys, src, put), M.put_batch(keys, src, put), D.PUT_FIELDS, "put")
    # no delete yet: every slot in use is one (replica, key, kind, id) entry of the replay
    assert engine.dht_store_count() == (M.count(), 0)
    same(engine.dht_get(keys, src, get1), M.get_batch(keys, src, get1), D.GET_FIELDS, "get")
    same(engine.dht_put(keys[sel], src[sel], over[sel]), M.put_batch(keys[sel], src[sel], over[sel]), D.PUT_FIELDS, "over")
    total = 0
    for now in (0, 40 * SEC, 70 * SEC, 200 * SEC):
        for v in range(0, n, max(1, n // 9)):
            got, want = engine.dht_dump(v, now), M.dump(v, now)
            assert len(got) == len(want), (v, now)
            for f in D.DUMP_DTYPE.names:
                assert np.array_equal(got[f], want[f]), (v, now, f)
            total += len(got)
    assert total > 0


def test_exported_tables_give_the_records_of_the_rule(engine: KbrEngine):
    bt, ref, _ = X.reference(1000)
    net = load(engine, 1000)
    leaf, tab = engine.pastry_export()
    engine.pastry_load_tables(net.ids, net.xy, leaf, tab, PastryParams.default(routeMsgAcks=0))
    check_sequence(engine, bt, ref, "load_tables(export)")
    bt, ref, _ = X.reference(3)                      # the replayed leaf sets of a small network
    net = load(engine, 3)
    leaf, tab = engine.pastry_export()
    engine.pastry_load_tables(net.ids, net.xy, leaf, tab, PastryParams.default(routeMsgAcks=0))
    check_sequence(engine, bt, ref, "load_tables(export) n=3")


def test_default_pastry_params_acks_on(engine: KbrEngine):
    """A DHT operation sends FindNodeCalls and direct RPCs, no route message: routeMsgAcks = true runs and gives the
    records of routeMsgAcks = false."""
    bt, ref, _ = X.reference(1000)
    net = X.population(1000)
    engine.set_params(Params.pastry().replace(routingType=0))
    engine.pastry_load(net.ids, net.xy, PastryParams.default())
    assert PastryParams.default().routeMsgAcks == 1
    check_sequence(engine, bt, ref, "acks on")


@pytest.mark.parametrize("tmo", [1.5, X.SHORT_TMO])
def test_dhttest_statistics(engine: KbrEngine, tmo):
    n = 1000
    bt, ref, _ = X.reference(n, tmo=tmo)
    keys, src, put, get1, over, sel, get2 = bt
    ex = np.zeros(len(src), dtype=D.EXPECT_DTYPE)
    ex["token"], ex["known"] = put["token"], 1
    ex["known"][::11] = 0
    ex["token"][::13] += 5
    ex["endtime_ns"] = np.where(put["ttl"] > 0, put["t0_ns"] + 60 * SEC, D.NEVER)
    load(engine, n, tmo=tmo)
    engine.dht_store_create(CAP)
    got = host_run(engine, bt)
    for T in (1000.0, 0.05):
        for gi, gops in ((1, get1), (3, get2)):
            want = D.dhttest_stats(n, ref[0], src, ref[gi], gops, src, ex, T)
            assert want["num_get_success"] > 0 and want["num_get_error"] > 0
            st = engine.dhttest_stats(got[0], src, got[gi], gops, src, ex, T)
            for f in D.STAT_INTS:
                assert int(getattr(st, f)) == int(want[f]), (f, getattr(st, f), want[f])
            for f in D.STAT_SDS:
                g, r = getattr(st, f), want[f]
                assert g.count == r["count"], f
                # the existing comparator's tolerance (tests/test_gpu_dht.py): double operations on exact integer sums
                for a in ("mean", "stddev", "min", "max"):
                    assert getattr(g, a) == pytest.approx(r[a], rel=1e-12, abs=1e-15), (f, a)
    if tmo < 1:
        assert (ref[0]["outcome"] == D.FAILED).any() and (ref[0]["outcome"] == D.LOOKUP_FAILED).any()


@pytest.mark.parametrize("tmo,R", [(1.5, 4), (X.SHORT_TMO, 4), (1.5, 8)])
def test_lookup_share_equals_the_pastry_lookup_call(engine: KbrEngine, tmo, R):
    """64 keys: hop_count, status and the lookup's share of each record are what ovs_pastry_lookup_batch reports for
    the same key and source -- the replay fed by the engine's own LookupCall gives the engine's DHT records."""
    bt = X.batches(X.population(1000), 64, 1234)
    keys, src, put, get1 = bt[:4]
    load(engine, 1000, tmo=tmo)
    look = engine.pastry_lookup_call(keys, src, R)
    assert look["siblings"].shape == (64, R)
    dp = dparams(R, min(R, 4))
    engine.dht_store_create(CAP)
    p, g = engine.dht_put(keys, src, put, dp), engine.dht_get(keys, src, get1, dp)
    valid = (look["is_valid"] != 0) & (look["num_siblings"] > 0)
    for r in (p, g):
        assert np.array_equal(r["status"], look["status"])
        assert np.array_equal(r["outcome"] == D.LOOKUP_FAILED, ~valid)
        assert np.array_equal(r["hop_count"][valid], look["hops"][valid]) and (r["hop_count"][~valid] == 0).all()
        assert (r["latency_ns"][valid] >= look["latency_ns"][valid]).all() and (r["latency_ns"][~valid] == -1).all()
    assert np.array_equal(p["num_sent"][valid], np.minimum(look["num_siblings"][valid], R))
    M = D.DhtModel(X.population(1000).xy, lambda k, s: engine.pastry_lookup_call(k, s, R), True, R, min(R, 4), rpc_udp_timeout=tmo)
    same(p, M.put_batch(keys, src, put), D.PUT_FIELDS, "put on the engine's lookups")
    same(g, M.get_batch(keys, src, get1), D.GET_FIELDS, "get on the engine's lookups")
    if tmo < 1:
        assert (~valid).any() and valid.any()


def test_refusals_leave_the_store_and_later_calls_unchanged(engine: KbrEngine):
    n, L = 64, 8
    bt, ref, _ = X.reference(n, 4, L)
    keys, src, put, get1 = bt[:4]
    net = X.population(n)
    base = Params.pastry().replace(routingType=0)
    load(engine, n, 4, L)
    engine.dht_store_create(CAP)
    same(engine.dht_put(keys, src, put), ref[0], D.PUT_FIELDS, "first")
    count = engine.dht_store_count()
    first = engine.dht_get(keys, src, get1)
    same(first, ref[1], D.GET_FIELDS, "first get")
    dflt = DhtParams.default()

    def unchanged(what):
        assert engine.dht_store_count() == count, what
        again = engine.dht_get(keys, src, get1)
        for f in D.GET_FIELDS:
            assert np.array_equal(again[f], first[f]), (what, f)

    def refused(match, fn):
        with pytest.raises(KbrError, match=match) as e:
            fn()
        assert "ENOTSUP" in str(e.value), str(e.value)

    # the overlay parameters, each refusal naming its key
    for match, kw in (("routingType", dict(routingType=1)), ("lookupParallelRpcs", dict(lookupParallelRpcs=3)),
                      ("lookupMerge", dict(lookupMerge=1))):
        engine.set_params(base.replace(**kw))
        refused(match, lambda: engine.dht_put(keys, src, put))
        refused(match, lambda: engine.dht_get(keys, src, get1))
        engine.set_params(base)
        unchanged(kw)
    # getMaxNumSiblings() = numberOfLeaves / 2 = 4 (DHT.cc:84-87)
    for R in (8, 5):
        refused("numReplica > getMaxNumSiblings", lambda: engine.dht_put(keys, src, put, dparams(R, 4)))
        refused("numReplica > getMaxNumSiblings", lambda: engine.dht_get(keys, src, get1, dparams(R, 4)))
        unchanged(R)
    # the tier's own
    for match, kw in (("numReplica", dict(numReplica=0)), ("numReplica", dict(numReplica=9)), ("numGetRequests", dict(numGetRequests=0)),
                      ("numGetRequests", dict(numGetRequests=9)), ("secureMaintenance", dict(secureMaintenance=1)),
                      ("invalidDataAttack", dict(invalidDataAttack=1)), ("maintenanceAttack", dict(maintenanceAttack=1)),
                      ("ratioIdentical", dict(ratioIdentical=0.0))):
        refused(match, lambda: engine.dht_put(keys, src, put, dflt.replace(**kw)))
        refused(match, lambda: engine.dht_get(keys, src, get1, dflt.replace(**kw)))
    unchanged("dht params")
    # the replica-team DHTs stay refused on Pastry, by name
    tp = DhtTeamParams.symmetric(2)
    refused("Pastry", lambda: engine.dht_team_put(keys, src, put, tp))
    refused("Pastry", lambda: engine.dht_team_get(keys, src, get1, tp))
    unchanged("teams")
    # the generic calls keep their pinned text on the same engine
    pinned = "Pastry: ovs_pastry_route_batch and ovs_pastry_find_node_batch only"
    refused(pinned, lambda: engine.lookupCall(keys, src))
    refused(pinned, lambda: engine.rpcCall(keys, src))
    refused(pinned, lambda: engine.lookup(keys, src))
    unchanged("generic calls")
    # a store that is too small: OVS_ENOMEM, nothing changes; device pointers count the refused batch
    engine.dht_store_create(100)
    with pytest.raises(KbrError, match="ENOMEM"):
        engine.dht_put(keys, src, put)
    assert engine.dht_store_count() == (0, 1)
    assert (engine.dht_get(keys, src, get1)["result_count"] == 0).all()
    assert all(len(engine.dht_dump(v, 0)) == 0 for v in range(0, n, 7))
    # and after all of it the sequence still gives the model's records
    engine.dht_store_create(CAP)
    for j, (g, r) in enumerate(zip(host_run(engine, bt), ref)):
        same(g, r, fields(j), ("after the refusals", j))
    # a context without a store, and another overlay's refusals as they were
    with KbrEngine(0) as e:
        e.set_params(base)
        e.pastry_load(net.ids, net.xy, PastryParams.default(routeMsgAcks=0, numberOfLeaves=L))
        with pytest.raises(KbrError, match="ESTATE"):
            e.dht_put(keys, src, put)
