"""The DHT tier on the GPU (ovs_dht_put_batch / ovs_dht_get_batch / ovs_dht_dump_node; oversim_amd/csrc/dht.hip):
every out-record field bit-exact against the message-level replay tests/refmodel_dht.py, whose LookupCalls come
from the CPU oracle."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import refmodel_dht as D
from oracle_lib import OracleNet, chord_params, kad_params
from oversim_amd import DHT_GET_DTYPE, DHT_PUT_DTYPE, DhtParams, KbrEngine, KbrError, Params, workload as W

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
SEC = 10**9
M_OPS = 2000
CAP = 1 << 15


@functools.lru_cache(maxsize=None)
def ring(n):
    return W.population(n, 0x4448 + n)


def batches(net, m, seed):
    """put, get, overwrite (every 7th a delete), get after the first TTLs ran out.  The first 64 operations share
    one key (conflicts within a batch); half the keys are node IDs."""
    rng = np.random.default_rng(seed)
    k1, s1 = W.lookups(net.ids, m // 2, seed, node_ids=True)
    k2, s2 = W.lookups(net.ids, m - m // 2, seed + 1, node_ids=False)
    keys, src = np.ascontiguousarray(np.concatenate([k1, k2])), np.ascontiguousarray(np.concatenate([s1, s2]))
    keys[:64] = keys[64]
    put = D.make_ops(m, t0_ns=rng.integers(0, 5 * SEC, m), token=np.arange(m) + 1, vlen=rng.integers(1, 200, m),
                     ttl=np.where(np.arange(m) % 2, 60, 0), kind=1 + np.arange(m) % 2, id=1 + np.arange(m) % 3)
    get1 = put.copy()
    get1["t0_ns"] = 20 * SEC + rng.integers(0, SEC, m)
    over = put.copy()
    over["t0_ns"] = 30 * SEC + rng.integers(0, SEC, m)
    over["token"] += 10**6
    over["vlen"] = np.where(np.arange(m) % 7 == 3, 0, rng.integers(1, 200, m))
    over["ttl"] = 0
    over[m // 2:] = put[m // 2:]                     # the second half is not overwritten: its odd entries expire
    over["t0_ns"][m // 2:] = 30 * SEC
    sel = np.arange(m) < m // 2
    get2 = put.copy()
    get2["t0_ns"] = 100 * SEC
    return keys, src, put, get1, over, sel, get2


def replay(M, b):
    keys, src, put, get1, over, sel, get2 = b
    r = [M.put_batch(keys, src, put), M.get_batch(keys, src, get1), M.put_batch(keys[sel], src[sel], over[sel]),
         M.get_batch(keys, src, get2)]
    for a in r:
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def chord_ref(n, rnd, m=M_OPS):
    net = ring(n)
    o = OracleNet("chord", net.ids, net.xy, chord_params(simtimeRound=rnd))
    b = batches(net, m, 7 + n)
    M = D.DhtModel(net.xy, D.oracle_lookup(o, 4), bool(rnd))
    return b, replay(M, b), M


def same(got, ref, fields, what):
    for f in fields:
        a, b = np.asarray(got[f]).astype(np.int64), ref[f].astype(np.int64)
        assert np.array_equal(a, b), (what, f, np.flatnonzero(a != b)[:5], a[a != b][:5], b[a != b][:5])


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


def check_sequence(engine, b, ref, what):
    for mode, run in (("host", host_run), ("device", device_run)):
        engine.dht_store_create(CAP)
        got = run(engine, b)
        for j, (g, r) in enumerate(zip(got, ref)):
            same(g, r, D.PUT_FIELDS if j % 2 == 0 else D.GET_FIELDS, (what, mode, j))
            if j % 2 == 0:
                assert not g["pad"].any()
        assert engine.dht_store_count()[1] == 0


def interesting(ref):
    p, g1, _, g2 = ref
    assert (p["outcome"] == D.SUCCESS).all()
    assert (g1["outcome"] == D.SUCCESS).all() and (g1["result_count"] == 1).sum() > len(g1) // 2
    assert (g2["result_count"] == 0).sum() > 0 and (g2["result_count"] == 1).sum() > 0
    assert (g2["value_token"] > 10**6).sum() > 0


@pytest.mark.parametrize("n", [2, 3, 9, 1000])
@pytest.mark.parametrize("rnd", [0, 1])
def test_chord_rings(engine: KbrEngine, n, rnd):
    b, ref, _ = chord_ref(n, rnd)
    interesting(ref)
    if n < 4:
        assert (ref[0]["num_sent"] == n).all()
    net = ring(n)
    engine.set_params(Params.chord().replace(simtimeRound=rnd))
    engine.chord_load(net.ids, net.xy)
    check_sequence(engine, b, ref, ("chord", n, rnd))


@pytest.mark.parametrize("rnd", [0, 1])
def test_kademlia_alpha_1(engine: KbrEngine, rnd):
    net = ring(2000)
    o = OracleNet("kademlia", net.ids, net.xy, kad_params(lookupParallelRpcs=1, simtimeRound=rnd))
    b = batches(net, M_OPS, 99)
    ref = replay(D.DhtModel(net.xy, D.oracle_lookup(o, 4), bool(rnd)), b)
    interesting(ref)
    engine.set_params(Params.kademlia().replace(lookupParallelRpcs=1, simtimeRound=rnd))
    engine.kad_load(net.ids, net.xy)
    check_sequence(engine, b, ref, ("kad", rnd))


def test_explicit_chord_tables(engine: KbrEngine):
    """Non-converged tables: short successor lists give fewer than numReplica siblings."""
    from test_gpu_chord import _broken_tables
    net, t = _broken_tables(1000, 33)
    o = OracleNet("chord", net.ids, net.xy, chord_params(simtimeRound=1), tables=t)
    b = batches(net, 500, 5)
    ref = replay(D.DhtModel(net.xy, D.oracle_lookup(o, 4), True), b)
    assert len(np.unique(ref[0]["num_sent"])) > 1
    engine.set_params(Params.chord().replace(simtimeRound=1))
    engine.chord_load_tables(net.ids, net.xy, t["pred"], t["succ"], t["nsucc"], t["fingers"], t["deque_size"])
    engine.dht_store_create(CAP)
    for j, (g, r) in enumerate(zip(host_run(engine, b), ref)):
        same(g, r, D.PUT_FIELDS if j % 2 == 0 else D.GET_FIELDS, ("explicit", j))


@pytest.mark.parametrize("n,G,ratio,tmo", [(1000, 1, 0.75, 1.5), (1000, 2, 1.0, 1.5), (9, 2, 0.75, 0.06), (9, 3, 1.0, 0.1),
                                           (9, 1, 0.75, 0.15), (9, 4, 1.0, 0.2), (41, 2, 0.75, 0.06), (41, 3, 1.0, 0.1),
                                           (41, 1, 0.75, 0.15), (41, 4, 1.0, 0.2)])
def test_num_get_requests_ratio_and_timeouts(engine: KbrEngine, n, G, ratio, tmo):
    """numGetRequests < numReplica with a 0.75 ratio (the ask-one-more branch); and, on small rings whose lookups
    take few FindNodeCalls, an rpcUdpTimeout between the fastest and the slowest replica RPC, so that puts fail, gets
    lose hash responses and value requests time out and are sent again."""
    net = ring(n)
    b = batches(net, 600, 11)
    o = OracleNet("chord", net.ids, net.xy, chord_params(simtimeRound=1, rpcUdpTimeout=tmo))
    ref = replay(D.DhtModel(net.xy, D.oracle_lookup(o, 4), True, 4, G, ratio, rpc_udp_timeout=tmo), b)
    if tmo < 1:
        for r in ref:
            ok = r["status"] == 0
            assert (r["outcome"][ok] == D.FAILED).any() and (r["outcome"][ok] == D.SUCCESS).any(), (n, G, tmo)
    else:
        assert (ref[1]["messages"] == 2 * 4 + 2).any()                      # every replica asked for its hash, one by one
    engine.set_params(Params.chord().replace(simtimeRound=1, rpcUdpTimeout=tmo))
    engine.chord_load(net.ids, net.xy)
    dp = DhtParams.default().replace(numGetRequests=G, ratioIdentical=ratio)
    engine.dht_store_create(CAP)
    for j, (g, r) in enumerate(zip(host_run(engine, b, dp), ref)):
        same(g, r, D.PUT_FIELDS if j % 2 == 0 else D.GET_FIELDS, (n, G, ratio, tmo, j))


def test_measure_auth_block(engine: KbrEngine):
    net = ring(9)
    o = OracleNet("chord", net.ids, net.xy, chord_params(simtimeRound=1, measureAuthBlock=1))
    b = batches(net, 300, 3)
    ref = replay(D.DhtModel(net.xy, D.oracle_lookup(o, 4), True, auth=True), b)
    engine.set_params(Params.chord().replace(simtimeRound=1, measureAuthBlock=1))
    engine.chord_load(net.ids, net.xy)
    engine.dht_store_create(CAP)
    for j, (g, r) in enumerate(zip(host_run(engine, b), ref)):
        same(g, r, D.PUT_FIELDS if j % 2 == 0 else D.GET_FIELDS, ("auth", j))


def test_dump_equals_the_replay_storage_on_the_9_node_ring(engine: KbrEngine):
    b, ref, M = chord_ref(9, 1)
    net = ring(9)
    engine.set_params(Params.chord().replace(simtimeRound=1))
    engine.chord_load(net.ids, net.xy)
    engine.dht_store_create(CAP)
    host_run(engine, b)
    total = 0
    for now in (0, 40 * SEC, 70 * SEC):
        for v in range(9):
            got, want = engine.dht_dump(v, now), M.dump(v, now)
            assert len(got) == len(want)
            for f in D.DUMP_DTYPE.names:
                assert np.array_equal(got[f], want[f]), (v, now, f)
            total += len(got)
    assert total > 0


def test_64_puts_to_one_key_from_different_sources(engine: KbrEngine):
    net = ring(1000)
    o = OracleNet("chord", net.ids, net.xy, chord_params(simtimeRound=1))
    keys = np.ascontiguousarray(np.repeat(net.ids[500][None], 64, axis=0))
    keys[:, 0] -= 1
    src = (np.arange(64, dtype=np.uint32) * 13) % 1000
    ops = D.make_ops(64, token=np.arange(64) + 1, vlen=5)
    ops["t0_ns"][32:] = 1000                          # equal times too: ties go to the higher operation index
    M = D.DhtModel(net.xy, D.oracle_lookup(o, 4), True)
    ref = M.put_batch(keys, src, ops)
    engine.set_params(Params.chord().replace(simtimeRound=1))
    engine.chord_load(net.ids, net.xy)
    engine.dht_store_create(1024)
    same(engine.dht_put(keys, src, ops), ref, D.PUT_FIELDS, "conflicts")
    assert engine.dht_store_count() == (4, 0)
    winners = []
    for v in M.store:
        got, want = engine.dht_dump(v, 0), M.dump(v, 0)
        assert len(got) == len(want) == 1 and got["token"][0] == want["token"][0]
        winners.append(int(got["token"][0]))
    assert len(winners) == 4


def test_refusals_leave_the_store_and_later_calls_unchanged(engine: KbrEngine):
    b, ref, _ = chord_ref(9, 1)
    keys, src, put, get1 = b[:4]
    net = ring(9)
    base = Params.chord().replace(simtimeRound=1)
    engine.set_params(base)
    engine.chord_load(net.ids, net.xy)
    engine.dht_store_create(CAP)
    same(engine.dht_put(keys, src, put), ref[0], D.PUT_FIELDS, "first")
    count = engine.dht_store_count()
    first = engine.dht_get(keys, src, get1)
    dflt = DhtParams.default()

    def refused(dp=dflt, ops=put, fn=None):
        with pytest.raises(KbrError, match="ENOTSUP"):
            (fn or engine.dht_put)(keys, src, ops, dp)
        assert engine.dht_store_count() == count
        again = engine.dht_get(keys, src, get1)
        for f in D.GET_FIELDS:
            assert np.array_equal(again[f], first[f]), f

    for kw in (dict(numReplica=0), dict(numReplica=9), dict(numGetRequests=0), dict(numGetRequests=9),
               dict(secureMaintenance=1), dict(invalidDataAttack=1), dict(maintenanceAttack=1)):
        refused(dflt.replace(**kw))
        refused(dflt.replace(**kw), get1, engine.dht_get)
    wild = put.copy()
    wild["id"][5] = 0
    refused(ops=wild)
    refused(ops=wild, fn=engine.dht_get)
    wild = get1.copy()
    wild["kind"][7] = 0
    refused(ops=wild, fn=engine.dht_get)
    for kw in (dict(lookupParallelRpcs=3), dict(routingType=1), dict(routingType=2), dict(successorListSize=3)):
        engine.set_params(base.replace(**kw))
        with pytest.raises(KbrError, match="ENOTSUP"):
            engine.dht_put(keys, src, put)
        with pytest.raises(KbrError, match="ENOTSUP"):
            engine.dht_get(keys, src, get1)
        engine.set_params(base)
        assert engine.dht_store_count() == count
        again = engine.dht_get(keys, src, get1)
        for f in D.GET_FIELDS:
            assert np.array_equal(again[f], first[f]), (kw, f)
    # a store that is too small: nothing changes, the same call on a large enough store gives the same records
    engine.dht_store_create(100)
    with pytest.raises(KbrError, match="ENOMEM"):
        engine.dht_put(keys, src, put)
    assert engine.dht_store_count()[0] == 0
    assert (engine.dht_get(keys, src, get1)["result_count"] == 0).all()


def test_koorde_is_refused():
    net = ring(1000)
    keys, src = W.lookups(net.ids, 8, 1)
    with KbrEngine(0) as e:
        e.set_params(Params.koorde())
        e.koorde_load(net.ids, net.xy)
        e.dht_store_create(64)
        with pytest.raises(KbrError, match="ENOTSUP"):
            e.dht_put(keys, src, D.make_ops(8, token=1, vlen=1))
        with pytest.raises(KbrError, match="ENOTSUP"):
            e.dht_get(keys, src, D.make_ops(8))


def test_golden_fixture(engine: KbrEngine):
    z = np.load(GOLD / "dht_chord_n1000.npz")
    engine.set_params(Params.chord().replace(simtimeRound=1))
    engine.chord_load(z["ids"], z["xy"])
    engine.dht_store_create(CAP)
    h = len(z["over"])
    same(engine.dht_put(z["keys"], z["src"], z["put"]), z["put_out"], D.PUT_FIELDS, "golden put")
    same(engine.dht_get(z["keys"], z["src"], z["get1"]), z["get1_out"], D.GET_FIELDS, "golden get")
    same(engine.dht_put(z["keys"][:h], z["src"][:h], z["over"]), z["over_out"], D.PUT_FIELDS, "golden overwrite")
    same(engine.dht_get(z["keys"], z["src"], z["get2"]), z["get2_out"], D.GET_FIELDS, "golden get 2")
    assert (z["get2_out"]["result_count"] == 0).any() and (z["get2_out"]["value_token"] > 10**6).any()


def stats_same(got, ref):
    for f in D.STAT_INTS:
        assert int(getattr(got, f)) == int(ref[f]), (f, getattr(got, f), ref[f])
    for f in D.STAT_SDS:
        g, r = getattr(got, f), ref[f]
        assert g.count == r["count"], f
        # a handful of double operations on exact integer sums (latencies) or on per-node counts in node order:
        # 1e-12 relative leaves room for the order of the sums, nothing else
        for a in ("mean", "stddev", "min", "max"):
            assert getattr(g, a) == pytest.approx(r[a], rel=1e-12, abs=1e-15), (f, a)


@pytest.mark.parametrize("n,tmo", [(1000, 1.5), (9, 0.1)])
def test_dhttest_statistics(engine: KbrEngine, n, tmo):
    net = ring(n)
    b = batches(net, 600, 11)
    keys, src, put, get1, over, sel, get2 = b
    o = OracleNet("chord", net.ids, net.xy, chord_params(simtimeRound=1, rpcUdpTimeout=tmo))
    ref = replay(D.DhtModel(net.xy, D.oracle_lookup(o, 4), True, rpc_udp_timeout=tmo), b)
    # the caller's GlobalDhtTestMap after the first put batch: what it believes it stored; some keys unknown, some
    # with a wrong value, the odd ones ended by their TTL
    ex = np.zeros(len(src), dtype=D.EXPECT_DTYPE)
    ex["token"], ex["known"] = put["token"], 1
    ex["known"][::11] = 0
    ex["token"][::13] += 5
    ex["endtime_ns"] = np.where(put["ttl"] > 0, put["t0_ns"] + 60 * SEC, D.NEVER)
    engine.set_params(Params.chord().replace(simtimeRound=1, rpcUdpTimeout=tmo))
    engine.chord_load(net.ids, net.xy)
    engine.dht_store_create(CAP)
    got = host_run(engine, b)
    for T in (1000.0, 0.05):
        for gi, gops in ((1, get1), (3, get2)):
            want = D.dhttest_stats(n, ref[0], src, ref[gi], gops, src, ex, T)
            assert want["num_get_success"] > 0 and want["num_get_error"] > 0
            stats_same(engine.dhttest_stats(got[0], src, got[gi], gops, src, ex, T), want)
    want = D.dhttest_stats(n, ref[0][:0], src[:0], ref[3], get2, src, ex, 1000.0)
    stats_same(engine.dhttest_stats(got[0][:0], src[:0], got[3], get2, src, ex, 1000.0), want)
    if tmo < 1:
        assert (ref[0]["outcome"] == D.FAILED).any() and (ref[3]["outcome"] == D.FAILED).any()


def _expect_enotsup(e, keys, src):
    with pytest.raises(KbrError, match="ENOTSUP"):
        e.dht_put(keys, src, D.make_ops(len(src), token=1, vlen=1))
    with pytest.raises(KbrError, match="ENOTSUP"):
        e.dht_get(keys, src, D.make_ops(len(src)))


def test_shard_context_epichord_and_kademlia_alpha_are_refused():
    import ctypes as C
    from epichord_snap import make_snapshot
    from oversim_amd import lib
    from oversim_amd import shard  # noqa: F401  (declares the shard entry points' signatures)
    net = ring(1000)
    keys, src = W.lookups(net.ids, 8, 1)
    with KbrEngine(0) as e:                                  # one arc of a sharded Chord ring
        e.set_params(Params.chord())
        ids, xy = np.ascontiguousarray(net.ids), np.ascontiguousarray(net.xy, dtype=np.float64)
        e._chk(lib().ovs_chord_load_shard(e._h, ids.ctypes.data_as(C.c_void_p), len(ids), xy.ctypes.data_as(C.c_void_p),
                                          0, 500, 0), "ovs_chord_load_shard")
        e.dht_store_create(64)
        _expect_enotsup(e, keys, src % 500)
    snap = make_snapshot(60, 21, list_size=4)
    with KbrEngine(0) as e:                                  # EpiChord
        e.set_params(Params.epichord().replace(successorListSize=snap["L"]))
        e.epichord_load(snap["ids"], np.zeros((snap["n"], 2)), snap["succ"], snap["nsucc"], snap["pred"], snap["npred"],
                        snap["full"], snap["cache_off"], snap["cache_node"], snap["cache_last"], snap["cache_ttl"])
        e.dht_store_create(64)
        _expect_enotsup(e, keys, src % 60)
    with KbrEngine(0) as e:                                  # Kademlia with alpha = 3: the one overlay where it matters
        e.set_params(Params.kademlia().replace(lookupParallelRpcs=3))
        e.kad_load(net.ids, net.xy)
        e.dht_store_create(1 << 12)
        _expect_enotsup(e, keys, src)
        assert e.dht_store_count() == (0, 0)
        e.set_params(Params.kademlia().replace(lookupParallelRpcs=1))
        assert (e.dht_put(keys, src, D.make_ops(8, token=1, vlen=1))["outcome"] == D.SUCCESS).all()


def test_a_put_batch_that_does_not_fit_changes_nothing_in_either_pointer_mode(engine: KbrEngine):
    b, ref, _ = chord_ref(9, 1)
    keys, src, put, get1, over, sel, get2 = b
    net = ring(9)
    engine.set_params(Params.chord().replace(simtimeRound=1))
    engine.chord_load(net.ids, net.xy)
    small = 400
    k0, s0, p0 = keys[:64], src[:64], put[:64]               # 64 puts x 4 replicas fit into 400 slots
    engine.dht_store_create(small)
    first_put = engine.dht_put(k0, s0, p0)
    count = engine.dht_store_count()
    assert 0 < count[0] <= 256 and count[1] == 0
    first = engine.dht_get(keys, src, get1)
    dumps = [engine.dht_dump(v, 0) for v in range(9)]

    def unchanged(refused):
        assert engine.dht_store_count() == (count[0], refused)
        again = engine.dht_get(keys, src, get1)
        for f in D.GET_FIELDS:
            assert np.array_equal(again[f], first[f]), f
        for v in range(9):
            assert np.array_equal(engine.dht_dump(v, 0), dumps[v])

    with pytest.raises(KbrError, match="ENOMEM"):            # 2000 puts do not
        engine.dht_put(keys, src, over)
    unchanged(1)
    dk = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    ds = torch.from_numpy(src.view(np.int32).copy()).cuda()
    dop = torch.from_numpy(over.view(np.uint8).copy()).cuda()
    do = torch.zeros(len(src) * DHT_PUT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    engine.dht_put_device(dk.data_ptr(), ds.data_ptr(), dop.data_ptr(), len(src), do.data_ptr())
    torch.cuda.synchronize()
    unchanged(2)
    # the same valid call afterwards gives identical arrays
    again_put = engine.dht_put(k0, s0, p0)
    for f in D.PUT_FIELDS:
        assert np.array_equal(again_put[f], first_put[f]), f
    assert engine.dht_store_count() == (count[0], 2)
