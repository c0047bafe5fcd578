"""Replica-team DHTs on the GPU (ovs_dht_team_keys / _put_batch / _get_batch, ovs_dhttest_team_stats_batch;
oversim_amd/csrc/dht_teams.hip): every field of team_out, out and the winner index bit-equal to the event-heap
model tests/refmodel_dht_teams.py, and the store equal to the model's through ovs_dht_dump_node.

The engine's loader takes rings of two nodes and more, so the smallest ring here is n = 2: all teams share
both replicas, the source is one of them, and its zero-delay self sends make same-nanosecond ties real."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import dht_teams_cases as K
import refmodel_dht as D
import refmodel_dht_teams as TM
from oversim_amd import (DHT_GET_DTYPE, DHT_PUT_DTYPE, DhtParams, DhtTeamParams, KbrEngine, KbrError, Params)

pytestmark = pytest.mark.gpu
SEC = K.SEC
CAP = 1 << 16
M_OPS = 256


def tparams(mode, T):
    return DhtTeamParams(mode, T)


def load(engine, n, rnd=1, **kw):
    net = K.ring(n)
    engine.set_params(Params.chord().replace(simtimeRound=rnd, **kw))
    engine.chord_load(net.ids, net.xy)
    engine.dht_store_create(CAP)
    return net


def run_host(engine, b, tp, dp):
    return [(engine.dht_team_put if is_put else engine.dht_team_get)(k, s, o, tp, dp) for is_put, k, s, o in K.sequence(b)]


def check_sequence(engine, b, ref, tp, dp, what):
    got = run_host(engine, b, tp, dp)
    for j, (g, r) in enumerate(zip(got, ref)):
        K.same_result(g, r, j % 2 == 0, (what, j))
        if j % 2 == 0:
            assert not g[0]["pad"].any() and not g[1]["pad"].any()
    assert engine.dht_store_count()[1] == 0


def check_store(engine, M, n, times):
    for v in range(n):
        for now in times:
            got, want = engine.dht_dump(v, now), M.dump(v, now)
            assert len(got) == len(want), (v, now, len(got), len(want))
            for f in D.DUMP_DTYPE.names:
                assert np.array_equal(got[f], want[f]), (v, now, f)


@functools.lru_cache(maxsize=None)
def small_ref(n, mode, T):
    b = K.batches(n, M_OPS, 40 + n)
    M = K.model(n, mode, T)
    return b, K.replay(M, b), M


@pytest.mark.parametrize("n", [2, 3, 9])
@pytest.mark.parametrize("mode,T", [(TM.SYMMETRIC, 4), (TM.SYMMETRIC, 8), (TM.REPEATED_HASHING, 2)])
def test_small_rings_records_and_store(engine: KbrEngine, n, mode, T):
    """Teams share replicas, the source is a replica or a responder; node-ID keys and random keys."""
    b, ref, M = small_ref(n, mode, T)
    assert (ref[1][0]["result_count"] == 1).sum() > M_OPS // 2 and (ref[3][0]["result_count"] == 0).any()
    if n == 2:
        assert len(np.unique(ref[0][2])) > 1                      # more than one team wins
    load(engine, n)
    check_sequence(engine, b, ref, tparams(mode, T), DhtParams.default().replace(numReplica=8), ("small", n, mode, T))
    check_store(engine, M, n, (0, 50 * SEC, 200 * SEC))


@functools.lru_cache(maxsize=None)
def big_ref(n, mode, T, R, rnd, auth, hcm):
    b = K.batches(n, M_OPS, 70 + n + T)
    return b, K.replay(K.model(n, mode, T, rnd, R, hop_max=hcm, auth=bool(auth)), b)


@pytest.mark.parametrize("n,mode,T,R,rnd,auth,hcm", [
    (1000, TM.SYMMETRIC, 1, 8, 1, 0, 50), (1000, TM.SYMMETRIC, 2, 8, 1, 0, 50), (1000, TM.SYMMETRIC, 4, 8, 1, 0, 50),
    (1000, TM.SYMMETRIC, 8, 8, 1, 0, 50), (1000, TM.SYMMETRIC, 4, 8, 0, 0, 50), (1000, TM.SYMMETRIC, 4, 8, 1, 1, 50),
    (1000, TM.SYMMETRIC, 4, 8, 1, 0, 3), (1000, TM.REPEATED_HASHING, 2, 8, 1, 0, 50), (1000, TM.REPEATED_HASHING, 4, 8, 0, 0, 50),
    (1000, TM.REPEATED_HASHING, 4, 4, 1, 0, 3), (64, TM.SYMMETRIC, 4, 8, 1, 0, 50), (64, TM.SYMMETRIC, 2, 2, 0, 1, 50),
    (64, TM.REPEATED_HASHING, 2, 4, 1, 0, 3), (64, TM.SYMMETRIC, 8, 8, 0, 0, 3)])
def test_rings_64_and_1000(engine: KbrEngine, n, mode, T, R, rnd, auth, hcm):
    """numReplica / T = 1 and 2 (and 8), both SimTime roundings, measureAuthBlock, hopCountMax 50 and 3."""
    b, ref = big_ref(n, mode, T, R, rnd, auth, hcm)
    if hcm == 3 and n == 1000:
        assert (ref[0][1]["status"] == 3).any() and (ref[0][1]["status"] == 0).any()      # the hop budget decides
    load(engine, n, rnd, measureAuthBlock=auth, hopCountMax=hcm)
    check_sequence(engine, b, ref, tparams(mode, T), DhtParams.default().replace(numReplica=R), (n, mode, T, R, rnd, auth, hcm))


@functools.lru_cache(maxsize=None)
def low_ref():
    b = K.batches(1000, 512, 9)
    return b, K.replay(K.model(1000, TM.SYMMETRIC, 4, **K.LOW), b)


def test_low_datarate_coupling_and_timeouts(engine: KbrEngine):
    b, ref = low_ref()
    t = ref[0][1]
    assert ((t["outcome"] != 0).any(1) & (t["outcome"] == 0).any(1)).any()
    load(engine, 1000, datarate=K.LOW["datarate"], rpcUdpTimeout=K.LOW["rpc_udp_timeout"])
    check_sequence(engine, b, ref, tparams(TM.SYMMETRIC, 4), DhtParams.default().replace(numReplica=8), "low")


@pytest.mark.parametrize("G,ratio,tmo", [(1, 0.75, 1.5), (2, 1.0, 1.5), (1, 0.75, 0.12), (2, 1.0, 0.08)])
def test_num_get_requests_below_the_teams_replicas(engine: KbrEngine, G, ratio, tmo):
    """numGetRequests < numReplica / T = 4: the ask-one-more branch, and timeouts that send value requests again."""
    b = K.batches(41, M_OPS, 5)
    ref = K.replay(K.model(41, TM.SYMMETRIC, 2, 1, 8, G, ratio, rpc_udp_timeout=tmo), b)
    if tmo < 1:
        ok = ref[1][1]["status"] == 0
        assert (ref[1][1]["outcome"][ok] == D.FAILED).any() and (ref[1][1]["outcome"][ok] == D.SUCCESS).any()
    load(engine, 41, rpcUdpTimeout=tmo)
    dp = DhtParams.default().replace(numReplica=8, numGetRequests=G, ratioIdentical=ratio)
    check_sequence(engine, b, ref, tparams(TM.SYMMETRIC, 2), dp, (G, ratio, tmo))


def test_one_team_equals_the_plain_dht_calls(engine: KbrEngine):
    b = K.batches(1000, M_OPS, 21)
    tp, dp = tparams(TM.SYMMETRIC, 1), DhtParams.default()
    load(engine, 1000)
    team = run_host(engine, b, tp, dp)
    dumps = [engine.dht_dump(v, 0) for v in range(0, 1000, 37)]
    engine.dht_store_create(CAP)
    for j, (is_put, k, s, o) in enumerate(K.sequence(b)):
        plain = (engine.dht_put if is_put else engine.dht_get)(k, s, o, dp)
        fields = D.PUT_FIELDS if is_put else D.GET_FIELDS
        K.same(team[j][0], plain, fields, ("plain", j))
        K.same(team[j][1][:, 0], plain, fields, ("plain team", j))
        assert not team[j][2].any()
    for v, d in zip(range(0, 1000, 37), dumps):
        assert np.array_equal(engine.dht_dump(v, 0), d)


@pytest.mark.parametrize("mode,T", [(TM.SYMMETRIC, 1), (TM.SYMMETRIC, 3), (TM.SYMMETRIC, 8), (TM.REPEATED_HASHING, 2),
                                    (TM.REPEATED_HASHING, 8)])
def test_team_keys_equal_the_model(engine: KbrEngine, mode, T):
    keys = np.ascontiguousarray(K.batches(1000, 300, 3)[0])
    keys[0] = 0
    keys[1] = 0xFFFFFFFF
    keys[2] = [5, 0, 0, 0, 0]                                     # leading zero nibbles
    keys[3] = [0, 0, 0, 0, 0x0000FFFF]
    assert np.array_equal(engine.dht_team_keys(keys, tparams(mode, T)), TM.team_keys(keys, mode, T))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def run_device(engine, b, tp, dp):
    res = []
    T = tp.numReplicaTeams
    for is_put, k, s, o in K.sequence(b):
        dt = DHT_PUT_DTYPE if is_put else DHT_GET_DTYPE
        n = len(s)
        dk, ds, dop = dev(k), dev(s), dev(o)
        do = torch.full((n * dt.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
        dteam = torch.full((n * T * dt.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
        dw = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        engine.dht_team_device(is_put, dk.data_ptr(), ds.data_ptr(), dop.data_ptr(), n, do.data_ptr(), dteam.data_ptr(),
                               dw.data_ptr(), tp, dp)
        torch.cuda.synchronize()
        res.append((do.cpu().numpy().view(dt).copy(), dteam.cpu().numpy().view(dt).reshape(n, T).copy(), dw.cpu().numpy()))
    return res


def test_device_pointers_equal_host_pointers_and_a_batch_that_does_not_fit(engine: KbrEngine):
    b, ref, _ = small_ref(9, TM.SYMMETRIC, 4)
    tp, dp = tparams(TM.SYMMETRIC, 4), DhtParams.default().replace(numReplica=8)
    load(engine, 9)
    for j, (g, r) in enumerate(zip(run_device(engine, b, tp, dp), ref)):
        K.same_result(g, r, j % 2 == 0, ("device", j))
    assert engine.dht_store_count()[1] == 0
    # a store with room for nothing more: the put batch changes nothing
    used = engine.dht_store_count()[0]
    before = [engine.dht_dump(v, 0) for v in range(9)]
    engine.dht_store_create(8)
    _, keys, src, put = K.sequence(b)[0]
    with pytest.raises(KbrError, match="ENOMEM|too small"):
        engine.dht_team_put(keys, src, put, tp, dp)
    assert engine.dht_store_count() == (0, 1)
    dt = DHT_PUT_DTYPE
    n = len(src)
    do, dteam = torch.zeros(n * dt.itemsize, dtype=torch.uint8, device="cuda"), torch.zeros(n * 4 * dt.itemsize, dtype=torch.uint8, device="cuda")
    dw = torch.zeros(n, dtype=torch.int32, device="cuda")
    dk, ds, dop = dev(keys), dev(src), dev(put)
    engine.dht_team_device(True, dk.data_ptr(), ds.data_ptr(), dop.data_ptr(), n, do.data_ptr(), dteam.data_ptr(), dw.data_ptr(), tp, dp)
    torch.cuda.synchronize()
    assert engine.dht_store_count() == (0, 2)
    assert all(len(engine.dht_dump(v, 0)) == 0 for v in range(9))
    assert used > 0 and any(len(d) for d in before)


def test_refusals_leave_the_store_and_a_plain_get_unchanged(engine: KbrEngine):
    b, _, _ = small_ref(9, TM.SYMMETRIC, 4)
    _, keys, src, put = K.sequence(b)[0]
    dp4 = DhtParams.default()
    load(engine, 9)
    engine.dht_put(keys, src, put, dp4)
    get = K.sequence(b)[1][3]
    want, count = engine.dht_get(keys, src, get, dp4), engine.dht_store_count()
    dumps = [engine.dht_dump(v, 0) for v in range(9)]
    dp8 = dp4.replace(numReplica=8)

    def refused(status, tp, dp, **params):
        if params:
            engine.set_params(Params.chord().replace(simtimeRound=1, **params))
        for fn in (engine.dht_team_put, engine.dht_team_get):
            with pytest.raises(KbrError, match=status):
                fn(keys, src, put, tp, dp)
        if params:
            engine.set_params(Params.chord().replace(simtimeRound=1))

    refused("EINVAL", tparams(TM.SYMMETRIC, 3), dp8)                                  # numReplica % T != 0
    refused("ENOTSUP", tparams(TM.SYMMETRIC, 0), dp8)
    refused("ENOTSUP", tparams(TM.SYMMETRIC, 9), dp8.replace(numReplica=9))
    refused("ENOTSUP", tparams(2, 4), dp8)
    refused("ENOTSUP", tparams(TM.SYMMETRIC, 1), dp8.replace(numReplica=16))            # numReplica > 8
    refused("ENOTSUP.*numReplica", tparams(TM.SYMMETRIC, 2), dp8.replace(numReplica=16))  # ... all teams together
    refused("ENOTSUP.*numReplica", tparams(TM.SYMMETRIC, 8), dp8.replace(numReplica=16))
    refused("ENOTSUP", tparams(TM.SYMMETRIC, 2), dp8, successorListSize=3)              # numReplica / T > getMaxNumSiblings()
    refused("ENOTSUP", tparams(TM.SYMMETRIC, 4), dp8, routingType=1)
    refused("ENOTSUP", tparams(TM.SYMMETRIC, 4), dp8, lookupParallelRpcs=2)
    refused("ENOTSUP", tparams(TM.SYMMETRIC, 4), dp8, hopCountMax=0)
    refused("ENOTSUP", tparams(TM.SYMMETRIC, 4), dp8.replace(secureMaintenance=1))
    refused("ENOTSUP", tparams(TM.SYMMETRIC, 4), dp8.replace(numGetRequests=0))
    zero_id = put.copy()
    zero_id["id"][3] = 0
    with pytest.raises(KbrError, match="ENOTSUP"):
        engine.dht_team_put(keys, src, zero_id, tparams(TM.SYMMETRIC, 4), dp8)
    assert engine.dht_store_count() == count
    for v, d in enumerate(dumps):
        assert np.array_equal(engine.dht_dump(v, 0), d)
    got = engine.dht_get(keys, src, get, dp4)
    K.same(got, want, D.GET_FIELDS, "plain get after the refusals")


def test_kademlia_and_explicit_tables_are_refused(engine: KbrEngine):
    from test_gpu_chord import _broken_tables
    b, _, _ = small_ref(9, TM.SYMMETRIC, 4)
    _, keys, src, put = K.sequence(b)[0]
    tp, dp = tparams(TM.SYMMETRIC, 4), DhtParams.default().replace(numReplica=8)
    net = K.ring(64)
    s64 = src % 64
    engine.set_params(Params.kademlia().replace(lookupParallelRpcs=1))
    engine.kad_load(net.ids, net.xy)
    engine.dht_store_create(CAP)
    with pytest.raises(KbrError, match="ENOTSUP.*Kademlia"):
        engine.dht_team_put(keys, s64, put, tp, dp)
    net, t = _broken_tables(1000, 33)
    with KbrEngine(0) as chord:
        chord.set_params(Params.chord())
        chord.chord_load_tables(net.ids, net.xy, t["pred"], t["succ"], t["nsucc"], t["fingers"], t["deque_size"])
        chord.dht_store_create(CAP)
        with pytest.raises(KbrError, match="ENOTSUP.*explicit"):
            chord.dht_team_get(keys, src, put, tp, dp)
        assert chord.dht_store_count() == (0, 0)


def test_team_statistics_equal_the_python_reduction(engine: KbrEngine):
    b, ref = low_ref()
    keys, src, put, get1 = b[0], b[1], b[2], b[3]
    (po, pt, _), (go, gt, _) = ref[0], ref[1]
    ex = np.zeros(len(src), dtype=D.EXPECT_DTYPE)
    ex["token"], ex["endtime_ns"], ex["known"] = put["token"], put["t0_ns"] + 60 * SEC, np.arange(len(src)) % 9 != 0
    want = TM.team_stats(1000, po, pt, src, go, gt, get1, src, ex, 7.0)
    load(engine, 1000)
    st = engine.dhttest_team_stats(tparams(TM.SYMMETRIC, 4), po, pt, src, go, gt, get1, src, ex, 7.0)
    for f in D.STAT_INTS:
        assert int(getattr(st, f)) == want[f], f
    for f in D.STAT_SDS:
        sd = getattr(st, f)
        assert sd.count == want[f]["count"], f
        # as tests/test_gpu_dht.py compares the DHT tier's cStdDevs: a handful of double operations on exact integer
        # sums, 1e-12 relative leaves room for the order of the sums, nothing else
        for a in ("mean", "stddev", "min", "max"):
            assert getattr(sd, a) == pytest.approx(want[f][a], rel=1e-12, abs=1e-15), (f, a)
    assert want["put_hop_count"] > want["num_put_success"] + want["num_put_error"]   # one sample per team, not per operation


def test_golden_fixture(engine: KbrEngine):
    g = np.load(K.GOLD / "dht_teams_n1000.npz")
    load(engine, 1000)
    for name, mode, T in (("sym", TM.SYMMETRIC, 4), ("rh", TM.REPEATED_HASHING, 2)):
        tp, dp = tparams(mode, T), DhtParams.default().replace(numReplica=8)
        engine.dht_store_clear()
        assert np.array_equal(engine.dht_team_keys(g["keys"], tp), g[name + "_team_keys"])
        p = engine.dht_team_put(g["keys"], g["src"], g["put_ops"].view(D.OP_DTYPE), tp, dp)
        q = engine.dht_team_get(g["keys"], g["src"], g["get_ops"].view(D.OP_DTYPE), tp, dp)
        for got, what, dt in ((p, "put", D.PUT_DTYPE), (q, "get", D.GET_DTYPE)):
            assert np.array_equal(got[0].view(np.uint8), g[f"{name}_{what}_out"].view(np.uint8)), (name, what)
            assert np.array_equal(got[1].reshape(-1).view(np.uint8), g[f"{name}_{what}_team"].view(np.uint8)), (name, what)
            assert np.array_equal(got[2], g[f"{name}_{what}_winner"]), (name, what)
