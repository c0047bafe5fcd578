"""Pastry routes with per-hop acks and KBRTestApp's RPC test on the GPU (k_pastry_route<true>, oversim_amd/csrc/
pastry.hip; ovs_pastry_acked_route_batch, ovs_pastry_rpc_batch) against the event replay of
tests/refmodel_pastry_acks.py, bit for bit on every field: route record, hop sequence, ack record, RPC record."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import refmodel_pastry as RP
import refmodel_pastry_acks as RA
import refmodel_rpc as RR
from oversim_amd import KbrEngine, KbrError, BrooseParams, Params, PastryParams, workload as W
from refmodel import simtime
from test_pastry_acks_model import ack_timeout_case

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
ROUTE = ("responsible", "hops", "status", "one_way_hops", "latency_ns")
ACK = ("acks", "max_ack_rtt_ns", "timeout_hop")


@functools.lru_cache(maxsize=None)
def _pop(n):
    return W.population(n, 81)


@functools.lru_cache(maxsize=None)
def _batch(n, nq=1024, seed=92):
    rng = np.random.default_rng(seed)
    keys = W.random_keys(nq, rng)
    keys[::4] = _pop(n).ids[rng.integers(0, n, len(keys[::4]))]
    return keys, rng.integers(0, n, nq).astype(np.uint32)


def _load(engine, n, acks=1, b=4, L=16, opt=0, reg=1, **pk):
    net = _pop(n)
    engine.set_params(Params.pastry().replace(**pk))
    engine.pastry_load(net.ids, net.xy, PastryParams.default(routeMsgAcks=acks, bitsPerDigit=b, numberOfLeaves=L, optimizeLookup=opt,
                                                             useRegularNextHop=reg))
    return net, RP.PastryNet(net.ids, net.xy, b, L, bool(opt), bool(reg), rnd=bool(pk.get("simtimeRound", 1)))


def _model_kw(pk):
    return dict(rec_num_redundant=pk.get("recNumRedundantNodes", 3), hop_max=pk.get("hopCountMax", 50),
                auth=bool(pk.get("measureAuthBlock", 0)), rpc_to=pk.get("rpcUdpTimeout", 1.5))


def _assert(got, want, fields, what):
    for f in fields:
        bad = np.flatnonzero(np.asarray(got[f]) != np.asarray(want[f]))
        assert bad.size == 0, (what, f, bad[:5], np.asarray(got[f])[bad[:5]], np.asarray(want[f])[bad[:5]])


def _check_routes(engine, m, keys, src, pk, what, hop_seq=True):
    want = RA.routes(m, keys, src, **_model_kw(pk))
    got = engine.pastry_acked_lookup(keys, src, record_hops=hop_seq)
    _assert(got, want, ROUTE + ACK + (("hop_seq",) if hop_seq else ()), what)
    return got, want


@pytest.mark.parametrize("n", [2, 3, 9, 17])
def test_small_networks(engine: KbrEngine, n):
    net, m = _load(engine, n)
    keys, src = _batch(n)
    got, want = _check_routes(engine, m, keys, src, {}, f"n={n}")
    assert (want["acks"] > 0).any()


@pytest.mark.parametrize("kw", [dict(b=1), dict(b=2), dict(b=4), dict(opt=1), dict(reg=0), dict(recNumRedundantNodes=1),
                                dict(simtimeRound=0), dict(measureAuthBlock=1), dict(hopCountMax=1), dict(hopCountMax=3),
                                dict(b=2, simtimeRound=0, measureAuthBlock=1, recNumRedundantNodes=1)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_acked_routes_main_matrix(engine: KbrEngine, kw):
    kw = dict(kw)
    shape = {k: kw.pop(k) for k in ("b", "opt", "reg") if k in kw}
    net, m = _load(engine, 1000, **shape, **kw)
    keys, src = _batch(1000)
    got, want = _check_routes(engine, m, keys, src, kw, str(kw))
    if kw.get("hopCountMax", 50) > 1:
        assert (want["acks"] >= 2).sum() > 100                    # forwarders: the queueing term is live
    if "hopCountMax" in kw:
        cut = want["status"] == RP.HOPMAX
        assert cut.sum() > 0 and (want["acks"][cut] == kw["hopCountMax"]).all() and (want["max_ack_rtt_ns"][cut] > 0).all()
    # without the hop sequence, and without the ack records
    _assert(engine.pastry_acked_lookup(keys, src), want, ROUTE + ACK, str(kw) + " no hop_seq")
    bare = engine.pastry_acked_lookup(keys, src, ack_records=False)
    assert set(bare) == set(ROUTE)
    _assert(bare, want, ROUTE, str(kw) + " ack_out NULL")


def test_thinned_explicit_tables(engine: KbrEngine):
    """30 % of the table slots emptied, as tests/test_gpu_pastry.py builds them: the closer-node path under acks.  A
    route that failed part-way would have sent, and had acknowledged, the calls of its hops; on these tables the
    model delivers every route (whole leaf sets always hold a closer node), so the HOPMAX cases of the main matrix
    are the failed routes with acks."""
    net, m = _load(engine, 1000)
    leaf, tab = engine.pastry_export()
    thin = tab.copy()
    thin[np.random.default_rng(85).random(tab.shape) < 0.3] = NONE
    engine.pastry_load_tables(net.ids, net.xy, leaf, thin, PastryParams.default())
    sm = RP.PastryNet(net.ids, net.xy, tables=(leaf, thin))
    keys, src = _batch(1000)
    for rnr in (1, 3):
        engine.set_params(Params.pastry().replace(recNumRedundantNodes=rnr))
        got, want = _check_routes(engine, sm, keys, src, dict(recNumRedundantNodes=rnr), f"thin rnr={rnr}")
    print("thinned: status", {int(s): int((want["status"] == s).sum()) for s in np.unique(want["status"])},
          "failed with acks", int(((want["status"] != 0) & (want["acks"] > 0)).sum()))


def test_without_acks_equals_the_plain_route(engine: KbrEngine):
    net, m = _load(engine, 1000, acks=0)
    keys, src = _batch(1000)
    plain = engine.pastry_lookup(keys, src, record_hops=True)
    got = engine.pastry_acked_lookup(keys, src, record_hops=True)
    _assert(got, plain, ROUTE + ("hop_seq",), "routeMsgAcks=0")
    assert (got["acks"] == 0).all() and (got["max_ack_rtt_ns"] == -1).all() and (got["timeout_hop"] == 0xFF).all()
    want = RA.routes(m, keys, src, acks=False)
    _assert(got, want, ROUTE + ACK + ("hop_seq",), "routeMsgAcks=0 model")


@pytest.mark.parametrize("hcm", [50, 3])
@pytest.mark.parametrize("n", [9, 1000])
def test_acked_and_plain_instantiations_share_their_paths(engine: KbrEngine, n, hcm):
    """k_pastry_route<true> (routeMsgAcks = 1 through pastry_acked_lookup) and k_pastry_route<false> (routeMsgAcks = 0
    through pastry_lookup) on the same tables and batch take the same paths to the same ends; only latency_ns, which
    the acks lengthen by design, is left out.  hopCountMax = 3 cuts routes of the 1000-node network at the limit."""
    keys, src = _batch(n)
    _load(engine, n, acks=1, hopCountMax=hcm)
    acked = engine.pastry_acked_lookup(keys, src, record_hops=True)
    _load(engine, n, acks=0, hopCountMax=hcm)
    plain = engine.pastry_lookup(keys, src, record_hops=True)
    _assert(acked, plain, ("responsible", "hops", "status", "one_way_hops", "hop_seq"), f"n={n} hopCountMax={hcm}")
    assert (acked["acks"] > 0).any()                              # the acked instantiation ran
    if n == 1000 and hcm == 3:
        assert (plain["status"] == RP.HOPMAX).any()


@pytest.mark.parametrize("acks", [1, 0])
def test_iterative_routing(engine: KbrEngine, acks):
    pk = dict(routingType=0, measureAuthBlock=1)
    net, m = _load(engine, 1000, acks=acks, **pk)
    keys, src = _batch(1000)
    got = engine.pastry_acked_lookup(keys, src, record_hops=True)
    want = RA.iterative_routes(m, keys, src, acks=bool(acks), auth=True)
    _assert(got, want, ROUTE + ACK + ("hop_seq",), f"iterative acks={acks}")
    assert acks == 0 or (want["acks"] == 1).sum() > 900
    # the lookup is ovs_pastry_iterative_route_batch's
    engine.pastry_load(net.ids, net.xy, PastryParams.default(routeMsgAcks=0))
    it = engine.pastry_iterative_lookup(keys, src, record_hops=True)
    _assert(got, it, ("responsible", "hops", "status", "one_way_hops", "hop_seq"), "iterative lookup")
    if not acks:
        assert np.array_equal(got["latency_ns"], it["latency_ns"])


def test_ack_timeouts_with_a_tie(engine: KbrEngine):
    m, keys, src, rpc_to, tie = ack_timeout_case()
    pk = dict(rpcUdpTimeout=rpc_to)
    net, _ = _load(engine, 1000, **pk)
    got, want = _check_routes(engine, m, keys, src, pk, "ack timeout")
    T = simtime(rpc_to, True)
    assert want["max_ack_rtt_ns"][tie] == T and want["timeout_hop"][tie] != 0xFF
    assert 0 < (want["timeout_hop"] != 0xFF).sum() < len(keys)
    engine.set_params(Params.pastry())
    base = engine.pastry_acked_lookup(keys, src, record_hops=True)
    _assert(got, base, ROUTE + ("hop_seq", "acks", "max_ack_rtt_ns"), "the route record is unchanged by the timeout")
    assert (base["timeout_hop"] == 0xFF).all()


def _stats_check(gpu, ref):
    for f in RR.INT_FIELDS:
        assert int(getattr(gpu, f)) == int(ref[f]), f
    assert list(gpu.status_count) == ref["status_count"] and list(gpu.hop_hist) == ref["hop_hist"]
    for f in ("hop_count_mean", "success_latency_mean_s", "total_latency_mean_s"):
        assert getattr(gpu, f) == pytest.approx(ref[f], rel=1e-12), f
    for f in RR.SD_FIELDS:
        g, o = getattr(gpu, f), ref[f]
        assert g.count == o["count"], f
        for k in ("mean", "stddev", "min", "max"):
            assert getattr(g, k) == pytest.approx(o[k], rel=1e-12, abs=1e-12), (f, k)


@pytest.mark.parametrize("acks", [1, 0])
@pytest.mark.parametrize("n", [2, 9, 1000])
def test_pastry_rpc(engine: KbrEngine, n, acks):
    net, m = _load(engine, n, acks=acks, measureAuthBlock=1)
    keys, src = _batch(n, 512)
    want = RA.rpc_batch(m, keys, src, bool(acks), auth=True)
    got = engine.pastry_rpc(keys, src)
    _assert(got, want, RR.FIELDS, f"rpc n={n} acks={acks}")
    assert (want["outcome"] == RR.ANSWERED).all()
    # rpcKeyTimeout inside the batch's round trips, at one RPC's exact round trip
    rtt = np.sort(want["rtt_ns"][want["rtt_ns"] > 0])
    t_ns = int(rtt[len(rtt) // 2])
    assert simtime(t_ns * 1e-9, True) == t_ns
    engine.set_params(Params.pastry().replace(measureAuthBlock=1, rpcKeyTimeout=t_ns * 1e-9))
    want = RA.rpc_batch(m, keys, src, bool(acks), auth=True, rpc_key_timeout=t_ns * 1e-9)
    got = engine.pastry_rpc(keys, src)
    _assert(got, want, RR.FIELDS, f"rpc timeout n={n} acks={acks}")
    late = want["outcome"] == RR.TIMEOUT
    assert 0 < late.sum() < len(keys) and (want["rtt_ns"] != t_ns).all()       # the tie is a timeout
    if n == 1000:
        st = engine.kbrtest_rpc_stats(got, keys, src, 120.0, failureLatency=7.5)
        _stats_check(st, RR.rpc_stats(want, net.ids, keys, src, 120.0, failure_latency=7.5))
        one = engine.pastry_acked_lookup(keys, src)
        assert engine.kbrtest_stats(one, keys, src, 120.0).num_sent == len(keys)


def test_scheduler_static_slices_and_dynamic_tail(engine: KbrEngine):
    """70 000 routes: more than one static slice and the dynamic tail; the same batch in four parts."""
    net, m = _load(engine, 1000)
    keys, src = _batch(1000, 70000, 93)
    whole = engine.pastry_acked_lookup(keys, src, record_hops=True)
    for lo, hi in ((0, 17500), (17500, 35001), (35001, 52000), (52000, 70000)):
        part = engine.pastry_acked_lookup(keys[lo:hi], src[lo:hi], record_hops=True)
        _assert(part, {f: v[lo:hi] for f, v in whole.items()}, ROUTE + ACK + ("hop_seq",), f"part {lo}")
    want = RA.routes(m, keys[-512:], src[-512:])
    _assert({f: v[-512:] for f, v in whole.items()}, want, ROUTE + ACK + ("hop_seq",), "tail against the model")


def test_refusals_and_pinned_behaviour(engine: KbrEngine):
    net, m = _load(engine, 1000)
    keys, src = _batch(1000, 64)
    base = engine.pastry_acked_lookup(keys, src)
    rpc = engine.pastry_rpc(keys, src)

    def refused(fn, match="ENOTSUP"):
        with pytest.raises(KbrError, match=match):
            fn()
        engine.set_params(Params.pastry())
        again = engine.pastry_acked_lookup(keys, src)                 # a refused call leaves the tables usable
        _assert(again, base, ROUTE + ACK, "after " + match)
        assert np.array_equal(engine.pastry_rpc(keys, src)["rtt_ns"], rpc["rtt_ns"])

    for kw, word in ((dict(routingType=2), "full-recursive"), (dict(routingType=4), "source-routing"),
                     (dict(numSiblings=2), "numSiblings"), (dict(recNumRedundantNodes=9), "recNumRedundantNodes"),
                     (dict(testMsgSize=1000000), "sendQueueLength")):
        for call in (engine.pastry_acked_lookup, engine.pastry_rpc):
            engine.set_params(Params.pastry().replace(**kw))
            refused(lambda: call(keys, src), "ENOTSUP: .*" + word)
    engine.set_params(Params.pastry().replace(routingType=0))
    refused(lambda: engine.pastry_rpc(keys, src), "ENOTSUP: .*semi-recursive")
    # the calls without acks keep refusing the default flag
    refused(lambda: engine.pastry_lookup(keys, src), "routeMsgAcks")
    refused(lambda: engine.rpcCall(keys, src), "Pastry: ovs_pastry_route_batch")
    engine.set_params(Params.pastry().replace(routingType=0))
    refused(lambda: engine.pastry_iterative_lookup(keys, src), "routeMsgAcks")


def test_other_overlays_are_refused(engine: KbrEngine):
    net = _pop(1000)
    keys, src = _batch(1000, 16)

    def both(eng, match):
        for call in (eng.pastry_acked_lookup, eng.pastry_rpc):
            with pytest.raises(KbrError, match=match):
                call(keys, src)

    both(engine, "ESTATE")                                            # no network
    loads = ((Params.chord(), lambda e: e.chord_load(net.ids, net.xy)),
             (Params.kademlia(), lambda e: e.kad_load(net.ids, net.xy)),
             (Params.broose(), lambda e: e.broose_load(net.ids, net.xy, BrooseParams.default())))
    for params, load in loads:
        with KbrEngine(0) as eng:
            eng.set_params(params)
            load(eng)
            both(eng, "ESTATE: no Pastry network loaded")
            if params.overlay == Params.chord().overlay:
                assert (eng.lookup(keys, src)["status"] == 0).all()   # the context stays usable


def test_sharded_context_is_refused(engine: KbrEngine):
    net = _pop(1000)
    keys, src = _batch(1000, 16)
    engine.set_params(Params.chord())
    xy = np.ascontiguousarray(net.xy)
    st = engine._L.ovs_chord_load_shard(engine._h, net.ids.ctypes.data_as(C.c_void_p), C.c_uint64(1000),
                                        xy.ctypes.data_as(C.c_void_p), C.c_uint64(250), C.c_uint64(750), C.c_uint32(0))
    assert st == 0
    engine.n = 1000
    for call in (engine.pastry_acked_lookup, engine.pastry_rpc):
        with pytest.raises(KbrError, match="ESTATE: no Pastry network loaded"):
            call(keys, src)
