"""The KBRTestApp RPC test on the GPU (ovs_rpc_batch; k_rpc_finish / k_rpc_fold, oversim_amd/csrc/kbr_rpc.hip):
every ovs_rpc_out field bit-exact against tests/refmodel_rpc.py, whose call and return legs come from the
CPU oracle here (tests/test_refmodel_rpc.py ties its own message-by-message Chord legs to the oracle)."""
from __future__ import annotations

import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import refmodel_rpc as R
from oracle_lib import OracleNet, chord_params, kad_params, koorde_params
from oversim_amd import RPC_OUT_DTYPE, KbrEngine, KbrError, Params, workload as W
from test_kad_recursive import _perturbed_tables

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
NONE = 0xFFFFFFFF
SIZES = (1, 63, 257, 1000)          # no batch a multiple of a wave (64) or a block (256)


@functools.lru_cache(maxsize=None)
def ring(n):
    return W.population(n, 0x5250 + n)


def batch(net, m, seed):
    """Half node-ID keys, half uniform keys; the first RPCs go to the caller's own key."""
    k1, s1 = W.lookups(net.ids, m // 2, seed, node_ids=True)
    k2, s2 = W.lookups(net.ids, m - m // 2, seed + 1, node_ids=False)
    keys, src = np.concatenate([k1, k2]), np.concatenate([s1, s2])
    own = min(4, m)
    keys[:own] = net.ids[src[:own]]
    return np.ascontiguousarray(keys), np.ascontiguousarray(src)


@functools.lru_cache(maxsize=None)
def chord_ref(n, rt, rnd, hcm=50, timeout=10.0, m=1000, seed=21):
    net = ring(n)
    keys, src = batch(net, m, seed)
    o = OracleNet("chord", net.ids, net.xy, chord_params(routingType=rt, simtimeRound=rnd, hopCountMax=hcm))
    ref = R.rpc_batch(net.ids, net.xy, keys, src, R.oracle_leg(o), rt, bool(rnd), rpc_key_timeout=timeout)
    ref.setflags(write=False)
    return keys, src, ref


def same(got: dict, ref: np.ndarray, what=""):
    for f in R.FIELDS:
        a, b = np.asarray(got[f]).astype(np.int64), ref[f].astype(np.int64)
        assert np.array_equal(a, b), (what, f, np.flatnonzero(a != b)[:5])
    assert not np.asarray(got["pad"]).any()


def load_chord(engine, n, rt, rnd, hcm=50, timeout=10.0):
    net = ring(n)
    engine.set_params(Params.chord().replace(routingType=rt, simtimeRound=rnd, hopCountMax=hcm, rpcKeyTimeout=timeout))
    engine.chord_load(net.ids, net.xy)
    return net


def device_call(engine, keys, src):
    dk = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    ds = torch.from_numpy(src.view(np.int32).copy()).cuda()
    do = torch.full((len(src) * 32,), 0x5A, dtype=torch.uint8, device="cuda")
    engine.rpc_device(dk.data_ptr(), ds.data_ptr(), len(src), do.data_ptr())
    torch.cuda.synchronize()
    out = do.cpu().numpy().view(RPC_OUT_DTYPE)
    return {f: out[f] for f in RPC_OUT_DTYPE.names}


@pytest.mark.parametrize("n", [2, 3, 9, 1000])
@pytest.mark.parametrize("rt", [0, 1, 2])
@pytest.mark.parametrize("rnd", [0, 1])
def test_chord_rings(engine: KbrEngine, n, rt, rnd):
    keys, src, ref = chord_ref(n, rt, rnd)
    own = np.all(keys == ring(n).ids[src], axis=1)
    assert own.sum() > 0 and (ref["rtt_ns"][own] == 0).all() and (ref["hop_count"][own] == 0).all()
    assert (ref["outcome"][own] == R.ANSWERED).all() and (ref["outcome"] == R.ANSWERED).sum() > len(ref) // 2
    load_chord(engine, n, rt, rnd)
    for m in SIZES:
        same(engine.rpcCall(keys[:m], src[:m]), ref[:m], ("host", m))
    for m in (63, 1000):
        same(device_call(engine, keys[:m], src[:m]), ref[:m], ("device", m))


@pytest.mark.parametrize("rt", [0, 1, 2])
def test_timeouts_between_the_smallest_and_largest_rtt(engine: KbrEngine, rt):
    keys, src, free = chord_ref(1000, rt, 1)
    rtts = np.sort(free["rtt_ns"][free["rtt_ns"] > 0])
    limit_ns = int(rtts[len(rtts) // 2])
    limit = limit_ns * 1e-9
    assert R.simtime(limit, True) == limit_ns and rtts[0] < limit_ns < rtts[-1]
    _, _, ref = chord_ref(1000, rt, 1, 50, limit)
    assert (ref["outcome"] == R.ANSWERED).any() and (ref["outcome"] == R.TIMEOUT).any()
    # the RPC whose response arrives at the very instant of the timeout: timed out (the timeout event was
    # scheduled first); and RPCs within one hop's delay of the limit, taking the response's 2 x 106.4 us
    # serialisation as the least a hop costs
    tie = free["rtt_ns"] == limit_ns
    assert tie.any() and (ref["outcome"][tie] == R.TIMEOUT).all()
    assert (np.abs(free["rtt_ns"] - limit_ns) <= 2 * R.simtime(133 * 8 / 10e6, True)).sum() > 0
    load_chord(engine, 1000, rt, 1, 50, limit)
    for m in (257, 1000):
        same(engine.rpcCall(keys[:m], src[:m]), ref[:m], m)
    same(device_call(engine, keys, src), ref, "device")


@pytest.mark.parametrize("rt", [0, 1, 2])
@pytest.mark.parametrize("rnd", [0, 1])
def test_dropped_routes_with_hop_count_max_3(engine: KbrEngine, rt, rnd):
    keys, src, ref = chord_ref(1000, rt, rnd, 3)
    assert (ref["status"] != 0).sum() > 0 and (ref["status"] == 0).sum() > 0
    assert ((ref["status"] != 0) == (ref["responder"] == NONE)).all()
    if rt == 2:     # a call that arrived whose response is dropped on the way back
        assert ((ref["status"] == 0) & (ref["resp_status"] != 0)).sum() > 0
        assert ((ref["status"] == 0) & (ref["outcome"] == R.ANSWERED)).sum() > 0
    load_chord(engine, 1000, rt, rnd, 3)
    for m in (63, 1000):
        same(engine.rpcCall(keys[:m], src[:m]), ref[:m], m)
    same(device_call(engine, keys[:257], src[:257]), ref[:257], "device")


@pytest.mark.parametrize("alpha", [1, 3])
def test_kademlia_iterative(engine: KbrEngine, alpha):
    net = W.population(2000, 0x4b52)
    keys, src = batch(net, 1000, 31)
    engine.set_params(Params.kademlia().replace(lookupParallelRpcs=alpha))
    engine.kad_load(net.ids, net.xy)
    o = OracleNet("kademlia", net.ids, net.xy, kad_params(lookupParallelRpcs=alpha))
    ref = R.rpc_batch(net.ids, net.xy, keys, src, R.oracle_leg(o), 0)
    assert (ref["outcome"] == R.ANSWERED).sum() > 900
    same(engine.rpcCall(keys, src), ref)
    same(device_call(engine, keys[:257], src[:257]), ref[:257], "device")


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("rt", [1, 2])
def test_kademlia_recursive_on_explicit_tables(engine: KbrEngine, b, rt):
    net, t = _perturbed_tables(1500, 0x4b70 + b, b)
    p = dict(b=b, routingType=rt, hopCountMax=12)
    engine.set_params(Params.kademlia().replace(**p))
    engine.kad_load_tables_csr(net.ids, net.xy, t["siblings"], t["bucket_off"], t["bucket_nodes"])
    o = OracleNet("kademlia", net.ids, net.xy, kad_params(**p), tables=t)
    keys, src = batch(net, 1000, 33)
    ref = R.rpc_batch(net.ids, net.xy, keys, src, R.oracle_leg(o), rt)
    assert (ref["outcome"] == R.ANSWERED).any()
    same(engine.rpcCall(keys, src), ref)


def test_kademlia_recursive_k_stride_tables(engine: KbrEngine):
    net, t = _perturbed_tables(1500, 0x4b72, 1)
    sib, cnt, nodes = OracleNet("kademlia", net.ids, net.xy, kad_params(), tables=t).kad_tables()
    p = dict(routingType=2, hopCountMax=12)
    engine.set_params(Params.kademlia().replace(**p))
    engine.kad_load_tables(net.ids, net.xy, sib, cnt, nodes)
    o = OracleNet("kademlia", net.ids, net.xy, kad_params(**p),
                  tables=dict(siblings=sib, bucket_count=cnt, bucket_nodes=nodes))
    keys, src = batch(net, 1000, 34)
    ref = R.rpc_batch(net.ids, net.xy, keys, src, R.oracle_leg(o), 2)
    same(engine.rpcCall(keys, src), ref)


def test_koorde_iterative(engine: KbrEngine):
    net = W.population(1000, 0x4b6f)
    keys, src = batch(net, 1000, 35)
    engine.set_params(Params.koorde())
    engine.koorde_load(net.ids, net.xy)
    ref = R.rpc_batch(net.ids, net.xy, keys, src, R.oracle_leg(OracleNet("koorde", net.ids, net.xy, koorde_params())), 0)
    assert (ref["outcome"] == R.ANSWERED).sum() > 900
    same(engine.rpcCall(keys, src), ref)


def test_golden_fixture(engine: KbrEngine):
    g = np.load(GOLD / "rpc_chord_n1000.npz")
    for rt in (0, 2):
        engine.set_params(Params.chord().replace(routingType=rt, simtimeRound=int(g["simtime_round"]),
                                                 hopCountMax=int(g["hop_count_max"]),
                                                 rpcKeyTimeout=float(g["rpc_key_timeout"])))
        engine.chord_load(g["ids"], g["xy"])
        got = engine.rpcCall(g["keys"], g["src"])
        for f in R.FIELDS:
            assert np.array_equal(np.asarray(got[f]).astype(np.int64), g[f"rt{rt}_{f}"].astype(np.int64)), (rt, f)
        ref = g[f"rt{rt}_outcome"]
        assert (ref == R.ANSWERED).any() and (ref == R.TIMEOUT).any()


# ---------------------------------------------------------------- refusals
def test_refusals_leave_results_unchanged(engine: KbrEngine):
    net = W.population(500, 31)
    keys, src = batch(net, 100, 5)
    engine.set_params(Params.kademlia().replace(routingType=1))
    engine.kad_load(net.ids, net.xy)
    ok = engine.rpcCall(keys, src)

    def unchanged():
        again = engine.rpcCall(keys, src)
        assert all(np.array_equal(ok[f], again[f]) for f in ok)

    for bad in (len(net.ids), NONE):
        s2 = src.copy()
        s2[57] = bad
        with pytest.raises(KbrError, match="EINVAL: source index out of range"):
            engine.rpcCall(keys, s2)
        unchanged()
    engine.set_params(Params.kademlia().replace(routingType=4))
    engine.lookup(keys, src)                                  # the one-way route takes routingType 4 ...
    with pytest.raises(KbrError, match="ENOTSUP: .*recorded hops back"):
        engine.rpcCall(keys, src)                             # ... the RPC's way back is not built
    engine.set_params(Params.kademlia().replace(routingType=3))
    with pytest.raises(KbrError, match="ENOTSUP"):
        engine.rpcCall(keys, src)
    engine.set_params(Params.kademlia().replace(routingType=1))
    unchanged()
    assert all(len(v) == 0 for v in engine.rpcCall(np.zeros((0, 5), np.uint32), np.zeros(0, np.uint32)).values())


def test_refused_on_a_shard_context_as_the_route_is(engine: KbrEngine):
    net = W.population(400, 35)
    engine.set_params(Params.chord())
    xy = np.ascontiguousarray(net.xy)
    st = engine._L.ovs_chord_load_shard(engine._h, net.ids.ctypes.data_as(C.c_void_p), C.c_uint64(400),
                                        xy.ctypes.data_as(C.c_void_p), C.c_uint64(100), C.c_uint64(300), C.c_uint32(0))
    assert st == 0
    engine.n = 400
    keys, src = batch(net, 10, 5)
    msgs = []
    for call in (engine.lookup, engine.rpcCall):
        with pytest.raises(KbrError, match="ESTATE: .*sharded ring") as e:
            call(keys, src)
        msgs.append(str(e.value).split(": ", 1)[1])
    assert msgs[0] == msgs[1]


def test_refused_on_epichord_as_the_route_is():
    from epichord_snap import make_snapshot
    snap = make_snapshot(500, 31, list_size=4)
    n = snap["n"]
    with KbrEngine(0) as eng:
        eng.set_params(Params.epichord().replace(successorListSize=snap["L"], cacheTTL=snap["cache_ttl_param"] / 10**9))
        eng.epichord_load(snap["ids"], np.zeros((n, 2)), snap["succ"], snap["nsucc"], snap["pred"], snap["npred"],
                          snap["full"], snap["cache_off"], snap["cache_node"], snap["cache_last"], snap["cache_ttl"])
        keys, src = np.ascontiguousarray(snap["ids"][:10]), np.arange(10, dtype=np.uint32)
        msgs = []
        for call in (eng.lookup, eng.rpcCall):
            with pytest.raises(KbrError, match="ENOTSUP: EpiChord") as e:
                call(keys, src)
            msgs.append(str(e.value).split(": ", 1)[1])
        assert msgs[0] == msgs[1]
