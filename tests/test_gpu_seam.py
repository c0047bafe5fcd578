"""The application tiers on the route and lookup seam (ctx.hpp: route_check / lookup_check): the refusals
a tier inherits from the router come out with the router's status and literal message, for an empty
batch and for a non-empty one, before the tier's own later refusals; and a multicast, which routes under
its own message length, leaves the context's parameters as they were.  200 nodes."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from oversim_amd import KbrEngine, KbrError, Params, workload as W
from oversim_amd.kbr import DHT_OP_DTYPE
from scribe_cases import messages, scenario

pytestmark = pytest.mark.gpu
N = 200
MERGE = r"EINVAL: Chord doesn't work with iterativeLookupConfig\.merge = true!$"
NO_KEYS, NO_U32 = np.zeros((0, 5), np.uint32), np.zeros(0, np.uint32)


@pytest.fixture(scope="module")
def net():
    return W.population(N, 41)


def _batch(net, n=8):
    return np.ascontiguousarray(net.ids[:n]), np.arange(n, dtype=np.uint32)


def _both(call, empty, full, match):
    """the same refusal for an empty batch and for a non-empty one"""
    for args in (empty, full):
        with pytest.raises(KbrError, match=match):
            call(*args)


def test_rpc_inherits_the_routes_refusals(net):
    keys, src = _batch(net)
    # Kademlia, numSiblings = 2: the route's refusal, before the RPC test's own of routingType = 4
    with KbrEngine(0) as e:
        e.set_params(Params.kademlia().replace(numSiblings=2, routingType=4))
        e.kad_load(net.ids, net.xy)
        _both(e.rpcCall, (NO_KEYS, NO_U32), (keys, src),
              r"ENOTSUP: the one-way route implements numSiblings = 1 \(LookupCall: ovs_lookup_batch\)$")
        e.set_params(Params.kademlia().replace(routingType=4))
        _both(e.rpcCall, (NO_KEYS, NO_U32), (keys, src), "ENOTSUP: KbrTestCall under source-routing-recursive routing")
        e.set_params(Params.kademlia())
        assert len(e.rpcCall(NO_KEYS, NO_U32)["status"]) == 0 and len(e.rpcCall(keys, src)["status"]) == len(src)
    with KbrEngine(0) as e:
        e.set_params(Params.koorde().replace(routingType=1))
        e.koorde_load(net.ids, net.xy)
        _both(e.rpcCall, (NO_KEYS, NO_U32), (keys, src), "ENOTSUP: Koorde routing is implemented for routingType = iterative$")
    with KbrEngine(0) as e:
        e.set_params(Params.chord())
        xy = np.ascontiguousarray(net.xy)
        assert e._L.ovs_chord_load_shard(e._h, net.ids.ctypes.data_as(C.c_void_p), C.c_uint64(N), xy.ctypes.data_as(C.c_void_p),
                                         C.c_uint64(50), C.c_uint64(150), C.c_uint32(0)) == 0
        _both(e.rpcCall, (NO_KEYS, NO_U32), (keys, src),
              "ESTATE: context holds one arc of a sharded ring: use ovs_shard_step$")


def test_dht_put_inherits_the_lookupcalls_refusals(engine: KbrEngine, net):
    keys, src = _batch(net)
    ops = np.zeros(len(src), DHT_OP_DTYPE)
    ops["kind"], ops["id"], ops["vlen"], ops["ttl"], ops["token"] = 1, 1, 16, 300, 7
    bad = ops.copy()
    bad["t0_ns"][3] = -1
    none = np.zeros(0, DHT_OP_DTYPE)
    merge = Params.chord().replace(lookupMerge=1)
    engine.set_params(merge)
    engine.chord_load(net.ids, net.xy)
    # the tier's refusals that precede the LookupCall's keep preceding them
    _both(engine.dht_put, (NO_KEYS, NO_U32, none), (keys, src, ops), "ESTATE: no DHT store: ovs_dht_store_create first$")
    engine.dht_store_create(4096)
    # the LookupCall's refusal (check_chord_route under it), before the per-operation checks
    _both(engine.dht_put, (NO_KEYS, NO_U32, none), (keys, src, bad), "ovs_dht_put_batch: " + MERGE)
    _both(engine.dht_get, (NO_KEYS, NO_U32, none), (keys, src, bad), "ovs_dht_get_batch: " + MERGE)
    engine.set_params(Params.chord().replace(lookupRedundantNodes=2))
    _both(engine.dht_put, (NO_KEYS, NO_U32, none), (keys, src, bad),
          "ENOTSUP: Chord route kernel implements lookupRedundantNodes=1, lookupParallelRpcs=1, numSiblings=1$")
    engine.set_params(Params.chord())
    with pytest.raises(KbrError, match="EINVAL: DHT operation with a negative time$"):
        engine.dht_put(keys, src, bad)
    assert len(engine.dht_put(NO_KEYS, NO_U32, none)) == 0
    out = engine.dht_put(keys, src, ops)
    assert len(out) == len(src)


def test_scribe_inherits_the_routes_refusals(engine: KbrEngine):
    """On the whole converged ring Scribe accepts, the route refuses nothing its shared parameter checks
    (check_common, check_chord_route) do not: those are what both calls inherit."""
    ids, xy, gk, members, _ = scenario(N)
    mg, ms, known = messages(N, members)
    good = Params.chord().replace(routingType=1)
    engine.set_params(good)
    engine.chord_load(ids, xy)
    build = lambda g, a, b: engine.scribe_build(g, a, b)
    cast = lambda a, b, k: engine.scribe_multicast(a, b, k, deliveries=False)
    none = (NO_U32, NO_U32, np.zeros(0, np.uint8))
    for bad, match in ((good.replace(lookupMerge=1), "ovs_scribe_\\w+: " + MERGE),
                       (good.replace(numSiblings=2), "ENOTSUP: recursive Chord routing implements numSiblings=1$")):
        engine.scribe_clear()
        engine.set_params(bad)
        # before the tier's own later refusals: a membership out of range, no forest
        _both(build, (NO_KEYS, NO_U32, NO_U32), (gk, [len(gk)], [5]), match)
        _both(cast, none, (mg, ms, known), match)
        engine.set_params(good)
        with pytest.raises(KbrError, match="EINVAL: membership 0: group or node out of range$"):
            engine.scribe_build(gk, [len(gk)], [5])
        _both(cast, none, (mg, ms, known), r"ESTATE: no Scribe forest \(ovs_scribe_build\)$")
        engine.scribe_build(gk, members[:, 0], members[:, 1])
        engine.set_params(bad)
        _both(cast, none, (mg, ms, known), match)
        engine.set_params(good)
        assert len(cast(mg, ms, known)[0]) == len(mg)


def test_a_multicast_leaves_the_parameters_untouched(engine: KbrEngine, net):
    ids, xy, gk, members, _ = scenario(N)
    mg, ms, known = messages(N, members)
    p = Params.chord().replace(routingType=1)
    engine.set_params(p)
    engine.chord_load(ids, xy)
    engine.scribe_build(gk, members[:, 0], members[:, 1])
    keys, src = W.population(64, 5).ids, (np.arange(64, dtype=np.uint32) * 3) % N
    before, lat = bytes(engine.get_params()), engine.lookup(keys, src)["latency_ns"]
    assert before == bytes(p)
    for payload in (0, 1000):
        assert payload != p.testMsgSize - 53
        out, _ = engine.scribe_multicast(mg, ms, known, payload_bytes=payload)
        assert len(out) == len(mg)
        assert bytes(engine.get_params()) == before
    # a longer publish takes longer on the wire: the call's length did reach the route
    short = engine.scribe_multicast(mg, ms, np.zeros(len(mg), np.uint8), payload_bytes=0, deliveries=False)[0]
    long_ = engine.scribe_multicast(mg, ms, np.zeros(len(mg), np.uint8), payload_bytes=1000, deliveries=False)[0]
    assert short.tobytes() != long_.tobytes()
    with pytest.raises(KbrError, match="EINVAL: payload_bytes must be 0..2\\^24$"):
        engine.scribe_multicast(mg, ms, known, payload_bytes=-1)
    with pytest.raises(KbrError, match="EINVAL: message 0: group or source out of range$"):
        engine.scribe_multicast([len(gk)], [0], [0], payload_bytes=1000)
    assert bytes(engine.get_params()) == before
    assert np.array_equal(engine.lookup(keys, src)["latency_ns"], lat)
