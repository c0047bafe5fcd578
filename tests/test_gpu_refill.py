"""The lane refill of the route kernels that share it (persist.hpp) at the batch sizes where a refill can go
wrong: fewer lookups than lanes, exactly one wave, one over, one block, one over.  One network of 1000 nodes per
overlay and one batch of 1025 lookups, answered once by the overlay's CPU model; the engine's answer for the first
m lookups must be the model's first m rows in every output array (records, hop lists, siblings, RPC counts)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from oversim_amd import BrooseParams, KbrEngine, Params, PastryParams, workload as W
from oracle_lib import OracleNet
import broose_cases as BC
import refmodel
import refmodel_broose as RB
import refmodel_pastry as RP
import refmodel_pastry_iter as RI

pytestmark = pytest.mark.gpu
N, NQ = 1000, 1025
SIZES = [NQ, 1, 63, 64, 65, 255, 256, 257]
NONE = 0xFFFFFFFF
RFIELDS = ("responsible", "hops", "status", "one_way_hops", "latency_ns")


@functools.lru_cache(maxsize=None)
def _batch():
    net = W.population(N, 81)
    rng = np.random.default_rng(120)
    keys = W.random_keys(NQ, rng)
    keys[::4] = net.ids[rng.integers(0, N, len(keys[::4]))]        # node ids as keys too
    return net, keys, rng.integers(0, N, NQ).astype(np.uint32), (np.arange(NQ) & 1).astype(np.uint8)


def _padded(seqs, H):
    out = np.full((len(seqs), H), NONE, dtype=np.uint32)
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out


@functools.lru_cache(maxsize=None)
def _want(overlay):
    """the model's answer for the whole batch, as the arrays the engine call returns; computed once and read only"""
    net, keys, src, right = _batch()
    if overlay == "broose":
        w = BC.model_routes(RB.BrooseNet(net.ids, net.xy, shifting_bits=2, user_dist=0, rnd=True), keys, src, right)
        out = {f: w[f] & 0xFFFFFFFF if f == "responsible" else w[f] for f in RFIELDS}
        out["rpcs"] = w["rpcs"]
        out["hop_seq"] = _padded(w["hop_seq"], 50)
    elif overlay == "koorde":
        R = refmodel.KoordeRing(net.ids, net.xy)
        res = [R.lookup(keys[i], int(src[i])) for i in range(NQ)]
        out = {f: np.array([r[f] for r in res], dtype=np.int64) for f in RFIELDS}
        out["hop_seq"] = _padded([r["hop_seq"] for r in res], 50)
        # the model counts no FindNodeCalls: those are the oracle's, the reading test_gpu_koorde checks them against
        out["rpcs"] = OracleNet("koorde", net.ids, net.xy).route(keys, src, count_rpcs=True)["rpcs"].astype(np.int64)
    else:
        m = RP.PastryNet(net.ids, net.xy, 4, 16, False, True, rnd=True)
        out = RP.routes(m, keys, src, rec_num_redundant=3) if overlay == "pastry" else RI.lookups(m, keys, src, 4)
    for a in out.values():
        a.setflags(write=False)
    return out


def _run(engine, overlay, m):
    net, keys, src, right = _batch()
    keys, src, right = keys[:m], src[:m], right[:m]
    if overlay == "broose":
        engine.set_params(Params.broose())
        engine.broose_load(net.ids, net.xy, BrooseParams.default())
        return engine.broose_lookup(keys, src, right, record_hops=True, count_rpcs=True)
    if overlay == "koorde":
        engine.set_params(Params.koorde())
        engine.koorde_load(net.ids, net.xy)
        return engine.lookup(keys, src, record_hops=True, count_rpcs=True)
    engine.set_params(Params.pastry() if overlay == "pastry" else Params.pastry().replace(routingType=0))
    engine.pastry_load(net.ids, net.xy, PastryParams.default(routeMsgAcks=0))
    if overlay == "pastry":
        return engine.pastry_lookup(keys, src, record_hops=True)
    return engine.pastry_lookup_call(keys, src, 4, record_hops=True)


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("overlay", ["broose", "pastry", "pastry_iter", "koorde"])
def test_first_m_lookups_equal_the_model(engine: KbrEngine, overlay, m):
    want = _want(overlay)
    got = _run(engine, overlay, m)
    assert got.keys() == want.keys()
    for f, w in want.items():
        g = got[f]
        assert g.shape == w[:m].shape, (f, g.shape)
        bad = np.flatnonzero((g.astype(np.int64) != w[:m].astype(np.int64)).reshape(m, -1).any(axis=1))
        assert len(bad) == 0, (f, bad[:5], g[bad[:5]], w[bad[:5]])
    if m == NQ:
        assert (want["status"] == 0).mean() > 0.9
