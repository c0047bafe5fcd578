"""The networks, batches and reference replays that tests/test_dht_pastry_model.py (CPU) and
tests/test_gpu_dht_pastry.py (GPU) share, and that tests/golden/make_golden_dht_pastry.py writes out -- test
infrastructure only, never calls the engine.

SHORT_TMO is the rpcUdpTimeout of the short-timeout case on the 1000-node network.  It was picked from the model
alone (the FindNodeCall round trips of this population run from about a millisecond to about a second, median
0.13 s): at 0.15 s some lookups succeed, some recover through a later start-vector entry after a timeout and
many fail, and of the operations whose lookup succeeds some puts gather their majority and some do not.
test_dht_pastry_model.py asserts that census.
"""
from __future__ import annotations

import functools

import numpy as np

import refmodel_dht as D
import refmodel_dht_pastry as DP
import refmodel_pastry as RP
from oversim_amd import workload as W

SEC = 10**9
SHORT_TMO = 0.15
M_OPS = 600
SEED = 0x5044


@functools.lru_cache(maxsize=None)
def population(n):
    return W.population(n, SEED + n)


@functools.lru_cache(maxsize=None)
def pastry_net(n, b=4, L=16, rnd=1):
    net = population(n)
    return RP.PastryNet(net.ids, net.xy, b, L, rnd=bool(rnd))


def batches(net, m, seed):
    """put, get, overwrite (every 7th a delete), get after the first TTLs ran out, as tests/test_gpu_dht.py
    builds them.  The first operations share one key (conflicts within a batch); half the keys are node IDs."""
    rng = np.random.default_rng(seed)
    k1, s1 = W.lookups(net.ids, m // 2, seed, node_ids=True)
    k2, s2 = W.lookups(net.ids, m - m // 2, seed + 1, node_ids=False)
    keys, src = np.ascontiguousarray(np.concatenate([k1, k2])), np.ascontiguousarray(np.concatenate([s1, s2]))
    keys[:min(64, m // 4)] = keys[min(64, m // 4)]
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


def model(n, b=4, L=16, rnd=1, R=4, G=4, tmo=1.5, auth=False, ratio=0.5, measured=False, ids=None, xy=None):
    """A fresh DhtModel on pastry_net(n, b, L, rnd), or on the n sorted ids and coordinates given, fed by the Pastry
    LookupCall (measured: through real queues)."""
    pn = pastry_net(n, b, L, rnd) if ids is None else RP.PastryNet(ids, xy, b, L, rnd=bool(rnd))
    look = (DP.pastry_measured_lookup if measured else DP.pastry_lookup)(pn, R, rpc_to=tmo, auth=auth)
    return D.DhtModel(pn.xy, look, bool(rnd), R, G, ratio, rpc_udp_timeout=tmo, auth=auth)


@functools.lru_cache(maxsize=None)
def reference(n, b=4, L=16, rnd=1, R=4, G=4, tmo=1.5, auth=False, m=M_OPS, seed=7):
    """(batches, the four replayed record arrays, the model after them), computed once and shared."""
    bt = batches(population(n), m, seed + n)
    M = model(n, b, L, rnd, R, G, tmo, auth)
    return bt, replay(M, bt), M


def census(ref):
    """What the short-timeout case must contain: counts over the four record arrays."""
    p = np.concatenate([ref[0], ref[2]])
    g = np.concatenate([ref[1], ref[3]])
    return dict(put_ok=int((p["outcome"] == D.SUCCESS).sum()), put_failed=int((p["outcome"] == D.FAILED).sum()),
                put_lookup_failed=int((p["outcome"] == D.LOOKUP_FAILED).sum()),
                get_ok=int((g["outcome"] == D.SUCCESS).sum()), get_failed=int((g["outcome"] == D.FAILED).sum()),
                get_lookup_failed=int((g["outcome"] == D.LOOKUP_FAILED).sum()),
                get_value=int((g["result_count"] == 1).sum()))
