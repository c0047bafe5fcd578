"""Iterative lookups on Pastry on the GPU (k_pastry_iter, oversim_amd/csrc/pastry.hip) against the model
(tests/refmodel_pastry_iter.py), bit for bit: status, hops, number of siblings, sibling vector, hop sequence, RPC
count, int64 latency -- LookupCalls and the one-way route, the committed golden vectors, tiny networks, the hop
and time limits, thinned explicit tables, the engine's own findNode kernel along the recorded hops, the refusals,
the device-pointer form and a large ring checked by properties."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from oversim_amd import KbrEngine, KbrError, LOOKUP_OUT_DTYPE, Params, PastryParams, ROUTE_OUT_DTYPE, workload as W
from oversim_amd.kbr import key_from_int
import refmodel_pastry as RP
import refmodel_pastry_iter as RI

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
NONE = 0xFFFFFFFF
LFIELDS = ("status", "hops", "num_siblings", "is_valid", "latency_ns", "rpcs")
RFIELDS = ("responsible", "hops", "status", "one_way_hops", "latency_ns")
MODEL_KW = dict(hopCountMax="hop_max", rpcUdpTimeout="rpc_to", lookupTimeout="lk_to", measureAuthBlock="auth")


def _iter_params(**pk):
    return Params.pastry().replace(routingType=0, **pk)


def _pp(**kw):
    return PastryParams.default(routeMsgAcks=0, **kw)


def _load(engine, n, seed=81, b=4, L=16, opt=0, reg=1, **pk):
    net = W.population(n, seed)
    engine.set_params(_iter_params(**pk))
    engine.pastry_load(net.ids, net.xy, _pp(bitsPerDigit=b, numberOfLeaves=L, optimizeLookup=opt, useRegularNextHop=reg))
    m = RP.PastryNet(net.ids, net.xy, b, L, bool(opt), bool(reg), rnd=bool(pk.get("simtimeRound", 1)))
    return net, m


def _mkw(pk):
    return {MODEL_KW[k]: (bool(v) if k == "measureAuthBlock" else v) for k, v in pk.items() if k in MODEL_KW}


def _batch(net, nq, seed):
    rng = np.random.default_rng(seed)
    keys = W.random_keys(nq, rng)
    keys[::4] = net.ids[rng.integers(0, len(net.ids), len(keys[::4]))]
    return keys, rng.integers(0, len(net.ids), nq).astype(np.uint32)


def _assert_lookups(got, want, what=""):
    for f in LFIELDS + ("siblings", "hop_seq"):
        g, w = got[f], want[f]
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        assert len(bad) == 0, (what, f, bad[:5], g[bad[:5]], w[bad[:5]])


def _assert_routes(got, want, what=""):
    for f in RFIELDS + ("hop_seq",):
        g, w = got[f], want[f]
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        assert len(bad) == 0, (what, f, bad[:5], g[bad[:5]], w[bad[:5]])


def _check(engine, m, keys, src, ns, what="", **pk):
    """One LookupCall batch against the model; ns -1 is getMaxNumSiblings()."""
    want = RI.lookups(m, keys, src, ns if ns > 0 else m.L // 2, **_mkw(pk))
    _assert_lookups(engine.pastry_lookup_call(keys, src, ns, record_hops=True), want, f"{what} ns={ns}")
    return want


def _census(r):
    return {int(s): int((r["status"] == s).sum()) for s in np.unique(r["status"])}


@pytest.mark.parametrize("rnd", [1, 0])
def test_golden_fixture(engine: KbrEngine, rnd):
    g = np.load(GOLD / "pastry_iter_n1000.npz")
    base = np.load(GOLD / "pastry_n1000.npz")
    engine.set_params(_iter_params(simtimeRound=rnd))
    engine.pastry_load(base["ids"], base["xy"], _pp())
    lat = "latency_ns" if rnd else "latency_ns_trunc"
    for ns in (1, 8):
        got = engine.pastry_lookup_call(base["keys"], base["src"], ns, record_hops=True)
        for f in ("status", "hops", "num_siblings", "rpcs", "siblings"):
            assert np.array_equal(got[f], g[f"l{ns}_{f}"]), (ns, f)
        assert np.array_equal(got["latency_ns"], g[f"l{ns}_{lat}"]), ns
        H = g[f"l{ns}_hop_seq"].shape[1]
        assert np.array_equal(got["hop_seq"][:, :H], g[f"l{ns}_hop_seq"]) and np.all(got["hop_seq"][:, H:] == NONE)
    got = engine.pastry_iterative_lookup(base["keys"], base["src"], record_hops=True)
    for f in RFIELDS[:-1]:
        assert np.array_equal(got[f], g[f"rt_{f}"]), f
    assert np.array_equal(got["latency_ns"], g[f"rt_{lat}"])
    H = g["rt_hop_seq"].shape[1]
    assert np.array_equal(got["hop_seq"][:, :H], g["rt_hop_seq"]) and np.all(got["hop_seq"][:, H:] == NONE)


@pytest.mark.parametrize("b,L", [(4, 16), (2, 8), (1, 2), (3, 32)])
@pytest.mark.parametrize("opt,reg,auth", [(0, 1, 0), (1, 1, 1), (0, 0, 1), (1, 0, 0)])
def test_lookups_equal_model(engine: KbrEngine, b, L, opt, reg, auth):
    pk = dict(measureAuthBlock=auth)
    net, m = _load(engine, 1000, b=b, L=L, opt=opt, reg=reg, **pk)
    keys, src = _batch(net, 1024, 95)
    for ns in (1, 4, 8, -1):
        if ns <= L // 2:
            want = _check(engine, m, keys, src, ns, f"b={b} L={L} opt={opt} reg={reg}", **pk)
            assert (want["status"] == RI.OK).mean() > 0.9
    _assert_routes(engine.pastry_iterative_lookup(keys, src, record_hops=True), RI.routes(m, keys, src, **_mkw(pk)), "route")


def test_truncating_simtime(engine: KbrEngine):
    net, m = _load(engine, 1000, simtimeRound=0)
    keys, src = _batch(net, 512, 96)
    _check(engine, m, keys, src, 8)
    _assert_routes(engine.pastry_iterative_lookup(keys, src, record_hops=True), RI.routes(m, keys, src), "route trunc")


@pytest.mark.parametrize("n", [2, 3, 9])
def test_tiny_networks_every_source(engine: KbrEngine, n):
    net, m = _load(engine, n, L=8)
    ids = m.ids
    fixed = [0, 1, RP.M - 1, 1 << 159, ids[0], ids[n - 1] + 1, (ids[0] + (ids[1] - ids[0]) // 2)]
    keys = np.array([key_from_int(k % RP.M) for k in fixed for _ in range(n)], dtype=np.uint32)
    src = np.array(list(range(n)) * len(fixed), dtype=np.uint32)
    short = local = 0
    for ns in (1, 2, 3, 4, -1):
        want = _check(engine, m, keys, src, ns, f"n={n}")
        ok = want["status"] == RI.OK
        short += int((ok & (want["num_siblings"] < (ns if ns > 0 else 4))).sum())
        local += int((ok & (want["hops"] == 0)).sum())
    assert local > 0 and (short > 0 or n == 9)      # fewer nodes than siblings asked for; lookups that end at the source
    _assert_routes(engine.pastry_iterative_lookup(keys, src, record_hops=True), RI.routes(m, keys, src), f"route n={n}")


@pytest.mark.parametrize("hcm", [1, 3])
def test_hop_limit(engine: KbrEngine, hcm):
    net, m = _load(engine, 1000, hopCountMax=hcm)
    keys, src = _batch(net, 1024, 95)
    for ns in (1, 8):
        want = _check(engine, m, keys, src, ns, f"hcm={hcm}", hopCountMax=hcm)
        assert (want["status"] == RI.HOPMAX).sum() > 0 and (want["status"] == RI.OK).sum() > 0
    _assert_routes(engine.pastry_iterative_lookup(keys, src, record_hops=True), RI.routes(m, keys, src, hop_max=hcm), "route")


def test_rpc_timeouts(engine: KbrEngine):
    """rpcUdpTimeout = 0.15 s, picked from the model on this batch (RTTs there run from 1.3 ms to 0.97 s, median
    0.13 s): 389 lookups succeed, 65 of them after a timeout moved the path to the start vector's next entry, 470
    end RPC_TIMEOUT and 165 NO_NEXT, most of those because a response names a node that timed out."""
    pk = dict(rpcUdpTimeout=0.15)
    net, m = _load(engine, 1000, **pk)
    keys, src = _batch(net, 1024, 95)
    want = _check(engine, m, keys, src, 1, "rpc timeout", **pk)
    recovered = (want["status"] == RI.OK) & (want["rpcs"] > want["hops"])
    assert (want["status"] == RI.RPC_TIMEOUT).sum() + recovered.sum() >= 20 and (want["status"] == RI.OK).sum() >= 20
    assert recovered.sum() >= 20 and (want["status"] == RI.NO_NEXT).sum() >= 20
    _check(engine, m, keys, src, 8, "rpc timeout", **pk)
    _assert_routes(engine.pastry_iterative_lookup(keys, src, record_hops=True), RI.routes(m, keys, src, rpc_to=0.15), "route")
    # a timeout below every RTT: each lookup walks the source's whole answer
    engine.set_params(_iter_params(rpcUdpTimeout=1e-6))
    all_out = _check(engine, m, keys[:256], src[:256], 1, "every call times out", rpcUdpTimeout=1e-6)
    assert (all_out["status"] == RI.RPC_TIMEOUT).sum() >= 20 and all_out["rpcs"].max() >= 16


def test_lookup_timeout(engine: KbrEngine):
    """lookupTimeout = 0.3 s, picked from the model on this batch (successful lookups there take 5.6 ms to 2.2 s,
    median 0.34 s): 439 succeed, 585 end TIMEOUT.  With rpcUdpTimeout = 0.15 s as well, TIMEOUT is also reached
    from handleTimeout."""
    for pk in (dict(lookupTimeout=0.3), dict(lookupTimeout=0.3, rpcUdpTimeout=0.15)):
        net, m = _load(engine, 1000, **pk)
        keys, src = _batch(net, 1024, 95)
        want = _check(engine, m, keys, src, 1, str(pk), **pk)
        assert (want["status"] == RI.TIMEOUT).sum() >= 20 and (want["status"] == RI.OK).sum() >= 20
        _check(engine, m, keys, src, 4, str(pk), **pk)


@pytest.mark.parametrize("opt", [0, 1])
def test_thinned_tables(engine: KbrEngine, opt):
    """30 % of the routing-table slots emptied, as test_gpu_pastry builds them.  With whole leaf sets no share of
    emptied table slots makes a lookup fail in the model, 100 % included: findCloserNode always finds a leaf that
    is closer.  So the second network also empties 30 % of the leaf slots, where the model shows NO_NEXT for
    num_siblings = 8 (a responder that is no sibling names itself)."""
    net, m = _load(engine, 1000, opt=opt)
    leaf, tab = engine.pastry_export()
    rng = np.random.default_rng(85)
    thin = tab.copy()
    thin[rng.random(tab.shape) < 0.3] = NONE
    keys, src = _batch(net, 1024, 86)
    engine.pastry_load_tables(net.ids, net.xy, leaf, thin, _pp(optimizeLookup=opt))
    sm = RP.PastryNet(net.ids, net.xy, optimize=bool(opt), tables=(leaf, thin))
    for ns in (1, 8):
        _check(engine, sm, keys, src, ns, "thin tables")
    _assert_routes(engine.pastry_iterative_lookup(keys, src, record_hops=True), RI.routes(sm, keys, src), "thin route")
    tl = leaf.copy()
    tl[rng.random(leaf.shape) < 0.3] = NONE
    empty = (tl != NONE).sum(axis=1) == 0
    tl[empty] = leaf[empty]
    engine.pastry_load_tables(net.ids, net.xy, tl, thin, _pp(optimizeLookup=opt))
    sm = RP.PastryNet(net.ids, net.xy, optimize=bool(opt), tables=(tl, thin))
    failed = 0
    for ns in (1, 4, 8):
        want = _check(engine, sm, keys, src, ns, "thin tables and leaves")
        failed += int((want["status"] == RI.NO_NEXT).sum())
        print("thinned tables and leaves: ns", ns, _census(want))
    assert failed >= 1


@pytest.mark.parametrize("ns", [1, 8])
def test_hops_through_the_find_node_kernel(engine: KbrEngine, ns):
    """Along the recorded hop sequences the engine's findNode batch names the next responder; at the last responder
    it gives the sibling flag and the sibling vector the lookup returned."""
    net, m = _load(engine, 1000)
    keys, src = _batch(net, 512, 97)
    r = engine.pastry_lookup_call(keys, src, ns, record_hops=True)
    ok = np.flatnonzero((r["status"] == RI.OK) & (r["hops"] > 0))
    assert len(ok) > 300
    node, nxt, kk = [], [], []
    for i in ok:
        h = r["hop_seq"][i, :r["hops"][i]]
        node += list(h[:-1]); nxt += list(h[1:]); kk += [keys[i]] * (len(h) - 1)
    out, cnt, sib, st = engine.pastry_find_node(np.array(node, dtype=np.uint32), np.array(kk, dtype=np.uint32), 1, ns, max_out=ns)
    assert np.all(st & 2 == 0) and np.all(sib == 0) and np.all(cnt == 1) and np.array_equal(out[:, 0], np.array(nxt, dtype=np.uint32))
    last = r["hop_seq"][ok, r["hops"][ok] - 1]
    out, cnt, sib, st = engine.pastry_find_node(last, keys[ok], 1, ns, max_out=ns)
    assert np.all(sib == 1) and np.all(st == 0) and np.array_equal(cnt, r["num_siblings"][ok].astype(np.uint8))
    assert np.array_equal(out, r["siblings"][ok])
    # the first target: the first entry of the source's answer for numberOfLeaves nodes
    out, cnt, sib, st = engine.pastry_find_node(src[ok], keys[ok], 16, ns, max_out=17)
    assert np.array_equal(out[:, 0], r["hop_seq"][ok, 0])


def test_default_pastry_params_acks_on(engine: KbrEngine):
    net = W.population(1000, 81)
    keys, src = _batch(net, 256, 98)
    engine.set_params(_iter_params())
    engine.pastry_load(net.ids, net.xy, _pp())
    off = engine.pastry_lookup_call(keys, src, 8, record_hops=True)
    engine.pastry_load(net.ids, net.xy, PastryParams.default())
    on = engine.pastry_lookup_call(keys, src, 8, record_hops=True)
    for f in on:
        assert np.array_equal(on[f], off[f]), f
    assert (on["status"] == RI.OK).all()
    with pytest.raises(KbrError, match="routeMsgAcks"):
        engine.pastry_iterative_lookup(keys, src)


def test_refusals_leave_the_context_usable(engine: KbrEngine):
    net = W.population(1000, 81)
    keys, src = _batch(net, 16, 89)
    engine.set_params(Params.pastry())
    engine.pastry_load(net.ids, net.xy, _pp())
    base = engine.pastry_lookup(keys, src)

    def refused(match, **kw):
        engine.set_params(_iter_params().replace(**kw))
        for fn in (lambda: engine.pastry_lookup_call(keys, src, 1), lambda: engine.pastry_iterative_lookup(keys, src)):
            with pytest.raises(KbrError, match=match) as e:
                fn()
            assert "ENOTSUP" in str(e.value)
        engine.set_params(Params.pastry())
        assert np.array_equal(engine.pastry_lookup(keys, src)["latency_ns"], base["latency_ns"])

    refused("lookupRedundantNodes", lookupRedundantNodes=2)
    refused("lookupParallelRpcs", lookupParallelRpcs=3)
    # lookupParallelPaths never reaches a call: ovs_set_params refuses it on every overlay, with its name
    with pytest.raises(KbrError, match="lookupParallelPaths") as e:
        engine.set_params(_iter_params(lookupParallelPaths=2))
    assert "ENOTSUP" in str(e.value)
    assert np.array_equal(engine.pastry_lookup(keys, src)["latency_ns"], base["latency_ns"])
    refused("lookupMerge", lookupMerge=1)
    refused("lookupVisitOnlyOnce", lookupVisitOnlyOnce=0)
    refused("lookupFinishOnFirstUnchanged", lookupFinishOnFirstUnchanged=1)
    refused("hopCountMax", hopCountMax=0)
    for rt in (1, 2, 4):      # 3, exhaustive-iterative, is refused by ovs_set_params outside Kademlia
        refused("routingType", routingType=rt)
    # the number of siblings
    engine.set_params(_iter_params())
    with pytest.raises(KbrError, match="num_siblings = 0"):
        engine.pastry_lookup_call(keys, src, 0)
    with pytest.raises(KbrError, match="EINVAL"):
        engine.pastry_lookup_call(keys, src, 9)
    with pytest.raises(KbrError, match="EINVAL"):
        engine.pastry_lookup_call(keys, np.full(16, 1000, dtype=np.uint32), 1)
    # the semi-recursive route still refuses iterative routing, and the iterative calls work after all of it
    with pytest.raises(KbrError, match="PastryFindNodeExtData"):
        engine.pastry_lookup(keys, src)
    assert (engine.pastry_lookup_call(keys, src, 1)["status"] == RI.OK).all()
    engine.set_params(Params.pastry())
    assert np.array_equal(engine.pastry_lookup(keys, src)["latency_ns"], base["latency_ns"])
    # another overlay's context
    with KbrEngine(0) as ec:
        ec.set_params(Params.chord())
        ec.chord_load(net.ids, net.xy)
        for fn in (lambda: ec.pastry_lookup_call(keys, src, 1), lambda: ec.pastry_iterative_lookup(keys, src)):
            with pytest.raises(KbrError, match="ESTATE"):
                fn()
        assert (ec.lookup(keys, src)["status"] == 0).all()


def test_device_pointer_form_and_empty_batch(engine: KbrEngine):
    import torch
    net, m = _load(engine, 1000)
    keys, src = _batch(net, 1024, 99)
    dev = torch.device("cuda:0")
    dk, ds = torch.from_numpy(keys.view(np.int32)).to(dev), torch.from_numpy(src.view(np.int32)).to(dev)
    for ns in (1, 8, -1):
        w = ns if ns > 0 else 8
        host = engine.pastry_lookup_call(keys, src, ns)
        out = torch.zeros(1024 * LOOKUP_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        sib = torch.zeros(1024 * w, dtype=torch.int32, device=dev)
        rpcs = torch.zeros(1024, dtype=torch.int32, device=dev)
        engine.pastry_lookup_call_device(dk.data_ptr(), ds.data_ptr(), 1024, ns, out.data_ptr(), sib.data_ptr(),
                                         rpcs_ptr=rpcs.data_ptr())
        torch.cuda.synchronize()
        o = out.cpu().numpy().view(LOOKUP_OUT_DTYPE)
        for f in LOOKUP_OUT_DTYPE.names:
            assert np.array_equal(o[f], host[f]), (ns, f)
        assert np.array_equal(sib.cpu().numpy().view(np.uint32).reshape(1024, w), host["siblings"])
        assert np.array_equal(rpcs.cpu().numpy().view(np.uint32), host["rpcs"])
    host = engine.pastry_iterative_lookup(keys, src)
    out = torch.zeros(1024 * ROUTE_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    engine.pastry_iterative_lookup_device(dk.data_ptr(), ds.data_ptr(), 1024, out.data_ptr())
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(ROUTE_OUT_DTYPE)
    for f in ROUTE_OUT_DTYPE.names:
        assert np.array_equal(o[f], host[f]), f
    # an empty batch
    e = engine.pastry_lookup_call(keys[:0], src[:0], 8)
    assert len(e["status"]) == 0 and e["siblings"].shape == (0, 8)
    assert len(engine.pastry_iterative_lookup(keys[:0], src[:0])["status"]) == 0
    engine.pastry_lookup_call_device(0, 0, 0, 1, 0, 0)
    engine.pastry_iterative_lookup_device(0, 0, 0, 0)


def test_large_ring_properties(engine: KbrEngine):
    n, nq = 1 << 16, 1 << 17
    net = W.population(n, 87)
    engine.set_params(_iter_params())
    engine.pastry_load(net.ids, net.xy, _pp())
    rng = np.random.default_rng(88)
    keys = W.random_keys(nq, rng)
    src = rng.integers(0, n, nq).astype(np.uint32)
    r = engine.pastry_lookup_call(keys, src, 8, record_hops=True)
    ok = r["status"] == RI.OK
    assert ok.mean() > 0.99 and (r["hops"] <= 50).all()
    assert np.array_equal(r["hops"][ok], (r["hop_seq"][ok] != NONE).sum(axis=1))
    assert np.array_equal(r["rpcs"][ok], r["hops"][ok].astype(np.uint32)) and (r["num_siblings"][ok] == 8).all()
    assert (r["latency_ns"][ok & (r["hops"] > 0)] > 0).all()
    m = RP.PastryNet(net.ids, net.xy, nodes=[])
    for i in rng.choice(nq, 2000, replace=False):
        if ok[i]:
            assert int(r["siblings"][i, 0]) in m.owner(RP.to_int(keys[i])), i
