"""The DHT replay on Pastry (tests/refmodel_dht_pastry.py): the Pastry LookupCall replayed through real per-node
transmit queues equals tests/refmodel_pastry_iter.py field by field, leaves the source's queue idle at completion
-- the premise under which the engine's DHT tier is exact on a Pastry context -- and the short-timeout case the
GPU test and the golden fixture use holds every outcome.  No GPU."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

import dht_pastry_cases as X
import refmodel_dht as D
import refmodel_dht_pastry as DP
import refmodel_pastry as RP
import refmodel_pastry_iter as RI
from oversim_amd import workload as W

ROOT = Path(__file__).resolve().parent.parent
SMALLEST = 2                       # PastryNet (like ovs_pastry_load) needs a leaf: two nodes


def _keys(net, m, seed):
    k1, s1 = W.lookups(net.ids, m // 2, seed, node_ids=True)
    k2, s2 = W.lookups(net.ids, m - m // 2, seed + 1, node_ids=False)
    return np.ascontiguousarray(np.concatenate([k1, k2])), np.ascontiguousarray(np.concatenate([s1, s2]))


@pytest.mark.parametrize("n", [SMALLEST, 9, 64, 1000])
@pytest.mark.parametrize("b,L", [(4, 16), (2, 8)])
@pytest.mark.parametrize("tmo", [1.5, X.SHORT_TMO])
def test_measured_lookup_equals_the_model_and_leaves_the_queue_idle(n, b, L, tmo):
    pn = X.pastry_net(n, b, L)
    keys, src = _keys(X.population(n), 200, 31 + n)
    R = min(4, L // 2)
    a = DP.pastry_measured_lookup(pn, R, rpc_to=tmo)(keys, src)
    want = RI.lookups(pn, keys, src, R, rpc_to=tmo)
    for f in DP.FIELDS:
        assert np.array_equal(np.asarray(a[f]).astype(np.int64), np.asarray(want[f]).astype(np.int64)), f
    ok = a["status"] == RI.OK
    assert ok.any() and (a["src_tx_finished"][ok] <= a["latency_ns"][ok]).all()
    # a lookup that sent a FindNodeCall used the queue; one answered by the source's own findNode never did
    assert (a["src_tx_finished"][ok & (a["hops"] > 0)] > 0).all()
    assert (a["src_tx_finished"][ok & (a["hops"] == 0)] == 0).all() and (a["latency_ns"][ok & (a["hops"] == 0)] == 0).all()
    if n == 1000 and tmo < 1:
        recovered = ok & (want["rpcs"] > want["hops"])          # a later start-vector entry after a timeout
        assert recovered.sum() >= 5 and (~ok).sum() >= 20 and ok.sum() >= 20
    if n < R:
        assert (a["num_siblings"][ok] == n).all()               # the sibling row is shorter than numReplica
    # the DHT replay on top of it asserts the idle queue per operation and gives the records of the plain lookup
    ops = D.make_ops(len(src), t0_ns=np.arange(len(src)) * 1000, token=np.arange(len(src)) + 1, vlen=30, ttl=60)
    M1 = D.DhtModel(pn.xy, DP.pastry_measured_lookup(pn, R, rpc_to=tmo), True, R, R, rpc_udp_timeout=tmo)
    M2 = D.DhtModel(pn.xy, DP.pastry_lookup(pn, R, rpc_to=tmo), True, R, R, rpc_udp_timeout=tmo)
    p1, p2 = M1.put_batch(keys, src, ops), M2.put_batch(keys, src, ops)
    for f in D.PUT_FIELDS:
        assert np.array_equal(p1[f], p2[f]), f
    g1, g2 = M1.get_batch(keys, src, ops), M2.get_batch(keys, src, ops)
    for f in D.GET_FIELDS:
        assert np.array_equal(g1[f], g2[f]), f
    assert M1.queue_measured == 2 * int(ok.sum()) and M2.queue_measured == 0


@pytest.mark.parametrize("rnd,auth", [(0, True), (1, True), (0, False)])
def test_measured_lookup_under_truncation_and_auth_block(rnd, auth):
    pn = X.pastry_net(64, 4, 16, rnd)
    keys, src = _keys(X.population(64), 200, 5)
    a = DP.pastry_measured_lookup(pn, 4, auth=auth)(keys, src)
    want = RI.lookups(pn, keys, src, 4, auth=auth)
    for f in DP.FIELDS:
        assert np.array_equal(np.asarray(a[f]).astype(np.int64), np.asarray(want[f]).astype(np.int64)), f
    plain = RI.lookups(pn, keys, src, 4)
    moved = want["latency_ns"] != plain["latency_ns"]
    assert moved.any() == auth                                  # + 100 B in every response changes the latencies
    ok = a["status"] == RI.OK
    assert (a["src_tx_finished"][ok] <= a["latency_ns"][ok]).all()


def test_message_lengths_carry_the_pastry_extension():
    # FINDNODECALL_L 440 + 224 bits = 83 B + 28 B UDP/IP; the response 264 + 208 k + 224 bits, + 800 with the block
    assert RI.call_bytes() == 83 + 28
    assert [RI.resp_bytes(k) for k in (0, 1, 4)] == [61 + 28, 87 + 28, 165 + 28]
    assert RI.resp_bytes(1, True) - RI.resp_bytes(1) == 100
    assert RI.call_bytes() - (440 + 7) // 8 - 28 == 28


def test_short_timeout_case_holds_every_outcome():
    """The case the GPU test and the golden fixture use: successful puts, failed puts, operations whose lookup
    failed, gets in both outcomes, a get that returns a value and one that returns none."""
    b, ref, M = X.reference(1000, tmo=X.SHORT_TMO)
    c = X.census(ref)
    print("short-timeout census:", c)
    assert min(c.values()) >= 10, c
    g = np.concatenate([ref[1], ref[3]])
    assert ((g["outcome"] == D.SUCCESS) & (g["result_count"] == 0)).any()
    # and the default timeout: everything succeeds, so the two cases differ in kind
    d = X.census(X.reference(1000)[1])
    assert d["put_failed"] == d["put_lookup_failed"] == d["get_failed"] == d["get_lookup_failed"] == 0 and d["get_value"] > 300


def test_short_timeout_case_through_measured_queues():
    """The whole put / get / overwrite / get sequence of the short-timeout case on the measured lookup: the idle-queue
    assert holds for every operation with a valid lookup, and the records are those of the plain lookup."""
    b, ref, _ = X.reference(1000, tmo=X.SHORT_TMO)
    M = X.model(1000, tmo=X.SHORT_TMO, measured=True)
    got = X.replay(M, b)
    valid = 0
    for j, (g, r) in enumerate(zip(got, ref)):
        for f in (D.PUT_FIELDS if j % 2 == 0 else D.GET_FIELDS):
            assert np.array_equal(g[f], r[f]), (j, f)
        valid += int((r["outcome"] != D.LOOKUP_FAILED).sum())
    assert M.queue_measured == valid > 0


@pytest.mark.parametrize("n", [SMALLEST, 3, 9])
def test_networks_smaller_than_num_replica(n):
    b, ref, M = X.reference(n, 4, 16 if n > 3 else 8)
    p = ref[0]
    assert (p["outcome"] == D.SUCCESS).all()
    assert (p["num_sent"] == min(n, 4)).all() and (p["num_responses"] == min(n, 4) // 2 + 1).all()
    assert (ref[1]["outcome"] == D.SUCCESS).all() and (ref[1]["num_sent"] == min(n, 4)).all()


def test_header_flag_and_golden_fixture_matches_the_model():
    assert "#define OVS_HAS_DHT_PASTRY 1" in (ROOT / "include" / "ovs_kbr.h").read_text()
    z = np.load(ROOT / "tests" / "golden" / "dht_pastry_n1000.npz")
    net = X.population(1000)
    assert np.array_equal(z["ids"], net.ids) and np.array_equal(z["xy"], net.xy)
    for tag, tmo in (("d", 1.5), ("s", X.SHORT_TMO)):
        b, ref, _ = X.reference(1000, tmo=tmo)
        assert np.array_equal(z["keys"], b[0]) and np.array_equal(z["src"], b[1])
        for name, r in zip(("put_out", "get1_out", "over_out", "get2_out"), ref):
            assert np.array_equal(z[f"{tag}_{name}"], r), (tag, name)
    assert float(z["short_timeout"]) == X.SHORT_TMO
