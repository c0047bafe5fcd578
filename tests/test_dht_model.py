"""The DHT replay (tests/refmodel_dht.py) on hand-counted cases, and the C ABI of the DHT calls: the struct
layouts a plain C compiler derives from include/ovs_kbr.h equal the numpy / ctypes mirrors, the library
exports the entry points and the ABI version is unchanged.  No GPU."""
from __future__ import annotations

import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import refmodel_dht as D
from oracle_lib import OracleNet, chord_params

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
SEC = 10**9


def ring9():
    z = np.load(GOLD / "chord_n9.npz")
    return z["ids"], z["xy"]


def model(ids, xy, R=4, G=4, **kw):
    net = OracleNet("chord", ids, xy, chord_params(simtimeRound=1))
    return D.DhtModel(xy, D.oracle_lookup(net, R), True, R, G, **kw)


def key_between(ids, a):
    """A key whose responsible node is a (its ID minus one)."""
    k = ids[a].copy()
    assert k[0] > 0
    k[0] -= 1
    return k


def one(keys, **kw):
    return np.ascontiguousarray(np.asarray(keys).reshape(-1, 5)), D.make_ops(1, **kw)


def test_put_then_get_returns_the_token():
    ids, xy = ring9()
    M = model(ids, xy)
    k, ops = one(key_between(ids, 4), token=77, vlen=20, ttl=300)
    p = M.put_batch(k, [0], ops)[0]
    # hand count: 4 DHTPutCalls of 864 + 20 bits = 111 B and 4 DHTPutResponses of 264 bits = 33 B
    assert (p["outcome"], p["num_sent"], p["num_responses"], p["messages"], p["bytes"]) == (D.SUCCESS, 4, 3, 8, 4 * (111 + 33))
    assert M.count() == 4 and all(len(M.dump(v, 0)) == 1 for v in (4, 5, 6, 7))
    g = M.get_batch(k, [1], D.make_ops(1, t0_ns=10 * SEC))[0]
    # 4 hash requests; 2 of 4 identical hashes reach ratioIdentical = 0.5, so the value request leaves after the
    # second hash response: GETCALL_L 481 bits = 61 B, hash response 436 bits = 55 B, value response
    # 416 + 20 + 608 bits = 131 B
    assert (g["outcome"], g["result_count"], g["value_token"], g["value_len"]) == (D.SUCCESS, 1, 77, 20)
    assert (g["num_sent"], g["messages"], g["bytes"]) == (4, 10, 5 * 61 + 4 * 55 + 131)
    assert g["server"] in (4, 5, 6, 7) and g["latency_ns"] > 0


def test_get_after_expiry_is_an_empty_success_and_overwrite_and_delete():
    ids, xy = ring9()
    M = model(ids, xy)
    k, ops = one(key_between(ids, 2), token=5, vlen=8, ttl=60)
    M.put_batch(k, [3], ops)
    g = M.get_batch(k, [3], D.make_ops(1, t0_ns=61 * SEC))[0]
    assert (g["outcome"], g["result_count"], g["value_token"]) == (D.SUCCESS, 0, 0)        # DHT.cc:585-598
    # hash responses without an entry carry no hash: 416 bits = 52 B, as does the empty value response
    assert g["bytes"] == 5 * 61 + 5 * 52
    M.put_batch(k, [5], D.make_ops(1, t0_ns=70 * SEC, token=6, vlen=9))
    M.put_batch(k, [6], D.make_ops(1, t0_ns=80 * SEC, token=7, vlen=10))
    g = M.get_batch(k, [0], D.make_ops(1, t0_ns=90 * SEC))[0]
    assert (g["result_count"], g["value_token"], g["value_len"]) == (1, 7, 10)
    M.put_batch(k, [6], D.make_ops(1, t0_ns=100 * SEC))                                     # a put of an empty value
    assert M.count() == 0
    assert M.get_batch(k, [0], D.make_ops(1, t0_ns=110 * SEC))[0]["result_count"] == 0


def test_the_source_is_a_replica_with_no_delay():
    ids, xy = ring9()
    M = model(ids, xy, R=1, G=1)
    k, ops = one(ids[3], token=1, vlen=4)
    p = M.put_batch(k, [3], ops)[0]
    assert (p["outcome"], p["latency_ns"], p["hop_count"], p["num_sent"]) == (D.SUCCESS, 0, 0, 1)
    g = M.get_batch(k, [3], D.make_ops(1))[0]
    assert (g["outcome"], g["latency_ns"], g["value_token"], g["server"]) == (D.SUCCESS, 0, 1, 3)


@pytest.mark.parametrize("n", [2, 3])
def test_rings_smaller_than_num_replica(n):
    ids, xy = ring9()
    sel = np.arange(n) * 3
    ids, xy = np.ascontiguousarray(ids[sel]), np.ascontiguousarray(xy[sel])
    M = model(ids, xy)
    k, ops = one(key_between(ids, 1), token=9, vlen=3)
    p = M.put_batch(k, [0], ops)[0]
    assert p["num_sent"] == n < 4 and p["outcome"] == D.SUCCESS and p["num_responses"] == n // 2 + 1
    g = M.get_batch(k, [0], D.make_ops(1))[0]
    assert (g["num_sent"], g["outcome"], g["value_token"]) == (n, D.SUCCESS, 9)


def test_ask_one_more_and_a_replica_without_the_entry():
    ids, xy = ring9()
    M = model(ids, xy, R=4, G=1, ratio_identical=0.75)
    k, ops = one(key_between(ids, 4), token=3, vlen=2)
    M.put_batch(k, [0], ops)
    g = M.get_batch(k, [0], D.make_ops(1))[0]
    # one hash request, then one more from replica.back() after each response until 3 of 4 agree
    assert (g["num_sent"], g["num_responses"], g["messages"], g["outcome"], g["value_token"]) == (1, 3, 8, D.SUCCESS, 3)
    # node 4 loses its entry: its hash is UNSPECIFIED_VALUE, a hash like any other; 3 of 4 still agree
    del M.store[4]
    M.G = 4
    g = M.get_batch(k, [0], D.make_ops(1))[0]
    assert (g["outcome"], g["value_token"], g["num_responses"]) == (D.SUCCESS, 3, 4) and g["server"] != 4
    # two replicas without it: 2 : 2, no 0.75 majority; nobody else to ask, so the first hash in map order with
    # the largest vector -- UNSPECIFIED_VALUE -- is taken and the get succeeds with an empty result
    del M.store[5]
    g = M.get_batch(k, [0], D.make_ops(1))[0]
    assert (g["outcome"], g["result_count"], g["num_responses"]) == (D.SUCCESS, 0, 4) and g["server"] in (4, 5)


def test_rpc_timeouts_including_the_exact_tie():
    ids, xy = ring9()
    free = model(ids, xy)
    k, ops = one(key_between(ids, 4), token=3, vlen=2)
    base = free.put_batch(k, [0], ops)[0]
    look = int(free.lookup(k, np.array([0], dtype=np.uint32))["latency_ns"][0])
    third = int(base["latency_ns"]) - look            # the third response's arrival after the calls left
    assert D.simtime(third * 1e-9, True) == third
    tie = model(ids, xy, rpc_udp_timeout=third * 1e-9).put_batch(k, [0], ops)[0]
    # the response that arrives at the very instant of its timeout has timed out: 2 of 4 fail, the put fails
    assert (tie["outcome"], tie["num_responses"], tie["latency_ns"]) == (D.FAILED, 2, look + third)
    ok = model(ids, xy, rpc_udp_timeout=(third + 1) * 1e-9).put_batch(k, [0], ops)[0]
    assert (ok["outcome"], ok["num_responses"]) == (D.SUCCESS, 3)
    # a get whose every RPC times out: no response, nobody else to ask
    M = model(ids, xy, rpc_udp_timeout=1e-6)
    g = M.get_batch(k, [0], D.make_ops(1))[0]
    assert (g["outcome"], g["num_responses"], g["latency_ns"]) == (D.FAILED, 0, look + 1000)


def test_within_batch_conflicts_resolve_by_arrival_then_operation():
    ids, xy = ring9()
    M = model(ids, xy)
    keys = np.repeat(key_between(ids, 4)[None], 9, axis=0)
    ops = D.make_ops(9, token=np.arange(9) + 100, vlen=4)
    M.put_batch(keys, np.arange(9), ops)
    winners = {v: int(M.dump(v, 0)[0]["token"]) for v in (4, 5, 6, 7)}
    assert M.count() == 4 and len(set(winners.values())) > 1      # the last arrival differs between replicas


# ---------------------------------------------------------------- C ABI
def test_dht_struct_layout(tmp_path):
    from oversim_amd import kbr
    exe = tmp_path / "abi_layout_dht"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "abi_layout_dht.c"), "-o", str(exe)], check=True)
    lay = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert lay["abi"] == 12
    assert lay["outcomes"] == [kbr.DHT_SUCCESS, kbr.DHT_FAILED, kbr.DHT_LOOKUP_FAILED] == [D.SUCCESS, D.FAILED, D.LOOKUP_FAILED]
    for name, dts in (("ovs_dht_op", (kbr.DHT_OP_DTYPE, D.OP_DTYPE)), ("ovs_dht_put_out", (kbr.DHT_PUT_DTYPE, D.PUT_DTYPE)),
                      ("ovs_dht_get_out", (kbr.DHT_GET_DTYPE, D.GET_DTYPE)),
                      ("ovs_dht_entry", (kbr.DHT_ENTRY_DTYPE, D.DUMP_DTYPE))):
        rec = lay[name]
        for dt in dts:
            assert dt.itemsize == rec["size"] and list(dt.names) == list(rec["fields"]), name
            for f, off in rec["fields"].items():
                assert dt.fields[f][1] == off, (name, f)
    st, cls = lay["ovs_dht_params"], kbr.DhtParams
    assert C.sizeof(cls) == st["size"] and [f for f, _ in cls._fields_] == list(st["fields"])
    for f, off in st["fields"].items():
        assert getattr(cls, f).offset == off, f


def test_library_exports_the_dht_calls():
    import oversim_amd
    L = oversim_amd.lib()
    for name in ("ovs_dht_params_default", "ovs_dht_store_create", "ovs_dht_store_clear", "ovs_dht_store_count",
                 "ovs_dht_put_batch", "ovs_dht_get_batch", "ovs_dht_dump_node"):
        assert hasattr(L, name), name
    assert L.ovs_abi_version() == 12
    assert "OVS_HAS_DHT" in (ROOT / "include" / "ovs_kbr.h").read_text()
    p = oversim_amd.DhtParams.default()
    assert (p.numReplica, p.numGetRequests, p.ratioIdentical) == (4, 4, 0.5)
    assert (p.secureMaintenance, p.invalidDataAttack, p.maintenanceAttack) == (0, 0, 0)
    for name in ("dht_store_create", "dht_store_clear", "dht_store_count", "dht_put", "dht_get", "dht_put_device",
                 "dht_get_device", "dht_dump"):
        assert callable(getattr(oversim_amd.KbrEngine, name))


# ---------------------------------------------------------------- the source's queue at lookup completion
@pytest.mark.parametrize("n,rnd,auth", [(9, 1, False), (9, 0, True), (1000, 1, False)])
def test_measured_lookup_equals_the_oracle_and_leaves_the_queue_idle(n, rnd, auth):
    """The replay's own LookupCall, message by message through real transmit queues, gives the oracle's siblings,
    hops, status and latency; the source's tx.finished it measures never lies beyond the lookup's completion, and
    the DHT replay on top of it (which asserts that per operation) gives the records of the oracle-fed replay."""
    import refmodel
    from oversim_amd import workload as W
    if n == 9:
        ids, xy = ring9()
    else:
        net = W.population(1000, 77)
        ids, xy = net.ids, net.xy
    o = OracleNet("chord", ids, xy, chord_params(simtimeRound=rnd, measureAuthBlock=int(auth)))
    look = D.chord_measured_lookup(refmodel.ChordRing(ids, xy, 8, bool(rnd)), 4, bool(rnd), auth=auth)
    k1, s1 = W.lookups(ids, 150, 5, node_ids=True)
    k2, s2 = W.lookups(ids, 150, 6, node_ids=False)
    keys, src = np.concatenate([k1, k2]), np.concatenate([s1, s2])
    a, b = look(keys, src), o.lookup_call(keys, src, 4)
    for f in ("num_siblings", "hops", "status", "is_valid", "latency_ns", "siblings"):
        assert np.array_equal(np.asarray(a[f]).astype(np.int64), np.asarray(b[f]).astype(np.int64)), f
    ok = a["status"] == 0
    assert ok.sum() > 200 and (a["src_tx_finished"][ok] <= a["latency_ns"][ok]).all()
    assert (a["src_tx_finished"][ok & (a["hops"] > 0)] > 0).all()
    ops = D.make_ops(len(src), t0_ns=np.arange(len(src)) * 1000, token=np.arange(len(src)) + 1, vlen=30, ttl=60)
    M1 = D.DhtModel(xy, look, bool(rnd), auth=auth)
    M2 = D.DhtModel(xy, D.oracle_lookup(o, 4), bool(rnd), auth=auth)
    p1, p2 = M1.put_batch(keys, src, ops), M2.put_batch(keys, src, ops)
    for f in D.PUT_FIELDS:
        assert np.array_equal(p1[f], p2[f]), f
    g1, g2 = M1.get_batch(keys, src, ops), M2.get_batch(keys, src, ops)
    for f in D.GET_FIELDS:
        assert np.array_equal(g1[f], g2[f]), f
    assert M1.queue_measured == 2 * int(ok.sum()) and M2.queue_measured == 0


def test_a_busy_queue_is_caught():
    ids, xy = ring9()
    o = OracleNet("chord", ids, xy, chord_params(simtimeRound=1))

    def busy(keys, src):
        r = o.lookup_call(keys, src, 4)
        r["src_tx_finished"] = r["latency_ns"] + 1
        return r
    k, ops = one(key_between(ids, 4), token=1, vlen=1)
    with pytest.raises(AssertionError, match="busy"):
        D.DhtModel(xy, busy, True).put_batch(k, [0], ops)


# ---------------------------------------------------------------- .ini binding
INI = """
[General]
**.tier1*.dht.numReplica = 4
**.tier1*.dht.numGetRequests = 4
**.tier1*.dht.ratioIdentical = 0.5
**.tier1*.dht.secureMaintenance = false
**.tier1*.dht.invalidDataAttack = false
**.tier1*.dht.maintenanceAttack = false
**.tier2*.dhtTestApp.testTtl = 300

[Config ChordDht]
**.tier1Type = "oversim.applications.dht.DHTModules"

[Config Mine]
extends = ChordDht
**.tier1*.dht.numReplica = 6
**.tier1*.dht.ratioIdentical = 0.75
**.tier1*.dht.secureMaintenance = true
**.tier2*.dhtTestApp.testTtl = 120
"""


def test_ini_keys_bind_to_dht_params(tmp_path):
    from oversim_amd import DhtParams, KbrError
    p, ttl = DhtParams.from_ini(INI, "ChordDht")
    assert (p.numReplica, p.numGetRequests, p.ratioIdentical, ttl) == (4, 4, 0.5, 300)
    assert (p.secureMaintenance, p.invalidDataAttack, p.maintenanceAttack) == (0, 0, 0)
    p, ttl = DhtParams.from_ini(INI, "Mine")
    assert (p.numReplica, p.numGetRequests, p.ratioIdentical, p.secureMaintenance, ttl) == (6, 4, 0.75, 1, 120)
    p, ttl = DhtParams.from_ini("[General]\n", None, DhtParams.default().replace(numGetRequests=2))
    assert (p.numReplica, p.numGetRequests, ttl) == (4, 2, None)
    (tmp_path / "base.ini").write_text(INI)
    (tmp_path / "top.ini").write_text("[Config Top]\nextends = Mine\n**.tier1*.dht.numGetRequests = 3\ninclude ./base.ini\n")
    p, ttl = DhtParams.from_ini_file(tmp_path / "top.ini", "Top")
    assert (p.numReplica, p.numGetRequests, ttl) == (6, 3, 120)
    with pytest.raises(KbrError):
        DhtParams.from_ini("[General]\n**.tier1*.dht.numReplica = many\n")
    with pytest.raises(KbrError):
        DhtParams.from_ini(INI, "NoSuchConfig")


# ---------------------------------------------------------------- DHTTestApp statistics
def test_dhttest_stats_branch_rules_by_hand():
    put = np.zeros(3, dtype=D.PUT_DTYPE)
    put["outcome"] = [D.SUCCESS, D.FAILED, D.LOOKUP_FAILED]
    put["latency_ns"] = [2 * SEC, 3 * SEC, -1]
    put["hop_count"], put["messages"], put["bytes"] = [2, 3, 0], [8, 8, 0], [100, 100, 0]
    get = np.zeros(7, dtype=D.GET_DTYPE)
    get["outcome"] = [D.SUCCESS] * 5 + [D.FAILED, D.LOOKUP_FAILED]
    get["latency_ns"] = [SEC] * 6 + [-1]
    get["result_count"] = [1, 1, 0, 1, 0, 0, 0]
    get["value_token"] = [7, 8, 0, 7, 0, 0, 0]
    ops = D.make_ops(7, t0_ns=10 * SEC)
    ex = np.zeros(7, dtype=D.EXPECT_DTYPE)
    ex["token"], ex["known"] = 7, [1, 1, 1, 1, 1, 1, 1]
    ex["endtime_ns"] = [11 * SEC, 20 * SEC, 20 * SEC, 10 * SEC, 10 * SEC, 20 * SEC, 20 * SEC]
    ex["known"][1] = 1
    # get 0: the response at the very endtime is not "> endtime": right value, success.  1: wrong value.  2: no value.
    # 3: an expired key still answered.  4: expired and gone, success.  5: the DHT said no.  6: the lookup failed.
    st = D.dhttest_stats(4, put, [0, 1, 2], get, ops, [0, 0, 1, 1, 2, 2, 3], ex, 10.0)
    assert (st["num_put_success"], st["num_put_error"], st["num_get_success"], st["num_get_error"]) == (1, 2, 2, 5)
    assert (st["put_hop_count"], st["put_hop_sum"], st["get_hop_count"]) == (2, 5, 6)
    assert (st["normal_messages"], st["num_bytes_normal"]) == (16, 200)
    assert st["put_latency_s"] == dict(count=1, mean=2.0, stddev=0.0, min=2.0, max=2.0)
    assert st["get_latency_s"]["count"] == 6 and st["get_latency_sumsq_lo"] == 6 * SEC * SEC
    assert st["get_success_ratio"]["count"] == 4 and st["get_success_ratio"]["mean"] == (0.5 + 0 + 0.5 + 0) / 4
    ex["known"][0] = 0
    assert D.dhttest_stats(4, put, [0, 1, 2], get, ops, [0, 0, 1, 1, 2, 2, 3], ex, 10.0)["num_get_success"] == 1
    assert D.dhttest_stats(4, put, [0, 1, 2], get, ops, [0, 0, 1, 1, 2, 2, 3], ex, 0.05)["put_success_per_s"]["count"] == 0


def test_dhttest_layout_and_exports(tmp_path):
    import oversim_amd
    from oversim_amd import kbr
    exe = tmp_path / "abi_layout_dht"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "abi_layout_dht.c"), "-o", str(exe)], check=True)
    lay = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    rec = lay["ovs_dhttest_expect"]
    for dt in (kbr.DHT_EXPECT_DTYPE, D.EXPECT_DTYPE):
        assert dt.itemsize == rec["size"] == 24 and list(dt.names) == list(rec["fields"])
        for f, off in rec["fields"].items():
            assert dt.fields[f][1] == off, f
    st, cls = lay["ovs_dhttest_stats"], kbr.DhtTestStats
    assert C.sizeof(cls) == st["size"] and [f for f, _ in cls._fields_] == list(st["fields"])
    for f, off in st["fields"].items():
        assert getattr(cls, f).offset == off, f
    assert [f for f, _ in cls._fields_] == list(D.STAT_INTS + D.STAT_SDS)
    L = oversim_amd.lib()
    for name in ("ovs_dhttest_stats_batch", "ovs_dht_params_from_ini", "ovs_dht_params_from_ini_file"):
        assert hasattr(L, name), name
    assert callable(oversim_amd.KbrEngine.dhttest_stats) and callable(oversim_amd.DhtParams.from_ini_file)
