"""refmodel_rpc (the independent reading of the KBRTestApp RPC test) against the CPU oracle and by hand:
its message-by-message Chord call leg equals OracleNet.route field by field, its delay function equals
the oracle's on the same pairs, and the round trip obeys the rules the reference states (a caller that
is itself responsible, the timeout tie, dropped calls, the full-recursive way back, the statistics)."""
from __future__ import annotations

import numpy as np
import pytest

import refmodel
import refmodel_rpc as R
from oracle_lib import OracleNet, chord_params
from oversim_amd import workload as W

ROUTE_FIELDS = ("responsible", "hops", "status", "one_way_hops", "latency_ns")


def _batch(net, m, seed):
    k1, s1 = W.lookups(net.ids, m // 2, seed, node_ids=True)
    k2, s2 = W.lookups(net.ids, m - m // 2, seed + 1, node_ids=False)
    keys, src = np.concatenate([k1, k2]), np.concatenate([s1, s2])
    keys[:3] = net.ids[src[:3]]                       # callers that own the key
    return keys, src


@pytest.mark.parametrize("n,m", [(2, 20), (3, 30), (9, 60), (200, 150)])
@pytest.mark.parametrize("rt", [0, 1, 2])
@pytest.mark.parametrize("rnd", [0, 1])
@pytest.mark.parametrize("hcm", [50, 3])
def test_chord_call_leg_equals_oracle(n, m, rt, rnd, hcm):
    net = W.population(n, 0x52 + n)
    keys, src = _batch(net, m, 7)
    o = OracleNet("chord", net.ids, net.xy, chord_params(routingType=rt, simtimeRound=rnd, hopCountMax=hcm))
    want = o.route(keys, src, record_hops=False)
    got = R.chord_leg(refmodel.ChordRing(net.ids, net.xy, rnd=bool(rnd)), rt, hop_max=hcm)(keys, src)
    ok = np.asarray(want["status"]) == 0
    for f in ROUTE_FIELDS:
        a, b = np.asarray(got[f]).astype(np.int64), np.asarray(want[f]).astype(np.int64)
        # a failed lookup's hop counters are not part of the RPC (nobody answers): status decides
        sel = ok if f in ("hops", "one_way_hops") else slice(None)
        assert np.array_equal(a[sel], b[sel]), f
    if hcm == 3 and n == 200:
        assert (~ok).any() and ok.any()


@pytest.mark.parametrize("rnd", [0, 1])
def test_delay_equals_oracle(rnd):
    net = W.population(300, 5)
    o = OracleNet("chord", net.ids, net.xy, chord_params(simtimeRound=rnd))
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, 300, 400), rng.integers(0, 300, 400)
    a[:5] = b[:5]
    for nbytes in (R.response_bytes(100), R.route_bytes(100), 83, 87, R.response_bytes(1)):
        for x, y in zip(a, b):
            assert R.calc_delay(net.xy, int(x), int(y), nbytes, bool(rnd)) == o.delay_ns(int(x), int(y), nbytes)
    assert R.response_bytes(100) == 133 and R.route_bytes(100) == 186


def _fixed_leg(rows):
    def leg(keys, src):
        got = [rows[(refmodel.to_int(k), int(s))] for k, s in zip(keys, src)]
        return {f: np.array([g[i] for g in got], dtype=np.int64) for i, f in enumerate(ROUTE_FIELDS)}
    return leg


def test_round_trip_rules_by_hand():
    net = W.population(9, 3)
    ids, xy = net.ids, net.xy
    K = [refmodel.to_int(w) for w in ids]
    d = lambda a, b: R.calc_delay(xy, a, b, 133)
    # (key, src) -> responsible, hops, status, one_way_hops, latency
    rows = {(K[4], 4): (4, 0, 0, 0, 0), (K[5], 1): (5, 2, 0, 3, 400_000_000), (K[6], 2): (NONE_, 3, 3, 0, -1),
            (K[7], 3): (8, 1, 0, 2, 7)}
    keys, src = ids[[4, 5, 6, 7]], np.array([4, 1, 2, 3], np.uint32)
    out = R.rpc_batch(ids, xy, keys, src, _fixed_leg(rows), 0)
    assert [int(x) for x in out["outcome"]] == [0, 0, 1, 0]
    assert [int(x) for x in out["rtt_ns"]] == [0, 400_000_000 + d(5, 1), -1, 7 + d(8, 3)]
    assert [int(x) for x in out["hop_count"]] == [0, 4, 0, 3]
    assert [int(x) for x in out["responder"]] == [4, 5, NONE_, 8]
    assert [int(x) for x in out["call_latency_ns"]] == [0, 400_000_000, -1, 7]
    # the tie: a response that arrives at the instant of the timeout finds the timeout event ahead of it
    rtt = int(out["rtt_ns"][1])
    assert R.simtime(rtt * 1e-9, True) == rtt
    tie = R.rpc_batch(ids, xy, keys, src, _fixed_leg(rows), 0, rpc_key_timeout=rtt * 1e-9)
    assert int(tie["outcome"][1]) == R.TIMEOUT and int(tie["rtt_ns"][1]) == -1 and int(tie["hop_count"][1]) == 0
    assert int(tie["responder"][1]) == 5 and int(tie["outcome"][3]) == R.ANSWERED
    late = R.rpc_batch(ids, xy, keys, src, _fixed_leg(rows), 0, rpc_key_timeout=(rtt + 1) * 1e-9)
    assert int(late["outcome"][1]) == R.ANSWERED
    # statistics: lookupNodeIds drops the RPC another node answered (#3) and the timeout (#2)
    st = R.rpc_stats(out, ids, keys, src, 2.0, True, failure_latency=10.0)
    assert (st["num_sent"], st["num_delivered"], st["num_dropped"], st["num_timeout"]) == (4, 2, 2, 1)
    assert st["hop_count_sum"] == 4 and st["success_latency_sum_ns"] == rtt
    assert st["total_latency_mean_s"] == pytest.approx((rtt * 1e-9 + 20.0) / 4, rel=1e-15)
    assert st["bytes_dropped"] == 200 and st["status_count"][:4] == [3, 0, 0, 1]
    assert st["delivered_msgs_per_s"]["count"] == 9 and st["delivery_ratio"]["count"] == 4
    assert st["delivery_ratio"]["mean"] == pytest.approx(0.5)
    st2 = R.rpc_stats(out, ids, keys, src, 2.0, False)
    assert (st2["num_delivered"], st2["num_dropped"], st2["num_timeout"]) == (3, 1, 1)
    assert all(R.rpc_stats(out, ids, keys, src, 0.05)[f]["count"] == 0 for f in R.SD_FIELDS)


NONE_ = R.NONE


def test_full_recursive_way_back():
    net = W.population(9, 3)
    ids, xy = net.ids, net.xy
    K = [refmodel.to_int(w) for w in ids]
    rows = {(K[5], 1): (5, 2, 0, 2, 300), (K[1], 5): (1, 4, 0, 4, 900),           # answered: 2 + 4 hops
            (K[6], 2): (6, 1, 0, 1, 100), (K[2], 6): (NONE_, 0, 3, 0, -1),          # the way back is dropped
            (K[7], 3): (NONE_, 0, 3, 0, -1),                                        # the call is dropped: no response
            (K[8], 0): (8, 1, 0, 1, 50), (K[0], 8): (7, 2, 0, 2, 60)}               # the response ends elsewhere
    keys, src = ids[[5, 6, 7, 8]], np.array([1, 2, 3, 0], np.uint32)
    out = R.rpc_batch(ids, xy, keys, src, _fixed_leg(rows), 2)
    assert [int(x) for x in out["outcome"]] == [0, 1, 1, 1]
    assert int(out["rtt_ns"][0]) == 1200 and int(out["hop_count"][0]) == 6
    assert [int(x) for x in out["resp_status"]] == [0, 3, 0, 0]
    assert [int(x) for x in out["responder"]] == [5, 6, NONE_, 8]


def test_chord_full_recursive_on_a_ring():
    """On a converged ring the way back is a second clockwise route: with few hops allowed it is dropped
    more often than the call."""
    net = W.population(200, 0x52 + 200)
    keys, src = _batch(net, 150, 7)
    leg = R.chord_leg(refmodel.ChordRing(net.ids, net.xy), 2, hop_max=3)
    out = R.rpc_batch(net.ids, net.xy, keys, src, leg, 2)
    assert ((out["status"] == 0) & (out["resp_status"] != 0)).any()
    own = np.all(keys == net.ids[src], axis=1)
    assert own[:3].all() and (out["rtt_ns"][own] == 0).all() and (out["hop_count"][own] == 0).all()
    assert (out["outcome"][own] == R.ANSWERED).all()
