"""KBRTestApp RPC-test statistics on the GPU (ovs_kbrtest_rpc_stats_batch; k_stats_lookups over the RPC
records, oversim_amd/csrc/stats.hip) against tests/refmodel_rpc.rpc_stats over reference RPC records: integer
fields exact, fp64 fields by the rule tests/test_stats.py applies to the one-way statistics (1e-12
relative / absolute: the reference adds doubles in event order, so its own sums are order dependent)."""
from __future__ import annotations

import numpy as np
import pytest

import refmodel_rpc as R
from oversim_amd import KbrEngine, KbrError, Params
from test_gpu_rpc import chord_ref, load_chord, ring

pytestmark = pytest.mark.gpu
N_RPC = 777                          # not a multiple of 256
DOUBLES = ("hop_count_mean", "success_latency_mean_s", "total_latency_mean_s")


def check(gpu, ref):
    for f in R.INT_FIELDS:
        assert int(getattr(gpu, f)) == int(ref[f]), f
    assert list(gpu.status_count) == ref["status_count"] and list(gpu.hop_hist) == ref["hop_hist"]
    for f in DOUBLES:
        assert getattr(gpu, f) == pytest.approx(ref[f], rel=1e-12), f
    for f in R.SD_FIELDS:
        g, o = getattr(gpu, f), ref[f]
        assert g.count == o["count"], f
        for k in ("mean", "stddev", "min", "max"):
            assert getattr(g, k) == pytest.approx(o[k], rel=1e-12, abs=1e-12), (f, k)


def case(rt, node_ids):
    """Reference records on the 1000-node ring with hopCountMax = 3 (answered RPCs, dropped calls and, under
    full-recursive routing, dropped responses); node_ids: only the node-ID half of the batch."""
    keys, src, ref = chord_ref(1000, rt, 1, 3)
    ids = ring(1000).ids
    # test_gpu_rpc.batch: the first half are node IDs, the second uniform keys, which no node owns
    sel = np.arange(500) if node_ids else np.arange(500, 1000)
    return ids, np.ascontiguousarray(keys[sel]), np.ascontiguousarray(src[sel]), ref[sel].copy()


@pytest.mark.parametrize("rt", [0, 2])
@pytest.mark.parametrize("lookup_node_ids,node_ids", [(True, True), (True, False), (False, False)])
@pytest.mark.parametrize("T", [0.05, 120.0])       # below and above GlobalStatistics::MIN_MEASURED
def test_rpc_stats_match_reference(engine: KbrEngine, rt, lookup_node_ids, node_ids, T):
    ids, keys, src, out = case(rt, node_ids)
    ref = R.rpc_stats(out, ids, keys, src, T, lookup_node_ids, failure_latency=7.5)
    answered = int((out["outcome"] == R.ANSWERED).sum())
    assert 0 < answered < len(out)
    if lookup_node_ids and node_ids:
        assert 0 < ref["num_delivered"] <= answered
    elif lookup_node_ids:
        # uniform keys: every answered RPC was answered by a node whose key differs, and is dropped
        assert ref["num_delivered"] == 0 and ref["num_dropped"] == len(out) > ref["num_timeout"] > 0
    else:
        assert ref["num_delivered"] == answered
    load_chord(engine, 1000, rt, 1, 3)
    got = engine.kbrtest_rpc_stats(out, keys, src, T, lookupNodeIds=lookup_node_ids, failureLatency=7.5)
    check(got, ref)
    assert (ref["delivered_msgs_per_s"]["count"] == 1000) == (T >= 0.1)


def test_stats_of_the_engines_own_results(engine: KbrEngine):
    keys, src, ref = chord_ref(1000, 2, 1, 3)
    load_chord(engine, 1000, 2, 1, 3)
    res = engine.rpcCall(keys[:N_RPC], src[:N_RPC])
    got = engine.kbrtest_rpc_stats(res, keys[:N_RPC], src[:N_RPC], 120.0)
    ids, keys, src = ring(1000).ids, keys[:N_RPC], src[:N_RPC].copy()
    check(got, R.rpc_stats(ref[:N_RPC], ids, keys, src, 120.0))
    # crafted on top: two delivered RPCs with the hop counts 63 and 200, which both belong to the last histogram
    # bucket, and a delivered and a dropped RPC from sources that are no node (in the sums, in no node's counters)
    out = ref[:N_RPC].copy()
    ok = (out["outcome"] == R.ANSWERED) & (ids[np.minimum(out["responder"], 999)] == keys).all(axis=1)
    deliv, drop = np.flatnonzero(ok), np.flatnonzero(~ok)
    out["hop_count"][deliv[0]], out["hop_count"][deliv[1]] = 63, 200
    src[deliv[2]], src[drop[0]] = 1000, 0xFFFFFFF0
    want = R.rpc_stats(out, ids, keys, src, 120.0)
    assert want["hop_hist"][63] == 2 and want["hop_count_max"] == 200
    assert want["num_delivered"] == len(deliv) and want["delivery_ratio"]["count"] <= 1000
    check(engine.kbrtest_rpc_stats(out, keys, src, 120.0), want)


def test_bad_times_are_refused_and_results_unchanged(engine: KbrEngine):
    ids, keys, src, out = case(0, True)
    load_chord(engine, 1000, 0, 1, 3)
    ok = bytes(engine.kbrtest_rpc_stats(out, keys, src, 120.0))
    for kw, msg in ((dict(measured_time_s=-1.0), "measured_time_s must be >= 0"),
                    (dict(measured_time_s=float("nan")), "measured_time_s must be >= 0"),
                    (dict(measured_time_s=120.0, failureLatency=-1.0), "failure_latency_s must be >= 0"),
                    (dict(measured_time_s=120.0, failureLatency=float("nan")), "failure_latency_s must be >= 0")):
        with pytest.raises(KbrError, match="EINVAL: " + msg):
            engine.kbrtest_rpc_stats(out, keys, src, **kw)
        assert bytes(engine.kbrtest_rpc_stats(out, keys, src, 120.0)) == ok
    empty = engine.kbrtest_rpc_stats(out[:0], keys[:0], src[:0], 120.0)
    assert empty.num_sent == 0 and empty.delivered_msgs_per_s.count == 1000 and empty.delivery_ratio.count == 0
