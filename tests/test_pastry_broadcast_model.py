"""The Pastry overlay broadcast without a GPU: the event-ordered replay (tests/refmodel_pastry_broadcast.py)
shows what Pastry::forwardBroadcast does on tables whose slots keep their row's prefix -- every node receives
the request at most once, on the rule's tables exactly once, along the path a direct walk takes -- and the C ABI
declares and exports the batched call."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from oversim_amd import workload as W
import refmodel_pastry as RP
from refmodel_pastry_broadcast import NONE, PastryBroadcastReplay

ROOT = Path(__file__).resolve().parent.parent
SIZES = (2, 3, 9, 17, 40, 200, 1000)
SHAPES = ((4, 16), (1, 4), (2, 8))


def _initiators(n):
    return sorted({0, n - 1, n // 2, (7 * n) // 9})


@pytest.fixture(scope="module")
def replays():
    """(n, b) -> (replay, initiators, records, stats, receptions) with ttl 100, computed once."""
    out = {}
    for n in SIZES:
        net = W.population(n, 81)
        for b, L in SHAPES:
            rp = PastryBroadcastReplay(RP.PastryNet(net.ids, net.xy, b, L))
            init = _initiators(n)
            out[n, b] = (rp, init) + rp.run_batch(init, 100)
    return out


@pytest.mark.parametrize("b", [b for b, _ in SHAPES])
@pytest.mark.parametrize("n", SIZES)
def test_every_node_is_reached_exactly_once(replays, n, b):
    rp, init, rec, stats, rx = replays[n, b]
    assert np.all(rx == 1)
    rows = rp.net.num_rows()
    for i, s in enumerate(stats):
        assert s["duplicated"] == 0 and s["extra"] == 0 and s["expired"] == 0
        assert s["expected"] == s["actual"] == n
        assert s["messages"] == 2 * n - 1
        assert rec[i]["parent"][init[i]] == NONE and rec[i]["arrival_ns"][init[i]] == 0
        assert np.count_nonzero(rec[i]["parent"] == NONE) == 1
        assert rec[i]["hops"].max() <= rows <= 160 // b


@pytest.mark.parametrize("b", [b for b, _ in SHAPES])
@pytest.mark.parametrize("n", SIZES)
def test_hops_equal_the_direct_walk_and_ranks_follow_the_scan(replays, n, b):
    """A node's hop count is the length of the walk that takes slot (shared digits, next digit) at every node; a
    parent receives strictly earlier; the children of one node are ranked 0 .. c-1 in (row, column) order."""
    rp, init, rec, _, _ = replays[n, b]
    ids = rp.net.ids
    for i, s in enumerate(init):
        r = rec[i]
        assert [rp.walk(s, u) for u in range(n)] == r["hops"].tolist()
        kids = {}
        for v in range(n):
            p = int(r["parent"][v])
            if p == NONE:
                continue
            assert r["arrival_ns"][p] < r["arrival_ns"][v] and r["hops"][v] == r["hops"][p] + 1
            kids.setdefault(p, []).append(v)
        for p, ch in kids.items():
            ch.sort(key=lambda v: int(r["rank"][v]))
            assert [int(r["rank"][v]) for v in ch] == list(range(len(ch)))
            slots = []
            for v in ch:
                row = RP.shared_prefix_length(ids[p], ids[v], b)
                slots.append((row, (ids[v] >> (160 - (row + 1) * b)) & ((1 << b) - 1)))
            assert slots == sorted(slots) and len(set(slots)) == len(slots)


@pytest.mark.parametrize("b", [b for b, _ in SHAPES])
def test_ttl_below_the_depth_expires_at_level_ttl(replays, b):
    rp, init, full, _, _ = replays[1000, b]
    ttl = 2
    assert full["hops"].max() > ttl
    for i, s in enumerate(init):
        rec, st, rx = rp.run(s, ttl)
        reached = rec["arrival_ns"] >= 0
        assert st["duplicated"] == 0 and st["extra"] == 0
        assert np.all(rx[reached] == 1) and np.all(rx[~reached] == 0)
        # the nodes reached are the full tree's first levels, the expired ones exactly its level ttl
        assert np.array_equal(reached, full[i]["hops"] <= ttl)
        assert np.array_equal(rec[reached], full[i][reached])
        assert st["expired"] == np.count_nonzero(full[i]["hops"] == ttl) > 0
        assert st["actual"] == np.count_nonzero(full[i]["hops"] < ttl)
        # nothing lies beyond an expired node
        assert not np.any(np.isin(rec["parent"][reached], np.flatnonzero(reached & (rec["hops"] == ttl))))
        assert np.all(rec["parent"][~reached] == NONE)


def test_thinned_tables_lose_exactly_the_subtrees_behind_emptied_slots():
    """The network, seed and thinning of test_gpu_pastry.test_thinned_tables_take_the_closer_node_path: 30 % of
    the slots emptied.  Still no node twice; a node is reached iff its direct walk meets no emptied slot."""
    net = W.population(1000, 81)
    leaf, tab = RP.PastryNet(net.ids, net.xy).tables()
    thin = tab.copy()
    thin[np.random.default_rng(85).random(tab.shape) < 0.3] = RP.NONE
    rp = PastryBroadcastReplay(RP.PastryNet(net.ids, net.xy, tables=(leaf, thin)))
    for s in _initiators(1000):
        rec, st, rx = rp.run(s, 100)
        assert st["duplicated"] == 0 and st["extra"] == 0 and rx.max() == 1
        walks = [rp.walk(s, u) for u in range(1000)]
        reached = rec["arrival_ns"] >= 0
        assert np.array_equal(reached, np.array([w is not None for w in walks]))
        assert [w for w in walks if w is not None] == rec["hops"][reached].tolist()
        assert 1 < st["actual"] == np.count_nonzero(reached) < st["expected"] == 1000
        assert st["messages"] == 2 * st["actual"] - 1


def test_forward_and_forget_is_false_for_every_request_forward_broadcast_makes(replays):
    rp = replays[40, 4][0]
    assert rp.forward_and_forget(0, None) is False
    for v in range(40):
        for f, info in rp.forward_broadcast(v, None):
            assert info["midpoint"] is False and rp.forward_and_forget(f, info) is False
    # the branch itself: a midpoint request for a domain that holds a leaf but not the node is forwarded and forgotten
    ids = rp.net.ids
    leaf = next(x for x in rp.net.nodes[0].leaves if x is not None)
    assert rp.forward_and_forget(0, dict(limit=1, midpoint=True, start=ids[leaf], end=(ids[leaf] + 1) % RP.M))
    assert not rp.forward_and_forget(0, dict(limit=1, midpoint=True, start=ids[0], end=(ids[0] + 1) % RP.M))


def test_golden_fixture_is_what_the_replay_gives():
    """tests/golden/pastry_broadcast_n1000.npz against its generator's replay: the first case in full."""
    g = np.load(ROOT / "tests" / "golden" / "pastry_broadcast_n1000.npz")
    assert g["ids"].shape == (1000, 5) and len(g["cases"]) == 4
    ttl, rnd = (int(x) for x in g["cases"][0])
    rp = PastryBroadcastReplay(RP.PastryNet(g["ids"], g["xy"]), simtimeRound=rnd)
    rec, stats, _ = rp.run_batch(g["initiators"], ttl)
    assert np.array_equal(rec, g["records_0"])
    assert [[s[f] for f in ("expected", "actual", "expired", "messages", "bytes", "last_arrival_ns")] for s in stats] \
        == g["stats_0"].tolist()


def test_library_and_header_declare_the_call():
    import oversim_amd
    text = (ROOT / "include" / "ovs_kbr.h").read_text()
    assert "#define OVS_HAS_PASTRY_BROADCAST 1" in text and "#define OVS_ABI_VERSION 12" in text
    L = oversim_amd.lib()
    assert hasattr(L, "ovs_pastry_broadcast_batch") and L.ovs_abi_version() == 12
    assert hasattr(oversim_amd.KbrEngine, "pastry_broadcast") and hasattr(oversim_amd.KbrEngine, "pastry_broadcast_device")
