"""The iterative-lookup model on Pastry (tests/refmodel_pastry_iter.py) against properties that do not come from
itself: the owner of the key by brute force, createSiblingVector and findNode of refmodel_pastry at the nodes the
lookup names, the hop count as a count of distinct responders.  CPU only."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from oversim_amd import workload as W
import refmodel_pastry as RP
import refmodel_pastry_iter as RI

ROOT = Path(__file__).resolve().parent.parent
BIG_TO = 1e6        # an rpcUdpTimeout and a LOOKUP_TIMEOUT no RTT of the unit square reaches


def _net(n, seed=91, L=16, **kw):
    p = W.population(n, seed)
    return RP.PastryNet(p.ids, p.xy, number_of_leaves=L, **kw)


def _cases(m, nq, seed):
    rng = np.random.default_rng(seed)
    ks = [RP.to_int(k) for k in W.random_keys(nq, rng)]
    for i in range(0, nq, 4):
        ks[i] = m.ids[int(rng.integers(0, m.n))]
    if m.n <= 17:
        return [(k, s) for k in ks[:24] for s in range(m.n)]
    return list(zip(ks, (int(s) for s in rng.integers(0, m.n, nq))))


@pytest.mark.parametrize("n", [2, 3, 9, 17, 1000])
@pytest.mark.parametrize("ns", [1, 4, 8])
def test_lookup_properties(n, ns):
    m = _net(n)
    diff = total = 0
    for k, s in _cases(m, 256, 92 + n):
        r = RI.lookup(m, k, s, ns, rpc_to=BIG_TO, lk_to=BIG_TO)
        assert r["status"] != RI.RPC_TIMEOUT and r["status"] != RI.TIMEOUT
        seq = r["hop_seq"]
        # hops: the distinct responders other than the source; none repeats; without timeouts every call is answered
        assert s not in seq and len(set(seq)) == len(seq) == r["hops"]
        assert r["targets"][:len(seq)] == seq and r["rpcs"] == len(r["targets"])
        # every responder after the first target is the single node the responder before it names
        for prev, nxt in zip(seq, seq[1:]):
            assert m.nodes[prev].find_node(k, 1, ns)[0][0] == nxt
        if seq:
            first = m.nodes[s].find_node(k, m.L, ns)[0][0]
            assert seq[0] == first
            rt = RP.routes(m, [k], [s])
            if rt["status"][0] == RP.OK and rt["hops"][0] > 0:
                total += 1
                diff += int(rt["hop_seq"][0, 0] != first)
        if r["status"] == RI.OK:
            last = seq[-1] if seq else s
            assert r["siblings"][0] in m.owner(k)
            assert r["siblings"] == m.nodes[last].sibling_vector(k, ns)
            assert 1 <= len(r["siblings"]) <= ns and r["latency_ns"] >= 0 and (r["latency_ns"] > 0) == bool(seq)
        else:
            assert r["siblings"] == [] and r["latency_ns"] == -1
    print(f"n={n} ns={ns}: first FindNodeCall target differs from the semi-recursive first hop in {diff} of {total} routes")


@pytest.mark.parametrize("n", [9, 1000])
def test_first_target_without_regular_next_hop(n):
    """useRegularNextHop = false: the start vector is the ring-metric vector, so the first target is the known node
    closest to the key on the ring, which need not be the prefix-routing hop."""
    m = _net(n, regular=False)
    diff = total = 0
    for k, s in _cases(m, 128, 93):
        r = RI.lookup(m, k, s, 1, rpc_to=BIG_TO, lk_to=BIG_TO)
        if not r["hop_seq"]:
            continue
        nd = m.nodes[s]
        known = nd.table_nodes() + [x for x in nd.leaves if x is not None]
        assert RP.ring_dist(m.ids[r["hop_seq"][0]], k) == min(RP.ring_dist(m.ids[x], k) for x in known)
        total += 1
        diff += int(r["hop_seq"][0] != nd.find_node(k, 1, 1)[0][0])
    print(f"n={n}: ring-closest first target differs from findNode's next hop in {diff} of {total} lookups")
    if n == 1000:
        assert diff > 0


def test_timeouts_walk_the_start_vector():
    """An rpcUdpTimeout below the smallest RTT: every call times out, the path walks the source's whole answer in its
    order (handleTimeout, sendRpc) and fails; LOOKUP_TIMEOUT ends it where the walk is longer than it allows."""
    m = _net(1000)
    for k, s in _cases(m, 32, 94):
        want, info = m.nodes[s].find_node(k, m.L, 1)
        r = RI.lookup(m, k, s, 1, rpc_to=1e-6, lk_to=BIG_TO)
        if info["sib"]:
            assert r["status"] == RI.OK and r["rpcs"] == 0
            continue
        assert r["status"] == RI.RPC_TIMEOUT and r["targets"] == want and r["hops"] == 0
        r = RI.lookup(m, k, s, 1, rpc_to=1e-6, lk_to=3.5e-6)
        assert r["status"] == RI.TIMEOUT and r["targets"] == want[:4]


def test_message_lengths():
    # FindNodeCall 55 B + the 28 B extension + UDP/IP; a response 33 B + 26 B a node + the extension (+ 100 B auth)
    assert RI.call_bytes() == 111
    assert [RI.resp_bytes(i) for i in (0, 1, 8)] == [89, 115, 297]
    assert RI.resp_bytes(1, auth=True) == 215


def test_header_declares_the_entry_points():
    text = (ROOT / "include" / "ovs_kbr.h").read_text()
    assert "#define OVS_HAS_PASTRY_ITERATIVE 1" in text and "#define OVS_ABI_VERSION 12" in text
    assert "ovs_pastry_lookup_batch(" in text and "ovs_pastry_iterative_route_batch(" in text
