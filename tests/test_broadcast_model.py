"""The Chord overlay broadcast without a GPU: the event-ordered replay (tests/refmodel_broadcast.py)
shows what Chord::forwardBroadcast does on a converged ring -- every node receives the request
exactly once, so the tree can be built level by level -- and the C ABI declares and exports the
batched call with the layouts the bindings mirror."""
from __future__ import annotations

import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oversim_amd import workload as W
from refmodel import M, to_int
from refmodel_broadcast import NONE, BroadcastReplay

ROOT = Path(__file__).resolve().parent.parent
RINGS = (1, 2, 3, 9, 64, 1000)


@pytest.fixture(scope="module")
def replays():
    """n -> (replay, initiators, records, stats, receptions) with ttl 100, computed once."""
    out = {}
    for n in RINGS:
        net = W.population(n, 40 + n)
        rp = BroadcastReplay(net.ids, net.xy)
        init = sorted({0, n - 1, n // 2, (7 * n) // 9})
        out[n] = (rp, init) + rp.run_batch(init, 100)
    return out


@pytest.mark.parametrize("n", RINGS)
def test_every_node_is_reached_exactly_once(replays, n):
    _, init, rec, stats, rx = replays[n]
    assert np.all(rx == 1)
    for b, s in enumerate(stats):
        assert s["duplicated"] == 0 and s["expired"] == 0
        assert s["expected"] == s["actual"] == n
        assert s["messages"] == 2 * n - 1
        assert rec[b]["parent"][init[b]] == NONE and rec[b]["arrival_ns"][init[b]] == 0
        assert np.count_nonzero(rec[b]["parent"] == NONE) == 1


@pytest.mark.parametrize("n", RINGS)
def test_tree_order(replays, n):
    """A parent receives strictly earlier, a child is one hop further, and the children of one node
    are ranked 0 .. c-1 by descending ring distance from it (highest finger first)."""
    rp, init, rec, _, _ = replays[n]
    for b in range(len(init)):
        r = rec[b]
        kids = {}
        for v in range(n):
            p = int(r["parent"][v])
            if p == NONE:
                continue
            assert r["arrival_ns"][p] < r["arrival_ns"][v]
            assert r["hops"][v] == r["hops"][p] + 1
            kids.setdefault(p, []).append(v)
        for p, ch in kids.items():
            ch.sort(key=lambda v: int(r["rank"][v]))
            assert [int(r["rank"][v]) for v in ch] == list(range(len(ch)))
            dist = [(rp.keys[v] - rp.keys[p]) % M for v in ch]
            assert dist == sorted(dist, reverse=True) and len(set(dist)) == len(dist)


def test_ttl_3_expires_at_hop_3(replays):
    rp = replays[1000][0]
    rec, st, rx = rp.run(123, 3)
    reached = rec["arrival_ns"] >= 0
    assert st["duplicated"] == 0 and np.all(rx[reached] == 1) and np.all(rx[~reached] == 0)
    assert rec["hops"][reached].max() == 3
    assert st["expired"] == np.count_nonzero(reached & (rec["hops"] == 3)) > 0
    assert st["actual"] == np.count_nonzero(reached & (rec["hops"] < 3))
    assert 0 < np.count_nonzero(reached) < 1000
    # nothing lies beyond an expired node
    assert not np.any(np.isin(rec["parent"][reached], np.flatnonzero(reached & (rec["hops"] == 3))))
    assert np.all(rec["parent"][~reached] == NONE)


def test_message_lengths():
    """The issue's derivation: 60 B call (65 B + 28 B on the wire) with an empty query, 34 B response,
    134 B with the auth block."""
    import refmodel_broadcast as R
    assert R.byte_length(R.request_bits(0)) == 60
    assert R.byte_length(R.BASEAPPDATA_L + R.request_bits(0)) + R.UDP_IP_BYTES == 93
    assert R.byte_length(R.request_bits(37)) == 65
    assert R.byte_length(R.response_bits(False)) == 34 and R.byte_length(R.response_bits(True)) == 134


def test_library_exports_the_broadcast():
    import oversim_amd
    L = oversim_amd.lib()
    assert hasattr(L, "ovs_chord_broadcast_batch")
    assert L.ovs_abi_version() == 12


def test_broadcast_struct_layout(tmp_path):
    from oversim_amd import kbr
    exe = tmp_path / "abi_layout_broadcast"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "abi_layout_broadcast.c"), "-o", str(exe)], check=True)
    lay = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert lay["abi"] == 12
    node, dt = lay["ovs_bcast_node"], kbr.BCAST_NODE_DTYPE
    assert dt.itemsize == node["size"] == 16 and list(dt.names) == list(node["fields"])
    for f, off in node["fields"].items():
        assert dt.fields[f][1] == off, f
    st, cls = lay["ovs_bcast_stats"], kbr.BcastStats
    assert C.sizeof(cls) == st["size"] and [f for f, _ in cls._fields_] == list(st["fields"])
    for f, off in st["fields"].items():
        assert getattr(cls, f).offset == off, f
