"""Window codes in the Chord finger entries (engine.hpp: finger_pack / finger_win_scan).

A finger entry carries its finger's gS0 on 48 bits and six 8-bit codes of the interior successor
distances; a lookup that arrives through the entry with K inside the finger's successor window picks
the successor from the codes and reads the WinRec only when a code ties with K's.  The GPU tests
compare every output field with the CPU oracle on rings where the coded path, the tie fallback, the
exact-key paths and the entries without codes are each taken; the CPU test checks the packing itself.
"""
from __future__ import annotations

import numpy as np
import pytest

from oversim_amd import KbrEngine, Params, workload as W
from oracle_lib import OracleNet, chord_params

gpu = pytest.mark.gpu
FIELDS = ("responsible", "hops", "status", "one_way_hops", "latency_ns")
LOOKUP_FIELDS = ("num_siblings", "hops", "status", "is_valid", "latency_ns")
M160 = (1 << 160) - 1


def _eq(a: dict, b: dict, label: str, hop_cols: int | None = None):
    for f in FIELDS:
        bad = np.nonzero(np.asarray(a[f]).astype(np.int64) != np.asarray(b[f]).astype(np.int64))[0]
        assert len(bad) == 0, f"{label}: {f} differs at {bad[:8]} gpu={np.asarray(a[f])[bad[:8]]} ref={np.asarray(b[f])[bad[:8]]}"
    if hop_cols is not None:
        assert np.array_equal(a["hop_seq"][:, :hop_cols], b["hop_seq"][:, :hop_cols]), f"{label}: hop sequences differ"


def _words(vals) -> np.ndarray:
    """160-bit Python ints -> (n, 5) uint32 words, w[0] least significant."""
    return np.array([[(v >> (32 * i)) & 0xFFFFFFFF for i in range(5)] for v in vals], dtype=np.uint32)


def _ints(ids: np.ndarray) -> list[int]:
    return [sum(int(w) << (32 * i) for i, w in enumerate(row)) for row in ids]


def _mixed_lookups(ids: np.ndarray, m: int, seed: int):
    """m node-ID keys and m random keys, random sources."""
    k1, s1 = W.lookups(ids, m, seed, node_ids=True)
    k2, s2 = W.lookups(ids, m, seed + 1, node_ids=False)
    return np.concatenate([k1, k2]), np.concatenate([s1, s2])


# ------------------------------------------------------------ 1. small rings, successorListSize 8

@gpu
@pytest.mark.parametrize("n", [5, 8, 9, 10, 11, 64, 1000])
def test_small_rings(engine: KbrEngine, n):
    """n = 9 is the smallest ring whose windows hold 8 successors (coded entries); on n = 5 and 8 the
    window is n - 1 < 8 successors, no entry carries codes and every window decision reads the WinRec."""
    net = W.population(n, 0x3C0 + n)
    engine.set_params(Params.chord())
    engine.chord_load(net.ids, net.xy)
    o = OracleNet("chord", net.ids, net.xy)
    keys, src = _mixed_lookups(net.ids, 2000, 0x3D0 + n)
    _eq(engine.lookup(keys, src, record_hops=True), o.route(keys, src, record_hops=True), f"n={n}", hop_cols=50)


# ------------------------------------------------------------ 2. forced ties

def _tie_ring():
    """64 nodes: 34 uniform IDs and three runs of 10 IDs spaced 2^140, 2^100 and 2^90 apart.  A window
    of 8 around a run spans about an eighth of the ring (gSL ~ 2^157 .. 2^158, one code step 2^150 or
    more), so the run's members share their code in every window that holds them; the 2^90 run also
    ties on the top 64 bits of the distances (closer than 2^96)."""
    rng = np.random.default_rng(0x71E5)
    vals = {int.from_bytes(rng.bytes(20), "little") for _ in range(34)}
    for step_bits in (140, 100, 90):
        base = int.from_bytes(rng.bytes(20), "little")
        vals |= {(base + i * (1 << step_bits)) & M160 for i in range(10)}
    vals = sorted(vals)
    assert len(vals) == 64
    return _words(vals), vals


@pytest.fixture(scope="module")
def tie_case():
    ids, vals = _tie_ring()
    xy = W.coordinates(len(ids), 0x71E6)
    rng = np.random.default_rng(0x71E7)
    keys = list(vals) + [(v + 1) & M160 for v in vals] + [(v - 1) & M160 for v in vals]
    # keys between the members of the runs: K's code equals the codes of the run
    for i in range(len(vals) - 1):
        gap = vals[i + 1] - vals[i]
        if gap < (1 << 145):
            keys += [vals[i] + int(rng.integers(1, 1 << 62)) * gap // (1 << 62) for _ in range(4)]
    keys = _words(keys)
    # every such key from 12 sources, and random keys
    keys = np.concatenate([np.repeat(keys, 12, axis=0), W.random_keys(2000, rng)])
    src = rng.integers(0, len(ids), len(keys)).astype(np.uint32)
    return ids, xy, np.ascontiguousarray(keys), src


@gpu
@pytest.mark.parametrize("rt", [0, 1])
def test_forced_ties(engine: KbrEngine, tie_case, rt):
    ids, xy, keys, src = tie_case
    engine.set_params(Params.chord().replace(routingType=rt))
    engine.chord_load(ids, xy)
    o = OracleNet("chord", ids, xy, chord_params(routingType=rt))
    _eq(engine.lookup(keys, src, record_hops=True), o.route(keys, src, record_hops=True), f"tie ring rt={rt}", hop_cols=50)


# ------------------------------------------------------------ 3. entries without codes

@gpu
@pytest.mark.parametrize("sls", [3, 16])
def test_entries_without_codes(engine: KbrEngine, sls):
    net = W.population(1000, 0x3E0 + sls)
    engine.set_params(Params.chord().replace(successorListSize=sls))
    engine.chord_load(net.ids, net.xy)
    o = OracleNet("chord", net.ids, net.xy, chord_params(successorListSize=sls))
    keys, src = _mixed_lookups(net.ids, 3000, 0x3E8 + sls)
    _eq(engine.lookup(keys, src, record_hops=True), o.route(keys, src, record_hops=True), f"successorListSize={sls}",
        hop_cols=50)


# ------------------------------------------------------------ 4. the other instantiations

@gpu
@pytest.mark.parametrize("n", [9, 11, 64, 1000])
def test_semi_recursive_and_lookup_calls(engine: KbrEngine, n):
    """The same rings through the semi-recursive route (hop-recording and not: two kernels) and
    through LookupCall batches with numSiblings 1 and 8."""
    net = W.population(n, 0x3C0 + n)
    keys, src = _mixed_lookups(net.ids, 2000, 0x3F0 + n)
    engine.set_params(Params.chord().replace(routingType=1))
    engine.chord_load(net.ids, net.xy)
    ref = OracleNet("chord", net.ids, net.xy, chord_params(routingType=1)).route(keys, src, record_hops=True)
    _eq(engine.lookup(keys, src, record_hops=True), ref, f"semi-recursive n={n}", hop_cols=50)
    _eq(engine.lookup(keys, src), ref, f"semi-recursive, no hop record, n={n}")
    engine.set_params(Params.chord())
    o = OracleNet("chord", net.ids, net.xy)
    # the one-way route without the hop record: the default-configuration kernel
    _eq(engine.lookup(keys, src), o.route(keys, src, record_hops=False), f"one-way, no hop record, n={n}")
    for ns in (1, 8):
        g, r = engine.lookupCall(keys, src, ns), o.lookup_call(keys, src, ns)
        for f in LOOKUP_FIELDS:
            assert np.array_equal(np.asarray(g[f]).astype(np.int64), np.asarray(r[f]).astype(np.int64)), (n, ns, f)
        assert np.array_equal(g["siblings"], r["siblings"]), (n, ns)


@gpu
@pytest.mark.parametrize("top", [0, 6])
def test_shard_step_two_arcs(top):
    """Two arcs of a 1000-node ring on one GPU (with and without replicated top finger levels): the
    shard step unpacks the re-packed entries, and decides windows through the WinRec as before."""
    import torch
    from oversim_amd.shard import GpuShardStepper, arc_bounds, done_to_numpy, route_local_shards
    world, n, m = 2, 1000, 3000
    net = W.population(n, 0x401)
    bounds = arc_bounds(n, world)
    dev = torch.device("cuda", 0)
    steppers = [GpuShardStepper(net.ids, net.xy, bounds, r, dev, capacity=world * m, params=Params.chord(), top_levels=top)
                for r in range(world)]
    ks, ss, qb, allk, alls = [], [], [], [], []
    for r in range(world):
        k, s = W.lookups(net.ids, m, 0x402 + r, node_ids=(r == 0))
        s = (bounds[r] + s.astype(np.int64) % (bounds[r + 1] - bounds[r])).astype(np.uint32)
        ks.append(torch.from_numpy(k).to(dev)); ss.append(torch.from_numpy(s).to(dev)); qb.append(r * m)
        allk.append(k); alls.append(s)
    for st in steppers:
        st.reset(world * m)
    dones, _ = route_local_shards(steppers, ks, ss, qb)
    d = np.concatenate([done_to_numpy(x) for x in dones])
    d = d[np.argsort(d["qid"])]
    assert np.array_equal(d["qid"], np.arange(world * m))
    ref = OracleNet("chord", net.ids, net.xy).route(np.concatenate(allk), np.concatenate(alls), record_hops=False)
    for f in FIELDS:
        assert np.array_equal(d[f].astype(np.int64), np.asarray(ref[f]).astype(np.int64)), f


# ------------------------------------------------------------ 5. the packing itself (no GPU)

def _msb(x: np.ndarray) -> np.ndarray:
    """Index of the highest set bit of nonzero uint64 values."""
    out = np.zeros(x.shape, dtype=np.int64)
    v = x.copy()
    for s in (32, 16, 8, 4, 2, 1):
        big = v >= (np.uint64(1) << np.uint64(s))
        out += np.where(big, s, 0)
        v = np.where(big, v >> np.uint64(s), v)
    return out


def test_packing_decides_or_ties():
    """The packing of engine.hpp rebuilt in numpy on a seeded 2^16-node ring: g_j = top64(succ_j - v),
    sh = max(msb(gSL) - 7, 0), code_j = g_j >> sh for j = 1..6.  Codes fit 8 bits and never decrease
    in j; for Dt inside the window, code_j != Dt >> sh decides g_j < Dt correctly; and the share of
    (node, Dt) pairs with a tying code -- those fall back to the WinRec -- is at most 10 % (a cap
    against a packing that always falls back, not a measurement: six codes at a resolution of 1/128
    to 1/256 of gSL tie with 2-5 % of the window)."""
    n = 1 << 16
    vals = _ints(W.sorted_unique_ids(n, 0xC0DE5))
    g = np.empty((n, 8), dtype=np.uint64)
    for j in range(8):
        g[:, j] = [((vals[(v + j + 1) % n] - vals[v]) & M160) >> 96 for v in range(n)]
    gSL = g[:, 7]
    assert np.all(gSL > 0)
    sh = np.maximum(_msb(gSL) - 7, 0).astype(np.uint64)
    codes = g[:, 1:7] >> sh[:, None]
    assert np.all(codes <= 255)
    assert np.all(codes[:, 1:] >= codes[:, :-1])
    rng = np.random.default_rng(0xC0DE6)
    roomy = np.nonzero(g[:, 7] - g[:, 0] > 1)[0]          # windows with a Dt strictly inside
    v = rng.choice(roomy, 100_000)
    Dt = rng.integers(g[v, 0] + np.uint64(1), g[v, 7], dtype=np.uint64)   # g_0 < Dt < g_7
    cD = Dt >> sh[v]
    cj, gj = codes[v], g[v, 1:7]
    decided = cj != cD[:, None]
    assert np.array_equal((cj < cD[:, None])[decided], (gj < Dt[:, None])[decided])
    # the scan's result where no code ties: the farthest successor short of Dt
    free = decided.all(axis=1)
    assert np.array_equal((cj < cD[:, None]).sum(axis=1)[free], (g[v] < Dt[:, None]).sum(axis=1)[free] - 1)
    tie_share = 1.0 - free.mean()
    print(f"tie share {tie_share:.4f}")
    assert tie_share <= 0.10
