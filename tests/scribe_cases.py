"""Shared Scribe scenarios of tests/test_scribe_model.py, tests/test_gpu_scribe.py and the golden maker."""
from __future__ import annotations

import numpy as np

from oversim_amd import workload as W
from refmodel import to_int


def key_words(x: int) -> np.ndarray:
    return np.array([(x >> (32 * i)) & 0xFFFFFFFF for i in range(5)], dtype=np.uint32)


def scenario(n: int, seed: int = 7, ids=None, xy=None):
    """A ring of n nodes with four groups: 0 has a node ID as its key and its root among the members; 1 has a
    key between two nodes and a root that is no member; 2 has no members; 3's key is 1's plus one, so both
    share root and forwarders.  Duplicate pairs are included.  ids, xy: the n sorted ids and coordinates to use
    instead of a random population.  Returns (ids, xy, group_keys, members)."""
    if ids is None:
        net = W.population(n, 100 + n)
        ids, xy = net.ids, net.xy
    rng = np.random.default_rng(seed + n)
    r0 = 3 % n
    k1 = (to_int(ids[(n // 2) % n]) + 12345) % (1 << 160)
    gk = np.stack([ids[r0], key_words(k1), key_words((k1 + (1 << 159)) % (1 << 160)), key_words((k1 + 1) % (1 << 160))])
    root1 = int(np.searchsorted([to_int(w) for w in ids], k1)) % n
    m = max(1, min(n - 1, 40))
    mem0 = sorted(set(rng.choice(n, size=m, replace=False).tolist()) | {r0})
    others = [x for x in range(n) if x != root1] or [0]
    mem1 = rng.choice(others, size=min(len(others), m), replace=False).tolist()
    mem3 = rng.choice(others, size=min(len(others), max(1, m // 2)), replace=False).tolist()
    members = [(0, x) for x in mem0] + [(1, x) for x in mem1] + [(3, x) for x in mem3]
    members += members[:3]                                    # duplicate pairs
    return ids, xy, gk, np.array(members, dtype=np.uint32), root1


def messages(n: int, members, rng_seed: int = 5):
    """Publishes to every group from members, non-members and roots, each once routed and once to a known root."""
    rng = np.random.default_rng(rng_seed)
    mg, ms = [], []
    for g in range(4):
        for s in {0, n - 1, int(rng.integers(n)), int(members[0][1]), 3 % n}:
            mg.append(g)
            ms.append(s)
    mg, ms = np.array(mg * 2, np.uint32), np.array(ms * 2, np.uint32)
    known = np.repeat([0, 1], len(mg) // 2).astype(np.uint8)
    return mg, ms, known
