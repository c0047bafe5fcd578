"""Pastry networks whose ids are not uniformly random, and the probe batches, models and comparators that
tests/test_pastry_model.py (CPU) and tests/test_gpu_pastry_deep.py (GPU) share -- test infrastructure only, never
calls the engine.

Uniformly random ids of a network of 1000 share about 16 bits, so their tables have four or five rows, every digit
lies in w[4] and no subtraction borrows through equal words.  The three families here reach what such ids never do:

  low_word   64 ids equal above w[0]: 128 shared bits, more than 128 / b rows of which the first 128 / b are empty,
             shared prefixes that end in w[0], and every k_sub between two ids borrows through equal middle words
  ladder(b)  0xA5..A5 and that key with one bit flipped, for every bit a digit of b bits can name: every shared
             prefix length occurs, the node 0xA5..A5 has an entry in every one of its 160 / b rows, and with b = 3
             the digits that straddle a 32-bit word (bits 31/32, 63/64, 95/96, 127/128) are live table slots
  wrap       0, 2^160 - 1 and ids within 2^40 of them on both sides: leaf sets and ring distances cross zero, the
             top table class ends at 2^160 and the classes are runs that touch both ends of the sorted ids

Two ids that differ only in bit 0 under bitsPerDigit = 3 share 159 // 3 = 53 digits, and the reference's
PastryRoutingTable::mergeNode then calls digitAt(53, .), whose getBitRange lies outside the key: no such network
exists in the reference.  checked() asserts that no family holds such a pair.
"""
from __future__ import annotations

import functools

import numpy as np

import refmodel_pastry as RP
from oversim_amd import workload as W
from oversim_amd.kbr import key_from_int

M = RP.M
NONE = 0xFFFFFFFF
FAMILIES = ("low_word", "ladder", "wrap")
SHAPES = [(1, 2), (2, 8), (3, 32), (4, 16)]                     # (bitsPerDigit, numberOfLeaves)
FORMS = [(0, 1), (1, 1), (0, 0)]                                # (optimizeLookup, useRegularNextHop)
FIXED_KEYS = (0, 1, M - 1, 1 << 159, (1 << 159) - 1, (1 << 64) - 1, 1 << 64, 1 << 96, (1 << 128) - 1)
ROUTE_FIELDS = ("responsible", "hops", "status", "one_way_hops", "latency_ns")


# --- the id families -------------------------------------------------------------------------------------------
def low_word(n: int = 64) -> list[int]:
    """The ids of test_gpu_pastry_broadcast.py::test_keys_that_differ_only_in_the_lowest_word."""
    rng = np.random.default_rng(64)
    low = np.sort(rng.choice(1 << 32, n, replace=False))
    high = (0x1234567 << 130 | 0x89ABCDEF << 40) & ~0xFFFFFFFF
    return sorted(high | int(w) for w in low)


def ladder(b: int) -> list[int]:
    """0xA5..A5 and its 160 (b = 3: 159) one-bit neighbours; bit j < 160 % b belongs to no digit."""
    base = int.from_bytes(b"\xA5" * 20, "big")
    return sorted([base] + [base ^ (1 << j) for j in range(160 % b, 160)])


def wrap(n: int = 48) -> list[int]:
    """0, 2^160 - 1, n / 2 ids just below 2^160 and n / 2 just above 0, offsets below 2^40."""
    rng = np.random.default_rng(48)
    off = rng.integers(2, 1 << 40, n)
    ids = sorted({0, M - 1} | {int(o) for o in off[:n // 2]} | {M - 1 - int(o) for o in off[n // 2:]})
    assert len(ids) == n + 2
    return ids


def checked(ids: list[int], b: int) -> list[int]:
    """ids, sorted and distinct, without a pair whose shared digits leave no digit to tell them apart."""
    assert all(x < y for x, y in zip(ids, ids[1:])) and 0 <= ids[0] and ids[-1] < M
    for x, y in zip(ids, ids[1:]):                   # sorted neighbours attain the longest shared prefix
        assert (RP.shared_prefix_length(x, y, b) + 1) * b <= 160, (hex(x), hex(y), b)
    return ids


@functools.lru_cache(maxsize=None)
def family(name: str, b: int):
    """(ids as sorted ints, ids as (n, 5) uint32 words, coordinates) of a family under bitsPerDigit = b."""
    ids = checked({"low_word": low_word, "wrap": wrap}[name]() if name != "ladder" else ladder(b), b)
    words = np.array([key_from_int(k) for k in ids], dtype=np.uint32)
    words.setflags(write=False)
    xy = W.coordinates(len(ids), 64)
    xy.setflags(write=False)
    return ids, words, xy


def probe_keys(ids: list[int], rng: np.random.Generator):
    """(keys (m, 5) uint32, sources (m,) uint32): every id, id + 1, id - 1, the point half-way to the ring successor
    (the isCloser tie), 64 random keys and FIXED_KEYS, each from a source drawn at random."""
    n = len(ids)
    ks = list(ids) + [(k + 1) % M for k in ids] + [(k - 1) % M for k in ids]
    ks += [(ids[i] + ((ids[(i + 1) % n] - ids[i]) % M) // 2) % M for i in range(n)]
    ks += [RP.to_int(k) for k in W.random_keys(64, rng)]
    ks += list(FIXED_KEYS)
    keys = np.array([key_from_int(k) for k in ks], dtype=np.uint32)
    return keys, rng.integers(0, n, len(ks)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def probes(name: str, b: int):
    keys, src = probe_keys(family(name, b)[0], np.random.default_rng(160 + b))
    keys.setflags(write=False)
    src.setflags(write=False)
    return keys, src


@functools.lru_cache(maxsize=None)
def model(name: str, b: int, L: int, opt: int = 0, reg: int = 1) -> RP.PastryNet:
    """The family's PastryNet on the converged-table rule, built once and left unchanged."""
    ids, _, xy = family(name, b)
    return RP.PastryNet(ids, xy, b, L, bool(opt), bool(reg))


@functools.lru_cache(maxsize=None)
def model_routes(name: str, b: int, L: int, opt: int, reg: int, rnr: int):
    keys, src = probes(name, b)
    want = RP.routes(model(name, b, L, opt, reg), keys, src, rec_num_redundant=rnr)
    for a in want.values():
        a.setflags(write=False)
    return want


def find_node_sources(m: RP.PastryNet, node, keys) -> dict:
    """Where findNode(key, 1, 1) at node[i] takes its next hop from, counted over the batch."""
    out = dict(self=0, leaf=0, table=0, closer=0, none=0, raised=0)
    for v, k in zip(node, keys):
        try:
            out[m.nodes[int(v)].find_node(RP.to_int(k), 1, 1)[1]["source"]] += 1
        except RP.PastryError:
            out["raised"] += 1
    return out


def status_census(r) -> dict:
    return {int(s): int((r["status"] == s).sum()) for s in np.unique(r["status"])}


# --- what the GPU tests compare with ---------------------------------------------------------------------------
def assert_routes(got, want, what=""):
    for f in ROUTE_FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, (what, f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])
    H = min(got["hop_seq"].shape[1], want["hop_seq"].shape[1])
    assert np.array_equal(got["hop_seq"][:, :H], want["hop_seq"][:, :H]), what
    assert np.all(got["hop_seq"][:, H:] == NONE) and np.all(want["hop_seq"][:, H:] == NONE), what


def find_node_want(m, node, keys, nr, ns, cols):
    out = np.full((len(node), cols), NONE, dtype=np.uint32)
    cnt, sib, st = (np.zeros(len(node), dtype=np.uint8) for _ in range(3))
    for i, (v, k) in enumerate(zip(node, keys)):
        try:
            res, info = m.nodes[int(v)].find_node(RP.to_int(k), nr, ns)
        except RP.PastryError:
            st[i] = 2
            continue
        out[i, :len(res)] = res
        cnt[i], sib[i], st[i] = len(res), info["sib"], 1 if info["err"] else 0
    return out, cnt, sib, st
