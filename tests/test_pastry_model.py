"""The Pastry model (tests/refmodel_pastry.py) checked on the CPU: the converged-table rule against what
PastryLeafSet::mergeNode builds and against a brute-force scan of all ids, delivered routes against the brute-force
owner, the isCloser tie, and the host-only logic (refusals, table validation, leaf replay, ini reader) as a
stand-alone program under the sanitizers."""
from __future__ import annotations

import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oversim_amd import workload as W
import pastry_cases as PC
import refmodel_pastry as RP
from refmodel_pastry import PastryNet, key_dist, ring_dist, shared_prefix_length

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("n", [2, 3, 9, 17, 18, 40])
@pytest.mark.parametrize("L", [2, 8, 16])
def test_leaf_rule_is_the_merge_replay(n, L):
    net = W.population(n, 5)
    m = PastryNet(net.ids, net.xy, 4, L, nodes=[])
    for v in range(n):
        want = m.rule_leaves(v)
        clockwise = [(v + 1 + j) % n for j in range(n - 1)]
        assert m.replay_leaves(v, clockwise) == want, v
        assert v not in want and len([x for x in want if x is not None]) == min(n - 1, L)
        if n > L + 1:
            for seed in range(3):
                order = list(clockwise)
                random.Random(seed * 100 + v).shuffle(order)
                assert m.replay_leaves(v, order) == want, (v, seed)
    if n - 1 >= L:
        # the predecessor sits in slot L/2 - 1, the successor in slot L/2
        assert m.rule_leaves(0)[L // 2 - 1] == n - 1 and m.rule_leaves(0)[L // 2] == 1


def _scan_rule(m, v):
    """Node v's rows by the rule and the two rows after them against a scan of all ids; rows past the key's last
    whole digit (bitsPerDigit = 3 leaves bit 0 over) do not exist."""
    ids, b = m.ids, m.b
    me = ids[v]
    rows = m.rule_rows(v)
    assert any(x is not None for x in rows[-1])
    for r in range(min(len(rows) + 2, 160 // b)):
        p = 160 - (r + 1) * b
        for c in range(1 << b):
            cls = [i for i, k in enumerate(ids)
                   if i != v and shared_prefix_length(k, me, b) >= r and ((k >> p) & ((1 << b) - 1)) == c
                   and (me >> (p + b)) == (k >> (p + b))]
            if ((me >> p) & ((1 << b) - 1)) == c:
                want = None
            elif not cls:
                want = None
            else:
                t = (me & ~(((1 << b) - 1) << p)) | (c << p)
                up = [i for i in cls if ids[i] >= t]
                want = min(up, key=lambda i: ids[i]) if up else min(cls, key=lambda i: ids[i])
            got = rows[r][c] if r < len(rows) else m.rule_entry(v, r, c)
            assert got == want, (v, r, c)
            if want is not None:
                assert shared_prefix_length(ids[want], me, b) == r


@pytest.mark.parametrize("b", [1, 2, 3, 4])
def test_table_rule_is_a_brute_force_scan(b):
    net = W.population(300, 6)
    m = PastryNet(net.ids, net.xy, b, 16, nodes=[])
    for v in random.Random(b).sample(range(300), 12):
        _scan_rule(m, v)


@pytest.mark.parametrize("b", [1, 2, 3, 4])
@pytest.mark.parametrize("name", PC.FAMILIES)
def test_table_rule_on_the_deep_families(name, b):
    """Every node of tests/pastry_cases.py's families: tables of 33 to 160 rows, classes that start at index 0 or
    end at n, the class whose upper bound is 2^160, digits that straddle a word."""
    ids, _, xy = PC.family(name, b)
    m = PastryNet(ids, xy, b, 16, nodes=[])
    for v in range(m.n):
        _scan_rule(m, v)
    rows = m.num_rows()
    if name == "low_word":
        assert 128 // b < rows <= 160 // b
        assert all(all(x is None for x in row) for row in m.rule_rows(0)[:128 // b])
    if name == "ladder":
        base = ids.index(int.from_bytes(b"\xA5" * 20, "big"))
        assert rows == m.num_rows(base) == 160 // b
        assert all(sum(x is not None for x in row) == b for row in m.rule_rows(base))     # one a bit of the digit
    if name == "wrap":
        top = m.rule_rows(0)[0]                                  # node 0's first row: the class that ends at 2^160
        assert top[(1 << b) - 1] is not None and ids[top[(1 << b) - 1]] >> (160 - b) == (1 << b) - 1


@pytest.mark.parametrize("b,L", PC.SHAPES)
@pytest.mark.parametrize("name", PC.FAMILIES)
def test_deep_family_routes_end_at_the_owner(name, b, L):
    """RP.routes over the families' probe keys in the three forms of the next hop: a delivered route ends at
    PastryNet.owner(key).  The census is what tests/test_gpu_pastry_deep.py relies on."""
    keys, src = PC.probes(name, b)
    for opt, reg in PC.FORMS:
        m = PC.model(name, b, L, opt, reg)
        for rnr in (1, 3):
            want = PC.model_routes(name, b, L, opt, reg, rnr)
            ok = want["status"] == RP.OK
            for i in np.flatnonzero(ok):
                assert int(want["responsible"][i]) in m.owner(RP.to_int(keys[i])), (opt, reg, rnr, i)
                assert (want["hops"][i] == 0) == (want["responsible"][i] == src[i])
            if L == 2 and rnr == 3:
                assert (want["status"] == RP.BROKEN).all()       # numRedundantNodes > numberOfLeaves: findNode throws
            else:
                assert ok.mean() >= 0.95, (opt, reg, rnr, PC.status_census(want))


def test_key_arithmetic():
    a, k = 5, RP.M - 3
    assert key_dist(a, k) == ring_dist(a, k) == ring_dist(k, a) == 8
    assert key_dist(7, 7) == 0 and ring_dist(1 << 159, 0) == 1 << 159
    assert shared_prefix_length(0, 1 << 159) == 0 and shared_prefix_length(1, 0) == 159
    assert shared_prefix_length(9, 9, 4) == 160 and shared_prefix_length(0xF0 << 152, 0xF8 << 152, 4) == 1


@pytest.mark.parametrize("b,L,opt,rnr", [(4, 16, False, 3), (4, 16, True, 1), (2, 8, False, 3), (1, 2, False, 2)])
def test_delivered_routes_end_at_the_owner(b, L, opt, rnr):
    net = W.population(500, 7)
    m = PastryNet(net.ids, net.xy, b, L, opt)
    rng = np.random.default_rng(8)
    keys = [RP.to_int(k) for k in W.random_keys(300, rng)]
    src = rng.integers(0, 500, 300)
    delivered = 0
    for k, s in zip(keys, src):
        r = m.route(k, int(s), rec_num_redundant=rnr)
        if r["status"] == RP.OK:
            delivered += 1
            best = min(range(500), key=lambda i: key_dist(m.ids[i], k))
            assert key_dist(m.ids[r["responsible"]], k) == key_dist(m.ids[best], k)
            assert r["hops"] == len(r["hop_seq"]) and (r["hops"] == 0) == (r["responsible"] == s)
    assert delivered >= 297


def test_node_id_keys_and_the_is_closer_tie():
    net = W.population(64, 9)
    m = PastryNet(net.ids, net.xy, 4, 8)
    ids = m.ids
    for s in range(0, 64, 5):
        for v in range(64):
            r = m.route(ids[v], s)
            assert r["status"] == RP.OK and r["responsible"] == v
    # a key half-way between two ids: isCloser is strict, so each of the two keeps a message that reaches it
    ties = 0
    for v in range(63):
        gap = ids[v + 1] - ids[v]
        if gap % 2:
            continue
        k = ids[v] + gap // 2
        ties += 1
        assert m.nodes[v].is_closest_node(k) and m.nodes[v + 1].is_closest_node(k)
        assert m.owner(k) == (v, v + 1)
        for s in (0, 17, 40, 63):
            r = m.route(k, s)
            assert r["status"] == RP.OK and r["responsible"] in (v, v + 1)
        assert m.route(k, v)["responsible"] == v and m.route(k, v + 1)["responsible"] == v + 1
    assert ties > 5


def test_sibling_vector_null_and_unlimited():
    net = W.population(40, 10)
    m = PastryNet(net.ids, net.xy, 4, 8)
    nd = m.nodes[3]
    k = m.ids[3] + 1
    assert nd.sibling_vector(k, 1) == [3]
    assert nd.sibling_vector(k, 0) is None                     # maxSize 0: every leaf is in it, the full set's ends too
    assert nd.is_sibling_for(k, 0) == (False, True)
    assert nd.is_sibling_for(k, 4) == (True, False) and len(nd.sibling_vector(k, 4)) == 4
    far = m.ids[20]
    assert nd.is_sibling_for(far, 4) == (False, True)
    res, info = nd.find_node(far, 8, 4)
    assert info["err"] and len(res) in (8, 9) and res[0] == nd.find_node(far, 1, 1)[0][0]


def test_host_driver_under_sanitizers(tmp_path):
    """tests/pastry_host_driver.cpp: refusals, table validation and the ini reader as a stand-alone program built
    with -fsanitize=address,undefined; its leaf replay of small networks equals the model's."""
    exe = tmp_path / "pastry_host_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "oversim_amd" / "csrc"),
                    str(ROOT / "tests" / "pastry_host_driver.cpp"), str(ROOT / "oversim_amd" / "csrc" / "ovs_ini.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("ok")
    seen = 0
    for line in r.stdout.splitlines():
        if not line.startswith("leaves "):
            continue
        head, vals = line.split(":")
        _, n, L, v = head.split()
        n, L, v = int(n), int(L), int(v)
        ids = [((3 * j + 1) << 152) + j for j in range(n)]
        m = PastryNet(ids, None, 4, L, nodes=[])
        assert [None if x == "-1" else int(x) for x in vals.split()] == m.rule_leaves(v), line
        seen += 1
    assert seen > 20
    # key160.hpp / pastry_host.hpp arithmetic against Python ints: k_sub, k_add, p_ring_dist, p_spl_bits, k_lt on
    # pairs whose borrows and carries run through equal or saturated words, and p_digit at every position
    pairs = digits = 0
    for line in r.stdout.splitlines():
        f = line.split()
        if f and f[0] == "arith":
            a, c, sub, add, dist = (int(x, 16) for x in f[1:6])
            assert sub == (a - c) % RP.M and add == (a + c) % RP.M and dist == ring_dist(a, c) == key_dist(a, c), line
            assert int(f[6]) == shared_prefix_length(a, c) and int(f[7]) == int(a < c), line
            pairs += 1
        elif f and f[0] == "digits":
            b, a = int(f[1]), int(f[2], 16)
            assert [int(x) for x in f[3:]] == [(a >> (160 - (n + 1) * b)) & ((1 << b) - 1) for n in range(160 // b)], line
            digits += 1
    assert pairs == 13 * 13 and digits == 13 * 4
