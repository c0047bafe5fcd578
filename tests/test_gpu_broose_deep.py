"""Broose on the GPU (oversim_amd/csrc/broose.hip) on the crafted networks of tests/broose_rings.py, against the model
(tests/refmodel_broose.py, built through BrooseBucket::add): ids that differ only below the top word, distance
estimates up to the key length, and every bucket shape broose_shape_ok accepts.  Everything is exact equality.

tests/test_gpu_broose.py loads uniform ids only; there every 160-bit compare, split bit and shift of the engine is
decided in word 4.  What the rings here reach, counted by broose_rings.census from the model alone and asserted
positive in tests/test_broose_model.py (512 lookups a ring, default shape (8, 8, 2, 0)):

    ring  n    rows with     rows split below bit       nodes     max   isSiblingFor: top 32    finishes            with the ring's timeout
               top-64 ties   128 / 96 / 64 / 32         dist>31   dist  equal / == / +1 / -1    OK/NO_NEXT/BROKEN   RPC_TIMEOUT, retries (low-word)
    lb96  160  538           402 / 384 /   1 /   1       7         66   672 / 33 / 24 / 26      501 /  6 /  5       259, 168 (25)
    lb64   48  288           177 / 177 / 160 /  14       3         98   672 / 29 / 33 / 15      493 / 10 /  9       190, 141 (26)
    lb40  160  749           603 / 603 / 603 /  14      11        122   609 / 22 / 21 / 25      469 / 36 /  7       254, 151 (13)
    lb33   48  288           200 / 200 / 200 / 157       5        128   599 / 31 / 34 / 20      483 / 16 / 13       198, 144 (62)
    lb32  160  560           464 / 464 / 464 / 443      16        132   732 / 30 / 20 / 22      495 / 14 /  3       281, 167 (46)
    lb31   48  288           189 / 189 / 189 / 174       4        132   621 / 30 / 29 / 18      497 / 12 /  3       173, 109 (46)
    lb5   160  628           407 / 407 / 407 / 407      31        158   636 / 34 / 30 / 40      407 / 56 / 49       257, 150 (23)
    edge   48  164            53 /  53 /  53 /  53       0          4   118 / 35 / 32 / 30      512 /  0 /  0       154, 100 (0)

  - tie fallback of k_broose_rows' insertion sort: "top-64 ties" (two adjacent row entries whose distances to the
    bucket key agree in their top 64 bits);
  - split bits of the trie descent below each word boundary: lb96 splits at bit 95, lb64 at 63, lb33 at 32, lb32 at
    31 (the first two members of every run differ there), edge at bit 159 and below bit 8 with nothing between;
  - scan_row and its has_lo walk: run members' distances to a route key in the run differ in the low words only
    (the findNode answers of 8 nodes, and "retries (low-word)": first-hop timeouts whose second candidate agrees with
    the first in the top 32 bits of the distance);
  - dist > 31: the feeders of a run ring (rBucket[0] key inside a run) and whatever else chance gives; their
    left-shifting starts are BROKEN, their right-shifting rounds start at steps up to 158 and take the prefix bits
    across every word boundary (also fed directly: steps 32 .. 160, broose_rings.BIG_STEPS);
  - the dist > KEYBITS cap: reachable, on the pair rings (ids X, X ^ 1(, X ^ 2)) loaded with bucketSize 1: capped
    to 160 at (shiftingBits 2, userDist 2) and to 159 at shiftingBits 3 on pair2 and at (3, 2) on pair3; (2, 0)
    gives exactly 160 uncapped.  With bucketSize >= n every key is a sibling's and no estimate is made;
  - isSiblingFor in mode 0 at the range distance, one above and one below, from the source and at responders
    ("isSiblingFor" columns);
  - bucket shapes: each of broose_rings.SHAPES on lb40 and on the uniform 1000-node network (there with the model's
    trie build: feeding 1000 nodes through add takes 10 s a shape).

Measured on an MI355X: the 56 tests of this file take 5.1 s.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from oversim_amd import BrooseParams, KbrEngine, KbrError, Params, workload as W
from oversim_amd.kbr import BROOSE_EXT_DTYPE, key_from_int, key_to_int
import broose_cases as BC
import broose_rings as BR
import refmodel_broose as RB

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
NONE = 0xFFFFFFFF
MODEL_KW = dict(hopCountMax="hop_max", rpcUdpTimeout="rpc_to", lookupTimeout="lk_to")


def _bp(shape):
    k, kr, sb, ud = shape
    return BrooseParams.default(bucketSize=k, rBucketSize=kr, shiftingBits=sb, userDist=ud)


def _load(engine, name, shape=BR.DEFAULT_SHAPE, **pk):
    net = BR.ring(name)[0]
    engine.set_params(Params.broose().replace(**pk))
    engine.broose_load(net.ids, net.xy, _bp(shape))
    return net, BR.model(name, shape)


def _check_export(engine, m):
    off, nodes = engine.broose_export()
    woff, wnodes = m.csr()
    assert np.array_equal(off, np.array(woff, dtype=np.uint64))
    assert np.array_equal(nodes, np.array(wnodes, dtype=np.uint32))


def _arrays(calls):
    node = np.array([c[0] for c in calls], dtype=np.uint32)
    keys = np.array([key_from_int(c[1]) for c in calls], dtype=np.uint32)
    ext = np.array([BC.ext_record(c[2]) for c in calls], dtype=BROOSE_EXT_DTYPE)
    right = np.array([c[3] for c in calls], dtype=np.uint8)
    return node, keys, right, ext


def _check_find_node(engine, m, calls):
    """next hop, sibling flag, status and the outgoing extension of every call; then the calls again with several
    nodes per answer (the has_lo walk) and with numSiblings = 0"""
    node, keys, right, ext = _arrays(calls)
    out, cnt, sib, st, eo = engine.broose_find_node(node, keys, right, ext)
    for i, (v, k, e, r, cls, res, e2) in enumerate(calls):
        if cls == "broken":
            assert st[i] == 1 and cnt[i] == 0, i
            continue
        assert st[i] == 0 and cnt[i] == len(res) == 1 and int(out[i, 0]) == res[0], (i, cls)
        assert bool(sib[i]) == (cls == "sibling"), (i, cls)
        assert eo["has_ext"][i] == (e2 is not None), (i, cls)
        if e2 is not None:
            got = (key_to_int(eo["route_key"][i]), int(eo["step"][i]), bool(eo["right_shifting"][i]), int(eo["last_node"][i]))
            assert got == e2.tup() + (e2.last_node,), (i, cls)

    def again(nred, nsib, mo):
        o, c, s, t, _ = engine.broose_find_node(node, keys, right, ext, numRedundantNodes=nred, numSiblings=nsib, max_out=mo)
        for i, (v, k, e, r) in enumerate(c4[:4] for c4 in calls):
            try:
                res = m.find_node(v, k, nred, nsib, {} if e is None else {"ext": e.copy()}, r)
            except RB.BrooseError:
                assert t[i] == 1 and c[i] == 0, i
                continue
            assert t[i] == 0 and bool(s[i]) == m.is_sibling_for(v, k, nsib), i
            assert list(o[i, :c[i]]) == res and np.all(o[i, c[i]:] == NONE), (i, calls[i][4])

    again(min(8, m.k), min(4, m.k), 8)
    again(1, 0, 1)


def _check_routes(engine, name, shape, keys, src, right, **pk):
    """both simtimeRound rules, half of the batch each; returns the model's records of the whole batch"""
    kw = {MODEL_KW[p]: v for p, v in pk.items()}
    half = len(keys) // 2
    wants = []
    for rnd, sl in ((1, slice(0, half)), (0, slice(half, None))):
        _, m = _load(engine, name, shape, simtimeRound=rnd, **pk)
        got = engine.broose_lookup(keys[sl], src[sl], right[sl], record_hops=True, count_rpcs=True)
        want = BC.model_routes(BC.with_rounding(m, bool(rnd)), keys[sl], src[sl], right[sl], **kw)
        BC.assert_routes_equal(got, want, pk.get("hopCountMax", 50))
        wants.append(want)
    return {f: np.concatenate([w[f] for w in wants]) for f in ("status", "hops", "rpcs")}


def _pool_calls(name, m, total, seed):
    direct = BR.direct_calls(name, m, seed)
    members = [i for run in BR.ring(name)[1] for i in run]
    return BC.find_node_calls(m, len(direct) + total, seed + 1, direct=direct, key_pool=BR.key_pool(name, m, seed + 2),
                              node_pool=members)


# -- a. the snapshot

@pytest.mark.parametrize("name", BR.RINGS)
def test_export_equals_model_buckets(engine: KbrEngine, name):
    _, m = _load(engine, name)
    _check_export(engine, m)


# -- b. findNode

@pytest.mark.parametrize("name", BR.RINGS)
def test_find_node_equals_model(engine: KbrEngine, name):
    _, m = _load(engine, name)
    calls = _pool_calls(name, m, 600, 81)
    classes = {c[4] for c in calls}
    need = ["sibling", "first_left", "first_right", "mid_left", "mid_right", "brother", "loop"]
    for cls in need + (["broken"] if name in BR.RUN_RINGS else []):
        assert cls in classes, cls
    if name in BR.RUN_RINGS:
        # first calls at nodes whose estimate is above 31: left is refused, right starts at step == dist
        far = [c for c in calls if c[2] is None and m.distance_estimate(c[0]) > 31 and c[4] != "sibling"]
        assert any(c[4] == "broken" and not c[3] for c in far)
        # (one round of findNode has run when the answer leaves: the outgoing step is dist - shiftingBits)
        assert any(c[4] == "first_right" and c[6].step == m.distance_estimate(c[0]) - m.sb for c in far)
        # mid-route calls whose prefix bits sit in every word of the key
        assert {c[2].step for c in calls if c[2] is not None and c[2].right} >= {32, 34, 64, 66, 96, 128, 158, 160}
    _check_find_node(engine, m, calls)


@pytest.mark.parametrize("name", BR.PAIR_RINGS)
@pytest.mark.parametrize("shape", BR.PAIR_SHAPES)
def test_pair_rings(engine: KbrEngine, name, shape):
    """distance estimates of 160 (159 at shiftingBits 3), capped and not (test_broose_model.py
    test_pair_rings_reach_the_distance_cap): the snapshot, first calls in both directions, steps up to 160, routes"""
    _, m = _load(engine, name, shape)
    _check_export(engine, m)
    assert all(m.distance_estimate(v) == 160 - 160 % m.sb for v in range(m.n))
    direct = BR.direct_calls(name, m, 82)
    calls = BC.find_node_calls(m, len(direct), 83, direct=direct)
    classes = {c[4] for c in calls}
    assert {"broken", "mid_right"} <= classes and classes & {"first_right", "loop"}
    _check_find_node(engine, m, calls)
    want = _check_routes(engine, name, shape, *BR.batch(name, shape))
    assert (want["status"] == 0).any() and (want["status"] == 5).any() and (want["hops"] > 0).any()


# -- c. routes

@pytest.mark.parametrize("name", BR.RINGS)
def test_routes_equal_model(engine: KbrEngine, name):
    want = _check_routes(engine, name, BR.DEFAULT_SHAPE, *BR.batch(name))
    print(name, {int(s): int((want["status"] == s).sum()) for s in np.unique(want["status"])})
    assert (want["status"] == 0).sum() > 100
    if name in BR.RUN_RINGS:
        assert (want["status"] == 4).any() and (want["status"] == 5).any()


@pytest.mark.parametrize("name", BR.RINGS)
def test_rpc_timeouts(engine: KbrEngine, name):
    """an rpcUdpTimeout between the ring's smallest and largest round trip (from the model's delays): FindNodeCalls
    time out, and at the first hop the source's further candidates -- scan_row(..., has_lo) -- are tried"""
    to = BR.timeout_between(BR.model(name))
    want = _check_routes(engine, name, BR.DEFAULT_SHAPE, *BR.batch(name), rpcUdpTimeout=to)
    assert (want["status"] == 2).sum() > 20 and (want["rpcs"] > want["hops"] + 1).sum() > 20


def test_hop_limit(engine: KbrEngine):
    want = _check_routes(engine, "lb5", BR.DEFAULT_SHAPE, *BR.batch("lb5"), hopCountMax=3)
    assert (want["status"] == 3).sum() > 20


# -- d. bucket shapes

@pytest.mark.parametrize("shape", BR.SHAPES)
def test_bucket_shapes_on_a_clustered_ring(engine: KbrEngine, shape):
    name = BR.SHAPE_RING
    _, m = _load(engine, name, shape)
    _check_export(engine, m)
    _check_find_node(engine, m, _pool_calls(name, m, 400, 84))
    want = _check_routes(engine, name, shape, *BR.batch(name, shape))
    if shape[0] == 1:
        assert (want["status"] == 4).sum() > 400           # bucketSize 1: the expected end of almost every route


@pytest.mark.parametrize("shape", BR.SHAPES)
def test_bucket_shapes_on_uniform_ids(engine: KbrEngine, shape):
    net = BC.network(1000)
    k, kr, sb, ud = shape
    m = RB.BrooseNet(net.ids, net.xy, bucket_size=k, r_bucket_size=kr, user_dist=ud, shifting_bits=sb, build="fast")
    engine.set_params(Params.broose())
    engine.broose_load(net.ids, net.xy, _bp(shape))
    _check_export(engine, m)
    _check_find_node(engine, m, BC.find_node_calls(m, 512, 85))
    rng = np.random.default_rng(86)
    keys, src = W.random_keys(256, rng), rng.integers(0, 1000, 256).astype(np.uint32)
    right = rng.integers(0, 2, 256).astype(np.uint8)
    got = engine.broose_lookup(keys, src, right, record_hops=True, count_rpcs=True)
    BC.assert_routes_equal(got, BC.model_routes(m, keys, src, right), 50)


# -- e. explicit tables

def test_explicit_tables_on_a_clustered_ring(engine: KbrEngine):
    name = "lb40"
    net, m = _load(engine, name)
    keys, src, right = BR.batch(name)
    ideal = engine.broose_lookup(keys, src, right, record_hops=True, count_rpcs=True)
    BC.assert_routes_equal(ideal, BC.model_routes(m, keys, src, right), 50)
    off, nodes = engine.broose_export()
    engine.broose_load_tables(net.ids, net.xy, off, nodes)
    again = engine.broose_lookup(keys, src, right, record_hops=True, count_rpcs=True)
    for f in ideal:
        assert np.array_equal(ideal[f], again[f]), f
    o2, n2 = engine.broose_export()
    assert np.array_equal(o2, off) and np.array_equal(n2, nodes)
    # sparse tables: every second entry of each row dropped
    soff, snodes = [0], []
    for g in range(len(off) - 1):
        snodes.extend(nodes[int(off[g]):int(off[g + 1]):2])
        soff.append(len(snodes))
    engine.broose_load_tables(net.ids, net.xy, soff, snodes)
    o3, n3 = engine.broose_export()
    assert np.array_equal(o3, np.array(soff, dtype=np.uint64)) and np.array_equal(n3, np.array(snodes, dtype=np.uint32))
    sm = RB.BrooseNet(net.ids, net.xy, rows=(soff, snodes))
    got = engine.broose_lookup(keys, src, right, record_hops=True, count_rpcs=True)
    BC.assert_routes_equal(got, BC.model_routes(sm, keys, src, right), 50)
    # two run members swapped in a run member's bBucket row: out of XOR order in the low words only
    v = BR.ring(name)[1][1][3]
    g = v * m.nrows + m.P + 1
    a = int(off[g])
    d1, d2 = (m.ids[int(nodes[a + j])] ^ m.ids[v] for j in (1, 2))
    assert 0 < d1 < d2 < 1 << 40
    bad = nodes.copy()
    bad[a + 1], bad[a + 2] = nodes[a + 2], nodes[a + 1]
    with pytest.raises(KbrError, match="EINVAL"):
        engine.broose_load_tables(net.ids, net.xy, off, bad)
    assert np.array_equal(engine.broose_lookup(keys, src, right)["latency_ns"], got["latency_ns"])


# -- f. refusals at the shape limits

def test_shape_limits(engine: KbrEngine):
    name = "lb40"
    net, m = _load(engine, name)
    keys, src, right = BR.batch(name)
    base = engine.broose_lookup(keys, src, right, record_hops=True)
    calls = _pool_calls(name, m, 0, 87)
    for shape in ((8, 16, 3, 0), (9, 8, 2, 0), (8, 8, 0, 0)):
        with pytest.raises(KbrError, match="ENOTSUP"):
            engine.broose_load(net.ids, net.xy, _bp(shape))
        # the network loaded before still answers: export, findNode, routes
        _check_export(engine, m)
        _check_find_node(engine, m, calls)
        again = engine.broose_lookup(keys, src, right, record_hops=True)
        for f in base:
            assert np.array_equal(base[f], again[f]), (shape, f)
    engine.broose_load(net.ids, net.xy, _bp((8, 4, 4, 0)))
    _check_export(engine, BR.model(name, (8, 4, 4, 0)))


# -- the committed vectors

def test_golden_runs_reproduce(engine: KbrEngine):
    g = np.load(GOLD / "broose_runs_n160.npz")
    engine.set_params(Params.broose())
    engine.broose_load(g["ids"], g["xy"])
    off, nodes = engine.broose_export()
    R = 6
    for j, v in enumerate(g["sample_nodes"]):
        want = g["sample_rows"][j]
        for r in range(R):
            row = nodes[int(off[v * R + r]):int(off[v * R + r + 1])]
            assert np.array_equal(row, want[r][want[r] != NONE]), (v, r)
    out, cnt, sib, st, eo = engine.broose_find_node(g["fn_node"], g["fn_keys"], g["fn_right"], g["fn_ext"])
    assert np.array_equal(st, g["fn_status"]) and np.array_equal(sib, g["fn_sib"])
    ok = g["fn_status"] == 0
    assert np.array_equal(out[ok, 0], g["fn_next"][ok]) and np.all(cnt[~ok] == 0)
    for f in ("step", "route_key", "has_ext", "right_shifting", "last_node"):
        assert np.array_equal(eo[f][ok], g["fn_ext_out"][f][ok]), f
    got = engine.broose_lookup(g["keys"], g["src"], g["right"], record_hops=True, count_rpcs=True)
    for f in BC.FIELDS + ("rpcs",):
        assert np.array_equal(got[f], g[f]), f
    H = g["hop_seq"].shape[1]
    assert np.array_equal(got["hop_seq"][:, :H], g["hop_seq"]) and np.all(got["hop_seq"][:, H:] == NONE)
    assert {0, 4, 5} <= set(g["status"].tolist())
