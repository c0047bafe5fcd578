"""ovs_scribe_build / ovs_scribe_multicast_batch on a Pastry context (ovs_pastry_load) against
tests/refmodel_scribe_pastry.py and the golden fixture, bit for bit, plus cross-checks against the engine's own
recorded Pastry routes that use no model, the refusals, and a Chord context left untouched by a Pastry one."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

import refmodel_scribe as RS
import refmodel_scribe_pastry as RSP
from oversim_amd import KbrEngine, KbrError, Params, PastryParams, workload as W
from oversim_amd.kbr import NONE
from refmodel import to_int
from scribe_cases import key_words, messages, scenario

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"


def _pp(**kw):
    return PastryParams.default(routeMsgAcks=0, **kw)


def _load(engine, ids, xy, b=4, L=16, opt=0, reg=1, **kw):
    p = Params.pastry().replace(**kw)
    engine.set_params(p)
    engine.pastry_load(ids, xy, _pp(bitsPerDigit=b, numberOfLeaves=L, optimizeLookup=opt, useRegularNextHop=reg))
    return RSP.ScribePastryModel(ids, xy, hopCountMax=p.hopCountMax, simtimeRound=p.simtimeRound, datarate=p.datarate,
                                 accessDelay=p.accessDelay, bitsPerDigit=b, numberOfLeaves=L, optimizeLookup=bool(opt),
                                 useRegularNextHop=bool(reg), recNumRedundantNodes=p.recNumRedundantNodes)


def _check_forest(engine, M, gk, members):
    state = M.closure(gk, members)
    ref = RS.ScribeModel.records(state)
    nodes, edges, rooted = engine.scribe_build(gk, members[:, 0], members[:, 1])
    rec = engine.scribe_export()
    assert rec.tolist() == ref.tolist()
    assert nodes == len(ref) and edges == sum(len(S["children"]) for S in state.values())
    assert rooted == int(np.count_nonzero(ref["flags"] & RS.ROOT))
    return state, rec


def _check_multicast(engine, M, state, gk, mg, ms, known, payload=100):
    out, deliv = engine.scribe_multicast(mg, ms, known, payload)
    ref, rdeliv = M.multicast(state, gk, mg, ms, known, payload)
    assert RS.msg_mismatches(out, ref) == []
    assert deliv.tolist() == rdeliv.tolist()
    return out, deliv


@pytest.mark.parametrize("b,L", [(4, 16), (1, 4), (2, 8)])
@pytest.mark.parametrize("n", [2, 3, 9, 17, 200])
def test_forest_and_publishes_match_the_model(engine: KbrEngine, n, b, L):
    """A group key equal to a node ID, a member that is the root, a sibling that is no member, duplicate pairs, a
    group without members (wrong root, no deliveries), two groups sharing forwarders, the known-rendezvous flag, both
    rounding rules; n <= L: host-replayed leaf sets, n = 17: the first rule-built leaf set at L = 16."""
    ids, xy, gk, members, _ = scenario(n)
    mg, ms, known = messages(n, members)
    for kw in (dict(), dict(simtimeRound=0), dict(recNumRedundantNodes=1)):
        M = _load(engine, ids, xy, b, L, **kw)
        state, rec = _check_forest(engine, M, gk, members)
        out, deliv = _check_multicast(engine, M, state, gk, mg, ms, known)
        assert np.all(out["status"][mg == 2] == RS.WRONG_ROOT) and np.all(out["receivers"][mg == 2] == 0)
        assert np.all(out["status"][mg != 2] == RS.OK) and not np.any(deliv["msg"][:, None] == np.flatnonzero(mg == 2))
    own1 = M.net.owner(to_int(gk[1]))
    r1 = rec[(rec["group"] == 1) & (rec["parent"] == rec["node"])]
    assert len(r1) == 1 and int(r1["node"][0]) in own1
    if n == 200:
        a = {(x, p) for g, x, p in zip(rec["group"], rec["node"], rec["parent"]) if g == 1 and p != x}
        c = {(x, p) for g, x, p in zip(rec["group"], rec["node"], rec["parent"]) if g == 3 and p != x}
        assert a & c, "groups 1 and 3 share forwarders"


@pytest.mark.parametrize("opt,reg", [(1, 1), (0, 0), (1, 0)])
def test_both_forms_of_the_next_hop(engine: KbrEngine, opt, reg):
    ids, xy, gk, members, _ = scenario(200)
    mg, ms, known = messages(200, members)
    M = _load(engine, ids, xy, opt=opt, reg=reg)
    state, _ = _check_forest(engine, M, gk, members)
    _check_multicast(engine, M, state, gk, mg, ms, known)


def test_hop_limits(engine: KbrEngine):
    """hopCountMax = 0 leaves every member parentless; 2 cuts nothing; 1 against the engine's own recorded routes, no
    model: a member has a parent iff its route is at most one hop long, and that parent is the route's end."""
    ids, xy, gk, members, _ = scenario(200)
    mg, ms, known = messages(200, members)
    M = _load(engine, ids, xy, hopCountMax=0)
    state, rec = _check_forest(engine, M, gk, members)
    assert np.all(rec["parent"] == NONE) and np.all(rec["flags"] == RS.SUBSCRIBER)
    out, _ = _check_multicast(engine, M, state, gk, mg, ms, known)
    assert np.all(out["status"] == RS.ROUTE_FAILED)      # no root to know, and sendToKey drops at the source
    M = _load(engine, ids, xy, hopCountMax=2)
    state, rec2 = _check_forest(engine, M, gk, members)
    _check_multicast(engine, M, state, gk, mg, ms, known)
    M50 = _load(engine, ids, xy)
    engine.scribe_build(gk, members[:, 0], members[:, 1])
    assert engine.scribe_export().tolist() == rec2.tolist() and not np.any(rec2["parent"] == NONE)
    # 1: the full routes first (hopCountMax 50), then the forest under the limit
    r = engine.pastry_lookup(gk[members[:, 0]], members[:, 1], record_hops=True)
    assert np.all(r["status"] == 0) and 0 < np.count_nonzero(r["hops"] <= 1) < len(members)
    M1 = _load(engine, ids, xy, hopCountMax=1)
    engine.scribe_build(gk, members[:, 0], members[:, 1])
    rec = engine.scribe_export()
    parent = {(int(g), int(x)): int(p) for g, x, p in zip(rec["group"], rec["node"], rec["parent"])}
    expect = {}
    for (g, x), h, R in zip(members.tolist(), r["hops"], r["responsible"]):
        expect[(g, x)] = int(R) if h <= 1 else NONE
        if h <= 1:
            expect[(g, int(R))] = int(R)
    assert parent == expect
    assert rec.tolist() == RS.ScribeModel.records(M1.closure(gk, members)).tolist()


def test_every_route_hop_is_a_forest_edge(engine: KbrEngine):
    """No model, n = 1000: the recorded hops of every member's route to its group key are (child, parent) edges of
    the exported forest, and every forest node lies on one of them."""
    ids, xy, gk, members, _ = scenario(1000)
    _load(engine, ids, xy)
    engine.scribe_build(gk, members[:, 0], members[:, 1])
    rec = engine.scribe_export()
    parent = {(int(g), int(x)): int(p) for g, x, p in zip(rec["group"], rec["node"], rec["parent"])}
    r = engine.pastry_lookup(gk[members[:, 0]], members[:, 1], record_hops=True)
    assert np.all(r["status"] == 0) and r["hops"].max() >= 2
    seen = set()
    for (g, x), hops, h in zip(members.tolist(), r["hop_seq"], r["hops"]):
        path = [x] + [int(v) for v in hops[:h]]
        for a, b in zip(path, path[1:]):
            assert parent[(g, a)] == b
        assert parent[(g, path[-1])] == path[-1]
        seen |= {(g, v) for v in path}
    assert seen == set(parent)


def test_one_group_of_all_1000_nodes(engine: KbrEngine):
    """Every node subscribes to one group: the widest child list (107 here) is wider than a wave, the tree 3 deep."""
    net = W.population(1000, 14)
    M = _load(engine, net.ids, net.xy)
    gk = key_words(to_int(net.ids[77]) - 5).reshape(1, 5)
    members = np.stack([np.zeros(1000, np.uint32), np.arange(1000, dtype=np.uint32)], axis=1)
    ref = RS.ScribeModel.records(M.closure(gk, members))
    widest = np.bincount(ref["parent"][ref["parent"] != ref["node"]]).max()
    assert (int(widest), int(ref["depth"].max())) == (107, 3)
    state, rec = _check_forest(engine, M, gk, members)
    out, _ = _check_multicast(engine, M, state, gk, [0, 0], [5, 77], [0, 1], payload=1000)
    assert out["receivers"].tolist() == [1000, 1000] and out["forwarded"].tolist() == [999, 999]


def test_device_pointers_match_host_pointers(engine: KbrEngine):
    import torch
    from oversim_amd import SCRIBE_DELIVERY_DTYPE, SCRIBE_MSG_DTYPE
    ids, xy, gk, members, _ = scenario(200)
    _load(engine, ids, xy)
    nodes, edges, rooted = engine.scribe_build(gk, members[:, 0], members[:, 1])
    forest = engine.scribe_export()
    mg, ms, known = messages(200, members)
    out0, d0 = engine.scribe_multicast(mg, ms, known)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    t_gk, t_mg, t_mn = up(gk), up(members[:, 0]), up(members[:, 1])
    t_pg, t_ps, t_pf = up(mg), up(ms), up(known)
    t_out = torch.zeros(len(mg) * SCRIBE_MSG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    t_d = torch.zeros(max(len(d0), 1) * SCRIBE_DELIVERY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert engine.scribe_build_device(t_gk.data_ptr(), len(gk), t_mg.data_ptr(), t_mn.data_ptr(), len(members), nodes,
                                          s.cuda_stream) == (nodes, edges, rooted)
        assert engine.scribe_export().tobytes() == forest.tobytes()
        cnt = engine.scribe_multicast_device(t_pg.data_ptr(), t_ps.data_ptr(), t_pf.data_ptr(), len(mg), 100,
                                             t_out.data_ptr(), t_d.data_ptr(), len(d0), s.cuda_stream)
        s.synchronize()
        assert cnt == len(d0)
        assert t_out.cpu().numpy().view(SCRIBE_MSG_DTYPE).tobytes() == out0.tobytes()
        d = t_d.cpu().numpy().view(SCRIBE_DELIVERY_DTYPE)[:cnt]
        assert d[np.lexsort((d["node"], d["msg"]))].tobytes() == d0.tobytes()
        # out-of-range memberships and messages in device memory are found on the device; forest and results stay
        for col, bad_ptr in ((0, t_mn), (1, t_mg)):
            bad = members[:, col].copy()
            bad[1] = 99 if col == 0 else 200
            t_bad = up(bad)
            args = (t_bad.data_ptr(), t_mn.data_ptr()) if col == 0 else (t_mg.data_ptr(), t_bad.data_ptr())
            with pytest.raises(KbrError, match="EINVAL: .*out of range"):
                engine.scribe_build_device(t_gk.data_ptr(), len(gk), *args, len(members), nodes, s.cuda_stream)
        for arr, val, which in ((mg, 99, 0), (ms, 200, 1)):
            bad = arr.copy()
            bad[0] = val
            t_bad = up(bad)
            ptrs = (t_bad.data_ptr(), t_ps.data_ptr()) if which == 0 else (t_pg.data_ptr(), t_bad.data_ptr())
            with pytest.raises(KbrError, match="EINVAL: .*out of range"):
                engine.scribe_multicast_device(*ptrs, t_pf.data_ptr(), len(mg), 100, t_out.data_ptr(), None, 0, s.cuda_stream)
    assert engine.scribe_export().tobytes() == forest.tobytes()
    out1, d1 = engine.scribe_multicast(mg, ms, known)
    assert out1.tobytes() == out0.tobytes() and d1.tobytes() == d0.tobytes()


def test_capacity_one_short_leaves_the_forest(engine: KbrEngine):
    ids, xy, gk, members, _ = scenario(200)
    mg, ms, known = messages(200, members)
    M = _load(engine, ids, xy)
    with pytest.raises(KbrError, match="ESTATE: no Scribe forest"):
        engine.scribe_multicast(mg, ms, known)
    nodes, _, _ = engine.scribe_build(gk, members[:, 0], members[:, 1])
    assert engine.scribe_build(gk, members[:, 0], members[:, 1], capacity=nodes)[0] == nodes
    before = engine.scribe_export()
    out0, d0 = engine.scribe_multicast(mg, ms, known)
    half = members[: len(members) // 2]
    need = len(RS.ScribeModel.records(M.closure(gk, half)))
    for cap in (need - 1, 1, 0):
        with pytest.raises(KbrError, match="ENOMEM: .*capacity"):
            engine.scribe_build(gk, half[:, 0], half[:, 1], capacity=cap)
        assert engine.scribe_export().tolist() == before.tolist()
    out1, d1 = engine.scribe_multicast(mg, ms, known)
    assert out1.tobytes() == out0.tobytes() and d1.tobytes() == d0.tobytes()
    with pytest.raises(KbrError, match="EINVAL"):
        engine.scribe_build(gk, [9], [5])
    assert engine.scribe_export().tolist() == before.tolist()
    # a forest is published on under the hopCountMax its joins were routed under
    engine.set_params(Params.pastry().replace(hopCountMax=1))
    with pytest.raises(KbrError, match="ESTATE: .*built under another"):
        engine.scribe_multicast(mg, ms, known)
    engine.set_params(Params.pastry())
    assert engine.scribe_multicast(mg, ms, known)[0].tobytes() == out0.tobytes()
    engine.scribe_clear()
    with pytest.raises(KbrError, match="ESTATE"):
        engine.scribe_export()


def test_refusals_leave_the_context_usable(engine: KbrEngine):
    ids, xy, gk, members, _ = scenario(200)
    mg, ms, known = messages(200, members)
    _load(engine, ids, xy)
    keys, src = gk[members[:16, 0]], members[:16, 1]
    base = engine.pastry_lookup(keys, src)
    engine.scribe_build(gk, members[:, 0], members[:, 1])
    forest, out0 = engine.scribe_export(), engine.scribe_multicast(mg, ms, known)

    def refused(match):
        for call in (lambda: engine.scribe_build(gk, members[:, 0], members[:, 1]), lambda: engine.scribe_multicast(mg, ms, known, deliveries=False),
                     # inherited refusals come before the tier's own: a membership or a message out of range
                     lambda: engine.scribe_build(gk, [len(gk)], [5]), lambda: engine.scribe_multicast([len(gk)], [0], [0], deliveries=False)):
            with pytest.raises(KbrError, match="ENOTSUP: .*" + match):
                call()

    for kw, match in ((dict(routingType=0), "iterative"), (dict(routingType=2), "full-recursive"),
                      (dict(routingType=4), "source-routing"), (dict(numSiblings=2), "numSiblings = 1"),
                      (dict(recNumRedundantNodes=9), "recNumRedundantNodes 1..8")):
        engine.set_params(Params.pastry().replace(**kw))
        refused(match)
        engine.set_params(Params.pastry())
        assert engine.scribe_export().tobytes() == forest.tobytes()
        assert np.array_equal(engine.pastry_lookup(keys, src)["latency_ns"], base["latency_ns"])
    out1 = engine.scribe_multicast(mg, ms, known)
    assert out1[0].tobytes() == out0[0].tobytes() and out1[1].tobytes() == out0[1].tobytes()
    # routeMsgAcks, the default, by name; a load drops the forest as it always has
    engine.pastry_load(ids, xy, PastryParams.default())
    refused("routeMsgAcks")
    # explicit tables, even the rule's own
    engine.pastry_load(ids, xy, _pp())
    leaf, tab = engine.pastry_export()
    engine.pastry_load_tables(ids, xy, leaf, tab, _pp())
    refused("explicit tables")
    assert np.array_equal(engine.pastry_lookup(keys, src)["latency_ns"], base["latency_ns"])
    engine.pastry_load(ids, xy, _pp())
    engine.scribe_build(gk, members[:, 0], members[:, 1])
    assert engine.scribe_export().tobytes() == forest.tobytes()
    # Broose stays refused
    with KbrEngine(0) as br:
        br.set_params(Params.broose())
        br.broose_load(ids, xy)
        with pytest.raises(KbrError, match="ENOTSUP: Scribe is implemented for Chord rings and Pastry"):
            br.scribe_build(gk, members[:, 0], members[:, 1])


def test_matches_golden_fixture(engine: KbrEngine):
    g = np.load(GOLD / "scribe_pastry_n1000.npz")
    for c, (rnd, rnr) in enumerate(g["cases"]):
        engine.set_params(Params.pastry().replace(simtimeRound=int(rnd), recNumRedundantNodes=int(rnr)))
        engine.pastry_load(g["ids"], g["xy"], _pp())
        engine.scribe_build(g["group_keys"], g["members"][:, 0], g["members"][:, 1])
        assert engine.scribe_export().tolist() == g[f"forest_{c}"].tolist()
        out, deliv = engine.scribe_multicast(g["msg_group"], g["msg_src"], g["msg_known"], int(g["payload"]))
        assert np.array([[int(out[f][m]) for f in RS.MSG_FIELDS] for m in range(len(out))]).tolist() == g[f"out_{c}"].tolist()
        assert deliv.tolist() == g[f"deliveries_{c}"].tolist()


@pytest.fixture(scope="module")
def net14():
    """2^14 nodes, 64 groups x 256 members, and the model's forest and publishes, computed once and left unchanged."""
    n = 1 << 14
    net = W.population(n, 14)
    rng = np.random.default_rng(14)
    gk = np.stack([key_words(int.from_bytes(rng.bytes(20), "little")) for _ in range(64)])
    members = np.stack([np.repeat(np.arange(64, dtype=np.uint32), 256),
                        np.concatenate([rng.choice(n, 256, replace=False) for _ in range(64)]).astype(np.uint32)], axis=1)
    M = RSP.ScribePastryModel(net.ids, net.xy)
    state = M.closure(gk, members)
    mg = np.arange(64, dtype=np.uint32)
    ms = rng.integers(0, n, 64).astype(np.uint32)
    known = (np.arange(64) % 2).astype(np.uint8)
    return net, gk, members, RS.ScribeModel.records(state), (mg, ms, known), M.multicast(state, gk, mg, ms, known, 100)


def test_matches_model_n16384(engine: KbrEngine, net14):
    net, gk, members, ref, (mg, ms, known), (routs, rdeliv) = net14
    engine.set_params(Params.pastry())
    engine.pastry_load(net.ids, net.xy, _pp())
    nodes, edges, rooted = engine.scribe_build(gk, members[:, 0], members[:, 1])
    assert engine.scribe_export().tolist() == ref.tolist()
    assert (nodes, rooted) == (len(ref), 64) and edges == nodes - 64
    out, deliv = engine.scribe_multicast(mg, ms, known, 100)
    assert RS.msg_mismatches(out, routs) == []
    assert deliv.tolist() == rdeliv.tolist()
    assert np.all(out["receivers"] == 256)


def test_a_chord_context_is_unchanged_by_a_pastry_one(engine: KbrEngine):
    """One library, two contexts (a context keeps its overlay): the Chord forest and publishes before a Pastry
    context builds and publishes beside it, after it, and built again -- identical bytes."""
    ids, xy, gk, members, _ = scenario(200)
    mg, ms, known = messages(200, members)
    engine.set_params(Params.chord().replace(routingType=1))
    engine.chord_load(ids, xy)

    def chord(build):
        if build:
            engine.scribe_build(gk, members[:, 0], members[:, 1])
        out, d = engine.scribe_multicast(mg, ms, known)
        return engine.scribe_export().tobytes(), out.tobytes(), d.tobytes()

    first = chord(True)
    with KbrEngine(0) as pe:
        M = _load(pe, ids, xy)
        state, rec = _check_forest(pe, M, gk, members)
        _check_multicast(pe, M, state, gk, mg, ms, known)
        assert rec.tobytes() != first[0]
        assert chord(False) == first
    assert chord(False) == first and chord(True) == first
