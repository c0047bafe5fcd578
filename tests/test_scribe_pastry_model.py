"""Scribe on Pastry without a GPU: the event simulation of tests/refmodel_scribe_pastry.py -- with the first hop's
own sendToKey restated in full -- does not depend on the order and times of the joins and equals the closed form
"closure of the memberships under the source-step pick"; the premise that makes the closed form exact on rule-built
tables, asserted node by node; publishes as events equal their closed form; the golden fixture reproduces."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

import refmodel_pastry as RP
import refmodel_scribe as RS
import refmodel_scribe_pastry as RSP
from oversim_amd import workload as W
from refmodel import to_int
from scribe_cases import messages, scenario

GOLD = Path(__file__).resolve().parent / "golden"
SIZES = [2, 3, 9, 17, 40, 200]
SHAPES = [(4, 16), (1, 4), (2, 8)]


def _same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert (a[k]["parent"], a[k]["subscribed"], sorted(a[k]["children"])) == \
               (b[k]["parent"], b[k]["subscribed"], sorted(b[k]["children"])), k


def _model(ids, xy, b, L, **kw):
    return RSP.ScribePastryModel(ids, xy, bitsPerDigit=b, numberOfLeaves=L, **kw)


@pytest.mark.parametrize("b,L", SHAPES)
@pytest.mark.parametrize("n", SIZES)
def test_joins_in_any_order_give_the_closed_form(n, b, L):
    ids, xy, gk, members, root1 = scenario(n)
    rng = np.random.default_rng(n)
    for hcm in (0, 1, 2, 50):
        for rnr in (1, 3):
            M = _model(ids, xy, b, L, hopCountMax=hcm, recNumRedundantNodes=rnr)
            closed = M.closure(gk, members)
            for trial in range(3):
                order = rng.permutation(len(members))
                # all at once, spread over seconds, and in bursts that overlap the join round trips
                times = [np.zeros(len(members), np.int64), rng.integers(0, 5_000_000_000, len(members)),
                         rng.integers(0, 200_000, len(members))][trial]
                log = {}
                _same_state(M.simulate_joins(gk, members[order], times.tolist(), log), closed)
                assert log == dict(src_drop=0, hop_drop=0, pick_differs=0), (hcm, rnr, log)
            rec = RS.ScribeModel.records(closed)
            assert not np.any(rec["group"] == 2)
            if hcm == 0:
                assert np.all(rec["parent"] == RS.NONE)
            elif hcm == 1:
                assert rec["depth"].max() <= 1
            else:
                # the sibling for group 1's key is no member, has absorbed a join and joined through itself
                own1 = M.net.owner(to_int(gk[1]))
                r1 = rec[(rec["group"] == 1) & (rec["parent"] == rec["node"])]
                assert len(r1) == 1 and int(r1["node"][0]) in own1 and np.all(rec["parent"] != RS.NONE)
                assert np.count_nonzero(rec["flags"] & RS.ROOT) == 3
    # hopCountMax >= 2 cuts no join
    a = RS.ScribeModel.records(_model(ids, xy, b, L, hopCountMax=2).closure(gk, members))
    assert np.array_equal(a, RS.ScribeModel.records(_model(ids, xy, b, L).closure(gk, members)))


@pytest.mark.parametrize("b,L", SHAPES)
@pytest.mark.parametrize("n", SIZES)
def test_no_first_hop_refuses_a_join_on_rule_built_tables(n, b, L):
    """The premise of the closed form (and of k_scribe_level_pastry): at every node and for group keys, random keys
    and node ids, the source step picks a node; a first hop that is not the sibling forwards the sender's join, and
    to the node its own source step picks; exactly one node per key picks itself."""
    ids, xy, gk, _, _ = scenario(n)
    rng = np.random.default_rng(1000 + n)
    keys = [to_int(k) for k in gk] + [to_int(k) for k in W.random_keys(6, rng)]
    keys += [to_int(ids[i]) for i in rng.choice(n, min(n, 6), replace=False)]
    for rnr in (1, 3):
        M = _model(ids, xy, b, L, recNumRedundantNodes=rnr)
        for k in keys:
            selfs = 0
            for x in range(n):
                p, st = M.step(x, k, None, x)
                assert p is not None and st == RP.OK, ("source", n, b, L, rnr, x, hex(k))
                selfs += p == x
                if p != x and not M.responsible(p, k):
                    q, st = M.step(p, k, x, x)
                    assert q is not None and q == M.step(p, k, None, p)[0], ("first hop", n, b, L, rnr, x, p, hex(k))
            assert selfs == 1, (n, b, L, rnr, hex(k), selfs)


@pytest.mark.parametrize("b,L", SHAPES)
@pytest.mark.parametrize("n", [3, 9, 17, 200])
def test_publish_events_equal_the_closed_form(n, b, L):
    ids, xy, gk, members, _ = scenario(n)
    for rnd in (1, 0):
        M = _model(ids, xy, b, L, simtimeRound=rnd)
        state = M.closure(gk, members)
        mg, ms, known = messages(n, members)
        ev, evd = M.multicast(state, gk, mg, ms, known, payload=100, events=True)
        cf, cfd = M.multicast(state, gk, mg, ms, known, payload=100)
        assert ev == cf
        assert np.array_equal(evd, cfd)
        st = np.array([o["status"] for o in cf])
        assert np.all(st[mg == 2] == RS.WRONG_ROOT) and np.all(st[mg != 2] == RS.OK)
        assert all(o["receivers"] == 0 and o["response_ns"] >= 0 for o, g in zip(cf, mg) if g == 2)
        assert any(o["publish_hops"] > 1 for o in cf) or n < 200


def test_golden_fixture_reproduces():
    g = np.load(GOLD / "scribe_pastry_n1000.npz")
    for c, (rnd, rnr) in enumerate(g["cases"]):
        M = RSP.ScribePastryModel(g["ids"], g["xy"], simtimeRound=int(rnd), recNumRedundantNodes=int(rnr))
        state = M.closure(g["group_keys"], g["members"])
        assert np.array_equal(RS.ScribeModel.records(state), g[f"forest_{c}"])
        outs, deliv = M.multicast(state, g["group_keys"], g["msg_group"], g["msg_src"], g["msg_known"], int(g["payload"]))
        assert np.array_equal(np.array([[o[f] for f in RS.MSG_FIELDS] for o in outs], np.int64), g[f"out_{c}"])
        assert np.array_equal(deliv, g[f"deliveries_{c}"])


def test_header_marks_the_addition():
    text = (Path(__file__).resolve().parent.parent / "include" / "ovs_kbr.h").read_text()
    assert "#define OVS_HAS_SCRIBE_PASTRY 1" in text and "#define OVS_ABI_VERSION 12" in text
