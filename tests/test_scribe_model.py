"""Scribe without a GPU: the event simulation of tests/refmodel_scribe.py does not depend on the order and
times of the joins and equals its closed form, the golden fixture reproduces, the header's symbols and
layouts match the Python mirrors."""
from __future__ import annotations

import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import refmodel_scribe as RS
from scribe_cases import messages, scenario

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"


def _same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert (a[k]["parent"], a[k]["subscribed"], sorted(a[k]["children"])) == \
               (b[k]["parent"], b[k]["subscribed"], sorted(b[k]["children"])), k


@pytest.mark.parametrize("rt", [1, 0], ids=["semi-recursive", "iterative"])
@pytest.mark.parametrize("n", [2, 3, 9, 200])
def test_joins_in_any_order_give_the_closed_form(n, rt):
    ids, xy, gk, members, root1 = scenario(n)
    M = RS.ScribeModel(ids, xy, routingType=rt)
    closed = M.closure(gk, members)
    rng = np.random.default_rng(n)
    for trial in range(3):
        order = rng.permutation(len(members))
        # all at once, spread over seconds, and in bursts that overlap the join round trips
        times = [np.zeros(len(members), np.int64), rng.integers(0, 5_000_000_000, len(members)),
                 rng.integers(0, 200_000, len(members))][trial]
        _same_state(M.simulate_joins(gk, members[order], times.tolist()), closed)
    rec = RS.ScribeModel.records(closed)
    # the responsible node of group 1 is no member, has absorbed a join and joined through itself
    r1 = rec[(rec["group"] == 1) & (rec["node"] == root1)]
    assert len(r1) == 1 and r1["parent"][0] == root1 and r1["flags"][0] == RS.ROOT | RS.FORWARDER
    assert not np.any(rec["group"] == 2)
    if rt == 0:
        assert rec["depth"].max() <= 1


@pytest.mark.parametrize("rt", [1, 0], ids=["semi-recursive", "iterative"])
@pytest.mark.parametrize("n", [3, 9, 200])
def test_publish_events_equal_the_closed_form(n, rt):
    ids, xy, gk, members, _ = scenario(n)
    for rnd in (1, 0):
        M = RS.ScribeModel(ids, xy, routingType=rt, simtimeRound=rnd)
        state = M.closure(gk, members)
        mg, ms, known = messages(n, members)
        ev, evd = M.multicast(state, gk, mg, ms, known, payload=100, events=True)
        cf, cfd = M.multicast(state, gk, mg, ms, known, payload=100)
        assert ev == cf
        assert np.array_equal(evd, cfd)
        st = np.array([o["status"] for o in cf])
        assert np.all(st[mg == 2] == RS.WRONG_ROOT) and np.all(st[mg != 2] == RS.OK)
        assert all(o["receivers"] == 0 and o["response_ns"] >= 0 for o, g in zip(cf, mg) if g == 2)


def test_a_small_hop_limit_cuts_joins():
    ids, xy, gk, members, _ = scenario(200)
    it = RS.ScribeModel(ids, xy, routingType=0, hopCountMax=2)
    rec = RS.ScribeModel.records(it.closure(gk, members))
    cut = rec[rec["parent"] == RS.NONE]
    assert 0 < len(cut) < len(rec) and np.all(cut["flags"] == RS.SUBSCRIBER)
    _same_state(it.simulate_joins(gk, members), it.closure(gk, members))
    # a semi-recursive join arrives at its first hop with hop count 1: a limit of 2 cuts nothing ...
    a = RS.ScribeModel.records(RS.ScribeModel(ids, xy, routingType=1, hopCountMax=2).closure(gk, members))
    b = RS.ScribeModel.records(RS.ScribeModel(ids, xy, routingType=1).closure(gk, members))
    assert np.array_equal(a, b)
    # ... and a limit of 1 leaves only the joins whose first hop is the responsible node (and its own)
    one = RS.ScribeModel(ids, xy, routingType=1, hopCountMax=1)
    r1 = RS.ScribeModel.records(one.closure(gk, members))
    _same_state(one.simulate_joins(gk, members), one.closure(gk, members))
    cut1 = r1[r1["parent"] == RS.NONE]
    assert 0 < len(cut1) < len(r1) and np.all(cut1["flags"] == RS.SUBSCRIBER) and r1["depth"].max() <= 1
    full = {(int(g), int(x)): int(p) for g, x, p in zip(b["group"], b["node"], b["parent"])}
    for g, x, p in zip(r1["group"], r1["node"], r1["parent"]):
        fp = full[(int(g), int(x))]
        assert p == (fp if full[(int(g), fp)] == fp else RS.NONE)
    z = RS.ScribeModel(ids, xy, routingType=1, hopCountMax=0)
    rz = RS.ScribeModel.records(z.closure(gk, members))
    assert np.all(rz["parent"] == RS.NONE)
    _same_state(z.simulate_joins(gk, members), z.closure(gk, members))


def test_golden_fixture_reproduces():
    g = np.load(GOLD / "scribe_chord_n200.npz")
    for c, (rt, rnd) in enumerate(g["cases"]):
        M = RS.ScribeModel(g["ids"], g["xy"], routingType=int(rt), simtimeRound=int(rnd))
        state = M.closure(g["group_keys"], g["members"])
        assert np.array_equal(RS.ScribeModel.records(state), g[f"forest_{c}"])
        outs, deliv = M.multicast(state, g["group_keys"], g["msg_group"], g["msg_src"], g["msg_known"], int(g["payload"]))
        assert np.array_equal(np.array([[o[f] for f in RS.MSG_FIELDS] for o in outs], np.int64), g[f"out_{c}"])
        assert np.array_equal(deliv, g[f"deliveries_{c}"])


def test_scribe_struct_layout_and_exports(tmp_path):
    import oversim_amd
    from oversim_amd import kbr
    exe = tmp_path / "abi_layout_scribe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "abi_layout_scribe.c"), "-o", str(exe)], check=True)
    lay = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert lay["abi"] == 12
    assert lay["status"] == [RS.OK, RS.WRONG_ROOT, RS.ROUTE_FAILED] == sorted(kbr.SCRIBE_STATUS)
    assert lay["flags"] == [kbr.SCRIBE_SUBSCRIBER, kbr.SCRIBE_ROOT, kbr.SCRIBE_FORWARDER] == [RS.SUBSCRIBER, RS.ROOT, RS.FORWARDER]
    for name, dts in (("ovs_scribe_node", (kbr.SCRIBE_NODE_DTYPE, RS.NODE_DTYPE)),
                      ("ovs_scribe_msg_out", (kbr.SCRIBE_MSG_DTYPE,)),
                      ("ovs_scribe_delivery", (kbr.SCRIBE_DELIVERY_DTYPE, RS.DELIVERY_DTYPE))):
        for dt in dts:
            assert dt.itemsize == lay[name]["size"], name
            assert {f: dt.fields[f][1] for f in dt.names} == lay[name]["fields"], name
    L = oversim_amd.lib()
    for sym in ("ovs_scribe_build", "ovs_scribe_clear", "ovs_scribe_count", "ovs_scribe_export", "ovs_scribe_multicast_batch"):
        assert hasattr(L, sym), sym
    assert L.ovs_abi_version() == 12


def test_scribe_params_from_ini():
    from oversim_amd import ScribeParams
    ini = "[General]\n**.tier*.almTest.messageLength = 100\n[Config Scribe]\n**.almTest.messageLength = 256  # bytes\n" \
          "[Config Other]\n**.almTest.messageLength = 7\n"
    assert ScribeParams.from_ini(ini).messageLength == 100
    assert ScribeParams.from_ini(ini, "Scribe").messageLength == 256
    assert ScribeParams.from_ini("").messageLength == 100
