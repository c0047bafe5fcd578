"""Inputs shared by the replica-team DHT tests (tests/test_dht_teams_model.py, tests/test_gpu_dht_teams.py and
tests/golden/make_dht_teams_golden.py): rings, operation batches, the model runs and their comparison."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np

import refmodel
import refmodel_dht as D
import refmodel_dht_teams as TM
from oversim_amd import Network, workload as W

GOLD = Path(__file__).resolve().parent / "golden"
SEC = 10**9

# The low-datarate configuration (coupling and timeouts): at 64 kbit/s a FindNodeCall takes 10.4 ms to
# serialise, so four teams' messages wait for one another in the source's queue, and an rpcUdpTimeout of
# 0.35 s lies inside the spread of the round-trip times while most lookups still finish.
LOW = dict(datarate=64e3, rpc_udp_timeout=0.35)


@functools.lru_cache(maxsize=None)
def ring(n):
    """n = 1000: the golden ring's identifiers and coordinates."""
    if n == 1000:
        g = np.load(GOLD / "chord_n1000_round.npz")
        return Network(np.ascontiguousarray(g["ids"]), np.ascontiguousarray(g["xy"]))
    return W.population(n, 0x5445 + n)


def chord_ring(n, rnd=1, sls=8):
    net = ring(n)
    return refmodel.ChordRing(net.ids, net.xy, sls, bool(rnd))


def batches(n, m, seed):
    """put, get, overwrite (every 5th a delete, vlen = 0), get after the first TTLs ran out.  Half the keys are
    node IDs; the first 16 operations share one key (conflicts within a batch)."""
    net = ring(n)
    rng = np.random.default_rng(seed)
    k1, s1 = W.lookups(net.ids, m // 2, seed, node_ids=True)
    k2, s2 = W.lookups(net.ids, m - m // 2, seed + 1, node_ids=False)
    keys, src = np.ascontiguousarray(np.concatenate([k1, k2])), np.ascontiguousarray(np.concatenate([s1, s2]))
    keys[:16] = keys[16]
    put = D.make_ops(m, t0_ns=rng.integers(0, 5 * SEC, m), token=np.arange(m) + 1, vlen=rng.integers(1, 200, m),
                     ttl=np.where(np.arange(m) % 2, 60, 0), kind=1 + np.arange(m) % 2, id=1 + np.arange(m) % 3)
    get1 = put.copy()
    get1["t0_ns"] = 20 * SEC + rng.integers(0, SEC, m)
    over = put.copy()
    over["t0_ns"] = 30 * SEC + rng.integers(0, SEC, m)
    over["token"] += 10**6
    over["vlen"] = np.where(np.arange(m) % 5 == 3, 0, rng.integers(1, 200, m))
    over["ttl"] = 0
    sel = np.arange(m) < m // 2                       # the second half is not overwritten: its odd entries expire
    get2 = put.copy()
    get2["t0_ns"] = 100 * SEC
    return keys, src, put, get1, over, sel, get2


def sequence(b):
    keys, src, put, get1, over, sel, get2 = b
    return [(True, keys, src, put), (False, keys, src, get1), (True, keys[sel], src[sel], over[sel]), (False, keys, src, get2)]


def replay(M, b):
    """[(out, team_out, winner)] of the four batches on model M."""
    res = [(M.put_batch if is_put else M.get_batch)(k, s, o) for is_put, k, s, o in sequence(b)]
    for r in res:
        for a in r:
            a.setflags(write=False)
    return res


def model(n, mode, T, rnd=1, R=8, G=4, ratio=0.5, hop_max=50, auth=False, **kw):
    return TM.TeamDhtModel(chord_ring(n, rnd), mode, T, bool(rnd), R, G, ratio, hop_max=hop_max, auth=auth, **kw)


def same(got, ref, fields, what):
    for f in fields:
        a, b = np.asarray(got[f]).astype(np.int64), np.asarray(ref[f]).astype(np.int64)
        assert a.shape == b.shape, (what, f, a.shape, b.shape)
        assert np.array_equal(a, b), (what, f, np.argwhere(a != b)[:5].tolist(), a[a != b][:5], b[a != b][:5])


def same_result(got, ref, is_put, what):
    """every field of out and team_out, and the winner index"""
    fields = D.PUT_FIELDS if is_put else D.GET_FIELDS
    same(got[0], ref[0], fields, (what, "out"))
    same(got[1], ref[1], fields, (what, "team_out"))
    assert np.array_equal(np.asarray(got[2]), ref[2]), (what, "winner")


# ---------------------------------------------------------------- the two anchors
def anchor_one_team(n, m=200, seed=31):
    """T = 1: the team model equals DhtModel fed by chord_measured_lookup, field by field, puts and gets."""
    b = batches(n, m, seed)
    ring_ = chord_ring(n)
    got = replay(model(n, TM.SYMMETRIC, 1, R=4), b)
    plain = D.DhtModel(ring_.xy, D.chord_measured_lookup(ring_, 4), True, 4, 4)
    for j, (is_put, k, s, o) in enumerate(sequence(b)):
        want = (plain.put_batch if is_put else plain.get_batch)(k, s, o)
        fields = D.PUT_FIELDS if is_put else D.GET_FIELDS
        same(got[j][0], want, fields, ("anchor 1", n, j))
        same(got[j][1][:, 0], want, fields, ("anchor 1 team", n, j))
        assert not got[j][2].any()
    assert plain.queue_measured > 0


def anchor_no_coupling(n, mode, T, m=120, seed=32):
    """At a datarate whose serialisation times all round to 0 ns, team j of every operation equals a single-team
    operation on key_j, and the operation's record is the earliest team's."""
    b = batches(n, m, seed)
    fast = dict(datarate=1e15)
    assert D.simtime(4000 * 8 / fast["datarate"], True) == 0
    got = replay(model(n, mode, T, **fast), b)
    tk = TM.team_keys(b[0], mode, T)
    singles = [TM.TeamDhtModel(chord_ring(n), TM.SYMMETRIC, 1, True, 8 // T, **fast) for _ in range(T)]
    for jb, (is_put, k, s, o) in enumerate(sequence(b)):
        idx = np.arange(len(b[1]))[b[5]] if len(s) != len(b[1]) else np.arange(len(s))
        fields = D.PUT_FIELDS if is_put else D.GET_FIELDS
        per_team = []
        for j in range(T):
            kj = np.ascontiguousarray(tk[idx, j])
            one = (singles[j].put_batch if is_put else singles[j].get_batch)(kj, s, o)[0]
            same(got[jb][1][:, j], one, fields, ("anchor 2", n, mode, T, jb, j))
            per_team.append(one)
        # the earliest team: a failed lookup ends when its last event fires, which its record does not hold,
        # so the comparison is made where every team's lookup succeeded
        lat = np.stack([p["latency_ns"] for p in per_team], axis=1)
        allok = (np.stack([p["outcome"] for p in per_team], axis=1) != D.LOOKUP_FAILED).all(1)
        first = lat.min(1)
        w = got[jb][2]
        assert allok.any()
        assert np.array_equal(lat[np.arange(len(w)), w][allok], first[allok]), ("anchor 2 winner", n, mode, T, jb)
        same(got[jb][0], got[jb][1][np.arange(len(w)), w], fields, ("anchor 2 out", jb))
