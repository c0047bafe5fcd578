"""Replica-team DHTs without a GPU: the team keys, the two anchors of the event-heap model
(tests/refmodel_dht_teams.py), the coupling its low-datarate configuration exercises, the .ini binder, the
parameter refusals, the golden fixture and the sanitizer build of the host pieces."""
from __future__ import annotations

import hashlib
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dht_teams_cases as K
import refmodel
import refmodel_dht as D
import refmodel_dht_teams as TM
from oversim_amd import DhtParams, DhtTeamParams, KbrError, lib

ROOT = Path(__file__).resolve().parent.parent
M160 = 1 << 160

# [Config ChordBroadcast] of the reference's simulations/omnetpp.ini (lines 87-105)
CHORD_BROADCAST = """
[Config ChordBroadcast]
description = Chord (SimpleUnderlayNetwork, blind-search)
**.measurementTime = 1000s
**.transitionTime = 100s
**.overlayType = "oversim.overlay.chord.ChordModules"
**.churnGeneratorTypes = "oversim.common.LifetimeChurn"
**.lifetimeMean = ${200s, 400s, 800s, 1600s, 3200s, 6400s}
**.targetOverlayTerminalNum = 1000
**.debugOutput = false
**.numTiers = 2
**.tier1Type = "oversim.applications.dht.SymmetricDHTModules"
**.tier1.dht.numReplica = 8
**.tier1.dht.numReplicaTeams = 4
**.tier2Type = "oversim.tier2.broadcasttestapp.BroadcastTestAppModules"
**.tier2.bcastTestApp.ttl = 100
**.tier2.bcastTestApp.itemsPerNode = 2
*.globalObserver.numGlobalFunctions = 1
*.globalObserver.globalFunctions[0].functionType = "oversim.tier2.broadcasttestapp.GlobalBroadcast"
*.globalObserver.globalFunctions[0].function.testInterval = 5s
"""


# ---------------------------------------------------------------- team keys
@pytest.mark.parametrize("T", range(1, 9))
def test_symmetric_offset(T):
    assert TM.offset(T) == (2**160 - 1) // T == DhtTeamParams.offset(T)


def test_key_plus_offset_wraps():
    k = M160 - 5
    assert TM.team_keys_int(k, TM.SYMMETRIC, 2) == [k, (k + (M160 - 1) // 2) % M160]
    assert TM.team_keys_int(k, TM.SYMMETRIC, 2)[1] < k
    assert np.array_equal(TM.team_keys(TM.words(k)[None], TM.SYMMETRIC, 2)[0, 1], TM.words((k + (M160 - 1) // 2) % M160))


def test_sha1_known_answers_and_first_step():
    # OverlayKey::test() (OverlayKey.cc:822-827): SHA-1 of the empty string and of "Hello World"
    def sha(b):
        return int.from_bytes(hashlib.sha1(b).digest(), "big")
    assert format(sha(b""), "040x") == "da39a3ee5e6b4b0d3255bfef95601890afd80709"
    assert format(sha(b"Hello World"), "040x") == "0a4d55a8d778e5022fab701977c5d840bbc486d0"
    for k in (0, 1, 0xABC, 1 << 100, M160 - 1, sha(b"Hello World")):
        text = format(k, "040x")
        assert len(text) == 40 and text == text.lower()
        assert TM.next_key(k, TM.REPEATED_HASHING, 2) == sha(text.encode())
    assert TM.next_key(0, TM.REPEATED_HASHING, 2) == sha(b"0" * 40)
    chain = TM.team_keys_int(5, TM.REPEATED_HASHING, 4)
    assert all(chain[j + 1] == sha(format(chain[j], "040x").encode()) for j in range(3))


# ---------------------------------------------------------------- the anchors
@pytest.mark.parametrize("n", [9, 1000])
def test_anchor_one_team_equals_the_plain_model(n):
    K.anchor_one_team(n)


@pytest.mark.parametrize("n,mode,T", [(1000, TM.SYMMETRIC, 4), (1000, TM.REPEATED_HASHING, 2), (9, TM.SYMMETRIC, 8)])
def test_anchor_no_coupling(n, mode, T):
    K.anchor_no_coupling(n, mode, T)


def test_coupling_is_exercised_by_the_low_datarate_configuration():
    m = 512
    b = K.batches(1000, m, 9)
    low = K.replay(K.model(1000, TM.SYMMETRIC, 4, **K.LOW), b)
    tk = TM.team_keys(b[0], TM.SYMMETRIC, 4)
    alone = TM.TeamDhtModel(K.chord_ring(1000), TM.SYMMETRIC, 1, True, 2, **K.LOW)
    differ = np.zeros(m, bool)
    for j in range(4):                                            # the uncoupled reading: every team on its own
        one = alone.put_batch(np.ascontiguousarray(tk[:, j]), b[1], b[2])[0]
        differ |= one["latency_ns"] != low[0][1][:, j]["latency_ns"]
    team = low[0][1]
    mixed = (team["outcome"] != D.SUCCESS).any(1) & (team["outcome"] == D.SUCCESS).any(1)
    print("operations that differ from the uncoupled reading:", int(differ.sum()), "of", m, "; mixed outcomes:", int(mixed.sum()))
    assert differ.sum() >= m // 2
    assert mixed.sum() >= 1
    assert (team["outcome"] != D.LOOKUP_FAILED).mean() > 0.5      # most lookups still finish
    first_is_failure = low[0][0]["outcome"][mixed] != D.SUCCESS
    assert first_is_failure.any() and (~first_is_failure).any()   # the first-response rule decides both ways


def test_zero_delay_ties_on_two_nodes_go_to_the_heap_order():
    b = K.batches(2, 64, 3)
    out, team, win = K.replay(K.model(2, TM.SYMMETRIC, 8), b)[0]       # one replica per team: the source itself for some
    tie = (team["latency_ns"] == team["latency_ns"].min(1)[:, None]).sum(1) > 1
    assert tie.any()
    first = np.argmax(team["latency_ns"] == team["latency_ns"].min(1)[:, None], axis=1)
    assert np.array_equal(win[tie], first[tie])                   # equal times: the team scheduled first


# ---------------------------------------------------------------- the binder and the refusals
def test_chord_broadcast_binds():
    tp = DhtTeamParams.from_ini(CHORD_BROADCAST, "ChordBroadcast")
    dp, _ = DhtParams.from_ini(CHORD_BROADCAST, "ChordBroadcast")
    assert (tp.mode, tp.numReplicaTeams, dp.numReplica) == (TM.SYMMETRIC, 4, 8)
    tp.check(dp)
    rh = CHORD_BROADCAST.replace("SymmetricDHTModules", "RepeatedHashingDHTModules")
    assert DhtTeamParams.from_ini(rh, "ChordBroadcast").mode == TM.REPEATED_HASHING
    plain = DhtTeamParams.from_ini(CHORD_BROADCAST.replace("SymmetricDHTModules", "DHTModules"), "ChordBroadcast")
    assert plain.numReplicaTeams == 1
    with pytest.raises(KbrError, match="ENOTSUP"):
        DhtTeamParams.from_ini(CHORD_BROADCAST.replace("dht.SymmetricDHTModules", "kbrtestapp.KBRTestAppModules"), "ChordBroadcast")
    assert DhtTeamParams.from_ini("[General]\n").numReplicaTeams == 1


@pytest.mark.parametrize("R,T,mode,status", [(8, 3, 0, "EINVAL"), (8, 0, 0, "ENOTSUP"), (9, 9, 0, "ENOTSUP"), (16, 1, 0, "ENOTSUP"),
                                             (8, 4, 2, "ENOTSUP"), (0, 2, 0, "ENOTSUP"), (16, 2, 0, "ENOTSUP"), (16, 4, 0, "ENOTSUP"),
                                             (16, 8, 0, "ENOTSUP"), (24, 8, 0, "ENOTSUP")])
def test_parameter_refusals(R, T, mode, status):
    with pytest.raises(KbrError, match=status):
        DhtTeamParams(mode, T).check(DhtParams.default().replace(numReplica=R))
    if status == "EINVAL":
        with pytest.raises(ValueError):
            TM.check_params(R, T)


def test_entry_points_are_exported():
    L = lib()
    for name in ("ovs_dht_team_keys", "ovs_dht_team_put_batch", "ovs_dht_team_get_batch", "ovs_dhttest_team_stats_batch",
                 "ovs_dht_team_params_default", "ovs_dht_team_params_from_ini", "ovs_dht_team_params_from_ini_file"):
        assert hasattr(L, name), name
    assert "#define OVS_HAS_DHT_TEAMS 1" in (ROOT / "include" / "ovs_kbr.h").read_text()


# ---------------------------------------------------------------- statistics, golden fixture, sanitizers
def test_team_statistics_with_one_team_are_the_plain_statistics():
    b = K.batches(9, 64, 4)
    (po, pt, _), (go, gt, _) = K.replay(K.model(9, TM.SYMMETRIC, 1, R=4), b)[:2]
    ex = np.zeros(64, dtype=D.EXPECT_DTYPE)
    ex["token"], ex["endtime_ns"], ex["known"] = b[2]["token"], 10**12, 1
    assert TM.team_stats(9, po, pt, b[1], go, gt, b[3], b[1], ex, 5.0) == D.dhttest_stats(9, po, b[1], go, b[3], b[1], ex, 5.0)
    (po, pt, _), (go, gt, _) = K.replay(K.model(9, TM.SYMMETRIC, 4), b)[:2]
    st = TM.team_stats(9, po, pt, b[1], go, gt, b[3], b[1], ex, 5.0)
    assert st["put_hop_count"] == 4 * 64 and st["normal_messages"] == int(pt["messages"].sum()) + int(gt["messages"].sum())


def test_golden_fixture_is_what_the_model_gives():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_dht_teams_golden", K.GOLD / "make_dht_teams_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want, g = mod.build(), np.load(K.GOLD / "dht_teams_n1000.npz")
    assert sorted(want) == sorted(g.files)
    for name in want:
        assert np.array_equal(np.asarray(want[name]), g[name]), name
    assert (K.GOLD / "dht_teams_n1000.npz").stat().st_size < 1 << 20


def test_host_pieces_under_sanitizers(tmp_path):
    """tests/dht_teams_driver.cpp: the offset division, the parameter checks and the .ini binder additions as a
    stand-alone program built with -fsanitize=address,undefined."""
    exe = tmp_path / "dht_teams_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "dht_teams_driver.cpp"),
                    str(ROOT / "oversim_amd" / "csrc" / "ovs_ini.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
