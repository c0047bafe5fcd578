"""The model of Pastry routes with per-hop acks (tests/refmodel_pastry_acks.py) against itself: the event replay with
a transmit queue per node equals the closed form the kernel evaluates, hand-worked routes, the RPC test's response
behind the responder's ack, and the ack timeout with a tie.  CPU only; the ABI layout and the host-side refusals of
the new calls are checked here too (tests/abi_layout_pastry_acks.c, tests/pastry_acks_host_driver.cpp)."""
from __future__ import annotations

import ctypes as C
import functools
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import refmodel_pastry as RP
import refmodel_pastry_acks as RA
import refmodel_rpc as RR
from oversim_amd import kbr, workload as W
from refmodel import coord_ns, simtime

ROOT = Path(__file__).resolve().parent.parent
RB = RR.route_bytes(100)                     # 186 B: the one-way message of testMsgSize = 100


@functools.lru_cache(maxsize=None)
def _pop(n, seed=81):
    return W.population(n, seed)


@functools.lru_cache(maxsize=None)
def _net(b, rnd, n=1000):
    p = _pop(n)
    return RP.PastryNet(p.ids, p.xy, b, 16, rnd=rnd)


@functools.lru_cache(maxsize=None)
def _batch(nq=512, seed=91, n=1000):
    rng = np.random.default_rng(seed)
    keys = W.random_keys(nq, rng)
    keys[::4] = _pop(n).ids[rng.integers(0, n, len(keys[::4]))]          # a quarter to node ids
    return keys, rng.integers(0, n, nq).astype(np.uint32)


@pytest.mark.parametrize("b", [2, 4])
@pytest.mark.parametrize("rnd", [True, False])
@pytest.mark.parametrize("auth", [False, True])
def test_closed_form_equals_the_event_replay(b, rnd, auth):
    """arrival = the ack-free route with the NextHopCall's length + forwards * T(ack bits / datarate)."""
    net = _net(b, rnd)
    keys, src = _batch()
    bw_ack = simtime(RA.ack_bytes(auth) * 8 / 10e6, rnd)
    fw = 0
    for k, s in zip(keys, src):
        r = RA.route(net, k, int(s), True, route_bytes=RB, auth=auth)
        plain = net.route(k, int(s), route_bytes=RA.call_bytes(RB))
        assert r["status"] == plain["status"] and r["hop_seq"] == plain["hop_seq"]
        assert r["forwards"] == max(len(r["hop_seq"]) - 1, 0)
        assert r["latency_ns"] == (plain["latency_ns"] + r["forwards"] * bw_ack if r["status"] == RP.OK else -1)
        assert r["acks"] == len(r["hop_seq"])
        fw += r["forwards"]
    assert fw > len(keys) // 2                # the batch forwards


def _find(net, hops):
    keys, src = _batch()
    for k, s in zip(keys, src):
        r = RA.route(net, k, int(s), True)
        if r["status"] == RP.OK and r["hops"] == hops:
            return k, int(s), r
    raise AssertionError(f"no {hops}-hop route in the batch")


def test_zero_hop_route_sends_no_ack():
    net = _net(4, True)
    r = RA.route(net, _pop(1000).ids[5], 5, True)                  # a node's own id from that node
    assert r["status"] == RP.OK and r["responsible"] == 5 and r["hops"] == 0
    assert (r["acks"], r["max_ack_rtt_ns"], r["timeout_hop"], r["latency_ns"], r["ack_rtt"]) == (0, -1, 0xFF, 0, [])


def test_one_hop_route_has_one_ack_and_no_queueing_term():
    net = _net(4, True)
    k, s, r = _find(net, 1)
    R = r["responsible"]
    bwc, bwa = simtime(RA.call_bytes(RB) * 8 / 10e6, True), simtime(RA.ack_bytes() * 8 / 10e6, True)
    cd = coord_ns(net.xy, s, R, True)
    assert r["latency_ns"] == 2 * bwc + cd
    assert r["ack_rtt"] == [2 * bwc + cd + 2 * bwa + cd] and r["acks"] == 1 and r["forwards"] == 0
    assert (bwc, bwa) == (174400, 48000)                          # 218 B and 60 B at 10 Mbit/s


def test_three_hop_route_by_calc_delay():
    """tx.finished = max(tx.finished, now) + bits / bandwidth at every sender, written out."""
    net = _net(4, True)
    k, s, r = _find(net, 3)
    h = [s] + r["hop_seq"]
    bwc, bwa = 174400, 48000
    cd = [coord_ns(net.xy, h[i], h[i + 1], True) for i in range(3)]
    a1 = (0 + bwc) + cd[0] + bwc                                  # the source's queue is idle
    ack1 = (a1 + bwa) + cd[0] + bwa                               # h1's queue: the ack first ...
    a2 = (a1 + bwa + bwc) + cd[1] + bwc                           # ... the forwarded call behind it
    ack2 = (a2 + bwa) + cd[1] + bwa
    a3 = (a2 + bwa + bwc) + cd[2] + bwc
    ack3 = (a3 + bwa) + cd[2] + bwa
    assert r["latency_ns"] == a3 and r["forwards"] == 2
    assert r["ack_rtt"] == [ack1 - 0, ack2 - a1, ack3 - a2]
    assert r["max_ack_rtt_ns"] == max(r["ack_rtt"]) and r["acks"] == 3


@pytest.mark.parametrize("auth", [False, True])
def test_rpc_response_waits_behind_the_ack(auth):
    net = _net(4, True)
    keys, src = _batch()
    keys, src = keys[:128].copy(), src[:128].copy()
    keys[:4] = _pop(1000).ids[src[:4]]                            # callers that are their own responder
    acked = RA.rpc_batch(net, keys, src, True, auth=auth)
    plain = RA.rpc_batch(net, keys, src, False, auth=auth)
    bwa = simtime(RA.ack_bytes(auth) * 8 / 10e6, True)
    longer = 2 * (simtime(RA.call_bytes(RB) * 8 / 10e6, True) - simtime(RB * 8 / 10e6, True))
    for f in ("responder", "call_hops", "status", "outcome", "hop_count"):
        assert np.array_equal(acked[f], plain[f]), f
    h = acked["call_hops"].astype(np.int64)
    assert (h[:4] == 0).all() and np.array_equal(acked["rtt_ns"][:4], plain["rtt_ns"][:4]) and (acked["rtt_ns"][:4] == 0).all()
    ok = h > 0
    assert ok.sum() > 100
    assert np.array_equal(acked["call_latency_ns"][ok], plain["call_latency_ns"][ok] + h[ok] * longer + (h[ok] - 1) * bwa)
    # the response: one ack's serialisation behind, on top of the longer call
    assert np.array_equal(acked["rtt_ns"][ok] - acked["call_latency_ns"][ok], plain["rtt_ns"][ok] - plain["call_latency_ns"][ok] + bwa)


def ack_timeout_case(b=4):
    """(net, keys, src, rpc_to, tie index): rpcUdpTimeout at the batch's median largest ack round trip, which is one
    route's exact round trip (the tie).  Shared with tests/test_gpu_pastry_acks.py."""
    net = _net(b, True)
    keys, src = _batch()
    rtt = np.array([RA.route(net, k, int(s), True)["max_ack_rtt_ns"] for k, s in zip(keys, src)])
    sent = np.sort(rtt[rtt >= 0])
    t_ns = int(sent[len(sent) // 2])                              # a quantile of the batch's own round trips
    assert sent[0] < t_ns < sent[-1]
    rpc_to = t_ns * 1e-9
    assert simtime(rpc_to, True) == t_ns
    return net, keys, src, rpc_to, int(np.flatnonzero(rtt == t_ns)[0])


def test_ack_timeout_flags_the_routes_that_reach_it():
    net, keys, src, rpc_to, tie = ack_timeout_case()
    T = simtime(rpc_to, True)
    flagged = 0
    for i, (k, s) in enumerate(zip(keys, src)):
        base = RA.route(net, k, int(s), True)
        r = RA.route(net, k, int(s), True, rpc_to=rpc_to)
        assert (r["timeout_hop"] != 0xFF) == (base["max_ack_rtt_ns"] >= T), i
        if r["timeout_hop"] != 0xFF:
            assert r["timeout_hop"] == next(j for j, x in enumerate(r["ack_rtt"]) if x >= T)
            flagged += 1
        for f in ("responsible", "hops", "status", "latency_ns", "hop_seq"):
            assert r[f] == base[f], (i, f)                        # the first copy is delivered all the same
    tied = RA.route(net, keys[tie], int(src[tie]), True, rpc_to=rpc_to)
    assert tied["max_ack_rtt_ns"] == T and tied["timeout_hop"] != 0xFF      # a tie is a timeout (BaseRpc.cc:191-211)
    assert 0 < flagged < len(keys)


# --- the ABI and the host-side refusals ------------------------------------------------------------------------
def test_ack_record_layout(tmp_path):
    """tests/abi_layout_pastry_acks.c, built with gcc -std=c99 against include/ovs_kbr.h alone, against the numpy
    mirror in oversim_amd/kbr.py."""
    exe = tmp_path / "abi_layout_pastry_acks"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "abi_layout_pastry_acks.c"), "-o", str(exe)], check=True)
    lay = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert lay["abi"] == 12 and lay["has_acks"] == 1 and lay["has_rpc"] == 1
    want = lay["ovs_pastry_ack_out"]
    dt = kbr.PASTRY_ACK_OUT_DTYPE
    assert dt.itemsize == want["size"] == 16
    assert list(dt.names) == list(want["fields"])
    for f, off in want["fields"].items():
        assert dt.fields[f][1] == off, f
    assert C.sizeof(kbr.PastryParams) == lay["ovs_pastry_params_size"] == 24


def test_host_driver_under_sanitizers(tmp_path):
    """tests/pastry_acks_host_driver.cpp: pastry_acked_refusal and the wire lengths as a stand-alone program built
    with -fsanitize=address,undefined."""
    exe = tmp_path / "pastry_acks_host_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "oversim_amd" / "csrc"),
                    str(ROOT / "tests" / "pastry_acks_host_driver.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("ok")
    lens = dict(line.split()[1:3] for line in r.stdout.splitlines() if line.startswith("len "))
    assert int(lens["call"]) == RA.call_bytes(RB) and int(lens["ack"]) == RA.ack_bytes() and int(lens["ack_auth"]) == RA.ack_bytes(True)
    assert int(lens["resp"]) == RR.response_bytes(100)
