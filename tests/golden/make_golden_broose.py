"""Writes tests/golden/broose_n1000.npz from the model (tests/refmodel_broose.py): a 1 000-node Broose network at
the default parameters -- the inputs, the buckets of three sample nodes, findNode answers and route records -- and
tests/golden/broose_runs_n160.npz, the same for the 160-node ring of tests/broose_rings.py whose runs of ids
differ in their low 40 bits only (model built through BrooseBucket::add).

    python tests/golden/make_golden_broose.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

from oversim_amd import workload as W  # noqa: E402
from oversim_amd.kbr import BROOSE_EXT_DTYPE, key_from_int  # noqa: E402
import broose_cases as BC  # noqa: E402
import broose_rings as BR  # noqa: E402
import refmodel_broose as RB  # noqa: E402

NONE = 0xFFFFFFFF


def main():
    net = W.population(1000, 61)
    m = RB.BrooseNet(net.ids, net.xy)
    rng = np.random.default_rng(62)
    sample = np.array([0, 417, 999], dtype=np.uint32)
    rows = np.full((3, 6, 56), NONE, dtype=np.uint32)
    for j, v in enumerate(sample):
        for r, row in enumerate(m.rows(int(v))):
            rows[j, r, :len(row)] = row
    calls = [c for c in BC.find_node_calls(m, 600, 63) if c[4] != "broken"][:512]
    fn_ext = np.array([BC.ext_record(c[2]) for c in calls], dtype=BROOSE_EXT_DTYPE)
    fn_ext_out = np.array([BC.ext_record(c[6]) for c in calls], dtype=BROOSE_EXT_DTYPE)
    nq = 1024
    keys = W.random_keys(nq, rng)
    src = rng.integers(0, 1000, nq).astype(np.uint32)
    right = rng.integers(0, 2, nq).astype(np.uint8)
    want = BC.model_routes(m, keys, src, right)
    H = max(max(len(s) for s in want["hop_seq"]), 1)
    hop = np.full((nq, H), NONE, dtype=np.uint32)
    for i, s in enumerate(want["hop_seq"]):
        hop[i, :len(s)] = s
    np.savez_compressed(
        HERE / "broose_n1000.npz", ids=net.ids, xy=net.xy, sample_nodes=sample, sample_rows=rows,
        fn_node=np.array([c[0] for c in calls], dtype=np.uint32),
        fn_keys=np.array([key_from_int(c[1]) for c in calls], dtype=np.uint32),
        fn_right=np.array([c[3] for c in calls], dtype=np.uint8), fn_ext=fn_ext, fn_ext_out=fn_ext_out,
        fn_next=np.array([c[5][0] for c in calls], dtype=np.uint32),
        fn_sib=np.array([c[4] == "sibling" for c in calls], dtype=np.uint8),
        keys=keys, src=src, right=right, responsible=(want["responsible"] & 0xFFFFFFFF).astype(np.uint32),
        hops=want["hops"].astype(np.uint16), status=want["status"].astype(np.uint8),
        one_way_hops=want["one_way_hops"].astype(np.uint8), latency_ns=want["latency_ns"], hop_seq=hop)
    print("wrote", HERE / "broose_n1000.npz", (HERE / "broose_n1000.npz").stat().st_size, "bytes")


def runs():
    name = "lb40"
    net, members, feed = BR.ring(name)
    m = BR.model(name)
    sample = np.array([members[0][0], feed[3], members[2][5]], dtype=np.uint32)      # run members and a feeder
    rows = np.full((3, 6, 56), NONE, dtype=np.uint32)
    for j, v in enumerate(sample):
        for r, row in enumerate(m.rows(int(v))):
            rows[j, r, :len(row)] = row
    direct = BR.direct_calls(name, m, 64)
    calls = BC.find_node_calls(m, len(direct) + 300, 65, direct=direct, key_pool=BR.key_pool(name, m, 66),
                               node_pool=[i for run in members for i in run])
    keys, src, right = BR.batch(name)
    want = BC.model_routes(m, keys, src, right)
    H = max(max(len(s) for s in want["hop_seq"]), 1)
    hop = np.full((len(keys), H), NONE, dtype=np.uint32)
    for i, s in enumerate(want["hop_seq"]):
        hop[i, :len(s)] = s
    path = HERE / "broose_runs_n160.npz"
    np.savez_compressed(
        path, ids=net.ids, xy=net.xy, sample_nodes=sample, sample_rows=rows,
        fn_node=np.array([c[0] for c in calls], dtype=np.uint32),
        fn_keys=np.array([key_from_int(c[1]) for c in calls], dtype=np.uint32),
        fn_right=np.array([c[3] for c in calls], dtype=np.uint8),
        fn_ext=np.array([BC.ext_record(c[2]) for c in calls], dtype=BROOSE_EXT_DTYPE),
        fn_ext_out=np.array([BC.ext_record(c[6]) for c in calls], dtype=BROOSE_EXT_DTYPE),
        fn_next=np.array([c[5][0] if c[5] else NONE for c in calls], dtype=np.uint32),
        fn_sib=np.array([c[4] == "sibling" for c in calls], dtype=np.uint8),
        fn_status=np.array([c[4] == "broken" for c in calls], dtype=np.uint8),
        keys=keys, src=src, right=right, responsible=(want["responsible"] & 0xFFFFFFFF).astype(np.uint32),
        hops=want["hops"].astype(np.uint16), status=want["status"].astype(np.uint8),
        one_way_hops=want["one_way_hops"].astype(np.uint8), latency_ns=want["latency_ns"],
        rpcs=want["rpcs"].astype(np.uint32), hop_seq=hop)
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
    runs()
