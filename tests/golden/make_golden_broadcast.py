"""Generate tests/golden/chord_bcast_n1000.npz: Chord overlay broadcasts on a 1000-node ring.

Provenance as tests/golden/make_golden.py: the reference cannot be built here, so the vectors come
from the event-ordered replay in tests/refmodel_broadcast.py (tables from the oracle).  They freeze
the restated semantics of BroadcastTestApp::rpcBroadcastRequest over Chord::forwardBroadcast:
4 initiators; ttl 100 and 3; query sizes 0 and 37 B; measureAuthBlock off and on.
Run: python tests/golden/make_golden_broadcast.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

from oversim_amd import workload as W  # noqa: E402
from refmodel_broadcast import STAT_FIELDS, BroadcastReplay  # noqa: E402

N, SEED = 1000, 77
INITIATORS = np.array([0, 311, 640, 999], dtype=np.uint32)
CASES = [(100, 0, 0), (100, 37, 1), (3, 0, 1), (3, 37, 0)]      # (ttl, query_bytes, measureAuthBlock)
SD_FIELDS = ("count", "mean", "stddev", "min", "max")


def main():
    net = W.population(N, SEED)
    out = dict(ids=net.ids, xy=net.xy, initiators=INITIATORS, cases=np.array(CASES, dtype=np.int32),
               simtime_round=np.int32(1), seed=np.int64(SEED))
    for c, (ttl, qb, auth) in enumerate(CASES):
        rp = BroadcastReplay(net.ids, net.xy, simtimeRound=1, measureAuthBlock=bool(auth))
        rec, stats, rx = rp.run_batch(INITIATORS, ttl, qb)
        assert all(s["duplicated"] == 0 for s in stats) and rx.max() == 1
        out[f"records_{c}"] = rec
        out[f"stats_{c}"] = np.array([[s[f] for f in STAT_FIELDS] for s in stats], dtype=np.int64)
        out[f"hop_count_{c}"] = np.array([[s["hop_count"][f] for f in SD_FIELDS] for s in stats], dtype=np.float64)
        print((ttl, qb, auth), "reached", [int((r["arrival_ns"] >= 0).sum()) for r in rec],
              "last", [s["last_arrival_ns"] for s in stats])
    np.savez_compressed(HERE / "chord_bcast_n1000.npz", **out)


if __name__ == "__main__":
    main()
