"""Generate tests/golden/pastry_broadcast_n1000.npz: Pastry overlay broadcasts on a 1000-node network.

Provenance as tests/golden/make_golden.py: the reference cannot be built here, so the vectors come from the
event-ordered replay in tests/refmodel_pastry_broadcast.py over the rule's tables (tests/refmodel_pastry.py) at
the default shape (bitsPerDigit 4, numberOfLeaves 16).  They freeze the restated semantics of
BroadcastTestApp::rpcBroadcastRequest over Pastry::forwardBroadcast: 4 initiators; ttl 100 and 2; simtimeRound 1
and 0; an empty query.
Run: python tests/golden/make_golden_pastry_broadcast.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

from oversim_amd import workload as W  # noqa: E402
from refmodel_pastry import PastryNet  # noqa: E402
from refmodel_pastry_broadcast import STAT_FIELDS, PastryBroadcastReplay  # noqa: E402

N, SEED = 1000, 91
INITIATORS = np.array([0, 311, 640, 999], dtype=np.uint32)
CASES = [(100, 1), (2, 1), (100, 0), (2, 0)]      # (ttl, simtimeRound)
SD_FIELDS = ("count", "mean", "stddev", "min", "max")


def main():
    net = W.population(N, SEED)
    model = PastryNet(net.ids, net.xy)
    out = dict(ids=net.ids, xy=net.xy, initiators=INITIATORS, cases=np.array(CASES, dtype=np.int32), seed=np.int64(SEED))
    for c, (ttl, rnd) in enumerate(CASES):
        rp = PastryBroadcastReplay(model, simtimeRound=rnd)
        rec, stats, rx = rp.run_batch(INITIATORS, ttl)
        assert all(s["duplicated"] == 0 and s["extra"] == 0 for s in stats) and rx.max() == 1
        out[f"records_{c}"] = rec
        out[f"stats_{c}"] = np.array([[s[f] for f in STAT_FIELDS] for s in stats], dtype=np.int64)
        out[f"hop_count_{c}"] = np.array([[s["hop_count"][f] for f in SD_FIELDS] for s in stats], dtype=np.float64)
        print((ttl, rnd), "reached", [int((r["arrival_ns"] >= 0).sum()) for r in rec],
              "last", [s["last_arrival_ns"] for s in stats])
    np.savez_compressed(HERE / "pastry_broadcast_n1000.npz", **out)


if __name__ == "__main__":
    main()
