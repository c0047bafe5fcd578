"""Writes tests/golden/pastry_iter_n1000.npz from the model (tests/refmodel_pastry_iter.py): the iterative lookups of
the network, keys and sources of pastry_n1000.npz (which holds those inputs; this file holds records only) --
LookupCalls with num_siblings 1 and 8 and the one-way route, each under both simtime rounding rules.

    python tests/golden/make_golden_pastry_iter.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import refmodel_pastry as RP  # noqa: E402
import refmodel_pastry_iter as RI  # noqa: E402

NONE = 0xFFFFFFFF


def main():
    base = np.load(HERE / "pastry_n1000.npz")
    m = RP.PastryNet(base["ids"], base["xy"])
    keys, src = base["keys"], base["src"]
    data = {}

    def both(fn):
        m.rnd = True
        r = fn()
        m.rnd = False
        t = fn()
        return r, t

    def record(tag, r, t, fields):
        assert (r["status"] == 0).mean() >= 0.99, "fewer than 99 % of the lookups succeed"
        H = max(int(r["hops"].max()), 1)
        for f in fields:
            assert np.array_equal(r[f], t[f])
            data[f"{tag}_{f}"] = r[f]
        data[f"{tag}_latency_ns"] = r["latency_ns"]
        data[f"{tag}_latency_ns_trunc"] = t["latency_ns"]
        data[f"{tag}_hop_seq"] = r["hop_seq"][:, :H]
        assert np.all(r["hop_seq"][:, H:] == NONE)

    for ns in (1, 8):
        r, t = both(lambda: RI.lookups(m, keys, src, ns))
        record(f"l{ns}", r, t, ("status", "hops", "num_siblings", "rpcs", "siblings"))
    r, t = both(lambda: RI.routes(m, keys, src))
    record("rt", r, t, ("responsible", "hops", "status", "one_way_hops"))
    out = HERE / "pastry_iter_n1000.npz"
    np.savez_compressed(out, **data)
    print("wrote", out, out.stat().st_size, "bytes (pastry_n1000.npz:", (HERE / "pastry_n1000.npz").stat().st_size, ")")


if __name__ == "__main__":
    main()
