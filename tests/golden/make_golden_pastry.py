"""Writes tests/golden/pastry_n1000.npz from the model (tests/refmodel_pastry.py): a 1 000-node Pastry network at
the default parameters with converged tables -- the inputs, 2 000 semi-recursive routes (half to node ids, half to
random keys) for recNumRedundantNodes 1 and 3 under both simtime rounding rules, and findNode answers.

    python tests/golden/make_golden_pastry.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

from oversim_amd import workload as W  # noqa: E402
import refmodel_pastry as RP  # noqa: E402

NONE = 0xFFFFFFFF
FN_CASES = [(1, 1), (3, 1), (8, 4), (16, 8)]
FN_COLS = 17


def find_node_rows(m, node, keys, nr, ns):
    """findNode answers as arrays: nodes NONE padded to FN_COLS, count, sibling flag, status bits."""
    out = np.full((len(node), FN_COLS), NONE, dtype=np.uint32)
    cnt = np.zeros(len(node), dtype=np.uint8)
    sib = np.zeros(len(node), dtype=np.uint8)
    st = np.zeros(len(node), dtype=np.uint8)
    src = []
    for i, (v, k) in enumerate(zip(node, keys)):
        try:
            res, info = m.nodes[int(v)].find_node(RP.to_int(k), nr, ns)
        except RP.PastryError:
            st[i] = 2
            src.append("broken")
            continue
        out[i, :len(res)] = res
        cnt[i], sib[i], st[i] = len(res), info["sib"], 1 if info["err"] else 0
        src.append(info["source"])
    return out, cnt, sib, st, src


def main():
    net = W.population(1000, 71)
    m = RP.PastryNet(net.ids, net.xy)
    rng = np.random.default_rng(72)
    nq = 2000
    keys = W.random_keys(nq, rng)
    keys[:nq // 2] = net.ids[rng.integers(0, 1000, nq // 2)]
    src = rng.integers(0, 1000, nq).astype(np.uint32)
    data = dict(ids=net.ids, xy=net.xy, params=np.array([m.b, m.L, int(m.optimize), int(m.regular), 50], dtype=np.int32),
                keys=keys, src=src)
    for rnr in (1, 3):
        m.rnd = True
        r = RP.routes(m, keys, src, rec_num_redundant=rnr)
        m.rnd = False
        t = RP.routes(m, keys, src, rec_num_redundant=rnr)
        assert (r["status"] == 0).mean() >= 0.99, "fewer than 99 % of the routes are delivered"
        H = max(int(r["hops"].max()), 1)
        for f in ("responsible", "hops", "status", "one_way_hops"):
            assert np.array_equal(r[f], t[f])
            data[f"r{rnr}_{f}"] = r[f]
        data[f"r{rnr}_latency_ns"] = r["latency_ns"]
        data[f"r{rnr}_latency_ns_trunc"] = t["latency_ns"]
        data[f"r{rnr}_hop_seq"] = r["hop_seq"][:, :H]
        assert np.all(r["hop_seq"][:, H:] == NONE)
    # findNode calls chosen from a pool so that every next-hop source is there
    pool_nodes = rng.integers(0, 1000, 20000).astype(np.uint32)
    pool_keys = W.random_keys(20000, rng)
    pool_keys[::5] = net.ids[rng.integers(0, 1000, len(pool_keys[::5]))]
    _, _, _, _, srcs = find_node_rows(m, pool_nodes, pool_keys, 1, 1)
    pick, quota = [], dict(closer=64, leaf=128, self=64, table=256)
    for i, s in enumerate(srcs):
        if quota.get(s, 0) > 0:
            quota[s] -= 1
            pick.append(i)
    fn_node, fn_keys = pool_nodes[pick], pool_keys[pick]
    data.update(fn_node=fn_node, fn_keys=fn_keys)
    seen = set()
    for nr, ns in FN_CASES:
        out, cnt, sib, st, s = find_node_rows(m, fn_node, fn_keys, nr, ns)
        seen |= set(s)
        data[f"fn_{nr}_{ns}_nodes"], data[f"fn_{nr}_{ns}_count"] = out, cnt
        data[f"fn_{nr}_{ns}_sib"], data[f"fn_{nr}_{ns}_status"] = sib, st
    for need in ("leaf", "table", "closer"):
        assert need in seen, f"no findNode case takes its next hop from: {need}"
    np.savez_compressed(HERE / "pastry_n1000.npz", **data)
    print("wrote", HERE / "pastry_n1000.npz", (HERE / "pastry_n1000.npz").stat().st_size, "bytes; findNode sources",
          {k: s.count(k) for k in set(s)})


if __name__ == "__main__":
    main()
