"""Regenerates tests/golden/dht_pastry_n1000.npz from the model alone: the DHT replay (tests/refmodel_dht.py) fed by
the Pastry iterative LookupCall (tests/refmodel_pastry_iter.py) on a 1000-node network -- a put batch, a get batch,
an overwrite batch and a get batch after the first TTLs ran out, 600 operations each, once with the default
rpcUdpTimeout (d_*) and once with the short one of tests/dht_pastry_cases.py (s_*).
Run from the repository root: python tests/golden/make_golden_dht_pastry.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dht_pastry_cases as X  # noqa: E402


def main():
    net = X.population(1000)
    b, dflt, _ = X.reference(1000)
    b2, short, _ = X.reference(1000, tmo=X.SHORT_TMO)
    keys, src, put, get1, over, sel, get2 = b
    assert all(np.array_equal(u, v) for u, v in zip(b, b2))
    res = dict(ids=net.ids, xy=net.xy, keys=keys, src=src, put=put, get1=get1, over=over[sel], get2=get2,
               short_timeout=np.float64(X.SHORT_TMO))
    for tag, ref in (("d", dflt), ("s", short)):
        for name, r in zip(("put_out", "get1_out", "over_out", "get2_out"), ref):
            res[f"{tag}_{name}"] = r
    out = ROOT / "tests" / "golden" / "dht_pastry_n1000.npz"
    np.savez_compressed(out, **res)
    print({k: v.shape for k, v in res.items()}, out.stat().st_size, "bytes")
    print("default:", X.census(dflt), "short:", X.census(short))


if __name__ == "__main__":
    main()
