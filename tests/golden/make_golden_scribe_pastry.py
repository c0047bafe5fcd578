"""Writes tests/golden/scribe_pastry_n1000.npz from tests/refmodel_scribe_pastry.py: inputs, forests and publish
records of 1000 Pastry nodes (default tables) under (simtimeRound, recNumRedundantNodes) = (1, 3), (0, 3), (1, 1).
Data only.

    python tests/golden/make_golden_scribe_pastry.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parent.parent)]

import refmodel_scribe as RS  # noqa: E402
import refmodel_scribe_pastry as RSP  # noqa: E402
from scribe_cases import messages, scenario  # noqa: E402

CASES = [(1, 3), (0, 3), (1, 1)]
PAYLOAD = 100


def main():
    ids, xy, gk, members, _ = scenario(1000)
    mg, ms, known = messages(1000, members)
    out = dict(ids=ids, xy=xy, group_keys=gk, members=members, msg_group=mg, msg_src=ms, msg_known=known,
               payload=np.int32(PAYLOAD), cases=np.array(CASES, np.int32))
    for c, (rnd, rnr) in enumerate(CASES):
        M = RSP.ScribePastryModel(ids, xy, simtimeRound=rnd, recNumRedundantNodes=rnr)
        state = M.closure(gk, members)
        outs, deliv = M.multicast(state, gk, mg, ms, known, PAYLOAD)
        out[f"forest_{c}"] = RS.ScribeModel.records(state)
        out[f"out_{c}"] = np.array([[o[f] for f in RS.MSG_FIELDS] for o in outs], np.int64)
        out[f"deliveries_{c}"] = deliv
    np.savez_compressed(HERE / "scribe_pastry_n1000.npz", **out)


if __name__ == "__main__":
    main()
