"""Writes tests/golden/scribe_chord_n200.npz from tests/refmodel_scribe.py: inputs, forests and publish
records of a 200-node ring under (routingType, simtimeRound) = (1, 1), (0, 1), (1, 0).  Data only.

    python tests/golden/make_golden_scribe.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parent.parent)]

import refmodel_scribe as RS  # noqa: E402
from scribe_cases import messages, scenario  # noqa: E402

CASES = [(1, 1), (0, 1), (1, 0)]
PAYLOAD = 100


def main():
    ids, xy, gk, members, _ = scenario(200)
    mg, ms, known = messages(200, members)
    out = dict(ids=ids, xy=xy, group_keys=gk, members=members, msg_group=mg, msg_src=ms, msg_known=known,
               payload=np.int32(PAYLOAD), cases=np.array(CASES, np.int32))
    for c, (rt, rnd) in enumerate(CASES):
        M = RS.ScribeModel(ids, xy, routingType=rt, simtimeRound=rnd)
        state = M.closure(gk, members)
        outs, deliv = M.multicast(state, gk, mg, ms, known, PAYLOAD)
        out[f"forest_{c}"] = RS.ScribeModel.records(state)
        out[f"out_{c}"] = np.array([[o[f] for f in RS.MSG_FIELDS] for o in outs], np.int64)
        out[f"deliveries_{c}"] = deliv
    np.savez_compressed(HERE / "scribe_chord_n200.npz", **out)


if __name__ == "__main__":
    main()
