"""Pastry on the GPU on the id families of tests/pastry_cases.py -- ids equal above w[0], a ladder of one-bit
neighbours, ids on both sides of zero -- against the models, bit for bit: the tables the device builds (33 to 160
rows), their round trip through explicit tables, BasePastry::findNode, semi-recursive routes, iterative LookupCalls
and routes, and one Scribe and one DHT case.  Random ids share about 16 bits; these reach the rows, digits, borrow
chains and table classes random ids never do (DESIGN.md §4 "Pastry rules").  Every vacuity condition is asserted
on the model's output, which tests/test_pastry_model.py checks on the CPU."""
from __future__ import annotations

import numpy as np
import pytest

import dht_pastry_cases as X
import pastry_cases as PC
import refmodel_pastry as RP
import refmodel_pastry_iter as RI
import test_gpu_dht_pastry as TD
import test_gpu_pastry_iter as TI
import test_gpu_scribe_pastry as TS
from oversim_amd import KbrEngine, Params, PastryParams
from scribe_cases import messages, scenario

pytestmark = pytest.mark.gpu
FN_CASES = [(1, 1), (1, 0), (3, 1), (8, 4), (16, 8)]           # (numRedundantNodes, numSiblings)
CASES = [pytest.param(name, b, L, id=f"{name}-b{b}-L{L}") for name in PC.FAMILIES for b, L in PC.SHAPES]
FORM_IDS = [f"opt{o}-reg{r}" for o, r in PC.FORMS]


def _pp(b, L, opt=0, reg=1):
    return PastryParams.default(routeMsgAcks=0, bitsPerDigit=b, numberOfLeaves=L, optimizeLookup=opt, useRegularNextHop=reg)


def _load(engine, name, b, L, opt=0, reg=1, params=None):
    """The family's converged tables on the engine and its model."""
    _, words, xy = PC.family(name, b)
    engine.set_params(params if params is not None else Params.pastry())
    engine.pastry_load(words, xy, _pp(b, L, opt, reg))
    return PC.model(name, b, L, opt, reg)


@pytest.mark.parametrize("name,b,L", CASES)
def test_tables_and_their_round_trip(engine: KbrEngine, name, b, L):
    m = _load(engine, name, b, L)
    _, words, xy = PC.family(name, b)
    leaf, tab = engine.pastry_export()
    wleaf, wtab = m.tables()
    rows = tab.shape[1]
    print(f"{name} b={b} L={L}: n={m.n} rows={rows}")
    assert rows == m.num_rows() == wtab.shape[1]
    if name == "low_word":
        assert rows > 128 // b and np.all(wtab[:, :128 // b] == PC.NONE)
    if name == "ladder":
        assert rows == 160 // b
    assert np.array_equal(leaf, wleaf)
    assert tab.shape == wtab.shape and np.array_equal(tab, wtab)
    keys, src = PC.probes(name, b)
    ideal = engine.pastry_lookup(keys, src, record_hops=True)
    engine.pastry_load_tables(words, xy, leaf, tab, _pp(b, L))
    l2, t2 = engine.pastry_export()
    assert np.array_equal(l2, leaf) and np.array_equal(t2, tab)
    again = engine.pastry_lookup(keys, src, record_hops=True)
    for f in ideal:
        assert np.array_equal(ideal[f], again[f]), f
    PC.assert_routes(again, PC.model_routes(name, b, L, 0, 1, 3), "explicit tables")


@pytest.mark.parametrize("opt,reg", PC.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name,b,L", CASES)
def test_find_node(engine: KbrEngine, name, b, L, opt, reg):
    m = _load(engine, name, b, L, opt, reg)
    keys, node = PC.probes(name, b)
    census = PC.find_node_sources(m, node, keys)
    print(f"{name} b={b} L={L} opt={opt} reg={reg}: findNode sources {census}")
    assert census["table"] > 0 and census["leaf"] > 0 and census["self"] > 0 and census["raised"] == 0
    assert (census["closer"] > 0) != (name == "ladder" and b == 1)
    ran = 0
    for nr, ns in FN_CASES:
        if nr > L or ns > L // 2:
            continue
        out, cnt, sib, st = engine.pastry_find_node(node, keys, nr, ns, max_out=L + 2)
        wout, wcnt, wsib, wst = PC.find_node_want(m, node, keys, nr, ns, L + 2)
        assert np.array_equal(st, wst), (nr, ns, np.flatnonzero(st != wst)[:5])
        assert np.array_equal(sib, wsib), (nr, ns, np.flatnonzero(sib != wsib)[:5])
        assert np.array_equal(cnt, wcnt), (nr, ns, np.flatnonzero(cnt != wcnt)[:5])
        bad = np.flatnonzero((out != wout).any(axis=1))
        assert len(bad) == 0, (nr, ns, bad[:5], out[bad[:2]], wout[bad[:2]])
        ran += 1
    assert ran == sum(nr <= L and ns <= L // 2 for nr, ns in FN_CASES) >= 2


@pytest.mark.parametrize("opt,reg", PC.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name,b,L", CASES)
def test_semi_recursive_routes(engine: KbrEngine, name, b, L, opt, reg):
    keys, src = PC.probes(name, b)
    for rnr in (1, 3):
        _load(engine, name, b, L, opt, reg, Params.pastry().replace(recNumRedundantNodes=rnr))
        want = PC.model_routes(name, b, L, opt, reg, rnr)
        census = PC.status_census(want)
        print(f"{name} b={b} L={L} opt={opt} reg={reg} rnr={rnr}: {len(keys)} routes, status {census}, "
              f"at most {int(want['hops'].max())} hops")
        if L == 2 and rnr == 3:
            assert census == {RP.BROKEN: len(keys)}              # numRedundantNodes > numberOfLeaves: findNode throws
        else:
            assert census.get(RP.OK, 0) >= 0.95 * len(keys)
        if (name, b, opt, rnr) == ("low_word", 1, 1, 1):
            assert census.get(RP.HOPMAX, 0) >= 1                 # routes that run into hopCountMax = 50
            assert (want["hop_seq"][want["status"] == RP.HOPMAX] != PC.NONE).all()
        PC.assert_routes(engine.pastry_lookup(keys, src, record_hops=True), want, f"rnr={rnr}")


@pytest.mark.parametrize("opt,reg", PC.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("b,L", [(3, 32), (4, 16)])
@pytest.mark.parametrize("name", ["low_word", "ladder"])
def test_iterative_lookups_and_routes(engine: KbrEngine, name, b, L, opt, reg):
    m = _load(engine, name, b, L, opt, reg, TI._iter_params())
    keys, src = PC.probes(name, b)
    for ns in (1, L // 2):
        want = TI._check(engine, m, keys, src, ns, f"{name} b={b} opt={opt} reg={reg}")
        print(f"{name} b={b} L={L} opt={opt} reg={reg} ns={ns}: LookupCall status {PC.status_census(want)}, "
              f"at most {int(want['hops'].max())} hops")
        assert (want["status"] == RI.OK).mean() >= 0.95
    TI._assert_routes(engine.pastry_iterative_lookup(keys, src, record_hops=True), RI.routes(m, keys, src), "route")


def test_scribe_on_low_word(engine: KbrEngine):
    """The build and one publish batch on the ids equal above w[0], bitsPerDigit = 4."""
    _, words, xy = PC.family("low_word", 4)
    n = len(words)
    ids, xy, gk, members, _ = scenario(n, ids=words, xy=xy)
    mg, ms, known = messages(n, members)
    M = TS._load(engine, ids, xy, 4, 16)
    state, rec = TS._check_forest(engine, M, gk, members)
    assert len(rec) > len(np.unique(members, axis=0)) and not np.any(rec["parent"] == PC.NONE)     # forwarders joined
    out, deliv = TS._check_multicast(engine, M, state, gk, mg, ms, known)
    assert np.all(out["status"][mg != 2] == TS.RS.OK) and len(deliv) > 0


def test_dht_on_low_word(engine: KbrEngine):
    """One put / get / overwrite / get round on the ids equal above w[0], bitsPerDigit = 4."""
    _, words, xy = PC.family("low_word", 4)
    n = len(words)
    bt = X.batches(TD.Network(ids=words, xy=xy), 128, 7 + n)
    ref = X.replay(X.model(n, 4, 16, ids=words, xy=xy), bt)
    c = X.census(ref)
    print("DHT on low_word:", c)
    assert c["put_ok"] >= 0.95 * (128 + 64) and c["get_value"] > 0
    TD.load(engine, n, 4, 16, ids=words, xy=xy)
    TD.check_sequence(engine, bt, ref, "low_word", TD.dparams())
