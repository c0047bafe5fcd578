"""ovs_pastry_broadcast_batch on the GPU against the event-ordered replay (tests/refmodel_pastry_broadcast.py)
and the golden fixture: every field of every record and every statistic bit-exact."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from oversim_amd import BCAST_NODE_DTYPE, BrooseParams, KbrEngine, KbrError, Params, PastryParams, key_from_int, workload as W
from oversim_amd.kbr import NONE
import refmodel_pastry as RP
from refmodel_pastry_broadcast import STAT_FIELDS, PastryBroadcastReplay, stats_equal

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
FIELDS = BCAST_NODE_DTYPE.names
LEAVES = {4: 16, 2: 8, 1: 4}
FORMS = pytest.mark.parametrize("wave_items", ["0", "1000000000"], ids=["lane-per-node", "wave-per-node"])


def _mismatches(rec, ref) -> dict:
    return {f: int(np.count_nonzero(rec[f] != ref[f])) for f in FIELDS if not np.array_equal(rec[f], ref[f])}


def _check(engine, replay, init, ttl, qb=0):
    rec, stats = engine.pastry_broadcast(init, ttl, qb)
    ref, rstats, rx = replay.run_batch(init, ttl, qb)
    assert rx.max() <= 1 and all(s["duplicated"] == 0 and s["extra"] == 0 for s in rstats)
    assert _mismatches(rec, ref) == {}
    for b in range(len(init)):
        assert stats_equal(stats[b], rstats[b]) == [], b
    return rec, stats


def _load(engine, ids, xy, b=4, model_nodes=None, acks=0, **kw):
    """The rule's tables on the engine and the replay over the model's."""
    p = Params.pastry().replace(**kw)
    engine.set_params(p)
    engine.pastry_load(ids, xy, PastryParams.default(routeMsgAcks=acks, bitsPerDigit=b, numberOfLeaves=LEAVES[b]))
    return PastryBroadcastReplay(RP.PastryNet(ids, xy, b, LEAVES[b], nodes=model_nodes), simtimeRound=p.simtimeRound,
                                 datarate=p.datarate, accessDelay=p.accessDelay, measureAuthBlock=bool(p.measureAuthBlock))


# --- n = 2^14 at the defaults: the levels pass the switch from a wave per node to a lane per node -------------

N14 = 1 << 14
INIT14 = np.array([0, 5000, 11111, N14 - 1], dtype=np.uint32)


@pytest.fixture(scope="module")
def net14():
    """The 2^14-node network and its replays (ttl 100 and 2), computed once and left unchanged.  The model builds
    a node's rows when the replay first reaches it; the broadcast needs no leaf sets."""
    net = W.population(N14, 14)
    rp = PastryBroadcastReplay(RP.PastryNet(net.ids, net.xy, nodes=[]), simtimeRound=Params.pastry().simtimeRound)
    return net, {ttl: rp.run_batch(INIT14, ttl) for ttl in (100, 2)}


@pytest.mark.parametrize("ttl", [100, 2])
def test_matches_replay_n16384(engine: KbrEngine, net14, ttl):
    net, refs = net14
    ref, rstats, rx = refs[ttl]
    assert rx.max() == 1 and all(s["duplicated"] == 0 and s["extra"] == 0 for s in rstats)
    engine.set_params(Params.pastry())
    engine.pastry_load(net.ids, net.xy, PastryParams.default())       # every default, routeMsgAcks = true among them
    rec, stats = engine.pastry_broadcast(INIT14, ttl)
    assert _mismatches(rec, ref) == {}
    for b in range(len(INIT14)):
        assert stats_equal(stats[b], rstats[b]) == [], b
    if ttl == 100:
        assert np.all(rec["arrival_ns"] >= 0) and rec["hops"].max() <= engine.pastry_export()[1].shape[1]
    else:
        assert 0 < np.count_nonzero(rec["arrival_ns"] >= 0) < rec.size and rec["hops"].max() == 2


def test_matches_golden_fixture(engine: KbrEngine):
    g = np.load(GOLD / "pastry_broadcast_n1000.npz")
    for c, (ttl, rnd) in enumerate(g["cases"]):
        engine.set_params(Params.pastry().replace(simtimeRound=int(rnd)))
        engine.pastry_load(g["ids"], g["xy"])
        rec, stats = engine.pastry_broadcast(g["initiators"], int(ttl))
        assert _mismatches(rec, g[f"records_{c}"]) == {}, c
        for b, s in enumerate(stats):
            assert [int(s[f]) for f in STAT_FIELDS] == g[f"stats_{c}"][b].tolist(), (c, b)
            assert [s["hop_count"][f] for f in ("count", "mean", "stddev", "min", "max")] == g[f"hop_count_{c}"][b].tolist()


# --- tiny, odd and deep networks, on both kernels ------------------------------------------------------------

@FORMS
@pytest.mark.parametrize("b", [1, 2, 4])
@pytest.mark.parametrize("n", [2, 3, 9, 17, 40])
def test_tiny_networks(engine: KbrEngine, monkeypatch, n, b, wave_items):
    """Fewer nodes than leaves (the leaf sets are replayed on the host), tables of one row, every initiator."""
    monkeypatch.setenv("OVS_BCAST_WAVE_ITEMS", wave_items)
    net = W.population(n, 81)
    rp = _load(engine, net.ids, net.xy, b)
    for ttl in (100, 1, 0):
        rec, _ = _check(engine, rp, np.arange(n, dtype=np.uint32), ttl)
        if ttl == 100:
            assert np.all(rec["arrival_ns"] >= 0)


@FORMS
@pytest.mark.parametrize("b", [1, 4])
def test_keys_that_differ_only_in_the_lowest_word(engine: KbrEngine, monkeypatch, b, wave_items):
    """64 keys equal above w[0]: 128 shared bits, so tables of up to 160 / b rows whose first 128 / b are empty,
    and items whose limit lies far down the table."""
    monkeypatch.setenv("OVS_BCAST_WAVE_ITEMS", wave_items)
    rng = np.random.default_rng(64)
    low = np.sort(rng.choice(1 << 32, 64, replace=False)).astype(np.uint32)
    ids = np.tile(key_from_int(0x1234567 << 130 | 0x89ABCDEF << 40), (64, 1))
    ids[:, 0] = low
    rp = _load(engine, ids, W.coordinates(64, 64), b)
    rows = engine.pastry_export()[1].shape[1]
    assert 128 // b < rows <= 160 // b
    rec, _ = _check(engine, rp, np.array([0, 17, 63], dtype=np.uint32), 100)
    assert np.all(rec["arrival_ns"] >= 0) and rec["hops"].max() <= rows - 128 // b
    _check(engine, rp, np.array([5, 62], dtype=np.uint32), 2)


@FORMS
def test_one_usable_column_a_row(engine: KbrEngine, monkeypatch, wave_items):
    """bitsPerDigit = 1: a row holds the owner's own digit and one other, so a node sends one request a row."""
    monkeypatch.setenv("OVS_BCAST_WAVE_ITEMS", wave_items)
    net = W.population(1000, 81)
    rp = _load(engine, net.ids, net.xy, 1)
    rec, _ = _check(engine, rp, np.array([0, 499, 999], dtype=np.uint32), 100)
    assert np.all(rec["arrival_ns"] >= 0)
    _check(engine, rp, np.array([7], dtype=np.uint32), 4)


@FORMS
def test_explicit_tables_with_emptied_slots(engine: KbrEngine, monkeypatch, wave_items):
    """The thinning of test_gpu_pastry's closer-node test: 30 % of the exported slots emptied and loaded through
    pastry_load_tables.  Accepted; the nodes behind emptied slots stay unreached, as in the replay."""
    monkeypatch.setenv("OVS_BCAST_WAVE_ITEMS", wave_items)
    net = W.population(1000, 81)
    engine.set_params(Params.pastry())
    engine.pastry_load(net.ids, net.xy, PastryParams.default(routeMsgAcks=0))
    leaf, tab = engine.pastry_export()
    thin = tab.copy()
    thin[np.random.default_rng(85).random(tab.shape) < 0.3] = NONE
    engine.pastry_load_tables(net.ids, net.xy, leaf, thin, PastryParams.default(routeMsgAcks=0))
    rp = PastryBroadcastReplay(RP.PastryNet(net.ids, net.xy, tables=(leaf, thin)))
    init = np.array([0, 333, 999], dtype=np.uint32)
    rec, stats = _check(engine, rp, init, 100)
    for b in range(len(init)):
        reached = int(np.count_nonzero(rec[b]["arrival_ns"] >= 0))
        assert 1 < reached < 1000 and stats[b]["actual"] == reached and stats[b]["expected"] == 1000
        assert np.all(rec[b]["parent"][rec[b]["arrival_ns"] < 0] == NONE)
    _check(engine, rp, init, 1)


@pytest.mark.parametrize("rnd", [0, 1])
def test_simtime_rounding_access_delay_auth_block_and_query(engine: KbrEngine, rnd):
    """routingType and routeMsgAcks do not enter (the requests go to nodes, over UDP): iterative routing with
    acks runs as semi-recursive routing without them does."""
    net = W.population(1000, 5)
    rp = _load(engine, net.ids, net.xy, 4, acks=rnd, simtimeRound=rnd, accessDelay=0.0123456789123, datarate=9.7e6,
               measureAuthBlock=rnd, routingType=rnd)
    _check(engine, rp, np.array([3, 998], dtype=np.uint32), 100, qb=37)


# --- pointer modes, stats only, properties at scale ---------------------------------------------------------

def test_device_pointers_and_stats_only(engine: KbrEngine):
    import torch
    net = W.population(5000, 8)
    engine.set_params(Params.pastry())
    engine.pastry_load(net.ids, net.xy)
    init = np.array([1, 4999, 2500], dtype=np.uint32)
    rec, stats = engine.pastry_broadcast(init, 100, 11)
    none, stats_only = engine.pastry_broadcast(init, 100, 11, nodes=False)
    assert none is None and stats_only == stats
    di = torch.from_numpy(init.view(np.int32)).cuda()
    dn = torch.empty(len(init) * 5000 * 16, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dstats = engine.pastry_broadcast_device(di.data_ptr(), len(init), 100, 11, dn.data_ptr(), s.cuda_stream)
    s.synchronize()
    drec = dn.cpu().numpy().view(BCAST_NODE_DTYPE).reshape(len(init), 5000)
    assert _mismatches(drec, rec) == {} and dstats == stats
    assert engine.pastry_broadcast_device(di.data_ptr(), len(init), 100, 11, None, s.cuda_stream) == stats
    # an initiator outside the network in device memory is found on the device and refused
    di[1] = 5000
    with pytest.raises(KbrError, match="initiator out of range"):
        engine.pastry_broadcast_device(di.data_ptr(), len(init), 100, 11, dn.data_ptr(), s.cuda_stream)
    again, stats2 = engine.pastry_broadcast(init, 100, 11)
    assert _mismatches(again, rec) == {} and stats2 == stats


def test_properties_n131072(engine: KbrEngine):
    """No replay at this size: every node reached once (one record each, one initiator), a parent earlier, one
    hop nearer and sharing at least hops - 1 digits with its child, ranks dense under each parent, statistics
    equal to a numpy reduction of the records."""
    n, nb = 1 << 17, 4
    net = W.population(n, 17)
    engine.set_params(Params.pastry())
    engine.pastry_load(net.ids, net.xy)
    init = np.random.default_rng(17).integers(0, n, nb).astype(np.uint32)
    rec, stats = engine.pastry_broadcast(init, 100)
    top = net.ids[:, 4].astype(np.int64)                      # the first 32 bits: 8 digits
    for b in range(nb):
        r = rec[b]
        assert np.all(r["arrival_ns"] >= 0)
        root = r["parent"] == NONE
        assert np.flatnonzero(root).tolist() == [int(init[b])] and r["arrival_ns"][init[b]] == 0
        kid = np.flatnonzero(~root)
        par = r["parent"][kid]
        assert np.all(r["arrival_ns"][par] < r["arrival_ns"][kid])
        assert np.all(r["hops"][kid] == r["hops"][par] + 1)
        # the request a child got came from row hops - 1 of its parent or a later one
        need = np.minimum(r["hops"][kid].astype(np.int64) - 1, 8)
        assert np.all((top[par] ^ top[kid]) >> (32 - 4 * need) == 0)
        pairs = par.astype(np.int64) * 1024 + r["rank"][kid]
        assert len(np.unique(pairs)) == len(pairs)
        cnt = np.bincount(par, minlength=n)
        most = np.zeros(n, np.int64)
        np.maximum.at(most, par, r["rank"][kid].astype(np.int64) + 1)
        assert np.array_equal(cnt, most)
        h = r["hops"].astype(np.int64)
        s = stats[b]
        assert (s["expected"], s["actual"], s["expired"], s["messages"]) == (n, n, 0, 2 * n - 1)
        assert s["bytes"] == (n - 1) * 60 + n * 34
        assert s["last_arrival_ns"] == r["arrival_ns"].max()
        hs, hq = int(h.sum()), int((h * h).sum())
        var = (float(hq) - float(hs) * float(hs) / float(n)) / float(n - 1)
        assert s["hop_count"] == dict(count=n, mean=float(hs) / float(n), stddev=float(np.sqrt(var)),
                                      min=float(h.min()), max=float(h.max()))


# --- refusals -------------------------------------------------------------------------------------------------

def test_refusals_leave_later_calls_unchanged(engine: KbrEngine):
    net = W.population(500, 31)
    engine.set_params(Params.pastry())
    engine.pastry_load(net.ids, net.xy)
    init = np.array([0, 499, 250], dtype=np.uint32)
    ok_rec, ok_stats = engine.pastry_broadcast(init, 100)

    def same():
        rec, stats = engine.pastry_broadcast(init, 100)
        assert _mismatches(rec, ok_rec) == {} and stats == ok_stats

    for bad in (500, 0xFFFFFFFF):
        with pytest.raises(KbrError, match="EINVAL: initiator out of range"):
            engine.pastry_broadcast(np.array([0, bad, 250], dtype=np.uint32), 100)
        same()
    for kw, msg in ((dict(ttl=-1), "ttl must be"), (dict(ttl=65536), "ttl must be"),
                    (dict(ttl=100, query_bytes=-1), "query_bytes must be")):
        with pytest.raises(KbrError, match="EINVAL: " + msg):
            engine.pastry_broadcast(init, **kw)
        same()
    # rows * 15 requests of 125 kB each would overrun one node's 1 MB transmit queue: drops are not modelled
    with pytest.raises(KbrError, match="ENOTSUP: .*sendQueueLength"):
        engine.pastry_broadcast(init, 100, query_bytes=1_000_000)
    same()
    rec, stats = engine.pastry_broadcast(init, 65535)                # the largest ttl is a valid call
    assert _mismatches(rec, ok_rec) == {} and stats == ok_stats
    # the Chord call keeps its answer on a Pastry context
    with pytest.raises(KbrError, match="ESTATE"):
        engine.chord_broadcast(init, 100)
    same()


def test_refused_on_other_overlays(engine: KbrEngine):
    """OVS_ESTATE on a context without a network and on Chord, Kademlia and Broose contexts, whose own calls
    still answer as before."""
    net = W.population(300, 33)
    keys = W.random_keys(64, np.random.default_rng(34))
    src = np.arange(64, dtype=np.uint32)

    def refused(eng):
        with pytest.raises(KbrError, match="ESTATE"):
            eng.pastry_broadcast([0], 100)

    engine.set_params(Params.chord())
    refused(engine)
    engine.chord_load(net.ids, net.xy)
    before = engine.chord_broadcast([0, 299], 100)
    refused(engine)
    after = engine.chord_broadcast([0, 299], 100)
    assert _mismatches(after[0], before[0]) == {} and after[1] == before[1]
    with KbrEngine(0) as kad:
        kad.set_params(Params.kademlia())
        kad.kad_load(net.ids, net.xy)
        before = kad.lookup(keys, src)
        refused(kad)
        assert np.array_equal(kad.lookup(keys, src)["latency_ns"], before["latency_ns"])
    with KbrEngine(0) as br:
        br.set_params(Params.broose())
        br.broose_load(net.ids, net.xy, BrooseParams.default())
        right, _ = br.broose_directions(keys, src)
        before = br.broose_lookup(keys, src, right)
        refused(br)
        assert np.array_equal(br.broose_lookup(keys, src, right)["latency_ns"], before["latency_ns"])
