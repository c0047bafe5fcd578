"""What the nine loaders, the shard steps and the refresh calls refuse, with status and literal message, and
the state a refused load leaves: no network ("ESTATE: no network loaded" from ovs_route_batch), after which a
correct load of the same overlay routes as it does on a fresh context.  64 nodes."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from epichord_snap import SEC, make_queries, make_snapshot
from oversim_amd import KbrEngine, KbrError, Params, workload as W
from oversim_amd.kbr import BrooseParams, DEVICE_PTRS, _ptr

pytestmark = pytest.mark.gpu
N = 64
SORTED = "EINVAL: node ids must be sorted ascending and unique$"
NO_NET = "ovs_route_batch: ESTATE: no network loaded$"
LOADERS = ("chord", "chord_shard", "chord_tables", "kad", "kad_tables", "kad_csr", "koorde", "epichord", "broose",
           "broose_tables")


class Case:
    """One loader: its parameters, its arguments for a network, and eight lookups through the loaded network."""

    def __init__(self, name: str, inputs):
        self.name, self.inp = name, inputs
        self.overlay = {"chord": "Chord", "kad": "Kademlia", "koorde": "Koorde", "epichord": "EpiChord",
                        "broose": "Broose"}[name.split("_")[0]]
        self.params = {"Chord": Params.chord, "Kademlia": Params.kademlia, "Koorde": Params.koorde,
                       "EpiChord": Params.epichord, "Broose": Params.broose}[self.overlay]()
        if self.overlay == "EpiChord":
            snap = inputs["snap"]
            self.params = self.params.replace(successorListSize=snap["L"], cacheTTL=snap["cache_ttl_param"] / SEC)

    def load(self, e: KbrEngine, ids=None, n=None, flags=0):
        """the loader on `ids` (default: the network's) or on their first n"""
        net, i = self.inp["net"], self.inp
        ids = net.ids if ids is None else ids
        n = len(ids) if n is None else n
        ids, xy = np.ascontiguousarray(ids[:n]), np.ascontiguousarray(net.xy[:n])
        if self.name == "chord":
            e.chord_load(ids, xy)
        elif self.name == "chord_shard":
            e._chk(e._L.ovs_chord_load_shard(e._h, _ptr(ids), C.c_uint64(n), _ptr(xy), C.c_uint64(0), C.c_uint64(n),
                                             C.c_uint32(0)), "ovs_chord_load_shard")
            e.n = n
        elif self.name == "chord_tables":
            t = i["chord"]
            e._chk(e._L.ovs_chord_load_tables(e._h, _ptr(ids), n, _ptr(xy), _ptr(t["pred"]), _ptr(t["succ"]), _ptr(t["nsucc"]),
                                              _ptr(t["fingers"]), _ptr(t["deque"]), flags), "ovs_chord_load_tables")
            e.n = n
        elif self.name == "kad":
            e.kad_load(ids, xy)
        elif self.name == "kad_tables":
            sib, bc, bn = i["kad"]
            e._chk(e._L.ovs_kad_load_tables(e._h, _ptr(ids), n, _ptr(xy), _ptr(sib), _ptr(bc), _ptr(bn), 0), "ovs_kad_load_tables")
            e.n = n
        elif self.name == "kad_csr":
            sib, off, nodes = i.get("csr_bad_off") if flags == "bad_off" else i["csr"]
            e._chk(e._L.ovs_kad_load_tables_csr(e._h, _ptr(ids), n, _ptr(xy), _ptr(sib), _ptr(off), _ptr(nodes), 0),
                   "ovs_kad_load_tables_csr")
            e.n = n
        elif self.name == "koorde":
            e.koorde_load(ids, xy)
        elif self.name == "epichord":
            s = i["snap"]
            arrs = [np.ascontiguousarray(a) for a in (s["succ"], s["nsucc"], s["pred"], s["npred"], s["full"], s["cache_off"],
                                                      s["cache_node"], s["cache_last"], s["cache_ttl"])]
            e._chk(e._L.ovs_epichord_load(e._h, _ptr(ids), n, _ptr(xy), *[_ptr(a) for a in arrs], 0), "ovs_epichord_load")
            e.n = n
        elif self.name == "broose":
            e.broose_load(ids, xy)
        else:
            off, nodes = i["broose"]
            bp = BrooseParams.default()
            e._chk(e._L.ovs_broose_load_tables(e._h, C.byref(bp), _ptr(ids), n, _ptr(xy), _ptr(off), _ptr(nodes), 0),
                   "ovs_broose_load_tables")
            e.n = n

    def route(self, e: KbrEngine) -> bytes:
        net = self.inp["net"]
        keys, src = W.lookups(net.ids, 8, 3, node_ids=False)
        if self.overlay == "EpiChord":
            node, keys, src, now = make_queries(self.inp["snap"], 8, 3)
            return b"".join(np.ascontiguousarray(a).tobytes() for a in e.epichord_find_node(node, keys, src, now, 2))
        if self.overlay == "Broose":
            out = e.broose_lookup(keys, src, e.broose_directions(keys, src)[0])
        else:
            out = e.lookup(keys, src)
        return b"".join(out[f].tobytes() for f in sorted(out))


@pytest.fixture(scope="module")
def inputs():
    """the 64-node network and its tables in every loader's form, exported from converged loads"""
    net = W.population(N, 77)
    snap = make_snapshot(N, 77, list_size=4)
    net_epi = type(net)(ids=snap["ids"], xy=net.xy)
    i = {"net": net, "snap": snap, "net_epi": net_epi}
    n = np.arange(N)
    with KbrEngine(0, Params.chord()) as e:
        e.chord_load(net.ids, net.xy)
        i["chord"] = dict(pred=((n - 1) % N).astype(np.uint32), succ=((n[:, None] + 1 + np.arange(8)[None, :]) % N).astype(np.uint32),
                          nsucc=np.full(N, 8, np.uint8), fingers=np.ascontiguousarray(e.chord_fingers()),
                          deque=np.full(N, 160, np.uint8))
    with KbrEngine(0, Params.kademlia()) as e:
        e.kad_load(net.ids, net.xy)
        i["kad"] = tuple(np.ascontiguousarray(a) for a in e.kad_tables())
        sib, off, nodes = (np.ascontiguousarray(a) for a in e.kad_tables_csr())
        i["csr"] = (sib, off, nodes)
        bad = off.copy()
        bad[0] = 1
        i["csr_bad_off"] = (sib, bad, nodes)
    with KbrEngine(0, Params.broose()) as e:
        e.broose_load(net.ids, net.xy)
        off, nodes = e.broose_export()[:2]
        i["broose"] = (np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(nodes, np.uint32))
    return i


def _case(name, inputs) -> Case:
    c = Case(name, inputs)
    if c.overlay == "EpiChord":
        c.inp = dict(inputs, net=inputs["net_epi"])
    return c


def _refused(e: KbrEngine, match: str, call, *a, **kw):
    with pytest.raises(KbrError, match=match):
        call(*a, **kw)


def _no_network(e: KbrEngine, net):
    keys, src = W.lookups(net.ids, 8, 3)
    _refused(e, NO_NET, e.lookup, keys, src)


K17 = r"ENOTSUP: Kademlia k must be 1\.\.16 \(two 96 B bucket blocks\) and 5\*s <= 64$"
# a refusal of the loader's own that needs parameters no loaded context takes: (parameter, value, message)
BY_PARAMS = {
    "kad": ("k", 17, K17),
    "kad_tables": ("k", 17, K17),
    "kad_csr": ("k", 17, r"ENOTSUP: Kademlia k must be 1\.\.16 and 5\*s <= 64$"),
    "koorde": ("shiftingBits", 17, r"ENOTSUP: Koorde shiftingBits must be 1\.\.16 and deBruijnListSize 1\.\.255$"),
    "epichord": ("successorListSize", 17, r"ENOTSUP: EpiChord successorListSize must be 1\.\.16$"),
}


@pytest.mark.parametrize("name", LOADERS)
def test_a_refused_load_leaves_no_network(name, inputs):
    c = _case(name, inputs)
    net = c.inp["net"]
    with KbrEngine(0, c.params) as fresh:
        c.load(fresh)
        want = c.route(fresh)

    def reload(e):
        e.set_params(c.params)
        c.load(e)
        assert c.route(e) == want

    swapped = net.ids.copy()
    swapped[[5, 6]] = swapped[[6, 5]]
    twice = net.ids.copy()
    twice[6] = twice[5]
    one = {"koorde": "EINVAL: Koorde needs at least 2 nodes$", "epichord": "EINVAL: node count out of range$",
           "broose": "EINVAL: Broose needs at least 2 nodes$",
           "broose_tables": "EINVAL: node count out of range$"}.get(name, "EINVAL: need at least 2 nodes$")
    with KbrEngine(0) as e:
        reload(e)
        # the explicit Broose loader checks its tables before it drops anything: rows of other ids are out of
        # XOR order, and the network loaded before stays
        order = SORTED if name != "broose_tables" else \
            r"EINVAL: Broose tables: node \d+ row \d+: not in ascending XOR order to the bucket key$"
        for ids, n, match in ((swapped, None, order), (twice, None, order), (net.ids, 1, one)):
            _refused(e, match, c.load, e, ids, n)
            if name == "broose_tables":
                assert c.route(e) == want
            else:
                _no_network(e, net)
                reload(e)
        if name == "chord_tables":
            # refused before anything is dropped
            _refused(e, "ENOTSUP: explicit tables are taken from host memory$", c.load, e, flags=DEVICE_PTRS)
            assert c.route(e) == want
        if name == "kad_csr":
            _refused(e, r"EINVAL: bucket_off\[0\] must be 0$", c.load, e, flags="bad_off")
            _no_network(e, net)
            reload(e)
    if name in BY_PARAMS:
        field, value, match = BY_PARAMS[name]
        with KbrEngine(0, c.params.replace(**{field: value})) as e:
            _refused(e, match, c.load, e)
            _no_network(e, net)
            reload(e)
    # the wrong overlay in the parameters: refused, and the other overlay's network loaded before it is gone
    with KbrEngine(0) as e:
        if c.overlay == "Kademlia":
            e.set_params(Params.chord())
            e.chord_load(net.ids, net.xy)
        else:
            e.set_params(Params.kademlia())
            e.kad_load(net.ids, net.xy)
        assert len(e.lookup(*W.lookups(net.ids, 8, 3))["hops"]) == 8
        _refused(e, f"ESTATE: params.overlay is not {c.overlay}$", c.load, e)
        _no_network(e, net)
        reload(e)


def _u64(*v):
    return (C.c_uint64 * len(v))(*v)


def _arc_refusals(e: KbrEngine, call, lo, hi):
    """the three arc-map refusals of one shard step on a context that holds [lo, hi) of N nodes"""
    for bounds, match in (((0, hi, lo, N), "EINVAL: shard_lo must be non-decreasing$"),
                          ((1, lo, hi, N), r"EINVAL: shard_lo must cover \[0, n\)$"),
                          ((0, lo, hi, N - 1), r"EINVAL: shard_lo must cover \[0, n\)$"),
                          ((0, lo, hi - 1, N), "EINVAL: this context's arc is not one of shard_lo's arcs$"),
                          ((0, lo + 1, hi, N), "EINVAL: this context's arc is not one of shard_lo's arcs$")):
        with pytest.raises(KbrError, match=match):
            e._chk(call(_u64(*bounds), C.c_uint32(len(bounds) - 1)), "step")


def test_shard_steps_refuse_a_bad_arc_map(inputs):
    net = inputs["net"]
    ids, xy = np.ascontiguousarray(net.ids), np.ascontiguousarray(net.xy)
    lo, hi = 16, 40
    null, zero = C.c_void_p(None), C.c_uint64(0)
    cnt = [(C.c_ulonglong * 1)(0) for _ in range(3)]
    buf = (C.c_uint8 * 4096)()
    with KbrEngine(0, Params.chord()) as e:
        L = e._L
        e._chk(L.ovs_chord_load_shard(e._h, _ptr(ids), C.c_uint64(N), _ptr(xy), C.c_uint64(lo), C.c_uint64(hi), C.c_uint32(0)),
               "ovs_chord_load_shard")
        _arc_refusals(e, lambda b, ns: L.ovs_shard_step(e._h, null, zero, null, zero, null, null, zero, null, b, ns, null), lo, hi)
    with KbrEngine(0, Params.kademlia()) as e:
        L = e._L
        e._chk(L.ovs_kad_load_shard(e._h, _ptr(ids), C.c_uint64(N), _ptr(xy), C.c_uint64(lo), C.c_uint64(hi), C.c_uint32(0)),
               "ovs_kad_load_shard")
        _arc_refusals(e, lambda b, ns: L.ovs_kad_shard_mig_step(e._h, null, zero, null, null, C.c_uint32(0), null, zero, null,
                                                                null, zero, null, b, ns, null), lo, hi)
        e._chk(L.ovs_kad_shard_begin(e._h, null, null, zero, C.c_uint32(0), null), "ovs_kad_shard_begin")
        e.sync()
        for bounds, match in (((0, hi, lo, N), "EINVAL: shard_lo must be non-decreasing$"),
                              ((1, lo, hi, N), r"EINVAL: shard_lo must cover \[0, n\)$"),
                              ((0, lo, hi - 1, N), "EINVAL: this context's arc is not one of shard_lo's arcs$")):
            with pytest.raises(KbrError, match=match):
                e._chk(L.ovs_kad_shard_step(e._h, buf, zero, cnt[0], buf, zero, cnt[1], cnt[2], _u64(*bounds),
                                            C.c_uint32(len(bounds) - 1), null), "ovs_kad_shard_step")


def test_refresh_calls_share_their_refusals(inputs):
    net = inputs["net"]
    keys, src = W.lookups(net.ids, 8, 3, node_ids=False)
    HOPS = "ENOTSUP: refresh lookups need hopCountMax >= 1$"
    MERGE = r"ENOTSUP: refresh lookups implement lookupMerge, strictParallelRpcs, parallelRpcs 1\.\.8$"
    RED = r"ENOTSUP: refresh lookups implement redundantNodes 1\.\.64$"
    with KbrEngine(0, Params.kademlia()) as e:
        e.kad_load(net.ids, net.xy)
        good = e.get_params().replace(lookupMerge=1, lookupStrictParallelRpcs=1)
        refresh = lambda R=8: e.kad_refresh(keys, src, R)
        maint = lambda: e.kad_maintenance_round(np.arange(4, dtype=np.uint32))
        e.set_params(good)
        assert len(refresh()["hops"]) == 8
        for bad, match in ((dict(hopCountMax=0), HOPS), (dict(lookupMerge=0), MERGE), (dict(lookupStrictParallelRpcs=0), MERGE),
                           (dict(lookupParallelRpcs=9), MERGE)):
            e.set_params(good.replace(**bad))
            _refused(e, "ovs_kad_refresh_batch: " + match, refresh)
            _refused(e, "ovs_kad_maintenance_round: " + match, maint)
        # each call's own order: the refresh batch checks its R first, a round its routingType first and
        # its redundancies last
        e.set_params(good.replace(hopCountMax=0))
        _refused(e, RED, refresh, 65)
        _refused(e, RED, refresh, 0)
        e.set_params(good.replace(hopCountMax=0, lookupRedundantNodes=65))
        _refused(e, HOPS, maint)
        e.set_params(good.replace(lookupRedundantNodes=65))
        _refused(e, "ovs_kad_maintenance_round: " + RED, maint)
        e.set_params(good.replace(routingType=1, hopCountMax=0))
        _refused(e, "ENOTSUP: maintenance rounds run iterative refresh lookups$", maint)
        e.set_params(good)
        _refused(e, "EINVAL: node index out of range$", e.kad_maintenance_round, [N])
        assert len(refresh()["hops"]) == 8


@pytest.mark.parametrize("name,match", [
    ("kad", "ENOTSUP: the snapshot rule builds b = 1 kademlia tables: other b / bucketType through ovs_kad_load_tables_csr$"),
    ("kad_tables", "ENOTSUP: k-stride tables hold b = 1 kademlia buckets: other b / bucketType through ovs_kad_load_tables_csr$"),
])
def test_b1_loaders_point_to_the_csr_loader(name, match, inputs):
    c = _case(name, inputs)
    for other in (dict(b=2), dict(bucketType=1), dict(b=2, k=17)):      # before the k / s refusal
        with KbrEngine(0, c.params.replace(**other)) as e:
            _refused(e, match, c.load, e)
            _no_network(e, c.inp["net"])
