"""The persistent route kernels' dynamic tail: a batch's last 30 % is handed out from
a per-launch device counter taken from the context's slot pool.  Concurrent device-pointer calls on
different streams of one context, and more calls than the pool has slots, must each see their own
counter: every result equals the same batch routed alone with static slices (OVS_NO_DYN=1)."""
from __future__ import annotations

import os

import numpy as np
import pytest

from oversim_amd import BrooseParams, KbrEngine, Params, PastryParams, workload as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("overlay", ["chord", "kademlia"])
def test_concurrent_streams_share_no_counter(engine: KbrEngine, overlay, monkeypatch):
    import torch
    dev = torch.device("cuda", 0)
    net = W.population(1 << 16, 91)
    if overlay == "chord":
        engine.set_params(Params.chord())
        engine.chord_load(net.ids, net.xy)
    else:
        engine.set_params(Params.kademlia().replace(lookupParallelRpcs=3))
        engine.kad_load(net.ids, net.xy)
    n = 1 << 18                                       # the dynamic tail's threshold
    batches = []
    for b in range(3):
        keys, src = W.lookups(net.ids, n, 100 + b, node_ids=False)
        batches.append((torch.from_numpy(keys.view(np.int32)).to(dev), torch.from_numpy(src.view(np.int32)).to(dev)))
    # reference: each batch alone, static slices
    monkeypatch.setenv("OVS_NO_DYN", "1")
    ref = []
    for k, s in batches:
        o = torch.empty((n, 16), dtype=torch.uint8, device=dev)
        engine.lookup_device(k.data_ptr(), s.data_ptr(), n, o.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ref.append(o.cpu().numpy())
    monkeypatch.delenv("OVS_NO_DYN")
    # 40 launches (more than the 32 slots) over three streams, queued without waiting
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    outs = []
    for i in range(40):
        b = i % 3
        k, s = batches[b]
        o = torch.empty((n, 16), dtype=torch.uint8, device=dev)
        engine.lookup_device(k.data_ptr(), s.data_ptr(), n, o.data_ptr(), streams[b].cuda_stream)
        outs.append((b, o))
    torch.cuda.synchronize()
    for i, (b, o) in enumerate(outs):
        assert np.array_equal(o.cpu().numpy(), ref[b]), f"launch {i} (batch {b}) differs from the static route"


# 3 * 2^18 + 37 lookups: at most 8 blocks of 4 waves fit on a CU, so with 256 CUs a static slice of
# 0.70 * n / (256 * 8 * 4) = 67 lookups holds the 64-lookup chunk of K1, K3, K4 and the Pastry kernels (and K2's 32) whatever the
# kernels' occupancy -- the tail is on -- and the dynamic region is no multiple of the chunk: the last
# chunk handed out is partial
N_PARTIAL = 3 * (1 << 18) + 37


def _static_and_dynamic(monkeypatch, run):
    """run() once with static slices only and once with the dynamic tail."""
    monkeypatch.setenv("OVS_NO_DYN", "1")
    ref = run()
    monkeypatch.delenv("OVS_NO_DYN")
    return ref, run()


def _assert_same(ref: dict, got: dict):
    assert ref.keys() == got.keys()
    for f in ref:
        assert np.array_equal(ref[f], got[f]), f"{f} differs from the static run"


@pytest.mark.parametrize("overlay", ["chord", "kademlia"])
def test_tail_with_partial_last_chunk_equals_static(engine: KbrEngine, overlay, monkeypatch):
    net = W.population(1 << 16, 91)
    if overlay == "chord":
        engine.set_params(Params.chord())
        engine.chord_load(net.ids, net.xy)
    else:
        engine.set_params(Params.kademlia().replace(lookupParallelRpcs=3))
        engine.kad_load(net.ids, net.xy)
    keys, src = W.lookups(net.ids, N_PARTIAL, 104, node_ids=False)
    ref, got = _static_and_dynamic(monkeypatch, lambda: engine.lookup(keys, src))
    _assert_same(ref, got)


def test_koorde_tail_equals_static(engine: KbrEngine, monkeypatch):
    net = W.population(1 << 12, 92)
    engine.set_params(Params.koorde())
    engine.koorde_load(net.ids, net.xy)
    keys, src = W.lookups(net.ids, N_PARTIAL, 105, node_ids=False)
    ref, got = _static_and_dynamic(monkeypatch, lambda: engine.lookup(keys, src))
    _assert_same(ref, got)


def test_broose_tail_equals_static(engine: KbrEngine, monkeypatch):
    net = W.population(1 << 12, 94)
    engine.set_params(Params.broose())
    engine.broose_load(net.ids, net.xy, BrooseParams.default())
    keys, src = W.lookups(net.ids, N_PARTIAL, 107, node_ids=False)
    right = (np.arange(N_PARTIAL) & 1).astype(np.uint8)
    ref, got = _static_and_dynamic(monkeypatch, lambda: engine.broose_lookup(keys, src, right, record_hops=True, count_rpcs=True))
    _assert_same(ref, got)


def test_pastry_tail_equals_static(engine: KbrEngine, monkeypatch):
    net = W.population(1 << 12, 95)
    engine.set_params(Params.pastry())
    engine.pastry_load(net.ids, net.xy, PastryParams.default(routeMsgAcks=0))
    keys, src = W.lookups(net.ids, N_PARTIAL, 108, node_ids=False)
    ref, got = _static_and_dynamic(monkeypatch, lambda: engine.pastry_lookup(keys, src, record_hops=True))
    _assert_same(ref, got)


def test_pastry_iter_tail_equals_static(engine: KbrEngine, monkeypatch):
    """k_pastry_iter in both of its forms: the LookupCall with 4 siblings and the one-way route, which needs
    routeMsgAcks off."""
    net = W.population(1 << 12, 96)
    engine.set_params(Params.pastry().replace(routingType=0))
    engine.pastry_load(net.ids, net.xy, PastryParams.default(routeMsgAcks=0))
    keys, src = W.lookups(net.ids, N_PARTIAL, 109, node_ids=False)
    ref, got = _static_and_dynamic(monkeypatch, lambda: engine.pastry_lookup_call(keys, src, 4, record_hops=True))
    _assert_same(ref, got)
    ref, got = _static_and_dynamic(monkeypatch, lambda: engine.pastry_iterative_lookup(keys, src, record_hops=True))
    _assert_same(ref, got)


def test_refresh_tail_equals_static(engine: KbrEngine, monkeypatch):
    """K2x (ovs_kad_refresh_batch): 4101 lookups fill 17 blocks = 68 waves, whose static slices of
    0.40 * 4101 / 68 = 24 lookups hold a 16-lookup chunk: the tail is on, its last chunk partial
    (4101 - 24 * 68 = 2469 = 154 * 16 + 5)."""
    net = W.population(1 << 12, 93)
    engine.set_params(Params.kademlia().replace(lookupParallelRpcs=3))
    engine.kad_load(net.ids, net.xy)
    keys, src = W.lookups(net.ids, 4101, 106, node_ids=False)
    ref, got = _static_and_dynamic(monkeypatch, lambda: engine.kad_refresh(keys, src, 8))
    _assert_same(ref, got)
