// app_dht.cpp -- the DHT tier (DHT.cc) and DHTTestApp's statistics.  The lookup phase is the LookupCall
// seam (lookup_check / lookup_device; on a Pastry context pastry_lookup_check / pastry_lookup_device) on this
// call's staged copies; dht.hip adds the replica phase and owns the storage.  Every refusal happens before
// anything is staged.
#include <algorithm>
#include <cstring>
#include <new>

#include "app_dht.hpp"
#include "cstddev.hpp"

using namespace ovs;

namespace ovs {

// the tier's own refusals, then the LookupCall's (lookup_check)
ovs_status dht_check(ovs_ctx* c, const ovs_dht_params* dp, hipStream_t s)
{
    if (!c->overlay) return fail(c, OVS_ESTATE, "no network loaded");
    if (c->overlay == OVS_OVERLAY_KOORDE)
        return fail(c, OVS_ENOTSUP, "DHT on Koorde: LookupCalls (ovs_lookup_batch) are not implemented for Koorde");
    if (c->overlay == OVS_OVERLAY_EPICHORD)
        return fail(c, OVS_ENOTSUP, "DHT on EpiChord: LookupCalls (ovs_lookup_batch) are not implemented for EpiChord");
    if (c->overlay == OVS_OVERLAY_BROOSE)
        return fail(c, OVS_ENOTSUP, "DHT on Broose: LookupCalls (ovs_lookup_batch) are not implemented for Broose");
    const bool chord = c->overlay == OVS_OVERLAY_CHORD;
    // a Pastry context is never a shard; its LookupCall is pastry_lookup_check / pastry_lookup_device
    const bool pastry = c->overlay == OVS_OVERLAY_PASTRY;
    if (!pastry &&
        (chord ? (c->ideal && (c->shard_lo != 0 || c->shard_hi != c->n)) : (c->kad.lo != 0 || c->kad.hi != c->n)))
        return fail(c, OVS_ENOTSUP, "DHT on a shard context: the storage and the LookupCall need the whole network on one device");
    if (c->P.routingType != 0)
        return fail(c, OVS_ENOTSUP, "DHT with a recursive or exhaustive routingType: the lookup's messages are not the "
                                    "source's own, so its transmit queue at lookup completion is not modelled; iterative only");
    if (c->P.lookupParallelRpcs > 1)
        return fail(c, OVS_ENOTSUP, "DHT with lookupParallelRpcs > 1: the source's transmit queue could still hold "
                                    "FindNodeCalls when the lookup completes");
    if (dp->secureMaintenance) return fail(c, OVS_ENOTSUP, "dht.secureMaintenance: sibling votes are not implemented");
    if (dp->invalidDataAttack) return fail(c, OVS_ENOTSUP, "dht.invalidDataAttack: malicious nodes are not implemented");
    if (dp->maintenanceAttack) return fail(c, OVS_ENOTSUP, "dht.maintenanceAttack: malicious nodes are not implemented");
    if (dp->numReplica < 1 || dp->numReplica > DHT_MAXR)
        return fail(c, OVS_ENOTSUP, "dht.numReplica outside 1..8");
    if (dp->numGetRequests < 1 || dp->numGetRequests > DHT_MAXR)
        return fail(c, OVS_ENOTSUP, "dht.numGetRequests outside 1..8");
    if (!(dp->ratioIdentical > 0 && dp->ratioIdentical <= 1))
        return fail(c, OVS_ENOTSUP, "dht.ratioIdentical outside (0, 1]: a get could wait for ever with no hash chosen");
    // DHT.cc:84-87: "numReplica bigger than what this overlay can handle"
    // ... on Pastry numberOfLeaves / 2 (BasePastry.cc:1090-1093)
    if (dp->numReplica > (pastry ? c->pastry.sh.L / 2 : chord ? c->P.successorListSize : c->P.s))
        return fail(c, OVS_ENOTSUP, "dht.numReplica > getMaxNumSiblings()");
    if (!c->dht.slots) return fail(c, OVS_ESTATE, "no DHT store: ovs_dht_store_create first");
    int32_t ns;
    // a DHT operation sends FindNodeCalls and direct RPCs, no route message: routeMsgAcks does not enter
    return pastry ? pastry_lookup_check(c, c->P, dp->numReplica, &ns) : lookup_check(c, c->P, dp->numReplica, s, &ns);
}

DhtConsts dht_consts(const ovs_ctx* c, const ovs_dht_params* dp)
{
    DhtConsts C{};
    C.timeout = simtime_host(c->P.rpcUdpTimeout, c->P.simtimeRound);
    C.access = simtime_host(c->P.accessDelay, c->P.simtimeRound);
    C.datarate = c->P.datarate;
    C.ratio = dp->ratioIdentical;
    C.round = c->P.simtimeRound;
    C.auth = c->P.measureAuthBlock ? 800 : 0;      // AUTHBLOCK_L (CommonMessages.msg:45-47, 57)
    C.R = dp->numReplica;
    C.G = dp->numGetRequests;
    C.nnodes = (uint32_t)c->n;
    return C;
}

// one launch of the statistics kernel over device records: the sums and, with node_rows, the four per-node
// counter rows (without: no per-node counting, the sources are not read against the network)
ovs_status dhttest_sums(ovs_ctx* c, CallFrame& F, const ovs_dht_put_out* dpo, const uint32_t* dps, uint64_t n_put,
                        const ovs_dht_get_out* dgo, const ovs_dht_op* dgp, const uint32_t* dgs, const ovs_dhttest_expect* dex,
                        uint64_t n_get, bool node_rows, hipStream_t s, DhtStatsDev* h, std::vector<uint32_t>* nc)
{
    const uint64_t N = node_rows ? c->n : 0;
    DhtStatsDev* S = F.scratch<DhtStatsDev>(1);
    uint32_t* counts = F.scratch<uint32_t>(4 * N);
    if (!F.ok()) return frame_fail(c, F);
    ovs_status st = OVS_OK;
    nc->assign(1, 0);          // without rows: one word, so that the read-back has somewhere to go
    if (node_rows && (st = node_counters(c, 4, *nc)) != OVS_OK) return st;
    const hipError_t e = launch_dhttest_stats(dpo, dps, n_put, dgo, dgp, dgs, dex, n_get, (uint32_t)N, S, counts, c->num_cu, s);
    return stats_read(c, s, e, h, S, sizeof *h, nc->data(), counts, sizeof(uint32_t) * nc->size(), "DHTTestApp statistics kernel");
}

void dhttest_finish(const DhtStatsDev& h, const std::vector<uint32_t>& nc, uint64_t N, double measured_time_s,
                    ovs_dhttest_stats* stats)
{
    ovs_dhttest_stats& o = *stats;
    std::memset(&o, 0, sizeof o);
    o.num_put_success = h.put_ok; o.num_put_error = h.put_err;
    o.num_get_success = h.get_ok; o.num_get_error = h.get_err;
    o.put_latency_sum_ns = h.put_lat; o.put_latency_sumsq_lo = h.put_sq_lo; o.put_latency_sumsq_hi = h.put_sq_hi;
    o.get_latency_sum_ns = h.get_lat; o.get_latency_sumsq_lo = h.get_sq_lo; o.get_latency_sumsq_hi = h.get_sq_hi;
    o.get_latency_count = h.get_lat_n;
    o.put_hop_count = h.put_hop_n; o.put_hop_sum = h.put_hop;
    o.get_hop_count = h.get_hop_n; o.get_hop_sum = h.get_hop;
    o.normal_messages = h.msgs; o.num_bytes_normal = h.bytes;
    // cStdDev of SIMTIME_DBL(latency) from the exact integer sums: sum and sum of squares in seconds
    auto lat = [](uint64_t cnt, uint64_t sum, uint64_t lo, uint64_t hi, uint64_t mn, uint64_t mx, int64_t* omin, int64_t* omax,
                  ovs_stddev& d) {
        if (!cnt) return;
        *omin = (int64_t)mn; *omax = (int64_t)mx;
        CStdDev::from_sums(cnt, (double)sum * 1e-9, ((double)hi * 18446744073709551616.0 + (double)lo) * 1e-18,
                           (double)mn * 1e-9, (double)mx * 1e-9).finish(d);
    };
    lat(h.put_ok, h.put_lat, h.put_sq_lo, h.put_sq_hi, h.put_min, h.put_max, &o.put_latency_min_ns, &o.put_latency_max_ns,
        o.put_latency_s);
    lat(h.get_lat_n, h.get_lat, h.get_sq_lo, h.get_sq_hi, h.get_min, h.get_max, &o.get_latency_min_ns, &o.get_latency_max_ns,
        o.get_latency_s);
    // DHTTestApp::finishApp (DHTTestApp.cc:439-467) at every node, in node order
    if (measured_time_s >= 0.1) {
        CStdDev a[5];
        for (uint64_t v = 0; v < N; ++v) {
            const uint32_t ps = nc[v], pe = nc[N + v], gs = nc[2 * N + v], ge = nc[3 * N + v];
            a[0].collect((double)ps / measured_time_s);
            a[1].collect((double)pe / measured_time_s);
            a[2].collect((double)gs / measured_time_s);
            a[3].collect((double)ge / measured_time_s);
            if (gs + ge > 0) a[4].collect((double)gs / (double)(gs + ge));
        }
        ovs_stddev* sd[5] = {&o.put_success_per_s, &o.put_error_per_s, &o.get_success_per_s, &o.get_error_per_s,
                             &o.get_success_ratio};
        for (int k = 0; k < 5; ++k) a[k].finish(*sd[k]);
    }
}

}  // namespace ovs

namespace {

// put (is_put) or get: checks, stages, runs the lookup and the replica phase
ovs_status dht_batch(ovs_ctx* c, const ovs_dht_params* dp, const ovs_key160* keys, const uint32_t* src, const ovs_dht_op* ops,
                     uint64_t n, void* out, bool is_put, uint32_t flags, void* stream)
{
    static_assert(sizeof(ovs_dht_op) == 32 && sizeof(ovs_dht_put_out) == 24 && sizeof(ovs_dht_get_out) == 40 &&
                  sizeof(ovs_dht_entry) == 48, "DHT record sizes");
    if (!c || !dp || (n && (!keys || !src || !ops || !out))) return OVS_EINVAL;
    const bool dev = flags & OVS_DEVICE_PTRS;
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;
    ovs_status st = dht_check(c, dp, s);
    if (st != OVS_OK) return st;
    if (n >= 0xFFFFFFFFull) return fail(c, OVS_EINVAL, "DHT batches hold fewer than 2^32 operations");
    if (n == 0) return OVS_OK;
    st = check_sources(c, src, n, dev);
    if (st != OVS_OK) return st;
    if (!dev) {
        for (uint64_t i = 0; i < n; ++i) {
            if (ops[i].t0_ns < 0) return fail(c, OVS_EINVAL, "DHT operation with a negative time");
            if (ops[i].id == 0)
                return fail(c, OVS_ENOTSUP, is_put ? "put with id = 0: DHT.cc:869-874 draws a random id; the caller draws it"
                                                   : "get with id = 0: wildcard gets are not implemented");
            if (ops[i].kind == 0)
                return fail(c, OVS_ENOTSUP, is_put ? "put with kind = 0 (DHTDataStorage.cc:170-173 refuses it)"
                                                   : "get with kind = 0: wildcard gets are not implemented");
        }
    }
    const DhtConsts C = dht_consts(c, dp);
    const uint64_t np = n * (uint64_t)C.R;
    CallFrame F(dev, s);
    const K160* dk = F.in(reinterpret_cast<const K160*>(keys), n);
    const uint32_t* ds = F.in(src, n);
    const ovs_dht_op* dops = F.in(ops, n);
    ovs_dht_put_out* dput = is_put ? F.out(static_cast<ovs_dht_put_out*>(out), n) : nullptr;
    ovs_dht_get_out* dget = is_put ? nullptr : F.out(static_cast<ovs_dht_get_out*>(out), n);
    if (!F.ok()) return frame_fail(c, F);
    const uint64_t o_sib = up256(sizeof(ovs_lookup_out) * n);
    const uint64_t o_pt = o_sib + up256(sizeof(uint32_t) * np);
    const uint64_t o_ps = o_pt + up256(sizeof(long long) * np);
    CachedBuf::Lease buf = c->dhtb.acquire(is_put ? o_ps + sizeof(uint32_t) * np : o_pt, s);
    if (!buf) return lease_fail(c, "DHT buffers", buf);
    ovs_lookup_out* dlook = reinterpret_cast<ovs_lookup_out*>(buf.data());
    uint32_t* dsib = reinterpret_cast<uint32_t*>(buf.data() + o_sib);
    // DHT.cc:504-516, 523-535: LookupCall{key, numSiblings = numReplica}, an internal RPC
    st = c->overlay == OVS_OVERLAY_PASTRY ? pastry_lookup_device(c, c->P, C.R, dk, ds, n, dlook, dsib, s)
                                          : lookup_device(c, c->P, C.R, dk, ds, n, reinterpret_cast<ovs_route_out*>(dlook), dsib, s);
    if (st != OVS_OK) return st;
    hipError_t e;
    DhtHeader h{};
    if (is_put) {
        long long* pt = reinterpret_cast<long long*>(buf.data() + o_pt);
        uint32_t* ps = reinterpret_cast<uint32_t*>(buf.data() + o_ps);
        e = launch_dht_put_plan(c->dht, C, dlook, dsib, dk, ds, dops, c->xy, n, dput, pt, c->num_cu, s);
        if (e == hipSuccess) e = launch_dht_put_apply(c->dht, C, dsib, dk, dops, n, pt, ps, c->num_cu, s);
        if (e == hipSuccess && !dev) e = hipMemcpyAsync(&h, c->dht.hdr, sizeof h, hipMemcpyDeviceToHost, s);
    } else {
        e = launch_dht_get(c->dht, C, dlook, dsib, dk, ds, dops, c->xy, n, dget, s);
    }
    buf.release();
    if (e != hipSuccess) return hip_fail(c, e, "DHT kernel");
    if (F.finish() != hipSuccess) return frame_fail(c, F);
    if (h.last_refused)
        return fail(c, OVS_ENOMEM, "DHT store too small for this put batch (slots in use + pairs without a slot > capacity); "
                                   "nothing was changed");
    if (h.last_collisions)
        return fail(c, OVS_EDEVICE, "DHT store: a put of this batch was dropped, another entry holds its 64-bit tag");
    return OVS_OK;
}

}  // namespace

extern "C" {

void ovs_dht_params_default(ovs_dht_params* out)
{
    if (!out) return;
    std::memset(out, 0, sizeof *out);
    out->numReplica = 4;         // default.ini: **.tier*.dht.numReplica = 4
    out->numGetRequests = 4;
    out->ratioIdentical = 0.5;
}

ovs_status ovs_dht_store_create(ovs_ctx* c, uint64_t capacity)
{
    if (!c) return OVS_EINVAL;
    if (!c->overlay) return fail(c, OVS_ESTATE, "no network loaded");
    if (capacity < 1 || capacity >= 0xFFFFFFFFull) return fail(c, OVS_EINVAL, "DHT store capacity outside 1..2^32-2");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->dht.slots) hipFree(c->dht.slots);
    if (c->dht.hdr) hipFree(c->dht.hdr);
    c->dht = DhtStore{};
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, sizeof(DhtSlot) * capacity);
    if (e != hipSuccess) return device_fail(c, e, "DHT store");
    c->dht.slots = static_cast<DhtSlot*>(p);
    e = hipMalloc(&p, sizeof(DhtHeader));
    if (e != hipSuccess) {
        hipFree(c->dht.slots);
        c->dht = DhtStore{};
        return device_fail(c, e, "DHT store header");
    }
    c->dht.hdr = static_cast<DhtHeader*>(p);
    c->dht.cap = capacity;
    return ovs_dht_store_clear(c);
}

ovs_status ovs_dht_store_clear(ovs_ctx* c)
{
    if (!c) return OVS_EINVAL;
    if (!c->dht.slots) return fail(c, OVS_ESTATE, "no DHT store: ovs_dht_store_create first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemsetAsync(c->dht.slots, 0, sizeof(DhtSlot) * c->dht.cap, c->stream));
    HIPCHK(c, hipMemsetAsync(c->dht.hdr, 0, sizeof(DhtHeader), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OVS_OK;
}

ovs_status ovs_dht_store_count(ovs_ctx* c, uint64_t* slots, uint64_t* refused, uint64_t* collisions)
{
    if (!c) return OVS_EINVAL;
    if (!c->dht.slots) return fail(c, OVS_ESTATE, "no DHT store: ovs_dht_store_create first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    DhtHeader h{};
    HIPCHK(c, hipMemcpy(&h, c->dht.hdr, sizeof h, hipMemcpyDeviceToHost));
    if (slots) *slots = h.used;
    if (refused) *refused = h.refused;
    if (collisions) *collisions = h.collisions;
    return OVS_OK;
}

ovs_status ovs_dht_put_batch(ovs_ctx* c, const ovs_dht_params* dp, const ovs_key160* keys, const uint32_t* src,
                             const ovs_dht_op* ops, uint64_t n, ovs_dht_put_out* out, uint32_t flags, void* stream)
{
    return dht_batch(c, dp, keys, src, ops, n, out, true, flags, stream);
}

ovs_status ovs_dht_get_batch(ovs_ctx* c, const ovs_dht_params* dp, const ovs_key160* keys, const uint32_t* src,
                             const ovs_dht_op* ops, uint64_t n, ovs_dht_get_out* out, uint32_t flags, void* stream)
{
    return dht_batch(c, dp, keys, src, ops, n, out, false, flags, stream);
}

// DHTTestApp::handlePutResponse / handleGetResponse / finishApp (DHTTestApp.cc:147-234, 439-467) and the DHT's
// counters: integer sums on the device (dht.hip), the cStdDevs finished here, the per-node ones in node order
ovs_status ovs_dhttest_stats_batch(ovs_ctx* c, const ovs_dht_put_out* put_out, const uint32_t* put_src, uint64_t n_put,
                                   const ovs_dht_get_out* get_out, const ovs_dht_op* get_ops, const uint32_t* get_src,
                                   const ovs_dhttest_expect* expect, uint64_t n_get, double measured_time_s,
                                   ovs_dhttest_stats* stats, uint32_t flags, void* stream)
{
    static_assert(sizeof(ovs_dhttest_expect) == 24, "ovs_dhttest_expect is 24 B");
    if (!c || !stats || (n_put && (!put_out || !put_src)) || (n_get && (!get_out || !get_ops || !get_src || !expect)))
        return OVS_EINVAL;
    bool dev;
    hipStream_t s;
    ovs_status st = stats_begin(c, measured_time_s, 0.0, flags, stream, &dev, &s);
    if (st != OVS_OK) return st;
    CallFrame F(dev, s);
    const ovs_dht_put_out* dpo = F.in(put_out, n_put);
    const uint32_t* dps = F.in(put_src, n_put);
    const ovs_dht_get_out* dgo = F.in(get_out, n_get);
    const ovs_dht_op* dgp = F.in(get_ops, n_get);
    const uint32_t* dgs = F.in(get_src, n_get);
    const ovs_dhttest_expect* dex = F.in(expect, n_get);
    DhtStatsDev h{};
    std::vector<uint32_t> nc;
    st = dhttest_sums(c, F, dpo, dps, n_put, dgo, dgp, dgs, dex, n_get, true, s, &h, &nc);
    if (st != OVS_OK) return st;
    dhttest_finish(h, nc, c->n, measured_time_s, stats);
    return OVS_OK;
}

// DHTdumpCall (DHT.cc:537-551) is a diagnostic: the table is read back and filtered on the host
ovs_status ovs_dht_dump_node(ovs_ctx* c, uint32_t node, int64_t now_ns, ovs_dht_entry* entries, uint64_t cap, uint64_t* count)
{
    if (!c || !count || (cap && !entries)) return OVS_EINVAL;
    if (!c->dht.slots) return fail(c, OVS_ESTATE, "no DHT store: ovs_dht_store_create first");
    if (node >= c->n) return fail(c, OVS_EINVAL, "node outside the network");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    std::vector<DhtSlot> t;
    try {
        t.resize(c->dht.cap);
    } catch (const std::bad_alloc&) {
        return fail(c, OVS_ENOMEM, "DHT dump");
    }
    HIPCHK(c, hipMemcpy(t.data(), c->dht.slots, sizeof(DhtSlot) * c->dht.cap, hipMemcpyDeviceToHost));
    std::vector<const DhtSlot*> live;
    for (const DhtSlot& sl : t)
        if (sl.tag && sl.node == node && sl.vlen > 0 && sl.expiry > now_ns) live.push_back(&sl);
    std::sort(live.begin(), live.end(), [](const DhtSlot* a, const DhtSlot* b) {
        if (a->ins_batch != b->ins_batch) return a->ins_batch < b->ins_batch;
        if (a->ins_t != b->ins_t) return a->ins_t < b->ins_t;
        return a->ins_op < b->ins_op;
    });
    *count = live.size();
    for (uint64_t i = 0; i < live.size() && i < cap; ++i) {
        ovs_dht_entry& o = entries[i];
        std::memcpy(o.key, live[i]->key, sizeof o.key);
        o.kind = live[i]->kind; o.id = live[i]->id; o.vlen = live[i]->vlen;
        o.token = live[i]->token; o.expiry_ns = live[i]->expiry;
    }
    return OVS_OK;
}

}  // extern "C"
