// app_bcast.cpp -- overlay broadcasts (BroadcastTestApp.cc:197-340) on fixed tables: over Chord::forwardBroadcast
// (Chord.cc:1410-1445) on converged rings and over Pastry::forwardBroadcast (Pastry.cc:1343-1390) on Pastry
// tables.  The two calls differ in their refusals and in the kernel that expands one level; the checks on the
// batch, the level loop and the statistics are bcast_batch, once.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "chord_bcast.hpp"
#include "cstddev.hpp"
#include "ctx.hpp"
#include "pastry_bcast.hpp"

using namespace ovs;

namespace {

// SimpleUnderlayNetwork.underlayConfigurator.sendQueueLength = 1MB (default.ini:553): a packet that would leave
// later than a full queue takes to drain is dropped (SimpleNodeEntry.cc:168-181); drops are not modelled.  Read
// as 10^6 B, the smaller of the two readings of "MB".
constexpr int64_t SEND_QUEUE_BYTES = 1000000;

// BROADCASTREQUESTCALL_L = BASECALL_L 256 + query.size() + NODEHANDLE_L 208 + REQUESTID_L 8 + TTL_L 8
// bits (CommonMessages.msg:59-71, 90: the query's size in bytes is added as bits); on the wire in a
// BaseAppDataMessage (40 bits, no BaseRouteMessage: BaseOverlay.cc:1340-1341) plus UDP/IP 28 B.  An overlay's
// BroadcastInfo object rides along by addObject and adds nothing to the call's length.
int64_t call_bits(int32_t query_bytes) { return 480 + (int64_t)query_bytes; }
int64_t call_wire_bytes(int32_t query_bytes) { return (call_bits(query_bytes) + 40 + 7) / 8 + 28; }

// What both broadcast calls do once their overlay's own refusals have passed: the checks on ttl, query_bytes,
// the initiators and the batch size, then the level loop and the statistics.  The level loop: level k's items
// are queue[lo, hi); its launch appends level k + 1 behind them and the queue length read back is the next hi.
// It ends on an empty level or after min(ttl, 161) levels (a node that receives TTL 0 forwards nothing; a Chord
// path uses each finger level and successor 0 once, a Pastry path each routing-table row once).
//   prepare(s): what the overlay's tables need before the first launch on s
//   level(queue, lo, hi, cap, dn, ctl, BC, wave_per_item, s): the launch of one level
//   overflow: the failure text for a queue that fills up, i.e. a node reached twice
template <class Prepare, class Level>
ovs_status bcast_batch(ovs_ctx* c, const uint32_t* initiators, uint64_t nb, int32_t ttl, int32_t query_bytes,
                       ovs_bcast_node* nodes, ovs_bcast_stats* stats, uint32_t flags, void* stream, const char* overflow,
                       Prepare prepare, Level level)
{
    if (ttl < 0 || ttl > 65535) return fail(c, OVS_EINVAL, "ttl must be 0..65535");
    if (query_bytes < 0) return fail(c, OVS_EINVAL, "query_bytes must be >= 0");
    ovs_status st = check_common(c, c->P);
    if (st != OVS_OK) return st;
    const bool dev = flags & OVS_DEVICE_PTRS;
    if (!dev)
        for (uint64_t b = 0; b < nb; ++b)
            if (initiators[b] >= c->n)
                return fail(c, OVS_EINVAL, "initiator out of range (broadcast " + std::to_string(b) + ")");
    if (nb > 0xFFFFFFFFull || nb > (1ull << 38) / c->n) return fail(c, OVS_EINVAL, "too many broadcasts in one batch");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;   // NULL = the default stream
    if (nb == 0) return OVS_OK;
    st = prepare(s);
    if (st != OVS_OK) return st;

    const uint64_t call_len = (uint64_t)((call_bits(query_bytes) + 7) / 8);
    const int64_t wire_bytes = call_wire_bytes(query_bytes);
    // BROADCASTREQUESTRESPONSE_L = BASERESPONSE_L (256 + AUTHBLOCK_L) + REQUESTID_L 8 + 1 bits
    const uint64_t resp_len = (uint64_t)((265 + (c->P.measureAuthBlock ? 800 : 0) + 7) / 8);
    BcastConsts BC{};
    BC.round = c->P.simtimeRound;
    BC.bw = simtime_host((double)(wire_bytes * 8) / c->P.datarate, c->P.simtimeRound);
    BC.access2 = 2 * simtime_host(c->P.accessDelay, c->P.simtimeRound);

    const uint64_t cap = nb * c->n;             // every (broadcast, node) is reached at most once
    CallFrame F(dev, s);
    const uint32_t* di = F.in(initiators, nb);
    ovs_bcast_node* dn = nodes ? F.out(nodes, cap) : nullptr;
    unsigned long long* ctl = F.scratch<unsigned long long>(2);
    unsigned long long* hist = stats ? F.scratch<unsigned long long>(nb * (BCAST_HIST + 1)) : nullptr;
    if (!F.ok()) return frame_fail(c, F);
    const CachedBuf::Lease ql = c->bq.acquire(sizeof(BcastItem) * cap, s);
    if (!ql) return lease_fail(c, "broadcast queue", ql);
    BcastItem* queue = reinterpret_cast<BcastItem*>(ql.data());

    HIPCHK(c, hipMemsetAsync(ctl, 0, 2 * sizeof *ctl, s));
    if (dn) HIPCHK(c, launch_bcast_fill(dn, cap, s));
    HIPCHK(c, launch_bcast_init(di, nb, (uint32_t)c->n, queue, cap, dn, ctl, s));
    // a wave per node while the level has fewer nodes than the device has wave slots to fill (their
    // rows are long there); a lane per node after that.  OVS_BCAST_WAVE_ITEMS moves the switch (A/B, tests)
    const char* wenv = std::getenv("OVS_BCAST_WAVE_ITEMS");
    const uint64_t wave_items = wenv ? (uint64_t)std::strtoull(wenv, nullptr, 10) : (uint64_t)c->num_cu * 16;
    const int levels = std::min<int>(ttl, BCAST_MAX_HOPS);
    unsigned long long h[2] = {0, 0};      // queue length, error bits
    HIPCHK(c, read_ctl(h, ctl, 2, s));
    uint64_t lo = 0, hi = nb;              // level 0: the initiators
    for (int k = 0; !h[1] && k < levels && hi > lo; ++k) {
        HIPCHK(c, level(queue, lo, hi, cap, dn, ctl, BC, hi - lo <= wave_items, s));
        HIPCHK(c, read_ctl(h, ctl, 2, s));
        lo = hi;
        hi = std::min<uint64_t>(h[0], cap);
    }
    if (h[1] & BCAST_ERR_INITIATOR) return fail(c, OVS_EINVAL, "initiator out of range");
    if (h[1]) return fail(c, OVS_EDEVICE, overflow);
    const uint64_t total = hi;

    std::vector<unsigned long long> hh;
    if (stats) {
        unsigned long long* last = hist + nb * BCAST_HIST;
        HIPCHK(c, hipMemsetAsync(hist, 0, sizeof(unsigned long long) * nb * (BCAST_HIST + 1), s));
        HIPCHK(c, launch_bcast_stats(queue, total, hist, last, s));
        hh.resize(nb * (BCAST_HIST + 1));
        HIPCHK(c, hipMemcpyAsync(hh.data(), hist, sizeof(unsigned long long) * hh.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    if (F.finish() != hipSuccess) return frame_fail(c, F);
    for (uint64_t b = 0; stats && b < nb; ++b) {
        const unsigned long long* hb = &hh[b * BCAST_HIST];
        ovs_bcast_stats& o = stats[b];
        std::memset(&o, 0, sizeof o);
        uint64_t reached = 0, sum = 0, sq = 0;
        int hmin = -1, hmax = 0;
        for (int k = 0; k < BCAST_HIST; ++k) {
            if (!hb[k]) continue;
            reached += hb[k]; sum += hb[k] * (uint64_t)k; sq += hb[k] * (uint64_t)k * (uint64_t)k;
            if (hmin < 0) hmin = k;
            hmax = k;
        }
        o.expected = c->n;
        o.expired = ttl < BCAST_HIST ? hb[ttl] : 0;            // received TTL 0 (BroadcastTestApp.cc:290-299)
        o.actual = reached - o.expired;
        o.messages = reached ? 2 * reached - 1 : 0;            // a call per node but the initiator + a response per node
        // an expired node's response never gets a bit length (BroadcastTestApp.cc:292-297): 0 bytes
        o.bytes = reached ? (reached - 1) * call_len + o.actual * resp_len : 0;
        o.last_arrival_ns = (int64_t)hh[nb * BCAST_HIST + b];
        // cStdDev of "Broadcast: Hop count" (BroadcastTestApp.cc:260) from the histogram's exact sums
        CStdDev::from_sums(reached, (double)sum, (double)sq, (double)hmin, (double)hmax).finish(o.hop_count);
    }
    return OVS_OK;
}

}  // namespace

extern "C" {

ovs_status ovs_chord_broadcast_batch(ovs_ctx* c, const uint32_t* initiators, uint64_t nb, int32_t ttl,
                                     int32_t query_bytes, ovs_bcast_node* nodes, ovs_bcast_stats* stats, uint32_t flags,
                                     void* stream)
{
    if (!c || (nb && !initiators)) return OVS_EINVAL;
    if (!c->overlay) return fail(c, OVS_ESTATE, "no network loaded");
    if (c->overlay == OVS_OVERLAY_BROOSE) return fail(c, OVS_ENOTSUP, "the broadcast is implemented for Chord rings, not Broose");
    if (c->overlay != OVS_OVERLAY_CHORD) return fail(c, OVS_ESTATE, "the broadcast is implemented for Chord rings");
    if (!c->ideal)
        return fail(c, OVS_ENOTSUP, "broadcast on explicit tables: the ranges overlap there and the first arrival in time "
                                    "decides who forwards, which needs a time-ordered replay (converged rings only)");
    if (c->shard_lo != 0 || c->shard_hi != c->n)
        return fail(c, OVS_ENOTSUP, "broadcast on one arc of a sharded ring is not implemented");
    return bcast_batch(
        c, initiators, nb, ttl, query_bytes, nodes, stats, flags, stream,
        "broadcast queue overflow: a node was reached twice (ring not converged?)",
        [&](hipStream_t s) -> ovs_status { return ensure_nodes(c, s); },
        [&](BcastItem* queue, uint64_t lo, uint64_t hi, uint64_t cap, ovs_bcast_node* dn, unsigned long long* ctl,
            const BcastConsts& BC, bool wave_per_item, hipStream_t s) {
            return launch_bcast_level(chord_view(c), BC, queue, lo, hi, cap, dn, ctl, wave_per_item, s);
        });
}

// Explicit tables run as the rule's do: the loader has verified every slot's prefix (pastry_validate_tables),
// which is all the exactly-once argument needs; nodes behind an emptied slot are not reached.
ovs_status ovs_pastry_broadcast_batch(ovs_ctx* c, const uint32_t* initiators, uint64_t nb, int32_t ttl,
                                      int32_t query_bytes, ovs_bcast_node* nodes, ovs_bcast_stats* stats, uint32_t flags,
                                      void* stream)
{
    if (!c || (nb && !initiators)) return OVS_EINVAL;
    if (!c->overlay) return fail(c, OVS_ESTATE, "no network loaded");
    if (c->overlay != OVS_OVERLAY_PASTRY) return fail(c, OVS_ESTATE, "no Pastry network loaded");
    // one node queues up to rows * (2^b - 1) requests at once; beyond sendQueueLength the reference drops
    const int64_t fanout = (int64_t)c->pastry.rows * (c->pastry.sh.P() - 1);
    if (query_bytes >= 0 && fanout * call_wire_bytes(query_bytes) > SEND_QUEUE_BYTES)
        return fail(c, OVS_ENOTSUP, "Pastry broadcast: " + std::to_string(fanout) + " requests of " +
                                        std::to_string(call_wire_bytes(query_bytes)) + " B can exceed sendQueueLength = 1MB in one "
                                        "node's transmit queue; drops there are not modelled");
    return bcast_batch(
        c, initiators, nb, ttl, query_bytes, nodes, stats, flags, stream,
        "broadcast queue overflow: a node was reached twice (a table slot outside its row's prefix?)",
        [](hipStream_t) -> ovs_status { return OVS_OK; },
        [&](BcastItem* queue, uint64_t lo, uint64_t hi, uint64_t cap, ovs_bcast_node* dn, unsigned long long* ctl,
            const BcastConsts& BC, bool wave_per_item, hipStream_t s) {
            return launch_pastry_bcast_level(c->pastry, c->xy, BC, queue, lo, hi, cap, dn, ctl, wave_per_item, s);
        });
}

}  // extern "C"
