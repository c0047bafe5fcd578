// chord_bcast.hpp -- host launchers of the Chord broadcast kernels (chord_bcast.hip; internal).
#pragma once
#include "engine.hpp"

namespace ovs {

// One reached (broadcast, node): the frontier item of the level it was reached in, kept afterwards
// for the statistics.  24 B; the queue holds every item of a call, level after level.
struct alignas(8) BcastItem {
    uint32_t b;        // broadcast of the batch
    uint32_t node;     // the node reached
    uint32_t limit;    // node whose key is the CoordBroadcastInfo limit the request carried
    uint16_t hops;     // ttl - TTL on arrival (= the level)
    uint16_t rank;     // position in the parent's request list
    int64_t t;         // arrival, ns
};
static_assert(sizeof(BcastItem) == 24, "BcastItem is 24 B");

constexpr int BCAST_MAX_HOPS = 161;          // a path uses every finger level and successor 0 at most once
constexpr int BCAST_HIST = BCAST_MAX_HOPS + 1;

struct BcastConsts {
    int64_t bw;        // T(L*8/datarate) of one BroadcastRequestCall on the wire
    int64_t access2;   // 2*T(accessDelay)
    int32_t round;     // SimTime(double) rounding rule
};

// ctl[0] = queue length (items appended so far), ctl[1] = error bits
constexpr unsigned long long BCAST_ERR_INITIATOR = 1, BCAST_ERR_OVERFLOW = 2;

// every record "not reached": {-1, NONE, 0, 0}
hipError_t launch_bcast_fill(ovs_bcast_node* nodes, uint64_t total, hipStream_t s);
// the initiators' items (queue[0 .. nb), hops 0, time 0) and records; ctl zeroed first by the caller
hipError_t launch_bcast_init(const uint32_t* initiators, uint64_t nb, uint32_t n, BcastItem* queue, uint64_t cap,
                             ovs_bcast_node* nodes, unsigned long long* ctl, hipStream_t s);
// one level: forwardBroadcast at queue[lo .. hi), children appended at ctl[0].  wave_per_item: a
// wave shares one node's row (few nodes, many children each); else one lane per node
hipError_t launch_bcast_level(const ChordView& V, const BcastConsts& BC, BcastItem* queue, uint64_t lo, uint64_t hi,
                              uint64_t cap, ovs_bcast_node* nodes, unsigned long long* ctl, bool wave_per_item,
                              hipStream_t s);
// hist[b * BCAST_HIST + hops] += nodes of broadcast b reached at that hop count, last[b] = latest
// arrival (both zeroed by the caller)
hipError_t launch_bcast_stats(const BcastItem* queue, uint64_t total, unsigned long long* hist,
                              unsigned long long* last, hipStream_t s);

}  // namespace ovs
