// scribe.hpp -- Scribe group trees and publishes on a converged Chord ring or converged Pastry tables
// (scribe.hip; internal).
#pragma once
#include "engine.hpp"
#include "pastry.hpp"

namespace ovs {

// The forest a context holds after ovs_scribe_build: T tree nodes sorted by (group << 32 | node) and
// their children as CSR lists in std::set<NodeHandle> order (ascending node index).  One allocation.
struct ScribeForest {
    void* block = nullptr;
    uint64_t* key = nullptr;      // [T]   group << 32 | node, ascending
    uint32_t* parent = nullptr;   // [T]   node index of the parent; the node itself: root; NONE: the join was dropped
    uint32_t* ptn = nullptr;      // [T]   tree-node index of the parent (NONE: root or none)
    uint32_t* info = nullptr;     // [T]   depth << 8 | OVS_SCRIBE_* flags
    uint32_t* coff = nullptr;     // [T+1] child list offsets
    uint32_t* cidx = nullptr;     // [T]   tree-node indices of the children (E used)
    uint32_t* root_tn = nullptr;  // [G]   tree node of the group's root (parent == itself), NONE without one
    uint32_t* goff = nullptr;     // [G+1] first tree node of each group
    K160* gkeys = nullptr;        // [G]
    uint64_t T = 0, E = 0, G = 0, roots = 0, max_tree = 0;
    int32_t routingType = 0, hopCountMax = 0;   // what the joins were routed under: a publish must match
};

constexpr unsigned long long SCRIBE_ERR_OVERFLOW = 1, SCRIBE_ERR_INPUT = 2;

// frontier item of the dissemination: message, tree node, hops from the root, arrival
struct alignas(8) ScribeItem {
    uint32_t m, tn, hops, pad;
    int64_t t;
};
static_assert(sizeof(ScribeItem) == 24, "ScribeItem is 24 B");

struct ScribeConsts {
    int64_t bwData;      // T(L*8/datarate) of one ScribeDataMessage copy on the wire
    int64_t bwResp;      // ... of the ScribePublishResponse
    int64_t msgDirect;   // 2*T(L*8/datarate) + 2*T(accessDelay) of a PublishCall sent straight to the rendezvous point
    int64_t access2;
    int32_t round;
    uint32_t nnodes;
};

// hash set of (group, node) with tab[hmask + 1] slots (all ones = empty); ctl[0] = tree nodes so far,
// ctl[1] = error bits.  The queue q[0 .. ctl[0]) holds every tree node, level after level.
hipError_t launch_scribe_init(const uint32_t* mgroup, const uint32_t* mnode, uint64_t nm, uint64_t G, uint32_t n,
                              unsigned long long* tab, uint64_t hmask, uint64_t* q, uint64_t cap,
                              unsigned long long* ctl, hipStream_t s);
// one level of joins: the parent of q[lo .. hi) by Chord's findNode, each new (group, parent) claimed once
// and appended.  hopCountMax = 0: every join is discarded at its source; 1: a join is discarded by a first
// hop that is not responsible for the key (sendToKey's hop check precedes forward())
hipError_t launch_scribe_level(const ChordView& V, const K160* gkeys, uint64_t* q, uint32_t* par, uint64_t lo,
                               uint64_t hi, uint64_t cap, unsigned long long* tab, uint64_t hmask,
                               unsigned long long* ctl, int hopCountMax, hipStream_t s);
// the same level on converged Pastry tables: the parent is the pick of the route's source step at the node
// (pastry_source_step), the node itself where it is the sibling for the key
hipError_t launch_scribe_level_pastry(const PastryTables& t, const K160* gkeys, uint64_t* q, uint32_t* par, uint64_t lo,
                                      uint64_t hi, uint64_t cap, unsigned long long* tab, uint64_t hmask,
                                      unsigned long long* ctl, int hopCountMax, int recNumRedundantNodes, hipStream_t s);
// iterative routing: the joins of q[0 .. m0) as a route batch's inputs, and its results as their parents
hipError_t launch_scribe_route_in(const K160* gkeys, const uint64_t* q, uint64_t m0, K160* keys, uint32_t* src,
                                  hipStream_t s);
hipError_t launch_scribe_route_level(const ovs_route_out* route, uint64_t* q, uint32_t* par, uint64_t m0, uint64_t cap,
                                     unsigned long long* tab, uint64_t hmask, unsigned long long* ctl, hipStream_t s);
// sort the T tree nodes, link parents, sort the edges, build the CSR lists, depths, flags, roots.
// work: scratch of scribe_finish_bytes(T) bytes
uint64_t scribe_finish_bytes(uint64_t T);
hipError_t launch_scribe_finish(const uint64_t* q, const uint32_t* par, uint64_t T, uint64_t m0, ScribeForest& F,
                                void* work, hipStream_t s);
hipError_t launch_scribe_export(const ScribeForest& F, ovs_scribe_node* out, hipStream_t s);

// the publish leg's end: status, response time and the level-0 item of every message
hipError_t launch_scribe_publish(const ScribeForest& F, const ScribeConsts& SC, const double2* xy,
                                 const ovs_route_out* route, const uint32_t* mgroup, const uint32_t* msrc,
                                 const uint8_t* mflags, uint64_t nm, ovs_scribe_msg_out* out, ScribeItem* queue,
                                 hipStream_t s);
hipError_t launch_scribe_down(const ScribeForest& F, const ScribeConsts& SC, const double2* xy, ScribeItem* queue,
                              uint64_t lo, uint64_t hi, uint64_t cap, unsigned long long* ctl, hipStream_t s);
// per-message sums and the delivery records of q[0 .. total); dctl[0] = records wanted
hipError_t launch_scribe_collect(const ScribeForest& F, const ScribeItem* queue, uint64_t total,
                                 ovs_scribe_msg_out* out, ovs_scribe_delivery* deliv, uint64_t dcap,
                                 unsigned long long* dctl, hipStream_t s);
// keys[i] = gkeys[group[i]] (a bad group: key 0 and the error bit), for the publish route
hipError_t launch_scribe_msg_keys(const ScribeForest& F, const uint32_t* mgroup, const uint32_t* msrc, uint64_t nm,
                                  uint32_t n, K160* keys, unsigned long long* ctl, hipStream_t s);

}  // namespace ovs
