// dht.hpp -- DHT tier: the replica phase of batched puts and gets and the device-resident storage (internal).
#pragma once
#include "engine.hpp"

namespace ovs {

constexpr int DHT_MAXR = 8;          // numReplica, numGetRequests <= 8

// one slot of the open-addressing table (96 B); tag 0 = never claimed
struct DhtSlot {
    unsigned long long tag;          // 64-bit mix of (node, key, kind, id), never 0
    unsigned long long arb_t;        // put arbitration within a batch: max(arrival + 1), 0 between batches
    unsigned long long arb_op;       // ... then max(operation + 1) among the puts of that arrival
    uint32_t key[5];
    uint32_t kind, id, node;
    unsigned long long token;
    long long expiry;                // INT64_MAX: never
    uint32_t vlen;                   // 0: no entry (deleted, or claimed and never written)
    uint32_t ins_batch;              // insertion order: (batch, arrival, operation) of the put that wrote it
    uint32_t ins_op;
    uint32_t pad;
    long long ins_t;
};
static_assert(sizeof(DhtSlot) == 96, "DhtSlot is 96 B");

struct DhtHeader {
    unsigned long long used;         // claimed slots
    unsigned long long used_prev;    // ... at the start of the running put batch
    unsigned long long need;         // the running put batch's count of pairs without a slot
    unsigned long long refused;      // put batches that did not fit
    unsigned long long last_refused; // the last put batch: 1 = it did not fit
    unsigned long long collisions;   // two different entries with one tag (2^-64 per pair): the later one is dropped
    unsigned long long batch;        // put batches so far
    unsigned long long coll_prev;    // collisions at the start of the last put batch
    unsigned long long last_collisions;   // ... and those of the last put batch alone
    unsigned long long team_overrun;      // replica-team operations whose replay ran out of its event bound (a defect)
};

struct DhtStore {
    DhtSlot* slots = nullptr;
    DhtHeader* hdr = nullptr;
    uint64_t cap = 0;
};

// per-launch constants of the replica phase (host: ovs_dht_put_batch / ovs_dht_get_batch)
struct DhtConsts {
    int64_t timeout;     // T(rpcUdpTimeout): a response at or after it is a timeout
    int64_t access;      // T(accessDelay)
    double datarate;
    double ratio;        // ratioIdentical
    int32_t round;
    int32_t auth;        // AUTHBLOCK_L in bits: 800 with measureAuthBlock, else 0
    int32_t R;           // numReplica = the sibling rows' stride
    int32_t G;           // numGetRequests
    uint32_t nnodes;
};

// put: records, each (operation, replica) pair's arrival (-1: none) and the count of pairs without a slot
hipError_t launch_dht_put_plan(const DhtStore& st, const DhtConsts& C, const ovs_lookup_out* look, const uint32_t* sib,
                               const K160* keys, const uint32_t* src, const ovs_dht_op* ops, const double2* xy, uint64_t n,
                               ovs_dht_put_out* out, long long* pair_t, int num_cu, hipStream_t s);
// put: claim, arbitrate, write, reset and close the batch (five launches; nothing happens when it does not fit)
hipError_t launch_dht_put_apply(const DhtStore& st, const DhtConsts& C, const uint32_t* sib, const K160* keys,
                                const ovs_dht_op* ops, uint64_t n, const long long* pair_t, uint32_t* pair_slot, int num_cu,
                                hipStream_t s);
hipError_t launch_dht_get(const DhtStore& st, const DhtConsts& C, const ovs_lookup_out* look, const uint32_t* sib,
                          const K160* keys, const uint32_t* src, const ovs_dht_op* ops, const double2* xy, uint64_t n,
                          ovs_dht_get_out* out, hipStream_t s);

// device-side integer sums of the DHTTestApp statistics
struct DhtStatsDev {
    unsigned long long put_ok, put_err, get_ok, get_err;
    unsigned long long put_lat, put_sq_lo, put_sq_hi, get_lat, get_sq_lo, get_sq_hi, get_lat_n;
    unsigned long long put_min, put_max, get_min, get_max;
    unsigned long long put_hop_n, put_hop, get_hop_n, get_hop, msgs, bytes;
};
// node_counts: 4 * nnodes u32 (put success, put error, get success, get error per node), zeroed here
hipError_t launch_dhttest_stats(const ovs_dht_put_out* put_out, const uint32_t* put_src, uint64_t n_put,
                                const ovs_dht_get_out* get_out, const ovs_dht_op* get_ops, const uint32_t* get_src,
                                const ovs_dhttest_expect* expect, uint64_t n_get, uint32_t nnodes, DhtStatsDev* S,
                                uint32_t* node_counts, int num_cu, hipStream_t s);

}  // namespace ovs
