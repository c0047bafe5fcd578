// broose.hpp -- Broose (src/overlay/broose/Broose.cc, BrooseBucket.cc) with fixed tables: device
// tables and launchers (internal).
//
// A Broose node keeps 2^shiftingBits + 2 buckets (Broose.cc:158-164), each the maxSize nodes it has
// seen that are XOR-closest to one bucket key (BrooseBucket::add, BrooseBucket.cc:70-115), ordered by
// that distance: rBucket[i] (key (self >> sb) + (i << (160 - sb)), rBucketSize entries), lBucket (key
// self << sb, 2^sb * rBucketSize entries) and bBucket (key self, 7 * bucketSize entries).  The node's
// own handle is fed through add like any other (changeState(READY), 233-239): it always sits in its
// bBucket (distance 0) and in another bucket only where it is among that bucket's closest.
//
// Device layout.  rows: every node owns `stride` 24 B entries (node key + node index; index NONE =
// empty slot), its buckets at fixed places -- rBucket[i] at i * rBucketSize, lBucket at P * rBucketSize,
// bBucket at 2 * P * rBucketSize -- so a hop knows the row's address from the responder's index alone
// and reads the row and the record together.  The entries carry the ids: a scan of up to 56 entries
// reads one contiguous run (at most 1344 B) and no dependent gather of 56 scattered id lines; the price
// is 24 B instead of 4 B an entry (2880 B a node at the defaults).  rec: one 64 B line per node with what
// findNode needs without touching a row.
#pragma once
#include "broose_host.hpp"
#include "engine.hpp"

namespace ovs {

struct alignas(64) BrooseRec {
    uint32_t w[5];       // node key
    uint8_t lp0, lp1;    // rBucket[0] / rBucket[1] ->longestPrefix() (BrooseBucket.cc:202-209)
    uint8_t bmode;       // bBucket->keyInRange (239-260): 0 compare with bd, 1 true (size <= maxSize/7), 2 false (empty)
    uint8_t pad0;
    uint32_t bd[5];      // bBucket getDist(maxSize/7 - 1)
    uint32_t pad1;
    double x, y;
};
static_assert(sizeof(BrooseRec) == 64, "BrooseRec is one 64 B line");

// BrooseFindNodeExtMessage (BrooseMessage.msg): mirrors ovs_broose_ext
struct BExt {
    K160 rk;
    int32_t step;
    uint8_t has;         // 0: the call carries no extension yet
    uint8_t right;       // rightShifting
    uint8_t pad[2];
    uint32_t last;       // lastNode
};
static_assert(sizeof(BExt) == 32, "BExt is 32 B");

struct BrooseTables {
    BrooseRec* rec = nullptr;
    KeyRec* rows = nullptr;
    uint32_t n = 0;
    BrooseShape sh{};
};

void broose_free(BrooseTables& t);
// the ideal snapshot: every bucket holds the maxSize nodes of the network XOR-closest to its key
hipError_t broose_build(const KeyRec* recs, const double2* xy, uint32_t n, const BrooseShape& sh, BrooseTables& t, hipStream_t st);
// explicit buckets in CSR form (device copies; validated on the host by broose_validate_tables)
hipError_t broose_build_from_csr(const KeyRec* recs, const double2* xy, uint32_t n, const BrooseShape& sh, const uint64_t* doff,
                                 const uint32_t* dnodes, BrooseTables& t, hipStream_t st);
// node indices of every row slot (n * stride, NONE = empty), for the export
hipError_t broose_row_nodes(const BrooseTables& t, uint32_t* dout, hipStream_t st);
// Broose::findNode at node[i] for keys[i]: ext[i] in / out, right[i] the direction of an extension created
// there; out_nodes[i * max_out ..] the answer (count[i] nodes), sib[i] isSiblingFor, status[i] 1 where the
// reference errors or is undefined
hipError_t broose_find_node(const BrooseTables& t, const uint32_t* node, const K160* keys, BExt* ext, const uint8_t* right,
                            uint64_t nq, int numRedundantNodes, int numSiblings, uint32_t* out_nodes, uint32_t max_out,
                            uint8_t* count, uint8_t* sib, uint8_t* status, hipStream_t st);
// batched one-way lookups (KBRTestApp -> IterativeLookup with Broose::findNode); hopseq (nq * hopCountMax)
// is required: it is also the lookup's visited list
hipError_t broose_route(const BrooseTables& t, const DelayConsts& DC, int hopCountMax, const K160* keys, const uint32_t* src,
                        const uint8_t* right, uint64_t nq, ovs_route_out* out, uint32_t* hopseq, uint32_t* rpcs, int num_cu,
                        hipStream_t st, unsigned long long* dyn = nullptr);

}  // namespace ovs
