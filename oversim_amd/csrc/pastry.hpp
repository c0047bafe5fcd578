// pastry.hpp -- Pastry (src/overlay/pastry/BasePastry.cc, PastryLeafSet.cc, PastryRoutingTable.cc) with fixed
// tables: device tables and launchers (internal).
//
// Device layout.  rec: one 64 B line per node (key, the number of its routing-table rows up to the last
// non-empty one, coordinates).  leaf: numberOfLeaves 24 B slots per node (node key + node index, index NONE =
// unspecified) in the reference's slot order, so a hop reads the whole leaf set as one contiguous run of at most
// 768 B.  tab: rows x 2^bitsPerDigit such slots per node; a hop addresses the slot (shared digits, next digit)
// directly and scans rows only for numRedundantNodes > 1 and for the closer-node fallback.  The slots carry
// the ids: no scan gathers id lines scattered over the node array.
#pragma once
#include "engine.hpp"
#include "pastry_host.hpp"

namespace ovs {

struct alignas(64) PastryRec {
    uint32_t w[5];       // node key
    uint32_t nrows;      // routing-table rows up to the last non-empty one
    uint32_t pad0[2];
    double x, y;
    uint32_t pad1[4];
};
static_assert(sizeof(PastryRec) == 64, "PastryRec is one 64 B line");

struct PastryTables {
    PastryRec* rec = nullptr;
    KeyRec* leaf = nullptr;
    KeyRec* tab = nullptr;
    uint32_t n = 0;
    int rows = 0;        // routing-table rows stored per node
    PastryShape sh{};
};

// Per-launch constants of routes under routeMsgAcks (host: pastry_ack_consts, ovs_pastry.cpp), beside DelayConsts.
// NextHopCall = BASECALL_L 256 bits around the route message, NextHopResponse = BASERESPONSE_L 256 bits + AUTHBLOCK_L
// (CommonMessages.msg:69-73, 88-89), each with the 28 B UDP/IP header.
struct PastryAckConsts {
    int64_t msgCall;     // 2*T(L*8/datarate) + 2*T(accessDelay) of the NextHopCall
    int64_t bwAck;       // T(L*8/datarate) of the NextHopResponse: what a forwarder's queue holds ahead of its call
    int64_t msgAck;      // 2*bwAck + 2*T(accessDelay): the ack's way back
    int64_t timeout;     // T(rpcUdpTimeout): an ack round trip >= timeout is a timeout
};

void pastry_free(PastryTables& t);
// the converged tables by the rule; n - 1 >= numberOfLeaves (smaller networks: the host replays
// the leaf sets and calls pastry_build_explicit with dtab = nullptr)
hipError_t pastry_build(const KeyRec* recs, const double2* xy, uint32_t n, const PastryShape& sh, PastryTables& t, hipStream_t st);
// explicit node indices (device copies, validated on the host); dtab nullptr: the table by the rule
hipError_t pastry_build_explicit(const KeyRec* recs, const double2* xy, uint32_t n, const PastryShape& sh, int rows,
                                 const uint32_t* dleaf, const uint32_t* dtab, PastryTables& t, hipStream_t st);
// the largest row count the rule gives a node of the sorted ids (reads back: synchronises st)
hipError_t pastry_rule_rows(const KeyRec* recs, uint32_t n, int b, int* rows, hipStream_t st);
// node indices of every slot: dleaf[n * L], dtab[n * rows * 2^b]
hipError_t pastry_slot_nodes(const PastryTables& t, uint32_t* dleaf, uint32_t* dtab, hipStream_t st);
hipError_t pastry_find_node(const PastryTables& t, const uint32_t* node, const K160* keys, uint64_t nq, int numRedundantNodes,
                            int numSiblings, uint32_t* out_nodes, uint32_t max_out, uint8_t* count, uint8_t* sib,
                            uint8_t* status, hipStream_t st);
// batched semi-recursive one-way routes (k_pastry_route<ACKS>); hopseq (nq * max(hopCountMax, 1), preset to NONE) or
// nullptr.  AC nullptr: plain routes, and ack_out must be nullptr too; else the same routes under routeMsgAcks, with
// their ack records where ack_out is given
hipError_t pastry_route(const PastryTables& t, const DelayConsts& DC, const PastryAckConsts* AC, int hopCountMax,
                        int recNumRedundantNodes, const K160* keys, const uint32_t* src, uint64_t nq, ovs_route_out* out,
                        ovs_pastry_ack_out* ack_out, uint32_t* hopseq, int num_cu, hipStream_t st, unsigned long long* dyn = nullptr);
// ack records of routes that sent no NextHopCall (routeMsgAcks = false)
hipError_t pastry_acks_none(uint64_t nq, ovs_pastry_ack_out* ack_out, hipStream_t st);
// ack records of pastry_iter's one-way routes: one NextHopCall src -> rout.responsible where the two differ
hipError_t pastry_iter_acks(const ovs_route_out* rout, const uint32_t* src, const double2* xy, uint32_t n, const PastryAckConsts& AC,
                            int round, uint64_t nq, ovs_pastry_ack_out* ack_out, hipStream_t st);
// batched iterative lookups (k_pastry_iter): LookupCalls with numSiblings 1..numberOfLeaves/2 into lout and
// siblings (nq * numSiblings, may be nullptr), or one-way routes (numSiblings 1) into rout -- one of the two.
// hopseq (nq * hopCountMax, hopCountMax >= 1) is required: it is the visited list; rpcs may be nullptr.  DC
// carries the call and response lengths with the PastryFindNodeExtData object.
hipError_t pastry_iter(const PastryTables& t, const DelayConsts& DC, int hopCountMax, int numSiblings, const K160* keys,
                       const uint32_t* src, uint64_t nq, ovs_route_out* rout, ovs_lookup_out* lout, uint32_t* siblings,
                       uint32_t* hopseq, uint32_t* rpcs, int num_cu, hipStream_t st, unsigned long long* dyn = nullptr);

}  // namespace ovs
