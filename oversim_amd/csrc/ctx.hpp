// ctx.hpp -- the context and the host helpers its entry points share (internal).
//
// The translation units that implement the C ABI include this: ovs_ctx.cpp (the context, its parameters,
// what every call shares), ovs_load.cpp (loaders, exports, Chord maintenance rounds; ovs_broose.cpp: Broose's, ovs_pastry.cpp: Pastry's),
// ovs_shard.cpp (shard steps), ovs_route.cpp (the route / lookup / findNode seam), ovs_kad_maint.cpp (Kademlia
// refresh and maintenance) and the application tiers app_*.cpp; host_checks.hpp holds the refusals on plain
// values.  The tiers reach the router through route_check / route_device and lookup_check / lookup_device,
// never through the public entry points: one argument check, one hipSetDevice and one CallFrame per call.
// Nothing writes c->P but ovs_set_params and the loaders; a tier that routes under another message length
// passes a copy.  shard_route.cpp drives a context through the public ABI and sees ctx_internal.hpp only.
#pragma once
#include <map>
#include <vector>

#include "broose.hpp"
#include "call_frame.hpp"
#include "ctx_internal.hpp"
#include "dht.hpp"
#include "epichord.hpp"
#include "host_checks.hpp"
#include "host_tables.hpp"
#include "kad.hpp"
#include "kad_shard.hpp"
#include "koorde.hpp"
#include "launch.hpp"
#include "pastry.hpp"
#include "scribe.hpp"

struct ovs_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    ovs_params P{};
    int overlay = 0;          // loaded overlay
    uint64_t n = 0;
    bool ideal = true;
    int num_cu = 0;
    // chord
    ovs::KeyRec* recs = nullptr;
    double2* xy = nullptr;
    ovs::FingerEnt* fingers = nullptr;  // ideal finger rows (64 B entries)
    uint64_t nfing = 0;
    ovs::NodeRec* nodes = nullptr;      // ideal node records + finger entries built for successorListSize = nodes_ns
    ovs::WinRec* win = nullptr;         // ideal successor windows of the arc [shard_lo, shard_hi)
    int nodes_ns = -1;
    uint32_t* pred = nullptr;
    uint32_t* succ = nullptr;
    uint8_t* nsucc = nullptr;
    uint32_t* fres = nullptr;
    int sls = 0;
    // explicit tables: host copies for batched maintenance (ovs_chord_fix_fingers / _stabilize)
    ovs::ChordHost ch;
    // explicit Kademlia tables: host copy for maintenance rounds (ovs_kad_maintenance_round)
    ovs::KadHost kh;
    uint64_t shard_lo = 0, shard_hi = 0;   // finger rows exist for [shard_lo, shard_hi)
    ovs::FingerEnt* ftop = nullptr;         // replicated top finger levels of every node (ovs_chord_shard_replicate)
    int ftl = 0;
    uint64_t* d_bounds = nullptr;           // device copy of the arc boundaries (MAXSHARDS + 1)
    std::vector<uint64_t> h_bounds;         // ... as last uploaded (uploaded again only on a change)
    std::map<hipStream_t, ovs::StageBuf> stage;  // shard-step stage records per stream (cohorts)
    bool bbox_ok = false;                   // the coordinates' bounding box (x0, x1, y0, y1), computed
    double bbox[4] = {0, 0, 0, 0};          // on first use (extendedFingerTable's acceptance rule)
    // kademlia
    ovs::KadTables kad{};
    // koorde (on the sorted ring in recs / xy)
    ovs::KoordeTables koorde{};
    // epichord routing snapshot (ovs_epichord_load)
    ovs::EpiTables epi{};
    // broose buckets and records (ovs_broose_load / _load_tables; on the sorted ids in recs / xy)
    ovs::BrooseTables broose{};
    // pastry leaf sets and routing tables (ovs_pastry_load / _load_tables; on the sorted ids in recs / xy)
    ovs::PastryTables pastry{};
    ovs_pastry_params pastry_bp{};
    bool pastry_rule = false;            // the tables came from the rule (ovs_pastry_load), not from ovs_pastry_load_tables
    ovs::CachedBuf kvis;                 // internal visited lists (K3 without hop_seq, K2x without responders)
    // K1's key-order buffers (ksort.hip): sorted keys, sources, caller indices and the sort's
    // histograms, one allocation shared by the calls on this context like kvis
    ovs::CachedBuf ks;
    ovs::CachedBuf bq;                   // the broadcast's item queue (ovs_chord_broadcast_batch), cached like kvis
    ovs::CachedBuf rpcb;                 // the RPC test's route records and return-route inputs (ovs_rpc_batch)
    ovs::CachedBuf dhtb;                 // the DHT calls' lookup records, sibling rows and pair arrays (ovs_dht_*_batch)
    ovs::DhtStore dht;                   // the DHT data storage (ovs_dht_store_create), dropped with the network
    ovs::ScribeForest scribe;            // the Scribe forest (ovs_scribe_build), dropped with the network
    ovs::CachedBuf scq;                  // the multicast's item queue (ovs_scribe_multicast_batch), cached like bq
    ovs::DynSlots dyn;                   // the persistent route kernels' dynamic-tail counters (dyn_acquire)
    // multi-GPU Kademlia: this rank's in-flight lookups (ovs_kad_shard_begin)
    void* kst = nullptr;                 // KadLookup<alpha> state records
    uint8_t* kact = nullptr;             // 0 never runs, 1 suspended in kst, 2 not started
    ovs::K160* kkeys = nullptr;          // the batch's keys and sources (a lookup starts from them)
    uint32_t* ksrc = nullptr;
    uint32_t* kqids = nullptr;
    void* kres = nullptr;                // alpha findNode result slots per lookup (KadResN<kfcap>)
    unsigned long long* kbad = nullptr;  // undeliverable responses
    uint64_t* kiota = nullptr;           // lookup indices 0..n-1: round 1's list, the source of the next lists
    uint64_t* klist[2] = {nullptr, nullptr};   // ping-pong lists of the still active lookups
    unsigned long long* knl = nullptr;   // [3]: length of iota (round 1), klist[0], klist[1]
    int kcur = 0;                        // list of the next round: 0 = iota, 1/2 = klist[0/1]
    uint64_t knlook = 0, kcap = 0;
    int kalpha = 0;
    int kfcap = 8;                       // findNode capacity of the shard records (8; 16 KademliaLarge)
    int32_t kns = -1;                    // LookupCall batch: numSiblings (-1: KBR routes)
    uint32_t* ksib = nullptr;            // ... and the caller's sibling rows
    // the sharded round loop (shard_route.cpp): cohort streams and cached buffers
    hipStream_t cohort[4] = {nullptr, nullptr, nullptr, nullptr};
    void* route_scratch = nullptr;
    void (*route_scratch_release)(void*) = nullptr;
};

namespace ovs {

// ---- failures as the call's status (fail itself: ctx_internal.hpp) ----
ovs_status hip_fail(ovs_ctx* c, hipError_t e, const char* where);
// a CallFrame's or a cached buffer's failure: OVS_ENOMEM when the device is out of memory
ovs_status device_fail(ovs_ctx* c, hipError_t e, const std::string& what);
ovs_status frame_fail(ovs_ctx* c, const CallFrame& F);
ovs_status lease_fail(ovs_ctx* c, const char* name, const CachedBuf::Lease& L);

#define HIPCHK(c, expr)                                             \
    do {                                                            \
        hipError_t e_ = (expr);                                     \
        if (e_ != hipSuccess) return ovs::hip_fail((c), e_, #expr); \
    } while (0)

// ---- the parameters as the kernels take them ----
// SimTime(double) on the host (identical IEEE double arithmetic to the device path)
int64_t simtime_host(double seconds, int round);
// T(L * 8 / datarate): the serialisation time of an L-byte packet
int64_t bw_host(const ovs_params& P, int32_t bytes);
int32_t route_bytes(const ovs_params& P);
DelayConsts delay_consts(const ovs_params& P);
// the response of a converged n-node ring's LookupCall there and back: min(ns, 1 + successors) NodeHandles
int64_t ring_sibling_response_ns(const DelayConsts& DC, const ovs_params& P, uint64_t n, int ns);
// a zeroed work counter for one launch of a persistent route kernel, or none (static slices only)
DynSlots::Lease dyn_acquire(ovs_ctx* c, uint64_t n, hipStream_t s);

// ---- refusals ----
ovs_status check_common(ovs_ctx* c, const ovs_params& P);
ovs_status check_chord_route(ovs_ctx* c, const ovs_params& P);
// host-pointer calls: every lookup's source must be a node of the network (a source past it would
// be read out of bounds by the lookup kernels); device-pointer calls leave that to the caller (ovs_kbr.h)
ovs_status check_sources(ovs_ctx* c, const uint32_t* src, uint64_t n, bool dev);

// ---- the visited lists of a batch of single-path iterative lookups (ovs_route.cpp) ----
// n lists of H responders on stream s.  Without a hop_seq request (*dhop null) they live in the context's
// cached kvis buffer, unpadded -- the kernels read back only the entries a lookup wrote -- and *dhop becomes
// its pointer; the caller's own list is set to 0xFF.  The caller releases *vis after the launch.
ovs_status visited_lists(ovs_ctx* c, uint32_t** dhop, uint64_t n, uint64_t H, hipStream_t s, CachedBuf::Lease* vis);

// ---- the loaders' common steps ----
// drop the loaded network and everything built on it
void free_tables(ovs_ctx* c);
void free_kad_shard(ovs_ctx* c);
// One load: selects the device, drops the loaded network and the shard state, and refuses a context whose
// params.overlay is not `overlay`.  A loader returns st unless that is OVS_OK, and commit() at its end;
// every other way out drops what the load had built.  Only commit() sets c->overlay.
struct LoadFrame {
    LoadFrame(ovs_ctx* c, int overlay, const char* name);
    ~LoadFrame() { if (live) free_tables(c); }
    ovs_status commit() { c->overlay = overlay; live = false; return OVS_OK; }
    ovs_ctx* c;
    int overlay;
    ovs_status st = OVS_OK;
    bool live = false;      // the device is selected and the load has not committed
};
// sorted ids (+ coordinates) into c->recs / c->xy; OVS_EINVAL unless ascending and unique
ovs_status upload_nodes(ovs_ctx* c, const ovs_key160* ids, uint64_t n, const double* xy, bool dev);
// k-stride Kademlia tables of c->n nodes, on the host, staged and built into T.  *staged = false: no staging
// buffers; hipErrorInvalidValue with bad[1] set: code bad[1] at node bad[0].  What either means is the caller's.
hipError_t kad_build_from_host(ovs_ctx* c, const uint32_t* siblings, const uint8_t* bucket_count,
                               const uint32_t* bucket_nodes, KadTables& T, bool* staged, uint32_t bad[2]);

// ---- the loaded ring ----
// NodeRec array of an ideal ring for the context's successorListSize (rebuilt when it changes)
ovs_status ensure_nodes(ovs_ctx* c, hipStream_t s);
ChordView chord_view(const ovs_ctx* c);

// ---- the route seam ----
// P is the context's parameters, or a copy that differs in what one call sets (the message length, the
// number of siblings); the tables (ensure_nodes, chord_view) always follow the context's.
//
// route_check: every refusal of a one-way route that does not depend on the batch, in ovs_route_batch's
// order; selects the device and brings an ideal ring's node records up to date on s.
ovs_status route_check(ovs_ctx* c, const ovs_params& P, hipStream_t s);
// route_device: n > 0 routes on device pointers, queued on s, after route_check and check_sources.
// dhop: the caller's hop rows (n * max(hopCountMax, 1)) or nullptr, drpc: its RPC counts or nullptr;
// F is the call's frame (exhaustive-iterative Kademlia takes a temporary from it).
ovs_status route_device(ovs_ctx* c, const ovs_params& P, CallFrame& F, const K160* dk, const uint32_t* ds, uint64_t n,
                        ovs_route_out* dout, uint32_t* dhop, uint32_t* drpc, hipStream_t s);
// route_device's counterpart on a Pastry context (ovs_pastry.cpp): n > 0 semi-recursive routes on device
// pointers, queued on s, after check_common, pastry_route_refusal (pastry_acked_refusal) and check_sources.
// AC: the routes run under routeMsgAcks with these constants; dack: ack records (empty ones without AC) or nullptr
ovs_status pastry_route_device(ovs_ctx* c, const ovs_params& P, const K160* dk, const uint32_t* ds, uint64_t n, ovs_route_out* dout,
                               uint32_t* dhop, hipStream_t s, const PastryAckConsts* AC = nullptr,
                               ovs_pastry_ack_out* dack = nullptr);
// The same for LookupCalls.  lookup_check resolves num_siblings (< 0: the overlay's maximum) into *ns;
// dsib has max(ns, 1) entries per lookup.
ovs_status lookup_check(ovs_ctx* c, const ovs_params& P, int32_t num_siblings, hipStream_t s, int32_t* ns);
ovs_status lookup_device(ovs_ctx* c, const ovs_params& P, int32_t ns, const K160* dk, const uint32_t* ds, uint64_t n,
                         ovs_route_out* dout, uint32_t* dsib, hipStream_t s);
// The iterative LookupCall on a Pastry context (ovs_pastry.cpp), for ovs_pastry_lookup_batch and the DHT tier.
// pastry_lookup_check: pastry_iterative_refusal, check_common, num_siblings (< 0: numberOfLeaves / 2; 0 and more
// than that refused) into *ns, the device selected.  route: the one-way message's refusals too (routeMsgAcks,
// numSiblings); name: the entry point a num_siblings = 0 refusal names.
ovs_status pastry_lookup_check(ovs_ctx* c, const ovs_params& P, int32_t num_siblings, int32_t* ns, bool route = false,
                               const char* name = "ovs_pastry_lookup_batch");
// pastry_lookup_device: n > 0 lookups on device pointers, queued on s, after pastry_lookup_check and
// check_sources; dsib has ns entries per lookup.  The visited lists come from the cached kvis buffer unless the
// caller brings dhop (n * hopCountMax); drout instead of dlook: the one-way route (ns = 1); drpc: RPC counts;
// DC: the delay constants where they differ from the lookup's own (the acked route's final message).
ovs_status pastry_lookup_device(ovs_ctx* c, const ovs_params& P, int32_t ns, const K160* dk, const uint32_t* ds, uint64_t n,
                                ovs_lookup_out* dlook, uint32_t* dsib, hipStream_t s, ovs_route_out* drout = nullptr,
                                uint32_t* dhop = nullptr, uint32_t* drpc = nullptr, const DelayConsts* DC = nullptr);

// ---- read-backs ----
// the control words of a frontier loop (queue length, error bits, ...), read after the launches queued on s
inline hipError_t read_ctl(unsigned long long* h, const unsigned long long* ctl, int words, hipStream_t s)
{
    const hipError_t e = hipMemcpyAsync(h, ctl, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, s);
    return e == hipSuccess ? hipStreamSynchronize(s) : e;
}

// What the statistics calls (ovs_kbrtest_*_stats_batch, ovs_dhttest_stats_batch) share.  stats_begin: the
// refusals that do not depend on the records, the device, the pointer mode and the stream.
// stats_read: after the launch (its error in `launched`), the kernel's sums and its second result (per-node
// counters or reductions) read back; it synchronises s in both pointer modes: the results are host values.
ovs_status stats_begin(ovs_ctx* c, double measured_time_s, double failure_latency_s, uint32_t flags, void* stream,
                       bool* dev, hipStream_t* s);
ovs_status stats_read(ovs_ctx* c, hipStream_t s, hipError_t launched, void* sums, const void* dsums, size_t sums_bytes,
                      void* rows, const void* drows, size_t rows_bytes, const char* what);
// rows * c->n zeroed host counters for stats_read
ovs_status node_counters(ovs_ctx* c, int rows, std::vector<uint32_t>& nc);

}  // namespace ovs
