// host_checks_driver.cpp -- the entry points' pure refusals (oversim_amd/csrc/host_checks.hpp) on the CPU:
// status and literal message of every case, built by tests/test_sanitizers.py with plain g++ under
// ASan/UBSan.  No HIP compiler, no HIP library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_checks.hpp"

using namespace ovs;

namespace {

int failures = 0;

void expect(bool ok, const char* what, int line)
{
    if (ok) return;
    std::printf("line %d: %s\n", line, what);
    ++failures;
}
#define EXPECT(x) expect((x), #x, __LINE__)

// status and message of one refusal; an accepted check leaves the message alone
bool is(ovs_status got, const std::string& err, ovs_status want, const char* msg)
{
    if (got == want && err == msg) return true;
    std::printf("  got %d \"%s\", want %d \"%s\"\n", (int)got, err.c_str(), (int)want, msg);
    return false;
}

const char* const DECR = "shard_lo must be non-decreasing";
const char* const COVER = "shard_lo must cover [0, n)";
const char* const ARC = "this context's arc is not one of shard_lo's arcs";

struct ArcResult {
    ovs_status st;
    std::string err;
    int me;
    std::vector<uint64_t> bounds;
};

ArcResult arc(std::vector<uint64_t> lo, uint64_t n, uint64_t a, uint64_t b)
{
    ArcResult r{OVS_OK, "untouched", -7, std::vector<uint64_t>(lo.size(), ~0ull)};
    r.st = check_arc_map(lo.data(), (uint32_t)lo.size() - 1, n, a, b, r.bounds.data(), &r.me, &r.err);
    return r;
}

void arc_maps()
{
    const uint64_t n = 1000;
    ArcResult r = arc({0, n}, n, 0, n);                             // one arc
    EXPECT(is(r.st, r.err, OVS_OK, "untouched") && r.me == 0 && r.bounds == (std::vector<uint64_t>{0, n}));
    r = arc({0, 400, n}, n, 0, 400);                                // two arcs, either of them
    EXPECT(is(r.st, r.err, OVS_OK, "untouched") && r.me == 0);
    r = arc({0, 400, n}, n, 400, n);
    EXPECT(is(r.st, r.err, OVS_OK, "untouched") && r.me == 1 && r.bounds == (std::vector<uint64_t>{0, 400, n}));
    std::vector<uint64_t> full(65);                                 // MAXSHARDS = 64 arcs of 10 nodes
    for (int i = 0; i <= 64; ++i) full[i] = 10ull * i;
    r = arc(full, 640, 630, 640);
    EXPECT(is(r.st, r.err, OVS_OK, "untouched") && r.me == 63 && r.bounds == full);
    r = arc(full, 640, 0, 10);
    EXPECT(is(r.st, r.err, OVS_OK, "untouched") && r.me == 0);
    r = arc({0, 0, 300, 300, 700, 700, n, n}, n, 300, 700);         // empty arcs around the context's
    EXPECT(is(r.st, r.err, OVS_OK, "untouched") && r.me == 3);
    r = arc({0, 0, 0, n}, n, 0, n);
    EXPECT(is(r.st, r.err, OVS_OK, "untouched") && r.me == 2);
    // the refusals, in their order: a decreasing bound before the cover, the cover before the arc
    r = arc({0, 700, 300, n}, n, 300, n);
    EXPECT(is(r.st, r.err, OVS_EINVAL, DECR));
    r = arc({5, 700, 300, n + 1}, n, 1, 2);
    EXPECT(is(r.st, r.err, OVS_EINVAL, DECR));
    r = arc({1, 400, n}, n, 400, n);
    EXPECT(is(r.st, r.err, OVS_EINVAL, COVER));
    r = arc({0, 400, n - 1}, n, 0, 400);
    EXPECT(is(r.st, r.err, OVS_EINVAL, COVER));
    r = arc({0, 400, n + 1}, n, 1, 2);
    EXPECT(is(r.st, r.err, OVS_EINVAL, COVER));
    r = arc({0, 400, 600, n}, n, 400, 700);                         // its lo is a bound, its hi is not
    EXPECT(is(r.st, r.err, OVS_EINVAL, ARC) && r.me == -1);
    r = arc({0, 400, 600, n}, n, 300, 600);                         // the other way round
    EXPECT(is(r.st, r.err, OVS_EINVAL, ARC));
    r = arc({0, 400, 600, n}, n, 400, n);                           // both are bounds, of different arcs
    EXPECT(is(r.st, r.err, OVS_EINVAL, ARC));
}

ovs_params kad_params()
{
    ovs_params P;
    std::memset(&P, 0, sizeof P);
    P.overlay = OVS_OVERLAY_KADEMLIA;
    P.k = 8; P.s = 8; P.b = 1; P.bucketType = 0; P.extraNodesFinalBucket = 0;
    P.hopCountMax = 50; P.lookupMerge = 1; P.lookupStrictParallelRpcs = 1; P.lookupParallelRpcs = 3; P.lookupParallelPaths = 1;
    return P;
}

// Kademlia::routingBucketSize, bucketType nr128: limit = (int)log2(extraNodesFinalBucket) (0 stands for the key
// length, 160), offset = limit - (160 - (index + 1)) = limit - 159 + index; the size is 2^offset where offset > 0
// and 2^offset > k, else k.  limit: 160 -> 7, 1 -> 0, 128 -> 7, 511 -> 8.  So with limit 7 index 159 holds
// 2^7 = 128, index 153 2^1 = 2 and index 152 (offset 0) k; with limit 8 they hold 2^8 = 256, 2^2 = 4, 2^1 = 2;
// with limit 0 no offset is positive.  k = 8 hides the sizes up to 8, k = 1 shows them all.
void bucket_sizes()
{
    const int index[4] = {0, 152, 153, 159}, extra[4] = {0, 1, 128, 511};
    const int want_k8[4][4] = {{8, 8, 8, 128}, {8, 8, 8, 8}, {8, 8, 8, 128}, {8, 8, 8, 256}};
    const int want_k1[4][4] = {{1, 1, 2, 128}, {1, 1, 1, 1}, {1, 1, 2, 128}, {1, 2, 4, 256}};
    ovs_params P = kad_params();
    for (int e = 0; e < 4; ++e)
        for (int i = 0; i < 4; ++i) {
            P.extraNodesFinalBucket = extra[e];
            for (const int k : {8, 1}) {
                P.k = k;
                P.bucketType = 0;                                   // kademlia: k everywhere
                EXPECT(kad_bucket_size_host(P, index[i], 160) == k);
                P.bucketType = 1;                                   // nkademlia: no maximum
                EXPECT(kad_bucket_size_host(P, index[i], 160) == 0);
                P.bucketType = 2;
                const int want = k == 8 ? want_k8[e][i] : want_k1[e][i];
                if (kad_bucket_size_host(P, index[i], 160) != want)
                    std::printf("  nr128 extra %d index %d k %d: %d, want %d\n", extra[e], index[i], k,
                                kad_bucket_size_host(P, index[i], 160), want);
                EXPECT(kad_bucket_size_host(P, index[i], 160) == want);
            }
        }
}

const char* const KS_BLOCKS = "Kademlia k must be 1..16 (two 96 B bucket blocks) and 5*s <= 64";
const char* const KS_CSR = "Kademlia k must be 1..16 and 5*s <= 64";
const char* const B1_SNAP = "the snapshot rule builds b = 1 kademlia tables: other b / bucketType through ovs_kad_load_tables_csr";
const char* const B1_KSTRIDE = "k-stride tables hold b = 1 kademlia buckets: other b / bucketType through ovs_kad_load_tables_csr";

struct Shape {
    ovs_status st;
    std::string err;
};

// the loaders as they call the check: the two that take b = 1 kademlia buckets only pass their own sentence
enum class KadLoader { Snapshot, KStride, Csr };

Shape shape(const ovs_params& P, KadLoader how)
{
    Shape r{OVS_OK, "untouched"};
    r.st = check_kad_shape(P, how == KadLoader::Csr ? nullptr : how == KadLoader::Snapshot ? B1_SNAP : B1_KSTRIDE, 16, &r.err);
    return r;
}

void table_shapes()
{
    const KadLoader all[3] = {KadLoader::Snapshot, KadLoader::KStride, KadLoader::Csr};
    for (const KadLoader how : all) {
        const char* ks = how == KadLoader::Csr ? KS_CSR : KS_BLOCKS;
        for (const int k : {0, 1, 16, 17}) {
            ovs_params P = kad_params();
            P.k = k;
            const Shape r = shape(P, how);
            EXPECT(k == 0 || k == 17 ? is(r.st, r.err, OVS_ENOTSUP, ks) : is(r.st, r.err, OVS_OK, "untouched"));
        }
        for (const int s : {0, 12, 13}) {
            ovs_params P = kad_params();
            P.s = s;
            const Shape r = shape(P, how);
            EXPECT(s == 12 ? is(r.st, r.err, OVS_OK, "untouched") : is(r.st, r.err, OVS_ENOTSUP, ks));
        }
        for (const int b : {0, 1, 5, 6}) {
            ovs_params P = kad_params();
            P.b = b;
            const Shape r = shape(P, how);
            if (how == KadLoader::Csr)
                EXPECT(b == 0 || b == 6 ? is(r.st, r.err, OVS_ENOTSUP, "Kademlia b must be 1..5 (numBuckets <= 992)")
                                        : is(r.st, r.err, OVS_OK, "untouched"));
            else
                EXPECT(b == 1 ? is(r.st, r.err, OVS_OK, "untouched")
                              : is(r.st, r.err, OVS_ENOTSUP, how == KadLoader::Snapshot ? B1_SNAP : B1_KSTRIDE));
        }
    }
    ovs_params P = kad_params();
    // the b / bucketType refusal comes before the k / s one
    P.bucketType = 1; P.k = 17;
    Shape r = shape(P, KadLoader::Snapshot);
    EXPECT(is(r.st, r.err, OVS_ENOTSUP, B1_SNAP));
    r = shape(P, KadLoader::KStride);
    EXPECT(is(r.st, r.err, OVS_ENOTSUP, B1_KSTRIDE));
    r = shape(P, KadLoader::Csr);
    EXPECT(is(r.st, r.err, OVS_ENOTSUP, KS_CSR));
    P = kad_params();
    for (const int t : {-1, 3}) {
        P.bucketType = t;
        r = shape(P, KadLoader::Csr);
        EXPECT(is(r.st, r.err, OVS_EINVAL, "bucketType must be 0..2 (kademlia, nkademlia, nr128)"));
    }
    P = kad_params();
    P.bucketType = 2; P.b = 2;
    r = shape(P, KadLoader::Csr);
    EXPECT(is(r.st, r.err, OVS_ENOTSUP, "nr128 buckets need b = 1"));
    P.b = 1;
    for (const int extra : {-1, 0, 511, 512}) {
        P.extraNodesFinalBucket = extra;
        r = shape(P, KadLoader::Csr);
        EXPECT(extra == -1 || extra == 512 ? is(r.st, r.err, OVS_ENOTSUP, "nr128: extraNodesFinalBucket must be 0..511")
                                           : is(r.st, r.err, OVS_OK, "untouched"));
    }
    P.bucketType = 1; P.extraNodesFinalBucket = 512;       // only nr128 reads it
    r = shape(P, KadLoader::Csr);
    EXPECT(is(r.st, r.err, OVS_OK, "untouched"));
}

void bad_codes()
{
    const char* const both[8] = {"", "sibling index out of range or the node itself", "sibling listed twice", nullptr,
                                 "bucket member out of range or the node itself", nullptr, "bucket member listed twice",
                                 "node is both sibling and bucket member"};
    for (uint32_t code = 1; code <= 7; ++code)
        for (const bool csr : {false, true}) {
            const char* want = both[code];
            if (code == 3) want = csr ? "bucket holds more than routingBucketSize(i) entries" : "bucket holds more than k entries";
            if (code == 5)
                want = csr ? "bucket member in the wrong bucket (routingBucketIndex(member) != bucket index)"
                           : "bucket member in the wrong bucket (msb(member ^ node) != bucket index)";
            EXPECT(kad_table_error(csr, 17 + code, code) ==
                   std::string(csr ? "CSR" : "explicit") + " Kademlia tables of node " + std::to_string(17 + code) + ": " + want);
        }
    EXPECT(kad_table_error(false, 3, 8) == "explicit Kademlia tables of node 3: ?");
    EXPECT(kad_table_error(false, 3, 99) == "explicit Kademlia tables of node 3: ?");
    EXPECT(kad_table_error(true, 3, 4000000000u) == "CSR Kademlia tables of node 3: ?");
    EXPECT(kad_table_error(false, 4294967295u, 5) ==
           "explicit Kademlia tables of node 4294967295: bucket member in the wrong bucket (msb(member ^ node) != bucket index)");
    EXPECT(kad_table_error(true, 0, 8) == "CSR Kademlia tables of node 0: ?");
}

void refresh()
{
    const char* const RED = "refresh lookups implement redundantNodes 1..64";
    const char* const HOPS = "refresh lookups need hopCountMax >= 1";
    const char* const MERGE = "refresh lookups implement lookupMerge, strictParallelRpcs, parallelRpcs 1..8";
    const char* const PATHS = "parallelPaths 1, no verify/majority siblings, jitter 0";
    for (const int R : {0, 1, 64, 65}) {
        std::string err = "untouched";
        const ovs_status st = check_refresh_redundant(R, true, &err);
        EXPECT(R == 0 || R == 65 ? is(st, err, OVS_ENOTSUP, RED) : is(st, err, OVS_OK, "untouched"));
        err = "untouched";                                          // a maintenance round's: bounded above only
        const ovs_status up = check_refresh_redundant(R, false, &err);
        EXPECT(R == 65 ? is(up, err, OVS_ENOTSUP, RED) : is(up, err, OVS_OK, "untouched"));
    }
    auto params = [](ovs_params P) {
        Shape r{OVS_OK, "untouched"};
        r.st = check_refresh_params(P, 8, &r.err);
        return r;
    };
    ovs_params P = kad_params();
    Shape r = params(P);
    EXPECT(is(r.st, r.err, OVS_OK, "untouched"));
    P.hopCountMax = 1; P.lookupParallelRpcs = 1;
    r = params(P);
    EXPECT(is(r.st, r.err, OVS_OK, "untouched"));
    P.lookupParallelRpcs = 8;
    r = params(P);
    EXPECT(is(r.st, r.err, OVS_OK, "untouched"));
    P = kad_params(); P.hopCountMax = 0; P.lookupMerge = 0; P.jitter = 0.1;     // the first of the three
    r = params(P);
    EXPECT(is(r.st, r.err, OVS_ENOTSUP, HOPS));
    P = kad_params(); P.lookupMerge = 0; P.lookupParallelPaths = 2;             // the second before the third
    r = params(P);
    EXPECT(is(r.st, r.err, OVS_ENOTSUP, MERGE));
    P = kad_params(); P.lookupStrictParallelRpcs = 0;
    r = params(P);
    EXPECT(is(r.st, r.err, OVS_ENOTSUP, MERGE));
    for (const int alpha : {0, 9}) {
        P = kad_params(); P.lookupParallelRpcs = alpha;
        r = params(P);
        EXPECT(is(r.st, r.err, OVS_ENOTSUP, MERGE));
    }
    P = kad_params(); P.lookupParallelPaths = 2;
    r = params(P);
    EXPECT(is(r.st, r.err, OVS_ENOTSUP, PATHS));
    P = kad_params(); P.lookupVerifySiblings = 1;
    r = params(P);
    EXPECT(is(r.st, r.err, OVS_ENOTSUP, PATHS));
    P = kad_params(); P.lookupMajoritySiblings = 1;
    r = params(P);
    EXPECT(is(r.st, r.err, OVS_ENOTSUP, PATHS));
    P = kad_params(); P.jitter = 0.1;
    r = params(P);
    EXPECT(is(r.st, r.err, OVS_ENOTSUP, PATHS));
}

void node_indices()
{
    const std::vector<uint32_t> node = {0, 9, 3, 10, 4, 4000000000u};
    std::string err = "untouched";
    uint64_t pos = 77;
    EXPECT(is(check_node_indices(node.data(), 3, 10, &err, &pos), err, OVS_OK, "untouched") && pos == 77);
    EXPECT(is(check_node_indices(nullptr, 0, 10, &err, &pos), err, OVS_OK, "untouched"));
    EXPECT(is(check_node_indices(node.data(), node.size(), 10, &err, &pos), err, OVS_EINVAL, "node index out of range") && pos == 3);
    err = "untouched";
    EXPECT(is(check_node_indices(node.data(), node.size(), 11, &err, &pos), err, OVS_EINVAL, "node index out of range") && pos == 5);
    err = "untouched";
    EXPECT(is(check_node_indices(node.data(), node.size(), 0, &err), err, OVS_EINVAL, "node index out of range"));
}

}  // namespace

int main()
{
    arc_maps();
    bucket_sizes();
    table_shapes();
    bad_codes();
    refresh();
    node_indices();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("clean\n");
    return 0;
}
