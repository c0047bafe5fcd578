// Stand-alone driver for the host-side validation of explicit Broose tables (broose_validate_tables in
// oversim_amd/csrc/broose_host.hpp: what ovs_broose_load_tables runs before it uploads anything), built
// without a HIP compiler under -fsanitize=address,undefined (tests/test_broose_model.py).  Each malformed
// CSR input must be refused -- the loader turns the refusal into OVS_EINVAL -- and nothing read out of bounds.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "broose_host.hpp"
#include "ovs_kbr.h"

using namespace ovs;

static int fails = 0;

// the loader's mapping: a refused table is OVS_EINVAL
static ovs_status load_status(const std::vector<K160>& ids, const BrooseShape& sh, const std::vector<uint64_t>& off,
                              const std::vector<uint32_t>& nodes, std::string* err)
{
    return broose_validate_tables(ids.data(), ids.size(), sh, off.data(), nodes.data(), err) ? OVS_OK : OVS_EINVAL;
}

static void expect(const char* what, ovs_status got, ovs_status want, const std::string& err)
{
    if (got != want) {
        std::printf("FAIL %s: status %d, want %d (%s)\n", what, (int)got, (int)want, err.c_str());
        ++fails;
    }
}

int main()
{
    BrooseShape sh;               // the defaults: rows of 8 x 4, 32, 56
    std::string err;
    if (!broose_shape_ok(sh, &err) || sh.nrows() != 6 || sh.stride() != 120u || sh.cap(4) != 32 || sh.cap(5) != 56) {
        std::printf("FAIL shape\n");
        return 1;
    }
    BrooseShape bad = sh;
    bad.sb = 5;
    if (broose_shape_ok(bad, &err)) { std::printf("FAIL shape sb=5 accepted\n"); return 1; }

    // 12 nodes, ids spread over the key space
    const uint64_t n = 12;
    std::vector<K160> ids(n);
    for (uint64_t i = 0; i < n; ++i) {
        ids[i].w[0] = (uint32_t)(i * 2654435761u); ids[i].w[1] = 7; ids[i].w[2] = (uint32_t)i; ids[i].w[3] = 0;
        ids[i].w[4] = (uint32_t)(i * 0x15000000u + 0x01000000u);
    }
    // the ideal tables by brute force
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> nodes;
    for (uint64_t v = 0; v < n; ++v)
        for (int r = 0; r < sh.nrows(); ++r) {
            const K160 bk = broose_bucket_key(sh, ids[v], r);
            std::vector<uint32_t> all(n);
            for (uint32_t j = 0; j < n; ++j) all[j] = j;
            std::sort(all.begin(), all.end(), [&](uint32_t a, uint32_t b) { return k_lt(k_xor(bk, ids[a]), k_xor(bk, ids[b])); });
            all.resize(std::min<size_t>(all.size(), (size_t)sh.cap(r)));
            nodes.insert(nodes.end(), all.begin(), all.end());
            off.push_back(nodes.size());
        }
    expect("ideal tables", load_status(ids, sh, off, nodes, &err), OVS_OK, err);
    {   // empty rows are a legal table
        std::vector<uint64_t> z(off.size(), 0);
        std::vector<uint32_t> none(1, 0);
        expect("empty tables", load_status(ids, sh, z, none, &err), OVS_OK, err);
    }
    {   // an unsorted row
        std::vector<uint32_t> m = nodes;
        std::swap(m[off[3]], m[off[3] + 1]);
        expect("unsorted row", load_status(ids, sh, off, m, &err), OVS_EINVAL, err);
    }
    {   // a node twice
        std::vector<uint32_t> m = nodes;
        m[off[5] + 1] = m[off[5]];
        expect("node twice", load_status(ids, sh, off, m, &err), OVS_EINVAL, err);
    }
    {   // an index >= n
        std::vector<uint32_t> m = nodes;
        m[off[7]] = (uint32_t)n;
        expect("index == n", load_status(ids, sh, off, m, &err), OVS_EINVAL, err);
        m[off[7]] = 0xFFFFFFFFu;
        expect("index 0xFFFFFFFF", load_status(ids, sh, off, m, &err), OVS_EINVAL, err);
    }
    {   // a row longer than maxSize: rBucket[0] of node 0 given 9 members (its neighbours keep theirs)
        std::vector<uint64_t> o = off;
        std::vector<uint32_t> m = nodes;
        m.insert(m.begin() + (long)off[1], 0u);
        for (size_t i = 1; i < o.size(); ++i) o[i] += 1;
        expect("row longer than maxSize", load_status(ids, sh, o, m, &err), OVS_EINVAL, err);
    }
    {   // offsets that decrease
        std::vector<uint64_t> o = off;
        o[4] = o[3] - 1;
        expect("offsets decrease", load_status(ids, sh, o, nodes, &err), OVS_EINVAL, err);
        o = off;
        o[0] = 1;
        expect("row_off[0] != 0", load_status(ids, sh, o, nodes, &err), OVS_EINVAL, err);
    }
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
