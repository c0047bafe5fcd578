// Stand-alone driver for Pastry's host-only logic, built with -fsanitize=address,undefined by
// tests/test_pastry_model.py: the parameter refusals and the validation of explicit tables
// (oversim_amd/csrc/pastry_host.hpp), the leaf-set replay of small networks, and the ini reader
// (oversim_amd/csrc/ovs_ini.cpp, compiled into this program).  Prints the replayed leaf sets for the test to
// compare with the model, then "ok".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pastry_host.hpp"

using namespace ovs;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

static K160 key(uint32_t top, uint32_t low)
{
    K160 k{};
    k.w[4] = top; k.w[0] = low;
    return k;
}

int main()
{
    // key arithmetic
    CHECK(p_spl_bits(key(0x80000000u, 0), key(0, 0)) == 0);
    CHECK(p_spl_bits(key(1, 0), key(1, 1)) == 159);
    CHECK(p_spl_digits(key(1, 0), key(1, 0), 4) == 160);
    CHECK(p_digit(key(0xA5000000u, 0), 0, 4) == 0xA && p_digit(key(0xA5000000u, 0), 1, 4) == 5);
    CHECK(p_digit(key(0xA5000000u, 0), 0, 3) == 5 && p_digit(key(0, 7), 52, 3) == 3);
    CHECK(k_eq(p_ring_dist(key(0, 1), key(0xFFFFFFFFu, 0)), p_ring_dist(key(0xFFFFFFFFu, 0), key(0, 1))));

    // refusals
    ovs_pastry_params bp{4, 16, 0, 0, 1, 0};
    ovs_params P;
    std::memset(&P, 0, sizeof P);
    P.routingType = 1; P.numSiblings = 1; P.recNumRedundantNodes = 3;
    CHECK(pastry_route_refusal(P, bp) == nullptr);
    for (int rt : {0, 2, 3, 4, 7}) { P.routingType = rt; CHECK(pastry_route_refusal(P, bp) != nullptr); }
    P.routingType = 1;
    bp.routeMsgAcks = 1;
    CHECK(std::string(pastry_route_refusal(P, bp)).find("routeMsgAcks") != std::string::npos);
    bp.routeMsgAcks = 0;
    for (int r : {0, 9}) { P.recNumRedundantNodes = r; CHECK(pastry_route_refusal(P, bp) != nullptr); }
    P.recNumRedundantNodes = 8;
    CHECK(pastry_route_refusal(P, bp) == nullptr);
    P.numSiblings = 2;
    CHECK(pastry_route_refusal(P, bp) != nullptr);
    P.numSiblings = 1;
    for (int b : {0, 5}) { bp.bitsPerDigit = b; CHECK(pastry_shape_refusal(bp) != nullptr && pastry_route_refusal(P, bp) != nullptr); }
    bp.bitsPerDigit = 4;
    for (int L : {0, 7, 34}) { bp.numberOfLeaves = L; CHECK(pastry_shape_refusal(bp) != nullptr); }
    bp.numberOfLeaves = 32;
    CHECK(pastry_shape_refusal(bp) == nullptr);
    bp.numberOfNeighbors = 1;
    CHECK(pastry_shape_refusal(bp) != nullptr);

    // explicit tables of four nodes, b = 2, L = 2, three rows
    const K160 ids[4] = {key(0x10000000u, 0), key(0x50000000u, 0), key(0x58000000u, 0), key(0xD0000000u, 0)};
    PastryShape sh;
    sh.b = 2; sh.L = 2;
    std::vector<uint32_t> leaf = {3, 1, 0, 2, 1, 3, 2, 0};
    std::vector<uint32_t> tab(4 * 3 * 4, PASTRY_NONE);
    tab[(0 * 3 + 0) * 4 + 1] = 1;        // node 0 row 0 column 1: 0x5...
    tab[(1 * 3 + 0) * 4 + 3] = 3;
    tab[(1 * 3 + 2) * 4 + 2] = 2;        // 0x50 and 0x58 share two digits; 0x58 has digit 2 next
    std::string err;
    CHECK(pastry_validate_tables(ids, 4, sh, 3, leaf.data(), tab.data(), &err));
    CHECK(!pastry_validate_tables(ids, 4, sh, 0, leaf.data(), tab.data(), &err));
    CHECK(!pastry_validate_tables(ids, 4, sh, 81, leaf.data(), tab.data(), &err));
    auto bad_tab = tab;
    bad_tab[(0 * 3 + 0) * 4 + 1] = 4;
    CHECK(!pastry_validate_tables(ids, 4, sh, 3, leaf.data(), bad_tab.data(), &err) && err.find("node 0") != std::string::npos);
    bad_tab = tab;
    bad_tab[(0 * 3 + 0) * 4 + 2] = 1;    // wrong column
    CHECK(!pastry_validate_tables(ids, 4, sh, 3, leaf.data(), bad_tab.data(), &err));
    bad_tab = tab;
    bad_tab[(1 * 3 + 0) * 4 + 1] = 2;    // shares two digits, not none
    CHECK(!pastry_validate_tables(ids, 4, sh, 3, leaf.data(), bad_tab.data(), &err));
    bad_tab = tab;
    bad_tab[(2 * 3 + 2) * 4 + 2] = 2;    // its owner
    CHECK(!pastry_validate_tables(ids, 4, sh, 3, leaf.data(), bad_tab.data(), &err));
    for (auto edit : {std::pair<int, uint32_t>{0, 0u}, {1, 3u}, {2, 9u}}) {
        auto bad_leaf = leaf;
        bad_leaf[(size_t)edit.first] = edit.second;   // the owner, a node twice, out of range
        CHECK(!pastry_validate_tables(ids, 4, sh, 3, bad_leaf.data(), tab.data(), &err));
    }
    auto none_leaf = leaf;
    none_leaf[0] = none_leaf[1] = PASTRY_NONE;
    CHECK(!pastry_validate_tables(ids, 4, sh, 3, none_leaf.data(), tab.data(), &err) && err.find("empty") != std::string::npos);

    // the ini reader
    char e[256];
    ovs_pastry_params ip{4, 16, 0, 0, 1, 1};
    const char* ini = "[General]\n**.overlay*.pastry.bitsPerDigit = 2\n**.overlay*.pastry.routeMsgAcks = false\n"
                      "[Config A]\n**.overlay*.pastry.numberOfLeaves = 8\n**.overlay*.pastry.useRegularNextHop = false\n"
                      "[Config B]\n**.overlay*.pastry.routingType = \"iterative\"\n"
                      "[Config C]\n**.overlay*.pastry.useDiscovery = true\n"
                      "[Config D]\n**.overlay*.pastry.bitsPerDigit = four\n"
                      "[Config E]\n**.overlay*.pastry.proximityNeighborSelection = false\n**.overlay*.pastry.routingType = \"semi-recursive\"\n";
    CHECK(ovs_pastry_params_from_ini(&ip, ini, "A", e, sizeof e) == OVS_OK);
    CHECK(ip.bitsPerDigit == 2 && ip.numberOfLeaves == 8 && ip.useRegularNextHop == 0 && ip.routeMsgAcks == 0);
    CHECK(ovs_pastry_params_from_ini(&ip, ini, "B", e, sizeof e) == OVS_ENOTSUP && std::strstr(e, "routingType"));
    CHECK(ovs_pastry_params_from_ini(&ip, ini, "C", e, sizeof e) == OVS_ENOTSUP && std::strstr(e, "useDiscovery"));
    CHECK(ovs_pastry_params_from_ini(&ip, ini, "D", e, sizeof e) == OVS_EINVAL);
    CHECK(ovs_pastry_params_from_ini(&ip, ini, "E", e, sizeof e) == OVS_OK);
    CHECK(ovs_pastry_params_from_ini(&ip, ini, "nope", e, sizeof e) == OVS_EINVAL);
    CHECK(ovs_pastry_params_from_ini(nullptr, ini, nullptr, e, 4) == OVS_EINVAL);

    // the leaf sets of small networks: ids 3 * j + 1 in the top word, every owner
    for (int n : {2, 3, 5, 9}) {
        std::vector<K160> ring;
        for (int j = 0; j < n; ++j) ring.push_back(key(0x01000000u * (uint32_t)(3 * j + 1), (uint32_t)j));
        for (int L : {2, 8, 16}) {
            if (n - 1 >= L) continue;
            for (int v = 0; v < n; ++v) {
                std::vector<uint32_t> out((size_t)L);
                pastry_host_leaves(ring.data(), (uint32_t)n, L, (uint32_t)v, out.data());
                std::printf("leaves %d %d %d:", n, L, v);
                for (uint32_t x : out) std::printf(" %d", x == PASTRY_NONE ? -1 : (int)x);
                std::printf("\n");
            }
        }
    }
    // key arithmetic for the test to redo in Python ints: borrows and carries through equal or saturated middle
    // words, shared prefixes that end in every word, every digit of every digit size (b = 3: the digits that
    // straddle bits 31/32, 63/64, 95/96, 127/128)
    const uint32_t F = 0xFFFFFFFFu;
    const uint32_t ks[][5] = {{0, 0, 0, 0, 0}, {1, 0, 0, 0, 0}, {F, F, 0, 0, 0}, {0, 0, 1, 0, 0}, {F, F, F, F, 0}, {0, 0, 0, 0, 1},
                              {F, F, F, F, F}, {0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u},
                              {0x12345678u, 0xABCDEF89u, 0x0D159E00u, 0x2000u, 0x048D159Cu}, {0x9ABCDEF0u, 0xABCDEF89u, 0x0D159E00u, 0x2000u, 0x048D159Cu},
                              {5, 0, 0x80000000u, 0, 0}, {9, 0, 0x80000000u, 0, 0x80000000u}, {0x80000001u, 3, 0, 0x80000000u, 1}};
    const int nk = (int)(sizeof ks / sizeof ks[0]);
    auto hex = [](const K160& k) { std::printf(" %08x%08x%08x%08x%08x", k.w[4], k.w[3], k.w[2], k.w[1], k.w[0]); };
    for (int i = 0; i < nk; ++i) {
        K160 a;
        std::memcpy(a.w, ks[i], sizeof a.w);
        for (int b = 1; b <= 4; ++b) {
            std::printf("digits %d", b);
            hex(a);
            for (int n = 0; n < 160 / b; ++n) std::printf(" %u", p_digit(a, n, b));
            std::printf("\n");
        }
        for (int j = 0; j < nk; ++j) {
            K160 c;
            std::memcpy(c.w, ks[j], sizeof c.w);
            std::printf("arith");
            hex(a); hex(c); hex(k_sub(a, c)); hex(k_add(a, c)); hex(p_ring_dist(a, c));
            std::printf(" %d %d\n", i == j ? 160 : p_spl_bits(a, c), k_lt(a, c) ? 1 : 0);
        }
    }
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
