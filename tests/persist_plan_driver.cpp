// persist_plan_driver.cpp -- the host plan of the persistent-slice scheduler (oversim_amd/csrc/persist.hpp,
// persist_plan) under ASan/UBSan (tests/test_sanitizers.py).  Plain C++: no HIP compiler, no HIP library.
//
// For every batch size, resident-wave count and kernel (K1, K2, K3 with the resident waves as their
// grid; K2x with its lane-capped grid), with and without a counter:
//   * the static slices and the dynamic region partition [0, n) exactly, and the launched blocks
//     cover the slices (and no block is launched without one, except in K2x's whole grid);
//   * the tail is off exactly when there is no counter or a static slice would be shorter than one
//     dynamic chunk;
//   * a replay of the waves taking lookups from their slices and claiming dynamic chunks from the
//     counter, in a pseudo-random interleaving, visits every index once;
// and per kernel a few (n, waves) cases give the literal values worked out by hand from the formulas
// the kernels' launchers used before they shared this header (quoted below by file and line of
// commit 83c17b0).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "persist.hpp"

using ovs::PersistPlan;
using ovs::PersistTune;

namespace {

int g_bad = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } \
    } while (0)

// the kernels' tunables, restated (chord.hip K1_TUNE, kad_route.hip KAD_TUNE, kad_refresh.hip KX_TUNE,
// koorde.hip K3_TUNE)
constexpr PersistTune K1{0.70, 64}, K2{0.70, 32}, KX{0.40, 16}, K3{0.70, 64};

// K2x's grid: the resident lanes, capped by the batch, in whole 256-lane blocks; as waves
uint64_t kx_grid_waves(uint64_t n, uint64_t resident_waves)
{
    uint64_t lanes = resident_waves * 64;
    if (lanes > n) lanes = n;
    lanes = (lanes + 255) / 256 * 256;
    return lanes / 64;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return g_rng >> 33;
}

void check_plan(uint64_t n, uint64_t waves, bool counter, PersistTune t, bool whole_grid)
{
    const PersistPlan p = ovs::persist_plan(n, waves, counter, t, whole_grid);
    const uint64_t grid = p.blocks * 4;
    const uint64_t lim = p.dyn_from;       // the static slices' end
    CHECK(p.chunk >= 1 && p.blocks >= 1);
    // the tail: only with a counter, and only when a static slice holds at least one dynamic chunk.
    // (This states the rule as the launchers did, so it pins the plan's consistency with its own
    // block count; the independent evidence for the rule's numbers is literals() below.)
    const uint64_t cs = (uint64_t)((double)n * t.static_share) / grid;
    CHECK(p.dyn == (counter && cs >= t.dyn_chunk));
    if (p.dyn) {
        CHECK(p.chunk == cs && p.chunk >= t.dyn_chunk);
        CHECK(p.dyn_from == p.chunk * grid && p.dyn_from < n);      // every static slice is full
    } else {
        CHECK(p.dyn_from == n);
        if (counter) CHECK(cs < t.dyn_chunk);
    }
    // the blocks cover the static slices; none is launched without a slice (K2x launches its whole grid)
    CHECK(grid * p.chunk >= lim);
    if (whole_grid) CHECK(grid == waves);
    else CHECK((grid - 4) * p.chunk < lim && grid <= (waves + 3) / 4 * 4);

    // replay: wave w starts on [w * chunk, min(w * chunk + chunk, lim)); a wave whose slice is spent
    // claims the next dyn_chunk lookups from the counter while the tail is on (the kernels' refill)
    std::vector<uint8_t> seen(n, 0);
    uint64_t visits = 0, ctr = 0;
    struct Wave { uint64_t cursor, end; bool more; };
    std::vector<Wave> w(grid);
    std::vector<uint32_t> live(grid);
    for (uint64_t i = 0; i < grid; ++i) {
        const uint64_t c = i * p.chunk;
        const uint64_t e = c + p.chunk < lim ? c + p.chunk : lim;
        w[i] = Wave{c, e, p.dyn};
        live[i] = (uint32_t)i;
        if (i > 0 && w[i - 1].end < lim) CHECK(w[i - 1].end == c);       // contiguous slices
    }
    while (!live.empty()) {
        const size_t li = (size_t)(rnd() % live.size());
        Wave& s = w[live[li]];
        const uint64_t need = 1 + rnd() % 64;                            // idle lanes of this refill
        if (s.more && s.cursor >= s.end) {
            const uint64_t nb = p.dyn_from + ctr;
            ctr += t.dyn_chunk;
            if (nb < n) {
                s.cursor = nb;
                s.end = nb + t.dyn_chunk < n ? nb + t.dyn_chunk : n;
            } else {
                s.more = false;
            }
        }
        if (s.cursor < s.end) {
            for (uint64_t r = 0; r < need; ++r) {
                const uint64_t mine = s.cursor + r;
                if (mine < s.end) { CHECK(mine < n && seen[mine] == 0); if (mine < n) seen[mine] = 1; ++visits; }
            }
            s.cursor += need;
        }
        if (s.cursor >= s.end && !s.more) { live[li] = live.back(); live.pop_back(); }
    }
    CHECK(visits == n);
    uint64_t got = 0;
    for (uint64_t i = 0; i < n; ++i) got += seen[i];
    CHECK(got == n);
}

void expect(const PersistPlan& p, uint64_t chunk, uint64_t blocks, uint64_t dyn_from, bool dyn)
{
    CHECK(p.chunk == chunk);
    CHECK(p.blocks == blocks);
    CHECK(p.dyn_from == dyn_from);
    CHECK(p.dyn == dyn);
}

void literals()
{
    // K1, chord.hip:1263-1267 (chunk = ceil(n / waves), >= 1; blocks = ceil(ceil(n / chunk) / 4)) and
    // 1280-1286 (cs = floor(floor(n * 0.70) / (4 blocks)); cs < 64: static; else chunk = cs,
    // dyn_from = cs * 4 blocks).  5120 waves = 256 CUs x 5 blocks x 4:
    //   n = 2^18: chunk 52, ceil(262144 / 52) = 5042 waves, 1261 blocks; cs = 183500 / 5044 = 36 < 64
    expect(ovs::persist_plan(262144, 5120, true, K1), 52, 1261, 262144, false);
    //   n = 786469: chunk 154, 5107 waves, 1277 blocks; cs = 550528 / 5108 = 107; 107 * 5108 = 546556
    expect(ovs::persist_plan(786469, 5120, true, K1), 107, 1277, 546556, true);
    //   n = 10^7: chunk 1954, 5118 waves, 1280 blocks; cs = 7000000 / 5120 = 1367; 1367 * 5120 = 6999040
    expect(ovs::persist_plan(10000000, 5120, true, K1), 1367, 1280, 6999040, true);
    //   n = 65 on 4 waves: chunk 17, 4 waves, 1 block; cs = 45 / 4 = 11 < 64
    expect(ovs::persist_plan(65, 4, true, K1), 17, 1, 65, false);
    //   the rule's boundary on 4 waves (1 block): the tail needs floor(0.70 n) / 4 >= 64, i.e. floor(0.70 n) >= 256.
    //   n = 365: floor(255.5) = 255, cs = 63: off, chunk ceil(365 / 4) = 92
    expect(ovs::persist_plan(365, 4, true, K1), 92, 1, 365, false);
    //   n = 366: floor(256.2) = 256, cs = 64: on, chunk 64, dyn_from 256; without a counter off, chunk 92
    expect(ovs::persist_plan(366, 4, true, K1), 64, 1, 256, true);
    expect(ovs::persist_plan(366, 4, false, K1), 92, 1, 366, false);

    // K2, kad_route.hip:561-565 (the same static arithmetic) and 566-575 (cs against 32).
    // 3072 waves = 256 CUs x 3 blocks x 4:
    //   n = 2^18: chunk 86, 3049 waves, 763 blocks; cs = 183500 / 3052 = 60 >= 32; 60 * 3052 = 183120
    expect(ovs::persist_plan(262144, 3072, true, K2), 60, 763, 183120, true);
    //   n = 63: chunk 1, 63 waves, 16 blocks; cs = 44 / 64 = 0
    expect(ovs::persist_plan(63, 3072, true, K2), 1, 16, 63, false);
    //   n = 786469 without a counter (io.dyn == nullptr): chunk 257, 3061 waves, 766 blocks
    expect(ovs::persist_plan(786469, 3072, false, K2), 257, 766, 786469, false);

    // K3, koorde.hip:680-693 (the slices lambda: the same arithmetic, cs against 64).  4096 waves:
    //   n = 786469: chunk 193, 4075 waves, 1019 blocks; cs = 550528 / 4076 = 135; 135 * 4076 = 550260
    expect(ovs::persist_plan(786469, 4096, true, K3), 135, 1019, 550260, true);
    //   n = 1 on 8192 waves: chunk max(ceil(1 / 8192), 1) = 1, 1 wave, 1 block; cs = 0
    expect(ovs::persist_plan(1, 8192, true, K3), 1, 1, 1, false);

    // K2x, kad_refresh.hip:989-991 (lanes = min(resident lanes, nq), up to a multiple of 256) and
    // 1013-1026 (blocks = lanes / 256, waves = lanes / 64, chunk = ceil(nq / waves);
    // cs = floor(floor(nq * 0.40) / waves) against 16, dyn_from = cs * waves):
    //   nq = 4101, 3072 resident waves: 4352 lanes, 17 blocks, 68 waves; cs = 1640 / 68 = 24; 24 * 68 = 1632
    CHECK(kx_grid_waves(4101, 3072) == 68);
    expect(ovs::persist_plan(4101, 68, true, KX, true), 24, 17, 1632, true);
    //   nq = 10^7, 8192 resident waves: 2048 blocks; cs = 4000000 / 8192 = 488; 488 * 8192 = 3997696
    CHECK(kx_grid_waves(10000000, 8192) == 8192);
    expect(ovs::persist_plan(10000000, 8192, true, KX, true), 488, 2048, 3997696, true);
    //   nq = 2^18 + 37, 3072 resident waves: all 768 blocks (the other kernels would launch 763);
    //   cs = 104872 / 3072 = 34; 34 * 3072 = 104448.  Static (OVS_NO_DYN): chunk ceil(262181 / 3072) = 86
    expect(ovs::persist_plan(262181, 3072, true, KX, true), 34, 768, 104448, true);
    expect(ovs::persist_plan(262181, 3072, false, KX, true), 86, 768, 262181, false);
    //   nq = 64, 4 resident waves: 256 lanes, 1 block, 4 waves, chunk 16; cs = 25 / 4 = 6 < 16
    CHECK(kx_grid_waves(64, 4) == 4);
    expect(ovs::persist_plan(64, 4, true, KX, true), 16, 1, 64, false);
}

}  // namespace

int main()
{
    const uint64_t ns[] = {1, 63, 64, 65, 1ull << 18, (1ull << 18) + 37, 786469, 10000000};
    const uint64_t ws[] = {4, 3072, 5120, 8192};
    for (uint64_t n : ns)
        for (uint64_t w : ws)
            for (int counter = 0; counter < 2; ++counter) {
                check_plan(n, w, counter != 0, K1, false);
                check_plan(n, w, counter != 0, K2, false);
                check_plan(n, w, counter != 0, K3, false);
                check_plan(n, kx_grid_waves(n, w), counter != 0, KX, true);
            }
    literals();
    if (g_bad) { std::printf("%d checks failed\n", g_bad); return 1; }
    std::printf("clean\n");
    return 0;
}
