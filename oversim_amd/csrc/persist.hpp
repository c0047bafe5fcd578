// persist.hpp -- the persistent-slice scheduler shared by the lane-refill route kernels: K1
// (k_chord_lanes, chord.hip), K2 (k_kad_route, kad_route.hip), K2x (k_kad_refresh, kad_refresh.hip),
// K3 (k_koorde_route, koorde.hip), K4 (k_broose_route, broose.hip) and the Pastry kernels
// (k_pastry_route<ACKS>: plain routes and routes under routeMsgAcks; k_pastry_iter; pastry.hip).
//
// Each launches an occupancy-sized persistent grid and gives every wave one contiguous static slice
// of the batch; a lane whose lookup ended takes the wave's next one by ballot + popcount (the
// refill).  Persistent waves finish their static slices up to a quarter of the
// kernel apart (the tail census below), so with a zeroed per-launch counter (PersistDyn) the static
// slices cover only a share of the batch and the rest goes out in chunks of a few lookups, one atomic
// a chunk: the waves that run ahead take more (the dynamic tail).  The share and the chunk are
// per-kernel tunables (PersistTune), kept next to their kernels.
//
// The plan (persist_plan) is plain C++: it compiles without a HIP compiler
// (tests/persist_plan_driver.cpp).  The occupancy query, the refill and the tail census need one
// (__HIPCC__).  On the device the refill is stated once, PersistFeed<CH>::take: K4 and the Pastry
// kernels, which are untuned, run it.  K1, K2, K2x and K3 keep cursor / end / more / lt_mask as
// locals of their own loops and share only the claim of the next dynamic chunk, persist_claim_chunk:
// as members of a shared object these compiled to different register allocations (K1's shard step
// +18 spilled SGPRs, K2 and K2x a few spilled VGPRs more or fewer; K3: see koorde.hip), and these
// kernels sit at their occupancy limits.
#pragma once

#include <cstdint>
#include <cstdlib>

namespace ovs {

// OVS_NO_DYN=1 (A/B and the dynamic-tail tests): static slices only.  Read per call, here only:
// the callers pass the decision down (no counter / dyn_tail = false)
inline bool persist_dyn_enabled() { return std::getenv("OVS_NO_DYN") == nullptr; }

struct PersistTune {
    double static_share;   // the share of a batch the static slices cover when the tail is on
    uint32_t dyn_chunk;    // lookups per dynamic chunk
};

struct PersistPlan {
    uint64_t chunk;        // lookups of each wave's static slice: wave w owns [w * chunk, (w + 1) * chunk)
    uint64_t blocks;       // 256-thread blocks (4 waves) to launch
    uint64_t dyn_from;     // the static slices end here (cut at n); [dyn_from, n) goes out in chunks
    bool dyn;              // the dynamic tail is on (dyn_from < n, the counter is used)
};

// n > 0 lookups over `waves` resident waves (blocks per CU x CUs x 4).  Static: slices of
// ceil(n / waves), and only the blocks whose waves have one are launched; whole_grid (K2x, whose grid
// is its lane-capped scratch: waves = lanes / 64, a multiple of 4) launches every wave.  With a
// counter the static slices shrink to static_share of the batch, unless a slice would then be shorter
// than one dynamic chunk (small batches stay static).
inline PersistPlan persist_plan(uint64_t n, uint64_t waves, bool counter, PersistTune t, bool whole_grid = false)
{
    PersistPlan p{};
    p.chunk = (n + waves - 1) / waves;
    if (p.chunk < 1) p.chunk = 1;
    const uint64_t used = whole_grid ? waves : (n + p.chunk - 1) / p.chunk;
    p.blocks = (used + 3) / 4;
    p.dyn_from = n;
    const uint64_t grid = p.blocks * 4;
    const uint64_t cs = (uint64_t)((double)n * t.static_share) / grid;
    if (counter && cs >= (uint64_t)t.dyn_chunk) {
        p.chunk = cs;
        p.dyn_from = cs * grid;
        p.dyn = true;
    }
    return p;
}

}  // namespace ovs

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

namespace ovs {

// A kernel instantiation as a type, so that a launch ladder chooses it once (a generic lambda takes
// PersistKernel<k<...>>{} and has the kernel as the constant K::fn for the occupancy and the launch)
template <auto Kernel>
struct PersistKernel {
    static constexpr auto fn = Kernel;
};

// resident 256-thread blocks per CU of a kernel instantiation (the same on every gfx950 device; a
// function-local static is initialised once, thread-safely)
template <auto Kernel>
int persist_blocks_per_cu()
{
    static const int bpc = [] {
        int b = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, Kernel, 256, 0) != hipSuccess || b < 1) b = 1;
        return b;
    }();
    return bpc;
}

// the resident waves of a kernel instantiation's occupancy-sized grid (4 waves per block)
template <auto Kernel>
uint64_t persist_waves(int num_cu)
{
    return (uint64_t)num_cu * (uint64_t)persist_blocks_per_cu<Kernel>() * 4;
}

// The claim of a wave's next dynamic chunk: lane 0 adds CH to the launch's counter (one atomic a
// chunk), and the chunk's first lookup, dyn_from + the counter's old value, comes back wave-uniform.
// The caller, a wave whose slice is spent, takes [nb, min(nb + CH, n)) when nb < n; otherwise the
// batch is handed out.  It returns a value only, so nothing new is live across a kernel's loop
template <uint32_t CH>
__device__ __forceinline__ uint64_t persist_claim_chunk(unsigned long long* ctr, uint64_t dyn_from, int lane)
{
    unsigned long long b = 0;
    if (lane == 0) b = atomicAdd(ctr, (unsigned long long)CH);
    return dyn_from + (((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) << 32) |
                       (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)b));
}

// the per-launch counter of the dynamic tail: static slices cover [0, from), the rest goes out a chunk
// at a time from the zeroed counter *ctr (nullptr: static slices only)
struct PersistDyn {
    unsigned long long* ctr;
    uint64_t from;
};

// What a launcher whose grid is the kernel's occupancy hands to hipLaunchKernelGGL (K3, K4, the Pastry
// kernels): the plan of nq lookups over the instantiation's resident waves, with the dynamic tail
// where the caller brings a zeroed counter and the plan uses it
struct PersistLaunch {
    unsigned blocks;
    uint64_t chunk;
    PersistDyn dy;
};
template <auto Kernel>
PersistLaunch persist_launch(uint64_t nq, int num_cu, unsigned long long* dyn, PersistTune t)
{
    const PersistPlan pl = persist_plan(nq, persist_waves<Kernel>(num_cu), dyn != nullptr, t);
    return {(unsigned)pl.blocks, pl.chunk, PersistDyn{pl.dyn ? dyn : nullptr, pl.dyn_from}};
}

// A wave's feed of lookups: its static slice [wave * chunk, (wave + 1) * chunk) cut at the end of the
// static region, then dynamic chunks of CH lookups while the batch lasts.  A kernel's loop head reads
//     if (feed.take(active, dy, nq, q)) { active = true; /* the kernel's own per-lookup init */ }
//     if (!__any(active)) break;
//     if (!active) continue;
template <uint32_t CH>
struct PersistFeed {
    uint64_t cursor, end;
    bool more;                 // dynamic chunks may be left
    uint64_t lt_mask;          // the lanes below this one

    __device__ __forceinline__ PersistFeed(uint64_t chunk, const PersistDyn& dy, uint64_t nq)
    {
        const int lane = threadIdx.x & 63;
        const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        cursor = wave * chunk;
        end = min(cursor + chunk, dy.ctr ? dy.from : nq);
        more = dy.ctr != nullptr;
        lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    }

    // Wave-uniform call.  The idle lanes (ballot) take the next lookups of the slice in lane order; a
    // spent slice is first replaced by a new dynamic chunk.  True where this lane was idle and now has
    // lookup q.
    __device__ __forceinline__ bool take(bool active, const PersistDyn& dy, uint64_t nq, uint64_t& q)
    {
        const uint64_t need = __ballot(!active);
        if (more && need != 0 && cursor >= end) {
            const uint64_t nb = persist_claim_chunk<CH>(dy.ctr, dy.from, threadIdx.x & 63);
            if (nb < nq) {
                cursor = nb;
                end = min(nb + (uint64_t)CH, nq);
            } else {
                more = false;
            }
        }
        bool taken = false;
        if (need != 0 && cursor < end) {
            const uint64_t mine = cursor + (uint64_t)__popcll(need & lt_mask);
            if (!active && mine < end) {
                q = mine;
                taken = true;
            }
            cursor += (uint64_t)__popcll(need);
        }
        return taken;
    }
};

// tail census (-DOVS_K1_TAIL / -DOVS_KAD_TAIL builds): each persistent wave's exit on the 100 MHz
// real-time clock, so the spread of the waves' finishing times (the kernel's tail) can be read off
// one launch
constexpr int PERSIST_TAIL_MAX = 1 << 16;
// lane 0 of the wave records the real-time counter in slot 2 * wave + which; the slot comes from
// wave-uniform values, so nothing stays live across the kernel's loop (a first version that kept the
// wave index and the start time live spilled the kernel)
__device__ __forceinline__ void ovs_tail_mark(unsigned long long* arr, int max, int which)
{
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x) >> 6;
    const uint64_t w = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wib;
    const unsigned long long t = wall_clock64();
    if (__lane_id() == 0 && w < (uint64_t)max) arr[2 * w + which] = t;
}
// the census array `sym` (a __device__ array of 2 * PERSIST_TAIL_MAX) read back after the launch on
// s: the waves' exit times as percentiles after the first exit
inline void persist_tail_report(const char* tag, const void* sym, uint64_t waves, uint64_t chunk, hipStream_t s)
{
    const uint64_t nw = waves < (uint64_t)PERSIST_TAIL_MAX ? waves : (uint64_t)PERSIST_TAIL_MAX;
    std::vector<unsigned long long> tt(2 * nw);
    hipMemcpyFromSymbolAsync(tt.data(), sym, sizeof(unsigned long long) * 2 * nw, 0, hipMemcpyDeviceToHost, s);
    hipStreamSynchronize(s);
    unsigned long long t0 = ~0ull;
    std::vector<double> fin;
    for (uint64_t w = 0; w < nw; ++w) t0 = tt[2 * w + 1] < t0 ? tt[2 * w + 1] : t0;
    for (uint64_t w = 0; w < nw; ++w) fin.push_back((double)(tt[2 * w + 1] - t0) * 0.01);   // 100 MHz -> us
    std::sort(fin.begin(), fin.end());
    auto pct = [&](double f) { return fin[(size_t)(f * (fin.size() - 1))]; };
    fprintf(stderr, "%s waves=%llu chunk=%llu finish_us_after_first_exit p0=%.1f p10=%.1f p50=%.1f p90=%.1f p99=%.1f max=%.1f\n",
            tag, (unsigned long long)nw, (unsigned long long)chunk, pct(0), pct(0.1), pct(0.5), pct(0.9), pct(0.99),
            fin.back());
}

}  // namespace ovs
#endif
