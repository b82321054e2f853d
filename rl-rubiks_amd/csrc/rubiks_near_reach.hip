// Beyond the near-solved table for MI355X (gfx950): the forward half of a bidirectional search.  Every sequence of j = 0 .. J moves
// from a state is walked and the state it reaches probed in the table of depth K, level by level; the first level with a hit gives
// the exact distance up to K + J and, with the table's optimal tail, an optimal solution (the rule: include/rubiks_hip.h).
//   rc_near_reach_begin:   level 0, one lane per state (rc_near_depth's probe)
//   rc_near_reach_level:   one range of work items of one level; a work item is (state, the first min(level, P) moves)
//   rc_near_reach_finish:  one lane per state: the winning sequence and rc_near_solve's tail behind it
// A lane of k_reach_level keeps the keys of the levels it walks in registers (the walk is a nest of loops, one per remaining move,
// 16 bytes each) and probes the leaves only, kFlight of them at a time: the first reads of the probes go out together (near_home),
// then each is followed to its end (near_finish).  Hits are rare: a lane keeps its smallest word and merges it with one vector
// atomic.  Every loop is bounded by the item's 12^(level - P) leaves and, inside a probe, by the table's size; every cell, meta
// byte and word read from memory is range-checked before it addresses anything: what fails sets RC_NEAR_CORRUPT, never a loop.
#include <algorithm>

#include "rubiks_near.h"

namespace rubiks {

// Probes a lane has in flight at the leaves.  profiles/near_reach_probe.txt compares 1 with 2; 2 is kept.
#ifndef RC_NEAR_REACH_FLIGHT
#define RC_NEAR_REACH_FLIGHT 2
#endif
constexpr int kFlight = RC_NEAR_REACH_FLIGHT;
static_assert(kFlight >= 1 && (int)kA % kFlight == 0, "the twelve children of a node are probed kFlight at a time");

constexpr u64 kNoWord = ~0ull;
constexpr int kDepthShift = 40, kLevelShift = 36;
constexpr u64 kIndexMask = (1ull << kLevelShift) - 1;
constexpr u32 kMaxExtra = RC_NEAR_REACH_MAX_EXTRA;

__host__ __device__ constexpr u64 pow12(u32 e) {
    u64 v = 1;
    for (u32 i = 0; i < e; ++i) v *= 12;
    return v;
}
static_assert(pow12(kMaxExtra) <= kIndexMask, "a sequence's index fits below the level");

__device__ __forceinline__ u64 reach_word(u32 d, u32 level, u64 index) { return (u64)d << kDepthShift | (u64)level << kLevelShift | index; }

// May action a follow p, which followed pp (-1: no such move)?  Not its inverse, not a third equal turn, and not the lower of two
// opposite faces (faces f and f ^ 1) right after the higher.
__device__ __forceinline__ bool reach_follows(int pp, int p, int a) {
    const bool inverse = a == (p ^ 1);
    const bool third = a == p && a == pp;
    const bool swapped = (a >> 1) == ((p >> 1) ^ 1) && (p >> 1) > (a >> 1);
    return !(inverse || third || swapped);
}

struct ReachLane {
    u64 best;
    bool corrupt;
};

// the depth of `key` in the table merged into the lane's word; (h, c): its home cell and what the cell holds
__device__ __forceinline__ void reach_hit(const rc_near_t &t, ReachLane &s, const uint4 &key, u32 h, int c, u32 level, u64 index) {
    const int node = near_finish(t, key, h, c);
    if (node == -1) return;
    const int d = node >= 0 ? near_depth_of(t, node) : -2;
    if (d < 0) {
        s.corrupt = true;
        return;
    }
    const u64 w = reach_word((u32)d, level, index);
    s.best = w < s.best ? w : s.best;
}

// The sequences of R more moves behind `key`, whose last two moves were pp, p and whose index so far is `index`.
template <int R>
__device__ __forceinline__ void reach_walk(const rc_near_t &t, const u8 *lut, ReachLane &s, const uint4 &key, int pp, int p, u64 index, u32 level) {
    if constexpr (R == 0) {
        const u32 h = near_home(t, key);
        reach_hit(t, s, key, h, t.hash[h], level, index);
    } else if constexpr (R == 1) {
#pragma unroll 1
        for (int a0 = 0; a0 < (int)kA; a0 += kFlight) {
            uint4 k[kFlight];
            u32 h[kFlight];
            int c[kFlight];
            bool go[kFlight];
#pragma unroll
            for (int u = 0; u < kFlight; ++u) {
                go[u] = reach_follows(pp, p, a0 + u);
                if (go[u]) {
                    k[u] = key_turned(key, (u32)(a0 + u), lut);
                    h[u] = near_home(t, k[u]);
                    c[u] = t.hash[h[u]];
                }
            }
#pragma unroll
            for (int u = 0; u < kFlight; ++u)
                if (go[u]) reach_hit(t, s, k[u], h[u], c[u], level, index * kA + (u32)(a0 + u));
        }
    } else {
#pragma unroll 1
        for (int a = 0; a < (int)kA; ++a) {
            if (!reach_follows(pp, p, a)) continue;
            reach_walk<R - 1>(t, lut, s, key_turned(key, (u32)a, lut), p, a, index * kA + (u32)a, level);
        }
    }
}

// ---- per state: level 0, the live bytes, the count the host reads ---------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_reach_begin(rc_near_t t, rc_near_reach_t r) {
    if (blockIdx.x == 0 && threadIdx.x == 0) r.status[1] = 0;
    const u8 *soa = reinterpret_cast<const u8 *>(r.soa);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < r.n; i += (size_t)gridDim.x * kBlock) {
        const uint4 key = key_from_column(soa, r.stride, i);
        const int node = near_find(t, key);
        int d = node >= 0 ? near_depth_of(t, node) : -1;
        if (node == -2 || d == -2) {
            r.status[0] = RC_NEAR_CORRUPT;
            d = -1;
        }
        r.best[i] = d >= 0 ? reach_word((u32)d, 0, 0) : kNoWord;
        r.live[i] = d < 0;
    }
}

__global__ __launch_bounds__(kBlock) void k_reach_settle(rc_near_reach_t r, u32 level) {
    if (blockIdx.x == 0 && threadIdx.x == 0) r.status[1] = 0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < r.n; i += (size_t)gridDim.x * kBlock) {
        const u64 w = r.best[i];
        r.live[i] = w == kNoWord || ((w >> kLevelShift) & 15u) == level;
    }
}

__global__ __launch_bounds__(kBlock) void k_reach_count(rc_near_reach_t r) {
    int mine = 0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < r.n; i += (size_t)gridDim.x * kBlock) mine += r.best[i] == kNoWord;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) mine += __shfl_xor(mine, o, kWave);
    if (threadIdx.x % kWave == 0 && mine) atomicAdd(&r.status[1], mine);
}

// ---- one range of a level's work items; R = level - min(level, P) moves are walked behind the item's prefix -------------------------------
template <int R>
__global__ __launch_bounds__(kBlock) void k_reach_level(rc_near_t t, rc_near_reach_t r, u32 level, u64 first, u64 count) {
    __shared__ u32 s_lut[sizeof(kTables.lut) / 4];
    stage_to_lds(s_lut, c_tables.lut, sizeof(kTables.lut));
    __syncthreads();
    const u8 *lut = reinterpret_cast<const u8 *>(s_lut);
    const u8 *soa = reinterpret_cast<const u8 *>(r.soa);
    const u32 pl = level - R;          // the prefix's moves (the host's word: min(level, P))
    const u64 items = pow12(pl);
    bool corrupt = false;
    for (u64 g = (u64)blockIdx.x * kBlock + threadIdx.x; g < count; g += (u64)gridDim.x * kBlock) {
        const u64 w = first + g;       // (< n * items: checked on the host)
        const u64 state = w / items;
        const u64 prefix = w - state * items;
        if (!r.live[state]) continue;
        uint4 key = key_from_column(soa, r.stride, state);
        int pp = -1, p = -1;
        bool go = true;
        u64 rest = prefix, div = items;
        for (u32 m = 0; m < pl && go; ++m) {   // the first move is the most significant digit
            div /= kA;
            const int a = (int)(rest / div);
            rest -= (u64)a * div;
            go = reach_follows(pp, p, a);
            if (go) key = key_turned(key, (u32)a, lut);
            pp = p;
            p = a;
        }
        if (!go) continue;
        ReachLane s{kNoWord, false};
        reach_walk<R>(t, lut, s, key, pp, p, prefix, level);
        corrupt |= s.corrupt;
        if (s.best != kNoWord) atomicMin(reinterpret_cast<unsigned long long *>(r.best) + state, (unsigned long long)s.best);
    }
    if (corrupt) r.status[0] = RC_NEAR_CORRUPT;
}

// ---- the winning sequence and the table's tail behind it ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_reach_finish(rc_near_t t, rc_near_reach_t r) {
    __shared__ u32 s_lut[sizeof(kTables.lut) / 4];
    stage_to_lds(s_lut, c_tables.lut, sizeof(kTables.lut));
    __syncthreads();
    const u8 *lut = reinterpret_cast<const u8 *>(s_lut);
    const u8 *soa = reinterpret_cast<const u8 *>(r.soa);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < r.n; i += (size_t)gridDim.x * kBlock) {
        const u64 w = r.best[i];
        int dist = -1, lev = -1;
        if (w != kNoWord) {
            const u32 d = (u32)(w >> kDepthShift), j = (u32)(w >> kLevelShift) & 15u;
            const u64 index = w & kIndexMask;
            // (out_width >= K + J: checked on the host)
            bool ok = d <= t.depth && j <= r.extra && index < pow12(j);
            if (ok) {
                u8 *row = r.out_queues + i * r.out_width;
                uint4 key = key_from_column(soa, r.stride, i);
                u64 rest = index, div = pow12(j);
                for (u32 m = 0; m < j; ++m) {
                    div /= kA;
                    const u32 a = (u32)(rest / div);
                    rest -= (u64)a * div;
                    row[m] = (u8)a;
                    key = key_turned(key, a, lut);
                }
                const int node = near_find(t, key);
                ok = node >= 0 && near_depth_of(t, node) == (int)d;
                // the tail undoes a_d first: the reverse of a_1 .. a_d with every move inverted (k_near_solve)
                if (ok && d > 0) ok = near_walk_back(t, key, node, (int)d, lut, [&](int s, u32 a) { row[j + s] = (u8)(a ^ 1u); });
            }
            if (ok) {
                dist = (int)(j + d);
                lev = (int)j;
            } else {
                r.status[0] = RC_NEAR_CORRUPT;
            }
        }
        r.dist_out[i] = (int8_t)dist;
        r.level_out[i] = (int8_t)lev;
        r.out_lens[i] = dist;
    }
}

static int check_reach(const rc_near_reach_t *r) {
    RC_REQUIRE(r != nullptr, RC_ERR_NULL);
    RC_CHECK_SOA(r->soa, r->n, r->stride);
    RC_REQUIRE(r->live && r->best && r->dist_out && r->level_out && r->out_queues && r->out_lens && r->status, RC_ERR_NULL);
    RC_REQUIRE((reinterpret_cast<uintptr_t>(r->best) & 7u) == 0 && (reinterpret_cast<uintptr_t>(r->out_lens) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(r->status) & 3u) == 0,
               RC_ERR_ALIGN);
    RC_REQUIRE(r->n >= 1 && r->n < ((size_t)1 << 31), RC_ERR_RANGE);
    RC_REQUIRE(r->extra <= kMaxExtra && r->prefix <= kMaxExtra, RC_ERR_RANGE);
    return RC_OK;
}

template <int R>
static void launch_level(const rc_near_t *t, const rc_near_reach_t *r, u32 level, u64 first, u64 count, hipStream_t st) {
    k_reach_level<R><<<grid_for((size_t)count), kBlock, 0, st>>>(*t, *r, level, first, count);
}

}  // namespace rubiks

using namespace rubiks;

extern "C" {

size_t rc_near_reach_struct_bytes(void) { return sizeof(rc_near_reach_t); }

uint64_t rc_near_reach_items(uint32_t level, uint32_t prefix) {
    if (level > kMaxExtra || prefix > kMaxExtra) return 0;
    return pow12(std::min(level, prefix));
}

// level 0 of the rule: rc_near_depth's probe of the state itself
int rc_near_reach_begin(const rc_near_t *t, const rc_near_reach_t *r, rc_stream_t stream) {
    if (int rc = check_near(t, false)) return rc;
    if (int rc = check_reach(r)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    k_reach_begin<<<grid_for(r->n), kBlock, 0, st>>>(*t, *r);
    k_reach_count<<<grid_for(r->n), kBlock, 0, st>>>(*r);
    return launch_status();
}

int rc_near_reach_level(const rc_near_t *t, const rc_near_reach_t *r, uint32_t level, uint64_t first, uint64_t count, rc_stream_t stream) {
    if (int rc = check_near(t, false)) return rc;
    if (int rc = check_reach(r)) return rc;
    RC_REQUIRE(level >= 1 && level <= r->extra, RC_ERR_RANGE);
    const u64 total = (u64)r->n * rc_near_reach_items(level, r->prefix);   // (n < 2^31, items < 2^36)
    RC_REQUIRE(count >= 1 && first < total && count <= total - first, RC_ERR_RANGE);
    hipStream_t st = static_cast<hipStream_t>(stream);
    k_reach_settle<<<grid_for(r->n), kBlock, 0, st>>>(*r, level);
    switch (level - std::min(level, r->prefix)) {
#define RC_REACH_CASE(R) \
    case R:              \
        launch_level<R>(t, r, level, first, count, st); \
        break;
        RC_REACH_CASE(0) RC_REACH_CASE(1) RC_REACH_CASE(2) RC_REACH_CASE(3) RC_REACH_CASE(4) RC_REACH_CASE(5)
        RC_REACH_CASE(6) RC_REACH_CASE(7) RC_REACH_CASE(8) RC_REACH_CASE(9) RC_REACH_CASE(10)
#undef RC_REACH_CASE
        default: return RC_ERR_RANGE;
    }
    k_reach_count<<<grid_for(r->n), kBlock, 0, st>>>(*r);
    return launch_status();
}

// rc_near_solve's tail behind the winning sequence
int rc_near_reach_finish(const rc_near_t *t, const rc_near_reach_t *r, rc_stream_t stream) {
    if (int rc = check_near(t, false)) return rc;
    if (int rc = check_reach(r)) return rc;
    RC_REQUIRE(r->out_width >= t->depth + r->extra, RC_ERR_RANGE);
    k_reach_finish<<<grid_for(r->n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(*t, *r);
    return launch_status();
}

}  // extern "C"
