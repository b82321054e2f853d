// The near-solved table for MI355X (gfx950): every state within K quarter turns of the solved cube, with its exact depth and the
// move that discovered it, and what it answers -- the distance of a state (rc_near_depth), an optimal solution of a near state
// (rc_near_solve), and the tightening of action queues (rc_near_tighten_*): every stretch of a queue whose product lies in the
// table is replaced by that product's optimal sequence, chosen by a dynamic programme over the queue (include/rubiks_hip.h).
//   rc_near_begin / rc_near_expand:  breadth-first search from the solved state, numbered as rubiks_bfs.hip numbers nodes
//   rc_near_depth, rc_near_solve:    one lane per state
//   rc_near_tighten_distances:       d(i, j) = depth of q[i] .. q[j-1] applied to solved, one lane per start i
//   rc_near_tighten_route:           best[j] over the band, one wave per game, and the chosen segments written out
// The table's cells are those of rubiks_keys.h (0 = free, c > 0 = node c - 1, c < 0 = a pending row while a chunk is filled).  Launch
// boundaries are the only synchronisation between workgroups, except the atomics on the cells while a chunk claims them.  Every
// probe is bounded by the table's size and every cell, meta byte, length and offset read from memory is range-checked before it
// addresses anything: what fails a check ends in RC_NEAR_CORRUPT / RC_NEAR_T_FAILED, never in a loop.
#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "rubiks_near.h"

namespace rubiks {

constexpr int kNone = 0xFF;      // band byte: the product is not in the table
constexpr int kStarts = 2;       // starts a lane of the distance pass advances at once: two probes in flight
constexpr int kRouteBlock = kWave;

// (lookups: near_home / near_finish / near_find / near_depth_of / near_walk_back and check_near are rubiks_near.h's)

// ---- build: rubiks_bfs.hip's chunk, without target and cut, the node count kept on the device ------------------------------------------
// words: [0] nodes stored, [1] 1 = a new state found no node row (capacity too small), [2] new rows of the last chunk
__global__ void k_near_begin(rc_near_t t) {
    constexpr uint4 key = solved_key();
    reinterpret_cast<uint4 *>(t.keys)[0] = key;
    t.meta[0] = 0;
    t.hash[key_hash(key) & (t.hash_size - 1)] = 1;
    t.words[0] = 1;
    t.words[1] = 0;
    t.words[2] = 0;
}

__global__ __launch_bounds__(kBlock) void k_near_children(rc_near_t t, u32 lo, u32 rows) {
    __shared__ u32 s_lut[sizeof(kTables.lut) / 4];
    stage_to_lds(s_lut, c_tables.lut, sizeof(kTables.lut));
    __syncthreads();
    const u8 *lut = reinterpret_cast<const u8 *>(s_lut);
    const uint4 *keys = reinterpret_cast<const uint4 *>(t.keys);
    uint4 *child_keys = reinterpret_cast<uint4 *>(t.child_keys);
    const u32 mask = t.hash_size - 1;
    const u32 stored = t.words[0];
    for (u32 r = blockIdx.x * kBlock + threadIdx.x; r < rows; r += gridDim.x * kBlock) {
        const uint4 ck = key_turned(keys[lo + r / kA], r % kA, lut);
        child_keys[r] = ck;
        // (as key_find, bounded: the cells hold nothing but free cells and nodes between two chunks)
        u32 h = key_hash(ck) & mask;
        int slot_or_node = 1;   // a cell that is no node, or no free cell: the row is dropped as if seen
        for (u32 probes = 0; probes <= mask; ++probes) {
            const int c = t.hash[h];
            if (c == 0) {
                slot_or_node = -(int)h - 1;
                break;
            }
            if (c < 0 || (u32)c > stored) {
                t.words[1] = 1;
                break;
            }
            if (key_eq(keys[c - 1], ck)) break;
            h = (h + 1) & mask;
        }
        t.child_slot[r] = slot_or_node;
    }
}

__global__ __launch_bounds__(kBlock) void k_near_claim(rc_near_t t, u32 rows) {
    const uint4 *child_keys = reinterpret_cast<const uint4 *>(t.child_keys);
    const u32 mask = t.hash_size - 1;
    for (u32 r = blockIdx.x * kBlock + threadIdx.x; r < rows; r += gridDim.x * kBlock) {
        const int cs = t.child_slot[r];
        if (cs >= 0) continue;
        const u32 h = claim_lowest_row(t.hash, (u32)(-cs - 1), mask, -(int)(r + 1), rows, child_keys, child_keys[r]);
        t.child_slot[r] = -(int)h - 1;
    }
}

__global__ __launch_bounds__(kBlock) void k_near_flags(rc_near_t t, u32 rows) {
    for (u32 r = blockIdx.x * kBlock + threadIdx.x; r < rows; r += gridDim.x * kBlock) {
        const int cs = t.child_slot[r];
        t.flags[r] = (cs < 0 && __hip_atomic_load(&t.hash[-cs - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == -(int)(r + 1)) ? 1u : 0u;
    }
}

// appends the chunk's new states in row order; a state without a node row frees its cell again
__global__ __launch_bounds__(kBlock) void k_near_commit(rc_near_t t, u32 rows, u32 level) {
    uint4 *keys = reinterpret_cast<uint4 *>(t.keys);
    const uint4 *child_keys = reinterpret_cast<const uint4 *>(t.child_keys);
    const u32 stored = t.words[0];
    for (u32 r = blockIdx.x * kBlock + threadIdx.x; r < rows; r += gridDim.x * kBlock) {
        if (!t.flags[r]) continue;
        const unsigned long long idx = (unsigned long long)stored + t.prefix[r];
        if (idx >= t.capacity) {
            t.hash[-t.child_slot[r] - 1] = 0;
            t.words[1] = 1;
            continue;
        }
        keys[idx] = child_keys[r];
        t.meta[idx] = (u8)(level << 4 | r % kA);
        t.hash[-t.child_slot[r] - 1] = (int)idx + 1;
    }
}

__global__ void k_near_advance(rc_near_t t, u32 rows) {
    const u32 fresh = t.prefix[rows - 1] + t.flags[rows - 1];
    t.words[2] = fresh;
    if (!t.words[1]) t.words[0] += fresh;
}

// ---- probe and optimal tail: one lane per state ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_near_depth(rc_near_t t, const u8 *__restrict__ soa, size_t n, size_t stride, int8_t *__restrict__ depth_out,
                                                       int *__restrict__ node_out, int *__restrict__ status) {
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        const uint4 key = key_from_column(soa, stride, i);
        int node = near_find(t, key);
        int d = node >= 0 ? near_depth_of(t, node) : -1;
        if (node == -2 || d == -2) {
            *status = RC_NEAR_CORRUPT;
            node = -1;
            d = -1;
        }
        depth_out[i] = (int8_t)d;
        if (node_out) node_out[i] = node;
    }
}

__global__ __launch_bounds__(kBlock) void k_near_solve(rc_near_t t, const u8 *__restrict__ soa, size_t n, size_t stride, u8 *__restrict__ out_queues,
                                                       u32 out_width, int *__restrict__ out_lens, int *__restrict__ status) {
    __shared__ u32 s_lut[sizeof(kTables.lut) / 4];
    stage_to_lds(s_lut, c_tables.lut, sizeof(kTables.lut));
    __syncthreads();
    const u8 *lut = reinterpret_cast<const u8 *>(s_lut);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        const uint4 key = key_from_column(soa, stride, i);
        const int node = near_find(t, key);
        int d = node >= 0 ? near_depth_of(t, node) : -1;
        bool ok = node != -2 && d != -2 && d <= (int)out_width;   // (out_width >= depth: checked on the host)
        if (ok && d > 0) {
            // the solution undoes a_d first: the reverse of a_1 .. a_d with every move inverted
            u8 *row = out_queues + i * out_width;
            ok = near_walk_back(t, key, node, d, lut, [&](int s, u32 a) { row[s] = (u8)(a ^ 1u); });
        }
        if (!ok) {
            *status = RC_NEAR_CORRUPT;
            d = -1;
        }
        out_lens[i] = d;
    }
}

// ---- tighten -------------------------------------------------------------------------------------------------------------------------------
struct TGame {
    u32 L, W;       // moves; band width min(L, window)
    size_t b0, p0;  // first band byte, first position
};

// What the struct says about game g, checked against the struct's own totals: false = not this batch's data.
__device__ __forceinline__ bool load_tgame(const rc_near_tighten_t &s, u32 g, TGame &q) {
    const int L = s.lens[g];
    if (L < 0 || (u32)L > s.max_len) return false;
    const unsigned long long b0 = s.band_off[g], b1 = s.band_off[g + 1], p0 = s.pos_off[g], p1 = s.pos_off[g + 1];
    const u32 W = min((u32)L, s.window);
    if (b1 < b0 || b1 > s.total_band || b1 - b0 < (unsigned long long)L * W) return false;
    if (p1 < p0 || p1 > s.total_positions || p1 - p0 < (unsigned long long)L + 1) return false;
    q.L = (u32)L;
    q.W = W;
    q.b0 = (size_t)b0;
    q.p0 = (size_t)p0;
    return true;
}

// status and out_lens of every game: one wave per game looks at the bytes inside its length before any of them indexes a table
__global__ __launch_bounds__(kWave) void k_near_t_status(rc_near_tighten_t s) {
    const u32 g = blockIdx.x;
    int st = RC_NEAR_T_SKIPPED;
    if (s.select[g]) {
        TGame q;
        st = RC_NEAR_T_FAILED;
        if (load_tgame(s, g, q)) {
            const u8 *row = s.queues + (size_t)g * s.queue_width;   // (max_len <= queue_width: checked on the host)
            bool bad = false;
            for (u32 i = threadIdx.x; i < q.L; i += kWave) bad |= row[i] >= kA;
            st = __any(bad) ? RC_NEAR_T_BAD_ACTION : RC_NEAR_T_OK;
        }
    }
    if (threadIdx.x == 0) {
        s.status[g] = st;
        s.out_lens[g] = -1;
    }
}

// d(i, j) for j = i + 1 .. min(L, i + W): grid (games, parts), a lane carries kStarts starts and their products move by move
__global__ __launch_bounds__(kBlock) void k_near_t_distances(rc_near_t t, rc_near_tighten_t s) {
    __shared__ u32 s_lut[sizeof(kTables.lut) / 4];
    stage_to_lds(s_lut, c_tables.lut, sizeof(kTables.lut));
    __syncthreads();
    const u8 *lut = reinterpret_cast<const u8 *>(s_lut);
    const u32 g = blockIdx.x;
    TGame q;
    if (s.status[g] != RC_NEAR_T_OK || !load_tgame(s, g, q)) return;
    const u8 *row = s.queues + (size_t)g * s.queue_width;
    u8 *band = s.band + q.b0;
    const u32 span = kBlock * gridDim.y;
    bool corrupt = false;
    for (u32 i0 = blockIdx.y * kBlock + threadIdx.x; i0 < q.L; i0 += kStarts * span) {
        uint4 key[kStarts];
        u32 start[kStarts];
#pragma unroll
        for (int u = 0; u < kStarts; ++u) {
            key[u] = solved_key();
            start[u] = i0 + u * span;   // (>= L: the lane's second start does not exist)
        }
        for (u32 k = 0; k < q.W; ++k) {
            u32 h[kStarts];
            int c[kStarts];
            bool live[kStarts];
#pragma unroll
            for (int u = 0; u < kStarts; ++u) {
                live[u] = start[u] < q.L && start[u] + k < q.L;
                if (live[u]) {
                    key[u] = key_turned(key[u], row[start[u] + k], lut);
                    h[u] = near_home(t, key[u]);
                    c[u] = t.hash[h[u]];
                }
            }
#pragma unroll
            for (int u = 0; u < kStarts; ++u) {
                if (!live[u]) continue;
                const int node = near_finish(t, key[u], h[u], c[u]);
                const int d = node >= 0 ? near_depth_of(t, node) : -1;
                corrupt |= node == -2 || d == -2;
                band[(size_t)start[u] * q.W + k] = (u8)(d >= 0 ? d : kNone);
            }
            if (!live[0]) break;   // (start[1] > start[0]: it ends no later)
        }
    }
    if (corrupt) s.status[g] = RC_NEAR_T_FAILED;
}

// a word another lane of the workgroup has stored since the launch began: read at L2, never from a stale L1 line
__device__ __forceinline__ int fresh(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// smallest cost << 32 | i over a wave; every lane gets it
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long x = __shfl_xor(v, o, kWave);
        v = x < v ? x : v;
    }
    return v;
}

// best[0] = 0, best[j] = min over max(0, j - W) <= i < j with d(i, j) defined of best[i] + d(i, j), the smallest i among equals;
// then the chosen i are followed back from L and every chosen segment writes the table's a_1 .. a_d of its product at best[i].
__global__ __launch_bounds__(kRouteBlock) void k_near_t_route(rc_near_t t, rc_near_tighten_t s) {
    __shared__ u32 s_lut[sizeof(kTables.lut) / 4];
    __shared__ int s_bad;
    stage_to_lds(s_lut, c_tables.lut, sizeof(kTables.lut));
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const u8 *lut = reinterpret_cast<const u8 *>(s_lut);
    const u32 g = blockIdx.x, lane = threadIdx.x;
    TGame q;
    if (s.status[g] != RC_NEAR_T_OK || !load_tgame(s, g, q)) return;
    const u8 *row = s.queues + (size_t)g * s.queue_width;
    const u8 *band = s.band + q.b0;
    int *best = s.best + q.p0, *from = s.from + q.p0;
    if (lane == 0) {
        best[0] = 0;
        from[0] = 0;
    }
    for (u32 j = 1; j <= q.L; ++j) {
        wave_store_fence();   // best[j - 1] of the step before
        __syncthreads();
        unsigned long long mine = ~0ull;
        for (u32 i = j - min(j, q.W) + lane; i < j; i += kWave) {
            const u32 d = band[(size_t)i * q.W + (j - i - 1)];
            if (d == (u32)kNone) continue;
            const unsigned long long cand = ((unsigned long long)(u32)(fresh(&best[i]) + (int)d) << 32) | i;
            mine = cand < mine ? cand : mine;
        }
        mine = wave_min_u64(mine);
        if (mine == ~0ull || (mine >> 32) > j) {   // d(j - 1, j) = 1 is always defined, so best[j] <= best[j - 1] + 1 <= j
            if (lane == 0) s.status[g] = RC_NEAR_T_FAILED;
            return;   // (uniform)
        }
        if (lane == 0) {
            best[j] = (int)(mine >> 32);
            from[j] = (int)(u32)mine;
        }
    }
    wave_store_fence();
    __syncthreads();
    const int len = fresh(&best[q.L]);
    if ((u32)len > s.out_width) {
        if (lane == 0) {
            s.out_lens[g] = len;
            s.status[g] = RC_NEAR_T_NO_ROOM;
        }
        return;
    }
    if (lane == 0)   // mark the chosen segments: from[j] = ~i (i < j, so the walk ends within L steps)
        for (u32 j = q.L; j > 0;) {
            const u32 i = (u32)from[j];
            if (i >= j) {   // (not what the loop above wrote)
                s_bad = 1;
                break;
            }
            from[j] = ~(int)i;
            j = i;
        }
    wave_store_fence();
    __syncthreads();
    u8 *out = s.out_queues + (size_t)g * s.out_width;
    for (u32 j = 1 + lane; j <= q.L; j += kWave) {
        const int word = fresh(&from[j]);
        if (word >= 0) continue;
        const u32 i = (u32)~word;
        const int at = fresh(&best[i]);
        const int d = band[(size_t)i * q.W + (j - i - 1)];
        if (d == 0) continue;
        uint4 key = solved_key();
        for (u32 k = i; k < j; ++k) key = key_turned(key, row[k], lut);
        const int node = near_find(t, key);
        u8 *dst = out + at;
        const bool ok = node >= 0 && near_depth_of(t, node) == d && at >= 0 && at + d <= len && at + d == fresh(&best[j]) &&
                        near_walk_back(t, key, node, d, lut, [&](int st, u32 a) { dst[d - 1 - st] = (u8)a; });
        if (!ok) s_bad = 1;
    }
    __syncthreads();
    if (lane == 0) {
        if (s_bad) {
            s.status[g] = RC_NEAR_T_FAILED;
        } else {
            s.out_lens[g] = len;
        }
    }
}

static int check_tighten(const rc_near_tighten_t *s) {
    RC_REQUIRE(s != nullptr, RC_ERR_NULL);
    RC_REQUIRE(s->queues && s->lens && s->select && s->band_off && s->pos_off && s->band && s->best && s->from && s->out_queues &&
                   s->out_lens && s->status,
               RC_ERR_NULL);
    auto misaligned = [](const void *p, unsigned m) { return (reinterpret_cast<uintptr_t>(p) & (m - 1)) != 0; };
    RC_REQUIRE(!misaligned(s->band_off, 8) && !misaligned(s->pos_off, 8), RC_ERR_ALIGN);
    RC_REQUIRE(!misaligned(s->lens, 4) && !misaligned(s->best, 4) && !misaligned(s->from, 4) && !misaligned(s->out_lens, 4) &&
                   !misaligned(s->status, 4),
               RC_ERR_ALIGN);
    RC_REQUIRE(s->n_games >= 1 && s->n_games < (1u << 31), RC_ERR_RANGE);
    RC_REQUIRE(s->queue_width >= 1 && s->out_width >= 1 && s->window >= 1, RC_ERR_RANGE);
    RC_REQUIRE(s->max_len <= (u32)RC_NEAR_T_MAX_LEN && s->max_len <= s->queue_width, RC_ERR_RANGE);
    RC_REQUIRE(s->total_positions >= 1 && s->total_positions < ((size_t)1 << 40) && s->total_band < ((size_t)1 << 46), RC_ERR_RANGE);
    return RC_OK;
}

}  // namespace rubiks

using namespace rubiks;

extern "C" {

size_t rc_near_struct_bytes(void) { return sizeof(rc_near_t); }
size_t rc_near_tighten_struct_bytes(void) { return sizeof(rc_near_tighten_t); }

size_t rc_near_scan_bytes(uint32_t chunk_rows) {
    size_t bytes = 0;
    const u32 *in = nullptr;
    u32 *out = nullptr;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)chunk_rows) != hipSuccess) return 0;
    return round_up(bytes ? bytes : 16, 256);
}

// the root of agents.py:92-103's search, here the solved state: node 0, depth 0
int rc_near_begin(const rc_near_t *t, rc_stream_t stream) {
    if (int rc = check_near(t, true)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipError_t e = hipMemsetAsync(t->hash, 0, (size_t)t->hash_size * sizeof(int32_t), st); e != hipSuccess) return hip_rc(e);
    k_near_begin<<<1, 1, 0, st>>>(*t);
    return launch_status();
}

// agents.py:104-129 for one chunk of a level, without target and max_states
int rc_near_expand(const rc_near_t *t, uint32_t lo, uint32_t n_parents, uint32_t level, rc_stream_t stream) {
    if (int rc = check_near(t, true)) return rc;
    RC_REQUIRE(n_parents >= 1 && (unsigned long long)n_parents * kA <= t->chunk_rows, RC_ERR_RANGE);
    RC_REQUIRE((unsigned long long)lo + n_parents <= t->capacity, RC_ERR_RANGE);
    RC_REQUIRE(level >= 1 && level <= t->depth, RC_ERR_RANGE);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const u32 rows = n_parents * kA;
    const unsigned grid = grid_for(rows);
    k_near_children<<<grid, kBlock, 0, st>>>(*t, lo, rows);
    k_near_claim<<<grid, kBlock, 0, st>>>(*t, rows);
    k_near_flags<<<grid, kBlock, 0, st>>>(*t, rows);
    size_t bytes = t->scan_tmp_bytes;
    if (hipError_t e = hipcub::DeviceScan::ExclusiveSum(t->scan_tmp, bytes, t->flags, t->prefix, (int)rows, st); e != hipSuccess) return hip_rc(e);
    k_near_commit<<<grid, kBlock, 0, st>>>(*t, rows, level);
    k_near_advance<<<1, 1, 0, st>>>(*t, rows);
    return launch_status();
}

int rc_near_depth(const rc_near_t *t, const int8_t *soa, size_t n, size_t stride, int8_t *depth_out, int32_t *node_out, int32_t *status,
                  rc_stream_t stream) {
    if (int rc = check_near(t, false)) return rc;
    RC_CHECK_SOA(soa, n, stride);
    RC_REQUIRE(depth_out && status, RC_ERR_NULL);
    RC_REQUIRE(n >= 1, RC_ERR_RANGE);
    k_near_depth<<<grid_for(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(*t, reinterpret_cast<const u8 *>(soa), n, stride, depth_out, node_out,
                                                                               status);
    return launch_status();
}

int rc_near_solve(const rc_near_t *t, const int8_t *soa, size_t n, size_t stride, uint8_t *out_queues, uint32_t out_width, int32_t *out_lens,
                  int32_t *status, rc_stream_t stream) {
    if (int rc = check_near(t, false)) return rc;
    RC_CHECK_SOA(soa, n, stride);
    RC_REQUIRE(out_queues && out_lens && status, RC_ERR_NULL);
    RC_REQUIRE(n >= 1 && out_width >= t->depth, RC_ERR_RANGE);
    k_near_solve<<<grid_for(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(*t, reinterpret_cast<const u8 *>(soa), n, stride, out_queues, out_width,
                                                                               out_lens, status);
    return launch_status();
}

int rc_near_tighten_distances(const rc_near_t *t, const rc_near_tighten_t *s, rc_stream_t stream) {
    if (int rc = check_near(t, false)) return rc;
    if (int rc = check_tighten(s)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    k_near_t_status<<<s->n_games, kWave, 0, st>>>(*s);
    const unsigned parts = (unsigned)std::min<size_t>(64, std::max<size_t>(1, ceil_div((size_t)s->max_len, (size_t)kBlock * kStarts)));
    k_near_t_distances<<<dim3(s->n_games, parts), kBlock, 0, st>>>(*t, *s);
    return launch_status();
}

int rc_near_tighten_route(const rc_near_t *t, const rc_near_tighten_t *s, rc_stream_t stream) {
    if (int rc = check_near(t, false)) return rc;
    if (int rc = check_tighten(s)) return rc;
    k_near_t_route<<<s->n_games, kRouteBlock, 0, static_cast<hipStream_t>(stream)>>>(*t, *s);
    return launch_status();
}

int rc_near_tighten(const rc_near_t *t, const rc_near_tighten_t *s, rc_stream_t stream) {
    if (int rc = rc_near_tighten_distances(t, s, stream)) return rc;
    return rc_near_tighten_route(t, s, stream);
}

}  // extern "C"
