// Generalised move patterns of a batch of action sequences, for MI355X (gfx950): the reference's find_generalized_patterns
// (librubiks/analysis/pattern_mining.py:8-45) as a level-wise trie, one level per pattern length (include/rubiks_hip.h).
//   rc_patterns_begin:  status of every sequence -> the lanes (one per start position) after their first symbol
//   rc_patterns_extend: memsets -> every live lane takes its next symbol, finds or creates its node, counts once per sequence
//   rc_patterns_close:  nodes with count >= min_count -> out_rows; lanes below it or at their sequence's end retire; live count
// Launch boundaries are the only synchronisation: within a launch lanes only meet in atomics whose result they use at once (a
// compare-and-swap that returns the cell, an add, a minimum), and no lane waits for a value another lane publishes.  Keys are
// 64-bit words compared whole, so no count, membership or order depends on where the hash puts a key.
#include <algorithm>

#include "rubiks_common.h"

namespace rubiks {

using ull = unsigned long long;

constexpr u32 kSymbols = kActions;
constexpr u32 kLetterShift = 12;   // lane_state: bits 0-11 symbols seen, bits 12 + 3 f .. 14 + 3 f the letter of face f
constexpr u32 kPairs = 0x555;      // the even bit of every face's pair of symbols

__host__ __device__ inline ull patterns_hash(ull x) {   // (splitmix64's finaliser)
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// The cell of `key` in a table of mask + 1 cells, created if it is not there; -1 if the probe went round the table.
// created: this call turned a free cell into the key's.
__device__ __forceinline__ long long find_or_insert(ull *keys, size_t mask, ull key, bool &created) {
    created = false;
    size_t h = (size_t)patterns_hash(key) & mask;
    for (size_t probes = 0; probes <= mask; ++probes) {
        ull c = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == 0) {
            c = atomicCAS(&keys[h], 0ull, key);
            if (c == 0) {
                created = true;
                return (long long)h;
            }
        }
        if (c == key) return (long long)h;
        h = (h + 1) & mask;   // another key's cell
    }
    return -1;
}

// Every lane of the wave calls it: the lanes that `want` get consecutive numbers from *counter, one add per wave.
__device__ __forceinline__ u32 wave_reserve(u32 *counter, bool want) {
    const ull m = __ballot(want);
    if (m == 0) return 0;   // (wave-uniform)
    const u32 lane = threadIdx.x & (kWave - 1), leader = (u32)__ffsll((long long)m) - 1;
    u32 base = 0;
    if (lane == leader) base = atomicAdd(counter, (u32)__popcll(m));
    base = __shfl(base, (int)leader);
    return base + (u32)__popcll(m & ((1ull << lane) - 1));
}

// ---- status of every sequence: one wave each ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_patterns_check(rc_patterns_t p) {
    const u32 lane = threadIdx.x & (kWave - 1);
    const size_t s = (size_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (s >= p.n_seqs) return;   // (wave-uniform)
    const int len = p.lens[s];
    const ull p0 = p.pos_off[s], p1 = p.pos_off[s + 1];
    int st = RC_PATTERNS_OK;
    if (len < 0 || (u32)len > p.width || p1 < p0 || p1 - p0 != (ull)len || p1 > p.total_positions ||
        (s + 1 == p.n_seqs && p1 != p.total_positions) || (s == 0 && p0 != 0)) {
        st = RC_PATTERNS_FAILED;
    } else {
        const u8 *row = p.acts + s * p.width;
        bool bad = false;
        for (u32 i = lane; i < (u32)len; i += kWave) bad |= row[i] >= kSymbols;
        if (__ballot(bad) != 0) st = RC_PATTERNS_BAD_ACTION;
    }
    if (lane == 0) p.status[s] = st;
}

// ---- level 1: one thread per position --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_patterns_init(rc_patterns_t p) {
    const size_t rounds = ceil_div(p.total_positions, (size_t)gridDim.x * kBlock);
    for (size_t r = 0; r < rounds; ++r) {   // wave-uniform trip count: wave_reserve below needs the whole wave
        const size_t pos = (r * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
        bool live = false;
        if (pos < p.total_positions) {
            size_t lo = 0, hi = p.n_seqs;   // the last s with pos_off[s] <= pos: the sequence that owns the position
            while (hi - lo > 1) {
                const size_t mid = (lo + hi) / 2;
                if (p.pos_off[mid] <= pos) lo = mid; else hi = mid;
            }
            const size_t s = lo;
            p.lane_seq[pos] = (u32)s;
            int node = -1;
            const ull p0 = p.pos_off[s];
            if (p.status[s] == RC_PATTERNS_OK && p0 <= pos && pos - p0 < (ull)p.lens[s]) {   // (a FAILED neighbour can make s wrong: then not OK or not inside)
                const u32 i = (u32)(pos - p0);
                const u32 c = p.acts[s * p.width + i];   // < 12: the launch before has looked
                p.lane_state[pos] = 1u << c;             // its face gets letter 0
                live = i + 2 <= (u32)p.lens[s];
                node = live ? 0 : -1;
            }
            p.lane_node[pos] = node;
        }
        const ull m = __ballot(live);
        if (m != 0 && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(&p.counters[0], (u32)__popcll(m));
    }
}

// ---- level j: the live lanes take symbol i + j - 1 ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_patterns_extend(rc_patterns_t p) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t pos = (size_t)blockIdx.x * kBlock + threadIdx.x; pos < p.total_positions; pos += stride) {
        const int parent = p.lane_node[pos];
        if (parent < 0) continue;
        const u32 s = p.lane_seq[pos];
        if (s >= p.n_seqs) continue;   // (not what rc_patterns_begin wrote)
        const ull p0 = p.pos_off[s];
        const int len = p.lens[s];
        const ull at = (ull)pos - p0 + p.level - 1;   // i + j - 1
        if (p0 > pos || len < 0 || (u32)len > p.width || at >= (ull)len) {
            p.lane_node[pos] = -1;
            continue;
        }
        const u32 c = p.acts[(size_t)s * p.width + (size_t)at];
        if (c >= kSymbols) {
            p.status[s] = RC_PATTERNS_BAD_ACTION;
            p.lane_node[pos] = -1;
            continue;
        }
        u32 state = p.lane_state[pos];
        const u32 f = c >> 1, shift = kLetterShift + 3 * f;
        const bool exact = (state >> c) & 1u, face = (state >> (2 * f)) & 3u;
        u32 letter = (state >> shift) & 7u, lower = 0;
        if (!face) {
            const u32 seen = (state | (state >> 1)) & kPairs;
            letter = (u32)__popc(seen);   // faces seen so far: the next unused letter
            state |= letter << shift;
        } else if (!exact) {
            lower = 1;
        }
        state |= 1u << c;
        p.lane_state[pos] = state;
        const u32 token = 2 * letter + lower;

        bool created;
        const long long node = find_or_insert(reinterpret_cast<ull *>(p.node_keys), p.node_cells - 1, ((ull)(parent + 1) << 8) | (token + 1), created);
        if (node < 0) {
            p.status[s] = RC_PATTERNS_NO_ROOM;
            p.lane_node[pos] = -1;
            continue;
        }
        const long long cell = find_or_insert(reinterpret_cast<ull *>(p.seen_keys), p.seen_cells - 1, ((ull)(node + 1) << 32) | ((ull)s + 1), created);
        if (cell < 0) {
            p.status[s] = RC_PATTERNS_NO_ROOM;
            p.lane_node[pos] = -1;
            continue;
        }
        p.lane_node[pos] = (int)node;
        if (created) atomicAdd(&p.node_count[node], 1u);
        atomicMin(reinterpret_cast<ull *>(p.node_first) + node, ((ull)s << 32) | (ull)(pos - p0));
    }
}

// ---- end of level j: rows out, lanes retired, live lanes counted -------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_patterns_close(rc_patterns_t p) {
    const size_t span = (size_t)gridDim.x * kBlock;
    const size_t cell_rounds = ceil_div(p.node_cells, span), lane_rounds = ceil_div(p.total_positions, span);
    const size_t me = (size_t)blockIdx.x * kBlock + threadIdx.x;
    for (size_t r = 0; r < cell_rounds; ++r) {   // wave-uniform trip counts: wave_reserve needs the whole wave
        const size_t h = r * span + me;
        u32 count = 0;
        ull first = 0;
        bool out = false;
        if (h < p.node_cells && p.node_keys[h] != 0) {
            count = p.node_count[h];
            first = p.node_first[h];
            out = count >= p.min_count;
        }
        const u32 row = wave_reserve(&p.counters[1], out);
        if (out) {
            if (row < p.out_cap) {
                uint4 *dst = reinterpret_cast<uint4 *>(p.out_rows) + row;
                *dst = make_uint4(count, (u32)(first >> 32), (u32)first, p.level);
            } else {
                atomicAdd(&p.counters[2], 1u);
            }
        }
    }
    for (size_t r = 0; r < lane_rounds; ++r) {
        const size_t pos = r * span + me;
        bool live = false;
        if (pos < p.total_positions) {
            const int node = p.lane_node[pos];
            if (node >= 0) {
                const u32 s = p.lane_seq[pos];
                if ((size_t)node < p.node_cells && s < p.n_seqs) {
                    const ull i = (ull)pos - p.pos_off[s];
                    const int len = p.lens[s];
                    live = p.node_count[node] >= p.min_count && len >= 0 && i + p.level + 1 <= (ull)len;
                }
                if (!live) p.lane_node[pos] = -1;
            }
        }
        const ull m = __ballot(live);
        if (m != 0 && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(&p.counters[0], (u32)__popcll(m));
    }
}

static bool pow2(size_t x) { return x >= 2 && (x & (x - 1)) == 0; }

static int check_patterns(const rc_patterns_t *p, bool leveled) {
    RC_REQUIRE(p != nullptr, RC_ERR_NULL);
    RC_REQUIRE(p->acts && p->lens && p->pos_off && p->lane_seq && p->lane_state && p->lane_node && p->node_keys && p->node_count &&
                   p->node_first && p->seen_keys && p->out_rows && p->counters && p->status,
               RC_ERR_NULL);
    auto misaligned = [](const void *q, unsigned m) { return (reinterpret_cast<uintptr_t>(q) & (m - 1)) != 0; };
    RC_REQUIRE(aligned16(p->out_rows) && aligned16(p->counters), RC_ERR_ALIGN);
    RC_REQUIRE(!misaligned(p->pos_off, 8) && !misaligned(p->node_keys, 8) && !misaligned(p->node_first, 8) && !misaligned(p->seen_keys, 8), RC_ERR_ALIGN);
    RC_REQUIRE(!misaligned(p->lens, 4) && !misaligned(p->lane_seq, 4) && !misaligned(p->lane_state, 4) && !misaligned(p->lane_node, 4) &&
                   !misaligned(p->node_count, 4) && !misaligned(p->status, 4),
               RC_ERR_ALIGN);
    RC_REQUIRE(p->n_seqs >= 1 && p->n_seqs < (1u << 31) && p->width >= 1, RC_ERR_RANGE);
    RC_REQUIRE(p->total_positions >= 1 && p->total_positions < ((size_t)1 << 40), RC_ERR_RANGE);
    if (leveled) {
        RC_REQUIRE(p->level >= 2 && p->level <= p->width, RC_ERR_RANGE);
        RC_REQUIRE(pow2(p->node_cells) && pow2(p->seen_cells) && p->node_cells <= ((size_t)1 << 31) && p->seen_cells <= ((size_t)1 << 42), RC_ERR_RANGE);
    }
    return RC_OK;
}

}  // namespace rubiks

using namespace rubiks;

extern "C" {

size_t rc_patterns_struct_bytes(void) { return sizeof(rc_patterns_t); }

size_t rc_patterns_table_cells(size_t keys) {
    if (keys >= ((size_t)1 << 40)) return 0;
    size_t cells = 2;
    while (cells < 2 * keys) cells *= 2;
    return cells;
}

size_t rc_patterns_workspace_bytes(size_t total_positions) {
    const size_t P = total_positions, C = rc_patterns_table_cells(total_positions);
    if (C == 0) return 0;
    return 3 * round_up(4 * P, 256) + round_up(8 * C, 256) + round_up(4 * C, 256) + round_up(8 * C, 256) + round_up(8 * C, 256) +
           round_up(16 * P, 256) + 256;
}

uint64_t rc_patterns_hash(uint64_t key) { return patterns_hash(key); }

int rc_patterns_begin(const rc_patterns_t *p, rc_stream_t stream) {
    if (int rc = check_patterns(p, false)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipError_t e = hipMemsetAsync(p->counters, 0, 4 * sizeof(u32), st); e != hipSuccess) return hip_rc(e);
    k_patterns_check<<<(unsigned)ceil_div(p->n_seqs, kBlock / kWave), kBlock, 0, st>>>(*p);
    k_patterns_init<<<grid_for(p->total_positions), kBlock, 0, st>>>(*p);
    return launch_status();
}

int rc_patterns_extend(const rc_patterns_t *p, rc_stream_t stream) {
    if (int rc = check_patterns(p, true)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(p->node_keys, 0, p->node_cells * sizeof(u64), st);
    if (e == hipSuccess) e = hipMemsetAsync(p->node_count, 0, p->node_cells * sizeof(u32), st);
    if (e == hipSuccess) e = hipMemsetAsync(p->node_first, 0xFF, p->node_cells * sizeof(u64), st);
    if (e == hipSuccess) e = hipMemsetAsync(p->seen_keys, 0, p->seen_cells * sizeof(u64), st);
    if (e == hipSuccess) e = hipMemsetAsync(p->counters, 0, 4 * sizeof(u32), st);
    if (e != hipSuccess) return hip_rc(e);
    k_patterns_extend<<<grid_for(p->total_positions), kBlock, 0, st>>>(*p);
    return launch_status();
}

int rc_patterns_close(const rc_patterns_t *p, rc_stream_t stream) {
    if (int rc = check_patterns(p, true)) return rc;
    k_patterns_close<<<grid_for(std::max(p->total_positions, p->node_cells)), kBlock, 0, static_cast<hipStream_t>(stream)>>>(*p);
    return launch_status();
}

int rc_patterns_level(const rc_patterns_t *p, rc_stream_t stream) {
    if (int rc = rc_patterns_extend(p, stream)) return rc;
    return rc_patterns_close(p, stream);
}

}  // extern "C"
