// Shortening action queues through the graph of the states they visit, for MI355X (gfx950): the reference's _complete_graph and
// _shorten_action_queue (librubiks/solving/agents.py:597-633) with a game's path in place of an MCTS tree, so that any agent's
// queue can be shortened (k_mcts_complete_graph / k_mcts_shorten of rubiks_mcts.hip stay what MCTS uses).  A batch of games is
// ragged: game g owns positions pos_off[g] .. and hash cells hash_off[g] .. of the workspace arrays (include/rubiks_hip.h).
//   rc_shorten_index:      replay (keys of every position) -> memset of the cells -> insert (smallest position of a state wins) -> ids
//   rc_shorten_neighbours: nbr[node][12] by one probe per (node, action)
//   rc_shorten_bfs:        ordered level-synchronous search, one workgroup per game, and the walk back
// Launch boundaries are the only synchronisation between workgroups, except the atomics on a game's hash cells while it is
// filled.  Every length, offset, table word and index read from memory is range-checked before it addresses anything: a game
// that fails a check ends RC_SHORTEN_FAILED.
#include <limits.h>

#include <algorithm>

#include "rubiks_keys.h"

namespace rubiks {

constexpr int kLanes = kPlanes;   // replay: one lane per cubie ...
constexpr int kWaveGames = 3;     // ... so three games per wave (lanes 60 .. 63 idle)
constexpr int kTile = 64;         // positions replayed between two packing passes
constexpr u32 kA = kActions;

struct Game {
    u32 L;          // moves; positions 0 .. L
    size_t p0, h0;  // first position / hash cell
    u32 hmask;      // cells - 1
};

// What the struct says about game g, checked against the struct's own totals (the host's words): false = not this batch's data.
__device__ __forceinline__ bool load_game(const rc_shorten_t &s, u32 g, Game &q) {
    const int L = s.lens[g];
    const unsigned long long p0 = s.pos_off[g], p1 = s.pos_off[g + 1], h0 = s.hash_off[g], h1 = s.hash_off[g + 1];
    if (L < 0 || (u32)L > s.max_len) return false;
    if (p1 < p0 || p1 > s.total_positions || p1 - p0 < (unsigned long long)L + 1) return false;
    if (h1 < h0 || h1 > s.total_hash_cells) return false;
    const unsigned long long cells = h1 - h0;
    if (cells < 2ull * ((unsigned long long)L + 1) || (cells & (cells - 1)) != 0 || cells > (1ull << 30)) return false;
    q.L = (u32)L;
    q.p0 = (size_t)p0;
    q.h0 = (size_t)h0;
    q.hmask = (u32)cells - 1;
    return true;
}

// game blockIdx.x if it is still RC_SHORTEN_OK (the kernels after the replay)
__device__ __forceinline__ bool game_ok(const rc_shorten_t &s, u32 g, Game &q) {
    return s.status[g] == RC_SHORTEN_OK && load_game(s, g, q);
}

// ---- status of every game, then s_0 .. s_L of the selected ones: three games per wave, one lane per cubie -------------------
// A move maps each of the 20 codes through the table on its own, so a lane carries one code along the path.  Per tile of
// kTile positions: the lanes fetch the tile's actions into LDS, walk it (one broadcast read of the action, one table read, one
// byte written per move), then pack the tile's states into keys, a position per lane.
__global__ __launch_bounds__(kWave) void k_shorten_replay(rc_shorten_t s) {
    __shared__ u32 s_lut[sizeof(kTables.lut) / 4];
    __shared__ u32 s_codes[kWaveGames][kTile][kLanes / 4];   // [position in tile][20 code bytes]
    __shared__ u8 s_act[kWaveGames][kTile];
    __shared__ int s_len[kWaveGames], s_bad[kWaveGames];
    stage_to_lds(s_lut, c_tables.lut, sizeof(kTables.lut));
    const u32 lane = threadIdx.x, gl = lane / kLanes, j = lane % kLanes;
    const u32 g = blockIdx.x * kWaveGames + gl;
    const bool live = gl < kWaveGames && g < s.n_games;
    if (lane < kWaveGames) {
        s_len[lane] = -1;
        s_bad[lane] = 0;
    }
    __syncthreads();
    Game q = {0, 0, 0, 0};
    int st = RC_SHORTEN_SKIPPED;
    bool run = false;
    if (live && s.select[g]) {
        run = load_game(s, g, q);
        st = run ? RC_SHORTEN_OK : RC_SHORTEN_FAILED;
    }
    const u8 *row = s.queues + (size_t)(live ? g : 0) * s.queue_width;   // (max_len <= queue_width: checked on the host)
    if (run) {   // a byte that is no action is found here, before any byte indexes the table
        bool bad = false;
        for (u32 i = j; i < q.L; i += kLanes) bad |= row[i] >= kA;
        if (bad) s_bad[gl] = 1;
    }
    __syncthreads();
    if (run && s_bad[gl]) {
        run = false;
        st = RC_SHORTEN_BAD_ACTION;
    }
    if (live && j == 0) {
        s.status[g] = st;
        s.out_lens[g] = -1;
        if (run) s_len[gl] = (int)q.L;
    }
    __syncthreads();
    const int l_max = max(s_len[0], max(s_len[1], s_len[2]));   // wave-uniform: the loop below holds barriers
    if (l_max < 0) return;
    const u8 *lut = reinterpret_cast<const u8 *>(s_lut) + (j >= (u32)kCorners ? kCodePad : 0);
    const u32 g_act = gl < kWaveGames ? gl : 0;
    u8 *codes = reinterpret_cast<u8 *>(&s_codes[g_act][0][0]);
    u32 c = run ? ((u32)(u8)s.roots_soa[(size_t)j * s.stride + g] & 31u) : 0u;
    uint4 *keys = reinterpret_cast<uint4 *>(s.keys) + q.p0;
    for (u32 base = 0; base <= (u32)l_max; base += kTile) {
        if (run)
            for (u32 i = j; i < (u32)kTile; i += kLanes) s_act[g_act][i] = base + i < q.L ? row[base + i] : (u8)15;   // 15: identity padding
        __syncthreads();
        if (run)
            for (u32 i = 0; i < (u32)kTile && base + i <= q.L; ++i) {
                codes[i * kLanes + j] = (u8)c;
                c = lut[(s_act[g_act][i] & 15u) * (2 * kCodePad) + c];
            }
        __syncthreads();
        if (run)
            for (u32 i = j; i < (u32)kTile && base + i <= q.L; i += kLanes) {
                u32 w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < kLanes / 4; ++k) {
                    const u32 four = s_codes[g_act][i][k];
#pragma unroll
                    for (int b = 0; b < 4; ++b) key_set(w, 4 * k + b, code_of(four, b));
                }
                keys[base + i] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        __syncthreads();
    }
}

// ---- `self.indices` (agents.py:597-611 reads it): every position enters its game's table; equal states elect the smallest --------
// grid (games, parts).  A cell only ever changes from 0 to a position's node and then to a smaller node of the SAME state, and a
// probe sequence never loses a cell, so all positions of a state meet in one cell whatever the order of the inserts: the cell
// ends as 1 + the state's first position, as A*'s first-occurrence election ends on the lowest row.
__global__ __launch_bounds__(kBlock) void k_shorten_insert(rc_shorten_t s) {
    const u32 g = blockIdx.x;
    Game q;
    if (!game_ok(s, g, q)) return;
    const uint4 *keys = reinterpret_cast<const uint4 *>(s.keys) + q.p0;
    int *tab = s.hash + q.h0;
    for (u32 p = blockIdx.y * kBlock + threadIdx.x; p <= q.L; p += kBlock * gridDim.y) {
        const uint4 key = keys[p];
        const int mine = (int)p + 1;
        u32 h = key_hash(key) & q.hmask;
        for (u32 probes = 0; probes <= q.hmask; ++probes) {
            int c = __hip_atomic_load(&tab[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c == 0) {
                c = atomicCAS(&tab[h], 0, mine);
                if (c == 0) break;
            }
            if (c > 0 && (u32)c <= q.L + 1 && key_eq(keys[c - 1], key)) {   // (keys: written by the launch before)
                atomicMin(&tab[h], mine);
                break;
            }
            h = (h + 1) & q.hmask;   // another state's cell
        }
    }
}

// cell of `key` in the game's table: its node, 0 if the state is no node, -1 if a word on the way is not a node of this game
__device__ __forceinline__ int find_node(const int *tab, const uint4 *keys, const int *ids, const Game &q, const uint4 &key) {
    u32 h = key_hash(key) & q.hmask;
    for (u32 probes = 0; probes <= q.hmask; ++probes) {
        const int c = tab[h];
        if (c == 0) return 0;
        if (c < 0 || (u32)c > q.L + 1 || (ids && ids[c - 1] != c)) return -1;
        if (key_eq(keys[c - 1], key)) return c;
        h = (h + 1) & q.hmask;
    }
    return -1;   // (a table without a free cell is not one this library filled: cells >= 2 (L + 1))
}

__global__ __launch_bounds__(kBlock) void k_shorten_ids(rc_shorten_t s) {
    const u32 g = blockIdx.x;
    Game q;
    if (!game_ok(s, g, q)) return;
    const uint4 *keys = reinterpret_cast<const uint4 *>(s.keys) + q.p0;
    const int *tab = s.hash + q.h0;
    int *ids = s.ids + q.p0;
    for (u32 p = blockIdx.y * kBlock + threadIdx.x; p <= q.L; p += kBlock * gridDim.y) {
        const int v = find_node(tab, keys, nullptr, q, keys[p]);
        if (v < 1 || (u32)v > p + 1) {   // every position is in the table, under a position that is not later than itself
            ids[p] = 0;
            s.status[g] = RC_SHORTEN_FAILED;
        } else {
            ids[p] = v;
        }
    }
}

// ---- _complete_graph (agents.py:597-611), every node a leaf: grid (games, parts), one thread per (position, action) ----------------
__global__ __launch_bounds__(kBlock) void k_shorten_neighbours(rc_shorten_t s) {
    __shared__ u32 s_lut[sizeof(kTables.lut) / 4];
    stage_to_lds(s_lut, c_tables.lut, sizeof(kTables.lut));
    __syncthreads();
    const u8 *lut = reinterpret_cast<const u8 *>(s_lut);
    const u32 g = blockIdx.x;
    Game q;
    if (!game_ok(s, g, q)) return;
    const uint4 *keys = reinterpret_cast<const uint4 *>(s.keys) + q.p0;
    const int *tab = s.hash + q.h0;
    const int *ids = s.ids + q.p0;
    int *nbr = s.nbr + q.p0 * kA;
    const unsigned long long work = ((unsigned long long)q.L + 1) * kA;
    for (unsigned long long w = (unsigned long long)blockIdx.y * kBlock + threadIdx.x; w < work; w += (unsigned long long)kBlock * gridDim.y) {
        const u32 p = (u32)(w / kA), a = (u32)(w % kA);
        if (ids[p] != (int)p + 1) continue;   // a state that was here before: its node is the earlier position
        const int found = find_node(tab, keys, ids, q, key_turned(keys[p], a, lut));
        if (found < 0) {
            s.status[g] = RC_SHORTEN_FAILED;
            continue;
        }
        nbr[(size_t)p * kA + a] = found;
    }
}

// ---- _shorten_action_queue (agents.py:613-633): ordered BFS, one workgroup per game ---------------------------------------------
// As k_mcts_shorten: level-synchronous, candidate (frontier place i, action a) carries the scan index 12 i + a, the smallest index
// claims the node (atomicMin), and the next frontier is the claimed nodes in scan-index order (block-wide ordered compaction),
// which is the order in which the reference's FIFO would hold them.  Node v's words are row v - 1 of the game's arrays.
__global__ __launch_bounds__(kBlock) void k_shorten_bfs(rc_shorten_t s) {
    __shared__ int s_scan[kBlock];
    __shared__ int s_base, s_done, s_bad;
    const u32 tid = threadIdx.x;
    const u32 g = blockIdx.x;
    Game q;
    if (!game_ok(s, g, q)) return;
    const int n = (int)q.L + 1;   // ids lie in 1 .. n
    const int *ids = s.ids + q.p0;
    const int target = ids[q.L];
    if (target < 1 || target > n || ids[target - 1] != target) {
        if (tid == 0) s.status[g] = RC_SHORTEN_FAILED;
        return;
    }
    if (target == 1) {   // agents.py:614 (here: the queue returns to the root, so nothing is left of it)
        if (tid == 0) s.out_lens[g] = 0;
        return;
    }
    const int *nbr = s.nbr + q.p0 * kA;
    int *claim = s.claim + q.p0 * 2;
    int *cur = s.frontier_a + q.p0, *nxt = s.frontier_b + q.p0;
    for (int i = tid; i < n; i += kBlock) {
        claim[2 * i] = INT_MAX;
        claim[2 * i + 1] = 0;   // parent << 4 | action; 0 = not visited
    }
    if (tid == 0) {
        cur[0] = 1;
        s_done = 0;
        s_bad = 0;
    }
    __syncthreads();
    if (tid == 0) claim[1] = -1;   // the root is visited and has no parent
    int fsize = 1;
    while (fsize > 0) {
        __syncthreads();
        const int work = fsize * (int)kA;   // fsize <= n < 2^27
        // phase 1: every unvisited neighbour is claimed by the smallest scan index that reaches it
        for (int idx = tid; idx < work; idx += kBlock) {
            const int p = cur[idx / kA];
            if (p < 1 || p > n) { s_bad = 1; continue; }
            const int c = nbr[(size_t)(p - 1) * kA + idx % kA];
            if ((u32)c > (u32)n) { s_bad = 1; continue; }
            if (c != 0 && claim[2 * (c - 1) + 1] == 0) atomicMin(&claim[2 * (c - 1)], idx);
        }
        // the claims are no-return atomics executed at L2: drain them before the barrier, and read them back
        // with L2-served loads (a plain load could hit a stale L1 line)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // phase 2: winners enter the next frontier in scan order
        if (tid == 0) s_base = 0;
        __syncthreads();
        if (s_bad) break;   // uniform: written before the barrier above
        for (int idx0 = 0; idx0 < work; idx0 += kBlock) {
            const int idx = idx0 + (int)tid;
            int c = 0, win = 0, p = 0;
            if (idx < work) {
                p = cur[idx / kA];
                c = nbr[(size_t)(p - 1) * kA + idx % kA];   // (both checked in phase 1)
                win = (c != 0 && claim[2 * (c - 1) + 1] == 0 &&
                       __hip_atomic_load(&claim[2 * (c - 1)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == idx) ? 1 : 0;
            }
            s_scan[tid] = win;
            __syncthreads();
            for (int o = 1; o < kBlock; o <<= 1) {
                const int x = (tid >= (u32)o) ? s_scan[tid - o] : 0;
                __syncthreads();
                s_scan[tid] += x;
                __syncthreads();
            }
            const int pos = s_base + s_scan[tid] - win;
            if (win) {
                if (pos < n) nxt[pos] = c;   // (a node wins once, so the winners of a level are at most n)
                else s_bad = 1;
                claim[2 * (c - 1) + 1] = (p << 4) | (idx % (int)kA);
                if (c == target) s_done = 1;
            }
            __syncthreads();
            if (tid == kBlock - 1) s_base += s_scan[tid];
            __syncthreads();
        }
        fsize = s_base;
        if (s_done || s_bad) break;
        int *tmp = cur; cur = nxt; nxt = tmp;
    }
    __syncthreads();
    if (tid != 0) return;
    if (s_bad || !s_done) {   // (the target is reachable along the path itself: an empty frontier is not this game's data)
        s.status[g] = RC_SHORTEN_FAILED;
        return;
    }
    // walk the parents back to the root: first the length, then the bytes, root first
    int len = 0;
    bool ok = true;
    for (int v = target; v != 1; ++len) {
        const int word = claim[2 * (v - 1) + 1];
        v = word >> 4;
        ok = word > 0 && (word & 15) < (int)kA && v >= 1 && v <= n && len < (int)q.L;
        if (!ok) break;
    }
    if (!ok) {
        s.status[g] = RC_SHORTEN_FAILED;
        return;
    }
    s.out_lens[g] = len;
    if ((u32)len > s.out_width) {
        s.status[g] = RC_SHORTEN_NO_ROOM;
        return;
    }
    u8 *out = s.out_queues + (size_t)g * s.out_width;
    int v = target;
    for (int i = len; i > 0; --i) {   // (the chain the loop above has checked)
        const int word = claim[2 * (v - 1) + 1];
        out[i - 1] = (u8)(word & 15);
        v = word >> 4;
    }
}

static int check_shorten(const rc_shorten_t *s) {
    RC_REQUIRE(s != nullptr, RC_ERR_NULL);
    RC_REQUIRE(s->roots_soa && s->queues && s->lens && s->select && s->pos_off && s->hash_off && s->keys && s->ids && s->nbr && s->claim &&
                   s->frontier_a && s->frontier_b && s->hash && s->out_queues && s->out_lens && s->status,
               RC_ERR_NULL);
    auto misaligned = [](const void *p, unsigned m) { return (reinterpret_cast<uintptr_t>(p) & (m - 1)) != 0; };
    RC_REQUIRE(aligned16(s->roots_soa) && (s->stride & 15u) == 0 && aligned16(s->keys) && aligned16(s->hash), RC_ERR_ALIGN);
    RC_REQUIRE(!misaligned(s->pos_off, 8) && !misaligned(s->hash_off, 8), RC_ERR_ALIGN);
    RC_REQUIRE(!misaligned(s->lens, 4) && !misaligned(s->ids, 4) && !misaligned(s->nbr, 4) && !misaligned(s->claim, 4) &&
                   !misaligned(s->frontier_a, 4) && !misaligned(s->frontier_b, 4) && !misaligned(s->out_lens, 4) && !misaligned(s->status, 4),
               RC_ERR_ALIGN);
    RC_REQUIRE(s->n_games >= 1 && s->n_games < (1u << 31), RC_ERR_RANGE);
    RC_REQUIRE(s->stride >= round_up(s->n_games, 16), RC_ERR_STRIDE);
    RC_REQUIRE(s->queue_width >= 1 && s->out_width >= 1, RC_ERR_RANGE);
    RC_REQUIRE(s->max_len <= (u32)RC_SHORTEN_MAX_LEN && s->max_len <= s->queue_width, RC_ERR_RANGE);
    RC_REQUIRE(s->total_positions >= 1 && s->total_hash_cells >= 2, RC_ERR_RANGE);
    RC_REQUIRE(s->total_positions < ((size_t)1 << 40) && s->total_hash_cells < ((size_t)1 << 40), RC_ERR_RANGE);
    return RC_OK;
}

// parts of a game's workgroups: enough for the longest game, the short ones' spare workgroups leave at once
static unsigned parts_for(const rc_shorten_t *s, size_t items_per_position) {
    return (unsigned)std::min<size_t>(32, std::max<size_t>(1, ceil_div(((size_t)s->max_len + 1) * items_per_position, (size_t)kBlock * 8)));
}

}  // namespace rubiks

using namespace rubiks;

extern "C" {

size_t rc_shorten_struct_bytes(void) { return sizeof(rc_shorten_t); }

size_t rc_shorten_workspace_bytes(size_t total_positions, size_t total_hash_cells) {
    const size_t P = total_positions, H = total_hash_cells;
    if (P >= ((size_t)1 << 40) || H >= ((size_t)1 << 40)) return 0;
    return round_up(16 * P, 256) + round_up(4 * P, 256) + round_up(48 * P, 256) + round_up(8 * P, 256) + 2 * round_up(4 * P, 256) +
           round_up(4 * H, 256);
}

// agents.py:597-611's `self.states` and `self.indices` of every selected game's path
int rc_shorten_index(const rc_shorten_t *s, rc_stream_t stream) {
    if (int rc = check_shorten(s)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    k_shorten_replay<<<(unsigned)ceil_div(s->n_games, kWaveGames), kWave, 0, st>>>(*s);
    if (hipError_t e = hipMemsetAsync(s->hash, 0, s->total_hash_cells * sizeof(int), st); e != hipSuccess) return hip_rc(e);
    const dim3 grid(s->n_games, parts_for(s, 1));
    k_shorten_insert<<<grid, kBlock, 0, st>>>(*s);
    k_shorten_ids<<<grid, kBlock, 0, st>>>(*s);
    return launch_status();
}

// agents.py:597-611 (_complete_graph), every node a leaf
int rc_shorten_neighbours(const rc_shorten_t *s, rc_stream_t stream) {
    if (int rc = check_shorten(s)) return rc;
    k_shorten_neighbours<<<dim3(s->n_games, parts_for(s, kA)), kBlock, 0, static_cast<hipStream_t>(stream)>>>(*s);
    return launch_status();
}

// agents.py:613-633 (_shorten_action_queue)
int rc_shorten_bfs(const rc_shorten_t *s, rc_stream_t stream) {
    if (int rc = check_shorten(s)) return rc;
    k_shorten_bfs<<<s->n_games, kBlock, 0, static_cast<hipStream_t>(stream)>>>(*s);
    return launch_status();
}

int rc_shorten(const rc_shorten_t *s, rc_stream_t stream) {
    if (int rc = rc_shorten_index(s, stream)) return rc;
    if (int rc = rc_shorten_neighbours(s, stream)) return rc;
    return rc_shorten_bfs(s, stream);
}

}  // extern "C"
