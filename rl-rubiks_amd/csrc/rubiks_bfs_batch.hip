// Breadth-first search of S games in lock step for MI355X (gfx950): the chunk bookkeeping of rubiks_bfs.hip kept per slot
// (librubiks/solving/agents.py:92-129 of the reference), with the decision that file leaves to the host after every chunk --
// commit, stop or path -- made by a kernel, so that a step of the whole batch is a fixed sequence of launches without a host read:
//   children + lookup -> claim -> flags -> one exclusive scan over the row space -> decide -> commit -> path.
// Row space: slot s owns rows 12 C s .. 12 C (s + 1) - 1; local row 12 p + k is action k on the p-th parent of the slot's chunk,
// rows beyond 12 n_par are dead (flag 0).  A slot's local prefix is prefix[r] - prefix[slot's first row].  Node indices and hash
// contents are per slot; a slot's offset into the batch arrays is size_t.  Launch boundaries are the only synchronisation between
// workgroups.  Words and indices read from memory are range-checked before they address anything: a slot whose words do not
// fit its arrays ends RC_BFSB_FAILED.
#include <hipcub/hipcub.hpp>

#include "rubiks_keys.h"

namespace rubiks {

constexpr unsigned long long kNoRow = ~0ull;

__device__ __forceinline__ long long &word(const rc_bfs_batch_t &b, int w, u32 s) {
    return reinterpret_cast<long long *>(b.words)[(size_t)w * b.n_slots + s];
}

// agents.py:105 for the slot's next chunk: `len(self) < max_states` before the pop, else its parents
__device__ void next_chunk(const rc_bfs_batch_t &b, u32 s, u32 n_nodes, u32 lo, u32 level_end) {
    const u32 max_states = (u32)word(b, RC_BFSB_W_MAX_STATES, s);
    u32 n_par = 0;
    if (n_nodes >= max_states) {
        word(b, RC_BFSB_W_STATUS, s) = RC_BFSB_CUT;
    } else {
        n_par = min(b.chunk, level_end - lo);
    }
    word(b, RC_BFSB_W_N_PAR, s) = n_par;
    word(b, RC_BFSB_W_FIRST_SOLVED, s) = (long long)kNoRow;
}

// grid (n, y): the y workgroups of a list entry share the slot's hash cells; y == 0 also writes node 0 and the words
__global__ __launch_bounds__(kBlock) void k_bfsb_plant(rc_bfs_batch_t b, const int *__restrict__ slots, const u8 *__restrict__ roots,
                                                       size_t stride, size_t first_col, const u32 *__restrict__ max_states) {
    const int si = slots[blockIdx.x];
    if (si < 0 || (u32)si >= b.n_slots) return;   // (the whole workgroup: nothing is written for a slot that does not exist)
    const u32 s = (u32)si;
    const uint4 key = key_from_column(roots, stride, first_col + blockIdx.x);
    const bool solved = key_is_solved(key);
    const u32 root_cell = key_hash(key) & (b.hash_size - 1);
    int4 *cells = reinterpret_cast<int4 *>(b.hash + (size_t)s * b.hash_size);   // (hash_size >= 32: whole int4s)
    for (u32 i = blockIdx.y * kBlock + threadIdx.x; i < b.hash_size / 4; i += gridDim.y * kBlock) {
        int4 v = make_int4(0, 0, 0, 0);
        if (!solved && i == root_cell / 4) (&v.x)[root_cell & 3u] = 1;   // node 0
        cells[i] = v;
    }
    if (blockIdx.y != 0 || threadIdx.x != 0) return;
    const size_t node0 = (size_t)s * b.capacity;
    reinterpret_cast<uint4 *>(b.keys)[node0] = key;
    b.parent[node0] = 0;
    b.action[node0] = 0;
    const u32 room = b.capacity - kActions * b.chunk - 1;
    word(b, RC_BFSB_W_MAX_STATES, s) = min(max_states[blockIdx.x], room);
    word(b, RC_BFSB_W_QUEUE_LEN, s) = 0;
    word(b, RC_BFSB_W_LO, s) = 0;
    word(b, RC_BFSB_W_C_ROWS, s) = 0;
    word(b, RC_BFSB_W_C_BASE, s) = 0;
    word(b, RC_BFSB_W_C_LO, s) = 0;
    word(b, RC_BFSB_W_SOLVED_PARENT, s) = 0;
    word(b, RC_BFSB_W_LAST_ACTION, s) = 0;
    if (solved) {   // agents.py:100: nothing stored
        word(b, RC_BFSB_W_STATUS, s) = RC_BFSB_ROOT_SOLVED;
        word(b, RC_BFSB_W_NODES, s) = 0;
        word(b, RC_BFSB_W_LEVELS, s) = 0;
        word(b, RC_BFSB_W_LEVEL_END, s) = 0;
        word(b, RC_BFSB_W_N_PAR, s) = 0;
        word(b, RC_BFSB_W_FIRST_SOLVED, s) = (long long)kNoRow;
        return;
    }
    word(b, RC_BFSB_W_STATUS, s) = RC_BFSB_RUNNING;
    word(b, RC_BFSB_W_NODES, s) = 1;
    word(b, RC_BFSB_W_LEVELS, s) = 1;
    word(b, RC_BFSB_W_LEVEL_END, s) = 1;
    next_chunk(b, s, 1, 0, 1);
}

// what a row thread needs of its slot; n_par is 0 for a slot that does nothing, which is every slot that is not running: the
// other words of a slot that was never planted are whatever the memory held
struct SlotRow {
    u32 s, local, n_par;
    size_t row0;
};

__device__ __forceinline__ SlotRow slot_row(const rc_bfs_batch_t &b, u32 r, int n_word) {
    const u32 seg = kActions * b.chunk;
    SlotRow q;
    q.s = r / seg;
    q.local = r - q.s * seg;
    q.row0 = (size_t)q.s * seg;
    q.n_par = word(b, RC_BFSB_W_STATUS, q.s) == RC_BFSB_RUNNING ? (u32)word(b, n_word, q.s) : 0;
    return q;
}

// children of the slots' chunks, membership test against the slot's committed table
__global__ __launch_bounds__(kBlock) void k_bfsb_children(rc_bfs_batch_t b, u32 rows) {
    __shared__ u32 s_lut[sizeof(kTables.lut) / 4];
    stage_to_lds(s_lut, c_tables.lut, sizeof(kTables.lut));
    __syncthreads();
    const u8 *lut = reinterpret_cast<const u8 *>(s_lut);
    uint4 *child_keys = reinterpret_cast<uint4 *>(b.child_keys);
    const u32 mask = b.hash_size - 1;
    for (u32 r = blockIdx.x * kBlock + threadIdx.x; r < rows; r += gridDim.x * kBlock) {
        const SlotRow q = slot_row(b, r, RC_BFSB_W_N_PAR);
        if (q.local >= kActions * q.n_par) continue;
        const uint4 *keys = reinterpret_cast<const uint4 *>(b.keys) + (size_t)q.s * b.capacity;
        const int *hash = b.hash + (size_t)q.s * b.hash_size;
        const u32 lo = (u32)word(b, RC_BFSB_W_LO, q.s);
        if ((unsigned long long)lo + q.n_par > b.capacity) continue;   // (k_bfsb_decide fails such a slot)
        const uint4 pk = keys[lo + q.local / kActions];
        const uint4 ck = key_turned(pk, q.local % kActions, lut);
        child_keys[r] = ck;
        int cell_or_node;
        if (key_is_solved(ck)) {
            cell_or_node = 0;   // never stored (agents.py:111-116)
            atomicMin(reinterpret_cast<unsigned long long *>(&word(b, RC_BFSB_W_FIRST_SOLVED, q.s)), (unsigned long long)q.local);
        } else {
            u32 h = key_hash(ck) & mask;
            int found = 0;
            for (u32 probes = 0; probes <= mask; ++probes) {
                const int c = hash[h];
                if (c == 0) break;
                if (c > 0 && (u32)c <= b.capacity && key_eq(keys[c - 1], ck)) { found = c; break; }
                h = (h + 1) & mask;
            }
            cell_or_node = found ? found : -(int)h - 1;
        }
        b.child_slot[r] = cell_or_node;
    }
}

// unseen rows claim a cell of their slot's table; equal states elect their lowest row
__global__ __launch_bounds__(kBlock) void k_bfsb_claim(rc_bfs_batch_t b, u32 rows) {
    const uint4 *child_keys = reinterpret_cast<const uint4 *>(b.child_keys);
    const u32 mask = b.hash_size - 1, seg = kActions * b.chunk;
    for (u32 r = blockIdx.x * kBlock + threadIdx.x; r < rows; r += gridDim.x * kBlock) {
        const SlotRow q = slot_row(b, r, RC_BFSB_W_N_PAR);
        if (q.local >= kActions * q.n_par) continue;
        const int cs = b.child_slot[r];
        if (cs >= 0) continue;
        int *hash = b.hash + (size_t)q.s * b.hash_size;
        const u32 h = claim_lowest_row(hash, (u32)(-cs - 1), mask, -(int)(q.local + 1), seg, child_keys + q.row0, child_keys[r]);
        b.child_slot[r] = -(int)h - 1;
    }
}

// every row of the row space gets its flag: the scan runs over all of them
__global__ __launch_bounds__(kBlock) void k_bfsb_flags(rc_bfs_batch_t b, u32 rows) {
    for (u32 r = blockIdx.x * kBlock + threadIdx.x; r < rows; r += gridDim.x * kBlock) {
        const SlotRow q = slot_row(b, r, RC_BFSB_W_N_PAR);
        u32 flag = 0;
        if (q.local < kActions * q.n_par) {
            const int cs = b.child_slot[r];
            if (cs < 0) {
                const int *hash = b.hash + (size_t)q.s * b.hash_size;
                flag = __hip_atomic_load(&hash[(u32)(-cs - 1) & (b.hash_size - 1)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                       -(int)(q.local + 1);
            }
        }
        b.flags[r] = flag;
    }
}

// One wave per slot: what BFSDevice.search decides on the host after a chunk, in its order.
__global__ __launch_bounds__(kWave) void k_bfsb_decide(rc_bfs_batch_t b) {
    __shared__ u32 s_cut;
    const u32 s = blockIdx.x;
    const u32 n_par = (u32)word(b, RC_BFSB_W_N_PAR, s);
    if (word(b, RC_BFSB_W_STATUS, s) != RC_BFSB_RUNNING || n_par == 0) {   // finished and empty slots do nothing
        if (threadIdx.x == 0) {
            word(b, RC_BFSB_W_C_ROWS, s) = 0;
            word(b, RC_BFSB_W_N_PAR, s) = 0;
        }
        return;
    }
    const u32 n_nodes = (u32)word(b, RC_BFSB_W_NODES, s), lo = (u32)word(b, RC_BFSB_W_LO, s);
    const u32 level_end = (u32)word(b, RC_BFSB_W_LEVEL_END, s), max_states = (u32)word(b, RC_BFSB_W_MAX_STATES, s);
    const bool sane = n_par <= b.chunk && lo < level_end && level_end - lo >= n_par && level_end <= n_nodes && n_nodes < max_states &&
                      (unsigned long long)max_states + (unsigned long long)kActions * b.chunk + 1 <= b.capacity;
    if (!sane) {
        if (threadIdx.x == 0) {
            word(b, RC_BFSB_W_STATUS, s) = RC_BFSB_FAILED;
            word(b, RC_BFSB_W_C_ROWS, s) = 0;
            word(b, RC_BFSB_W_N_PAR, s) = 0;
        }
        return;
    }
    const u32 *prefix = b.prefix + (size_t)s * kActions * b.chunk;
    const u32 *flags = b.flags + (size_t)s * kActions * b.chunk;
    const u32 p0 = prefix[0];
    // the first parent before whose pop max_states states are stored (agents.py:105); n_par: none
    if (threadIdx.x == 0) s_cut = n_par;
    __syncthreads();
    u32 cut = n_par;
    for (u32 j = threadIdx.x; j < n_par; j += kWave)
        if (n_nodes + (prefix[j * kActions] - p0) >= max_states) { cut = j; break; }   // (monotone in j: a lane's first is its least)
    if (cut < n_par) atomicMin(&s_cut, cut);
    __syncthreads();
    if (threadIdx.x != 0) return;
    cut = s_cut;
    const u32 rows = n_par * kActions;
    const unsigned long long fs = (unsigned long long)word(b, RC_BFSB_W_FIRST_SOLVED, s);
    word(b, RC_BFSB_W_C_ROWS, s) = 0;
    word(b, RC_BFSB_W_N_PAR, s) = 0;
    if (fs < (unsigned long long)kActions * cut) {   // solved before the cut (agents.py:111-116)
        word(b, RC_BFSB_W_NODES, s) = n_nodes + (prefix[fs] - p0);
        word(b, RC_BFSB_W_SOLVED_PARENT, s) = lo + (u32)fs / kActions;
        word(b, RC_BFSB_W_LAST_ACTION, s) = (u32)fs % kActions;
        word(b, RC_BFSB_W_QUEUE_LEN, s) = -1;
        word(b, RC_BFSB_W_STATUS, s) = RC_BFSB_SOLVED;
        return;
    }
    if (cut < n_par) {   // the cut falls inside the chunk
        word(b, RC_BFSB_W_NODES, s) = n_nodes + (prefix[cut * kActions] - p0);
        word(b, RC_BFSB_W_STATUS, s) = RC_BFSB_CUT;
        return;
    }
    const u32 n_new = prefix[rows - 1] + flags[rows - 1] - p0;
    if (n_new > rows) {   // (not a sum of this chunk's flags)
        word(b, RC_BFSB_W_STATUS, s) = RC_BFSB_FAILED;
        return;
    }
    word(b, RC_BFSB_W_C_ROWS, s) = rows;
    word(b, RC_BFSB_W_C_BASE, s) = n_nodes;
    word(b, RC_BFSB_W_C_LO, s) = lo;
    const u32 nodes_now = n_nodes + n_new, lo_now = lo + n_par;
    u32 end_now = level_end;
    word(b, RC_BFSB_W_NODES, s) = nodes_now;
    word(b, RC_BFSB_W_LO, s) = lo_now;
    if (lo_now == level_end) {
        if (nodes_now == lo_now) {   // nothing new in a whole level
            word(b, RC_BFSB_W_STATUS, s) = RC_BFSB_GRAPH_DONE;
            return;
        }
        end_now = nodes_now;
        word(b, RC_BFSB_W_LEVEL_END, s) = end_now;
        word(b, RC_BFSB_W_LEVELS, s) += 1;
    }
    next_chunk(b, s, nodes_now, lo_now, end_now);
}

// appends the new states of the slots whose decision was to commit, in row order, and finalises their hash cells
__global__ __launch_bounds__(kBlock) void k_bfsb_commit(rc_bfs_batch_t b, u32 rows) {
    const uint4 *child_keys = reinterpret_cast<const uint4 *>(b.child_keys);
    for (u32 r = blockIdx.x * kBlock + threadIdx.x; r < rows; r += gridDim.x * kBlock) {
        const u32 seg = kActions * b.chunk, s = r / seg, local = r - s * seg;
        if (local >= (u32)word(b, RC_BFSB_W_C_ROWS, s) || !b.flags[r]) continue;
        const u32 idx = (u32)word(b, RC_BFSB_W_C_BASE, s) + (b.prefix[r] - b.prefix[(size_t)s * seg]);
        const int cs = b.child_slot[r];
        if (idx >= b.capacity || cs >= 0) continue;   // (k_bfsb_decide allows a commit only where it fits)
        const size_t node = (size_t)s * b.capacity + idx;
        reinterpret_cast<uint4 *>(b.keys)[node] = child_keys[r];
        b.parent[node] = (u32)word(b, RC_BFSB_W_C_LO, s) + local / kActions;
        b.action[node] = (u8)(local % kActions);
        b.hash[(size_t)s * b.hash_size + ((u32)(-cs - 1) & (b.hash_size - 1))] = (int)idx + 1;
    }
}

// actions from the root to the solved state of the slots that have just solved, root first (agents.py:112-115).  A parent has
// a lower index than its child, which bounds the walk; anything else, or a chain that does not fit the row, fails the slot.
__global__ __launch_bounds__(kBlock) void k_bfsb_path(rc_bfs_batch_t b) {
    const u32 s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= b.n_slots) return;
    if (word(b, RC_BFSB_W_STATUS, s) != RC_BFSB_SOLVED || word(b, RC_BFSB_W_QUEUE_LEN, s) >= 0) return;
    const unsigned long long start = (unsigned long long)word(b, RC_BFSB_W_SOLVED_PARENT, s);
    const unsigned long long last = (unsigned long long)word(b, RC_BFSB_W_LAST_ACTION, s);
    const u32 *parent = b.parent + (size_t)s * b.capacity;
    const u8 *action = b.action + (size_t)s * b.capacity;
    bool ok = start < b.capacity && last < (unsigned long long)kActions;
    u32 depth = 0;
    for (u32 node = ok ? (u32)start : 0; ok && node != 0; ++depth) {
        const u32 p = parent[node];
        ok = p < node && depth + 1 < b.queue_width && action[node] < kActions;
        node = p;
    }
    if (!ok) {
        word(b, RC_BFSB_W_QUEUE_LEN, s) = 0;
        word(b, RC_BFSB_W_STATUS, s) = RC_BFSB_FAILED;
        return;
    }
    u8 *row = b.queues + (size_t)s * b.queue_width;
    u32 node = (u32)start;
    for (u32 i = depth; i > 0; --i) {   // (the chain the loop above has checked)
        row[i - 1] = action[node];
        node = parent[node];
    }
    row[depth] = (u8)last;
    word(b, RC_BFSB_W_QUEUE_LEN, s) = depth + 1;
}

static int check_bfs_batch(const rc_bfs_batch_t *b) {
    RC_REQUIRE(b != nullptr, RC_ERR_NULL);
    RC_REQUIRE(b->keys && b->parent && b->action && b->hash && b->child_keys && b->child_slot && b->flags && b->prefix && b->words &&
                   b->queues && b->scan_tmp,
               RC_ERR_NULL);
    RC_REQUIRE(aligned16(b->keys) && aligned16(b->child_keys) && aligned16(b->hash), RC_ERR_ALIGN);
    RC_REQUIRE((reinterpret_cast<uintptr_t>(b->words) & 7u) == 0, RC_ERR_ALIGN);
    RC_REQUIRE(b->n_slots >= 1 && b->chunk >= 1 && b->queue_width >= 1, RC_ERR_RANGE);
    RC_REQUIRE((unsigned long long)b->n_slots * kActions * b->chunk < (1ull << 31), RC_ERR_RANGE);
    RC_REQUIRE((unsigned long long)b->capacity >= (unsigned long long)kActions * b->chunk + 2 && b->capacity < (1u << 30), RC_ERR_RANGE);
    RC_REQUIRE(b->hash_size >= 32 && (b->hash_size & (b->hash_size - 1)) == 0, RC_ERR_RANGE);
    RC_REQUIRE((unsigned long long)b->capacity * 2 <= b->hash_size, RC_ERR_RANGE);
    return RC_OK;
}

}  // namespace rubiks

using namespace rubiks;

extern "C" {

size_t rc_bfs_batch_struct_bytes(void) { return sizeof(rc_bfs_batch_t); }

size_t rc_bfs_batch_scan_bytes(uint32_t n_slots, uint32_t chunk) {
    const unsigned long long rows = (unsigned long long)n_slots * kActions * chunk;
    if (rows == 0 || rows >= (1ull << 31)) return 0;
    size_t bytes = 0;
    const u32 *in = nullptr;
    u32 *out = nullptr;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)rows) != hipSuccess) return 0;
    return round_up(bytes ? bytes : 16, 256);
}

// agents.py:92-103 (`search` up to its loop) for the listed slots
int rc_bfs_batch_plant(const rc_bfs_batch_t *b, const int32_t *slots, uint32_t n, const int8_t *roots_soa, size_t stride,
                       size_t first_col, const uint32_t *max_states, rc_stream_t stream) {
    if (int rc = check_bfs_batch(b)) return rc;
    RC_REQUIRE(slots && roots_soa && max_states, RC_ERR_NULL);
    RC_REQUIRE(aligned16(roots_soa) && (stride & 15u) == 0 && (reinterpret_cast<uintptr_t>(max_states) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(slots) & 3u) == 0,
               RC_ERR_ALIGN);
    RC_REQUIRE(n <= b->n_slots && first_col <= stride && stride - first_col >= n, RC_ERR_RANGE);
    if (n == 0) return RC_OK;
    const unsigned y = (unsigned)std::min<size_t>(64, ceil_div(b->hash_size / 4, (size_t)kBlock * 4));
    hipLaunchKernelGGL(k_bfsb_plant, dim3(n, y), dim3(kBlock), 0, (hipStream_t)stream, *b, (const int *)slots, (const u8 *)roots_soa, stride,
                       first_col, max_states);
    return launch_status();
}

// agents.py:104-129 for the next chunk of every running slot
int rc_bfs_batch_step(const rc_bfs_batch_t *b, rc_stream_t stream) {
    if (int rc = check_bfs_batch(b)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const u32 rows = b->n_slots * kActions * b->chunk;
    const unsigned grid = grid_for(rows);
    k_bfsb_children<<<grid, kBlock, 0, st>>>(*b, rows);
    k_bfsb_claim<<<grid, kBlock, 0, st>>>(*b, rows);
    k_bfsb_flags<<<grid, kBlock, 0, st>>>(*b, rows);
    size_t bytes = b->scan_tmp_bytes;
    if (hipError_t e = hipcub::DeviceScan::ExclusiveSum(b->scan_tmp, bytes, b->flags, b->prefix, (int)rows, st); e != hipSuccess)
        return hip_rc(e);
    k_bfsb_decide<<<b->n_slots, kWave, 0, st>>>(*b);
    k_bfsb_commit<<<grid, kBlock, 0, st>>>(*b, rows);
    k_bfsb_path<<<grid_for(b->n_slots, kBlock, 1 << 30), kBlock, 0, st>>>(*b);
    return launch_status();
}

}  // extern "C"
