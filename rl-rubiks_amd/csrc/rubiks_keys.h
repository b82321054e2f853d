// Packed node states and the per-game open-addressing tables over them, shared by the search translation units (rubiks_mcts,
// rubiks_astar, rubiks_bfs, rubiks_bfs_batch, rubiks_shorten).
// A node's state is stored packed: 20 codes of 5 bits, 6 per dword (cubies 0-5, 6-11, 12-17, 18-19).  A table is a power-of-two row
// of int cells probed linearly from key_hash & mask: 0 = free, c > 0 = a node, c < 0 = the pending row -(c + 1) of the launch that
// is filling it.  What a lookup does with a cell that is none of these is the caller's policy: the loops that report one
// (k_bfsb_children, k_mcts_complete_graph, rubiks_shorten.hip, k_mcts_rehash) are spelled out where they report it.
#pragma once
#include "rubiks_common.h"

namespace rubiks {

__device__ __forceinline__ bool key_eq(const uint4 &a, const uint4 &b) {
    return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
}

__device__ __forceinline__ u32 key_hash(const uint4 &k) {
    u32 h = k.x * 0x9E3779B1u;
    h ^= h >> 15;
    h += k.y * 0x85EBCA77u;
    h ^= h >> 13;
    h += k.z * 0xC2B2AE3Du;
    h ^= h >> 16;
    h += k.w * 0x27D4EB2Fu;
    h ^= h >> 15;
    h *= 0x165667B1u;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ u32 key_code(const uint4 &k, int j) {   // j compile-time after unrolling
    const u32 w = (j < 6) ? k.x : (j < 12) ? k.y : (j < 18) ? k.z : k.w;
    return (w >> (5 * (j % 6))) & 31u;
}

__device__ __forceinline__ void key_set(u32 (&w)[4], int j, u32 code) { w[j / 6] |= code << (5 * (j % 6)); }

constexpr uint4 solved_key() {
    u32 w[4] = {0, 0, 0, 0};
    for (int j = 0; j < kPlanes; ++j) w[j / 6] |= (u32)(u8)kTables.solved[j] << (5 * (j % 6));
    return uint4{w[0], w[1], w[2], w[3]};
}

__device__ __forceinline__ bool key_is_solved(const uint4 &k) {
    constexpr uint4 s = solved_key();
    return k.x == s.x && k.y == s.y && k.z == s.z && k.w == s.w;
}

// Key of the cube in column `col` of a batch stored plane by plane (20 rows of `stride` bytes); a 20-byte state is stride 1, column 0.
__device__ __forceinline__ uint4 key_from_column(const u8 *soa, size_t stride, size_t col) {
    u32 w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < kPlanes; ++j) key_set(w, j, soa[(size_t)j * stride + col] & 31u);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// ... and a key's 20 codes written to such a column (int8_t or uint8_t planes)
__device__ __forceinline__ void key_to_column(const uint4 &k, void *soa, size_t stride, size_t col) {
#pragma unroll
    for (int j = 0; j < kPlanes; ++j) static_cast<u8 *>(soa)[(size_t)j * stride + col] = (u8)key_code(k, j);
}

// Key of child `a` of the state `pk`; `lut`: MoveTables::lut staged in LDS.
__device__ __forceinline__ uint4 key_turned(const uint4 &pk, u32 a, const u8 *lut) {
    u32 w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < kPlanes; ++j) key_set(w, j, lut[a * (2 * kCodePad) + (j >= kCorners ? kCodePad : 0) + key_code(pk, j)]);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// A kBlock workgroup zeroes a game's table row with 16-byte stores (`cells`: a multiple of 4, the row 16-byte aligned).  The caller
// holds the barrier before anyone reads the row.
__device__ __forceinline__ void hash_row_clear(int *row, u32 cells) {
    uint4 *row4 = reinterpret_cast<uint4 *>(row);
    for (u32 i = threadIdx.x; i < cells / 4; i += kBlock) row4[i] = make_uint4(0, 0, 0, 0);
}

// The node of `ck` in a table that holds nothing but free cells and nodes (keys[c]: the key of cell value c), or 0 with `h` the
// free cell where the probe stopped.
__device__ __forceinline__ int key_find(const int *tab, u32 mask, const uint4 *keys, const uint4 &ck, u32 &h) {
    h = key_hash(ck) & mask;
    for (;;) {
        const int c = tab[h];
        if (c == 0) return 0;
        if (key_eq(keys[c], ck)) return c;
        h = (h + 1) & mask;
    }
}

// First-occurrence election among the rows of one launch whose state `key_find` did not find: row r (`mine` = -(r + 1), key `ck`
// = key_of_row[r]) probes on from cell `h` and claims the first free cell, or joins the pending row with its state there; atomicMax
// then leaves the lowest such row in the cell.  Returns that cell.  The probe ends within the table, and a cell is taken for a
// pending row only if it names one below n_rows.
__device__ __forceinline__ u32 claim_lowest_row(int *tab, u32 h, u32 mask, int mine, u32 n_rows, const uint4 *key_of_row,
                                                const uint4 &ck) {
    h &= mask;
    for (u32 probes = 0; probes <= mask; ++probes) {
        int c = __hip_atomic_load(&tab[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == 0) {
            c = atomicCAS(&tab[h], 0, mine);
            if (c == 0) break;
        }
        if (c < 0 && (u32)(-(c + 1)) < n_rows && key_eq(key_of_row[(u32)(-(c + 1))], ck)) {
            atomicMax(&tab[h], mine);   // -(row+1): the larger value is the smaller row
            break;
        }
        h = (h + 1) & mask;   // another state (a node or another pending row)
    }
    return h;
}

}  // namespace rubiks
