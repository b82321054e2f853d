// Lookups in the near-solved table (rc_near_t, include/rubiks_hip.h), shared by the translation units that read it: rubiks_near.hip
// (build, depth, solve, tighten) and rubiks_near_reach.hip (the forward half of the bidirectional search).  The table's cells are
// those of rubiks_keys.h (0 = free, c > 0 = node c - 1).  Every probe is bounded by the table's size, and every cell and meta byte
// read from memory is range-checked before it addresses anything.
#pragma once
#include "rubiks_keys.h"

namespace rubiks {

constexpr u32 kA = kActions;

// Node of `ck` (>= 0), -1 if the state is not in the table, -2 if a cell on the way names no node of the table or the probe went
// round the table.  Split in two so that a lane can issue the first reads of several lookups before it waits for any.
__device__ __forceinline__ u32 near_home(const rc_near_t &t, const uint4 &ck) { return key_hash(ck) & (t.hash_size - 1); }

__device__ __forceinline__ int near_finish(const rc_near_t &t, const uint4 &ck, u32 h, int c) {
    const uint4 *keys = reinterpret_cast<const uint4 *>(t.keys);
    const u32 mask = t.hash_size - 1;
    for (u32 probes = 0; probes <= mask; ++probes) {
        if (c == 0) return -1;
        if (c < 0 || (u32)c > t.n_nodes) return -2;
        if (key_eq(keys[c - 1], ck)) return c - 1;
        h = (h + 1) & mask;
        c = t.hash[h];
    }
    return -2;
}

__device__ __forceinline__ int near_find(const rc_near_t &t, const uint4 &ck) {
    const u32 h = near_home(t, ck);
    return near_finish(t, ck, h, t.hash[h]);
}

// depth of a node found by near_find, -2 if its meta byte is not one the build writes
__device__ __forceinline__ int near_depth_of(const rc_near_t &t, int node) {
    const u32 m = t.meta[node];
    return ((m >> 4) <= t.depth && (m & 15u) < kA) ? (int)(m >> 4) : -2;
}

// a_1 .. a_d of the state `key` at node `node`, depth d: walking back gives a_d first.  write(s, a): s = 0 for a_d.  false: a
// state on the way is not in the table at the depth it must have.
template <typename Write>
__device__ __forceinline__ bool near_walk_back(const rc_near_t &t, uint4 key, int node, int d, const u8 *lut, Write write) {
    for (int s = 0; s < d; ++s) {
        const u32 a = t.meta[node] & 15u;
        write(s, a);
        if (s + 1 == d) break;
        key = key_turned(key, a ^ 1u, lut);
        node = near_find(t, key);
        if (node < 0 || near_depth_of(t, node) != d - 1 - s) return false;
    }
    return true;
}

// What every entry point that reads or builds the table requires of the struct (host).
inline int check_near(const rc_near_t *t, bool building) {
    RC_REQUIRE(t != nullptr, RC_ERR_NULL);
    RC_REQUIRE(t->keys && t->meta && t->hash, RC_ERR_NULL);
    RC_REQUIRE(aligned16(t->keys), RC_ERR_ALIGN);
    RC_REQUIRE(t->depth >= 1 && t->depth <= (u32)RC_NEAR_MAX_DEPTH, RC_ERR_RANGE);
    RC_REQUIRE(t->capacity >= 1 && t->capacity < (1u << 30), RC_ERR_RANGE);
    RC_REQUIRE(t->hash_size >= 2 && t->hash_size <= (1u << 30) && (t->hash_size & (t->hash_size - 1)) == 0, RC_ERR_RANGE);
    RC_REQUIRE((unsigned long long)t->capacity * 2 <= t->hash_size, RC_ERR_RANGE);
    RC_REQUIRE(t->n_nodes <= t->capacity, RC_ERR_RANGE);
    if (building) {
        RC_REQUIRE(t->words && t->child_keys && t->child_slot && t->flags && t->prefix && t->scan_tmp, RC_ERR_NULL);
        RC_REQUIRE(aligned16(t->child_keys), RC_ERR_ALIGN);
        RC_REQUIRE(t->chunk_rows >= kA && t->chunk_rows < (1u << 30), RC_ERR_RANGE);
    } else {
        RC_REQUIRE(t->n_nodes >= 1, RC_ERR_RANGE);
    }
    return RC_OK;
}

}  // namespace rubiks
