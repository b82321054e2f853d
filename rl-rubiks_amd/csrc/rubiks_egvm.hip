// Batched EGVM for MI355X (gfx950): S games of W epsilon-greedy rollouts each, advanced in lock step without the host.
// Restates the per-game semantics of the reference's agent (librubiks/solving/agents.py:649-726) exactly: the actions are the
// host's random draws or NumPy's argmax of the policy logits, the first solved worker of the first solved depth ends a game,
// and a round without one jumps to np.argmax of the visited states' values in worker-major order.
//
// This is byte work beside the network (about 100 B per row and step against 24.9 MFLOP): what the kernels buy is a round of
// D steps with no host round trip in it.  Rows are few (S W: hundreds to half a million), so rc_egvm_step gives every lane one
// dword of each SoA plane -- four consecutive rows, a wave covers 256 contiguous bytes of a plane -- rather than the 16 bytes per
// lane of the streaming environment kernels: at 640 rows that is three waves at work instead of one.
#include <limits.h>

#include "rubiks_common.h"
#include "rubiks_rollout.h"

namespace rubiks {

// ---- one depth step (agents.py:690-716) ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_egvm_step(rc_egvm_t e, u32 d, const u8 *__restrict__ dec, const void *__restrict__ head,
                                                      size_t ld, bool bf16) {
    __shared__ u32 s_lut[sizeof(kTables.lut) / 4];
    stage_to_lds(s_lut, c_tables.lut, sizeof(kTables.lut));
    __syncthreads();
    const u8 *lut = reinterpret_cast<const u8 *>(s_lut);
    const u32 W = e.workers, D = e.depth;
    const size_t R = (size_t)e.n_slots * W;
    const size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x;   // this lane's dword of every plane: rows 4 q .. 4 q + 3
    if (4 * q >= R) return;

    u32 abase[4], live = 0, take = 0, slot[4], worker[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const size_t r = 4 * q + c;
        u32 a = kActions;   // identity padding of the move table: rows that are not played keep their state
        slot[c] = worker[c] = 0;
        if (r < R) {
            const u32 g = (u32)(r / W);
            slot[c] = g;
            worker[c] = (u32)(r - (size_t)g * W);
            // a game that was hit at an earlier depth is frozen for the rest of the round (agents.py:710-713 returns there); claims
            // of THIS depth, which other workgroups may be making right now, leave the test as it is
            if (e.status[g] == RC_EGVM_RUNNING && (e.hit[g] >> 16) >= d) {
                live |= 1u << c;
                if (d > 0) {   // this forward's value belongs to the state reached at depth d - 1 (row w D + d - 1 of agents.py:681-682)
                    const float v = egvm_head_elem(head, r * ld + kActions, bf16);
                    if (e.best_depth[r] < 0 || egvm_better(v, e.best_value[r])) {
                        e.best_value[r] = v;
                        e.best_depth[r] = (int)d - 1;
                        take |= 1u << c;
                    }
                }
                a = dec[r];
                if (a >= (u32)kActions) {   // RC_EGVM_POLICY: logits.argmax (agents.py:700-703), first maximum, a NaN is the maximum
                    float best = egvm_head_elem(head, r * ld, bf16);
                    a = 0;
                    if (!isnan(best)) {
                        for (u32 k = 1; k < (u32)kActions; ++k) {
                            const float x = egvm_head_elem(head, r * ld + k, bf16);
                            if (isnan(x)) { a = k; break; }
                            if (x > best) { best = x; a = k; }
                        }
                    }
                }
                e.paths[r * D + d] = (u8)a;   // agents.py:705
            }
        }
        abase[c] = a * (2 * kCodePad);
    }
    if (!live) return;

    const size_t sdw = e.stride / 4;
    u32 *rows = reinterpret_cast<u32 *>(e.rows_soa) + q;
    u32 *best = reinterpret_cast<u32 *>(e.best_soa) + q;
    u32 tmask = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) tmask |= ((take >> c) & 1u) * (0xffu << (8 * c));
    u32 same = 0xf;
#pragma unroll
    for (int j = 0; j < kPlanes; ++j) {
        const int kofs = (j >= kCorners) ? kCodePad : 0;
        const u32 v = rows[(size_t)j * sdw];
        if (tmask) best[(size_t)j * sdw] = (tmask == 0xffffffffu) ? v : ((best[(size_t)j * sdw] & ~tmask) | (v & tmask));
        u32 out = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u32 code = lut[abase[c] + kofs + code_of(v, c)];
            out |= code << (8 * c);
            if (code != (u32)(u8)kTables.solved[j]) same &= ~(1u << c);
        }
        rows[(size_t)j * sdw] = out;
    }
    same &= live;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if ((same >> c) & 1u) atomicMin(&e.hit[slot[c]], (d << 16) | worker[c]);   // first depth, then lowest worker (agents.py:710-713)
}

// ---- end of a round (agents.py:666-677, 710-713): one workgroup per game ---------------------------------------------------
// b's candidate (value, worker) beats a's in np.argmax's order: a NaN before everything, then the greater value, then the lower worker
__device__ __forceinline__ bool egvm_wins(float bv, int bw, float av, int aw) {
    if (bw == INT_MAX) return false;
    if (aw == INT_MAX) return true;
    const bool an = isnan(av), bn = isnan(bv);
    if (an != bn) return bn;
    if (an) return bw < aw;
    return bv > av || (bv == av && bw < aw);
}

__global__ __launch_bounds__(kBlock) void k_egvm_round_end(rc_egvm_t e, const float *__restrict__ values_last, u64 max_states) {
    __shared__ float s_v[kBlock];
    __shared__ int s_w[kBlock];
    __shared__ u8 s_state[kPlanes];
    const u32 g = blockIdx.x, tid = threadIdx.x, W = e.workers, D = e.depth;
    const size_t row0 = (size_t)g * W;
    // (every condition below that guards a barrier is the same for the whole workgroup)
    const bool running = e.status[g] == RC_EGVM_RUNNING;
    const u32 h = e.hit[g];
    const bool was_hit = h != RC_EGVM_NO_HIT;
    const long long qlen = e.queue_len[g];
    __syncthreads();   // the words above are read before anybody rewrites them
    if (running) {
        u32 w_end, len;
        if (was_hit) {
            w_end = h & 0xffffu;
            len = (h >> 16) + 1;
        } else {
            float tv = 0.f;
            int tw = INT_MAX;
            for (u32 w = tid; w < W; w += kBlock) {   // ascending w per thread: a strictly better value replaces, so the lowest worker stays
                const size_t r = row0 + w;
                float v = e.best_value[r];
                const float last = values_last[r];   // the state after the last depth: row w D + D - 1
                if (e.best_depth[r] < 0 || egvm_better(last, v)) {
                    v = last;
                    e.best_value[r] = v;
                    e.best_depth[r] = (int)D - 1;
                }
                if (tw == INT_MAX || egvm_better(v, tv)) { tv = v; tw = (int)w; }
            }
            s_v[tid] = tv;
            s_w[tid] = tw;
            __syncthreads();
            for (u32 s = kBlock / 2; s > 0; s >>= 1) {
                if (tid < s && egvm_wins(s_v[tid + s], s_w[tid + s], s_v[tid], s_w[tid])) {
                    s_v[tid] = s_v[tid + s];
                    s_w[tid] = s_w[tid + s];
                }
                __syncthreads();
            }
            w_end = (u32)s_w[0];                        // np.argmax over w D + d (agents.py:674)
            len = (u32)e.best_depth[row0 + w_end] + 1;  // (written by this workgroup before the barriers above)
        }
        const bool fits = (u64)qlen + len <= e.queue_width;
        if (fits) {
            const u8 *path = e.paths + (row0 + w_end) * D;
            u8 *queue = e.queues + (size_t)g * e.queue_width + qlen;
            for (u32 i = tid; i < len; i += kBlock) queue[i] = path[i];   // agents.py:677,712
            if (!was_hit) {   // every worker of the next round starts from the best state (agents.py:675-676,679)
                const u8 *src = reinterpret_cast<const u8 *>(len == D ? e.rows_soa : e.best_soa) + row0 + w_end;
                if (tid < (u32)kPlanes) s_state[tid] = src[(size_t)tid * e.stride];
                __syncthreads();
                if (tid < (u32)kPlanes) e.current[(size_t)g * kPlanes + tid] = (int8_t)s_state[tid];
                for (u32 i = tid; i < W * (u32)kPlanes; i += kBlock) {
                    const u32 j = i / W, w = i - j * W;
                    e.rows_soa[(size_t)j * e.stride + row0 + w] = (int8_t)s_state[j];
                }
            }
        }
        if (tid == 0) {
            if (!fits) {
                e.status[g] = RC_EGVM_QUEUE_FULL;
            } else {
                const long long nodes = e.nodes[g] + (was_hit ? (long long)len * W : (long long)W * D);   // agents.py:672,711
                e.nodes[g] = nodes;
                e.queue_len[g] = qlen + len;
                e.rounds[g] += 1;
                if (was_hit) e.status[g] = RC_EGVM_SOLVED;
                else if ((u64)nodes + (u64)W * D > max_states) e.status[g] = RC_EGVM_EXHAUSTED;   // agents.py:665
            }
        }
    }
    __syncthreads();
    for (u32 w = tid; w < W; w += kBlock) e.best_depth[row0 + w] = -1;
    if (tid == 0) e.hit[g] = RC_EGVM_NO_HIT;
}

// ---- plant: listed slots restart from new roots.  One workgroup per listed slot ------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_egvm_plant(rc_egvm_t e, const int *__restrict__ slots, const u8 *__restrict__ roots,
                                                       size_t stride, size_t first_col) {
    __shared__ u8 s_state[kPlanes];
    const int s = slots[blockIdx.x];
    if (s < 0 || (u32)s >= e.n_slots) return;   // (the whole workgroup: nothing is written for a slot that does not exist)
    const u32 tid = threadIdx.x, W = e.workers;
    const size_t row0 = (size_t)s * W;
    if (tid < (u32)kPlanes) s_state[tid] = roots[(size_t)tid * stride + first_col + blockIdx.x] & 31u;
    __syncthreads();
    if (tid < (u32)kPlanes) e.current[(size_t)s * kPlanes + tid] = (int8_t)s_state[tid];
    for (u32 i = tid; i < W * (u32)kPlanes; i += kBlock) {
        const u32 j = i / W, w = i - j * W;
        e.rows_soa[(size_t)j * e.stride + row0 + w] = (int8_t)s_state[j];
    }
    for (u32 w = tid; w < W; w += kBlock) e.best_depth[row0 + w] = -1;
    if (tid == 0) {
        bool solved = true;
        for (int j = 0; j < kPlanes; ++j) solved &= s_state[j] == (u8)kTables.solved[j];
        e.status[s] = solved ? RC_EGVM_ROOT_SOLVED : RC_EGVM_RUNNING;   // agents.py:661
        e.nodes[s] = 0;
        e.queue_len[s] = 0;
        e.rounds[s] = 0;
        e.hit[s] = RC_EGVM_NO_HIT;
    }
}

}  // namespace rubiks

using namespace rubiks;

static int check_egvm(const rc_egvm_t *e) {
    RC_REQUIRE(e != nullptr, RC_ERR_NULL);
    RC_REQUIRE(e->rows_soa && e->best_soa && e->best_value && e->best_depth && e->paths && e->hit && e->current && e->queues &&
                   e->status && e->nodes && e->queue_len && e->rounds,
               RC_ERR_NULL);
    RC_REQUIRE(e->n_slots > 0 && e->workers > 0 && e->workers <= 0xffffu && e->depth > 0 && e->depth <= 0x8000u && e->queue_width > 0,
               RC_ERR_RANGE);
    RC_REQUIRE((size_t)e->n_slots * e->workers <= (size_t)1 << 30, RC_ERR_RANGE);
    RC_REQUIRE(aligned16(e->rows_soa) && aligned16(e->best_soa) && (e->stride & 15u) == 0, RC_ERR_ALIGN);
    RC_REQUIRE(e->stride >= round_up((size_t)e->n_slots * e->workers, 16), RC_ERR_STRIDE);
    return RC_OK;
}

extern "C" {

// agents.py:690-716 (one iteration of the depth loop of `_expand`, for every game of the batch)
int rc_egvm_step(const rc_egvm_t *e, uint32_t d, const uint8_t *decisions_row, const void *head, size_t ld, int head_is_bf16,
                 rc_stream_t stream) {
    if (int rc = check_egvm(e)) return rc;
    RC_REQUIRE(decisions_row && head, RC_ERR_NULL);
    RC_REQUIRE((reinterpret_cast<uintptr_t>(head) & (head_is_bf16 ? 1u : 3u)) == 0, RC_ERR_ALIGN);
    RC_REQUIRE(d < e->depth && ld >= (size_t)kActions + 1, RC_ERR_RANGE);
    const size_t dwords = ceil_div((size_t)e->n_slots * e->workers, 4);
    hipLaunchKernelGGL(k_egvm_step, dim3(grid_for(dwords, kBlock, 1 << 30)), dim3(kBlock), 0, (hipStream_t)stream, *e, d, decisions_row,
                       head, ld, head_is_bf16 != 0);
    return launch_status();
}

// agents.py:666-677 (the jump to the best visited state) and :710-713 (a solved worker ends the game)
int rc_egvm_round_end(const rc_egvm_t *e, const float *values_last, uint64_t max_states, rc_stream_t stream) {
    if (int rc = check_egvm(e)) return rc;
    RC_REQUIRE(values_last, RC_ERR_NULL);
    RC_REQUIRE((reinterpret_cast<uintptr_t>(values_last) & 3u) == 0, RC_ERR_ALIGN);
    hipLaunchKernelGGL(k_egvm_round_end, dim3(e->n_slots), dim3(kBlock), 0, (hipStream_t)stream, *e, values_last, (u64)max_states);
    return launch_status();
}

// agents.py:657-663 (`search` up to its loop) for the listed slots
int rc_egvm_plant(const rc_egvm_t *e, const int32_t *slots, uint32_t n, const int8_t *roots_soa, size_t stride, size_t first_col,
                  rc_stream_t stream) {
    if (int rc = check_egvm(e)) return rc;
    RC_REQUIRE(slots && roots_soa, RC_ERR_NULL);
    RC_REQUIRE(aligned16(roots_soa) && (stride & 15u) == 0, RC_ERR_ALIGN);
    RC_REQUIRE(n <= e->n_slots && stride >= first_col + n, RC_ERR_RANGE);
    if (n == 0) return RC_OK;
    hipLaunchKernelGGL(k_egvm_plant, dim3(n), dim3(kBlock), 0, (hipStream_t)stream, *e, (const int *)slots, (const u8 *)roots_soa, stride,
                       first_col);
    return launch_status();
}

// agents.py:694-698 for one round of the listed games (host only: nothing is launched)
int rc_egvm_draw(uint32_t *mt_keys, int32_t *mt_pos, uint32_t n_games, const int32_t *games, const int32_t *slots, uint32_t n,
                 double cdf0, uint32_t workers, uint32_t depth, uint8_t *table, size_t table_stride, size_t n_rows) {
    RC_REQUIRE(mt_keys && mt_pos && table, RC_ERR_NULL);
    RC_REQUIRE(n == 0 || (games && slots), RC_ERR_NULL);
    RC_REQUIRE(workers > 0 && workers <= 0xffffu && depth > 0 && depth <= 0x8000u && table_stride >= n_rows, RC_ERR_RANGE);
    for (u32 i = 0; i < n; ++i) {
        RC_REQUIRE(games[i] >= 0 && (u32)games[i] < n_games && slots[i] >= 0 && ((size_t)slots[i] + 1) * workers <= n_rows, RC_ERR_RANGE);
        RC_REQUIRE(mt_pos[games[i]] >= 0 && mt_pos[games[i]] <= 624, RC_ERR_RANGE);
    }
    for (u32 i = 0; i < n; ++i) {
        Mt19937 mt{mt_keys + (size_t)games[i] * 624, mt_pos[games[i]]};
        for (u32 d = 0; d < depth; ++d) {
            u8 *row = table + (size_t)d * table_stride + (size_t)slots[i] * workers;
            for (u32 w = 0; w < workers; ++w) {
                const u32 a = mt.next() >> 5, b = mt.next() >> 6;
                const double u = (a * 67108864.0 + b) / 9007199254740992.0;
                row[w] = u >= cdf0 ? 0 : RC_EGVM_POLICY;
            }
            for (u32 w = 0; w < workers; ++w) {
                if (row[w] == RC_EGVM_POLICY) continue;
                u32 v;
                do v = mt.next() & 15u; while (v > 11u);
                row[w] = (u8)v;
            }
        }
        mt_pos[games[i]] = mt.pos;
    }
    return RC_OK;
}

}  // extern "C"
