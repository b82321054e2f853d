// The one-step agents for MI355X (gfx950): S games of RandomSearch, PolicySearch or ValueSearch, one move per launch, without the
// host.  Restates the reference's `Agent.search` loop with the three `_step`s (librubiks/solving/agents.py:23-38, 82-90, 132-169)
// per game: the action is the host's draw, NumPy's argmax of the policy logits, np.random.choice of their softmax for the
// host's uniform, or the first solved child / np.argmax of the children's values.
//
// Byte work beside the network, as in rubiks_egvm.hip, and the same layout: a lane owns one dword of every SoA plane, which is
// four consecutive games, and the move table is in LDS; a game that is not played is turned by the identity action.  The value
// step also writes the 12 children of the four new states -- 48 contiguous bytes of every child plane -- so that a value move
// is the value network on 12 S rows plus one launch.
#include "rubiks_common.h"
#include "rubiks_rollout.h"

namespace rubiks {

// np.random.choice(12, p=softmax(logits)) for its one uniform u (agents.py:139-140): p is the fp32 softmax, choice normalises
// the double cumulative sum of p and answers cdf.searchsorted(u, side="right").  12: a probability is NaN (NumPy raises).
__device__ __forceinline__ u32 rollout_sample12(const void *head, size_t i0, bool bf16, double u) {
    float x[kActions];
#pragma unroll
    for (int k = 0; k < kActions; ++k) x[k] = egvm_head_elem(head, i0 + k, bf16);
    float m = x[0];
#pragma unroll
    for (int k = 1; k < kActions; ++k) m = fmaxf(m, x[k]);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kActions; ++k) {
        x[k] = expf(x[k] - m);
        s += x[k];
    }
    double cdf[kActions], c = 0.0;
    bool nan = false;
#pragma unroll
    for (int k = 0; k < kActions; ++k) {
        const float p = x[k] / s;
        nan |= isnan(p);
        c += (double)p;
        cdf[k] = c;
    }
    if (nan) return kActions;
    u32 a = 0;
#pragma unroll
    for (int k = 0; k < kActions; ++k) a += (cdf[k] / c <= u) ? 1u : 0u;
    return a < (u32)kActions ? a : (u32)kActions - 1;
}

// The bookkeeping of one move of game g, whose action is `a` (agents.py:32): false if the game cannot make it.
__device__ __forceinline__ bool rollout_append(const rc_rollout_t &r, size_t g, long long n, u32 a) {
    if (a >= (u32)kActions) {
        r.status[g] = RC_ROLLOUT_BAD_POLICY;
        return false;
    }
    r.queues[g * r.queue_width + (size_t)n] = (u8)a;
    r.steps[g] = n + 1;
    return true;
}

// ---- RandomSearch._step / PolicySearch._step (agents.py:83-86, 138-142) ---------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rollout_step_policy(rc_rollout_t r, const void *__restrict__ head, size_t ld, bool bf16,
                                                                const u8 *__restrict__ dec, const double *__restrict__ uni,
                                                                u64 max_steps) {
    __shared__ u32 s_lut[sizeof(kTables.lut) / 4];
    stage_to_lds(s_lut, c_tables.lut, sizeof(kTables.lut));
    __syncthreads();
    const u8 *lut = reinterpret_cast<const u8 *>(s_lut);
    const size_t S = r.n_slots;
    const size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x;   // this lane's dword of every plane: games 4 q .. 4 q + 3
    if (4 * q >= S) return;

    u32 acts = 0, live = 0, last = 0;
    for (int c = 0; c < 4; ++c) {
        const size_t g = 4 * q + c;
        u32 a = kActions;   // identity padding of the move table: games that are not played keep their state
        if (g < S && r.status[g] == RC_ROLLOUT_RUNNING) {
            const long long n = r.steps[g];
            if ((u64)n >= r.queue_width) {
                r.status[g] = RC_ROLLOUT_QUEUE_FULL;
            } else {
                u32 want = dec ? dec[g] : (u32)RC_ROLLOUT_POLICY;
                if (want >= (u32)kActions && head) want = uni ? rollout_sample12(head, g * ld, bf16, uni[g]) : egvm_argmax12(head, g * ld, 1, bf16);
                if (rollout_append(r, g, n, want)) {
                    a = want;
                    live |= 1u << c;
                    if ((u64)n + 1 >= max_steps) last |= 1u << c;
                }
            }
        }
        acts |= a << (8 * c);
    }
    if (!live) return;

    const size_t sdw = r.stride / 4;
    u32 *rows = reinterpret_cast<u32 *>(r.states_soa) + q;
    u32 same = 0xf;
#pragma unroll
    for (int j = 0; j < kPlanes; ++j) {
        const int kofs = (j >= kCorners) ? kCodePad : 0;
        const u32 v = rows[(size_t)j * sdw];
        u32 out = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u32 code = lut[((acts >> (8 * c)) & 0xffu) * (2 * kCodePad) + kofs + code_of(v, c)];
            out |= code << (8 * c);
            if (code != (u32)(u8)kTables.solved[j]) same &= ~(1u << c);
        }
        rows[(size_t)j * sdw] = out;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!((live >> c) & 1u)) continue;
        if ((same >> c) & 1u) r.status[4 * q + c] = RC_ROLLOUT_SOLVED;            // agents.py:33-35
        else if ((last >> c) & 1u) r.status[4 * q + c] = RC_ROLLOUT_EXHAUSTED;
    }
}

// ---- ValueSearch._step (agents.py:156-166) and the children of the new states -----------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rollout_step_value(rc_rollout_t r, const float *__restrict__ values, u64 max_steps) {
    __shared__ u32 s_lut[sizeof(kTables.lut) / 4];
    __shared__ u32 s_lut4[sizeof(kTables.lut4) / 4];
    stage_to_lds(s_lut, c_tables.lut, sizeof(kTables.lut));
    stage_to_lds(s_lut4, c_tables.lut4, sizeof(kTables.lut4));
    __syncthreads();
    const u8 *lut = reinterpret_cast<const u8 *>(s_lut);
    const size_t S = r.n_slots;
    const size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (4 * q >= S) return;

    u32 acts = 0, live = 0, last = 0, won = 0;
    for (int c = 0; c < 4; ++c) {
        const size_t g = 4 * q + c;
        u32 a = kActions;
        if (g < S && r.status[g] == RC_ROLLOUT_RUNNING) {
            const long long n = r.steps[g];
            if ((u64)n >= r.queue_width) {
                r.status[g] = RC_ROLLOUT_QUEUE_FULL;
            } else {
                u32 want = kActions;
                for (u32 k = 0; k < (u32)kActions; ++k)
                    if (r.kid_solved[12 * g + k]) { want = k; break; }        // np.where(solutions)[0][0] (agents.py:160)
                if (want < (u32)kActions) won |= 1u << c;
                else want = egvm_argmax12(values, 12 * g, 1, false);         // agents.py:165
                if (rollout_append(r, g, n, want)) {
                    a = want;
                    live |= 1u << c;
                    if ((u64)n + 1 >= max_steps) last |= 1u << c;
                }
            }
        }
        acts |= a << (8 * c);
    }
    if (!live) return;

    const size_t sdw = r.stride / 4;
    u32 *rows = reinterpret_cast<u32 *>(r.states_soa) + q;
    u32 same[4] = {0xfffu, 0xfffu, 0xfffu, 0xfffu};   // per game: which of the 12 new children are the solved cube
#pragma unroll
    for (int j = 0; j < kPlanes; ++j) {
        const int kind = (j >= kCorners) ? 1 : 0;
        const u32 v = rows[(size_t)j * sdw];
        const u32 sol = (u32)(u8)kTables.solved[j];
        u32 out = 0, kd[12];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u32 code = lut[((acts >> (8 * c)) & 0xffu) * (2 * kCodePad) + kind * kCodePad + code_of(v, c)];
            out |= code << (8 * c);
            const u32 *row = s_lut4 + (kind * kCodePad + code) * (kActions / 4);   // the code under actions 0 .. 11
#pragma unroll
            for (int i = 0; i < kActions / 4; ++i) {
                const u32 w = row[i];
                kd[3 * c + i] = w;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (((w >> (8 * b)) & 0xffu) != sol) same[c] &= ~(1u << (4 * i + b));
            }
        }
        rows[(size_t)j * sdw] = out;   // the chosen child (agents.py:161,166) is the state under the chosen action
        uint4 *dst = reinterpret_cast<uint4 *>(r.kids_soa + (size_t)j * 12 * r.stride) + 3 * q;
        dst[0] = make_uint4(kd[0], kd[1], kd[2], kd[3]);
        dst[1] = make_uint4(kd[4], kd[5], kd[6], kd[7]);
        dst[2] = make_uint4(kd[8], kd[9], kd[10], kd[11]);
    }
    u32 fl[12];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            u32 w = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) w |= ((same[c] >> (4 * i + b)) & 1u) << (8 * b);
            fl[3 * c + i] = w;
        }
    uint4 *fdst = reinterpret_cast<uint4 *>(r.kid_solved) + 3 * q;
    fdst[0] = make_uint4(fl[0], fl[1], fl[2], fl[3]);
    fdst[1] = make_uint4(fl[4], fl[5], fl[6], fl[7]);
    fdst[2] = make_uint4(fl[8], fl[9], fl[10], fl[11]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!((live >> c) & 1u)) continue;
        if ((won >> c) & 1u) r.status[4 * q + c] = RC_ROLLOUT_SOLVED;             // agents.py:159-161
        else if ((last >> c) & 1u) r.status[4 * q + c] = RC_ROLLOUT_EXHAUSTED;
    }
}

// ---- plant: listed slots restart from new roots (agents.py:26-29).  One thread per listed slot ---------------------------------
__global__ __launch_bounds__(kWave) void k_rollout_plant(rc_rollout_t r, const int *__restrict__ slots, u32 n, const u8 *__restrict__ roots,
                                                         size_t stride, size_t first_col, bool with_children) {
    const u32 i = blockIdx.x * kWave + threadIdx.x;
    if (i >= n) return;
    const int s = slots[i];
    if (s < 0 || (u32)s >= r.n_slots) return;   // nothing is written for a slot that does not exist
    bool solved = true;
    u32 kids = 0xfffu;
    for (int j = 0; j < kPlanes; ++j) {
        const u32 code = roots[(size_t)j * stride + first_col + i] & 31u;
        const u32 sol = (u32)(u8)c_tables.solved[j];
        r.states_soa[(size_t)j * r.stride + s] = (int8_t)code;
        solved &= code == sol;
        if (with_children) {
            for (int k = 0; k < kActions; ++k) {
                const u32 kc = c_tables.lut4[j >= kCorners ? 1 : 0][code][k];
                r.kids_soa[(size_t)j * 12 * r.stride + (size_t)12 * s + k] = (int8_t)kc;
                if (kc != sol) kids &= ~(1u << k);
            }
        }
    }
    if (with_children)
        for (int k = 0; k < kActions; ++k) r.kid_solved[(size_t)12 * s + k] = (u8)((kids >> k) & 1u);
    r.status[s] = solved ? RC_ROLLOUT_ROOT_SOLVED : RC_ROLLOUT_RUNNING;
    r.steps[s] = 0;
}

}  // namespace rubiks

using namespace rubiks;

static int check_rollout(const rc_rollout_t *r, bool children) {
    RC_REQUIRE(r != nullptr, RC_ERR_NULL);
    RC_REQUIRE(r->states_soa && r->queues && r->status && r->steps, RC_ERR_NULL);
    RC_REQUIRE(!children || (r->kids_soa && r->kid_solved), RC_ERR_NULL);
    RC_REQUIRE(r->n_slots > 0 && r->n_slots <= 1u << 30 && r->queue_width > 0, RC_ERR_RANGE);
    RC_REQUIRE(aligned16(r->states_soa) && (r->stride & 15u) == 0, RC_ERR_ALIGN);
    RC_REQUIRE(!children || (aligned16(r->kids_soa) && aligned16(r->kid_solved)), RC_ERR_ALIGN);
    RC_REQUIRE(r->stride >= round_up((size_t)r->n_slots, 16), RC_ERR_STRIDE);
    return RC_OK;
}

extern "C" {

size_t rc_rollout_struct_bytes(void) { return sizeof(rc_rollout_t); }

// agents.py:26-29 (`search` up to its loop) for the listed slots
int rc_rollout_plant(const rc_rollout_t *r, const int32_t *slots, uint32_t n, const int8_t *roots_soa, size_t stride, size_t first_col,
                     int with_children, rc_stream_t stream) {
    if (int rc = check_rollout(r, with_children != 0)) return rc;
    RC_REQUIRE(slots && roots_soa, RC_ERR_NULL);
    RC_REQUIRE(aligned16(roots_soa) && (stride & 15u) == 0, RC_ERR_ALIGN);
    RC_REQUIRE(n <= r->n_slots && first_col <= stride && stride - first_col >= n, RC_ERR_RANGE);
    if (n == 0) return RC_OK;
    hipLaunchKernelGGL(k_rollout_plant, dim3((unsigned)ceil_div(n, kWave)), dim3(kWave), 0, (hipStream_t)stream, *r, (const int *)slots, n,
                       (const u8 *)roots_soa, stride, first_col, with_children != 0);
    return launch_status();
}

// agents.py:30-35 with RandomSearch._step (:83-86) or PolicySearch._step (:138-142): one iteration of the loop for every game
int rc_rollout_step_policy(const rc_rollout_t *r, const void *head, size_t ld, int head_is_bf16, const uint8_t *decisions_row,
                           const double *uniforms_row, uint64_t max_steps, rc_stream_t stream) {
    if (int rc = check_rollout(r, false)) return rc;
    RC_REQUIRE(head || decisions_row, RC_ERR_NULL);
    RC_REQUIRE(head || !uniforms_row, RC_ERR_NULL);
    RC_REQUIRE((reinterpret_cast<uintptr_t>(head) & (head_is_bf16 ? 1u : 3u)) == 0, RC_ERR_ALIGN);
    RC_REQUIRE((reinterpret_cast<uintptr_t>(uniforms_row) & 7u) == 0, RC_ERR_ALIGN);
    RC_REQUIRE((!head || ld >= (size_t)kActions + 1) && max_steps > 0, RC_ERR_RANGE);
    const size_t dwords = ceil_div((size_t)r->n_slots, 4);
    hipLaunchKernelGGL(k_rollout_step_policy, dim3(grid_for(dwords, kBlock, 1 << 30)), dim3(kBlock), 0, (hipStream_t)stream, *r, head, ld,
                       head_is_bf16 != 0, decisions_row, uniforms_row, (u64)max_steps);
    return launch_status();
}

// agents.py:30-35 with ValueSearch._step (:156-166)
int rc_rollout_step_value(const rc_rollout_t *r, const float *values, uint64_t max_steps, rc_stream_t stream) {
    if (int rc = check_rollout(r, true)) return rc;
    RC_REQUIRE(values, RC_ERR_NULL);
    RC_REQUIRE((reinterpret_cast<uintptr_t>(values) & 3u) == 0, RC_ERR_ALIGN);
    RC_REQUIRE(max_steps > 0, RC_ERR_RANGE);
    const size_t dwords = ceil_div((size_t)r->n_slots, 4);
    hipLaunchKernelGGL(k_rollout_step_value, dim3(grid_for(dwords, kBlock, 1 << 30)), dim3(kBlock), 0, (hipStream_t)stream, *r, values,
                       (u64)max_steps);
    return launch_status();
}

// np.random.seed(seed) right before a game (host only): MT19937's init_genrand, which RandomState runs for an integer seed
int rc_rollout_seed(uint32_t *mt_keys, int32_t *mt_pos, uint32_t n_games, const int32_t *games, uint32_t n, const int64_t *seeds) {
    RC_REQUIRE(mt_keys && mt_pos, RC_ERR_NULL);
    RC_REQUIRE(n == 0 || (games && seeds), RC_ERR_NULL);
    for (u32 i = 0; i < n; ++i)
        RC_REQUIRE(games[i] >= 0 && (u32)games[i] < n_games && seeds[games[i]] >= 0 && seeds[games[i]] <= 0xffffffffll, RC_ERR_RANGE);
    for (u32 i = 0; i < n; ++i) {
        u32 *key = mt_keys + (size_t)games[i] * 624;
        key[0] = (u32)seeds[games[i]];
        for (u32 k = 1; k < 624; ++k) key[k] = 1812433253u * (key[k - 1] ^ (key[k - 1] >> 30)) + k;
        mt_pos[games[i]] = 624;
    }
    return RC_OK;
}

// agents.py:84 (mode 0) and the uniform behind :140 (mode 1) for the next `steps` moves of the listed games (host only)
int rc_rollout_draw(uint32_t *mt_keys, int32_t *mt_pos, uint32_t n_games, const int32_t *games, const int32_t *slots, uint32_t n,
                    int mode, uint32_t steps, void *table, size_t table_stride) {
    RC_REQUIRE(mt_keys && mt_pos && table, RC_ERR_NULL);
    RC_REQUIRE(n == 0 || (games && slots), RC_ERR_NULL);
    RC_REQUIRE(mode == 0 || (reinterpret_cast<uintptr_t>(table) & 7u) == 0, RC_ERR_ALIGN);
    RC_REQUIRE((mode == 0 || mode == 1) && steps > 0, RC_ERR_RANGE);
    for (u32 i = 0; i < n; ++i) {
        RC_REQUIRE(games[i] >= 0 && (u32)games[i] < n_games && slots[i] >= 0 && (size_t)slots[i] < table_stride, RC_ERR_RANGE);
        RC_REQUIRE(mt_pos[games[i]] >= 0 && mt_pos[games[i]] <= 624, RC_ERR_RANGE);
    }
    for (u32 i = 0; i < n; ++i) {
        Mt19937 mt{mt_keys + (size_t)games[i] * 624, mt_pos[games[i]]};
        for (u32 t = 0; t < steps; ++t) {
            const size_t at = (size_t)t * table_stride + (size_t)slots[i];
            if (mode == 0) {
                u32 v;
                do v = mt.next() & 15u; while (v > 11u);
                static_cast<u8 *>(table)[at] = (u8)v;
            } else {
                const u32 a = mt.next() >> 5, b = mt.next() >> 6;
                static_cast<double *>(table)[at] = (a * 67108864.0 + b) / 9007199254740992.0;
            }
        }
        mt_pos[games[i]] = mt.pos;
    }
    return RC_OK;
}

}  // extern "C"
