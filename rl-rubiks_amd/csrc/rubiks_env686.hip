// The 6x8x6 representation on MI355X (gfx950): the environment kernels over 48 sticker planes, the one-hot / correctness
// encoders, and the bridge from the 20 code planes of DeviceCubes (reference librubiks/cube/cube.py:311-388).
//
// Device form: 48 int8 planes of sticker colour 0..5, plane f*8+p = sticker p of face f, structure-of-arrays with the stride
// rule of the 20 code planes.  Every action is one fixed permutation of the 48 planes' bytes (kTables686.perm, 576 B), so
// every kernel has the same shape: a workgroup stages a tile of states as bytes in LDS (16-byte or dword global loads), picks the
// bytes of its outputs out of the tile through the LDS-resident table, and writes whole 16-byte chunks of the output, coalesced.
// Byte work, HBM-bound by design, no MFMA.  All global stores are ordinary vector stores.
#include "rubiks_common.h"
#include "rubiks_tables686.h"

namespace rubiks {

static __constant__ Tables686 c_tables686 = kTables686;

constexpr int kPermBytes = kActionPad * kStickers;                 // 768
constexpr int kBridgeBytes = kPlanes * kCodePad * 3 * 2;           // 3840

// Leading dimension of a staged tile of SB states: sticker s of state r is byte stk[s * ld686(SB) + r].  The 4 bytes of padding per
// sticker row put consecutive stickers of one state 17 (65) dwords apart, i.e. in different LDS banks: the emitters' lanes walk the
// stickers of one state (a row of the output), and with rows exactly SB bytes apart they would all hit the same two banks.
__host__ __device__ constexpr int ld686(int sb) { return sb + 4; }

__device__ __forceinline__ u32 pack4(u32 b0, u32 b1, u32 b2, u32 b3) { return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24); }

// -------------------------------------------------------------------------------------------------
// Staging a tile of SB states as sticker bytes stk[s * ld686(SB) + r]  (s = sticker 0..47, r = state in tile)
// -------------------------------------------------------------------------------------------------
// ... from sticker planes: dword loads, plane by plane
template <int SB>
__device__ __forceinline__ void stage_from_planes(u32 *s_stk, const u32 *__restrict__ soa, size_t row0, size_t n_dw, size_t stride_dw) {
    for (int i = threadIdx.x; i < kStickers * SB / 4; i += kBlock) {
        const int s = i / (SB / 4), w = i % (SB / 4);
        const size_t dw = row0 / 4 + w;
        s_stk[s * (ld686(SB) / 4) + w] = (dw < n_dw) ? soa[(size_t)s * stride_dw + dw] : 0u;
    }
}

// ... from the 20 code planes through the bridge table: cubie i with code v writes its 3 / 2 sticker bytes.  A valid state writes
// each of the 48 bytes of its column exactly once; columns of padding states hold whatever was there and are never emitted.
template <int SB>
__device__ __forceinline__ void stage_from_codes(u8 *stk, const u8 *bridge, const u32 *__restrict__ soa, size_t row0, size_t n_dw,
                                                 size_t stride_dw) {
    for (int i = threadIdx.x; i < kPlanes * SB / 4; i += kBlock) {
        const int j = i / (SB / 4), w = i % (SB / 4);
        const size_t dw = row0 / 4 + w;
        if (dw >= n_dw) continue;
        const u32 v = soa[(size_t)j * stride_dw + dw];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const u8 *e = bridge + ((j * kCodePad + code_of(v, b)) * 3) * 2;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k == 2 && j >= kCorners) break;
                const u32 s = e[2 * k];
                if (s < (u32)kStickers) stk[s * ld686(SB) + 4 * w + b] = e[2 * k + 1];
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------
// Emitting rows from a staged tile, 16 bytes per lane, whole rows coalesced
// -------------------------------------------------------------------------------------------------
// one-hot (n, 288): element e of a row is 1 iff sticker e / 6 has colour e % 6      (cube.py:363-369)
template <int SB, bool BF16>
__device__ __forceinline__ void emit_oh(const u8 *stk, uint4 *__restrict__ dst, u32 rows) {
    constexpr int EPC = BF16 ? 8 : 4;            // elements per 16-byte chunk
    constexpr int CPR = kOh686 / EPC;            // chunks per row: 72 (f32) / 36 (bf16)
    const u32 total = rows * CPR;
    for (u32 x = threadIdx.x; x < total; x += kBlock) {
        const u32 r = x / CPR, c = x - r * CPR;
        const u32 e0 = c * EPC, s0 = e0 / kColours;
        // a chunk starts at an even offset into a sticker's six entries, so its 4 / 8 elements span exactly two stickers:
        // the position of each one's 1 relative to the chunk
        int rel[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const u32 s = s0 + q;
            rel[q] = (s < (u32)kStickers) ? (int)(s * kColours + stk[s * ld686(SB) + r]) - (int)e0 : -1;
        }
        u32 bit = 0;   // bit i set: element e0 + i is the 1 of its sticker
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (rel[q] >= 0 && rel[q] < EPC) bit |= 1u << rel[q];
        uint4 v;
        if (BF16) {
            const u32 lo = 0x3f80u, hi = 0x3f800000u;
            v.x = ((bit & 1u) ? lo : 0u) | ((bit & 2u) ? hi : 0u);
            v.y = ((bit & 4u) ? lo : 0u) | ((bit & 8u) ? hi : 0u);
            v.z = ((bit & 16u) ? lo : 0u) | ((bit & 32u) ? hi : 0u);
            v.w = ((bit & 64u) ? lo : 0u) | ((bit & 128u) ? hi : 0u);
        } else {
            const u32 one = 0x3f800000u;
            v = make_uint4((bit & 1u) ? one : 0u, (bit & 2u) ? one : 0u, (bit & 4u) ? one : 0u, (bit & 8u) ? one : 0u);
        }
        dst[x] = v;
    }
}

// correctness (n, 6, 8) f32: +1 where sticker s has its face's colour s / 8, -1 elsewhere      (cube.py:372-380)
template <int SB>
__device__ __forceinline__ void emit_correct(const u8 *stk, uint4 *__restrict__ dst, u32 rows) {
    constexpr int CPR = kStickers / 4;   // 12 chunks per row
    const u32 total = rows * CPR;
    for (u32 x = threadIdx.x; x < total; x += kBlock) {
        const u32 r = x / CPR, c = x - r * CPR;
        const u32 face = (4 * c) / 8;   // the four stickers of a chunk share a face
        const u32 plus = 0x3f800000u, minus = 0xbf800000u;
        uint4 v;
        v.x = stk[(4 * c + 0) * ld686(SB) + r] == face ? plus : minus;
        v.y = stk[(4 * c + 1) * ld686(SB) + r] == face ? plus : minus;
        v.z = stk[(4 * c + 2) * ld686(SB) + r] == face ? plus : minus;
        v.w = stk[(4 * c + 3) * ld686(SB) + r] == face ? plus : minus;
        dst[x] = v;
    }
}

// the tile back out as sticker planes (dwords; rows beyond n inside the last 16 are padding)
template <int SB>
__device__ __forceinline__ void emit_planes(const u32 *s_stk, u32 *__restrict__ soa, size_t row0, size_t n_dw, size_t stride_dw) {
    for (int i = threadIdx.x; i < kStickers * SB / 4; i += kBlock) {
        const int s = i / (SB / 4), w = i % (SB / 4);
        const size_t dw = row0 / 4 + w;
        if (dw < n_dw) soa[(size_t)s * stride_dw + dw] = s_stk[s * (ld686(SB) / 4) + w];
    }
}

enum Src { kFromPlanes = 0, kFromCodes = 1 };
enum Dst { kToOhF32 = 0, kToOhBf16 = 1, kToCorrect = 2, kToPlanes = 3 };

// One kernel shape for every encoder: SRC planes or codes -> LDS tile -> DST rows.  as_oh is write-bound (1152 B f32 / 576 B bf16
// per state against 48 or 20 B read), so the fused form from the code planes costs the same as the one from sticker planes.
template <int SB, int SRC, int DST>
__global__ __launch_bounds__(kBlock) void k_encode686(const u32 *__restrict__ soa, void *__restrict__ out, size_t n, size_t n_dw,
                                                      size_t stride_dw, size_t stride_out_dw) {
    __shared__ u32 s_stk[kStickers * ld686(SB) / 4];
    __shared__ u32 s_bridge[SRC == kFromCodes ? kBridgeBytes / 4 : 1];
    const size_t row0 = (size_t)blockIdx.x * SB;
    if (SRC == kFromCodes) {
        stage_to_lds(s_bridge, c_tables686.bridge, kBridgeBytes);
        if (DST == kToPlanes)   // padding columns are written out: give them defined bytes
            for (int i = threadIdx.x; i < kStickers * ld686(SB) / 4; i += kBlock) s_stk[i] = 0u;
        __syncthreads();
        stage_from_codes<SB>(reinterpret_cast<u8 *>(s_stk), reinterpret_cast<const u8 *>(s_bridge), soa, row0, n_dw, stride_dw);
    } else {
        stage_from_planes<SB>(s_stk, soa, row0, n_dw, stride_dw);
    }
    __syncthreads();
    const u32 rows = (u32)((n - row0 < (size_t)SB) ? n - row0 : SB);
    const u8 *stk = reinterpret_cast<const u8 *>(s_stk);
    if (DST == kToOhF32) emit_oh<SB, false>(stk, reinterpret_cast<uint4 *>(out) + row0 * (kOh686 / 4), rows);
    else if (DST == kToOhBf16) emit_oh<SB, true>(stk, reinterpret_cast<uint4 *>(out) + row0 * (kOh686 / 8), rows);
    else if (DST == kToCorrect) emit_correct<SB>(stk, reinterpret_cast<uint4 *>(out) + row0 * (kStickers / 4), rows);
    else emit_planes<SB>(s_stk, reinterpret_cast<u32 *>(out), row0, n_dw, stride_out_dw);
}

// =================================================================================================
// multi_rotate: out[s][i] = in[perm[act[i]][s]][i]                      (reference cube.py:349-361)
// The reference walks the states in a Python loop; here a workgroup stages 256 states (48 x 16-byte loads per 16 states) and every
// lane assembles 16-byte chunks of the output planes from LDS bytes.  in and out may alias exactly: a tile is read completely
// before any of its columns is written, and no other workgroup touches those columns.
// =================================================================================================
constexpr int kRotTile = 256;

typedef unsigned v4u686 __attribute__((ext_vector_type(4)));

// NT: non-temporal loads and stores for large batches (every byte is touched once; as rc_multi_rotate does from 2^20 states on).
template <bool NT>
__global__ __launch_bounds__(kBlock) void k686_multi_rotate(const uint4 *in, const uint4 *__restrict__ act, uint4 *out, size_t n_vec,
                                                            size_t sin_vec, size_t sout_vec) {
    constexpr int VPT = kRotTile / 16;   // 16-byte vectors per plane per tile
    constexpr int LDV = VPT + 1;         // ... and per sticker row of the LDS tile: one vector of padding moves the rows across the banks
    __shared__ uint4 s_tile[kStickers * LDV];
    __shared__ uint4 s_act[VPT];
    __shared__ u32 s_perm[kPermBytes / 4];
    stage_to_lds(s_perm, c_tables686.perm, kPermBytes);
    const u8 *perm = reinterpret_cast<const u8 *>(s_perm);
    const u8 *tile = reinterpret_cast<const u8 *>(s_tile);
    const u8 *acts = reinterpret_cast<const u8 *>(s_act);
    const size_t n_tiles = ceil_div(n_vec, (size_t)VPT);
    for (size_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const size_t v0 = t * VPT;
        __syncthreads();   // the previous tile's readers are done (and perm is staged)
        for (int i = threadIdx.x; i < kStickers * VPT; i += kBlock) {
            const int s = i / VPT, w = i % VPT;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (v0 + w < n_vec) {
                if (NT) {
                    const v4u686 x = __builtin_nontemporal_load(reinterpret_cast<const v4u686 *>(&in[(size_t)s * sin_vec + v0 + w]));
                    v = make_uint4(x[0], x[1], x[2], x[3]);
                } else v = in[(size_t)s * sin_vec + v0 + w];
            }
            s_tile[s * LDV + w] = v;
        }
        if (threadIdx.x < VPT) s_act[threadIdx.x] = (v0 + threadIdx.x < n_vec) ? act[v0 + threadIdx.x] : make_uint4(0, 0, 0, 0);
        __syncthreads();
        for (int i = threadIdx.x; i < kStickers * VPT; i += kBlock) {
            const int s = i / VPT, w = i % VPT;
            if (v0 + w >= n_vec) continue;
            // The 16 lanes that share a sticker read rows 4 dwords apart; were they all on dword d of their chunk at the same time they
            // would share 16 of the 64 banks with the other three stickers of the wave.  Lane w takes its dwords in the order j ^ (w & 3).
            const int rot = w & 3;
            u32 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = j ^ rot;
                u32 b[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int r = 16 * w + 4 * d + k;
                    b[k] = tile[(u32)perm[(acts[r] & (kActionPad - 1)) * kStickers + s] * (16 * LDV) + r];
                }
                v[j] = pack4(b[0], b[1], b[2], b[3]);
            }
            u32 o[4];   // o[d] = v[d ^ rot]
#pragma unroll
            for (int d = 0; d < 4; ++d) o[d] = rot == 0 ? v[d] : rot == 1 ? v[d ^ 1] : rot == 2 ? v[d ^ 2] : v[d ^ 3];
            if (NT) {
                const v4u686 x = {o[0], o[1], o[2], o[3]};
                __builtin_nontemporal_store(x, reinterpret_cast<v4u686 *>(&out[(size_t)s * sout_vec + v0 + w]));
            } else out[(size_t)s * sout_vec + v0 + w] = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
}

// =================================================================================================
// expand12: children[12 p + k] = action k on parent p, with the solved flags of rc_expand12_flags
// A tile is 64 parents = 768 children = 48 16-byte chunks per plane; child byte c of the tile reads parent c / 12 through
// perm[c % 12].  A child is the solved cube iff its parent is the solved cube turned by k ^ 1: such a parent has exactly 36 of its
// 48 stickers in place (the 12 around the turned face are not), so the 12 full compares run for those parents only.
// =================================================================================================
constexpr int kExpTile = 64;

template <bool FLAGS>
__global__ __launch_bounds__(kBlock) void k686_expand12(const u32 *__restrict__ par, uint4 *__restrict__ child, size_t n_parents,
                                                        size_t n_par_dw, size_t n_chunks, size_t sp_dw, size_t sc_vec,
                                                        u8 *__restrict__ parent_flags, u32 *__restrict__ child_flags) {
    constexpr int CPP = kExpTile * kActions / 16;   // child chunks per plane per tile: 48
    constexpr int LD = ld686(kExpTile);
    __shared__ u32 s_stk[kStickers * LD / 4];
    __shared__ u32 s_perm[kPermBytes / 4];
    stage_to_lds(s_perm, c_tables686.perm, kPermBytes);
    const u8 *perm = reinterpret_cast<const u8 *>(s_perm);
    const u8 *stk = reinterpret_cast<const u8 *>(s_stk);
    const size_t n_tiles = ceil_div(n_parents, (size_t)kExpTile);
    for (size_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const size_t row0 = t * kExpTile;
        __syncthreads();
        stage_from_planes<kExpTile>(s_stk, par, row0, n_par_dw, sp_dw);
        __syncthreads();
        if (FLAGS && threadIdx.x < kExpTile && row0 + threadIdx.x < round_up(n_parents, 16)) {
            const u32 r = threadIdx.x;
            u32 cnt = 0;
#pragma unroll
            for (int s = 0; s < kStickers; ++s) cnt += stk[s * LD + r] == (u32)(s / 8);
            parent_flags[row0 + r] = cnt == (u32)kStickers;
            u32 cf[3] = {0, 0, 0};
            if (cnt == (u32)kStickers - 12)
                for (int k = 0; k < kActions; ++k) {
                    bool same = true;
                    for (int s = 0; s < kStickers; ++s) same &= stk[(u32)perm[k * kStickers + s] * LD + r] == (u32)(s / 8);
                    if (same) cf[k >> 2] |= 1u << (8 * (k & 3));
                }
#pragma unroll
            for (int i = 0; i < 3; ++i) child_flags[3 * (row0 + r) + i] = cf[i];
        }
        const size_t q0 = t * CPP;
        for (int i = threadIdx.x; i < kStickers * CPP; i += kBlock) {
            const int s = i / CPP, q = i % CPP;
            if (q0 + q >= n_chunks) continue;
            u32 o[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                // dword d of the chunk: children 16 q + 4 d .. + 3 = four consecutive actions of ONE parent (12 % 4 == 0)
                const u32 c = 16 * q + 4 * d, p = c / kActions, k0 = c - p * kActions;
                u32 b[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) b[k] = stk[(u32)perm[(k0 + k) * kStickers + s] * LD + p];
                o[d] = pack4(b[0], b[1], b[2], b[3]);
            }
            child[(size_t)s * sc_vec + q0 + q] = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
}

// =================================================================================================
// is_solved: plane s equals s / 8 everywhere                                   (reference cube.py:85-89)
// =================================================================================================
__device__ __forceinline__ u32 zero_bytes_to_flags686(u32 x) {
    const u32 nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
    return (nz >> 7) ^ 0x01010101u;
}

__global__ __launch_bounds__(kBlock) void k686_is_solved(const uint4 *__restrict__ soa, uint4 *__restrict__ flags, size_t n, size_t n_vec,
                                                         size_t stride_vec) {
    for (size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x; g < n_vec; g += (size_t)gridDim.x * kBlock) {
        uint4 acc = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < kStickers; ++s) {
            const u32 want = 0x01010101u * (u32)(s / 8);
            const uint4 v = soa[(size_t)s * stride_vec + g];
            acc.x |= v.x ^ want; acc.y |= v.y ^ want; acc.z |= v.z ^ want; acc.w |= v.w ^ want;
        }
        u32 f[4] = {zero_bytes_to_flags686(acc.x), zero_bytes_to_flags686(acc.y), zero_bytes_to_flags686(acc.z), zero_bytes_to_flags686(acc.w)};
        const size_t first = g * 16;
        if (first + 16 > n) {   // ragged tail: padding cubes are never solved
            const u32 valid = (u32)(n - first);
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if ((u32)c >= valid) f[c >> 2] &= ~(0xffu << (8 * (c & 3)));
        }
        flags[g] = make_uint4(f[0], f[1], f[2], f[3]);
    }
}

// =================================================================================================
// apply_moves: in place, cube i <- action moves[d][i] for d = 0 .. depth - 1 (the scramble loop, cube.py:206-211)
// A workgroup keeps 64 cubes in LDS and ping-pongs between two tiles, one permutation per step.
// =================================================================================================
constexpr int kMovTile = 64;

__global__ __launch_bounds__(kBlock) void k686_apply_moves(u32 *__restrict__ soa, const u8 *__restrict__ moves, size_t n, size_t n_dw,
                                                           size_t stride_dw, size_t moves_stride, size_t depth) {
    constexpr int LD = ld686(kMovTile);
    __shared__ u32 s_a[kStickers * LD / 4], s_b[kStickers * LD / 4];
    __shared__ u32 s_perm[kPermBytes / 4];
    stage_to_lds(s_perm, c_tables686.perm, kPermBytes);
    const u8 *perm = reinterpret_cast<const u8 *>(s_perm);
    const size_t n_tiles = ceil_div(n, (size_t)kMovTile);
    for (size_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const size_t row0 = t * kMovTile;
        __syncthreads();
        stage_from_planes<kMovTile>(s_a, soa, row0, n_dw, stride_dw);
        __syncthreads();
        u8 *cur = reinterpret_cast<u8 *>(s_a), *nxt = reinterpret_cast<u8 *>(s_b);
        for (size_t d = 0; d < depth; ++d) {
            for (int i = threadIdx.x; i < kStickers * kMovTile; i += kBlock) {
                const int s = i / kMovTile, r = i % kMovTile;
                const u32 a = (row0 + r < n) ? (moves[d * moves_stride + row0 + r] & (kActionPad - 1)) : (u32)kActions;   // identity padding
                nxt[s * LD + r] = cur[(u32)perm[a * kStickers + s] * LD + r];
            }
            __syncthreads();
            u8 *tmp = cur; cur = nxt; nxt = tmp;
        }
        emit_planes<kMovTile>(reinterpret_cast<const u32 *>(cur), soa, row0, n_dw, stride_dw);
    }
}

// =================================================================================================
// Boundary: the reference's (n, 6, 8, 6) int8 one-hot arrays <-> sticker planes, 64 states per workgroup through LDS
// =================================================================================================
constexpr int kTB686 = 64;

__global__ __launch_bounds__(kBlock) void k686_aos_to_soa(const u32 *__restrict__ aos, u32 *__restrict__ soa, size_t n, size_t n_dw,
                                                          size_t stride_dw) {
    __shared__ u32 s_in[kTB686 * kOh686 / 4];
    __shared__ u32 s_stk[kStickers * ld686(kTB686) / 4];
    const size_t row0 = (size_t)blockIdx.x * kTB686;
    const u32 rows = (u32)((n - row0 < (size_t)kTB686) ? n - row0 : kTB686);
    const u32 *src = aos + row0 * (kOh686 / 4);   // a row is 72 dwords: no partial dword at the end of the array
    for (u32 i = threadIdx.x; i < kTB686 * kOh686 / 4; i += kBlock) s_in[i] = (i < rows * (kOh686 / 4)) ? src[i] : 0u;
    __syncthreads();
    const u8 *oh = reinterpret_cast<const u8 *>(s_in);
    u8 *stk = reinterpret_cast<u8 *>(s_stk);
    for (u32 i = threadIdx.x; i < kStickers * kTB686; i += kBlock) {
        const u32 s = i / kTB686, r = i % kTB686;
        u32 colour = 0;
#pragma unroll
        for (u32 c = 1; c < (u32)kColours; ++c) colour = oh[r * kOh686 + s * kColours + c] ? c : colour;
        stk[s * ld686(kTB686) + r] = (u8)colour;
    }
    __syncthreads();
    emit_planes<kTB686>(s_stk, soa, row0, n_dw, stride_dw);
}

__global__ __launch_bounds__(kBlock) void k686_soa_to_aos(const u32 *__restrict__ soa, u32 *__restrict__ aos, size_t n, size_t n_dw,
                                                          size_t stride_dw) {
    __shared__ u32 s_stk[kStickers * ld686(kTB686) / 4];
    const size_t row0 = (size_t)blockIdx.x * kTB686;
    const u32 rows = (u32)((n - row0 < (size_t)kTB686) ? n - row0 : kTB686);
    stage_from_planes<kTB686>(s_stk, soa, row0, n_dw, stride_dw);
    __syncthreads();
    const u8 *stk = reinterpret_cast<const u8 *>(s_stk);
    u32 *dst = aos + row0 * (kOh686 / 4);
    for (u32 i = threadIdx.x; i < rows * (kOh686 / 4); i += kBlock) {
        const u32 r = i / (kOh686 / 4), e0 = 4 * (i - r * (kOh686 / 4));
        u32 v = 0;
#pragma unroll
        for (u32 b = 0; b < 4; ++b) {
            const u32 e = e0 + b, s = e / kColours;
            v |= (u32)(stk[s * ld686(kTB686) + r] == e - s * kColours) << (8 * b);
        }
        dst[i] = v;
    }
}

// ---- small calls on the reference's own (n, 6, 8, 6) one-hot int8 layout (pinned host memory or device memory, one launch) ----
__global__ __launch_bounds__(kBlock) void k686_multi_rotate_aos(const u8 *__restrict__ in, const u8 *__restrict__ actions, u8 *__restrict__ out,
                                                                size_t n) {
    __shared__ u32 s_perm[kPermBytes / 4];
    stage_to_lds(s_perm, c_tables686.perm, kPermBytes);
    __syncthreads();
    const u8 *perm = reinterpret_cast<const u8 *>(s_perm);
    for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < n * kOh686; idx += (size_t)gridDim.x * kBlock) {
        const size_t i = idx / kOh686;
        const u32 e = (u32)(idx - i * kOh686), s = e / kColours, c = e - s * kColours;
        const u32 a = actions[i] & (kActionPad - 1);
        out[idx] = in[i * kOh686 + (u32)perm[a * kStickers + s] * kColours + c];
    }
}

__global__ __launch_bounds__(kBlock) void k686_is_solved_aos(const u8 *__restrict__ in, u8 *__restrict__ flags, size_t n) {
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        bool ok = true;
        for (u32 e = 0; e < (u32)kOh686; ++e) ok &= in[i * kOh686 + e] == (u8)(e % kColours == e / (8 * kColours));
        flags[i] = ok ? 1 : 0;
    }
}

__global__ __launch_bounds__(kBlock) void k686_as_oh_aos(const int8_t *__restrict__ in, float *__restrict__ out, size_t n) {
    for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < n * kOh686; idx += (size_t)gridDim.x * kBlock)
        out[idx] = (float)in[idx];   // the representation is one-hot already (cube.py:363-369)
}

// =================================================================================================
// (n, 288) one-hot network input -> (n, 6, 8) correctness, in the input's dtype: what ConvNet.forward feeds its convolutions
// (reference model.py:326 through cube.py:135-137,372-380: all six entries of a sticker equal the solved cube's).
// =================================================================================================
template <typename T> struct Ones;
template <> struct Ones<float> { static constexpr u32 one = 0x3f800000u, plus = 0x3f800000u, minus = 0xbf800000u; };
template <> struct Ones<u16> { static constexpr u32 one = 0x3f80u, plus = 0x3f80u, minus = 0xbf80u; };

template <typename T, typename B>
__global__ __launch_bounds__(kBlock) void k686_as_correct_oh(const B *__restrict__ in, B *__restrict__ out, size_t n) {
    for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < n * kStickers; idx += (size_t)gridDim.x * kBlock) {
        const u32 s = (u32)(idx % kStickers), face = s / 8;
        const B *p = in + idx * kColours;
        bool ok = true;
#pragma unroll
        for (u32 c = 0; c < (u32)kColours; ++c) ok &= p[c] == (B)(c == face ? Ones<T>::one : 0u);
        out[idx] = (B)(ok ? Ones<T>::plus : Ones<T>::minus);
    }
}

}  // namespace rubiks

// =================================================================================================
// C ABI
// =================================================================================================
using namespace rubiks;

template <int SRC, int DST>
static int encode_impl(const int8_t *soa, void *out, size_t n, size_t stride, size_t stride_out, rc_stream_t stream) {
    if (n == 0) return RC_OK;
    RC_CHECK_SOA(soa, n, stride);
    RC_REQUIRE(out != nullptr, RC_ERR_NULL);
    RC_REQUIRE(aligned16(out), RC_ERR_ALIGN);
    if (DST == kToPlanes) RC_CHECK_SOA(out, n, stride_out);
    hipStream_t s = (hipStream_t)stream;
    const size_t n_dw = round_up(n, 16) / 4;
    if (n >= ((size_t)1 << 16)) {   // the tables' staging is amortised over 256 states once there are enough tiles to fill the chip
        constexpr int SB = 256;
        hipLaunchKernelGGL((k_encode686<SB, SRC, DST>), dim3((unsigned)ceil_div(n, SB)), dim3(kBlock), 0, s, (const u32 *)soa, out, n, n_dw,
                           stride / 4, stride_out / 4);
    } else {
        constexpr int SB = 64;
        hipLaunchKernelGGL((k_encode686<SB, SRC, DST>), dim3((unsigned)ceil_div(n, SB)), dim3(kBlock), 0, s, (const u32 *)soa, out, n, n_dw,
                           stride / 4, stride_out / 4);
    }
    return launch_status();
}

template <bool FLAGS>
static int expand686_impl(const int8_t *par, int8_t *child, size_t n, size_t sp, size_t sc, uint8_t *pf, uint8_t *cf, rc_stream_t stream) {
    if (n == 0) return RC_OK;
    RC_CHECK_SOA(par, n, sp);
    RC_CHECK_SOA(child, n * kActions, sc);
    if (FLAGS) {
        RC_REQUIRE(pf != nullptr && cf != nullptr, RC_ERR_NULL);
        RC_REQUIRE(aligned16(pf) && aligned16(cf), RC_ERR_ALIGN);
    }
    const size_t tiles = ceil_div(n, (size_t)kExpTile);
    hipLaunchKernelGGL(k686_expand12<FLAGS>, dim3((unsigned)(tiles < 16384 ? tiles : 16384)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const u32 *)par, (uint4 *)child, n, round_up(n, 16) / 4, ceil_div(n * kActions, 16), sp / 4, sc / 16, pf, (u32 *)cf);
    return launch_status();
}

extern "C" {

int rc686_get_perm_table(uint8_t *out576) {
    RC_REQUIRE(out576 != nullptr, RC_ERR_NULL);
    for (int a = 0; a < kActions; ++a)
        for (int s = 0; s < kStickers; ++s) out576[a * kStickers + s] = kTables686.perm[a][s];
    return RC_OK;
}

int rc686_get_bridge_table(uint8_t *out2880) {
    RC_REQUIRE(out2880 != nullptr, RC_ERR_NULL);
    for (int i = 0; i < kPlanes; ++i)
        for (int v = 0; v < kCodes; ++v)
            for (int k = 0; k < 3; ++k)
                for (int x = 0; x < 2; ++x) out2880[((i * kCodes + v) * 3 + k) * 2 + x] = kTables686.bridge[i][v][k][x];
    return RC_OK;
}

int rc686_aos_to_soa(const int8_t *oh_aos, int8_t *soa, size_t n, size_t stride, rc_stream_t stream) {
    if (n == 0) return RC_OK;
    RC_CHECK_SOA(soa, n, stride);
    RC_REQUIRE(oh_aos != nullptr, RC_ERR_NULL);
    RC_REQUIRE(aligned16(oh_aos), RC_ERR_ALIGN);
    hipLaunchKernelGGL(k686_aos_to_soa, dim3((unsigned)ceil_div(n, kTB686)), dim3(kBlock), 0, (hipStream_t)stream, (const u32 *)oh_aos,
                       (u32 *)soa, n, round_up(n, 16) / 4, stride / 4);
    return launch_status();
}

int rc686_soa_to_aos(const int8_t *soa, int8_t *oh_aos, size_t n, size_t stride, rc_stream_t stream) {
    if (n == 0) return RC_OK;
    RC_CHECK_SOA(soa, n, stride);
    RC_REQUIRE(oh_aos != nullptr, RC_ERR_NULL);
    RC_REQUIRE(aligned16(oh_aos), RC_ERR_ALIGN);
    hipLaunchKernelGGL(k686_soa_to_aos, dim3((unsigned)ceil_div(n, kTB686)), dim3(kBlock), 0, (hipStream_t)stream, (const u32 *)soa,
                       (u32 *)oh_aos, n, round_up(n, 16) / 4, stride / 4);
    return launch_status();
}

int rc686_multi_rotate(const int8_t *in_soa, const uint8_t *actions, int8_t *out_soa, size_t n, size_t stride_in, size_t stride_out,
                       rc_stream_t stream) {
    if (n == 0) return RC_OK;
    RC_CHECK_SOA(in_soa, n, stride_in);
    RC_CHECK_SOA(out_soa, n, stride_out);
    RC_REQUIRE(actions != nullptr, RC_ERR_NULL);
    RC_REQUIRE(aligned16(actions), RC_ERR_ALIGN);
    const size_t n_vec = ceil_div(n, 16), tiles = ceil_div(n_vec, (size_t)(kRotTile / 16));
    if (n >= ((size_t)1 << 20))
        hipLaunchKernelGGL(k686_multi_rotate<true>, dim3((unsigned)(tiles < 65536 ? tiles : 65536)), dim3(kBlock), 0, (hipStream_t)stream,
                           (const uint4 *)in_soa, (const uint4 *)actions, (uint4 *)out_soa, n_vec, stride_in / 16, stride_out / 16);
    else
        hipLaunchKernelGGL(k686_multi_rotate<false>, dim3((unsigned)(tiles < 16384 ? tiles : 16384)), dim3(kBlock), 0, (hipStream_t)stream,
                           (const uint4 *)in_soa, (const uint4 *)actions, (uint4 *)out_soa, n_vec, stride_in / 16, stride_out / 16);
    return launch_status();
}

int rc686_expand12(const int8_t *parents_soa, int8_t *children_soa, size_t n_parents, size_t stride_p, size_t stride_c, rc_stream_t stream) {
    return expand686_impl<false>(parents_soa, children_soa, n_parents, stride_p, stride_c, nullptr, nullptr, stream);
}

int rc686_expand12_flags(const int8_t *parents_soa, int8_t *children_soa, size_t n_parents, size_t stride_p, size_t stride_c,
                         uint8_t *parent_solved, uint8_t *child_solved, rc_stream_t stream) {
    return expand686_impl<true>(parents_soa, children_soa, n_parents, stride_p, stride_c, parent_solved, child_solved, stream);
}

int rc686_is_solved(const int8_t *soa, uint8_t *flags, size_t n, size_t stride, rc_stream_t stream) {
    if (n == 0) return RC_OK;
    RC_CHECK_SOA(soa, n, stride);
    RC_REQUIRE(flags != nullptr, RC_ERR_NULL);
    RC_REQUIRE(aligned16(flags), RC_ERR_ALIGN);
    const size_t n_vec = ceil_div(n, 16);
    hipLaunchKernelGGL(k686_is_solved, dim3(grid_for(n_vec)), dim3(kBlock), 0, (hipStream_t)stream, (const uint4 *)soa, (uint4 *)flags, n,
                       n_vec, stride / 16);
    return launch_status();
}

int rc686_as_oh_f32(const int8_t *soa, float *out, size_t n, size_t stride, rc_stream_t stream) {
    return encode_impl<kFromPlanes, kToOhF32>(soa, out, n, stride, 0, stream);
}
int rc686_as_oh_bf16(const int8_t *soa, uint16_t *out, size_t n, size_t stride, rc_stream_t stream) {
    return encode_impl<kFromPlanes, kToOhBf16>(soa, out, n, stride, 0, stream);
}
int rc686_as_correct_f32(const int8_t *soa, float *out, size_t n, size_t stride, rc_stream_t stream) {
    return encode_impl<kFromPlanes, kToCorrect>(soa, out, n, stride, 0, stream);
}

int rc686_apply_moves(int8_t *soa, const uint8_t *moves, size_t n, size_t stride, size_t moves_stride, size_t depth, rc_stream_t stream) {
    if (n == 0 || depth == 0) return RC_OK;
    RC_CHECK_SOA(soa, n, stride);
    RC_REQUIRE(moves != nullptr, RC_ERR_NULL);
    RC_REQUIRE(moves_stride >= n, RC_ERR_STRIDE);
    const size_t tiles = ceil_div(n, (size_t)kMovTile);
    hipLaunchKernelGGL(k686_apply_moves, dim3((unsigned)(tiles < 16384 ? tiles : 16384)), dim3(kBlock), 0, (hipStream_t)stream, (u32 *)soa,
                       moves, n, round_up(n, 16) / 4, stride / 4, moves_stride, depth);
    return launch_status();
}

int rc686_multi_rotate_aos(const int8_t *in_aos, const uint8_t *actions, int8_t *out_aos, size_t n, rc_stream_t stream) {
    if (n == 0) return RC_OK;
    RC_REQUIRE(in_aos && actions && out_aos, RC_ERR_NULL);
    RC_REQUIRE(in_aos != out_aos, RC_ERR_RANGE);
    hipLaunchKernelGGL(k686_multi_rotate_aos, dim3(grid_for(n * kOh686)), dim3(kBlock), 0, (hipStream_t)stream, (const u8 *)in_aos, actions,
                       (u8 *)out_aos, n);
    return launch_status();
}

int rc686_is_solved_aos(const int8_t *in_aos, uint8_t *flags, size_t n, rc_stream_t stream) {
    if (n == 0) return RC_OK;
    RC_REQUIRE(in_aos && flags, RC_ERR_NULL);
    hipLaunchKernelGGL(k686_is_solved_aos, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, (const u8 *)in_aos, flags, n);
    return launch_status();
}

int rc686_as_oh_aos_f32(const int8_t *in_aos, float *out, size_t n, rc_stream_t stream) {
    if (n == 0) return RC_OK;
    RC_REQUIRE(in_aos && out, RC_ERR_NULL);
    hipLaunchKernelGGL(k686_as_oh_aos, dim3(grid_for(n * kOh686)), dim3(kBlock), 0, (hipStream_t)stream, in_aos, out, n);
    return launch_status();
}

int rc_2024_to_686(const int8_t *soa, int8_t *soa686, size_t n, size_t stride, size_t stride686, rc_stream_t stream) {
    return encode_impl<kFromCodes, kToPlanes>(soa, soa686, n, stride, stride686, stream);
}
int rc_as_oh686_from2024_f32(const int8_t *soa, float *out, size_t n, size_t stride, rc_stream_t stream) {
    return encode_impl<kFromCodes, kToOhF32>(soa, out, n, stride, 0, stream);
}
int rc_as_oh686_from2024_bf16(const int8_t *soa, uint16_t *out, size_t n, size_t stride, rc_stream_t stream) {
    return encode_impl<kFromCodes, kToOhBf16>(soa, out, n, stride, 0, stream);
}
int rc_as_correct_from2024_f32(const int8_t *soa, float *out, size_t n, size_t stride, rc_stream_t stream) {
    return encode_impl<kFromCodes, kToCorrect>(soa, out, n, stride, 0, stream);
}

int rc686_as_correct_oh_f32(const float *oh, float *out, size_t n, rc_stream_t stream) {
    if (n == 0) return RC_OK;
    RC_REQUIRE(oh && out, RC_ERR_NULL);
    RC_REQUIRE(((uintptr_t)oh & 3u) == 0 && ((uintptr_t)out & 3u) == 0, RC_ERR_ALIGN);
    hipLaunchKernelGGL((k686_as_correct_oh<float, u32>), dim3(grid_for(n * kStickers)), dim3(kBlock), 0, (hipStream_t)stream, (const u32 *)oh,
                       (u32 *)out, n);
    return launch_status();
}
int rc686_as_correct_oh_bf16(const uint16_t *oh, uint16_t *out, size_t n, rc_stream_t stream) {
    if (n == 0) return RC_OK;
    RC_REQUIRE(oh && out, RC_ERR_NULL);
    RC_REQUIRE(((uintptr_t)oh & 1u) == 0 && ((uintptr_t)out & 1u) == 0, RC_ERR_ALIGN);
    hipLaunchKernelGGL((k686_as_correct_oh<u16, u16>), dim3(grid_for(n * kStickers)), dim3(kBlock), 0, (hipStream_t)stream, oh, out, n);
    return launch_status();
}

}  // extern "C"
