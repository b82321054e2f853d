/*
 * rubiks_hip.h -- C ABI of librubiks_hip.so, the MI355X (gfx950) implementation of the
 * rl-rubiks cube-environment + search hot path.
 *
 * The reference (peleiden/rl-rubiks) is pure Python/NumPy and has no FFI of its own; these entry
 * points are what the Python shim `rl-rubiks_amd/librubiks/` binds with ctypes to implement the
 * reference's module API (INTEGRATION.md shows the binding).  Each entry point cites the reference
 * expression it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - Every pointer named *_soa / out / flags / mask / count / actions / moves is a DEVICE pointer
 *     (hipMalloc'ed; e.g. torch.Tensor.data_ptr()), 16-byte aligned.  No entry point allocates.
 *   - State layout in HBM is structure-of-arrays: plane j (0..19) of cube i lives at
 *     soa[j * stride + i]; `stride` is in bytes, a multiple of 16 and >= round_up(n, 16).
 *     Bytes of a plane beyond n are padding: kernels may overwrite them with unspecified values.
 *   - State bytes are the reference's codes: corner cubie j<8 -> 3*pos+ori, edge cubie j-8 ->
 *     2*pos+ori, all in 0..23 (librubiks/cube/cube.py:58-65).  Bytes outside 0..23 give
 *     unspecified results but never out-of-bounds accesses.
 *   - Actions are the reference's action indices 0..11: a = 2*face + (1 - direction)
 *     (`action_space`, librubiks/cube/cube.py:33-34).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous
 *     on that stream and safe to capture into a hipGraph.
 *   - Return value: 0 on success; RC_ERR_* (< 0) on argument errors; -(hipError_t) - 1000 when a
 *     HIP call fails.  rc_error_string() describes any of them.
 *   - Thread-safe for distinct streams.
 */
#ifndef RUBIKS_HIP_H
#define RUBIKS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RC_ABI_VERSION 10

#define RC_OK 0
#define RC_ERR_NULL (-1)      /* required pointer is NULL */
#define RC_ERR_ALIGN (-2)     /* pointer or stride not 16-byte aligned */
#define RC_ERR_STRIDE (-3)    /* stride < round_up(n, 16) */
#define RC_ERR_RANGE (-4)     /* size / index argument out of range */
#define RC_ERR_NODEVICE (-5)  /* no gfx950 device / wrong architecture */
#define RC_ERR_HIP_BASE (-1000)

typedef void *rc_stream_t;

/* ---- library / host-only helpers ------------------------------------------------------------ */

int rc_abi_version(void);
const char *rc_error_string(int code);

/* Selects `device`, verifies it is gfx950.  Must be called once per process before device calls. */
int rc_init(int device);

/* Host-side copies of the constant tables the kernels use (no GPU needed):
 * out576[a*48 + kind*24 + v] = code v after action a  (v + maps[dir,face,kind,v],
 * librubiks/cube/maps.py:107-145 + librubiks/cube/cube.py:239). */
int rc_get_move_table(uint8_t *out576);
/* out20 = solved state (librubiks/cube/cube.py:58-65,73-74). */
int rc_get_solved(int8_t *out20);

/* ---- layout: the reference's (n,20) row-major arrays <-> SoA -------------------------------- */

int rc_aos_to_soa(const int8_t *aos, int8_t *soa, size_t n, size_t stride, rc_stream_t stream);
int rc_soa_to_aos(const int8_t *soa, int8_t *aos, size_t n, size_t stride, rc_stream_t stream);

/* ---- small calls on the reference's own layout ------------------------------------------------
 * The same three operations on (n,20) row-major int8 states, for the sizes at which the reference's callers use the
 * stateless functions (n = 1 .. a few thousand: librubiks/solving/agents.py:109,513).  One launch each, no SoA
 * staging; every pointer may be device memory OR pinned host memory mapped into the device (hipHostMalloc), so a
 * NumPy caller pays one launch and one stream synchronisation per call.  No alignment requirement.
 *   rc_multi_rotate_aos  out[i] = move actions[i] on in[i]      (librubiks/cube/cube.py:49-52,256-263)
 *   rc_is_solved_aos     flags[i] = in[i] == solved             (librubiks/cube/cube.py:85-89)
 *   rc_as_oh_aos_f32     out[i, 24 j + in[i, j]] = 1, else 0    (librubiks/cube/cube.py:130-133,265-277) */
int rc_multi_rotate_aos(const int8_t *in_aos, const uint8_t *actions, int8_t *out_aos, size_t n, rc_stream_t stream);
int rc_is_solved_aos(const int8_t *in_aos, uint8_t *flags, size_t n, rc_stream_t stream);
int rc_as_oh_aos_f32(const int8_t *in_aos, float *out, size_t n, rc_stream_t stream);

/* ---- cube environment ------------------------------------------------------------------------ */

/* out[i] = move actions[i] applied to in[i].  Replaces _Cube2024.multi_rotate
 * (librubiks/cube/cube.py:256-263, dispatcher :49-52).  in and out may alias exactly.
 * Algorithmic HBM bytes: 41 per state. */
int rc_multi_rotate(const int8_t *in_soa, const uint8_t *actions, int8_t *out_soa, size_t n,
                    size_t stride_in, size_t stride_out, rc_stream_t stream);

/* children[12p + k] = action k applied to parents[p]  (parent-major, action-minor).  Replaces the
 * repeat/tile + multi_rotate idiom (librubiks/solving/agents.py:277-281,513; librubiks/train.py:285).
 * stride_c >= round_up(12 n_parents, 16).  Algorithmic HBM bytes: 260 per parent. */
int rc_expand12(const int8_t *parents_soa, int8_t *children_soa, size_t n_parents, size_t stride_p,
                size_t stride_c, rc_stream_t stream);
/* rc_expand12 that also answers multi_is_solved (cube.py:85-89) for the parents and for every child in the same launch -- the
 * three calls one data-generation step of an ADI rollout makes (train.py:285-296).  The flags come from the staged parents
 * (child k of p is solved iff p is the solved cube turned by rev(k)); no child is read back.
 *   parent_solved: uint8[round_up(n_parents, 16)]   child_solved: uint8[12 round_up(n_parents, 16)]   (1 = solved; 16-byte aligned;
 *   entries behind n_parents / 12 n_parents are padding).  Algorithmic HBM bytes: 273 per parent. */
int rc_expand12_flags(const int8_t *parents_soa, int8_t *children_soa, size_t n_parents, size_t stride_p, size_t stride_c,
                      uint8_t *parent_solved, uint8_t *child_solved, rc_stream_t stream);

/* Solved test.  Replaces multi_is_solved (librubiks/cube/cube.py:85-89).  Any of the three
 * outputs may be NULL:
 *   flags[i]  = 1 if state i is solved else 0                (n bytes, padded to round_up(n,16))
 *   mask      = bit (i % 64) of word (i / 64) set iff solved  (round_up(n,64)/64 words... written
 *               as 16-bit pieces: buffer must hold round_up(n,16)/8 bytes)
 *   *count   += number of solved states                       (caller zeroes it)
 * Algorithmic HBM bytes: 20.125 per state with mask output, 21 with flags. */
int rc_is_solved(const int8_t *soa, uint8_t *flags, uint64_t *mask, uint32_t *count, size_t n,
                 size_t stride, rc_stream_t stream);

/* One-hot network input: out[i][24 j + s[i][j]] = 1, everything else 0; row-major (n, 480).
 * Replaces _Cube2024.as_oh (librubiks/cube/cube.py:265-277).  Every element of all n rows is
 * written (no pre-zeroing needed).  Algorithmic HBM bytes: 1940 (f32) / 980 (bf16) per state. */
int rc_as_oh_f32(const int8_t *soa, float *out, size_t n, size_t stride, rc_stream_t stream);
int rc_as_oh_bf16(const int8_t *soa, uint16_t *out, size_t n, size_t stride, rc_stream_t stream);

/* In place: for d in 0..depth-1: cube i <- action moves[d * n + i] applied to cube i.
 * Replaces the sequential rotate loop of scramble (librubiks/cube/cube.py:206-211) for n cubes at
 * once; the random draws stay on the host so the reference's RNG stream is preserved. */
int rc_apply_moves(int8_t *soa, const uint8_t *moves, size_t n, size_t stride, size_t depth,
                   rc_stream_t stream);

/* sequence_scrambler's state trajectory (librubiks/cube/cube.py:218-234): starting from `games`
 * solved cubes, out row g*depth + d holds game g after (d + 1 - with_solved) moves
 * (row g*depth is the solved cube when with_solved != 0); moves[d * games + g] as above.
 * out_soa has games*depth columns. */
int rc_sequence_states(const uint8_t *moves, int8_t *out_soa, size_t games, size_t depth,
                       int with_solved, size_t stride_out, rc_stream_t stream);

/* ---- network input layer fused with the one-hot encoding ------------------------------------------
 * out[i][c] = act( bias[c] + sum_j W1[c][24 j + s[i][j]] )   (bf16 out, fp32 accumulation)
 * = activation(Linear(480, H)(as_oh(states))) of the reference (librubiks/cube/cube.py:265-277 feeding
 * the first nn.Linear of librubiks/model.py:123-127,150-157) on the matrix cores, without materialising the
 * one-hot matrix: the one-hot A-fragments of v_mfma_f32_32x32x16_{f16,bf16} are generated in registers from the
 * cube codes and a 128-column slice of W1 is resident in LDS as the B operand.
 *   w1  : [H][480] row-major = the nn.Linear weight as stored, IEEE half if table_is_f16 != 0 (11 mantissa bits:
 *         the default whenever every weight fits half's range), else bf16
 *   bias: float[H], out: bf16 [n][H];  H: multiple of 128;  activation: 0 = none, 1 = ReLU, 2 = ELU(alpha)
 * Algorithmic HBM bytes per state: 20 in + 2 H out (W1 is 0.96 H KB, L2-resident). */
#define RC_ACT_NONE 0
#define RC_ACT_RELU 1
#define RC_ACT_ELU 2
int rc_first_layer_mfma_bf16(const int8_t *soa, size_t n, size_t stride, const uint16_t *w1, const float *bias,
                             uint16_t *out, size_t H, int activation, float alpha, int table_is_f16, rc_stream_t stream);

/* In-place ReLU / ELU(alpha) of a contiguous bf16 tensor of n elements (n % 8 == 0): the activation pass between
 * two library GEMMs (model.py:150-157: Linear -> activation), 16 bytes per lane.  4 B of HBM traffic per element. */
int rc_act_bf16_inplace(uint16_t *x, size_t n, int activation, float alpha, rc_stream_t stream);

/* A hidden layer of the bf16 engine as ONE kernel: out = act(a w^T + bias) in bf16, fp32 accumulation on MFMA
 * (model.py:123-127,150-157).  a: bf16 [n_rows][k], w: bf16 [n_out][k] (nn.Linear layout), bias: float[n_out], out: bf16
 * [n_rows][n_out].  The kernel of rc_split_gemm_f16 (below) with one product instead of three: 352 x 256 tiles (tile 1,
 * n_out % 256 == 0) or 352 x 128 (tile 3, n_out % 128 == 0), tile 0 = choose; k % 64 == 0.  Replaces the library GEMM +
 * rc_act_bf16_inplace where it is the faster of the two (librubiks/model.py::InferenceNet decides by shape). */
int rc_gemm_bias_act_bf16(const uint16_t *a, const uint16_t *w, const float *bias, size_t n_rows, size_t n_out, size_t k,
                          int activation, float alpha, uint16_t *out, int tile, rc_stream_t stream);

/* ---- fp32-accurate network on the f16 matrix cores (f16x3 split) -------------------------------------------------
 * A float x travels as two IEEE halves, x = hi + lo * 2^-11 with hi = half(x), lo = half((x - hi) * 2^11); a layer is
 *   y = act(hi_x W_hi^T + 2^-11 (hi_x W_lo^T + lo_x W_hi^T) + b)      (fp32 accumulation on MFMA, library GEMMs)
 * which is closer to the float64 result than an fp32 GEMM (librubiks/model.py::SplitF32Net; replaces the fp32 forward
 * of librubiks/model.py:131-141).  These two kernels build the GEMM operands:
 *   rc_oh_split_f16   out[r] = [onehot(r), onehot(r) * 2^-11] as IEEE half, row pitch 960 (the one-hot is exact in half:
 *                     its product with [W_hi | W_lo] IS the input layer)                      (cube.py:265-277)
 *   rc_split_act_f16  y = act(c + corr_scale * c_corr + bias) per element of the fp32 GEMM outputs c, c_corr
 *                     [n_rows][n_cols] (c_corr may be NULL); writes out_hi_lo[r] = [hi(y row), lo(y row)] (row pitch
 *                     2 n_cols, may be NULL) and / or y itself to out_f32 (may be NULL).  n_cols % 8 == 0; ELU uses expm1f. */
int rc_oh_split_f16(const int8_t *soa, size_t n, size_t stride, uint16_t *out, rc_stream_t stream);
/* The whole input layer of that network in one kernel on the matrix cores, straight from the cube states:
 *   out_hi_lo[r] = [hi(y), lo(y)],  y = act(onehot(r) w_hi^T + 2^-11 onehot(r) w_lo^T + bias)      (row pitch 2 H halves)
 * w_hi, w_lo: IEEE half [H][480] row-major (the nn.Linear weight split as above), H % 64 == 0.  Replaces rc_oh_split_f16 +
 * the K = 960 GEMM + rc_split_act_f16 for the first layer (cube.py:265-277 + model.py:123-127,150-157 at fp32 accuracy). */
int rc_first_layer_split_f16(const int8_t *soa, size_t n, size_t stride, const uint16_t *w_hi, const uint16_t *w_lo,
                             const float *bias, uint16_t *out_hi_lo, size_t H, int activation, float alpha, rc_stream_t stream);
/* The same with the half-range flag of rc_split_layer_t: *range_flag |= 1 when an output is beyond +-65504 or not finite. */
int rc_first_layer_split_flag_f16(const int8_t *soa, size_t n, size_t stride, const uint16_t *w_hi, const uint16_t *w_lo,
                                  const float *bias, uint16_t *out_hi_lo, size_t H, int activation, float alpha,
                                  int32_t *range_flag, rc_stream_t stream);
/* The input layer as a sum of rows: a one-hot state times W is the sum of the 20 rows of W^T its cubies select,
 *   out_hi_lo[r] = [hi(y), lo(y)],  y = act(bias + sum_{j < 20} w_rows[24 j + code_j(r)])          (row pitch 2 H halves)
 * in fp32, in the order j = 0 .. 19 behind the bias (one order whatever the batch).  w_rows: float [480][H] = the nn.Linear
 * weight transposed, H % 64 == 0.  20 additions per output instead of 960 multiply-adds: what librubiks.model.SplitF32Net
 * runs (cube.py:265-277 + model.py:123-127,150-157); range_flag as above (may be NULL). */
int rc_first_layer_gather_f16(const int8_t *soa, size_t n, size_t stride, const float *w_rows, const float *bias,
                              uint16_t *out_hi_lo, size_t H, int activation, float alpha, int32_t *range_flag, rc_stream_t stream);
/* The same for packed rows: output row r is the layer of state src_map[r], for r < min(*rows_dev, n) only (both on the device,
 * both or neither; src_map[r] < n).  The launch is shaped by n, the rows that exist are shared evenly among its workgroups; a
 * state's outputs are the bits rc_first_layer_gather_f16 gives it.  form: 0 = by batch size, 1 / 2 = the small- / large-batch
 * form of the kernel (same bits). */
int rc_first_layer_gather_rows_f16(const int8_t *soa, size_t n, size_t stride, const float *w_rows, const float *bias,
                                   uint16_t *out_hi_lo, size_t H, int activation, float alpha, int32_t *range_flag,
                                   const uint32_t *rows_dev, const int32_t *src_map, int form, rc_stream_t stream);
int rc_split_act_f16(const float *c, const float *c_corr, float corr_scale, size_t n_rows, size_t n_cols, const float *bias,
                     int activation, float alpha, uint16_t *out_hi_lo, float *out_f32, rc_stream_t stream);

/* The same layer with its K loop cut in two for layers too narrow to fill the chip with 352 x 256 tiles: twice the workgroups,
 * raw fp32 accumulators out_partials[2][n_rows][n_out] with  y = act(out_partials[1] + 2^-11 * out_partials[0] + bias)  left to
 * the consumer (rc_head_split_f32 / rc_split_act_f16 take them as c = out_partials[1], c_corr = out_partials[0]).
 * n_out % 256 == 0, k % 128 == 0. */
int rc_split_gemm_partials_f16(const uint16_t *a_hi_lo, const uint16_t *w_lo_hi_hi, size_t n_rows, size_t n_out, size_t k,
                               float *out_partials, rc_stream_t stream);

/* Last hidden activation + output layer of that network in one pass (the fp32 counterpart of rc_head_bf16):
 *   y = act(c + corr_scale * c_corr + bias_h)  (never written),   out[i][o] = bias_o[o] + sum_k w[o][k] * y[i][k],  o < n_out <= 16
 * c, c_corr: the fp32 GEMM outputs [n][K] (c_corr may be NULL), K = 512 or 1024;  w: float [n_out][K];  out: float, row pitch 16
 * (columns >= n_out are written as 0): the layout rc_mcts_backup_head reads.  fp32 FMA chains on the exact fp32 MFMA.
 * Replaces rc_split_act_f16's fp32 output + the 13-wide fp32 library GEMM (model.py:124-129,150-159 at fp32 accuracy). */
int rc_head_split_f32(const float *c, const float *c_corr, float corr_scale, size_t n, size_t K, const float *bias_h,
                      int activation, float alpha, const float *w, const float *bias_o, size_t n_out, float *out, rc_stream_t stream);
/* The same for packed rows: only rows r < min(*rows_dev, n) of c / c_corr exist, and row r's outputs go to row src_map[r] < n
 * of out ([n][16]); rows of out that no r maps to are not written. */
int rc_head_split_rows_f32(const float *c, const float *c_corr, float corr_scale, size_t n, size_t K, const float *bias_h,
                           int activation, float alpha, const float *w, const float *bias_o, size_t n_out, float *out,
                           const uint32_t *rows_dev, const int32_t *src_map, rc_stream_t stream);
/* One hidden layer of that network as ONE kernel (own MFMA GEMM, fused epilogue; csrc/rubiks_gemm.hip):
 *   y = act(hi_x W_hi^T + 2^-11 (hi_x W_lo^T + lo_x W_hi^T) + bias)          (model.py:123-127,150-157 at fp32 accuracy)
 * a_hi_lo: [n_rows][2 k] halves (hi | lo), as the kernels above write it;  w_lo_hi_hi: [n_out][3 k] halves, the layer's
 * weight split and laid out [W_lo | W_hi | W_hi] (the order the K loop walks: both correction products, a 2^-11 scaling of
 * the accumulator, the main product);  exactly one of out_hi_lo ([n_rows][2 n_out] halves) and out_f32 ([n_rows][n_out])
 * is non-NULL.  k % 64 == 0;  tile: 0 = choose, 1 = 352 x 256 (n_out % 256 == 0), 3 = 352 x 128, 2 = 176 x 128 (n_out % 128 == 0).
 * Every tile walks K in the same order: a row's result does not depend on the tile or on the other rows of the launch.
 * Replaces two library GEMMs + rc_split_act_f16; the fp32 partial matrices never reach HBM. */
int rc_split_gemm_f16(const uint16_t *a_hi_lo, const uint16_t *w_lo_hi_hi, const float *bias, size_t n_rows, size_t n_out,
                      size_t k, int activation, float alpha, uint16_t *out_hi_lo, float *out_f32, int tile, rc_stream_t stream);

/* The layer kernels above with every option, as one request (zero-initialise, then fill what applies):
 *   y = post_scale * act(acc + bias + residual) + post_shift,   acc = the layer's products in fp32 on the matrix cores
 * residual: the skip connection of the reference's NonConvResBlock (librubiks/model.py:221-247), in the format of the
 * layer's own input ([n_rows][2 n_out] halves hi | lo; [n_rows][n_out] bf16 for rc_gemm_layer_bf16).  post_scale / post_shift
 * ([n_out] floats, both or neither): an eval-mode BatchNorm1d BEHIND the activation that cannot be folded into the next
 * Linear because a skip connection reads its output too (the last shared layer of the res_* architectures, model.py:249-264).
 * range_flag (device int, optional): OR-ed with 1 when a value written to out_hi_lo leaves IEEE half's range (|y| > 65504, or
 * not finite) -- the f16x3 split cannot carry it; librubiks.model.SplitF32Net then falls back to the fp32 GEMM chain.
 * Exactly one output.  rc_split_layer_f16: out_hi_lo | out_f32 | out_partials; with out_partials the K loop (3 k / 64 steps) is
 * cut into k_splits chunks (a divisor of 3 k / 64 leaving >= 2 steps per chunk, 2 .. 32; tile 0 / 1: 352 x 256 tiles, n_out % 256
 * == 0; tile 3: 352 x 128 tiles for small batches, n_out % 128 == 0; tile 7: 352 x 64), one workgroup per tile and chunk storing raw
 * accumulators out_partials[k_splits][n_rows][n_out] (no bias / residual / activation): the first rc_split_layer_corr_chunks(k,
 * k_splits) of them hold correction products only and still carry the factor 2^11, the others are in units of y
 * (rc_split_reduce_f16 finishes the layer).  rc_gemm_layer_bf16: a, w, residual, out_bf16 in bf16, one product. */
typedef struct rc_split_layer {
    const uint16_t *a;          /* [n_rows][2 k] halves hi | lo        (bf16 layer: [n_rows][k]) */
    const uint16_t *w;          /* [n_out][3 k] halves lo | hi | hi    (bf16 layer: [n_out][k]) */
    const float *bias;          /* [n_out] */
    const uint16_t *residual;   /* optional */
    const float *post_scale, *post_shift;   /* optional */
    uint16_t *out_hi_lo;        /* [n_rows][2 n_out] halves */
    float *out_f32;             /* [n_rows][n_out] */
    float *out_partials;        /* [k_splits][n_rows][n_out] */
    uint16_t *out_bf16;         /* [n_rows][n_out] (rc_gemm_layer_bf16 only) */
    size_t n_rows, n_out, k;
    int activation;             /* RC_ACT_* */
    float alpha;
    int tile;                   /* 0 = choose (see rc_split_gemm_f16) */
    int k_splits;               /* 0 / 1 = whole K per workgroup */
    int32_t *range_flag;        /* optional */
    int products;               /* rc_split_layer_f16: 0 / 3 = the three products of the split layer; 1 = ONE f16 product of a [n_rows][k]
                                 * and w [n_out][k] as they are (the input layer: a = [onehot | 2^-11 onehot], w = [W_hi | W_lo], k = 960) */
    const uint32_t *rows_dev;   /* optional (rc_split_layer_f16; tile 1 / 3, or out_partials): a device word R.  Only rows < min(R, n_rows) exist: the
                                 * grid stays the one n_rows gives, each of its row tiles takes an even share of the R rows in whole 16-row
                                 * fragments, rows >= R are neither computed nor written.  Rows < R get the bits a plain launch gives them. */
} rc_split_layer_t;
size_t rc_split_layer_struct_bytes(void);
int rc_split_layer_f16(const rc_split_layer_t *layer, rc_stream_t stream);
int rc_gemm_layer_bf16(const rc_split_layer_t *layer, rc_stream_t stream);
int rc_split_layer_corr_chunks(size_t k, int k_splits);   /* host only; -1 on a malformed request */
/* Finishes a layer whose products came as partial sums (rc_split_layer_f16 with out_partials, or the two fp32 library GEMMs
 * c_corr, c as partials[0], partials[1] with n_corr = 1):
 *   y = post_scale * act(sum_{p >= n_corr} partials[p] + 2^-11 sum_{p < n_corr} partials[p] + bias + residual) + post_shift
 * summed in the order p = 0, 1, ... (deterministic); partial p starts at partials + p * partial_stride floats.  Writes
 * out_hi_lo ([n_rows][2 n_cols] halves) and / or out_f32; n_cols % 8 == 0.  residual, post_*, range_flag as above. */
int rc_split_reduce_f16(const float *partials, size_t partial_stride, int n_partials, int n_corr, size_t n_rows, size_t n_cols,
                        const float *bias, const uint16_t *residual_hi_lo, int activation, float alpha, const float *post_scale,
                        const float *post_shift, uint16_t *out_hi_lo, float *out_f32, int32_t *range_flag, rc_stream_t stream);
/* The same on the rows < min(*rows_dev, n_rows) only (a device word); the others are neither read nor written. */
int rc_split_reduce_rows_f16(const float *partials, size_t partial_stride, int n_partials, int n_corr, size_t n_rows, size_t n_cols,
                             const float *bias, const uint16_t *residual_hi_lo, int activation, float alpha, const float *post_scale,
                             const float *post_shift, uint16_t *out_hi_lo, float *out_f32, int32_t *range_flag,
                             const uint32_t *rows_dev, rc_stream_t stream);

/* ---- network head: last activation + skinny output layer in one pass -----------------------------------------
 * out[i][o] = bias[o] + sum_k w[o][k] * act(x[i][k])   for o < n_out <= 16   (float out, row pitch 16)
 * Replaces the final activation pass and the 1024 -> 13 GEMM of the merged policy/value heads
 * (librubiks/model.py:124-129,150-159): the 2 KB activation row is read once, the weights live in registers.
 *   x: bf16 [n][K] raw pre-activations (bias already added), K = 1024;  w: bf16 [n_out][K];  bias: float[n_out]. */
int rc_head_bf16(const uint16_t *x, size_t n, size_t K, const uint16_t *w, const float *bias, size_t n_out,
                 float *out, int activation, float alpha, rc_stream_t stream);

/* ---- Autodidactic-iteration targets (librubiks/train.py:292-325) ----------------------------------
 * For state i with children 12 i .. 12 i + 11 (rc_expand12 order):
 *   q[k]   = values[12 i + k] + (child_solved[12 i + k] ? win_reward : -1)
 *   policy_target[i] = first argmax_k q[k];   value_target[i] = q[policy_target[i]]
 *   fix_mode 1 ("lapanfix")  : value_target[i] = 0 where state_solved[i]
 *   fix_mode 2 ("schultzfix"): value_target[i] = 0 where i % depth == 0
 * values: float[12 n]; child_solved: uint8[12 n]; state_solved: uint8[n] (may be NULL unless fix_mode 1). */
int rc_adi_targets(const float *values, const uint8_t *child_solved, const uint8_t *state_solved, size_t n,
                   size_t depth, float win_reward, int fix_mode, int64_t *policy_target, float *value_target,
                   rc_stream_t stream);

/* ---- batched MCTS: one independent tree per scramble, lock-step iterations -------------------
 *
 * Replaces the per-tree Python loop of librubiks/solving/agents.py:415-645 (class MCTS) for B
 * trees at once.  One iteration of every running tree =
 *     rc_mcts_expand  ->  [network on the 11 B child rows]  ->  rc_mcts_backup  ->  rc_mcts_select
 * Node indices are 1-based per tree, 0 = "no neighbour" (agents.py:419-421); node arrays are
 * tree-major with capacity + 1 rows per tree.  All pointers are device pointers owned by the
 * caller (zero-initialised once, before the first rc_mcts_plant); the struct itself lives in host memory.
 */
#define RC_MCTS_NODE_WORDS 64   /* 32-bit words per node record (see rc_mcts_t) */
#define RC_MCTS_RUNNING 0
#define RC_MCTS_SOLVED 1        /* a child of the expanded leaf is the solved cube (agents.py:540-543) */
#define RC_MCTS_EXHAUSTED 2     /* len + 12 > max_states (agents.py:476) or node capacity reached */
#define RC_MCTS_PATH_OVERFLOW 3 /* a PUCT descent reached max_path levels: the path store is exhausted (the reference has no limit,
                                 * agents.py:575-595; max_path is a resource bound the caller chooses, not a search parameter) */
#define RC_MCTS_ROOT_SOLVED 4   /* the scramble itself is solved (agents.py:468) */
#define RC_MCTS_CORRUPT 5       /* rc_mcts_complete_graph / rc_mcts_shorten met an index that does not name a node of the tree (1 .. n_nodes)
                                 * in its hash table or neighbour rows: the rows are not this tree's data.  The tree is left as it is.
                                 * Also rc_mcts_copy_trees, in the destination, for a source tree with more nodes than the destination has
                                 * rows per tree (n_nodes > capacity): nothing else of that tree is written. */

typedef struct rc_mcts {
    uint32_t n_trees;    /* B */
    uint32_t capacity;   /* largest node index per tree; capacity + 1 < 2^24 (32-bit byte offsets into a tree's 256-byte records) */
    uint32_t hash_size;  /* slots per tree, power of two, >= 2 * (capacity + 1) */
    uint32_t max_path;   /* levels the path store can hold per tree (>= 2; see "descent path" below): a whole number of path blocks */
    uint32_t rows_per_tree; /* network rows reserved per tree and iteration: 11 (see child_soa) */
    uint32_t node_words;    /* 32-bit words between consecutive nodes in N / W / P / nbr / rec: RC_MCTS_NODE_WORDS.  A forest that
                             * only waits for rc_mcts_complete_graph / rc_mcts_shorten (finished trees) may instead pass 12 with
                             * nbr as a plain [B][capacity + 1][12] array; every other entry point rejects that */
    /* per node, [B][capacity + 1] */
    void *keys;          /* uint32[4]: the 20 codes packed 5 bits each (6 codes per dword) */
    /* The per-action arrays of a node (the reference's agents.py:421-426 attributes) are the fields of ONE record of
     * RC_MCTS_NODE_WORDS 32-bit words = 256 bytes = two cache lines, [B][capacity + 1][64], 256-byte aligned:
     *   line 0: words 0-11 N | 12-23 W | 24-27 walk record (rec, below) | 28-31 spare       (what backup / re-validation write)
     *   line 1: words 32-43 P | 44-55 nbr | 56-63 spare                                      (read-only once the children exist)
     * Each pointer below addresses its field of node 0 of tree 0: entry a of node n is X[n * RC_MCTS_NODE_WORDS + a].
     * Re-deciding a level of the previous descent path reads one record and dirties one line of it.
     * The reference's L (virtual losses, agents.py:427) is NOT stored: every backup clears exactly the entries the descent
     * before it raised (agents.py:569-570, 589-591), so between iterations L == nu x (how often the pending descent path
     * path_node / path_act leaves a node by an action or arrives by its reverse), and zero once a tree is solved.  The
     * kernels take their loss counts from the path; MCTSForest.tree_arrays() reports L from it. */
    int32_t *nbr;        /* x12  neighbors   (agents.py:421) */
    float *P;            /* x12  policy      (agents.py:423); values are float32-exact in the reference too */
    float *W;            /* x12  max value   (agents.py:426) */
    int32_t *N;          /* x12  visit count (agents.py:425) */
    float *V;            /*      value       (agents.py:424) */
    uint8_t *leaf;       /*      is leaf     (agents.py:422) */
    int32_t *hash;       /* [B][hash_size] open addressing, slot = node index or 0; full-key compare via keys */
    /* per tree, [B] */
    int32_t *n_nodes;    /* len(agent) (agents.py:644-645) */
    int32_t *status;     /* RC_MCTS_* */
    int32_t *solved_idx; /* node index of the solved child, solve_action = its action */
    int32_t *solved_action;
    int32_t *iterations;
    int32_t *path_len;   /* number of nodes on the current descent path, root included */
    int32_t *pending;    /* 0, or (carried action + 2) of a descent that rc_mcts_select suspended at its level budget */
    /* The descent path (agents.py:581-582,592-593) has no length limit in the reference.  The path arrays path_node / path_act /
     * path_next / short_act are therefore BLOCKED: level k of tree t is element
     *     ((k >> path_block_log2) * B + t) << path_block_log2  |  (k & (2^path_block_log2 - 1)),
     * i.e. [max_path >> path_block_log2][B][2^path_block_log2] -- block 0 is the dense [B][block] array a shallow tree lives in,
     * and deeper blocks can be address space that gets memory only for the trees that go that deep (path_rows). */
    int32_t *path_node;  /* indices_visited (agents.py:581,592) */
    uint8_t *path_act;   /* actions_taken   (agents.py:582,593) */
    /* per iteration staging */
    int8_t *child_soa;   /* [20][child_stride]: network input: the NEW children of tree t's leaf, packed in child order at
                          * columns 11 t + rank.  A non-root leaf always has a known child (its parent), so 11 rows
                          * suffice; a root's iteration takes two steps (phase): [root, children 0..9], then [children 10, 11] */
    size_t child_stride;
    int32_t *child_idx;  /* [B][12] node index of every child of the expanded leaf */
    uint32_t *new_mask;  /* [B] bit k set iff child k was not in the tree before */
    uint8_t *expanded;   /* [B] 1 iff the tree expanded a leaf in the current iteration */
    int32_t *select_stats; /* optional (may be NULL): [B][8] = first sequentially walked level, new path length,
                              10-ns ticks spent re-validating the old path, ticks and shader cycles spent in the
                              sequential walk, revisited levels that fell back to float64, revisited levels,
                              line-following rounds << 16 | levels they appended */
    /* optional, only needed by rc_mcts_shorten (may be NULL otherwise) */
    int32_t *bfs;        /* [B][capacity + 1][2] scratch: {claim, parent << 4 | action} */
    uint8_t *short_act;  /* (blocked like path_act) shortened action queue of every solved tree; never longer than the tree's last path */
    int32_t *short_len;  /* [B] its length, -1 where no shortened queue was produced */
    /* per node: the 16-byte walk record, owned by the kernels (words 24-27 of the node record):
     *   uint32 {neighbour through best0, neighbour through best1, best0 | best1 << 8 | leaf << 16, 0}
     * best0 = the action a PUCT descent takes at the node while no virtual loss is pending there, best1 = the same
     * with one loss on best0 (the descent arrived through rev(best0)).  rc_mcts_init / rc_mcts_expand write leaf
     * records, rc_mcts_select refreshes the records of the path it re-validates and walks by them. */
    void *rec;
    /* per tree: the last ring_k descent paths ("lines"), used by rc_mcts_select to validate the likely continuation of
     * a descent many levels at a time.  Path number s (= the tree's iteration count when it was walked) lives in slot
     * s % ring_k; zero-initialised by the caller, owned by the kernels.  ring_k: a power of two, 1 .. 64. */
    uint32_t ring_k;
    int32_t *ring_node;  /* [B][ring_k][ring_levels]: the first ring_levels levels of a path (deeper levels are walked one by one) */
    uint8_t *ring_act;   /* [B][ring_k][ring_levels] action taken at each level, 15 at the path's leaf */
    int32_t *ring_len;   /* [B][ring_k] */
    /* per tree, [B]: 0 = ordinary iterations; 1 / 2 = first / second step of a planted root's own iteration (| 16: that
     * expansion found a solved child, reported as RC_MCTS_SOLVED when the second step has completed the tree) */
    int32_t *phase;
    /* Optional (NULL = every tree, in order): the trees the per-iteration entry points work on.  Workgroup i serves tree
     * active[i] (a negative entry = nobody) and that tree's network rows are 11 i .. 11 i + 10: rows are packed by POSITION in
     * the list, not by tree index.  Dropping finished trees from a running batch is therefore a new list -- no tree moves in
     * memory, whatever the capacity -- and the network runs on 11 n_active rows.  rc_mcts_complete_graph / rc_mcts_shorten
     * read it the same way (the finished trees to post-process).  Device pointer, n_active <= n_trees entries. */
    const int32_t *active;
    uint32_t n_active;
    /* rc_mcts_select's re-validation re-decides in float64 the levels float32 could not settle ("pass B"): from a list while
     * there are at most unc_list_cap of them (the kernel clamps it to 128, the production value), from a bitmap beyond.  Tests
     * lower it to drive the bitmap form with the few unsettled levels real networks produce; results do not depend on it. */
    uint32_t unc_list_cap;
    /* Optional (NULL = every row of the node arrays is backed by memory): [B] number of node rows (indices 0 .. mapped_rows[t] - 1)
     * of tree t that the per-node arrays keys / node records / V / leaf currently have memory behind -- for forests whose node
     * arrays are reserved address ranges mapped on demand (rc_vmm_*: the reference grows its arrays as a tree grows,
     * agents.py:450-459).  A tree whose next expansion would reach beyond it simply does not expand in that iteration (it stays
     * RUNNING, `expanded` stays 0, its iteration count does not advance) and tries again in the next one: the host maps ahead
     * of the trees' growth, the kernels never touch a row that is not there. */
    const int32_t *mapped_rows;
    /* ---- descent paths of any length (the reference walks until it meets a leaf, agents.py:575-595) ----
     * rc_mcts_select keeps the first lds_levels levels of the path it works on in LDS; deeper levels are read and written in
     * path_node / path_act in place, and chained by node through path_next (same blocked layout; only entries of levels >=
     * lds_levels are used).  Results do not depend on lds_levels (tests run 8 and 64 against the reference's traces). */
    uint32_t path_block_log2; /* log2 of the levels per path block (12 in production) */
    uint32_t lds_levels;      /* 1 .. 4096 */
    uint32_t ring_levels;     /* levels per ring line, 1 .. 4096 (the line tag holds 12 bits of level) */
    uint32_t *path_next;      /* scratch owned by the kernels */
    /* Optional (NULL = max_path for every tree): [B] levels of tree t's path blocks that have memory behind them (a multiple of
     * the block size).  A descent that reaches it is SUSPENDED (pending, as at a level budget) and resumes in the next call;
     * the host maps the next block in between.  Only a descent that reaches max_path itself ends the tree (PATH_OVERFLOW). */
    const int32_t *path_rows;
} rc_mcts_t;

/* sizeof(rc_mcts_t) as the library was compiled: a binding that mirrors the struct (ctypes, cgo, JNI) checks its own
 * layout against it before the first call.  Host-only, needs no device. */
size_t rc_mcts_struct_bytes(void);

/* (Re)starts trees: for i < n_slots, tree slots[i] (or tree i if slots is NULL) is emptied -- its hash table is cleared,
 * nothing else needs to be -- and gets roots_soa column first_col + i as node 1; a solved root gets RC_MCTS_ROOT_SOLVED.
 * The root is evaluated and expanded (agents.py:466-473 and the first expand_leaf) inside the next two ordinary
 * iterations, on the tree's own 11 network rows: see `phase`.  Other trees of the forest are not touched, so finished
 * trees of a running batch can hand their slots to waiting scrambles between two iterations. */
int rc_mcts_plant(const rc_mcts_t *m, const int32_t *slots, uint32_t n_slots, const int8_t *roots_soa, size_t stride,
                  size_t first_col, rc_stream_t stream);
/* expand_leaf part 1 (agents.py:505-544): 12 children of the path's leaf, dedup against the tree,
 * new indices in child order, links both ways, first solved child. */
int rc_mcts_expand(const rc_mcts_t *m, uint32_t max_states, rc_stream_t stream);
/* expand_leaf part 2 (agents.py:555-571): P, V of new children, W/N/L updates along the path.
 * probs = softmax(policy logits) rows, values = value head, both for the 11 B child rows. */
int rc_mcts_backup(const rc_mcts_t *m, const float *probs, const float *values, rc_stream_t stream);
/* Same as rc_mcts_backup, but straight from the network's head output: row r of `head` (bf16 when
 * head_is_bf16 != 0, else float; `ld` elements per row) holds the 12 policy logits followed by the value.
 * P = softmax(logits) is evaluated in float32 inside the kernel (max-subtracted, expf), which removes the
 * separate cast / slice / softmax / copy launches of the generic path. */
int rc_mcts_backup_head(const rc_mcts_t *m, const void *head, size_t ld, int head_is_bf16, rc_stream_t stream);
/* find_leaf (agents.py:575-595): PUCT descent with virtual loss, float64 arithmetic as NumPy's.
 * level_budget = 0: every running tree descends to its leaf (strict lock step).
 * level_budget > 0: a tree walks at most that many NEW levels per call; if it has not reached a leaf it is
 * suspended (pending) and resumes in the next call, and rc_mcts_expand / rc_mcts_backup skip it meanwhile.
 * Each tree still performs exactly the reference's sequence of iterations; only their timing changes, so the
 * slowest descent of the batch no longer sets the pace of every iteration. */
int rc_mcts_select(const rc_mcts_t *m, double c, uint32_t level_budget, rc_stream_t stream);
/* rc_mcts_backup (or rc_mcts_backup_head) followed by rc_mcts_select as ONE kernel with the same results: the path part of
 * the backup is applied by the lanes that re-decide the path's levels, to the rows they hold in registers anyway. */
int rc_mcts_backup_select(const rc_mcts_t *m, const float *probs, const float *values, double c, uint32_t level_budget,
                          rc_stream_t stream);
int rc_mcts_backup_select_head(const rc_mcts_t *m, const void *head, size_t ld, int head_is_bf16, double c, uint32_t level_budget,
                               rc_stream_t stream);
/* The tree side of an iteration as ONE launch: rc_mcts_backup_select (rc_mcts_step) / rc_mcts_backup_select_head
 * (rc_mcts_step_head) followed by the rc_mcts_expand of the NEXT iteration, done by the wave that walked to the leaf.  An
 * iteration is then  [network on the rows the previous step left] -> rc_mcts_step*;  trees enter through
 * rc_mcts_plant_expanded, which is rc_mcts_plant + the root's expansion (its rows use list position == tree index: every tree
 * listed in order, as while scrambles are still waiting for slots).  Results are those of the three-kernel form.
 * Launch shape: 256 threads per tree in a forest of more than 512 listed trees, 512 / 1 024 threads and four waves checking a
 * descent line together below that (idle CUs; same results).  RUBIKS_STEP_THREADS=256|512|1024 and RUBIKS_LINE_WAVES=1|4 in the
 * environment pin the two choices, for A/B measurements only (read once per process). */
int rc_mcts_plant_expanded(const rc_mcts_t *m, const int32_t *slots, uint32_t n_slots, const int8_t *roots_soa, size_t stride,
                           size_t first_col, uint32_t max_states, rc_stream_t stream);
int rc_mcts_step(const rc_mcts_t *m, const float *probs, const float *values, double c, uint32_t level_budget, uint32_t max_states,
                 rc_stream_t stream);
int rc_mcts_step_head(const rc_mcts_t *m, const void *head, size_t ld, int head_is_bf16, double c, uint32_t level_budget,
                      uint32_t max_states, rc_stream_t stream);
/* The five entry points above that take the exploration constant, with c per tree: for forests whose trees are searched under
 * different c (a grid over c as one pool: the reference's GridSearch, librubiks/solving/hyper_optim.py:94-111, runs one agent
 * per point).  c_each is a device array of n_trees doubles (8-byte aligned), indexed by TREE INDEX -- not by position in
 * rc_mcts_t::active --, read once per workgroup: tree t's PUCT scores (agents.py:583-585) use c_each[t] wherever the scalar
 * forms use c -- the float32 walk, its float64 re-evaluations and the re-validation of the previous path.
 * What the kernel relies on: a tree's c is CONSTANT from its plant to its end.  The 16-byte walk records (best0 / best1) and
 * the ring lines cache decisions made under it and are re-derived only for the nodes of the path being backed up; the caller
 * writes c_each[t] (in stream order) before the plant of tree t's root and leaves it alone while the tree runs.
 * Everything else is what the scalar forms do, launch shapes included (rc_mcts_step*_each: 256 / 512 / 1 024 threads, one or
 * four line waves): a forest whose array holds one value evolves exactly as under the scalar export with that value.
 * NULL m or c_each: RC_ERR_NULL; c_each not 8-byte aligned: RC_ERR_ALIGN -- both before anything is launched. */
int rc_mcts_select_each(const rc_mcts_t *m, const double *c_each, uint32_t level_budget, rc_stream_t stream);
int rc_mcts_backup_select_each(const rc_mcts_t *m, const float *probs, const float *values, const double *c_each,
                               uint32_t level_budget, rc_stream_t stream);
int rc_mcts_backup_select_head_each(const rc_mcts_t *m, const void *head, size_t ld, int head_is_bf16, const double *c_each,
                                    uint32_t level_budget, rc_stream_t stream);
int rc_mcts_step_each(const rc_mcts_t *m, const float *probs, const float *values, const double *c_each, uint32_t level_budget,
                      uint32_t max_states, rc_stream_t stream);
int rc_mcts_step_head_each(const rc_mcts_t *m, const void *head, size_t ld, int head_is_bf16, const double *c_each,
                           uint32_t level_budget, uint32_t max_states, rc_stream_t stream);
/* The network rows that hold a state, packed.  The tree at list position i fills the first cnt(i) of its 11 row slots: 0 if it
 * did not expand, 11 / 2 in the two root phases, else the number of its new children.  One workgroup scans the counts in list
 * order:  first[i] = sum of cnt(j < i),  *rows = R = their total,  src[first[i] + j] = 11 i + j  (first: [list length], src:
 * [11 x list length], all on the device).  No atomics: the placement is a function of the list and the trees' state alone.  The
 * network then runs on the R packed rows (rc_first_layer_gather_rows_f16, rc_split_layer_t::rows_dev, rc_split_reduce_rows_f16)
 * and rc_head_split_rows_f32 writes every output to its row slot: the tree kernels read the layout they always read. */
int rc_mcts_row_map(const rc_mcts_t *m, uint32_t *rows, int32_t *first, int32_t *src, rc_stream_t stream);
/* _complete_graph (agents.py:597-611) for every tree with status RC_MCTS_SOLVED: each leaf is linked, both
 * ways, to those of its 12 children that already exist in the tree (looked up in the tree's hash table). */
int rc_mcts_complete_graph(const rc_mcts_t *m, rc_stream_t stream);
/* _shorten_action_queue (agents.py:613-633) for every solved tree, after rc_mcts_complete_graph: breadth-first
 * search over the tree's neighbour table from the root to the solved node, discovering nodes in exactly the
 * order of the reference's FIFO queue (frontier order, then action order), so the returned queue is the
 * reference's.  Overwrites the tree's hash table (used as the two frontier arrays). */
int rc_mcts_shorten(const rc_mcts_t *m, rc_stream_t stream);

/* Copies the finished (or suspended) trees src_trees[0 .. n) of `src` into slots dst_first .. dst_first + n - 1 of `dst`: rows
 * 0 .. n_nodes of keys, leaf and -- into a search forest (dst->node_words == RC_MCTS_NODE_WORDS) -- the node records and V, or --
 * into a results-only forest (dst->node_words == 12) -- the neighbour rows alone; plus the tree's whole hash table.  Only rows
 * that exist are touched (both forests may be mapped on demand); the per-tree words are the caller's to copy.  Same capacity
 * and hash_size on both sides; src must be a search forest.  Replaces whole-capacity tensor copies (capacity x 285 B per
 * tree) where finished trees leave a running forest (MCTSForest.bury / subset). */
int rc_mcts_copy_trees(const rc_mcts_t *src, const rc_mcts_t *dst, const int32_t *src_trees, uint32_t n, uint32_t dst_first,
                       rc_stream_t stream);

/* ---- node storage on demand (HIP virtual memory management) ---------------------------------------------------------------
 * The reference's node arrays grow by doubling as a tree grows (librubiks/solving/agents.py:450-459): max_states = 175 000 costs
 * only the nodes a search creates.  rc_vmm_reserve reserves an address range of the array's full size, rc_vmm_map puts memory
 * behind [offset, offset + bytes) of it, chunk by chunk (chunk_bytes: a multiple of 2 MiB; a chunk already mapped is left
 * alone); addresses never change, so structs, kernels and captured graphs are unaffected.  rc_vmm_map is host-synchronous and
 * may be called while kernels work on other parts of the range (*out_new_bytes = bytes it added, also when it fails part of
 * the way).  rc_vmm_release: after the caller has synchronised; unmaps, flushes the GPU's translations and puts the address
 * range on the idle list of its size class (reservations are whole powers of two), where the next rc_vmm_reserve of that class
 * finds it: rc_vmm_retired_bytes = address space idle on those lists, bounded by one range per class and live overlap.
 * Diagnosis: every call is recorded (the last 512 events in memory; all of them, flushed line by line, in the file the
 * environment variable RUBIKS_VMM_LOG names, "stderr" = stderr); rc_vmm_dump writes the live ranges with their mapped chunk runs,
 * the idle ranges and the recent events as text (at most cap - 1 characters; *out_needed = full length incl. NUL);
 * rc_vmm_classify says what an address -- that of a GPU memory access fault, say -- is to the library at this moment;
 * rc_vmm_chunk_map copies the per-chunk "has memory" flags of a range. */
#define RC_VMM_ADDR_UNKNOWN 0    /* not inside any reservation of this library */
#define RC_VMM_ADDR_MAPPED 1     /* live range, memory behind the chunk */
#define RC_VMM_ADDR_UNMAPPED 2   /* live range, NO memory behind the chunk: a row touched before it was mapped */
#define RC_VMM_ADDR_SLACK 3      /* live reservation, outside the range handed out (alignment slack, rest of the size class) */
#define RC_VMM_ADDR_IDLE 4       /* a released range waiting for reuse: nothing mapped */
int rc_vmm_granularity(size_t *out_bytes);
int rc_vmm_reserve(size_t bytes, size_t chunk_bytes, void **out_base);
int rc_vmm_map(void *base, size_t offset, size_t bytes, size_t *out_new_bytes);
int rc_vmm_mapped_bytes(void *base, size_t *out_bytes);
int rc_vmm_chunk_map(void *base, uint8_t *out_flags, size_t cap, size_t *out_chunks);
int rc_vmm_release(void *base);
int rc_vmm_retired_bytes(size_t *out_bytes);
int rc_vmm_classify(const void *addr, int *out_kind, void **out_base, size_t *out_offset);
int rc_vmm_dump(char *out, size_t cap, size_t *out_needed);

/* ---- batched weighted A*: B independent problems, N expansions each per iteration --------------
 *
 * Replaces the per-problem Python loop of librubiks/solving/agents.py:171-413 (class AStar).
 * One iteration of every running problem =
 *     rc_astar_pop_expand -> [prefix sum of new_count on the caller's side] -> rc_astar_gather_new
 *     -> [value network on the compacted new states] -> rc_astar_push_relax
 * Node indices are 1-based per problem (index 0 unused, agents.py:189); arrays are problem-major
 * with capacity + 1 rows.  Device pointers, zero-initialised by the caller except `claim`, which
 * must be filled with INT32_MAX.
 * Invariant: between iterations every `claim` row is INT32_MAX again -- the row that wins an election
 * in rc_astar_pop_expand or rc_astar_push_relax releases it -- so a slot replanted by rc_astar_plant
 * needs no claim rows rewritten.
 * Continuous batching: after an iteration, rc_astar_solutions reads the finished problems' queues and
 * rc_astar_plant restarts their slots from waiting scrambles; the other problems are not touched.
 */
#define RC_ASTAR_RUNNING 0
#define RC_ASTAR_SOLVED 1        /* a NEW state of the batch is the solved cube (agents.py:321-323) */
#define RC_ASTAR_EXHAUSTED 2     /* len + 12 N > max_states (agents.py:236) or capacity reached */
#define RC_ASTAR_OPEN_EMPTY 3    /* open list ran dry (the reference would spin; defined as unsolved) */
#define RC_ASTAR_ROOT_SOLVED 4   /* agents.py:230 */

typedef struct rc_astar {
    uint32_t n_problems; /* B */
    uint32_t capacity;   /* largest node index per problem */
    uint32_t hash_size;  /* slots per problem, power of two, >= 2 * (capacity + 1) */
    uint32_t expansions; /* N (agents.py:218) */
    /* per node, [B][capacity + 1] */
    void *keys;              /* uint32[4] packed state (as rc_mcts) */
    int32_t *G;              /* path cost; integer valued in the reference's float array (agents.py:203,311) */
    int32_t *parents;        /* agents.py:204 */
    uint8_t *parent_actions; /* agents.py:205 */
    int32_t *claim;          /* scratch for first-/last-occurrence election, INT32_MAX when idle */
    int32_t *hash;           /* [B][hash_size]: > 0 node index, < 0 pending child row -(row+1), 0 empty */
    /* open list: binary min-heap on (cost, index), [B][capacity + 1] */
    double *heap_cost;
    int32_t *heap_idx;
    /* per problem, [B] */
    int32_t *heap_size;
    int32_t *n_nodes;        /* len(agent) (agents.py:409-410) */
    int32_t *status;         /* RC_ASTAR_* */
    int32_t *solved_idx;
    int32_t *iterations;
    int32_t *n_popped;       /* parents expanded in the current iteration */
    int32_t *new_count;      /* states added in the current iteration */
    /* per iteration staging, [B][N] and [B][12 N] */
    int32_t *popped;         /* node indices in pop order (agents.py:238-239) */
    void *child_keys;        /* uint32[4] per child row 12 p + k */
    int32_t *child_node;     /* node index of a seen child / hash slot of an unseen one */
    int32_t *row_tmp;        /* scratch per row (relaxation values) */
    uint8_t *row_flags;      /* bit0 first occurrence & unseen (new state), bit1 first occurrence & seen */
} rc_astar_t;

/* Root = node 1 with G = 0 and cost 0 on the open list (agents.py:233-234). */
int rc_astar_init(const rc_astar_t *a, const int8_t *roots_soa, size_t stride, rc_stream_t stream);
/* Pops min(len(open), N) lowest (cost, index) nodes, expands their 12 N children, dedups against
 * the problem's states and inside the batch (first occurrence in row order, agents.py:286-295),
 * appends the new states with G, parent, parent_action (agents.py:299-313).  Sets new_count. */
int rc_astar_pop_expand(const rc_astar_t *a, uint32_t max_states, rc_stream_t stream);
/* Writes the new states of every problem into out_soa at columns new_offset[b] .. (exclusive prefix
 * sum of new_count, B + 1 entries) -- the compacted network input of this iteration. */
int rc_astar_gather_new(const rc_astar_t *a, const int32_t *new_offset, int8_t *out_soa, size_t stride,
                        rc_stream_t stream);
/* cost = lambda * G - value (float64, agents.py:383), push on the open list (agents.py:315-317),
 * win check on the new states (agents.py:321-323), else relaxation of the first-seen children
 * (agents.py:326-328,333-367).  values[new_offset[b] + i] belongs to new state i of problem b. */
int rc_astar_push_relax(const rc_astar_t *a, const int32_t *new_offset, const float *values, double lambda,
                        rc_stream_t stream);
/* The two phases above with N and lambda per problem, for batches whose problems are searched under different settings (a grid
 * of (lambda, expansions) points as one pool: the reference's GridSearch, librubiks/solving/hyper_optim.py:94-111, runs one
 * agent per point).  expansions[b] and lambda[b] are device arrays of n_problems entries: problem b's own N (agents.py:218)
 * and lambda (agents.py:380-383).  Here a->expansions is the row stride of the per-iteration staging -- popped is
 * [B][a->expansions], child_* and row_* are [B][12 a->expansions], as above -- and the upper bound of every expansions[b].
 * rc_astar_pop_expand_each: problem b is exhausted when n + 12 expansions[b] > max_states (agents.py:236) or > capacity, and
 * pops min(len(open), expansions[b]) nodes (agents.py:238).  expansions[b] is read clamped to 0 .. a->expansions, so no value
 * leads outside the problem's own staging rows; a clamped 0 pops nothing and ends the problem as RC_ASTAR_OPEN_EMPTY.
 * rc_astar_push_relax_each: cost = lambda[b] * G - value in float64, product and sum rounded separately (agents.py:383).
 * Everything else is what rc_astar_pop_expand / rc_astar_push_relax do: a batch whose arrays all hold a->expansions and one
 * lambda evolves exactly as under those. */
int rc_astar_pop_expand_each(const rc_astar_t *a, uint32_t max_states, const int32_t *expansions, rc_stream_t stream);
int rc_astar_push_relax_each(const rc_astar_t *a, const int32_t *new_offset, const float *values, const double *lambda,
                             rc_stream_t stream);
/* Restarts listed problem slots of a running batch: for i < n, slot slots[i] (device int32 list) gets roots_soa column
 * first_col + i as its root -- its hash row is cleared, then it holds exactly what rc_astar_init writes for a problem (node 1,
 * G 0, open list (0, 1), counters, status incl. RC_ASTAR_ROOT_SOLVED, solved_idx -1).  A listed index outside
 * 0 .. n_problems - 1 is skipped (nothing is written for it).  Pass the column, not a shifted pointer: the SoA's planes are
 * 16-byte aligned only at column 0.  Needs stride >= first_col + n. */
int rc_astar_plant(const rc_astar_t *a, const int32_t *slots, uint32_t n, const int8_t *roots_soa, size_t stride,
                   size_t first_col, rc_stream_t stream);
/* Action queues of the listed problems (device int32 list of n problem indices), the walk of agents.py:244-251 from
 * solved_idx back to node 1: row i of the [n][width] byte table `queues` gets problem problems[i]'s queue in root-to-goal
 * order, lengths[i] its length.  lengths[i]: 0 for RC_ASTAR_ROOT_SOLVED, RC_ASTAR_PATH_UNSOLVED for any other status but
 * RC_ASTAR_SOLVED; a queue longer than `width` reports its length and leaves its row unwritten (read it again with a wider
 * table).  Every index read from memory is checked against the problem's 1 .. n_nodes, and a walk ends within n_nodes steps:
 * otherwise RC_ASTAR_PATH_CORRUPT (the rows are not this problem's), and RC_ASTAR_PATH_NO_PROBLEM for a listed index outside
 * 0 .. n_problems - 1. */
#define RC_ASTAR_PATH_UNSOLVED (-1)
#define RC_ASTAR_PATH_CORRUPT (-2)
#define RC_ASTAR_PATH_NO_PROBLEM (-3)
int rc_astar_solutions(const rc_astar_t *a, const int32_t *problems, uint32_t n, uint8_t *queues, uint32_t width,
                       int32_t *lengths, rc_stream_t stream);

/* ---- batched EGVM: S games of W epsilon-greedy rollouts each, all advanced in lock step ------------
 *
 * Replaces the per-game Python loop of librubiks/solving/agents.py:649-726 (class EGVM).  A round of every running game =
 *     for d in 0 .. D - 1:  [network on the S W rows of rows_soa: 12 logits + value per row] -> rc_egvm_step(d)
 *     [network on the rows once more: the values of the last depth] -> rc_egvm_round_end
 * Row g W + w of rows_soa is worker w of the game in slot g.  The random decisions of a round are the host's (one byte per row
 * and depth, drawn from the game's own np.random stream in the reference's order, agents.py:694-698): they do not depend on the
 * device, so a round runs without the host.  The value of the state a worker reaches at depth d arrives with the forward pass
 * of step d + 1, so no W x D array of visited states is kept (agents.py:681-682): every row keeps a running best of (value,
 * depth, state), replaced on a strictly greater value, and the round ends on the best row of lowest index -- np.argmax over
 * the reference's worker-major index w D + d (agents.py:674-676), a NaN counting as the maximum.
 * Device pointers; nothing needs initialising except through rc_egvm_plant.
 */
#define RC_EGVM_RUNNING 0
#define RC_EGVM_SOLVED 1        /* a worker reached the solved cube (agents.py:710-713) */
#define RC_EGVM_EXHAUSTED 2     /* nodes + W D > max_states (agents.py:665) */
#define RC_EGVM_QUEUE_FULL 3    /* the round's path prefix does not fit the queue row: nothing was written for that round */
#define RC_EGVM_ROOT_SOLVED 4   /* agents.py:661 */
#define RC_EGVM_NO_HIT 0xffffffffu
#define RC_EGVM_POLICY 255      /* decision byte: the first maximum of the row's 12 logits; 0 .. 11: that action */

typedef struct rc_egvm {
    uint32_t n_slots;     /* S: games searched at a time */
    uint32_t workers;     /* W (agents.py:651), 1 .. 65 535 */
    uint32_t depth;       /* D (agents.py:652), 1 .. 32 768 */
    uint32_t queue_width; /* bytes per row of `queues` */
    size_t stride;        /* bytes between the planes of rows_soa and of best_soa: multiple of 16, >= round_up(S W, 16) */
    int8_t *rows_soa;     /* [20][stride] the workers' current states = the network's input */
    int8_t *best_soa;     /* [20][stride] per row: the visited state of highest value so far in this round */
    float *best_value;    /* [S W] its value ... */
    int32_t *best_depth;  /* [S W] ... and depth (-1: none yet) */
    uint8_t *paths;       /* [S][W][D] actions taken in this round (agents.py:680) */
    uint32_t *hit;        /* [S] (d << 16 | w) of the round's first solved worker: first depth, then lowest worker; RC_EGVM_NO_HIT */
    int8_t *current;      /* [S][20] the state the game's next round starts from (agents.py:676) */
    uint8_t *queues;      /* [S][queue_width] action queues (agents.py:677,712) */
    int64_t *status;      /* [S] RC_EGVM_* */
    int64_t *nodes;       /* [S] len(agent) (agents.py:672,711) */
    int64_t *queue_len;   /* [S] */
    int64_t *rounds;      /* [S] rounds completed since the plant */
} rc_egvm_t;

/* Depth step d of the round (agents.py:690-716) for all S W rows in one launch: with d > 0 the value column of `head` is the
 * value of the row's current state and updates its running best; the action is decisions_row[row] (0 .. 11) or, for
 * RC_EGVM_POLICY, the first maximum of the row's 12 logits as np.argmax finds it (a NaN is the maximum); the cube is turned,
 * paths[g][w][d] written, and a solved row claims its game's hit word with atomicMin.  Rows of games that are not running, or
 * whose hit word names an earlier depth, are not touched.  `head` is [S W][ld] with 12 logits then the value per row, float or
 * bf16 (head_is_bf16), ld >= 13: what rc_mcts_step_head reads.  decisions_row: S W bytes. */
int rc_egvm_step(const rc_egvm_t *e, uint32_t d, const uint8_t *decisions_row, const void *head, size_t ld, int head_is_bf16,
                 rc_stream_t stream);
/* End of the round for every running game (agents.py:666-677,710-713).  With a hit (d, w): nodes += (d + 1) W, the queue gets
 * paths[w][0 .. d], status RC_EGVM_SOLVED.  Without: values_last[row] (float [S W]) is the value of the row's state after the
 * last depth and is folded into the running bests, the best row of lowest index (w*, d*) is found, nodes += W D, the queue
 * gets paths[w*][0 .. d*], every worker of the game restarts from that state, and the game is RC_EGVM_EXHAUSTED if
 * nodes + W D > max_states.  A prefix that does not fit the queue row is not written: RC_EGVM_QUEUE_FULL.  Resets the
 * per-round words (hit, best_depth). */
int rc_egvm_round_end(const rc_egvm_t *e, const float *values_last, uint64_t max_states, rc_stream_t stream);
/* For i < n, slot slots[i] (device int32 list) restarts from roots_soa column first_col + i: every worker and `current` hold
 * that state, counters and queue length are 0, status RC_EGVM_RUNNING or, for the solved cube, RC_EGVM_ROOT_SOLVED.  Other slots
 * are not touched, nor is anything written for a listed index outside 0 .. n_slots - 1.  Needs stride >= first_col + n. */
int rc_egvm_plant(const rc_egvm_t *e, const int32_t *slots, uint32_t n, const int8_t *roots_soa, size_t stride, size_t first_col,
                  rc_stream_t stream);

/* Host only (no GPU needed): the decision tables of one round for n games, drawn from the games' own MT19937 streams exactly as
 * the reference draws them from np.random (agents.py:694-698): per depth step W doubles as RandomState.random_sample makes them
 * (two 32-bit outputs each: (a >> 5) * 2^26 + (b >> 6), over 2^53), compared with cdf0 -- what RandomState.choice(2, W, p=[1 - eps,
 * eps]) does with the normalised cumulative sum of p -- then, for every worker whose double is >= cdf0 and in worker order, an
 * action as RandomState.randint(0, 12, k) draws it (32-bit outputs masked to 4 bits until one is <= 11).  Game games[i] has its
 * generator in mt_keys[games[i]][624] / mt_pos[games[i]] (RandomState.get_state()'s key and pos; both are advanced) and plays
 * in slot slots[i]: table[d * table_stride + slots[i] * W + w] = action 0 .. 11 or RC_EGVM_POLICY.  n_rows: rows of the table
 * (every slots[i] * W + W must fit; table_stride >= n_rows); n_games: rows of mt_keys. */
int rc_egvm_draw(uint32_t *mt_keys, int32_t *mt_pos, uint32_t n_games, const int32_t *games, const int32_t *slots, uint32_t n,
                 double cdf0, uint32_t workers, uint32_t depth, uint8_t *table, size_t table_stride, size_t n_rows);

/* ---- one-step rollout agents: S games advanced one move per launch, in lock step ------------------
 *
 * Replaces the per-move Python of librubiks/solving/agents.py:23-38 (Agent.search) with the `_step` of RandomSearch (:82-90),
 * PolicySearch (:132-151) and ValueSearch (:154-169).  A move of every running game =
 *     policy / random:  [network on the S rows of states_soa: 12 logits per row] -> rc_rollout_step_policy
 *     value:            [network on the 12 S rows of kids_soa: one value per row] -> rc_rollout_step_value
 * The random numbers are the host's (rc_rollout_draw: one byte or one double per game and move, from the game's own np.random
 * stream), so any number of moves is queued without the host.  Device pointers; nothing needs initialising except through
 * rc_rollout_plant.  kids_soa and kid_solved are needed by the value step (and by a plant with children) only.
 */
#define RC_ROLLOUT_RUNNING 0
#define RC_ROLLOUT_SOLVED 1        /* the move reached the solved cube (agents.py:33-35) */
#define RC_ROLLOUT_EXHAUSTED 2     /* max_steps moves made */
#define RC_ROLLOUT_QUEUE_FULL 3    /* the move's byte does not fit the queue row: the move was not made */
#define RC_ROLLOUT_ROOT_SOLVED 4   /* agents.py:29 */
#define RC_ROLLOUT_BAD_POLICY 5    /* a NaN probability where the policy is sampled (np.random.choice raises there) */
#define RC_ROLLOUT_POLICY 255      /* decision byte: ask the network; 0 .. 11: that action */

typedef struct rc_rollout {
    uint32_t n_slots;     /* S: games played at a time */
    uint32_t queue_width; /* bytes per row of `queues` */
    size_t stride;        /* bytes between the planes of states_soa; kids_soa has 12 stride: multiple of 16, >= round_up(S, 16) */
    int8_t *states_soa;   /* [20][stride] current states = the policy network's input */
    int8_t *kids_soa;     /* [20][12 stride] child row 12 g + k = action k on state g (rc_expand12 order) = the value network's input */
    uint8_t *kid_solved;  /* [12 stride] multi_is_solved of the children (agents.py:158) */
    uint8_t *queues;      /* [S][queue_width] action queues (agents.py:32) */
    int64_t *status;      /* [S] RC_ROLLOUT_* */
    int64_t *steps;       /* [S] moves made = len(agent) = len(action_queue) (agents.py:34,37) */
} rc_rollout_t;
size_t rc_rollout_struct_bytes(void);

/* For i < n, slot slots[i] (device int32 list) restarts from roots_soa column first_col + i (agents.py:26-29): steps 0, status
 * RC_ROLLOUT_RUNNING or, for the solved cube, RC_ROLLOUT_ROOT_SOLVED; with_children also writes the slot's 12 children and their
 * solved flags (what the first value step reads).  Other slots are not touched, nor is anything written for a listed index
 * outside 0 .. n_slots - 1.  Needs stride >= first_col + n. */
int rc_rollout_plant(const rc_rollout_t *r, const int32_t *slots, uint32_t n, const int8_t *roots_soa, size_t stride, size_t first_col,
                     int with_children, rc_stream_t stream);
/* One move of every running game by RandomSearch._step (agents.py:83-86) or PolicySearch._step (:138-142), in one launch.  The
 * action of game g is decisions_row[g] if that is 0 .. 11 (decisions_row NULL: every byte is RC_ROLLOUT_POLICY).  Otherwise,
 * with uniforms_row (double [S]), it is np.random.choice(12, p=softmax(logits)) for the double u = uniforms_row[g] that call
 * would draw: the fp32 softmax with the row maximum subtracted, its running sum in double divided by the total, and the number
 * of entries <= u, at most 11 (cdf.searchsorted(u, side="right")); a NaN probability ends the game RC_ROLLOUT_BAD_POLICY.
 * Without uniforms_row it is the first maximum of the 12 logits as np.argmax finds it (a NaN is the maximum) -- the reference
 * takes the maximum of their fp32 softmax, which differs only where the softmax rounds two distinct logits to one probability.
 * Then the cube is turned, the action appended to the queue row (a byte that does not fit: RC_ROLLOUT_QUEUE_FULL, nothing is
 * written and the cube stays), steps incremented, and the game is RC_ROLLOUT_SOLVED if the new state is the solved cube, else
 * RC_ROLLOUT_EXHAUSTED if steps == max_steps.  `head` is [S][ld], 12 logits first, float or bf16, ld >= 13 (what
 * rc_mcts_step_head and rc_egvm_step read); it may be NULL where every decision byte is an action -- a byte that asks a
 * network that is not there ends the game RC_ROLLOUT_BAD_POLICY. */
int rc_rollout_step_policy(const rc_rollout_t *r, const void *head, size_t ld, int head_is_bf16, const uint8_t *decisions_row,
                           const double *uniforms_row, uint64_t max_steps, rc_stream_t stream);
/* One move of every running game by ValueSearch._step (agents.py:156-166): the first child whose kid_solved flag is set, which
 * ends the game RC_ROLLOUT_SOLVED (:158-161), else the first maximum of the game's 12 values, a NaN being the maximum (:165);
 * values is float [12 S] in child order.  The child becomes the current state; queue byte, steps and RC_ROLLOUT_EXHAUSTED as
 * above; and the 12 children of the new state with their solved flags are written for the next forward pass. */
int rc_rollout_step_value(const rc_rollout_t *r, const float *values, uint64_t max_steps, rc_stream_t stream);
/* Host only (no GPU needed): the next `steps` draws of n games from their own MT19937 streams, as in rc_egvm_draw (mt_keys,
 * mt_pos, n_games, games, slots; generators are advanced as NumPy leaves them).  Game games[i] gets column slots[i] of a
 * [steps][table_stride] table.  mode 0: bytes, as RandomState.randint(12) draws them (32-bit outputs masked to 4 bits until
 * one is <= 11; agents.py:84).  mode 1: doubles, as RandomState.random_sample draws them (((a >> 5) 2^26 + (b >> 6)) / 2^53):
 * the one number np.random.choice consumes (agents.py:140).  Every slots[i] must be < table_stride. */
int rc_rollout_draw(uint32_t *mt_keys, int32_t *mt_pos, uint32_t n_games, const int32_t *games, const int32_t *slots, uint32_t n,
                    int mode, uint32_t steps, void *table, size_t table_stride);

/* Host only: game games[i] (i < n) gets the generator np.random.RandomState(seeds[games[i]]) starts with -- MT19937's
 * init_genrand of the seed, pos 624 -- which is what np.random.seed(seed) right before the reference's `search` leaves.  seeds is
 * int64 [n_games]; a listed seed outside 0 .. 2^32 - 1 (NumPy raises there) is RC_ERR_RANGE and nothing is written. */
int rc_rollout_seed(uint32_t *mt_keys, int32_t *mt_pos, uint32_t n_games, const int32_t *games, uint32_t n, const int64_t *seeds);

/* ---- breadth-first search (one problem per call sequence, GPU-wide levels) -----------------------
 *
 * Replaces the FIFO loop of librubiks/solving/agents.py:92-131 (class BFS) with level-synchronous
 * chunks that keep its bookkeeping exactly: nodes are numbered in discovery order (node 0 = the
 * start state), child row 12 p + k = action k on the p-th parent of the chunk, a row is new iff its
 * state is neither stored nor produced by a lower row, the first solved row ends the search, and
 * the `len(self) < max_states` test before each pop (agents.py:105) becomes the "cutoff parent".
 * Per chunk:  rc_bfs_expand -> [host reads result[0..4]] -> rc_bfs_commit (if neither solved nor cut).
 * Device pointers; nothing needs initialising except through rc_bfs_init.
 */
typedef struct rc_bfs {
    uint32_t capacity;   /* node slots; rc_bfs_expand needs n_nodes + 12 * n_parents <= capacity */
    uint32_t hash_size;  /* power of two, >= 2 * capacity */
    uint32_t chunk;      /* most parents per rc_bfs_expand */
    uint32_t reserved;
    void *keys;          /* uint32[4] packed state per node (as rc_mcts) */
    uint32_t *parent;    /* agents.py:102,119: the state a node was reached from ... */
    uint8_t *action;     /* ... and the action taken */
    int32_t *hash;       /* [hash_size]: > 0 node index + 1, < 0 pending row -(row+1), 0 empty */
    void *child_keys;    /* uint32[4] per row, [12 * chunk] */
    int32_t *child_slot; /* [12 * chunk] */
    uint32_t *flags;     /* [12 * chunk] 1 = new state */
    uint32_t *prefix;    /* [12 * chunk] exclusive prefix sum of flags */
    uint64_t *result;    /* [5]: first solved row (or ~0), new rows, cutoff parent (n_parents = none),
                            new rows before the solved row, new rows before the cutoff parent */
    void *scan_tmp;      /* rc_bfs_scan_bytes(chunk) bytes */
    size_t scan_tmp_bytes;
} rc_bfs_t;

size_t rc_bfs_scan_bytes(uint32_t chunk);
/* Clears the table and stores root_state (int8[20], device) as node 0.  result[0] = 0 if it is solved
 * (agents.py:100), ~0 otherwise. */
int rc_bfs_init(const rc_bfs_t *b, const int8_t *root_state, rc_stream_t stream);
/* Expands parents lo .. lo + n_parents - 1 with n_nodes states stored so far; fills result. */
int rc_bfs_expand(const rc_bfs_t *b, uint32_t lo, uint32_t n_parents, uint32_t n_nodes, uint32_t max_states,
                  rc_stream_t stream);
/* Appends the new states of the last rc_bfs_expand (same lo, n_parents, n_nodes) in row order. */
int rc_bfs_commit(const rc_bfs_t *b, uint32_t lo, uint32_t n_parents, uint32_t n_nodes, rc_stream_t stream);
/* Actions from the start state to `node`, last action first (agents.py:112-115); *out_len = ~0 if
 * the chain is longer than max_len. */
int rc_bfs_path(const rc_bfs_t *b, uint32_t node, uint8_t *out_actions, uint32_t *out_len, uint32_t max_len,
                rc_stream_t stream);

/* ---- batched breadth-first search: S problems advanced in lock step (csrc/rubiks_bfs_batch.hip) ------
 *
 * Replaces the FIFO loop of librubiks/solving/agents.py:92-129 for S games at once, with the bookkeeping of rc_bfs_* above kept
 * per slot and the decision rc_bfs_* leaves to the host after every chunk (commit, stop, path) made on the device.  A slot owns
 * `capacity` node rows (16-byte packed key, parent, action; node indices are per slot and 32-bit), `hash_size` hash cells and a
 * segment of 12 * chunk child rows: row 12 * chunk * s + 12 p + k = action k on the p-th parent of slot s's chunk.  Rows beyond
 * 12 * n_par of a slot are dead.  Offsets of a slot's arrays inside the batch arrays are size_t.
 * words[w * n_slots + s] is word w of slot s (RC_BFSB_W_*): what the host reads per round are the first RC_BFSB_HOST_WORDS rows.
 * Device pointers; nothing needs initialising except that every status starts RC_BFSB_EMPTY; games enter through
 * rc_bfs_batch_plant.  Launch boundaries are the only synchronisation between workgroups.
 */
#define RC_BFSB_RUNNING 0
#define RC_BFSB_SOLVED 1        /* the first solved row lies before the cut (agents.py:111-116) */
#define RC_BFSB_CUT 2           /* len(self) >= max_states before a pop (agents.py:105) */
#define RC_BFSB_FAILED 3        /* a word or an index read from memory was out of range, or the parent chain is longer than the queue row */
#define RC_BFSB_ROOT_SOLVED 4   /* agents.py:100 */
#define RC_BFSB_GRAPH_DONE 5    /* a whole level brought nothing new (the reference would pop from an empty deque) */
#define RC_BFSB_EMPTY 6         /* no game in the slot */

#define RC_BFSB_W_STATUS 0
#define RC_BFSB_W_NODES 1       /* len(agent) */
#define RC_BFSB_W_LEVELS 2
#define RC_BFSB_W_QUEUE_LEN 3   /* -1 while a solved slot's path is not written yet */
#define RC_BFSB_W_LO 4          /* frontier = nodes lo .. level_end - 1 */
#define RC_BFSB_W_LEVEL_END 5
#define RC_BFSB_W_MAX_STATES 6
#define RC_BFSB_HOST_WORDS 7
#define RC_BFSB_W_N_PAR 7       /* parents of the next chunk (0: the slot does nothing) */
#define RC_BFSB_W_FIRST_SOLVED 8 /* lowest solved local row of the chunk, ~0 = none */
#define RC_BFSB_W_C_ROWS 9      /* the commit the last decision allows: its rows (0 = none), */
#define RC_BFSB_W_C_BASE 10     /*   the node count before it */
#define RC_BFSB_W_C_LO 11       /*   and the first parent of its chunk */
#define RC_BFSB_W_SOLVED_PARENT 12
#define RC_BFSB_W_LAST_ACTION 13
#define RC_BFSB_WORDS 14

typedef struct rc_bfs_batch {
    uint32_t n_slots;     /* S */
    uint32_t chunk;       /* C: most parents of a slot per step; S * 12 * C < 2^31 */
    uint32_t capacity;    /* node rows per slot >= 12 * C + 2: max_states of a slot is at most capacity - 12 * C - 1 */
    uint32_t hash_size;   /* hash cells per slot: power of two, >= 2 * capacity */
    uint32_t queue_width; /* bytes per queue row */
    uint32_t reserved;
    void *keys;           /* [S][capacity] uint32[4] packed state per node (as rc_bfs) */
    uint32_t *parent;     /* [S][capacity] */
    uint8_t *action;      /* [S][capacity] */
    int32_t *hash;        /* [S][hash_size]: > 0 node index + 1, < 0 pending local row -(row+1), 0 empty */
    void *child_keys;     /* [S * 12 * C] uint32[4] */
    int32_t *child_slot;  /* [S * 12 * C] */
    uint32_t *flags;      /* [S * 12 * C] 1 = new state; 0 on dead rows */
    uint32_t *prefix;     /* [S * 12 * C] exclusive prefix sum of flags over the whole row space */
    int64_t *words;       /* [RC_BFSB_WORDS][S] */
    uint8_t *queues;      /* [S][queue_width] actions from the root to the solution */
    void *scan_tmp;       /* rc_bfs_batch_scan_bytes(S, C) bytes */
    size_t scan_tmp_bytes;
} rc_bfs_batch_t;

size_t rc_bfs_batch_struct_bytes(void);
size_t rc_bfs_batch_scan_bytes(uint32_t n_slots, uint32_t chunk);
/* agents.py:92-103 (`search` up to its loop) for the listed slots: slot slots[i] (int32 [n], device; entries < 0 or >= S are
 * skipped) restarts from column first_col + i of roots_soa (20 code planes, as rc_egvm_plant) with max_states[i] (uint32 [n],
 * device; clamped to what the slot's node rows hold).  Clears the slot's hash cells, stores the root as node 0 and resets the
 * slot's words; the solved cube ends at once, RC_BFSB_ROOT_SOLVED with 0 nodes (agents.py:100).  A former tenant's node rows
 * above the new node count are never read.  A slot may be listed once. */
int rc_bfs_batch_plant(const rc_bfs_batch_t *b, const int32_t *slots, uint32_t n, const int8_t *roots_soa, size_t stride,
                       size_t first_col, const uint32_t *max_states, rc_stream_t stream);
/* agents.py:104-129 for the next chunk (at most C parents) of every running slot, without a host read: children and table
 * lookup, claims (the lowest row of a state wins within its slot), flags, one exclusive scan over the row space, the per-slot
 * decision -- solved before the cut (agents.py:111-116: nodes += new rows before it), cut inside the chunk (agents.py:105:
 * nodes += new rows before the cut parent), else commit and advance (at a level's end level_end = nodes, levels += 1; nothing new
 * in a whole level: RC_BFSB_GRAPH_DONE), then the test of agents.py:105 for the next chunk --, the gated commit, and the path of
 * the slots that have just solved (agents.py:112-115), root first, into their queue rows.  Finished and empty slots do nothing. */
int rc_bfs_batch_step(const rc_bfs_batch_t *b, rc_stream_t stream);

/* ---- shortening action queues through the graph of the states they visit (csrc/rubiks_shorten.hip) -------------------
 *
 * The reference shortens the solution of a solved MCTS(search_graph=True) only: _complete_graph (agents.py:597-611) fills the
 * neighbour table of the tree, _shorten_action_queue (agents.py:613-633) runs an ordered breadth-first search from the root to
 * the solved node.  Here the same two procedures run on the graph of a QUEUE, whichever agent made it.  For game g with root
 * s_0 and queue a_0 .. a_{L-1}, s_{i+1} = s_i turned by a_i.  The nodes are the distinct states among s_0 .. s_L: node 1 + p is
 * the state whose first occurrence is at position p (so node 1 is the root and the ids of a game lie in 1 .. L + 1, with gaps
 * where a state returns); 0 is "no node".  nbr[v][a] is the node of state(v) turned by a, or 0 (_complete_graph with every node
 * a leaf).  The target is the node of s_L.  The result is the empty queue if the target is node 1 (agents.py:614), else what the
 * FIFO search of agents.py:616-633 returns: neighbours scanned in action order 0 .. 11, visited nodes skipped, the first scan
 * that meets the target ends the search, actions read back along the discoverers.  It is a shortest route within that graph,
 * never longer than L, ends in s_L, and depends on the game alone.
 *
 * Workspace: game g owns positions pos_off[g] .. pos_off[g + 1] - 1 (at least L + 1 of them) of the per-position arrays and
 * cells hash_off[g] .. hash_off[g + 1] - 1 of `hash`, a power of two >= 2 (L + 1).  Rows of the per-node arrays (nbr, claim) are
 * indexed by position too: node v of game g is row pos_off[g] + v - 1.  All pointers are device pointers.
 * rc_shorten_workspace_bytes(P, H) = r(16 P) + r(4 P) + r(48 P) + r(8 P) + 2 r(4 P) + r(4 H) with r(x) = x rounded up to 256:
 * keys, ids, nbr, claim, the two frontiers and the hash cells, 84 bytes per position and 4 per cell (8 .. 16 more per position).
 *
 * Lengths: parent << 4 | action and the scan index 12 i + a are int32 words, so L + 1 < 2^27: L <= RC_SHORTEN_MAX_LEN.  The host
 * states the longest selected queue in max_len; an entry point returns RC_ERR_RANGE if that exceeds RC_SHORTEN_MAX_LEN or the
 * queue rows, and a game whose lens[g] or offsets do not fit what the struct states ends RC_SHORTEN_FAILED untouched. */
#define RC_SHORTEN_MAX_LEN ((1 << 27) - 2)
#define RC_SHORTEN_OK 0          /* so far every step has run; after rc_shorten_bfs: out_lens[g] holds the result's length */
#define RC_SHORTEN_SKIPPED 1     /* select[g] == 0: the game is left alone */
#define RC_SHORTEN_BAD_ACTION 2  /* a queue byte >= 12 inside the game's length: found before it indexes anything */
#define RC_SHORTEN_FAILED 3      /* a length, an offset, a table word or an index read from memory does not name this game's data */
#define RC_SHORTEN_NO_ROOM 4     /* the result is longer than out_width: out_lens[g] holds its length, no byte of the row is written */

typedef struct rc_shorten {
    uint32_t n_games;         /* G >= 1 */
    uint32_t queue_width;     /* bytes per row of `queues` */
    uint32_t out_width;       /* bytes per row of `out_queues` */
    uint32_t max_len;         /* the host's word: no selected game has lens[g] above it; <= min(queue_width, RC_SHORTEN_MAX_LEN) */
    size_t stride;            /* bytes between the planes of roots_soa: multiple of 16, >= round_up(G, 16) */
    size_t total_positions;   /* P = pos_off[G]: rows of the per-position arrays */
    size_t total_hash_cells;  /* H = hash_off[G] */
    const int8_t *roots_soa;  /* [20][stride] root state of game g in column g */
    const uint8_t *queues;    /* [G][queue_width] */
    const int32_t *lens;      /* [G] L */
    const uint8_t *select;    /* [G] 0: leave the game alone */
    const uint64_t *pos_off;  /* [G + 1] prefix sums made on the host: >= L + 1 positions per selected game */
    const uint64_t *hash_off; /* [G + 1] ... and a power of two >= 2 (L + 1) of cells */
    uint32_t *keys;           /* [P][4] the packed state of every position (20 codes of 5 bits, 6 per word), 16-byte aligned */
    int32_t *ids;             /* [P] node of the position: 1 + the first position of its state */
    int32_t *nbr;             /* [P][12] row v - 1: the neighbours of node v; rows of positions that are no first occurrence are not written */
    int32_t *claim;           /* [P][2] row v - 1: {smallest scan index that reached v (INT_MAX: none), parent << 4 | action (0: not
                                 visited, -1: the root)} */
    int32_t *frontier_a;      /* [P] the two frontiers of the search, swapped level by level */
    int32_t *frontier_b;      /* [P] */
    int32_t *hash;            /* [H] open addressing, linear probing: a cell holds the node of a state, 0 = free; 16-byte aligned */
    uint8_t *out_queues;      /* [G][out_width] the result, root first */
    int32_t *out_lens;        /* [G] its length; -1 where there is none (skipped, bad action, failed) */
    int32_t *status;          /* [G] RC_SHORTEN_* */
} rc_shorten_t;

size_t rc_shorten_struct_bytes(void);
/* Host only: bytes of the workspace arrays of P positions and H hash cells by the formula above (each array starts on a 256-byte
 * boundary); 0 if the sum does not fit size_t. */
size_t rc_shorten_workspace_bytes(size_t total_positions, size_t total_hash_cells);
/* The states of agents.py:597-611's `self.states` / `self.indices` for every selected game: status and out_lens are written for
 * ALL games (SKIPPED / BAD_ACTION / FAILED / OK; -1); then for the games that are OK the queue is replayed from the root (20
 * lanes per game, one cubie each), keys[p] is stored for p = 0 .. L, the hash cells are cleared, every position is inserted with
 * full-key compare -- equal states elect their smallest position, exactly, whatever the order of the inserts -- and ids[p] =
 * the elected node.  Three launches and one memset. */
int rc_shorten_index(const rc_shorten_t *s, rc_stream_t stream);
/* _complete_graph (agents.py:597-611) with every node a leaf: nbr[v][a] for every node v (position p with ids[p] == p + 1) and
 * a = 0 .. 11 by one table probe each, bounded by the table's size.  A cell that does not name a node of the game (outside
 * 1 .. L + 1, or a position that is not its own node) ends the game RC_SHORTEN_FAILED.  Games that are not OK are not touched. */
int rc_shorten_neighbours(const rc_shorten_t *s, rc_stream_t stream);
/* _shorten_action_queue (agents.py:613-633) for every game that is OK, one workgroup each: target = ids[L]; target 1 gives
 * out_lens[g] = 0 (agents.py:614).  Else level-synchronous: every unvisited neighbour of the frontier is claimed by the smallest
 * scan index 12 i + a that reaches it (i: place in the frontier), the winners enter the next frontier in scan-index order, which
 * is the order of the reference's FIFO; the level that claims the target is the last.  The actions are read back along the
 * parents and written root first to out_queues[g], the length to out_lens[g]; a result longer than out_width leaves the row
 * unwritten (RC_SHORTEN_NO_ROOM).  Every neighbour, frontier entry and parent the kernel follows is checked against 1 .. L + 1
 * and a walk back longer than L ends the game RC_SHORTEN_FAILED. */
int rc_shorten_bfs(const rc_shorten_t *s, rc_stream_t stream);
/* rc_shorten_index, rc_shorten_neighbours, rc_shorten_bfs on `stream`. */
int rc_shorten(const rc_shorten_t *s, rc_stream_t stream);

/* ---- the near-solved table: exact distances, optimal tails, tighter queues (csrc/rubiks_near.hip) ---------------------
 *
 * Every state within K quarter turns of the solved cube, found by the breadth-first search of librubiks/solving/agents.py:92-131
 * (class BFS) started at the SOLVED state, with rc_bfs_*'s numbering: nodes in discovery order (node 0 = solved, depth 0), the
 * frontier of a level a contiguous node range, child row 12 p + k = action k on the p-th parent of a chunk, a row new iff its
 * state is neither stored nor produced by a lower row of the chunk, new rows appended in row order.  There is no target and no
 * max_states, and the solved state is stored.  A level is expanded in chunks of at most chunk_rows / 12 parents; the table does
 * not depend on the chunking.  Per node: the packed key (20 codes of 5 bits, 6 per word, as rc_bfs) and one meta byte
 * depth << 4 | action, the action being the k of the row that created the node (0 for the root).  Cells: open addressing, linear
 * probing from key_hash & (hash_size - 1); 0 = free, c > 0 = node c - 1, c < 0 = pending row -(c + 1) while a chunk is filled.
 *
 * With a_1 .. a_d the actions along the discoverers from solved to a state, solved turned by a_1, .., a_d IS the state, d is
 * its exact distance, and rev(a_d), .., rev(a_1) (rev(a) = a ^ 1) is an optimal solution.  States correspond one to one to
 * group elements, so two action sequences with the same product on solved have the same effect on every state: a stretch of a
 * queue whose product lies in the table may be replaced by that product's a_1 .. a_d (tightening), from any root.
 *
 * Node ids and cells are int32 and a depth is 4 bits; K <= RC_NEAR_MAX_DEPTH = 8 (86 049 153 nodes, 2^28 cells: about 2.5 GB).
 * Device pointers throughout; words, and the build arrays, are only needed by rc_near_begin / rc_near_expand. */
#define RC_NEAR_MAX_DEPTH 8
#define RC_NEAR_OK 0
#define RC_NEAR_CORRUPT 1        /* a cell, meta byte or walk back did not name what the build writes: the lane's result is -1 */

typedef struct rc_near {
    uint32_t depth;       /* K, 1 .. RC_NEAR_MAX_DEPTH */
    uint32_t capacity;    /* node rows, < 2^30 */
    uint32_t hash_size;   /* cells: a power of two >= 2 * capacity, <= 2^30 */
    uint32_t n_nodes;     /* nodes a lookup may meet (the host's word after the build; 0 while building) */
    uint32_t chunk_rows;  /* build: rows of the child arrays, >= 12 */
    uint32_t reserved;
    void *keys;           /* [capacity] uint32[4], 16-byte aligned */
    uint8_t *meta;        /* [capacity] depth << 4 | action */
    int32_t *hash;        /* [hash_size] */
    uint32_t *words;      /* build, [4]: nodes stored, 1 = a new state found no node row, new rows of the last chunk, 0 */
    void *child_keys;     /* build, [chunk_rows] uint32[4] */
    int32_t *child_slot;  /* build, [chunk_rows] */
    uint32_t *flags;      /* build, [chunk_rows] 1 = new state */
    uint32_t *prefix;     /* build, [chunk_rows] exclusive prefix sum of flags */
    void *scan_tmp;       /* build, rc_near_scan_bytes(chunk_rows) bytes */
    size_t scan_tmp_bytes;
} rc_near_t;

size_t rc_near_struct_bytes(void);
size_t rc_near_scan_bytes(uint32_t chunk_rows);
/* agents.py:92-103 with the solved state as the root: clears the cells, stores node 0, words = {1, 0, 0}. */
int rc_near_begin(const rc_near_t *t, rc_stream_t stream);
/* agents.py:104-129 for parents lo .. lo + n_parents - 1 (12 n_parents <= chunk_rows) of level `level` - 1: children, lookup
 * against the cells, claims (the lowest row of a state wins), flags, scan, append with meta level << 4 | k, words[0] += new rows.
 * Nothing is read back: the host reads words once a level is done (its count decides whether another level starts).  A new
 * state beyond `capacity` is not stored and sets words[1]. */
int rc_near_expand(const rc_near_t *t, uint32_t lo, uint32_t n_parents, uint32_t level, rc_stream_t stream);
/* One lane per state of soa ([20][stride] code planes, state i in column i): depth_out[i] = its depth, -1 if it is farther
 * than K; node_out (may be NULL) its node or -1.  *status (int32, set to RC_NEAR_OK by the caller) becomes RC_NEAR_CORRUPT if a
 * probe met a cell or meta byte the build does not write; probes are bounded by hash_size. */
int rc_near_depth(const rc_near_t *t, const int8_t *soa, size_t n, size_t stride, int8_t *depth_out, int32_t *node_out, int32_t *status,
                  rc_stream_t stream);
/* One lane per state: out_lens[i] = its depth d or -1, and for d > 0 row i of out_queues ([n][out_width], out_width >= K) holds
 * rev(a_d) .. rev(a_1), found by walking back d times: a = action(node), state <- state turned by rev(a), looked up at depth
 * one less.  A state on the way that is not there at that depth: RC_NEAR_CORRUPT and length -1. */
int rc_near_solve(const rc_near_t *t, const int8_t *soa, size_t n, size_t stride, uint8_t *out_queues, uint32_t out_width, int32_t *out_lens,
                  int32_t *status, rc_stream_t stream);

/* Tightening a batch of action queues (rows, lengths and a select mask as rc_shorten_t; no roots).  For game g with queue q of L
 * moves and W = min(L, window): d(i, j) = depth of solved turned by q[i] .. q[j - 1] for i < j <= min(L, i + W), or none; byte
 * band[band_off[g] + i W + (j - i - 1)] holds it (255 = none).  best[0] = 0, best[j] = min over max(0, j - W) <= i < j with d(i, j)
 * defined of best[i] + d(i, j), a tie going to the smallest i (from[j]); d(j - 1, j) = 1 always.  The chosen i are followed back
 * from L and every chosen segment writes a_1 .. a_d of its product at out_queues[g][best[i] ..]; the length best[L] <= L goes to
 * out_lens[g].  Game g owns positions pos_off[g] .. (at least L + 1) of best / from and at least L W band bytes. */
#define RC_NEAR_T_MAX_LEN ((1 << 27) - 2)
#define RC_NEAR_T_OK 0          /* as RC_SHORTEN_*: so far every step has run */
#define RC_NEAR_T_SKIPPED 1     /* select[g] == 0 */
#define RC_NEAR_T_BAD_ACTION 2  /* a queue byte >= 12 inside the game's length: found before it indexes anything */
#define RC_NEAR_T_FAILED 3      /* a length, offset, cell or word read from memory does not name this game's or the table's data */
#define RC_NEAR_T_NO_ROOM 4     /* best[L] > out_width: out_lens[g] holds it, no byte of the row is written */

typedef struct rc_near_tighten {
    uint32_t n_games;         /* G >= 1 */
    uint32_t queue_width;     /* bytes per row of `queues` */
    uint32_t out_width;       /* bytes per row of `out_queues` */
    uint32_t max_len;         /* the host's word: no selected game has lens[g] above it; <= min(queue_width, RC_NEAR_T_MAX_LEN) */
    uint32_t window;          /* >= 1; the whole queue: any value >= max_len */
    uint32_t reserved;
    size_t total_positions;   /* P = pos_off[G] >= 1 */
    size_t total_band;        /* band_off[G] */
    const uint8_t *queues;    /* [G][queue_width] */
    const int32_t *lens;      /* [G] */
    const uint8_t *select;    /* [G] 0: leave the game alone */
    const uint64_t *band_off; /* [G + 1] prefix sums made on the host */
    const uint64_t *pos_off;  /* [G + 1] */
    uint8_t *band;            /* [total_band] */
    int32_t *best;            /* [P] */
    int32_t *from;            /* [P] the chosen i; ~i once the walk back has chosen the segment */
    uint8_t *out_queues;      /* [G][out_width] */
    int32_t *out_lens;        /* [G] -1 where there is no result */
    int32_t *status;          /* [G] RC_NEAR_T_* */
} rc_near_tighten_t;

size_t rc_near_tighten_struct_bytes(void);
/* status and out_lens of ALL games (one wave per game reads its bytes), then the band of the games that are OK: one lane per
 * start i carries the product move by move and probes the table at every step, two starts per lane in flight. */
int rc_near_tighten_distances(const rc_near_t *t, const rc_near_tighten_t *s, rc_stream_t stream);
/* The dynamic programme above, one wave per OK game reducing over i, then the walk back and the segments' sequences. */
int rc_near_tighten_route(const rc_near_t *t, const rc_near_tighten_t *s, rc_stream_t stream);
/* rc_near_tighten_distances, rc_near_tighten_route on `stream`. */
int rc_near_tighten(const rc_near_t *t, const rc_near_tighten_t *s, rc_stream_t stream);

/* ---- beyond the table: exact distances and optimal solutions up to K + J quarter turns (csrc/rubiks_near_reach.hip) -----------
 *
 * The table is one half of a bidirectional search; this is the other.  For a state s and `extra` = J, levels j = 0, 1, .., J in
 * turn: a sequence q of j actions (all 12^j of them, numbered as base-12 numbers with the first move most significant) is a HIT
 * if s turned by q lies in the table, at depth d <= K.  The first level j* with a hit gives the exact distance D = j* + min d
 * (a hit at level j with depth d means D <= j + d <= j + K, so the first level with a hit is max(0, D - K) and its smallest d is
 * D - j*); no hit up to J: -1, "farther than K + J".  The solution is the hit with the smallest (d, index), followed by the
 * optimal tail of the state it reaches exactly as rc_near_solve writes it; its length is D.
 *
 * Only CANONICAL sequences are walked, which changes no result, the tie included: (1) an action right after its inverse and
 * (2) a third equal quarter turn in a row never occur in a hit at level j* (their product has a sequence two moves shorter,
 * which would have hit two levels earlier); (3) an action on the higher-numbered of two opposite faces directly followed by one
 * on the lower-numbered face has the same product as the two swapped, at a smaller index.
 *
 * Per state: best, a uint64 word that orders by (d, index): d << 40 | level << 36 | index (12^10 < 2^36), all ones = no hit yet;
 * live, a byte that is 0 once the state has its distance from an EARLIER level.  A level is cut into work items: item w of
 * level j is (state w / I, prefix w % I) with I = rc_near_reach_items(j, prefix) = 12^min(j, prefix); the lane of an item drops a
 * prefix that is not canonical, else turns the state by it and walks the remaining j - min(j, prefix) moves depth-first, probing
 * the leaves (the lower levels were hit-free) with two probes in flight, and merges its smallest hit into best by one 64-bit
 * atomic minimum.  The host passes item ranges, so a launch is as long as the host lets it be; the results depend on neither
 * the ranges nor `prefix`.  status: int32[2]; [0] is set to RC_NEAR_OK by the caller and becomes RC_NEAR_CORRUPT as for
 * rc_near_depth (the lane's result is then no hit / -1); [1] is written by every begin / level call: the states that have no
 * distance yet, which the host reads once a level is done to decide whether the next one runs. */
#define RC_NEAR_REACH_MAX_EXTRA 10

typedef struct rc_near_reach {
    size_t n;             /* states, >= 1 */
    size_t stride;        /* of soa */
    uint32_t extra;       /* J, 0 .. RC_NEAR_REACH_MAX_EXTRA */
    uint32_t prefix;      /* P, 0 .. RC_NEAR_REACH_MAX_EXTRA: moves of a sequence that the work-item number holds */
    uint32_t out_width;   /* bytes per row of out_queues, >= K + J */
    uint32_t reserved;
    const int8_t *soa;    /* [20][stride] code planes, state i in column i */
    uint8_t *live;        /* [n] */
    uint64_t *best;       /* [n] */
    int8_t *dist_out;     /* [n] finish: D or -1 */
    int8_t *level_out;    /* [n] finish: j* or -1 */
    uint8_t *out_queues;  /* [n][out_width] finish: the solution */
    int32_t *out_lens;    /* [n] finish: D or -1 */
    int32_t *status;      /* [2] see above */
} rc_near_reach_t;

size_t rc_near_reach_struct_bytes(void);
/* Work items per state of level `level` with `prefix` = P: 12^min(level, P); 0 if either exceeds RC_NEAR_REACH_MAX_EXTRA. */
uint64_t rc_near_reach_items(uint32_t level, uint32_t prefix);
/* Level 0, which is rc_near_depth's probe: best[i] = d << 40 or all ones, live[i] = 1 where there is no hit; status[1]. */
int rc_near_reach_begin(const rc_near_t *t, const rc_near_reach_t *r, rc_stream_t stream);
/* Items first .. first + count - 1 (count >= 1, within n * rc_near_reach_items(level, prefix)) of level 1 <= `level` <= extra.
 * First live[i] = (best[i] is all ones, or a word of this level) for every state, so the levels are to be called in turn and the
 * ranges of one level in any order; then the items; then status[1].  Every loop of an item is bounded by its 12^(level - P)
 * leaves and, within a probe, by the table's size as rc_near_depth's is. */
int rc_near_reach_level(const rc_near_t *t, const rc_near_reach_t *r, uint32_t level, uint64_t first, uint64_t count, rc_stream_t stream);
/* One lane per state: the winning word's index gives the first j* moves, rc_near_solve's walk back from the state they reach gives
 * the rest (rev(a_d) .. rev(a_1)); dist_out, level_out, out_lens and the row are written.  A word that is not one a level writes,
 * or a walk back that leaves the table: RC_NEAR_CORRUPT and -1.  out_width < K + J: RC_ERR_RANGE. */
int rc_near_reach_finish(const rc_near_t *t, const rc_near_reach_t *r, rc_stream_t stream);

/* ---- generalised move patterns in a batch of action sequences (csrc/rubiks_patterns.hip) ------------------------------
 *
 * The reference's find_generalized_patterns (librubiks/analysis/pattern_mining.py:8-45): over every contiguous sub-sequence of
 * length j >= 2 of every sequence, the pattern is the sub-sequence with its faces renamed in order of first appearance, and a
 * pattern is counted once per sequence that holds it.  A symbol is an action 0 .. 11 (face a / 2 with its direction).  Token of
 * position k of a sub-sequence, c its symbol: neither c nor its face seen earlier in the sub-sequence -> the next unused letter
 * (0 = A), upper case; the face seen but not c -> the face's letter, lower case; c itself seen -> the face's letter, upper case
 * (so F f f is A a A, as in the reference).  Token word: 2 letter + (1 if lower case).  The token at k depends on the symbols up
 * to k only, so the patterns form a trie and a pattern's count never exceeds its prefix's.
 *
 * Level-wise: sequence s owns positions pos_off[s] .. pos_off[s + 1] - 1, one LANE per start (s, i) at position pos_off[s] + i.
 * A lane carries lane_state (bits 0-11 the symbols seen, bits 12 + 3 f .. the letter of face f) and lane_node, its pattern's node
 * at the current level, -1 once it is retired.  The node of a pattern of length j is the cell of the key (parent + 1) << 8 |
 * token + 1 in this level's table node_keys (open addressing, linear probing from rc_patterns_hash(key), 0 = free; the parent is
 * the lane's node of level j - 1, and 0 at level 2, where every parent is the pattern A).  Keys are compared whole.  seen_keys
 * holds the keys (node + 1) << 32 | s + 1 in the same way: the lane whose insert creates the key adds 1 to node_count[node].
 * node_first[node] is the smallest s << 32 | i among the node's lanes.  Both tables are cleared at the start of every level and
 * the host states their sizes for the level: powers of two >= 2 x the live lanes, so an insert finds a cell; the probe is
 * bounded by the size all the same and a lane that finds none sets status[s] = RC_PATTERNS_NO_ROOM and retires.  No lane waits
 * for another: a launch boundary completes everything a later step reads.
 *
 * rc_patterns_workspace_bytes(P) with C = rc_patterns_table_cells(P) and r(x) = x rounded up to 256:
 *   3 r(4 P) + r(8 C) + r(4 C) + r(8 C) + r(8 C) + r(16 P) + 256
 * (lane_seq, lane_state, lane_node; node_keys, node_count, node_first, seen_keys; out_rows; counters): 28 B per position and
 * 28 B per cell, 2 .. 4 cells per position, whatever the support. */
#define RC_PATTERNS_OK 0
#define RC_PATTERNS_BAD_ACTION 1 /* a byte >= 12 inside the sequence's length: no lane of the sequence ever runs */
#define RC_PATTERNS_FAILED 2     /* lens[s] or the offsets of s do not fit what the struct states: as above */
#define RC_PATTERNS_NO_ROOM 3    /* a lane of s found no cell in a table smaller than the header asks for */

typedef struct rc_patterns {
    uint32_t n_seqs;          /* n >= 1 */
    uint32_t width;           /* bytes per row of `acts`, >= 1 */
    uint32_t level;           /* j >= 2: the length of the patterns that rc_patterns_extend / rc_patterns_close work on */
    uint32_t min_count;       /* nodes below it are not reported and retire their lanes */
    size_t total_positions;   /* P = pos_off[n] >= 1: rows of the lane arrays */
    size_t node_cells;        /* cells of node_keys, node_count, node_first used at this level: a power of two >= 2 */
    size_t seen_cells;        /* cells of seen_keys used at this level: a power of two >= 2 */
    size_t out_cap;           /* rows of out_rows; a level has at most as many nodes as live lanes, so P is always enough */
    const uint8_t *acts;      /* [n][width] */
    const int32_t *lens;      /* [n] moves of sequence s, 0 .. width */
    const uint64_t *pos_off;  /* [n + 1] prefix sums of lens, made on the host */
    uint32_t *lane_seq;       /* [P] s of the position (written for every position by rc_patterns_begin) */
    uint32_t *lane_state;     /* [P] symbols seen and letters given, see above */
    int32_t *lane_node;       /* [P] node at the current level; -1: retired */
    uint64_t *node_keys;      /* [node_cells] */
    uint32_t *node_count;     /* [node_cells] sequences that hold the node's pattern */
    uint64_t *node_first;     /* [node_cells] smallest s << 32 | i; all ones: free cell */
    uint64_t *seen_keys;      /* [seen_cells] */
    uint32_t *out_rows;       /* [out_cap][4] {count, first s, first i, level} of the nodes with count >= min_count, in any order */
    uint32_t *counters;       /* [4] {live lanes, rows written by this level, rows that found out_rows full, 0} */
    int32_t *status;          /* [n] RC_PATTERNS_* */
} rc_patterns_t;

size_t rc_patterns_struct_bytes(void);
/* Host only.  Cells of a table for `keys` keys: the smallest power of two >= max(2 keys, 2); 0 if keys >= 2^40. */
size_t rc_patterns_table_cells(size_t keys);
/* Host only: the formula above; 0 if P >= 2^40. */
size_t rc_patterns_workspace_bytes(size_t total_positions);
/* Host only: the cell at which the probe of `key` starts is rc_patterns_hash(key) & (cells - 1). */
uint64_t rc_patterns_hash(uint64_t key);
/* Level 1.  status[s] for every sequence (a length outside 0 .. width or offsets that disagree with it: FAILED; else a byte
 * >= 12 inside the length: BAD_ACTION).  Then lane_seq for every position, and for the positions of the sequences that are OK
 * the state after the lane's first symbol and node 0 -- every pattern of length 1 is A, so level 1 has one node and is not
 * counted --, or -1 where the sequence ends before a second symbol; every other position gets -1 and nothing else.
 * counters = {live lanes, 0, 0, 0}. */
int rc_patterns_begin(const rc_patterns_t *p, rc_stream_t stream);
/* Level j = p->level: clears the tables and counters, then every live lane (s, i) reads acts[s][i + j - 1], forms its token,
 * finds or creates its node and the (node, s) key, counts and records the first occurrence as described above. */
int rc_patterns_extend(const rc_patterns_t *p, rc_stream_t stream);
/* After rc_patterns_extend of the same level: appends {count, first s, first i, j} of every node with count >= min_count to
 * out_rows (counters[1] rows; a row beyond out_cap is counted in counters[2] and not written), retires the lanes whose node
 * is below min_count or whose sequence has no symbol i + j, and leaves the number of live lanes in counters[0]. */
int rc_patterns_close(const rc_patterns_t *p, rc_stream_t stream);
/* rc_patterns_extend, rc_patterns_close on `stream`. */
int rc_patterns_level(const rc_patterns_t *p, rc_stream_t stream);

/* ---- the 6x8x6 representation (csrc/rubiks_env686.hip) -------------------------------------------------------------
 * The reference's second representation (librubiks/cube/cube.py:67-71,311-388): a state is int8[6][8][6], the one-hot colour of
 * the 8 non-centre stickers of each face.  Device form: 48 int8 planes of sticker colour 0..5, plane f*8+p = sticker p of face f
 * (so the one-hot index of the network input is (f*8+p)*6 + colour), structure-of-arrays under the rules of the 20 code planes
 * above (*_soa686: soa686[s * stride + i], stride a multiple of 16 and >= round_up(n, 16)).  Every action is one permutation of
 * the 48 stickers; the two representations are isomorphic, so searches keep 20-byte states and cross the bridge only for the
 * network input.
 *
 * Host-side copies of the tables (no GPU needed), both derived at compile time from the 20x24 move table and the sticker layout:
 *   out576[a*48 + s]                 = the sticker that action a moves onto sticker s
 *   out2880[((i*24 + v)*3 + k)*2 ..] = (sticker, colour) pair k of cubie i with code v; sticker 255 = no such pair (edges have 2) */
int rc686_get_perm_table(uint8_t *out576);
int rc686_get_bridge_table(uint8_t *out2880);

/* The reference's (n,6,8,6) int8 one-hot arrays (row-major, 288 bytes per state) <-> sticker planes. */
int rc686_aos_to_soa(const int8_t *oh_aos, int8_t *soa686, size_t n, size_t stride, rc_stream_t stream);
int rc686_soa_to_aos(const int8_t *soa686, int8_t *oh_aos, size_t n, size_t stride, rc_stream_t stream);

/* out[i] = move actions[i] on in[i].  Replaces _Cube686.multi_rotate, a Python loop over the states
 * (librubiks/cube/cube.py:349-361; one state: :330-347).  in and out may alias exactly.  Algorithmic HBM bytes: 97 per state. */
int rc686_multi_rotate(const int8_t *in_soa686, const uint8_t *actions, int8_t *out_soa686, size_t n, size_t stride_in,
                       size_t stride_out, rc_stream_t stream);
/* children[12p + k] = action k on parents[p], as rc_expand12 / rc_expand12_flags (librubiks/solving/agents.py:277-281,513;
 * librubiks/train.py:285-296 with cube.py:349-361 underneath).  Same flag buffers as rc_expand12_flags. */
int rc686_expand12(const int8_t *parents_soa686, int8_t *children_soa686, size_t n_parents, size_t stride_p, size_t stride_c,
                   rc_stream_t stream);
int rc686_expand12_flags(const int8_t *parents_soa686, int8_t *children_soa686, size_t n_parents, size_t stride_p, size_t stride_c,
                         uint8_t *parent_solved, uint8_t *child_solved, rc_stream_t stream);
/* flags[i] = 1 iff every sticker of state i has its face's colour (multi_is_solved, librubiks/cube/cube.py:85-89 against
 * _get_686solved :67-71); flags holds round_up(n, 16) bytes. */
int rc686_is_solved(const int8_t *soa686, uint8_t *flags, size_t n, size_t stride, rc_stream_t stream);
/* (n, 288) one-hot network input, every element written.  Replaces _Cube686.as_oh (librubiks/cube/cube.py:363-369).
 * Algorithmic HBM bytes: 1200 (f32) / 624 (bf16) per state. */
int rc686_as_oh_f32(const int8_t *soa686, float *out, size_t n, size_t stride, rc_stream_t stream);
int rc686_as_oh_bf16(const int8_t *soa686, uint16_t *out, size_t n, size_t stride, rc_stream_t stream);
/* (n, 6, 8) float32: +1 where a sticker has its face's colour, -1 elsewhere.  Replaces _Cube686.as_correct
 * (librubiks/cube/cube.py:372-380, dispatcher :135-137) from the states themselves. */
int rc686_as_correct_f32(const int8_t *soa686, float *out, size_t n, size_t stride, rc_stream_t stream);
/* In place: cube i <- action moves[d * moves_stride + i] for d = 0 .. depth-1 (scramble's rotate loop,
 * librubiks/cube/cube.py:206-211); action 12 is the identity. */
int rc686_apply_moves(int8_t *soa686, const uint8_t *moves, size_t n, size_t stride, size_t moves_stride, size_t depth,
                      rc_stream_t stream);

/* Small calls on the reference's own (n,6,8,6) int8 one-hot layout: one launch each, pointers may be pinned host memory mapped
 * into the device, no alignment requirement (as the *_aos calls of the 20x24 representation).  in and out must differ.
 *   rc686_multi_rotate_aos   librubiks/cube/cube.py:330-361      rc686_is_solved_aos   :85-89      rc686_as_oh_aos_f32   :363-369 */
int rc686_multi_rotate_aos(const int8_t *in_aos, const uint8_t *actions, int8_t *out_aos, size_t n, rc_stream_t stream);
int rc686_is_solved_aos(const int8_t *in_aos, uint8_t *flags, size_t n, rc_stream_t stream);
int rc686_as_oh_aos_f32(const int8_t *in_aos, float *out, size_t n, rc_stream_t stream);

/* The bridge from the 20 code planes (`soa` as everywhere above; a column window of a batch is soa + lo with lo % 16 == 0):
 *   rc_2024_to_686               the 48 sticker planes of the same cubes
 *   rc_as_oh686_from2024_*       _Cube686.as_oh (cube.py:363-369) of the same cubes, (n, 288): the agents' encoder for a network with
 *                                is2024 = false, one launch, no sticker planes in HBM
 *   rc_as_correct_from2024_f32   _Cube686.as_correct (cube.py:372-380) of the same cubes, (n, 6, 8) */
int rc_2024_to_686(const int8_t *soa, int8_t *soa686, size_t n, size_t stride, size_t stride686, rc_stream_t stream);
int rc_as_oh686_from2024_f32(const int8_t *soa, float *out, size_t n, size_t stride, rc_stream_t stream);
int rc_as_oh686_from2024_bf16(const int8_t *soa, uint16_t *out, size_t n, size_t stride, rc_stream_t stream);
int rc_as_correct_from2024_f32(const int8_t *soa, float *out, size_t n, size_t stride, rc_stream_t stream);

/* (n, 288) one-hot network input -> (n, 6, 8) correctness in the same dtype: cube.as_correct as ConvNet.forward calls it on its
 * input (librubiks/model.py:326 -> librubiks/cube/cube.py:135-137,372-380). */
int rc686_as_correct_oh_f32(const float *oh, float *out, size_t n, rc_stream_t stream);
int rc686_as_correct_oh_bf16(const uint16_t *oh, uint16_t *out, size_t n, rc_stream_t stream);

/* The conv branch of ConvNet (reference librubiks/model.py:279-338: `shared_conv_net` built at :290-303, run at :326-329 on
 * cube.as_correct(x), cube.py:372-380) from the 20 code planes, one launch (csrc/rubiks_conv686.hip):
 *     out[i][col0 + c * 8 + p] = act(conv3(pad(act(conv2(pad(conv1(pad(as_correct(state i)))))))))[c][p],   c < 128, p < 8
 * -- kernel-size-3 convolutions, circular over the 8 stickers of a face, channels 6 -> 32 -> 64 -> 128, no activation behind the
 * first (model.py:294-296), flattened (channel, position) as `conv_out.reshape(len(x), -1)` does (:329).  The BatchNorms are the
 * caller's business: folded into the weights (librubiks/model.py `_fold_conv`).  fp32 multiply-adds in a fixed order per output,
 * whatever n, the window (soa + lo, lo % 16 == 0) or the launch: bit-reproducible per state.
 *   weights  31 296 floats, 16-byte aligned: layer l (c_in -> c_out, G = c_out / 16) at offset 0 / 576 / 6 720 as
 *            [c_in][16][3 taps][G]: element ((c * 16 + o / G) * 3 + t) * G + o % G = W_l[o][c][t] of nn.Conv1d's weight
 *   biases   224 floats: b_1 (32), b_2 (64), b_3 (128)
 *   out      row pitch `out_pitch` and first column `col0` in ELEMENTS of the format (both multiples of 8), out 16-byte aligned:
 *            out_format 0: float;  1: bf16;  2: IEEE half [hi | lo] with y = hi + lo 2^-11, a row being out_pitch halves, the hi
 *            block at column col0, the lo block at column out_pitch / 2 + col0.  Columns outside the block are not touched.
 *   range_flag (may be NULL): formats 1 and 2 OR 1 into it when an output is not finite, format 2 also beyond +-65 504.
 * rc_conv686_packed_floats: the sizes of the two packed arrays for conv_channels (c1, c2, c3); RC_ERR_RANGE for any other than
 * the reference's (32, 64, 128) (model.py:21), which is all the kernel is built for. */
int rc_conv686_packed_floats(int c1, int c2, int c3, size_t *n_weights, size_t *n_biases);
int rc_conv686_branch(const int8_t *soa, size_t n, size_t stride, const float *weights, const float *biases, void *out,
                      size_t out_pitch, size_t col0, int out_format, int activation, float alpha, int32_t *range_flag,
                      rc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RUBIKS_HIP_H */
