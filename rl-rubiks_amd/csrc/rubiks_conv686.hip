// The convolutional branch of the reference's ConvNet (librubiks/model.py:279-338: `shared_conv_net`, three kernel-size-3
// convolutions, circular over the 8 stickers of a face, 6 -> 32 -> 64 -> 128 channels) as ONE kernel from the 20 code planes of
// the search states to the (n, 1024) block of activations that `cat_net` reads next to the fully connected trunk's output:
//     out[n][col0 + c * 8 + p] = act(conv3(pad(act(conv2(pad(conv1(pad(as_correct(state)))))))))
// with every BatchNorm already folded into the following layer on the host (librubiks/model.py, `_fold_conv`), so a layer here is
// bias + sum over (c_in, tap) + activation; the first convolution has no activation (reference model.py:294-296).
//
// What was chosen and why
//   * Arithmetic: fp32 fused multiply-adds on the VALU in a fixed order per output: the input channels in blocks of 8, a block
//     summed from zero as the chain
//         fma(w[o][c][2], x[c][p+1], fma(w[o][c][1], x[c][p], fma(w[o][c][0], x[c][p-1], ...)))   for c = 8 k, ..., 8 k + 7
//     and the blocks added in order behind the bias (the first layer, 6 channels, is one chain behind the bias).  One chain over
//     all 192 terms of the last layer is 2.4e-6 from float64 on outputs up to 4 where torch's fp32 evaluation is 1.1e-6 (partial
//     sums of the size of the result are rounded 192 times); in blocks of 24 terms it is 0.9e-6, for one more addition per 24
//     multiply-adds.  An output's order depends on nothing but the state: not on n, not on the window, not on the workgroup or
//     lane that takes it -- F32_SPLIT_DET's promise holds across this kernel.  Both engines (bf16, f16x3 split) and the fp32 chain
//     call it; only the store differs.
//   * Decomposition: a workgroup of 16 waves takes 16 states.  A lane is (state s = lane % 16, position pair q = lane / 16:
//     positions 2q and 2q + 1); a wave owns 1/16 of a layer's output channels (2, 4, 8 of them), so its weights are WAVE-UNIFORM:
//     they are read with scalar loads straight from the packed global array (122 KiB for the three layers: it stays in L2 and in
//     the scalar cache) and enter the multiply-adds as scalar operands, two adjacent output channels per packed instruction.  The
//     122 KiB are therefore NOT staged in LDS -- there they would leave room for a dozen states' intermediates and cost every
//     workgroup a 122 KiB copy; LDS holds only the activations of the 16 states, [channel][position][state] fp32 (48 x 16, 256 x 16,
//     512 x 16 floats: 51 KiB, two workgroups per CU), which a lane reads as 4 values per input channel for 12 G multiply-adds
//     (G = the wave's channels).  Positions are stored even ones first (slot = p / 2 + 4 (p % 2)): the four position pairs of
//     a wave then read 64 consecutive floats whichever neighbour they fetch -- no bank conflicts.
//     Cutting the output channels across the 16 waves of ONE workgroup (not across workgroups) keeps the tail of a search short:
//     352 rows are 22 workgroups whose longest dependent chain is 64 input channels x 24 packed multiply-adds.
//   * The input: the +-1 correctness map is painted into LDS from the code planes through the LDS-resident bridge table (cubie j
//     with code v colours 3 or 2 stickers; every sticker belongs to exactly one cubie) and never reaches HBM.  A window of a batch is
//     a shifted base pointer (lo % 16 == 0), as for the other fused input kernels.
//   * Stores: a lane holds two adjacent positions of a channel, so a store is 8 bytes (float) or 4 bytes (bf16, each half of the
//     split format); the 16 states of a wave's store instruction each receive one 32-byte run.
//   * The f32 matrix-core form (v_mfma_f32_32x32x2_f32 over rows = states x positions: the same peak rate, with the im2col operand
//     of every layer read from LDS in the fragment layout) was NOT built and so not measured against this one;
//     tools/net686_probe.py measures what this form reaches and its share of the engines' forward.
#include "rubiks_netmath.h"
#include "rubiks_tables686.h"

namespace rubiks {

static __constant__ Tables686 c_tables686_conv = kTables686;

constexpr int kCvStates = 16;                    // states per workgroup
constexpr int kCvWaves = 16;                     // waves per workgroup: each owns C_out / 16 output channels of every layer
constexpr int kCvThreads = kCvWaves * kWave;
constexpr int kCvC0 = 6, kCvC1 = 32, kCvC2 = 64, kCvC3 = 128, kCvPos = 8;
constexpr int kCvW1 = 0, kCvW2 = kCvW1 + kCvC0 * 3 * kCvC1, kCvW3 = kCvW2 + kCvC1 * 3 * kCvC2;   // offsets into the packed weights
constexpr int kCvWeights = kCvW3 + kCvC2 * 3 * kCvC3;                                               // 31 296 floats
constexpr int kCvB1 = 0, kCvB2 = kCvC1, kCvB3 = kCvC1 + kCvC2, kCvBiases = kCvC1 + kCvC2 + kCvC3;   // 224 floats
constexpr int kCvBridgeBytes = (int)sizeof(Tables686::bridge);

typedef float cv_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u32 cv_slot(u32 p) { return (p >> 1) + 4u * (p & 1u); }

// One layer for this wave's G output channels (og G .. og G + G - 1) and this lane's (state, position pair).
// x: [CIN][8 slots][16 states] in LDS; w: the layer's packed weights [CIN][16 waves][3 taps][G]; returns acc[G / 2][2 positions],
// each a pair of adjacent output channels.  The input channels are summed in blocks of kCvBlock (see the header of this file).
constexpr int kCvBlock = 8;
template <int CIN, int G>
__device__ __forceinline__ void cv_layer(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias, u32 og,
                                         u32 s, u32 q, cv_f32x2 (&acc)[G / 2][2]) {
    static_assert(G % 2 == 0, "pairs of output channels");
#pragma unroll
    for (int i = 0; i < G / 2; ++i) {
        const cv_f32x2 b = {bias[og * G + 2 * i], bias[og * G + 2 * i + 1]};
        acc[i][0] = b;
        acc[i][1] = b;
    }
    // the lane's four inputs per channel: positions 2q - 1, 2q, 2q + 1, 2q + 2 (mod 8)
    const u32 a0 = (4u + ((q + 3u) & 3u)) * kCvStates + s, a1 = q * kCvStates + s, a2 = (4u + q) * kCvStates + s,
              a3 = ((q + 1u) & 3u) * kCvStates + s;
    const float *wl = w + (size_t)og * (3 * G);
    constexpr bool kBlocked = CIN > kCvBlock;
    static_assert(!kBlocked || CIN % kCvBlock == 0, "whole blocks of input channels");
    constexpr int kStep = kBlocked ? kCvBlock : CIN;
    for (int c0 = 0; c0 < CIN; c0 += kStep) {
        cv_f32x2 part[G / 2][2];
#pragma unroll
        for (int i = 0; i < G / 2; ++i) part[i][0] = part[i][1] = kBlocked ? cv_f32x2{0.f, 0.f} : acc[i][0];
#pragma unroll 4
        for (int cc = 0; cc < kStep; ++cc) {
            const int c = c0 + cc;
            const float *xc = x + c * (kCvPos * kCvStates);
            const float xin[4] = {xc[a0], xc[a1], xc[a2], xc[a3]};
            const float *wc = wl + (size_t)c * (kCvWaves * 3 * G);
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int i = 0; i < G / 2; ++i) {
                    const cv_f32x2 wp = {wc[t * G + 2 * i], wc[t * G + 2 * i + 1]};
                    part[i][0] = __builtin_elementwise_fma(wp, cv_f32x2{xin[t], xin[t]}, part[i][0]);
                    part[i][1] = __builtin_elementwise_fma(wp, cv_f32x2{xin[t + 1], xin[t + 1]}, part[i][1]);
                }
        }
#pragma unroll
        for (int i = 0; i < G / 2; ++i) {
            acc[i][0] = kBlocked ? acc[i][0] + part[i][0] : part[i][0];
            acc[i][1] = kBlocked ? acc[i][1] + part[i][1] : part[i][1];
        }
    }
}

template <int G, int ACT>
__device__ __forceinline__ void cv_keep(float *__restrict__ y, u32 og, u32 s, u32 q, cv_f32x2 (&acc)[G / 2][2], float alpha) {
#pragma unroll
    for (int i = 0; i < G / 2; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const cv_f32x2 v = act_value2<ACT>(acc[i][h], alpha);
            const u32 slot = h ? 4u + q : q;
            y[((og * G + 2 * i) * kCvPos + slot) * kCvStates + s] = v.x;
            y[((og * G + 2 * i + 1) * kCvPos + slot) * kCvStates + s] = v.y;
        }
}

// FMT 0: float out[n][pitch]; 1: bf16; 2: IEEE halves, hi at column col0 + i, lo at column pitch / 2 + col0 + i.
template <int ACT, int FMT>
__global__ __launch_bounds__(kCvThreads) void k_conv686_branch(const u8 *__restrict__ soa, size_t n, size_t stride,
                                                               const float *__restrict__ weights, const float *__restrict__ biases,
                                                               unsigned char *__restrict__ out, size_t pitch, size_t col0, float alpha,
                                                               int *__restrict__ range_flag) {
    __shared__ u32 s_bridge[kCvBridgeBytes / 4];
    __shared__ float s_x0[kCvC0 * kCvPos * kCvStates];
    __shared__ float s_y1[kCvC1 * kCvPos * kCvStates];
    __shared__ float s_y2[kCvC2 * kCvPos * kCvStates];
    const u32 tid = threadIdx.x, lane = tid & 63u;
    const u32 og = __builtin_amdgcn_readfirstlane(tid >> 6);
    const u32 s = lane & 15u, q = lane >> 4;
    const size_t row0 = (size_t)blockIdx.x * kCvStates;
    stage_to_lds(s_bridge, c_tables686_conv.bridge, kCvBridgeBytes);
    __syncthreads();
    if (tid < kCvStates * kPlanes) {   // (state, cubie): paint the cubie's 3 or 2 stickers; rows past the end repeat the last state
        const u32 st = tid & 15u, j = tid >> 4;
        const size_t row = row0 + st < n ? row0 + st : n - 1;
        const u32 code = soa[(size_t)j * stride + row] & 31u;
        const u8 *br = reinterpret_cast<const u8 *>(s_bridge) + ((j * kCodePad + code) * 3) * 2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u32 sticker = br[2 * k], colour = br[2 * k + 1];
            if (sticker < (u32)kStickers)
                s_x0[((sticker >> 3) * kCvPos + cv_slot(sticker & 7u)) * kCvStates + st] = colour == (sticker >> 3) ? 1.0f : -1.0f;
        }
    }
    __syncthreads();
    {
        cv_f32x2 acc[1][2];
        cv_layer<kCvC0, 2>(s_x0, weights + kCvW1, biases + kCvB1, og, s, q, acc);
        cv_keep<2, RC_ACT_NONE>(s_y1, og, s, q, acc, alpha);   // no activation behind the first convolution
    }
    __syncthreads();
    {
        cv_f32x2 acc[2][2];
        cv_layer<kCvC1, 4>(s_y1, weights + kCvW2, biases + kCvB2, og, s, q, acc);
        cv_keep<4, ACT>(s_y2, og, s, q, acc, alpha);
    }
    __syncthreads();
    cv_f32x2 acc[4][2];
    cv_layer<kCvC2, 8>(s_y2, weights + kCvW3, biases + kCvB3, og, s, q, acc);
    const size_t row = row0 + s;
    const bool live = row < n;
    bool bad = false;
    // the lane's outputs: channels og 8 + 2 i (+ 1), positions 2 q and 2 q + 1 -- two adjacent columns per channel
    const size_t esz = FMT == 0 ? 4 : 2;
    unsigned char *orow = out + (row * pitch + col0) * esz;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const cv_f32x2 v0 = act_value2<ACT>(acc[i][0], alpha), v1 = act_value2<ACT>(acc[i][1], alpha);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float ya = e ? v0.y : v0.x, yb = e ? v1.y : v1.x;   // positions 2 q, 2 q + 1 of channel og 8 + 2 i + e
            const size_t col = (size_t)(og * 8 + 2 * i + e) * kCvPos + 2 * q;
            if (FMT == 0) {
                if (live) *reinterpret_cast<float2 *>(orow + col * 4) = make_float2(ya, yb);
            } else if (FMT == 1) {
                bad |= !(fabsf(ya) <= 3.3895314e38f) || !(fabsf(yb) <= 3.3895314e38f);   // bf16's largest finite value: beyond it the store is inf
                if (live) *reinterpret_cast<u32 *>(orow + col * 2) = pack_bf16(ya, yb);
            } else {
                bad |= !(fabsf(ya) <= 65504.0f) || !(fabsf(yb) <= 65504.0f);
                const SplitPair sp = split_pair(ya, yb);
                if (live) {
                    *reinterpret_cast<u32 *>(orow + col * 2) = sp.hi;
                    *reinterpret_cast<u32 *>(orow + (col + pitch / 2) * 2) = sp.lo;
                }
            }
        }
    }
    if (FMT != 0 && range_flag && live && bad) atomicOr(range_flag, 1);
}

}  // namespace rubiks

using namespace rubiks;

extern "C" int rc_conv686_packed_floats(int c1, int c2, int c3, size_t *n_weights, size_t *n_biases) {
    RC_REQUIRE(n_weights != nullptr && n_biases != nullptr, RC_ERR_NULL);
    RC_REQUIRE(c1 == kCvC1 && c2 == kCvC2 && c3 == kCvC3, RC_ERR_RANGE);
    *n_weights = kCvWeights;
    *n_biases = kCvBiases;
    return RC_OK;
}

extern "C" int rc_conv686_branch(const int8_t *soa, size_t n, size_t stride, const float *weights, const float *biases, void *out,
                                 size_t out_pitch, size_t col0, int out_format, int activation, float alpha, int32_t *range_flag,
                                 rc_stream_t stream) {
    RC_REQUIRE(out_format >= 0 && out_format <= 2, RC_ERR_RANGE);
    RC_REQUIRE(activation == RC_ACT_NONE || activation == RC_ACT_RELU || activation == RC_ACT_ELU, RC_ERR_RANGE);
    if (n == 0) return RC_OK;
    RC_CHECK_SOA(soa, n, stride);
    RC_REQUIRE(weights != nullptr && biases != nullptr && out != nullptr, RC_ERR_NULL);
    RC_REQUIRE(aligned16(weights) && aligned16(biases) && aligned16(out), RC_ERR_ALIGN);
    RC_REQUIRE((out_pitch & 7u) == 0 && (col0 & 7u) == 0, RC_ERR_ALIGN);   // aligned 8-byte (float) / 4-byte stores, in the hi and lo blocks alike
    const size_t width = out_format == 2 ? out_pitch / 2 : out_pitch;
    RC_REQUIRE(width >= col0 + (size_t)kCvC3 * kCvPos, RC_ERR_STRIDE);
    RC_REQUIRE(n <= (size_t)0x7fffffff, RC_ERR_RANGE);
    const dim3 grid((unsigned)ceil_div(n, (size_t)kCvStates)), block(kCvThreads);
    hipStream_t s = (hipStream_t)stream;
#define RC_CONV_LAUNCH(ACT, FMT)                                                                                                         \
    hipLaunchKernelGGL((k_conv686_branch<ACT, FMT>), grid, block, 0, s, (const u8 *)soa, n, stride, weights, biases, (unsigned char *)out, \
                       out_pitch, col0, alpha, (int *)range_flag)
#define RC_CONV_FMT(ACT)                       \
    do {                                       \
        if (out_format == 0) RC_CONV_LAUNCH(ACT, 0);      \
        else if (out_format == 1) RC_CONV_LAUNCH(ACT, 1); \
        else RC_CONV_LAUNCH(ACT, 2);           \
    } while (0)
    if (activation == RC_ACT_ELU) RC_CONV_FMT(RC_ACT_ELU);
    else if (activation == RC_ACT_RELU) RC_CONV_FMT(RC_ACT_RELU);
    else RC_CONV_FMT(RC_ACT_NONE);
#undef RC_CONV_FMT
#undef RC_CONV_LAUNCH
    return launch_status();
}
