// K9 - weight / bias gradient of the channel mixing of channels-first tensors (K8, channel_mix.hip: the 1x1 convolution of
// pointwise_op_2D/3D, reference integral_operators.py:210-243, 430-468, and the lift / projection Linear layers of the U-NO models).
//
//   K9  gW[o][i]   = sum_{b,p} gY[b][o][p] * X[b][i][p],  gb[o] = sum_{b,p} gY[b][o][p]      weight / bias gradient
//
// gY, X are (B, C, P) with the pixel axis contiguous - the reduction axis here; as in K8 both operands are staged through LDS with
// unit-stride loads along the pixel axis and consumed as v_mfma_f32_16x16x4_f32 fragments (exact f32).  First stage: partial sums
// per split of the pixels; second stage (channel_wgrad_reduce_kernel): their sum in a fixed order.
#include "channel_mix_common.h"
#include <cstdlib>

namespace uno {

// ------------------------------------------------------------------------------------------------ K9
constexpr int CW_T = 64;            // tile of output channels x tile of input channels per workgroup
constexpr int CW_PK = 32;           // pixels per staged chunk
constexpr int CW_S = CW_PK + 2;     // LDS row stride: 2 r16 + kk hits 32 distinct banks per half-wave

struct ChannelWgradParams {
    const void* gy;         // (B, Co, P) f32 | bf16
    const void* x;          // (B, C1, P) f32 | bf16
    const void* x2;         // (B, Ci - C1, P): input channels [C1, Ci) of a two-source layer (vector kernel only), or nullptr
    int C1;                 // == Ci without a second source
    float* part;            // (nsplit, Co, Ci + 1) partial sums; column Ci holds the bias gradient
    int B, Ci, Co, P, nsplit;
    PixMap pm;              // plane stride + pixel window of gy, x and x2 (vector and split kernels; dense: pm.PS == P)
    const float* vh_x; const float* vh_w; const float* vh_b; int vh_ci;     // vector kernel, VHX: x is VIRTUAL (see ChannelMixParams)
    int act_x;              // scalar kernel: x := gelu(x)
    long long span;         // pixels per split (informational)
    int rev;                // alternating sweep direction (vector and split kernels): pixel splits in descending order
    // split kernel, template PB (round 6): gy is the PRE-ACTIVATION of the layer and the gradient at its output is never stored -
    // gy[b][o][q] stands for pb_w2[o] gelu'(gy[b][o][q]) pb_g[b][q] (see ChannelMixParams::pb_w2); the kernel also leaves the partial sums
    // of the projection's own gradients in part2 (nsplit, Co + 1): sum_q gelu(gy[b][o][q]) pb_g[b][q] per channel, sum_q pb_g[b][q] in slot Co
    const float* pb_w2; const float* pb_g; float* part2;
};

template <bool BF>
__global__ __launch_bounds__(256) void channel_wgrad_kernel(ChannelWgradParams p, int npc, int chunks_per_split) {
    using T = typename IoElem<BF>::type;
    __shared__ float sG[2][CW_T * CW_S];
    __shared__ float sXc[2][CW_T * CW_S];
    const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, kk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntile_i = (p.Ci + CW_T - 1) / CW_T;
    const int o0 = (blockIdx.x / ntile_i) * CW_T, i0 = (blockIdx.x % ntile_i) * CW_T;
    const int split = blockIdx.y;
    const int c_begin = split * chunks_per_split, c_end = min(c_begin + chunks_per_split, p.B * npc);

    // staging: each operand chunk = 64 rows x 32 px of one batch entry -> 8 elements per thread (row e / 32, px e % 32)
    float rg[8], rxv[8];
    auto load_chunk = [&](int idx) {
        const int b = idx / npc, pp0 = (idx - b * npc) * CW_PK;
        const T* gb = reinterpret_cast<const T*>(p.gy) + (size_t)b * p.Co * p.P;
        const T* xb = reinterpret_cast<const T*>(p.x) + (size_t)b * p.Ci * p.P;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + 256 * u;
            const int row = e >> 5, px = pp0 + (e & 31);
            rg[u] = (px < p.P && o0 + row < p.Co) ? io_widen(gb[(size_t)(o0 + row) * p.P + px]) : 0.f;
            rxv[u] = (px < p.P && i0 + row < p.Ci) ? io_widen(xb[(size_t)(i0 + row) * p.P + px]) : 0.f;
            if (p.act_x) rxv[u] = cm_gelu(rxv[u]);
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + 256 * u;
            sG[buf][(e >> 5) * CW_S + (e & 31)] = rg[u];
            sXc[buf][(e >> 5) * CW_S + (e & 31)] = rxv[u];
        }
    };

    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0, 0, 0, 0};
    float bsum = 0.f;                                   // bias gradient: threads 0..63 own one output channel each (i-tile 0 only)

    if (c_begin < c_end) { load_chunk(c_begin); store_chunk(0); }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const int buf = (c - c_begin) & 1;
        const bool more = c + 1 < c_end;
        if (more) load_chunk(c + 1);
#pragma unroll
        for (int ks = 0; ks < CW_PK / 4; ++ks) {
            const float a = sG[buf][(16 * wave + r16) * CW_S + 4 * ks + kk];          // A[o][k = px]
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                acc[nt] = mfma16(a, sXc[buf][(16 * nt + r16) * CW_S + 4 * ks + kk], acc[nt]);   // B[k = px][i]
        }
        if (i0 == 0 && tid < CW_T) {
            const float* g = sG[buf] + tid * CW_S;
#pragma unroll
            for (int k = 0; k < CW_PK; ++k) bsum += g[k];
        }
        if (more) store_chunk(buf ^ 1);
        __syncthreads();
    }

    // D[o = 16 wave + 4 kk + r][i = 16 nt + r16]
    float* part = p.part + (size_t)split * p.Co * (p.Ci + 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = o0 + 16 * wave + 4 * kk + r;
        if (o < p.Co) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int i = i0 + 16 * nt + r16;
                if (i < p.Ci) part[(size_t)o * (p.Ci + 1) + i] = acc[nt][r];
            }
        }
    }
    if (i0 == 0 && tid < CW_T && o0 + tid < p.Co) part[(size_t)(o0 + tid) * (p.Ci + 1) + p.Ci] = bsum;
}

// Vector variant (P >= 64): 64-pixel chunks enumerated per batch entry, 16-byte loads, next chunk in registers
// (32 dwords per thread in flight), bias partial sums taken from the registers on their way to LDS.
constexpr int CWV_PK = 64;
constexpr int CWV_S = CWV_PK + 4;       // 272-byte rows: 16-byte aligned for ds_write_b128; fragment reads hit banks 4 r16 + kk,
                                        // distinct over all 64 lanes (gfx950 LDS: 64 banks; a stride of 66 cost one conflict cycle per read)

// NI: 16-channel tiles of the INPUT side per workgroup, 4 or - layers with at most 32 input channels (the lift's fc0: 32 -> 64 at full
// resolution) - 2: the 64-wide tile spent half of its MFMAs, X loads, GELUs and LDS writes on channels that do not exist.
template <bool ACTX, bool BF, int NI = 4, bool VHX = false>          // ACTX: x := gelu(x) on its way to LDS (the layer's input is kept pre-activation)
__global__ __launch_bounds__(256, 4) void channel_wgrad_vec_kernel(ChannelWgradParams p, int npc, int chunks_per_split) {
    using T = typename IoElem<BF>::type;
    constexpr int ES = BF ? 2 : 4;          // bytes per element
    __shared__ __attribute__((aligned(16))) float sG[CW_T * CWV_S];
    __shared__ __attribute__((aligned(16))) float sXc[CW_T * CWV_S];
    __shared__ float4 sVH[VHX ? 64 : 1];
    if constexpr (VHX) {
        if ((int)threadIdx.x < p.Ci) {
            const float* wr = p.vh_w + threadIdx.x * p.vh_ci;
            sVH[threadIdx.x] = make_float4(wr[0], p.vh_ci > 1 ? wr[1] : 0.f, p.vh_ci > 2 ? wr[2] : 0.f, p.vh_b ? p.vh_b[threadIdx.x] : 0.f);
        }
        __syncthreads();
    }
    const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, kk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntile_i = (p.Ci + CW_T - 1) / CW_T;
    const int ntile = ((p.Co + CW_T - 1) / CW_T) * ntile_i;
    // XCD-aware order: workgroups go round-robin to the 8 XCDs; all weight tiles of one pixel split (they read the same
    // gy / x rows) are given to one XCD so that the re-reads hit its L2 (measured before: 1.78x the algorithmic bytes
    // fetched over the fabric for a 2-tile layer)
    const int bxr = sweep_x(p.rev);
    const int xcd = bxr & 7, j = bxr >> 3;
    const int split = (j / ntile) * 8 + xcd, tile = j % ntile;
    if (split >= p.nsplit) return;
    const int o0 = (tile / ntile_i) * CW_T, i0 = (tile % ntile_i) * CW_T;
    const int c_begin = split * chunks_per_split, c_end = min(c_begin + chunks_per_split, p.B * npc);

    // The loads deliver raw 16-byte pieces from clamped addresses; the zero-fill past the row end (shift network) and past
    // the channel count is applied when the chunk goes to LDS, AFTER the MFMA block - applied at load time it consumed the
    // loaded registers at once and the wave waited for its loads (s_waitcnt vmcnt(0)) before every MFMA block.
    float4 rg[4], rxv[4];
    float4 rvx[3];          // VHX: the raw pieces of the real channels at this thread's four pixels
    int sh_cur = 0;
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
    const int c4 = (tid & 15) * 4, row0 = tid >> 4;
    // buffer loads (uniform base in SGPRs + 32-bit lane offset): the intrinsic is a fixed 128-bit access - as plain loads
    // of a 4-byte-aligned struct the compiler split these into pairs of 8-byte loads once the registers had to stay
    // live across the MFMA block, doubling the vector-memory instructions
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    // the 64 input channels of this tile lie in one source (C1 % 64 == 0 in two-source calls): xs = its tensor, Cs its channel
    // count, il the tile's first channel inside it; the GELU-on-read form applies to the first source only
    const bool src2 = i0 >= p.C1;
    const T* xs = reinterpret_cast<const T*>(src2 ? p.x2 : p.x);
    const int Cs = src2 ? p.Ci - p.C1 : p.C1, il = src2 ? i0 - p.C1 : i0;
    const bool actx = ACTX && !src2;
    auto load_chunk = [&](int idx) {
        const int b = idx / npc, pp = (idx - b * npc) * CWV_PK;
        const int PS = p.pm.PS;
        const __amdgpu_buffer_rsrc_t rg_ = __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const T*>(p.gy) + (size_t)b * p.Co * PS), 0, p.Co * PS * ES, 0x00020000);
        const __amdgpu_buffer_rsrc_t rx_ = __builtin_amdgcn_make_buffer_rsrc((void*)(xs + (size_t)b * Cs * PS), 0, Cs * PS * ES, 0x00020000);
        const int px = pp + c4, pl = min(px, p.P - 4);
        sh_cur = px - pl;
        const int pc = pix_run(p.pm, pp)(pl);            // offset of the piece inside its channel plane
        if constexpr (VHX) {
            const __amdgpu_buffer_rsrc_t rv_ = __builtin_amdgcn_make_buffer_rsrc((void*)(p.vh_x + (size_t)b * p.vh_ci * p.P), 0, p.vh_ci * p.P * 4, 0x00020000);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rv_, (min(kx, p.vh_ci - 1) * p.P + pl) * 4, 0, 0);
                rvx[kx] = make_float4(__uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z), __uint_as_float(t.w));
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = row0 + 16 * u;
            if constexpr (BF) {
                typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                const u32x2 tg = __builtin_amdgcn_raw_buffer_load_b64(rg_, (min(o0 + row, p.Co - 1) * PS + pc) * 2, 0, 0);
                rg[u] = make_float4(__uint_as_float(tg.x << 16), __uint_as_float(tg.x & 0xffff0000u), __uint_as_float(tg.y << 16), __uint_as_float(tg.y & 0xffff0000u));
                if (u < NI) {
                    const u32x2 tx = __builtin_amdgcn_raw_buffer_load_b64(rx_, (min(il + row, Cs - 1) * PS + pc) * 2, 0, 0);
                    rxv[u] = make_float4(__uint_as_float(tx.x << 16), __uint_as_float(tx.x & 0xffff0000u), __uint_as_float(tx.y << 16), __uint_as_float(tx.y & 0xffff0000u));
                }
            } else {
                const u32x4 tg = __builtin_amdgcn_raw_buffer_load_b128(rg_, (min(o0 + row, p.Co - 1) * PS + pc) * 4, 0, 0);
                rg[u] = make_float4(__uint_as_float(tg.x), __uint_as_float(tg.y), __uint_as_float(tg.z), __uint_as_float(tg.w));
                if (u < NI && !VHX) {
                    const u32x4 tx = __builtin_amdgcn_raw_buffer_load_b128(rx_, (min(il + row, Cs - 1) * PS + pc) * 4, 0, 0);
                    rxv[u] = make_float4(__uint_as_float(tx.x), __uint_as_float(tx.y), __uint_as_float(tx.z), __uint_as_float(tx.w));
                }
            }
        }
    };
    auto shifted = [&](const float4& v, bool valid) {
        float t0 = v.x, t1 = v.y, t2 = v.z, t3 = v.w;
        if (sh_cur & 1) { t0 = t1; t1 = t2; t2 = t3; t3 = 0.f; }
        if (sh_cur & 2) { t0 = t2; t1 = t3; t2 = 0.f; t3 = 0.f; }
        if (sh_cur >= 4 || !valid) { t0 = 0.f; t1 = 0.f; t2 = 0.f; t3 = 0.f; }
        return make_float4(t0, t1, t2, t3);
    };
    auto store_chunk = [&]() {
        float4 q[3];
        if constexpr (VHX) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) { q[kx] = shifted(rvx[kx], kx < p.vh_ci); }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = row0 + 16 * u;
            const float4 g = shifted(rg[u], o0 + row < p.Co);
            *reinterpret_cast<float4*>(sG + row * CWV_S + c4) = g;
            bs[u] += (g.x + g.y) + (g.z + g.w);
            if (u < NI) {
                float4 v;
                if constexpr (VHX) {
                    // (pixels past the row end carry the bias instead of zero: they meet the zero fill of gy)
                    const float4 t = sVH[min(il + row, p.Ci - 1)];
                    v = make_float4(fmaf(t.z, q[2].x, fmaf(t.y, q[1].x, fmaf(t.x, q[0].x, t.w))), fmaf(t.z, q[2].y, fmaf(t.y, q[1].y, fmaf(t.x, q[0].y, t.w))),
                                    fmaf(t.z, q[2].z, fmaf(t.y, q[1].z, fmaf(t.x, q[0].z, t.w))), fmaf(t.z, q[2].w, fmaf(t.y, q[1].w, fmaf(t.x, q[0].w, t.w))));
                    if (il + row >= Cs) v = make_float4(0.f, 0.f, 0.f, 0.f);
                } else v = shifted(rxv[u], il + row < Cs);
                if constexpr (ACTX) { if (actx) v = cm_gelu4(v); }             // gelu(0) = 0: the zero fill survives
                *reinterpret_cast<float4*>(sXc + row * CWV_S + c4) = v;
            }
        }
    };

    f32x4 acc[NI];
#pragma unroll
    for (int nt = 0; nt < NI; ++nt) acc[nt] = f32x4{0, 0, 0, 0};

    if (c_begin < c_end) load_chunk(c_begin);
    for (int c = c_begin; c < c_end; ++c) {
        store_chunk();
        __syncthreads();
        load_chunk(min(c + 1, c_end - 1));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < CWV_PK / 4; ++ks) {
            const float a = sG[(16 * wave + r16) * CWV_S + 4 * ks + kk];
#pragma unroll
            for (int nt = 0; nt < NI; ++nt)
                acc[nt] = mfma16(a, sXc[(16 * nt + r16) * CWV_S + 4 * ks + kk], acc[nt]);
        }
        __syncthreads();
    }

    float* part = p.part + (size_t)split * p.Co * (p.Ci + 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = o0 + 16 * wave + 4 * kk + r;
        if (o < p.Co) {
#pragma unroll
            for (int nt = 0; nt < NI; ++nt) {
                const int i = i0 + 16 * nt + r16;
                if (i < p.Ci) part[(size_t)o * (p.Ci + 1) + i] = acc[nt][r];
            }
        }
    }
    if (i0 == 0) {          // bias gradient: the 16 threads that share a row hold its partial sums
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float v = bs[u];
            v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
            const int o = o0 + row0 + 16 * u;
            if ((tid & 15) == 0 && o < p.Co) part[(size_t)o * (p.Ci + 1) + p.Ci] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ K9-S
// The weight gradient of the wide layers (both channel counts >= 96) on the bf16 matrix pipe with both operands split into three
// bfloat16 pieces - the arrangement of K8-S (six products, f32 accumulation, ~1e-7 relative: profiles/r04_split_bf16_error.txt).
// Why: gW = sum over 16 x P pixels of gY X^T has Co x Ci outputs for 4 (Co + Ci) bytes per pixel - 2 Co Ci / (4 (Co + Ci)) flop/B =
// 64 at 256 x 256, 43 at 128 x 256, 21 at 64 x 128 (fc1, + its GELU on read) - against the f32 ridge of 20: the vector kernel above ran
// these layers at 1.5-3.6 TB/s, i.e. at the f32 MFMA peak (256 x 256 at 111^2: 25.8 GFLOP, 258 us; fc1 at 446^2: 52 GFLOP + 204 M
// GELUs, 673 us for 2.44 GB).
//   * workgroup = (32 MR) x 128 weight tile x one split of the pixels, MR = 4 (Co >= 96) or 2 (Co <= 64 .. 95: fc1 128 -> 64, conv5's
//     256 -> 64); wave (a, b) owns output channels 16 MR a .. x input channels 64 b .. + 63 = MR x 4 accumulator tiles; K = pixels,
//     staged 32 at a time;
//   * BOTH operands have their k axis (pixels) contiguous in memory, so the MFMA operand of a lane - 8 consecutive k of one row - is
//     16 contiguous bytes of an LDS row: planes [piece][row: 128 gY + 128 X][32 px] of bf16, rows 80 bytes apart (the 16 rows of a
//     fragment read cover the 64 banks once), one ds_read_b128 per fragment and piece, no transposing reads;
//   * the split happens once per element, in the thread that stages it (as K8-S); the next 32 pixels are in flight in registers
//     while the current ones are multiplied; 60 KB of LDS, two workgroups per CU.
// Partial sums leave in the (split, Co, Ci + 1) layout of the other first-stage kernels; the second stage is shared.
constexpr int CWS_T = 128;
constexpr int CWS_PK = 32;
constexpr int CWS_RS = CWS_PK * 2 + 16;             // bytes per row of a plane
constexpr int CWS_PLANE = 2 * CWS_T * CWS_RS;       // 20 480

// From 100 000 pixels per launch: below, a launch is a handful of 128 x 128 tiles with a few chunks each and the 60 KB workgroups lose to
// the vector kernel (A/B on one box: the NS-2D roll-out - 64^2 .. 16^2 grids at batch 32, at most 74 000 pixels per call - 80.7 ms
// per step with this form on its wide layers, 79.5 without; the Darcy model's smallest level is 197 000).
static bool wgrad_split_shape(int B, int Ci, int Co, long long P) {
#ifdef UNO_CMS_DEV
    static const bool off = getenv("UNO_CW_SPLIT_OFF") != nullptr;         // development build only: A/B against the f32-MFMA form
#else
    constexpr bool off = false;
#endif
    return !off && Ci >= 96 && Co >= 48 && P >= 64 && (long long)B * P >= 100000;
}
static int wgrad_split_rows(int Co) { return Co >= 96 ? CWS_T : 64; }      // output channels per weight tile

// BF: bfloat16 activations (exact in ONE piece: gY x X is one product; with the GELU applied on read, gelu(x) is an f32 value again: three
// pieces of X against the one of gY)
// PB: the gy operand is the projected-back gradient of ChannelWgradParams::pb_* - gelu' (and gelu, for the projection's weight gradient)
// where the staged quad is split, pb_g as a fifth staged row, pb_w2 on the finished sums.
template <bool ACTX, int MR, bool BF, bool PB = false>
__global__ __launch_bounds__(256, 2) void channel_wgrad_split_kernel(ChannelWgradParams p, int npc, int chunks_per_split) {
    static_assert(!(PB && BF), "the projected-back operand is float32");
    __shared__ __attribute__((aligned(16))) char smem[3 * CWS_PLANE];
    const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, kk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wa = wave & 1, wb = wave >> 1;
    const int ntile_i = (p.Ci + CWS_T - 1) / CWS_T;
    constexpr int TO = 32 * MR;                                     // output channels per tile
    using T = typename IoElem<BF>::type;
    constexpr int ES = BF ? 2 : 4;
    constexpr int NPG = BF ? 1 : 3, NPX = (BF && !ACTX) ? 1 : 3;    // bf16 pieces of the two operands
    const int ntile = ((p.Co + TO - 1) / TO) * ntile_i;
    const int bxr = sweep_x(p.rev);
    const int xcd = bxr & 7, j = bxr >> 3;                          // all weight tiles of one pixel split on one XCD (as the vector kernel)
    const int split = (j / ntile) * 8 + xcd, tile = j % ntile;
    if (split >= p.nsplit) return;
    const int o0 = (tile / ntile_i) * TO, i0 = (tile % ntile_i) * CWS_T;
    const int c_begin = split * chunks_per_split, c_end = min(c_begin + chunks_per_split, p.B * npc);

    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const int c4 = (tid & 7) * 4, row0 = tid >> 3;                  // a thread stages four pixels of rows row0 + 32 u of both operands
    // the 32 input channels of band u lie in one source (C1 % 32 == 0 in two-source calls)
    const T* xsrc[4];
    int xcs[4], xrow[4];
    bool xact[4], xok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int ci = i0 + 32 * u;
        const bool s2 = ci >= p.C1;
        xsrc[u] = reinterpret_cast<const T*>(s2 ? p.x2 : p.x);
        xcs[u] = s2 ? p.Ci - p.C1 : p.C1;
        const int il = (s2 ? ci - p.C1 : ci) + row0;
        xok[u] = ci + row0 < p.Ci;
        xrow[u] = min(il, xcs[u] - 1);
        xact[u] = ACTX && !s2;
        if (ci >= p.Ci) { xsrc[u] = reinterpret_cast<const T*>(p.x); xcs[u] = p.C1; xrow[u] = 0; }
    }
    // two half chunks in flight (register sets 0 / 1): with one, the loads had the 96 MFMAs of ONE half (~0.8 us) to arrive in and the
    // wave waited for them at every store (256 x 256 at 111^2: 173 us at 45 % MFMA-pipe use)
    u32x4 rqs[2] = {u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}};  // PB: the four pixels' pb_g
    float bs2[4] = {0.f, 0.f, 0.f, 0.f}, qs = 0.f;                  // PB: sums of gelu(pre) pb_g per staged row, of pb_g
    u32x4 rgs[2][4], rxs[2][4];                                     // RAW loaded pieces: anything computed from them at load time makes the wave wait for its loads at once
    int shs[2] = {0, 0};
    // the zero fill past the row end / past the channel counts is needed only in the last half chunk of a row and in partial weight
    // tiles - both wave-uniform; everywhere else the staged values go straight to the split (12 of 34 VALU instructions per four values)
    bool tails[2] = {false, false};
    const bool edge = o0 + TO > p.Co || i0 + CWS_T > p.Ci;
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
    auto load_half = [&](int it, u32x4 (&rg)[4], u32x4 (&rxv)[4], u32x4& rq, int& sh_cur, bool& tail) {     // half chunk it: 32 pixels of chunk it >> 1
        const int idx = it >> 1;
        const int b = idx / npc, pp = (idx - b * npc) * CWV_PK + (it & 1) * CWS_PK;
        const int PS = p.pm.PS;
        const __amdgpu_buffer_rsrc_t rg_ = __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const T*>(p.gy) + (size_t)b * p.Co * PS), 0, p.Co * PS * ES, 0x00020000);
        typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
        auto raw2 = [](const u32x2& t) { return u32x4{t.x, t.y, 0u, 0u}; };
        const int px = pp + c4, pl = min(px, p.P - 4);
        sh_cur = px - pl;
        tail = pp + CWS_PK > p.P;
        const int pc = pix_run(p.pm, pp)(pl);            // offset of the piece inside its channel plane
        if constexpr (PB) {
            const __amdgpu_buffer_rsrc_t rq_ = __builtin_amdgcn_make_buffer_rsrc((void*)(p.pb_g + (size_t)b * PS), 0, PS * 4, 0x00020000);
            rq = __builtin_amdgcn_raw_buffer_load_b128(rq_, pc * 4, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const __amdgpu_buffer_rsrc_t rx_ = __builtin_amdgcn_make_buffer_rsrc((void*)(xsrc[u] + (size_t)b * xcs[u] * PS), 0, xcs[u] * PS * ES, 0x00020000);
            if constexpr (BF) {
                if (u < MR) rg[u] = raw2(__builtin_amdgcn_raw_buffer_load_b64(rg_, (min(o0 + row0 + 32 * u, p.Co - 1) * PS + pc) * 2, 0, 0));
                rxv[u] = raw2(__builtin_amdgcn_raw_buffer_load_b64(rx_, (xrow[u] * PS + pc) * 2, 0, 0));
            } else {
                if (u < MR) rg[u] = __builtin_amdgcn_raw_buffer_load_b128(rg_, (min(o0 + row0 + 32 * u, p.Co - 1) * PS + pc) * 4, 0, 0);
                rxv[u] = __builtin_amdgcn_raw_buffer_load_b128(rx_, (xrow[u] * PS + pc) * 4, 0, 0);
            }
        }
    };
    auto shifted = [&](const u32x4& r, bool valid, int sh_cur, bool slow) {    // slow: zero fill past the row end / past the channel count (see the vector kernel)
        float t0, t1, t2, t3;
        if constexpr (BF) { t0 = __uint_as_float(r.x << 16); t1 = __uint_as_float(r.x & 0xffff0000u); t2 = __uint_as_float(r.y << 16); t3 = __uint_as_float(r.y & 0xffff0000u); }
        else { t0 = __uint_as_float(r.x); t1 = __uint_as_float(r.y); t2 = __uint_as_float(r.z); t3 = __uint_as_float(r.w); }
        if (slow) {
            if (sh_cur & 1) { t0 = t1; t1 = t2; t2 = t3; t3 = 0.f; }
            if (sh_cur & 2) { t0 = t2; t1 = t3; t2 = 0.f; t3 = 0.f; }
            if (sh_cur >= 4 || !valid) { t0 = 0.f; t1 = 0.f; t2 = 0.f; t3 = 0.f; }
        }
        return make_float4(t0, t1, t2, t3);
    };
    auto put1 = [&](char* d, const float4& v) {                    // widened bf16 values: exact in one piece
        *reinterpret_cast<uint2*>(d) = make_uint2(bf16_pack2(v.x, v.y), bf16_pack2(v.z, v.w));
    };
    auto put3 = [&](char* d, const float4& v) {
        unsigned h0, m0, l0, h1, m1, l1;
        cms_split3(v.x, v.y, h0, m0, l0);
        cms_split3(v.z, v.w, h1, m1, l1);
        *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(d + CWS_PLANE) = make_uint2(m0, m1);
        *reinterpret_cast<uint2*>(d + 2 * CWS_PLANE) = make_uint2(l0, l1);
    };
    // Position of a row's four 16-byte k-groups inside its 64 bytes: rows 4 .. 11 of every 16 keep them pairwise swapped.  ds_read_b128 is
    // serviced in lane groups {0-3, 12-15, 20-27}, ... - rows 0-3 / 12-15 at k-group g together with rows 4-11 at k-group g ^ 1 - and with
    // 80-byte rows in plain order three of the 16 accesses of every group met another one's banks (PMC, 256 x 256 at 111^2:
    // SQ_LDS_BANK_CONFLICT 19.0 M of 38.0 M LDS cycles); with the swap the 16 four-bank windows of a group are distinct.
    const int wpos = 16 * ((c4 >> 2 >> 1) ^ (((row0 & 15) + 4) >> 3 & 1)) + 8 * ((c4 >> 2) & 1);       // rows row0 + 32 u: the same row0 & 15
    auto store_half = [&](const u32x4 (&rg)[4], const u32x4 (&rxv)[4], const u32x4& rq, int sh_cur, bool slow) {
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (PB) { q = shifted(rq, true, sh_cur, slow); qs += (q.x + q.y) + (q.z + q.w); }      // (zero past the row end: the products below vanish there)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = row0 + 32 * u;
            if (u < MR) {
                float4 g = shifted(rg[u], o0 + row < p.Co, sh_cur, slow);
                if constexpr (PB) {
                    // (the four products are summed like the bias gradient's below, not fma-chained into bs2[u]: the chained form was packed by
                    // the SLP vectoriser into v_pk_fma_f32 on the (bs2[0], bs2[1]) pair and - in the ACTX = false, MR = 2 instantiation only -
                    // lanes 48-63 of a wave lost one half chunk's terms of bs2[0] in about every fourth launch; -fno-slp-vectorize and this
                    // form are both clean over hundreds of launches: tests/test_hip_project_backward.py repeats the launch)
                    auto back = [&](float v, float qv, float& t) {
                        const float cdf = 0.5f * (1.f + uno_erf(v * 0.70710678118654752440f));
                        const float pdf = 0.39894228040143267794f * __expf(-0.5f * v * v);
                        t = v * cdf * qv;
                        return fmaf(v, pdf, cdf) * qv;
                    };
                    float t0, t1, t2, t3;
                    g = make_float4(back(g.x, q.x, t0), back(g.y, q.y, t1), back(g.z, q.z, t2), back(g.w, q.w, t3));
                    bs2[u] += (t0 + t1) + (t2 + t3);
                }
                if constexpr (NPG == 1) put1(smem + row * CWS_RS + wpos, g); else put3(smem + row * CWS_RS + wpos, g);
                bs[u] += (g.x + g.y) + (g.z + g.w);
            }
            float4 v = shifted(rxv[u], xok[u], sh_cur, slow);
            if constexpr (ACTX) { if (xact[u]) v = cm_gelu4(v); }   // gelu(0) = 0: the zero fill survives
            if constexpr (NPX == 1) put1(smem + (CWS_T + row) * CWS_RS + wpos, v); else put3(smem + (CWS_T + row) * CWS_RS + wpos, v);
        }
    };

    f32x4 acc[MR][4];                   // [output-channel tile m][input-channel tile t]
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[m][t] = f32x4{0, 0, 0, 0};
    const int rpos = 16 * (kk ^ ((r16 + 4) >> 3 & 1));
    const char* abase = smem + (16 * MR * wa + r16) * CWS_RS + rpos;
    const char* bbase = smem + (CWS_T + 64 * wb + r16) * CWS_RS + rpos;
    auto compute = [&]() {
        cms_u32x4 A[MR][NPG];
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int pl = 0; pl < NPG; ++pl) A[m][pl] = *reinterpret_cast<const cms_u32x4*>(abase + pl * CWS_PLANE + m * 16 * CWS_RS);
        if constexpr (MR >= 4) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                cms_u32x4 Bp[NPX];
#pragma unroll
                for (int pl = 0; pl < NPX; ++pl) Bp[pl] = *reinterpret_cast<const cms_u32x4*>(bbase + pl * CWS_PLANE + t * 16 * CWS_RS);
                // products (i, j) with i + j <= 2, smallest first; the MR row tiles between two uses of an accumulator
#pragma unroll
                for (int sum = 2; sum >= 0; --sum)
#pragma unroll
                    for (int i = NPG - 1; i >= 0; --i) {
                        const int jx = sum - i;
                        if (jx < 0 || jx >= NPX) continue;
#pragma unroll
                        for (int m = 0; m < MR; ++m) acc[m][t] = cms_mfma(A[m][i], Bp[jx], acc[m][t]);
                    }
            }
        } else {
            // two row tiles: with the column tiles in the outer loop an accumulator came round again after TWO MFMAs (32 cycles, less than
            // the instruction's latency: cycle stamps of the -DUNO_CWS_STAMPS build, fc1 128 -> 64 at 446^2: 2 320 cycles per half chunk
            // for 48 MFMAs = 768 cycles of matrix pipe).  All four column tiles' fragments are read first and the column tiles run
            // inside each product: eight MFMAs between two uses of an accumulator.
            cms_u32x4 Bp[4][NPX];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int pl = 0; pl < NPX; ++pl) Bp[t][pl] = *reinterpret_cast<const cms_u32x4*>(bbase + pl * CWS_PLANE + t * 16 * CWS_RS);
#pragma unroll
            for (int sum = 2; sum >= 0; --sum)
#pragma unroll
                for (int i = NPG - 1; i >= 0; --i) {
                    const int jx = sum - i;
                    if (jx < 0 || jx >= NPX) continue;
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int m = 0; m < MR; ++m) acc[m][t] = cms_mfma(A[m][i], Bp[t][jx], acc[m][t]);
                }
        }
    };

    const int it_begin = 2 * c_begin, it_end = 2 * c_end;          // an even number of half chunks
    if (it_begin < it_end) {
        load_half(it_begin, rgs[0], rxs[0], rqs[0], shs[0], tails[0]);
        __builtin_amdgcn_sched_barrier(0);          // set 0's loads strictly before set 1's: the loop's vmcnt waits are derived from BOTH orders
        load_half(it_begin + 1, rgs[1], rxs[1], rqs[1], shs[1], tails[1]);
        __builtin_amdgcn_sched_barrier(0);
    }
    // development build (-DUNO_CWS_STAMPS, tools/dev/mkvariant.py): cycles per phase of every wave of one workgroup, summed over its
    // half chunks - store (incl. the wait for the loads), barrier, fragment reads + MFMAs, barrier - printed at the end of the kernel
#ifdef UNO_CWS_STAMPS
    unsigned long long tS = 0, tB1 = 0, tC = 0, tB2 = 0, t_prev = __builtin_readcyclecounter();
    const unsigned long long t_begin = t_prev;
#define CWS_STAMP(acc_) do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const unsigned long long t_ = __builtin_readcyclecounter(); (acc_) += t_ - t_prev; t_prev = t_; } while (0)
#else
#define CWS_STAMP(acc_) do { } while (0)
#endif
    for (int it = it_begin; it < it_end; it += 2) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (tails[h] || edge) store_half(rgs[h], rxs[h], rqs[h], shs[h], true);          // (waits for this half chunk's loads only: vmcnt counts the other set's)
            else store_half(rgs[h], rxs[h], rqs[h], shs[h], false);
            CWS_STAMP(tS);
            __syncthreads();
            CWS_STAMP(tB1);
            load_half(min(it + h + 2, it_end - 1), rgs[h], rxs[h], rqs[h], shs[h], tails[h]);
            __builtin_amdgcn_sched_barrier(0);
            compute();
            __builtin_amdgcn_sched_barrier(0);
            CWS_STAMP(tC);
            __syncthreads();
            CWS_STAMP(tB2);
        }
    }
#ifdef UNO_CWS_STAMPS
    if (blockIdx.x == 9 && lane == 0)
        printf("K9-S stamps wg %d wave %d halves %d: store %llu  barrier1 %llu  multiply %llu  barrier2 %llu  loop %llu cycles\n", (int)blockIdx.x, wave,
               it_end - it_begin, tS, tB1, tC, tB2, t_prev - t_begin);
#endif
#undef CWS_STAMP

    float* part = p.part + (size_t)split * p.Co * (p.Ci + 1);
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = o0 + 16 * MR * wa + 16 * m + 4 * kk + r;
            if (o < p.Co) {
                const float sc = PB ? p.pb_w2[o] : 1.f;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int i = i0 + 64 * wb + 16 * t + r16;
                    if (i < p.Ci) part[(size_t)o * (p.Ci + 1) + i] = PB ? acc[m][t][r] * sc : acc[m][t][r];
                }
            }
        }
    if (i0 == 0) {          // bias gradient: the 8 threads that share a row hold its partial sums
        float* part2 = PB ? p.part2 + (size_t)split * (p.Co + 1) : nullptr;
#pragma unroll
        for (int u = 0; u < MR; ++u) {
            float v = bs[u];
            v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
            const int o = o0 + row0 + 32 * u;
            if constexpr (PB) {
                float v2 = bs2[u];
                v2 += __shfl_xor(v2, 1); v2 += __shfl_xor(v2, 2); v2 += __shfl_xor(v2, 4);
                if ((tid & 7) == 0 && o < p.Co) { part[(size_t)o * (p.Ci + 1) + p.Ci] = v * p.pb_w2[o]; part2[o] = v2; }
            } else if ((tid & 7) == 0 && o < p.Co) part[(size_t)o * (p.Ci + 1) + p.Ci] = v;
        }
        if constexpr (PB) {
            float v = qs;
            v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
            if (tid == 0 && o0 == 0) part2[p.Co] = v;
        }
    }
}

// second stage of the projection's own gradients (PB): one wave per entry, lanes stride over the splits, fixed order
__global__ __launch_bounds__(256) void channel_wgrad_pb_reduce_kernel(const float* __restrict__ part2, float* __restrict__ gw2, float* __restrict__ gb2,
                                                                      int Co, int nsplit) {
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e > Co) return;
    float v = 0.f;
    for (int k = lane; k < nsplit; k += 64) v += part2[(size_t)k * (Co + 1) + e];
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) {
        if (e < Co) gw2[e] = v;
        else if (gb2) gb2[0] = v;
    }
}


// Weight gradient with few input channels (CI <= 4): a thread owns four pixels at a time and accumulates its 16 output channels x
// (CI + 1) sums in registers over the pixels of its split (the + 1: the bias gradient); fixed-order reduction inside the workgroup
// (butterfly within a wave, the four waves through LDS in order), then the usual partials (split, Co, Ci + 1) for the reduce kernel.
template <int CI, bool BF>
__global__ __launch_bounds__(256) void channel_wgrad_few_in_kernel(ChannelWgradParams p, long long quads_per_split) {
    using T = typename IoElem<BF>::type;
    __shared__ float sred[4][16 * (CI + 1)];
    const int split = blockIdx.x, o0 = blockIdx.y * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long qrow = ((long long)p.P + 3) >> 2;                   // pixel quads per (batch entry, channel) row
    const long long qa = (long long)split * quads_per_split, qb = min(qa + quads_per_split, (long long)p.B * qrow);
    float acc[16][CI + 1];
#pragma unroll
    for (int o = 0; o < 16; ++o)
#pragma unroll
        for (int i = 0; i <= CI; ++i) acc[o][i] = 0.f;
    for (long long q = qa + tid; q < qb; q += 256) {
        const int b = (int)(q / qrow), px = (int)(4 * (q - (long long)b * qrow));
        const T* xb = reinterpret_cast<const T*>(p.x) + (size_t)b * CI * p.P + px;
        const T* gb = reinterpret_cast<const T*>(p.gy) + ((size_t)b * p.Co + o0) * p.P + px;
        const bool full = px + 3 < p.P;
        float xv[CI][4];
#pragma unroll
        for (int i = 0; i < CI; ++i) {
            if (full) { const float4 v = io_ld4(xb + (size_t)i * p.P); xv[i][0] = v.x; xv[i][1] = v.y; xv[i][2] = v.z; xv[i][3] = v.w; }
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) xv[i][e] = px + e < p.P ? io_widen(xb[(size_t)i * p.P + e]) : 0.f;
            }
        }
#pragma unroll
        for (int o = 0; o < 16; ++o) {
            float gv[4] = {0.f, 0.f, 0.f, 0.f};
            if (o0 + o < p.Co) {
                if (full) { const float4 v = io_ld4(gb + (size_t)o * p.P); gv[0] = v.x; gv[1] = v.y; gv[2] = v.z; gv[3] = v.w; }
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) gv[e] = px + e < p.P ? io_widen(gb[(size_t)o * p.P + e]) : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < CI; ++i) acc[o][i] += (gv[0] * xv[i][0] + gv[1] * xv[i][1]) + (gv[2] * xv[i][2] + gv[3] * xv[i][3]);
            acc[o][CI] += (gv[0] + gv[1]) + (gv[2] + gv[3]);
        }
    }
#pragma unroll
    for (int o = 0; o < 16; ++o)
#pragma unroll
        for (int i = 0; i <= CI; ++i) {
            float v = acc[o][i];
            v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
            if (lane == 0) sred[wave][o * (CI + 1) + i] = v;
        }
    __syncthreads();
    if (tid < 16 * (CI + 1)) {
        const int o = tid / (CI + 1), i = tid % (CI + 1);
        const float v = ((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid];
        if (o0 + o < p.Co) p.part[((size_t)split * p.Co + o0 + o) * (CI + 1) + i] = v;
    }
}

// fixed-order sum of the split-K partials (deterministic): gw (Co, Ci), gb (Co).  32 consecutive elements x 8
// interleaved groups of splits per workgroup, the 8 group sums combined in order through LDS.
__global__ __launch_bounds__(256) void channel_wgrad_reduce_kernel(const float* part, float* gw, float* gb, int Co, int Ci, int nsplit,
                                                                   int accumulate) {
    __shared__ float sh[8][33];
    const int el = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int e = blockIdx.x * 32 + el;
    const int n = Co * (Ci + 1);
    float acc = 0.f;
    if (e < n) {
        // 8 independent loads per round (the plain loop issued one load per iteration: a chain of nsplit / 8 memory latencies);
        // the order of the additions stays fixed
        int s = grp;
        for (; s + 56 < nsplit; s += 64) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = part[(size_t)(s + 8 * i) * n + e];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc += v[i];
        }
        for (; s < nsplit; s += 8) acc += part[(size_t)s * n + e];
    }
    sh[grp][el] = acc;
    __syncthreads();
    if (grp == 0 && e < n) {
        float t = sh[0][el];
#pragma unroll
        for (int g = 1; g < 8; ++g) t += sh[g][el];
        const int o = e / (Ci + 1), i = e % (Ci + 1);
        // accumulate: the results are added to what gw / gb hold (a parameter's gradient buffer written in place)
        if (i < Ci) gw[(size_t)o * Ci + i] = accumulate == 1 ? gw[(size_t)o * Ci + i] + t : t;
        else if (gb) gb[o] = accumulate == 1 ? gb[o] + t : t;
    }
}

// split-K plan: ~1024 workgroups, each at least 4 chunks long; splits are whole chunks of one batch entry
static void wgrad_plan(int B, int Ci, int Co, long long P, int* nsplit, int* npc, int* cps, int* pk) {
    const int tiles = ((Co + CW_T - 1) / CW_T) * ((Ci + CW_T - 1) / CW_T);
    *pk = P >= 64 ? CWV_PK : CW_PK;
    *npc = (int)((P + *pk - 1) / *pk);
    const long long nchunks = (long long)B * *npc;
    long long want = (1024 + tiles - 1) / tiles;
    if (wgrad_split_shape(B, Ci, Co, P)) {             // K9-S: 128 x 128 weight tiles, two resident workgroups per CU = 512
        const int to = wgrad_split_rows(Co);
        const int tiles_s = ((Co + to - 1) / to) * ((Ci + CWS_T - 1) / CWS_T);
        want = (512 + tiles_s - 1) / tiles_s;
    }
    long long per = (nchunks + want - 1) / want;
    if (per < 4) per = 4;
    *cps = (int)per;
    *nsplit = (int)((nchunks + per - 1) / per);
}

long long channel_wgrad_ws_floats(int B, int Ci, int Co, long long P, int* nsplit_out) {
    int nsplit, npc, cps, pk;
    wgrad_plan(B, Ci, Co, P, &nsplit, &npc, &cps, &pk);
    if (nsplit_out) *nsplit_out = nsplit;
    return (long long)nsplit * Co * (long long)(Ci + 1);
}

int launch_channel_wgrad(const void* gy, const void* x, float* gw, float* gb, float* ws, int B, int Ci, int Co, long long P,
                         int act_x, int bf16, hipStream_t s) {
    return launch_channel_wgrad2(gy, x, nullptr, Ci, gw, gb, ws, B, Ci, Co, P, act_x, 0, bf16, s);
}

int launch_channel_wgrad_vh(const void* gy, const float* vh_x, const float* vh_w, const float* vh_b, int vh_ci, float* gw, float* gb, float* ws,
                            int B, int Ci, int Co, long long P, int act_x, hipStream_t s, int accumulate) {
    if (Ci > 32 || Ci < 5 || vh_ci < 1 || vh_ci > 3 || P < 64 || !act_x || (long long)Co * P >= (1LL << 29) || (long long)B * ((P + 31) / 32) > 0x7fffffffLL) {
        set_error("channel_wgrad: the virtual-input form takes 5 .. 32 virtual channels of <= 3 real ones, read through the GELU, >= 64 pixels");
        return -2;
    }
    ChannelWgradParams p;
    p.gy = gy; p.x = vh_x; p.x2 = nullptr; p.C1 = Ci; p.part = ws; p.B = B; p.Ci = Ci; p.Co = Co; p.P = (int)P; p.act_x = 1;
    p.pm = pix_map(PixelWindow(), P);
    p.vh_x = vh_x; p.vh_w = vh_w; p.vh_b = vh_b; p.vh_ci = vh_ci;
    p.pb_w2 = nullptr; p.pb_g = nullptr; p.part2 = nullptr;
    int npc, cps, pk;
    wgrad_plan(B, Ci, Co, P, &p.nsplit, &npc, &cps, &pk);
    p.span = (long long)cps * pk;
    p.rev = next_sweep_reversed(SWEEP_K9);
    const int tiles = ((Co + CW_T - 1) / CW_T) * ((Ci + CW_T - 1) / CW_T);
    {
        ProfScope prof("uno::channel_wgrad_vec_kernel", 4.0 * B * (double)P * (vh_ci + Co), s);
        hipLaunchKernelGGL((channel_wgrad_vec_kernel<true, false, 2, true>), dim3(8 * tiles * ((p.nsplit + 7) / 8)), dim3(256), 0, s, p, npc, cps);
    }
    hipLaunchKernelGGL(channel_wgrad_reduce_kernel, dim3((Co * (Ci + 1) + 31) / 32), dim3(256), 0, s, ws, gw, gb, Co, Ci, p.nsplit, accumulate ? 1 : 0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("channel_wgrad launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

bool channel_wgrad_pb_applies(int B, int Ci, int Co, int C1, long long P) {
    int nsplit, npc, cps, pk;
    if (B < 1 || P < 64) return false;
    wgrad_plan(B, Ci, Co, P, &nsplit, &npc, &cps, &pk);
    return wgrad_split_shape(B, Ci, Co, P) && pk == CWV_PK && Ci > 4 && (C1 == Ci || C1 % 32 == 0);
}
long long channel_wgrad_pb_ws_floats(int B, int Ci, int Co, long long P) {
    int nsplit;
    const long long n = channel_wgrad_ws_floats(B, Ci, Co, P, &nsplit);
    return n + (long long)nsplit * (Co + 1);
}

int launch_channel_wgrad2(const void* gy, const void* x, const void* x2, int C1, float* gw, float* gb, float* ws, int B, int Ci, int Co,
                          long long P, int act_x, int accumulate, int bf16, hipStream_t s, const PixelWindow& win, const WgradProjectedBack& pb) {
    const bool windowed = win.cols != 0;
    if (const char* why = pix_window_error(win, P)) { set_error("channel_wgrad: %s", why); return -2; }
    const long long PSl = windowed ? win.plane : P;
    if ((long long)(Ci > Co ? Ci : Co) * PSl >= (1LL << 29) || (long long)B * ((P + 31) / 32) > 0x7fffffffLL) {
        set_error("channel_wgrad: tensor too large (channels * pixels must stay below 2^29)");
        return -2;
    }
    if (x2 && (P < 64 || C1 < CW_T || C1 >= Ci || C1 % CW_T)) {
        set_error("channel_wgrad: a two-source call needs >= 64 pixels and a split at a multiple of %d inside (0, Ci) (got %d of %d)", CW_T, C1, Ci);
        return -2;
    }
    ChannelWgradParams p;
    p.gy = gy; p.x = x; p.x2 = x2; p.C1 = x2 ? C1 : Ci; p.part = ws; p.B = B; p.Ci = Ci; p.Co = Co; p.P = (int)P; p.act_x = act_x ? 1 : 0;
    p.pm = pix_map(win, P);
    p.vh_x = nullptr; p.vh_w = nullptr; p.vh_b = nullptr; p.vh_ci = 0;
    int npc, cps, pk;
    wgrad_plan(B, Ci, Co, P, &p.nsplit, &npc, &cps, &pk);
    p.pb_w2 = pb.w2; p.pb_g = pb.g; p.part2 = ws + (size_t)p.nsplit * Co * (Ci + 1);
    if (pb.w2 && (!pb.g || !pb.gw2 || bf16 || accumulate == 3 || !channel_wgrad_pb_applies(B, Ci, Co, x2 ? C1 : Ci, P))) {
        set_error("channel_wgrad: the projected-back gradient goes with the float32 split kernel (both stages)");
        return -3;
    }
    if (windowed && (pk != CWV_PK || (Ci <= 4 && !act_x))) { set_error("channel_wgrad: the pixel window goes with the vector / split kernels (>= 64 pixels, > 4 input channels)"); return -2; }
    p.span = (long long)cps * pk;
    p.rev = next_sweep_reversed(SWEEP_K9);
    const int tiles = ((Co + CW_T - 1) / CW_T) * ((Ci + CW_T - 1) / CW_T);
    if (Ci <= 4 && !act_x && P >= 1024) {
        const long long quads = (long long)B * ((P + 3) / 4), qps = (quads + p.nsplit - 1) / p.nsplit;
        {
            ProfScope prof("uno::channel_wgrad_few_in_kernel", (bf16 ? 2.0 : 4.0) * B * (double)P * (Ci + Co), s);
            const dim3 grid((unsigned)p.nsplit, (unsigned)((Co + 15) / 16));
#define UNO_CWF(C) do { if (bf16) hipLaunchKernelGGL((channel_wgrad_few_in_kernel<C, true>), grid, dim3(256), 0, s, p, qps); \
                        else hipLaunchKernelGGL((channel_wgrad_few_in_kernel<C, false>), grid, dim3(256), 0, s, p, qps); } while (0)
            if (Ci == 1) UNO_CWF(1); else if (Ci == 2) UNO_CWF(2); else if (Ci == 3) UNO_CWF(3); else UNO_CWF(4);
#undef UNO_CWF
        }
        const int nf = Co * (Ci + 1);
        if (accumulate != 3)
            hipLaunchKernelGGL(channel_wgrad_reduce_kernel, dim3((nf + 31) / 32), dim3(256), 0, s, ws, gw, gb, Co, Ci, p.nsplit, accumulate);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { set_error("channel_wgrad launch: %s", hipGetErrorString(e)); return -5; }
        return 0;
    }
    const bool split_form = wgrad_split_shape(B, Ci, Co, P) && pk == CWV_PK && (!x2 || C1 % 32 == 0);
    {
        ProfScope prof(split_form ? "uno::channel_wgrad_split_kernel" : pk == CWV_PK ? "uno::channel_wgrad_vec_kernel" : "uno::channel_wgrad_kernel",
                       (bf16 ? 2.0 : 4.0) * B * (double)P * (Ci + Co + (pb.w2 ? 1 : 0)), s);
        const dim3 gv(8 * tiles * ((p.nsplit + 7) / 8));
        if (split_form) {
            const int to = wgrad_split_rows(Co);
            const int tiles_s = ((Co + to - 1) / to) * ((Ci + CWS_T - 1) / CWS_T);
            const dim3 gs(8 * tiles_s * ((p.nsplit + 7) / 8));
#define UNO_CWS(A_, M_) do { if (bf16) hipLaunchKernelGGL((channel_wgrad_split_kernel<A_, M_, true>), gs, dim3(256), 0, s, p, npc, cps); \
                             else hipLaunchKernelGGL((channel_wgrad_split_kernel<A_, M_, false>), gs, dim3(256), 0, s, p, npc, cps); } while (0)
#define UNO_CWS_PB(A_, M_) hipLaunchKernelGGL((channel_wgrad_split_kernel<A_, M_, false, true>), gs, dim3(256), 0, s, p, npc, cps)
            if (pb.w2) {
                if (to == CWS_T) { if (act_x) UNO_CWS_PB(true, 4); else UNO_CWS_PB(false, 4); }
                else { if (act_x) UNO_CWS_PB(true, 2); else UNO_CWS_PB(false, 2); }
            }
            else if (to == CWS_T) { if (act_x) UNO_CWS(true, 4); else UNO_CWS(false, 4); }
            else { if (act_x) UNO_CWS(true, 2); else UNO_CWS(false, 2); }
#undef UNO_CWS_PB
#undef UNO_CWS
        } else if (pk == CWV_PK && Ci <= 32) {           // (one tile of input channels: the narrow form)
            if (act_x) { if (bf16) hipLaunchKernelGGL((channel_wgrad_vec_kernel<true, true, 2>), gv, dim3(256), 0, s, p, npc, cps);
                         else hipLaunchKernelGGL((channel_wgrad_vec_kernel<true, false, 2>), gv, dim3(256), 0, s, p, npc, cps); }
            else { if (bf16) hipLaunchKernelGGL((channel_wgrad_vec_kernel<false, true, 2>), gv, dim3(256), 0, s, p, npc, cps);
                   else hipLaunchKernelGGL((channel_wgrad_vec_kernel<false, false, 2>), gv, dim3(256), 0, s, p, npc, cps); }
        } else if (pk == CWV_PK && act_x) {
            if (bf16) hipLaunchKernelGGL((channel_wgrad_vec_kernel<true, true>), gv, dim3(256), 0, s, p, npc, cps);
            else hipLaunchKernelGGL((channel_wgrad_vec_kernel<true, false>), gv, dim3(256), 0, s, p, npc, cps);
        } else if (pk == CWV_PK) {
            if (bf16) hipLaunchKernelGGL((channel_wgrad_vec_kernel<false, true>), gv, dim3(256), 0, s, p, npc, cps);
            else hipLaunchKernelGGL((channel_wgrad_vec_kernel<false, false>), gv, dim3(256), 0, s, p, npc, cps);
        } else if (bf16) {
            hipLaunchKernelGGL(channel_wgrad_kernel<true>, dim3(tiles, p.nsplit), dim3(256), 0, s, p, npc, cps);
        } else {
            hipLaunchKernelGGL(channel_wgrad_kernel<false>, dim3(tiles, p.nsplit), dim3(256), 0, s, p, npc, cps);
        }
    }
    const int n = Co * (Ci + 1);
    if (accumulate != 3)        // 3: the partial sums stay in ws; launch_channel_wgrad_finish sums any number of such blocks later
        hipLaunchKernelGGL(channel_wgrad_reduce_kernel, dim3((n + 31) / 32), dim3(256), 0, s, ws, gw, gb, Co, Ci, p.nsplit, accumulate);
    if (pb.w2) hipLaunchKernelGGL(channel_wgrad_pb_reduce_kernel, dim3((Co + 1 + 3) / 4), dim3(256), 0, s, p.part2, pb.gw2, pb.gb2, Co, p.nsplit);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("channel_wgrad launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

// second stage alone: nparts consecutive (Co, Ci + 1) blocks of partial sums (the ws of one or more stage-1 calls with
// accumulate = 3, laid out one after the other) -> gw, gb, in the fixed order of the blocks
int launch_channel_wgrad_finish(const float* parts, float* gw, float* gb, int Ci, int Co, long long nparts, int accumulate, hipStream_t s) {
    if (nparts < 1 || nparts > 0x7fffffffLL) { set_error("channel_wgrad_finish: %lld partial blocks", nparts); return -2; }
    const int n = Co * (Ci + 1);
    hipLaunchKernelGGL(channel_wgrad_reduce_kernel, dim3((n + 31) / 32), dim3(256), 0, s, parts, gw, gb, Co, Ci, (int)nparts, accumulate ? 1 : 0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("channel_wgrad_finish launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

}  // namespace uno
