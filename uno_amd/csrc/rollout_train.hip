// K19 / K19-B - the NS-2D TRAINING roll-out (reference ns_train_2d.py:46-68) without a window tensor.
//
// The window of roll-out step t is T_in consecutive frames of the sequence "the T_in given frames, then the predictions":
//   frame j = given[:, j] for j < T_in, otherwise pred[:, j - T_in]            given (B, T_in, P), pred (B, T, P) time-major (K18 writes it)
// and the only layer that reads the window is the first lift `fc`, a point-wise C -> Cm map with C = T_in + F: the F positional
// features feat (F, P) are one table for all batch entries.  So nothing is concatenated, forwards or backwards:
//
//   K19    h[b][m][p]       = bias[m] + sum_{k<T_in} w[m][k] frame_{t+k}[b][p] + sum_{f<F} w[m][T_in+f] feat[f][p]      (ascending c)
//   K19-B  parts[t][b][chunk][m][c] = sum_{p in chunk} gh[b][m][p] x[c][p],  column C: sum_p gh[b][m][p]                   (Cm, C + 1) blocks
//          gpred[b][q][p]  += sum_m w[m][k] gh[b][m][p]      for every predicted frame q = t + k - T_in >= 0 of the window but the newest
//          gframe[b][p]     = gpred[b][t-1][p] + sum_m w[m][T_in-1] gh[b][m][p] + gL (pred - target)[b][t-1][p] / (sqrt(num) sqrt(den))     (t >= 1)
//   seed   gframe[b][p]     = gL (pred - target)[b][T-1][p] / (sqrt(num) sqrt(den))       the last frame: no lift follows it
//
// The backward pass walks the steps in reverse, so when window t runs every later window has already added its share to gpred[:, t - 1]:
// gframe is the COMPLETE gradient of the model's output of step t - 1 (its uses as an input frame and its loss term).  num / den are
// the `sums` of uno_rollout_finish; gL (the gradient at the loss) is read through a device pointer: no host synchronisation.  Where
// num == 0 the loss term is 0, as the backward of torch.linalg.vector_norm gives; a zero den gives inf / NaN as torch does.
//
// The parts blocks have the layout channel_wgrad_reduce_kernel sums (bias sums in column C), the blocks of all T windows lie in one
// workspace in the order [t][b][chunk]: ONE launch_channel_wgrad_finish per training step turns them into gw and gb.
//
// No atomics: a thread owns its pixel's column of gpred, launches are stream-ordered.  The chunk decomposition is rollout_chunks(P) -
// a function of P alone, never of the CU count or uno_reserve_cus - and every sum runs in a fixed order (a weight sum: one thread walks
// the chunk's pixels in ascending order on four interleaved accumulators), so two calls, a call under reserved CUs and a graph replay
// give the same bits.
//
// K19-B stages a tile of TP pixels of gh (Cm rows) and of the inputs (C rows + a row of ones for the bias sums) in LDS, row pitch
// TP + 4 floats: ds_read_b128 banks are (a / 4) % 64, so 16 consecutive rows start on 16 different 16-byte slots of the bank row and the
// 16-lane groups of a read (lanes of one group differ in the row, not in the pixel) do not collide.  TP = 256 while the tile stays
// below 48 KB (Cm + C + 1 <= 47: 31 rows = 32 KB for UNO(14, 32)), 128 up to the limits Cm = 64, C = 32 (97 rows = 51 KB); with the
// 8 KB weight image that is under the 64 KB a workgroup gets without opting in, and two to four workgroups fit the CU's 160 KB.
#include "uno_common.h"

namespace uno {

enum { RT_THREADS = 256, RT_MAX_C = 32, RT_MAX_CM = 64, RT_PAD = 4, RT_NE = (RT_MAX_CM * (RT_MAX_C + 1) + RT_THREADS - 1) / RT_THREADS };

template <int V> struct RtVec;
template <> struct RtVec<1> {
    typedef float type;
    static __device__ __forceinline__ float ld(const float* p) { return *p; }
    static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
    static __device__ __forceinline__ float splat(float v) { return v; }
    static __device__ __forceinline__ void fma(float w, float x, float& acc) { acc = fmaf(w, x, acc); }
};
template <> struct RtVec<4> {           // 16 bytes per lane at 4-byte alignment (f4u), as K18
    typedef float4 type;
    static __device__ __forceinline__ float4 ld(const float* p) { return io_ld4(p); }
    static __device__ __forceinline__ void st(float* p, const float4& v) { io_store4(p, v.x, v.y, v.z, v.w); }
    static __device__ __forceinline__ float4 splat(float v) { return make_float4(v, v, v, v); }
    static __device__ __forceinline__ void fma(float w, const float4& x, float4& acc) {
        acc.x = fmaf(w, x.x, acc.x); acc.y = fmaf(w, x.y, acc.y); acc.z = fmaf(w, x.z, acc.z); acc.w = fmaf(w, x.w, acc.w);
    }
};

// frame j of the sequence [given frames, predictions] of batch entry b
__device__ __forceinline__ const float* rt_frame(const float* given, const float* pred, size_t b, int j, int T_in, int T, size_t P) {
    return j < T_in ? given + (b * (size_t)T_in + (size_t)j) * P : pred + (b * (size_t)T + (size_t)(j - T_in)) * P;
}

// the weight as a zero-padded [Cm][RT_MAX_C] image in LDS (rows 16-byte aligned: four weights per read)
__device__ __forceinline__ void rt_stage_weight(float* s_w, const float* __restrict__ w, int Cm, int C) {
    for (int i = threadIdx.x; i < Cm * RT_MAX_C; i += RT_THREADS) {
        const int m = i / RT_MAX_C, c = i % RT_MAX_C;
        s_w[i] = c < C ? w[m * C + c] : 0.f;
    }
}

// gL / (sqrt(num) sqrt(den)) of (b, q): what multiplies (pred - target)[b][q] in the gradient of sum_b ||d|| / ||y||
__device__ __forceinline__ float rt_loss_scale(const float* __restrict__ sums, const float* __restrict__ gL, size_t b, int T, int q) {
    const float num = sums[2 * (b * (size_t)T + (size_t)q)], den = sums[2 * (b * (size_t)T + (size_t)q) + 1];
    return num == 0.f ? 0.f : gL[0] / (sqrtf(num) * sqrtf(den));
}

// ------------------------------------------------------------------------------------------------ K19
// grid: NC * B workgroups, workgroup g = b * NC + c owns pixels [c * CP, min((c + 1) * CP, P)) of batch entry b.  V = 4 needs P % 4 == 0
template <int V>
__global__ __launch_bounds__(RT_THREADS) void rollout_lift_kernel(const float* __restrict__ given, const float* __restrict__ pred,
                                                                  const float* __restrict__ feat, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, float* __restrict__ h, long long P, int T_in,
                                                                  int F, int Cm, int T, int t, long long CP, int NC) {
    typedef RtVec<V> R;
    typedef typename R::type vec;
    __shared__ __attribute__((aligned(16))) float s_w[RT_MAX_CM * RT_MAX_C];
    __shared__ float s_b[RT_MAX_CM];
    const int tid = threadIdx.x;
    const int C = T_in + F;
    rt_stage_weight(s_w, w, Cm, C);
    for (int i = tid; i < Cm; i += RT_THREADS) s_b[i] = bias ? bias[i] : 0.f;
    __syncthreads();
    const size_t b = blockIdx.x / (unsigned)NC;
    const int c = (int)(blockIdx.x % (unsigned)NC);
    const long long p0 = (long long)c * CP;
    const long long p1 = p0 + CP < P ? p0 + CP : P;
    const size_t sP = (size_t)P;
    float* __restrict__ hb = h + b * (size_t)Cm * sP;
    for (long long p = p0 + (long long)tid * V; p < p1; p += (long long)RT_THREADS * V) {
        vec x[RT_MAX_C];                                        // the pixel's C inputs, statically indexed: registers
#pragma unroll
        for (int k = 0; k < RT_MAX_C; ++k) {
            if (k < T_in) x[k] = R::ld(rt_frame(given, pred, b, t + k, T_in, T, sP) + p);
            else if (k < C) x[k] = R::ld(feat + (size_t)(k - T_in) * sP + p);
            else x[k] = R::splat(0.f);
        }
        for (int m = 0; m < Cm; ++m) {
            vec acc = R::splat(s_b[m]);
#pragma unroll
            for (int k4 = 0; k4 < RT_MAX_C; k4 += 4) {
                if (k4 < C) {                                   // (uniform; the padding of the last group is 0 * 0)
                    const float4 wv = *reinterpret_cast<const float4*>(s_w + m * RT_MAX_C + k4);
                    R::fma(wv.x, x[k4], acc);
                    R::fma(wv.y, x[k4 + 1], acc);
                    R::fma(wv.z, x[k4 + 2], acc);
                    R::fma(wv.w, x[k4 + 3], acc);
                }
            }
            R::st(hb + (size_t)m * sP + p, acc);
        }
    }
}

int launch_rollout_lift(const float* given, const float* pred, const float* feat, const float* w, const float* bias, float* h, int B, int T_in,
                        int F, int Cm, long long P, int T, int t, hipStream_t s) {
    long long cp = 0;
    const long long nc = rollout_chunks(P, &cp);
    if (nc * B > 0x7fffffffLL) { set_error("rollout_lift: %lld chunks x %d batch entries exceed the grid limit", nc, B); return -2; }
    {
        ProfScope prof("uno::rollout_lift_kernel", 4.0 * B * (double)P * (T_in + Cm) + 4.0 * F * (double)P, s);
        if (P % 4 == 0)
            hipLaunchKernelGGL(rollout_lift_kernel<4>, dim3((unsigned)(nc * B)), dim3(RT_THREADS), 0, s, given, pred, feat, w, bias, h, P, T_in, F, Cm,
                               T, t, cp, (int)nc);
        else
            hipLaunchKernelGGL(rollout_lift_kernel<1>, dim3((unsigned)(nc * B)), dim3(RT_THREADS), 0, s, given, pred, feat, w, bias, h, P, T_in, F, Cm,
                               T, t, cp, (int)nc);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("rollout_lift launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

// ------------------------------------------------------------------------------------------------ K19-B
struct RolloutLiftBwdParams {
    const float* gh;            // (B, Cm, P)
    const float* given;         // (B, T_in, P)
    const float* pred;          // (B, T, P)
    const float* target;        // (B, T, P)       t >= 1
    const float* feat;          // (F, P)          F > 0
    const float* w;             // (Cm, C)
    const float* sums;          // (B, T, 2)       t >= 1
    const float* gL;            // (1)             t >= 1
    float* gpred;               // (B, T, P)       t >= 1
    float* gframe;              // (B, P)          t >= 1
    float* parts;               // (T, B, NC, Cm, C + 1)
    long long P, CP;
    int B, T_in, F, Cm, T, t, NC;
};

// floats of all T windows' blocks; the chunk count is rollout_chunks(P): the blocks must lie back to back for the one finish launch
long long rollout_lift_bwd_ws_floats(int B, int C, int Cm, long long P, int T) {
    return (long long)T * B * rollout_chunks(P, nullptr) * Cm * (C + 1);
}

// grid as K19.  Phase A (threads < TP, one pixel each): stage the tile, form the pixel's input gradients; phase B (all threads): thread
// tid owns the sums e = tid, tid + 256, ... of the (Cm, C + 1) block.
template <int TP>
__global__ __launch_bounds__(RT_THREADS) void rollout_lift_bwd_kernel(RolloutLiftBwdParams q) {
    constexpr int PITCH = TP + RT_PAD;
    extern __shared__ __attribute__((aligned(16))) float s_tile[];      // gh rows [Cm][PITCH], then input rows [C + 1][PITCH]
    __shared__ __attribute__((aligned(16))) float s_w[RT_MAX_CM * RT_MAX_C];
    const int tid = threadIdx.x;
    const int T_in = q.T_in, Cm = q.Cm, T = q.T, t = q.t;
    const int C = T_in + q.F;
    const int n = Cm * (C + 1);
    float* s_g = s_tile;
    float* s_x = s_tile + Cm * PITCH;
    rt_stage_weight(s_w, q.w, Cm, C);
    const size_t b = blockIdx.x / (unsigned)q.NC;
    const int c = (int)(blockIdx.x % (unsigned)q.NC);
    const long long p0 = (long long)c * q.CP;
    const long long p1 = p0 + q.CP < q.P ? p0 + q.CP : q.P;
    const size_t sP = (size_t)q.P;
    const int k0 = T_in - t > 0 ? T_in - t : 0;                 // frames k0 ... T_in - 1 of the window are predictions
    const float ls = t >= 1 ? rt_loss_scale(q.sums, q.gL, b, T, t - 1) : 0.f;
    const float* __restrict__ ghb = q.gh + b * (size_t)Cm * sP;

    float acc[RT_NE][4];
    int row_g[RT_NE], row_x[RT_NE];
#pragma unroll
    for (int j = 0; j < RT_NE; ++j) {
        const int e = j * RT_THREADS + tid;
        const int m = e < n ? e / (C + 1) : 0, cc = e < n ? e % (C + 1) : 0;
        row_g[j] = m * PITCH;
        row_x[j] = cc * PITCH;
        acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.f;
    }
    __syncthreads();

    for (long long tile0 = p0; tile0 < p1; tile0 += TP) {
        if (tid < TP) {
            // Every load of a stage is issued before its first use (unrolled, into statically indexed registers): with one workgroup per
            // CU there is nothing else to hide a memory round trip behind, and a load-use-load chain of C + Cm + T_in of them per tile
            // was the whole run time of this kernel.  A pixel past the chunk reads the chunk's last one (in bounds) and stages zeros.
            const long long p = tile0 + tid;
            const bool valid = p < p1;
            const size_t pc = (size_t)(valid ? p : p1 - 1);
            float xv[RT_MAX_C];
#pragma unroll
            for (int k = 0; k < RT_MAX_C; ++k) {
                if (k < T_in) xv[k] = rt_frame(q.given, q.pred, b, t + k, T_in, T, sP)[pc];
                else if (k < C) xv[k] = q.feat[(size_t)(k - T_in) * sP + pc];
            }
#pragma unroll
            for (int k = 0; k < RT_MAX_C; ++k)
                if (k < C) s_x[k * PITCH + tid] = valid ? xv[k] : 0.f;
            s_x[C * PITCH + tid] = valid ? 1.f : 0.f;
            float gx[RT_MAX_C];                                 // statically indexed: registers
#pragma unroll
            for (int k = 0; k < RT_MAX_C; ++k) gx[k] = 0.f;
            for (int m0 = 0; m0 < Cm; m0 += 8) {                // eight rows of gh in flight
                float g[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) g[i] = m0 + i < Cm ? ghb[(size_t)(m0 + i) * sP + pc] : 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (m0 + i < Cm) {                          // (uniform)
                        const int m = m0 + i;
                        const float gv = valid ? g[i] : 0.f;
                        s_g[m * PITCH + tid] = gv;
#pragma unroll
                        for (int k4 = 0; k4 < RT_MAX_C; k4 += 4) {
                            if (k4 < T_in && k4 + 4 > k0) {     // (uniform) a group that holds a predicted frame
                                const float4 wv = *reinterpret_cast<const float4*>(s_w + m * RT_MAX_C + k4);
                                gx[k4] = fmaf(wv.x, gv, gx[k4]);
                                gx[k4 + 1] = fmaf(wv.y, gv, gx[k4 + 1]);
                                gx[k4 + 2] = fmaf(wv.z, gv, gx[k4 + 2]);
                                gx[k4 + 3] = fmaf(wv.w, gv, gx[k4 + 3]);
                            }
                        }
                    }
                }
            }
            if (valid && t >= 1) {
                float* gpb = q.gpred + b * (size_t)T * sP + (size_t)p;          // this thread's column of gpred: no other thread touches it
                const size_t o = (b * (size_t)T + (size_t)(t - 1)) * sP + (size_t)p;
                float old[RT_MAX_C];
#pragma unroll
                for (int k = 0; k < RT_MAX_C; ++k)
                    if (k >= k0 && k < T_in - 1) old[k] = gpb[(size_t)(t + k - T_in) * sP];
                const float g_new = gpb[(size_t)(t - 1) * sP], pr = q.pred[o], tg = q.target[o];
                float gx_new = 0.f;
#pragma unroll
                for (int k = 0; k < RT_MAX_C; ++k) {
                    if (k >= k0 && k < T_in - 1) gpb[(size_t)(t + k - T_in) * sP] = old[k] + gx[k];      // an older predicted frame
                    else if (k == T_in - 1) gx_new = gx[k];
                }
                q.gframe[b * sP + (size_t)p] = (g_new + gx_new) + ls * (pr - tg);       // the newest: complete after this launch
            }
        }
        __syncthreads();
        const long long left = p1 - tile0;
        const int quads = left >= TP ? TP / 4 : (int)((left + 3) / 4);
#pragma unroll
        for (int j = 0; j < RT_NE; ++j) {
            if (j * RT_THREADS < n && j * RT_THREADS + tid < n) {
                const float4* __restrict__ gp = reinterpret_cast<const float4*>(s_g + row_g[j]);
                const float4* __restrict__ xp = reinterpret_cast<const float4*>(s_x + row_x[j]);
#pragma unroll 4
                for (int i = 0; i < quads; ++i) {
                    const float4 a = gp[i], x = xp[i];
                    acc[j][0] = fmaf(a.x, x.x, acc[j][0]);
                    acc[j][1] = fmaf(a.y, x.y, acc[j][1]);
                    acc[j][2] = fmaf(a.z, x.z, acc[j][2]);
                    acc[j][3] = fmaf(a.w, x.w, acc[j][3]);
                }
            }
        }
        __syncthreads();
    }
    float* __restrict__ block = q.parts + (((size_t)t * (size_t)q.B + b) * (size_t)q.NC + (size_t)c) * (size_t)n;
#pragma unroll
    for (int j = 0; j < RT_NE; ++j) {
        const int e = j * RT_THREADS + tid;
        if (e < n) block[e] = (acc[j][0] + acc[j][1]) + (acc[j][2] + acc[j][3]);
    }
}

int launch_rollout_lift_backward(const float* gh, const float* given, const float* pred, const float* target, const float* feat, const float* w,
                                 const float* sums, const float* gL, float* gpred, float* gframe, float* parts, int B, int T_in, int F, int Cm,
                                 long long P, int T, int t, hipStream_t s) {
    RolloutLiftBwdParams q;
    q.gh = gh; q.given = given; q.pred = pred; q.target = target; q.feat = feat; q.w = w; q.sums = sums; q.gL = gL; q.gpred = gpred;
    q.gframe = gframe; q.parts = parts; q.P = P; q.B = B; q.T_in = T_in; q.F = F; q.Cm = Cm; q.T = T; q.t = t;
    const long long nc = rollout_chunks(P, &q.CP);
    q.NC = (int)nc;
    if (nc * B > 0x7fffffffLL) { set_error("rollout_lift_backward: %lld chunks x %d batch entries exceed the grid limit", nc, B); return -2; }
    const int rows = Cm + T_in + F + 1;
    const bool wide = (size_t)rows * (256 + RT_PAD) * sizeof(float) <= 48u * 1024u;
    const size_t lds = (size_t)rows * ((wide ? 256 : 128) + RT_PAD) * sizeof(float);
    {
        const int older = t > 1 ? (t - 1 < T_in - 1 ? t - 1 : T_in - 1) : 0;
        ProfScope prof("uno::rollout_lift_bwd_kernel", 4.0 * B * (double)P * (Cm + T_in + 2 * older + (t >= 1 ? 4 : 0)) + 4.0 * F * (double)P, s);
        if (wide) hipLaunchKernelGGL(rollout_lift_bwd_kernel<256>, dim3((unsigned)(nc * B)), dim3(RT_THREADS), lds, s, q);
        else hipLaunchKernelGGL(rollout_lift_bwd_kernel<128>, dim3((unsigned)(nc * B)), dim3(RT_THREADS), lds, s, q);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("rollout_lift_backward launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

// ------------------------------------------------------------------------------------------------ the last frame's loss gradient
__global__ __launch_bounds__(RT_THREADS) void rollout_loss_seed_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                       const float* __restrict__ sums, const float* __restrict__ gL,
                                                                       float* __restrict__ gframe, long long P, int T, long long CP, int NC) {
    const size_t b = blockIdx.x / (unsigned)NC;
    const int c = (int)(blockIdx.x % (unsigned)NC);
    const long long p0 = (long long)c * CP;
    const long long p1 = p0 + CP < P ? p0 + CP : P;
    const float ls = rt_loss_scale(sums, gL, b, T, T - 1);
    const size_t o = (b * (size_t)T + (size_t)(T - 1)) * (size_t)P;
    for (long long p = p0 + threadIdx.x; p < p1; p += RT_THREADS) gframe[b * (size_t)P + p] = ls * (pred[o + p] - target[o + p]);
}

int launch_rollout_loss_seed(const float* pred, const float* target, const float* sums, const float* gL, float* gframe, int B, long long P, int T,
                             hipStream_t s) {
    long long cp = 0;
    const long long nc = rollout_chunks(P, &cp);
    if (nc * B > 0x7fffffffLL) { set_error("rollout_loss_seed: %lld chunks x %d batch entries exceed the grid limit", nc, B); return -2; }
    {
        ProfScope prof("uno::rollout_loss_seed_kernel", 12.0 * B * (double)P, s);
        hipLaunchKernelGGL(rollout_loss_seed_kernel, dim3((unsigned)(nc * B)), dim3(RT_THREADS), 0, s, pred, target, sums, gL, gframe, P, T, cp, (int)nc);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("rollout_loss_seed launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

}  // namespace uno
