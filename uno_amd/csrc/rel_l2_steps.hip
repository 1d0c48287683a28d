// K17 - the per-time-step relative L2 error of the NS-3D loop in one pass over pred and target (its gradient: K17-B, at the end):
//
//   sums[b][t]  = [ sum_p (pred[b][p][t] - target[b][p][t])^2,  sum_p target[b][p][t]^2 ]
//   rel[b][t]   = sqrt(num) / sqrt(den) for t < T;  rel[b][T] = sqrt(sum_t num) / sqrt(sum_t den)
//   totals      = [ sum_b sum_t rel[b][t],  sum_b rel[b][T] ]
//
// The reference's training and validation loops (ns_train_3d.py:55-62, 84-98) form totals[0] slice by slice under no_grad:
// T times `LpLoss(size_average=False)(out[..., t], y[..., t])` = 6 small launches per time step on strided views, each touching
// every cache line of both tensors.  Here: one streaming launch over (chunk, batch entry) and one one-workgroup finish launch.
//
// No atomics, and the chunk decomposition depends on (P, T) alone (never on the CU count or on uno_reserve_cus): the summation
// order is fixed, so two calls - or a call and a graph replay - give the same bits.  No clamping: a zero target slice gives
// rel = +inf (or NaN for 0 / 0) as torch.norm(.) / torch.norm(.) does.
//
// Partial kernel: 256 threads, A = T * (256 / T) of them active.  A chunk starts on a pixel boundary and A is a multiple of T, so an
// active thread's t = tid % T is constant over its strided walk: two float accumulators in registers, consecutive threads read
// consecutive addresses.  The loads are scalar (4 bytes per lane): a batch entry starts b * P * T floats into the tensor, which is
// not 16-byte aligned when P * T is odd, and a 16-byte lane would carry four different t.  Threads with equal t are combined
// through LDS in ascending thread order.
#include <cstdint>
#include "uno_common.h"

namespace uno {

enum { RL2_THREADS = 256, RL2_CHUNK_FLOATS = 4096, RL2_MAX_CHUNKS = 64, RL2_FINISH_THREADS = 1024 };

// pixels per chunk (a multiple of the 256 / T pixels one pass covers) and the chunk count: about RL2_CHUNK_FLOATS elements per chunk,
// larger chunks once that would give more than RL2_MAX_CHUNKS of them (the finish kernel reads every partial in one workgroup)
long long rel_l2_steps_chunks(long long P, int T, long long* chunk_pixels) {
    const long long R = RL2_THREADS / T;
    const long long passes = (RL2_CHUNK_FLOATS + R * T - 1) / (R * T);
    long long cp = passes * R;
    const long long per = (P + RL2_MAX_CHUNKS - 1) / RL2_MAX_CHUNKS;
    if (per > cp) cp = (per + R - 1) / R * R;
    if (chunk_pixels) *chunk_pixels = cp;
    return (P + cp - 1) / cp;
}

// an upper bound of the chunk count that never shrinks as P grows (the workspace size)
long long rel_l2_steps_ws_floats(int B, long long P, int T) {
    const long long R = RL2_THREADS / T;
    const long long cp_min = (RL2_CHUNK_FLOATS + R * T - 1) / (R * T) * R;
    long long nc = (P + cp_min - 1) / cp_min;
    if (nc > RL2_MAX_CHUNKS) nc = RL2_MAX_CHUNKS;
    return 2LL * B * nc * T;
}

// grid: NC * B workgroups, workgroup g = b * NC + c; ws[b][c][t] = (num, den) of chunk c
__global__ __launch_bounds__(RL2_THREADS) void rel_l2_steps_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                           float2* __restrict__ ws, long long P, int T, long long CP, int NC) {
    __shared__ float s_num[RL2_THREADS];
    __shared__ float s_den[RL2_THREADS];
    const int tid = threadIdx.x;
    const int A = (RL2_THREADS / T) * T;
    const long long b = blockIdx.x / (unsigned)NC;
    const int c = (int)(blockIdx.x % (unsigned)NC);
    const long long p0 = (long long)c * CP;
    const long long p1 = p0 + CP < P ? p0 + CP : P;
    const long long n = (p1 - p0) * T;                          // elements of this chunk; chunk and batch entry start at t = 0
    const size_t base = ((size_t)b * (size_t)P + (size_t)p0) * (size_t)T;
    float num = 0.f, den = 0.f;
    if (tid < A) {
        const float* __restrict__ x = pred + base;
        const float* __restrict__ y = target + base;
        long long e = tid;
        for (; e + 3LL * A < n; e += 4LL * A) {                 // four independent loads of each tensor in flight
            const float x0 = x[e], x1 = x[e + A], x2 = x[e + 2LL * A], x3 = x[e + 3LL * A];
            const float y0 = y[e], y1 = y[e + A], y2 = y[e + 2LL * A], y3 = y[e + 3LL * A];
            const float d0 = x0 - y0, d1 = x1 - y1, d2 = x2 - y2, d3 = x3 - y3;
            num += d0 * d0; den += y0 * y0;
            num += d1 * d1; den += y1 * y1;
            num += d2 * d2; den += y2 * y2;
            num += d3 * d3; den += y3 * y3;
        }
        for (; e < n; e += A) {
            const float xv = x[e], yv = y[e];
            const float d = xv - yv;
            num += d * d; den += yv * yv;
        }
    }
    s_num[tid] = num;
    s_den[tid] = den;
    __syncthreads();
    if (tid < T) {
        float a = 0.f, d = 0.f;
        for (int k = tid; k < A; k += T) { a += s_num[k]; d += s_den[k]; }
        ws[((size_t)b * NC + c) * T + tid] = make_float2(a, d);
    }
}

__device__ __forceinline__ double rl2_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);      // a + b = b + a: every lane ends with the same bits
    return v;
}

// one workgroup of 16 waves: a wave per batch entry, lanes over t; chunk partials are summed in double and rounded once
__global__ __launch_bounds__(RL2_FINISH_THREADS) void rel_l2_steps_finish_kernel(const float2* __restrict__ ws, float* __restrict__ sums,
                                                                                 float* __restrict__ rel, float* __restrict__ totals,
                                                                                 int B, int T, int NC) {
    __shared__ double s_step[RL2_FINISH_THREADS / 64];
    __shared__ double s_full[RL2_FINISH_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double w_step = 0.0, w_full = 0.0;
    for (long long b = wave; b < B; b += RL2_FINISH_THREADS / 64) {
        double num_b = 0.0, den_b = 0.0, step_b = 0.0;
        for (int t = lane; t < T; t += 64) {
            const float2* p = ws + (size_t)b * NC * T + t;
            double dn = 0.0, dd = 0.0;
            for (int c = 0; c < NC; ++c) {
                const float2 v = p[(size_t)c * T];
                dn += (double)v.x; dd += (double)v.y;
            }
            const float fn = (float)dn, fd = (float)dd;
            const size_t o = (size_t)b * T + t;
            sums[2 * o] = fn;
            sums[2 * o + 1] = fd;
            const float r = sqrtf(fn) / sqrtf(fd);
            rel[(size_t)b * (T + 1) + t] = r;
            num_b += (double)fn; den_b += (double)fd; step_b += (double)r;
        }
        num_b = rl2_wave_sum(num_b);
        den_b = rl2_wave_sum(den_b);
        step_b = rl2_wave_sum(step_b);
        const float full = sqrtf((float)num_b) / sqrtf((float)den_b);
        if (lane == 0) rel[(size_t)b * (T + 1) + T] = full;
        w_step += step_b;
        w_full += (double)full;
    }
    if (lane == 0) { s_step[wave] = w_step; s_full[wave] = w_full; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, f = 0.0;
        for (int w = 0; w < RL2_FINISH_THREADS / 64; ++w) { a += s_step[w]; f += s_full[w]; }
        totals[0] = (float)a;
        totals[1] = (float)f;
    }
}

// the finish launch alone: K18 (rollout.hip) fills a workspace of this layout step by step and finishes it with its own chunk count
int launch_rel_l2_steps_finish(const float* ws, float* sums, float* rel, float* totals, int B, int T, long long nc, hipStream_t s) {
    {
        ProfScope prof("uno::rel_l2_steps_finish_kernel", 8.0 * B * (double)nc * T, s);
        hipLaunchKernelGGL(rel_l2_steps_finish_kernel, dim3(1), dim3(RL2_FINISH_THREADS), 0, s, (const float2*)ws, sums, rel, totals, B, T, (int)nc);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("rel_l2_steps finish launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

int launch_rel_l2_steps(const float* pred, const float* target, float* sums, float* rel, float* totals, float* ws, int B, long long P, int T,
                        hipStream_t s) {
    long long cp = 0;
    const long long nc = rel_l2_steps_chunks(P, T, &cp);
    if (nc * B > 0x7fffffffLL) { set_error("rel_l2_steps: %lld chunks x %d batch entries exceed the grid limit", nc, B); return -2; }
    {
        ProfScope prof("uno::rel_l2_steps_partial_kernel", 8.0 * B * (double)P * T, s);
        hipLaunchKernelGGL(rel_l2_steps_partial_kernel, dim3((unsigned)(nc * B)), dim3(RL2_THREADS), 0, s, pred, target, (float2*)ws, P, T, cp, (int)nc);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("rel_l2_steps partial launch: %s", hipGetErrorString(e)); return -5; }
    return launch_rel_l2_steps_finish(ws, sums, rel, totals, B, T, nc, s);
}

// K17-B - the gradient of totals[1] (whole-trajectory loss, upstream g_full) and totals[0] (per-step sum, upstream g_step) at pred:
//
//   gx[b][p][t] = (pred - target)[b][p][t] * (cf[b] + cs[b][t])
//   cf[b]       = g_full / (sqrt(sum_t num) * sqrt(sum_t den)),   cs[b][t] = g_step / (sqrt(num[b][t]) * sqrt(den[b][t]))
//
// with (num, den) = sums[b][t] of the forward call and the whole-trajectory sums formed as the finish kernel forms them (lanes over t
// in double, xor-shuffle wave sum, rounded once).  A coefficient whose num is 0 is 0 (K20's rule, the backward of
// torch.linalg.vector_norm); den is not clamped.  Every element is its own product, so the result does not depend on how the elements
// are spread over workgroups: the launch is sized by the device (usable_cus) and W workgroups share one batch entry, each loading that
// entry's T + 1 coefficients into LDS once.  V = 4: T % 4 == 0 and the three bases 16-byte aligned - a lane's four elements then lie in
// one pixel (no wrap of t) and every batch entry starts aligned.  The host reads neither g_full nor g_step.
template <int V>
__global__ __launch_bounds__(RL2_THREADS) void rel_l2_steps_backward_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                            const float* __restrict__ sums, const float* __restrict__ g_full,
                                                                            const float* __restrict__ g_step, float* __restrict__ gx,
                                                                            long long P, int T, int W) {
    __shared__ float s_c[RL2_THREADS + 1];                      // cs[t] for t < T, cf at [T]
    const int tid = threadIdx.x;
    const long long b = blockIdx.x / (unsigned)W;
    const int w = (int)(blockIdx.x % (unsigned)W);
    if (tid < 64) {
        const float gs = g_step ? g_step[0] : 0.f;
        double num_b = 0.0, den_b = 0.0;
        for (int t = tid; t < T; t += 64) {
            const size_t o = (size_t)b * T + t;
            const float fn = sums[2 * o], fd = sums[2 * o + 1];
            s_c[t] = fn == 0.f ? 0.f : gs / (sqrtf(fn) * sqrtf(fd));
            num_b += (double)fn; den_b += (double)fd;
        }
        num_b = rl2_wave_sum(num_b);
        den_b = rl2_wave_sum(den_b);
        if (tid == 0) {
            const float fn = (float)num_b, fd = (float)den_b;
            s_c[T] = fn == 0.f ? 0.f : (g_full ? g_full[0] : 0.f) / (sqrtf(fn) * sqrtf(fd));
        }
    }
    __syncthreads();
    const float cf = s_c[T];
    const long long n = P * T;                                  // elements of a batch entry
    const size_t base = (size_t)b * (size_t)n;
    const long long stride = (long long)W * RL2_THREADS * V;
    long long e = ((long long)w * RL2_THREADS + tid) * V;
    int t = (int)(e % T);
    const int dt = (int)(stride % T);
    if (V == 4) {
        for (; e < n; e += stride) {                            // n % 4 == 0: a whole group of four or nothing
            const float4 x = *reinterpret_cast<const float4*>(pred + base + e);
            const float4 y = *reinterpret_cast<const float4*>(target + base + e);
            *reinterpret_cast<float4*>(gx + base + e) = make_float4((x.x - y.x) * (cf + s_c[t]), (x.y - y.y) * (cf + s_c[t + 1]),
                                                                    (x.z - y.z) * (cf + s_c[t + 2]), (x.w - y.w) * (cf + s_c[t + 3]));
            t += dt;
            if (t >= T) t -= T;
        }
    } else {
        for (; e < n; e += stride) {
            gx[base + e] = (pred[base + e] - target[base + e]) * (cf + s_c[t]);
            t += dt;
            if (t >= T) t -= T;
        }
    }
}

static bool rl2_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int launch_rel_l2_steps_backward(const float* pred, const float* target, const float* sums, const float* g_full, const float* g_step, float* gx,
                                 int B, long long P, int T, hipStream_t s) {
    const bool wide = T % 4 == 0 && rl2_aligned16(pred) && rl2_aligned16(target) && rl2_aligned16(gx);
    const long long per_wg = (long long)RL2_THREADS * (wide ? 4 : 1);
    const long long n = P * T;
    // workgroups per batch entry: eight per usable CU over the whole launch, never more than the entry has work for
    long long W = ((long long)current_usable_cus() * 8 + B - 1) / B;
    const long long most = (n + per_wg - 1) / per_wg;
    if (W > most) W = most;
    if (W < 1) W = 1;
    if (W * B > 0x7fffffffLL) { set_error("rel_l2_steps_backward: %lld workgroups x %d batch entries exceed the grid limit", W, B); return -2; }
    {
        ProfScope prof("uno::rel_l2_steps_backward_kernel", 12.0 * B * (double)P * T, s);
        if (wide)
            hipLaunchKernelGGL(rel_l2_steps_backward_kernel<4>, dim3((unsigned)(W * B)), dim3(RL2_THREADS), 0, s, pred, target, sums, g_full, g_step,
                               gx, P, T, (int)W);
        else
            hipLaunchKernelGGL(rel_l2_steps_backward_kernel<1>, dim3((unsigned)(W * B)), dim3(RL2_THREADS), 0, s, pred, target, sums, g_full, g_step,
                               gx, P, T, (int)W);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("rel_l2_steps_backward launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

}  // namespace uno
