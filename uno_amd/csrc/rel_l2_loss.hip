// K20 - the relative L2 training loss of the reference (utilities3.py:86-100, `LpLoss(...)(x.view(B, -1), y.view(B, -1))`), forward and
// backward, for x, y seen as (B, N):
//
//   sums[b]   = [ sum_e (x[b][e] - y[b][e])^2,  sum_e y[b][e]^2 ]
//   ratio[b]  = sqrt(num_b) / sqrt(den_b)
//   total     = sum_b ratio[b]
//   gx[b][e]  = g[b] * scale * (x[b][e] - y[b][e]) / (sqrt(num_b) * sqrt(den_b)),   0 where num_b == 0
//
// Stock ops spend about six small launches forward and eight backward on it, 40 times per NS-2D roll-out.  Here: one streaming launch
// over (chunk, batch entry) and one one-workgroup finish launch forward, one launch backward.  K17 (rel_l2_steps.hip) and K18 / K19-B
// (rollout.hip, rollout_train.hip) are forward-only or tied to the roll-out state; this one takes what the training scripts pass:
// every operand has a row stride and an element stride in elements, because ns_train_3d.py:58-61 calls the loss on
// `out[..., t].view(B, -1)`, whose element stride is T_f.
//
// No atomics.  The chunk decomposition is a function of N alone (never of the CU count or uno_reserve_cus) and every sum runs in a fixed
// order (thread-strided walk, xor-shuffle wave sums, waves in ascending order, chunk partials in ascending order in double, rounded
// once), so two calls - or a call and a graph replay - give the same bits.  No clamping: a zero target row gives +inf (NaN for 0 / 0) as
// torch.norm(.) / torch.norm(.) does; num_b == 0 gives a zero gradient, the rule of torch.linalg.vector_norm's backward.
//
// Loads are 16 bytes per lane where both element strides are 1 and every row of both operands starts 16-byte aligned (the host decides:
// an aligned base and, for B > 1, row strides that are multiples of 4), 4 bytes per lane otherwise.  Chunk lengths are multiples of 4, so
// a chunk starts aligned where its row does; the up to three elements past the last whole group of four are read one by one.
#include <cstdint>
#include "uno_common.h"

namespace uno {

enum { RLL_THREADS = 256, RLL_CHUNK = 4096, RLL_MAX_CHUNKS = 64 };

// elements per chunk (a multiple of 4) and the chunk count: RLL_CHUNK elements per chunk, larger chunks once that would give more than
// RLL_MAX_CHUNKS of them (the finish kernel reads every partial of a row in one thread)
long long rel_l2_chunks(long long N, long long* chunk_elems) {
    long long ce = RLL_CHUNK;
    const long long per = (N + RLL_MAX_CHUNKS - 1) / RLL_MAX_CHUNKS;
    if (per > ce) ce = (per + 3) / 4 * 4;
    if (chunk_elems) *chunk_elems = ce;
    return (N + ce - 1) / ce;
}

// an upper bound of the chunk count that never shrinks as N grows (the workspace size); the chunk count itself while that is below the cap
long long rel_l2_ws_floats(int B, long long N) {
    long long nc = (N + RLL_CHUNK - 1) / RLL_CHUNK;
    if (nc > RLL_MAX_CHUNKS) nc = RLL_MAX_CHUNKS;
    return 2LL * B * nc;
}

__device__ __forceinline__ float rll_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);      // a + b = b + a: every lane ends with the same bits
    return v;
}

__device__ __forceinline__ double rll_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ void rll_acc(float xv, float yv, float& num, float& den) {
    const float d = xv - yv;
    num += d * d; den += yv * yv;
}

__device__ __forceinline__ void rll_acc(const float4& xv, const float4& yv, float& num, float& den) {
    rll_acc(xv.x, yv.x, num, den);
    rll_acc(xv.y, yv.y, num, den);
    rll_acc(xv.z, yv.z, num, den);
    rll_acc(xv.w, yv.w, num, den);
}

// grid: NC * B workgroups, workgroup g = b * NC + c owns elements [c * CE, min((c + 1) * CE, N)) of row b; ws[b][c] = (num, den) of it.
// V = 4: both element strides are 1 and every row starts 16-byte aligned (xes, yes are not read).
template <int V>
__global__ __launch_bounds__(RLL_THREADS) void rel_l2_partial_kernel(const float* __restrict__ x, long long xrs, long long xes,
                                                                     const float* __restrict__ y, long long yrs, long long yes,
                                                                     float2* __restrict__ ws, long long N, long long CE, int NC) {
    __shared__ float s_num[RLL_THREADS / 64];
    __shared__ float s_den[RLL_THREADS / 64];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x / (unsigned)NC;
    const int c = (int)(blockIdx.x % (unsigned)NC);
    const long long e0 = (long long)c * CE;
    const long long e1 = e0 + CE < N ? e0 + CE : N;
    const long long n = e1 - e0;                                // elements of this chunk, >= 1
    float num = 0.f, den = 0.f;
    if (V == 4) {
        const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + b * xrs + e0);
        const float4* __restrict__ yv = reinterpret_cast<const float4*>(y + b * yrs + e0);
        const long long n4 = n >> 2;                            // whole groups of four
        long long q = tid;
        for (; q + 3LL * RLL_THREADS < n4; q += 4LL * RLL_THREADS) {        // four independent loads of each tensor in flight
            const float4 x0 = xv[q], x1 = xv[q + RLL_THREADS], x2 = xv[q + 2 * RLL_THREADS], x3 = xv[q + 3 * RLL_THREADS];
            const float4 y0 = yv[q], y1 = yv[q + RLL_THREADS], y2 = yv[q + 2 * RLL_THREADS], y3 = yv[q + 3 * RLL_THREADS];
            rll_acc(x0, y0, num, den);
            rll_acc(x1, y1, num, den);
            rll_acc(x2, y2, num, den);
            rll_acc(x3, y3, num, den);
        }
        for (; q < n4; q += RLL_THREADS) rll_acc(xv[q], yv[q], num, den);
        const long long e = e0 + 4 * n4 + tid;                  // the row's last 1 ... 3 elements (the last chunk only)
        if (e < e1) rll_acc(x[b * xrs + e], y[b * yrs + e], num, den);
    } else {
        const float* __restrict__ xr = x + b * xrs + e0 * xes;
        const float* __restrict__ yr = y + b * yrs + e0 * yes;
        long long e = tid;
        for (; e + 3LL * RLL_THREADS < n; e += 4LL * RLL_THREADS) {         // four independent loads of each tensor in flight
            const float x0 = xr[e * xes], x1 = xr[(e + RLL_THREADS) * xes], x2 = xr[(e + 2 * RLL_THREADS) * xes], x3 = xr[(e + 3 * RLL_THREADS) * xes];
            const float y0 = yr[e * yes], y1 = yr[(e + RLL_THREADS) * yes], y2 = yr[(e + 2 * RLL_THREADS) * yes], y3 = yr[(e + 3 * RLL_THREADS) * yes];
            rll_acc(x0, y0, num, den);
            rll_acc(x1, y1, num, den);
            rll_acc(x2, y2, num, den);
            rll_acc(x3, y3, num, den);
        }
        for (; e < n; e += RLL_THREADS) rll_acc(xr[e * xes], yr[e * yes], num, den);
    }
    num = rll_wave_sum(num);
    den = rll_wave_sum(den);
    if ((tid & 63) == 0) { s_num[tid >> 6] = num; s_den[tid >> 6] = den; }
    __syncthreads();
    if (tid == 0) {
        float a = 0.f, d = 0.f;
#pragma unroll
        for (int w = 0; w < RLL_THREADS / 64; ++w) { a += s_num[w]; d += s_den[w]; }
        ws[(size_t)b * NC + c] = make_float2(a, d);
    }
}

// one workgroup: a thread per row sums the row's chunk partials in ascending order in double and rounds once; total = sum_b ratio[b] in
// double (rows in ascending order per thread, xor-shuffle wave sums, waves in ascending order), rounded once
__global__ __launch_bounds__(RLL_THREADS) void rel_l2_finish_kernel(const float2* __restrict__ ws, float* __restrict__ sums,
                                                                    float* __restrict__ ratio, float* __restrict__ total, int B, int NC) {
    __shared__ double s_tot[RLL_THREADS / 64];
    const int tid = threadIdx.x;
    double t = 0.0;
    for (long long b = tid; b < B; b += RLL_THREADS) {
        const float2* p = ws + (size_t)b * NC;
        double dn = 0.0, dd = 0.0;
        for (int c = 0; c < NC; ++c) { dn += (double)p[c].x; dd += (double)p[c].y; }
        const float fn = (float)dn, fd = (float)dd;
        sums[2 * b] = fn;
        sums[2 * b + 1] = fd;
        const float r = sqrtf(fn) / sqrtf(fd);
        ratio[b] = r;
        t += (double)r;
    }
    t = rll_wave_sum(t);
    if ((tid & 63) == 0) s_tot[tid >> 6] = t;
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < RLL_THREADS / 64; ++w) a += s_tot[w];
        total[0] = (float)a;
    }
}

// grid: NC * B workgroups as the partial kernel's; gx is dense (B, N).  V = 4: as above, and N % 4 == 0 or B == 1 with gx 16-byte aligned
// (every row of gx starts aligned).  g[b] (per_row) or g[0]; no host read.
template <int V>
__global__ __launch_bounds__(RLL_THREADS) void rel_l2_backward_kernel(const float* __restrict__ x, long long xrs, long long xes,
                                                                      const float* __restrict__ y, long long yrs, long long yes,
                                                                      const float* __restrict__ sums, const float* __restrict__ g, int per_row,
                                                                      float scale, float* __restrict__ gx, long long N, long long CE, int NC) {
    const int tid = threadIdx.x;
    const long long b = blockIdx.x / (unsigned)NC;
    const int c = (int)(blockIdx.x % (unsigned)NC);
    const long long e0 = (long long)c * CE;
    const long long e1 = e0 + CE < N ? e0 + CE : N;
    const long long n = e1 - e0;
    const float num = sums[2 * b], den = sums[2 * b + 1];
    const float k = num == 0.f ? 0.f : g[per_row ? b : 0] * scale / (sqrtf(num) * sqrtf(den));
    float* __restrict__ o = gx + b * N + e0;
    if (V == 4) {
        const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + b * xrs + e0);
        const float4* __restrict__ yv = reinterpret_cast<const float4*>(y + b * yrs + e0);
        float4* __restrict__ ov = reinterpret_cast<float4*>(o);
        const long long n4 = n >> 2;
        long long q = tid;
        for (; q + 3LL * RLL_THREADS < n4; q += 4LL * RLL_THREADS) {
            const float4 x0 = xv[q], x1 = xv[q + RLL_THREADS], x2 = xv[q + 2 * RLL_THREADS], x3 = xv[q + 3 * RLL_THREADS];
            const float4 y0 = yv[q], y1 = yv[q + RLL_THREADS], y2 = yv[q + 2 * RLL_THREADS], y3 = yv[q + 3 * RLL_THREADS];
            ov[q] = make_float4(k * (x0.x - y0.x), k * (x0.y - y0.y), k * (x0.z - y0.z), k * (x0.w - y0.w));
            ov[q + RLL_THREADS] = make_float4(k * (x1.x - y1.x), k * (x1.y - y1.y), k * (x1.z - y1.z), k * (x1.w - y1.w));
            ov[q + 2 * RLL_THREADS] = make_float4(k * (x2.x - y2.x), k * (x2.y - y2.y), k * (x2.z - y2.z), k * (x2.w - y2.w));
            ov[q + 3 * RLL_THREADS] = make_float4(k * (x3.x - y3.x), k * (x3.y - y3.y), k * (x3.z - y3.z), k * (x3.w - y3.w));
        }
        for (; q < n4; q += RLL_THREADS) {
            const float4 xq = xv[q], yq = yv[q];
            ov[q] = make_float4(k * (xq.x - yq.x), k * (xq.y - yq.y), k * (xq.z - yq.z), k * (xq.w - yq.w));
        }
        const long long t = 4 * n4 + tid;                       // the row's last 1 ... 3 elements (B == 1 only)
        if (t < n) o[t] = k * (x[b * xrs + e0 + t] - y[b * yrs + e0 + t]);
    } else {
        const float* __restrict__ xr = x + b * xrs + e0 * xes;
        const float* __restrict__ yr = y + b * yrs + e0 * yes;
        long long e = tid;
        for (; e + 3LL * RLL_THREADS < n; e += 4LL * RLL_THREADS) {
            const float x0 = xr[e * xes], x1 = xr[(e + RLL_THREADS) * xes], x2 = xr[(e + 2 * RLL_THREADS) * xes], x3 = xr[(e + 3 * RLL_THREADS) * xes];
            const float y0 = yr[e * yes], y1 = yr[(e + RLL_THREADS) * yes], y2 = yr[(e + 2 * RLL_THREADS) * yes], y3 = yr[(e + 3 * RLL_THREADS) * yes];
            o[e] = k * (x0 - y0);
            o[e + RLL_THREADS] = k * (x1 - y1);
            o[e + 2 * RLL_THREADS] = k * (x2 - y2);
            o[e + 3 * RLL_THREADS] = k * (x3 - y3);
        }
        for (; e < n; e += RLL_THREADS) o[e] = k * (xr[e * xes] - yr[e * yes]);
    }
}

static bool rll_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// every row of both operands starts 16-byte aligned and is dense
static bool rll_wide_loads(const float* x, long long xrs, long long xes, const float* y, long long yrs, long long yes, int B) {
    return xes == 1 && yes == 1 && rll_aligned16(x) && rll_aligned16(y) && (B == 1 || (xrs % 4 == 0 && yrs % 4 == 0));
}

int launch_rel_l2_forward(const float* x, long long xrs, long long xes, const float* y, long long yrs, long long yes, float* sums, float* ratio,
                          float* total, float* ws, int B, long long N, hipStream_t s) {
    long long ce = 0;
    const long long nc = rel_l2_chunks(N, &ce);
    if (nc * B > 0x7fffffffLL) { set_error("rel_l2_forward: %lld chunks x %d rows exceed the grid limit", nc, B); return -2; }
    {
        ProfScope prof("uno::rel_l2_partial_kernel", 8.0 * B * (double)N, s);
        if (rll_wide_loads(x, xrs, xes, y, yrs, yes, B))
            hipLaunchKernelGGL(rel_l2_partial_kernel<4>, dim3((unsigned)(nc * B)), dim3(RLL_THREADS), 0, s, x, xrs, xes, y, yrs, yes, (float2*)ws, N, ce,
                               (int)nc);
        else
            hipLaunchKernelGGL(rel_l2_partial_kernel<1>, dim3((unsigned)(nc * B)), dim3(RLL_THREADS), 0, s, x, xrs, xes, y, yrs, yes, (float2*)ws, N, ce,
                               (int)nc);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("rel_l2_forward partial launch: %s", hipGetErrorString(e)); return -5; }
    {
        ProfScope prof("uno::rel_l2_finish_kernel", 8.0 * B * (double)nc, s);
        hipLaunchKernelGGL(rel_l2_finish_kernel, dim3(1), dim3(RLL_THREADS), 0, s, (const float2*)ws, sums, ratio, total, B, (int)nc);
    }
    e = hipGetLastError();
    if (e != hipSuccess) { set_error("rel_l2_forward finish launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

int launch_rel_l2_backward(const float* x, long long xrs, long long xes, const float* y, long long yrs, long long yes, const float* sums,
                           const float* g, int per_row, float scale, float* gx, int B, long long N, hipStream_t s) {
    long long ce = 0;
    const long long nc = rel_l2_chunks(N, &ce);
    if (nc * B > 0x7fffffffLL) { set_error("rel_l2_backward: %lld chunks x %d rows exceed the grid limit", nc, B); return -2; }
    {
        ProfScope prof("uno::rel_l2_backward_kernel", 12.0 * B * (double)N, s);
        if (rll_wide_loads(x, xrs, xes, y, yrs, yes, B) && rll_aligned16(gx) && (B == 1 || N % 4 == 0))
            hipLaunchKernelGGL(rel_l2_backward_kernel<4>, dim3((unsigned)(nc * B)), dim3(RLL_THREADS), 0, s, x, xrs, xes, y, yrs, yes, sums, g, per_row,
                               scale, gx, N, ce, (int)nc);
        else
            hipLaunchKernelGGL(rel_l2_backward_kernel<1>, dim3((unsigned)(nc * B)), dim3(RLL_THREADS), 0, s, x, xrs, xes, y, yrs, yes, sums, g, per_row,
                               scale, gx, N, ce, (int)nc);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("rel_l2_backward launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

}  // namespace uno
