// K18 - everything the NS-2D evaluation roll-out does between two forward passes, in one launch per roll-out step t:
//
//   ws[b][c][t]       = [ sum_{p in chunk c} (frame[b][p] - target[b][t][p])^2,  sum_{p in chunk c} target[b][t][p]^2 ]
//   pred[b][t][p]     = frame[b][p]                                   (if pred is given)
//   window[b][k][p]   = window[b][k + 1][p]  for k < T_in - 1,  window[b][T_in - 1][p] = frame[b][p]      (if shift)
//
// Without ground truth (target and ws both null: a free-running roll-out, harness.predict) the same pass runs with no sums - the second
// and third line only.  T is then nothing but pred's time length (the 256-step cap belongs to the finish kernel's workspace).
//
// The reference's loops (ns_train_2d.py:94-107, 141-157) spend per step one `cat` for the window, a strided slice of the target, six
// launches of LpLoss and a `cat` that rebuilds the whole prediction.  Here the window (B, C, P) is channels-first and moves IN PLACE:
// its first T_in channels are the frames, the other C - T_in the model's positional features, which are never touched.  target and
// pred are time-major (B, T, P), so every step reads and writes one dense slice.  ws has K17's layout (float2 [b][chunk][t]): after the
// last step K17's finish kernel turns it into sums / rel / totals (rel_l2_steps.hip), and the whole-trajectory error
// sqrt(sum_t num) / sqrt(sum_t den) comes out without the prediction ever being assembled.
//
// No races in the shift: one thread owns a pixel (or four) and moves that pixel's whole column of T_in frames in ascending k - it reads
// window[k + 1] before it writes window[k], and no address is written by one thread and read by another: no second buffer, no
// grid-wide ordering.  No atomics.  The chunk decomposition is a function of P alone (never of the CU count or uno_reserve_cus) and
// the summation order inside a chunk is fixed (thread-strided walk, xor-shuffle wave sums, waves in ascending order), so two calls - or
// a call and a graph replay - give the same bits.  No clamping: a zero target slice gives +inf / NaN in the finish kernel as
// torch.norm(.) / torch.norm(.) does.
//
// Loads and stores are 16 bytes per lane where P % 4 == 0 (every batch entry, channel and chunk then starts 16-byte aligned when the
// tensors do: chunk lengths are multiples of 4), 4 bytes per lane otherwise.
#include "uno_common.h"

namespace uno {

enum { RO_THREADS = 256, RO_CHUNK_PIXELS = 1024, RO_MAX_CHUNKS = 64 };

// pixels per chunk (a multiple of 4) and the chunk count: RO_CHUNK_PIXELS pixels per chunk, larger chunks once that would give more than
// RO_MAX_CHUNKS of them (the finish kernel reads every partial in one workgroup)
long long rollout_chunks(long long P, long long* chunk_pixels) {
    long long cp = RO_CHUNK_PIXELS;
    const long long per = (P + RO_MAX_CHUNKS - 1) / RO_MAX_CHUNKS;
    if (per > cp) cp = (per + 3) / 4 * 4;
    if (chunk_pixels) *chunk_pixels = cp;
    return (P + cp - 1) / cp;
}

// an upper bound of the chunk count that never shrinks as P grows (the workspace size); the chunk count itself while that is below the cap
long long rollout_ws_floats(int B, long long P, int T) {
    long long nc = (P + RO_CHUNK_PIXELS - 1) / RO_CHUNK_PIXELS;
    if (nc > RO_MAX_CHUNKS) nc = RO_MAX_CHUNKS;
    return 2LL * B * nc * T;
}

template <int V> struct RoVec;
template <> struct RoVec<1> {
    typedef float type;
    static __device__ __forceinline__ float ld(const float* p) { return *p; }
    static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
    static __device__ __forceinline__ void acc(float f, float y, float& num, float& den) { const float d = f - y; num += d * d; den += y * y; }
};
template <> struct RoVec<4> {           // 16 bytes per lane at 4-byte alignment (f4u): a caller's base pointer need not be 16-byte aligned
    typedef float4 type;
    static __device__ __forceinline__ float4 ld(const float* p) { return io_ld4(p); }
    static __device__ __forceinline__ void st(float* p, const float4& v) { io_store4(p, v.x, v.y, v.z, v.w); }
    static __device__ __forceinline__ void acc(const float4& f, const float4& y, float& num, float& den) {
        const float d0 = f.x - y.x, d1 = f.y - y.y, d2 = f.z - y.z, d3 = f.w - y.w;
        num += d0 * d0; den += y.x * y.x;
        num += d1 * d1; den += y.y * y.y;
        num += d2 * d2; den += y.z * y.z;
        num += d3 * d3; den += y.w * y.w;
    }
};

__device__ __forceinline__ float ro_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);      // a + b = b + a: every lane ends with the same bits
    return v;
}

// grid: NC * B workgroups, workgroup g = b * NC + c owns pixels [c * CP, min((c + 1) * CP, P)) of batch entry b.  V = 4 needs P % 4 == 0
// (CP is a multiple of 4 always).  window is read and written through one pointer on purpose: a thread's loads of frame k + 1 precede
// its store of frame k in program order.  SUMS = false: no target, no ws - neither is read or written, nothing is reduced.
template <int V, bool SUMS>
__global__ __launch_bounds__(RO_THREADS) void rollout_advance_kernel(float* window, const float* __restrict__ frame, const float* __restrict__ target,
                                                                     float* __restrict__ pred, float2* __restrict__ ws, long long P, int C,
                                                                     int T_in, int T, int t, int shift, long long CP, int NC) {
    typedef RoVec<V> R;
    typedef typename R::type vec;
    __shared__ float s_num[RO_THREADS / 64];
    __shared__ float s_den[RO_THREADS / 64];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x / (unsigned)NC;
    const int c = (int)(blockIdx.x % (unsigned)NC);
    const long long p0 = (long long)c * CP;
    const long long p1 = p0 + CP < P ? p0 + CP : P;
    const size_t sP = (size_t)P;
    const float* __restrict__ fr = frame + b * sP;
    const float* __restrict__ tg = SUMS ? target + (b * (size_t)T + (size_t)t) * sP : nullptr;
    float* __restrict__ pr = pred ? pred + (b * (size_t)T + (size_t)t) * sP : nullptr;
    float* wn = window + b * (size_t)C * sP;
    float num = 0.f, den = 0.f;
    for (long long p = p0 + (long long)tid * V; p < p1; p += (long long)RO_THREADS * V) {
        const vec f = R::ld(fr + p);
        if (SUMS) {
            const vec y = R::ld(tg + p);
            R::acc(f, y, num, den);
        }
        if (pr) R::st(pr + p, f);
        if (shift) {
            float* col = wn + p;
            int k = 0;
            for (; k + 4 < T_in; k += 4) {                              // four frames in flight: all four loads precede the four stores
                const vec a0 = R::ld(col + (size_t)(k + 1) * sP);
                const vec a1 = R::ld(col + (size_t)(k + 2) * sP);
                const vec a2 = R::ld(col + (size_t)(k + 3) * sP);
                const vec a3 = R::ld(col + (size_t)(k + 4) * sP);
                R::st(col + (size_t)k * sP, a0);
                R::st(col + (size_t)(k + 1) * sP, a1);
                R::st(col + (size_t)(k + 2) * sP, a2);
                R::st(col + (size_t)(k + 3) * sP, a3);
            }
            for (; k + 1 < T_in; ++k) {
                const vec a = R::ld(col + (size_t)(k + 1) * sP);
                R::st(col + (size_t)k * sP, a);
            }
            R::st(col + (size_t)(T_in - 1) * sP, f);
        }
    }
    if (!SUMS) return;
    num = ro_wave_sum(num);
    den = ro_wave_sum(den);
    if ((tid & 63) == 0) { s_num[tid >> 6] = num; s_den[tid >> 6] = den; }
    __syncthreads();
    if (tid == 0) {
        float a = 0.f, d = 0.f;
#pragma unroll
        for (int w = 0; w < RO_THREADS / 64; ++w) { a += s_num[w]; d += s_den[w]; }
        ws[(b * (size_t)NC + (size_t)c) * (size_t)T + (size_t)t] = make_float2(a, d);
    }
}

int launch_rollout_advance(float* window, const float* frame, const float* target, float* pred, float* ws, int B, int C, int T_in, long long P,
                           int T, int t, int shift, hipStream_t s) {
    long long cp = 0;
    const long long nc = rollout_chunks(P, &cp);
    if (nc * B > 0x7fffffffLL) { set_error("rollout_advance: %lld chunks x %d batch entries exceed the grid limit", nc, B); return -2; }
    {
        // frame read (+ target read where there is one), pred written, the shift's T_in - 1 reads and T_in writes
        const double moved = 4.0 * B * (double)P * (1 + (target ? 1 : 0) + (pred ? 1 : 0) + (shift ? 2.0 * T_in - 1 : 0));
        ProfScope prof("uno::rollout_advance_kernel", moved, s);
#define UNO_RO_LAUNCH(V, SUMS)                                                                                                                  \
        hipLaunchKernelGGL((rollout_advance_kernel<V, SUMS>), dim3((unsigned)(nc * B)), dim3(RO_THREADS), 0, s, window, frame, target, pred,      \
                           (float2*)ws, P, C, T_in, T, t, shift, cp, (int)nc)
        if (target) { if (P % 4 == 0) UNO_RO_LAUNCH(4, true); else UNO_RO_LAUNCH(1, true); }
        else        { if (P % 4 == 0) UNO_RO_LAUNCH(4, false); else UNO_RO_LAUNCH(1, false); }
#undef UNO_RO_LAUNCH
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("rollout_advance launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

}  // namespace uno
