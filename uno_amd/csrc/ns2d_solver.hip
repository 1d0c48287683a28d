// K22: the 2-D Navier-Stokes pseudo-spectral solver of the reference's data generator (ns_datagen.py:15-140), vorticity form, Crank-Nicolson
// in time.  C ABI: uno_ns2d_forward, uno_ns2d_inverse, uno_ns2d_steps (capi_ns2d.hip).
//
// State: the half spectrum w_h (B, N, h = N/2 + 1) c64, interleaved, un-normalised like fft2.  The reference keeps the full (N, N) spectrum
// and inverts it with irfft(onesided=False), which reads columns 0 ... N/2 only: the half spectrum is exactly equivalent.  N is a power of two,
// 32 ... 256; f32 throughout.  One time step is three launches - a step has three transposition points - through a caller-provided workspace
// of five (B, N, h) c64 planes:
//   K22-A  per (sample, 4 spectrum columns): psi = w_h / lap, kx psi, w_h, kx w_h formed in registers -> LDS; complex inverse DFT of
//          length N along axis 0 (MFMA) -> planes 0 ... 3.  The ky multipliers commute with this axis: K22-B applies them.
//   K22-B  per (sample, 8 rows): the four rows x (2 pi i ky | -+ 2 pi i) / N^2 -> LDS; half spectrum -> real along axis 1 (MFMA, Hermitian
//          weights 1, 2, ..., 2, 1 with the imaginary parts of columns 0 and N/2 ignored, as irfft2 does); q w_x + v w_y in registers -> LDS;
//          real -> half spectrum along axis 1 (MFMA) -> plane 4.  The four physical fields never reach memory.
//   K22-C  per (sample, 8 spectrum columns): forward DFT of length N along axis 0 (MFMA), dealias mask, Crank-Nicolson update of w_h in place.
// The end pieces are the same stages: forward = K22-B's second half on real rows + K22-C with a plain store; inverse = K22-A on w_h alone +
// K22-B's first half with a store of the real rows.
//
// Every sum is DENSE (length-N stages, not radix splits) on v_mfma_f32_16x16x4_f32 - exact f32, k-ordered - on interleaved (re, im)
// columns as ResampleWide::complex_stage of resample3d_wide.hip does, with the twiddle looked up in an LDS table at (a b) mod N.  The summation order
// is fixed and a sample's arithmetic does not depend on B: two runs, a split run and any batch give the same bits.  Stores are plain
// global stores (no buffer resource, no scalar offset: DESIGN.md section 4, K3v).  Every state / workspace offset is a 64-bit product.
// Workgroups are persistent.  h is odd at every N, so every column-blocked stage has a ragged last block; it is handled by bounds, not by size.
#include "resample3d_common.h"

namespace uno {

struct Ns2dParams {
    float2* w_h;                // (B, N, h) c64: the state (K22-A reads, K22-C updates in place; forward end piece: written)
    const float2* f_h;          // (N, h) or (B, N, h) c64: the forcing's half spectrum
    float2* ws;                 // 5 planes of (B, N, h) c64
    const float* w_in;          // forward end piece: (B, N, N) f32
    float* w_out;               // inverse end piece: (B, N, N) f32
    const float2* tw;           // (cos, sin)(2 pi n / N)
    int B, N, f_batched;
    float dt, half_dt_visc;     // delta_t, 0.5 delta_t visc
};

constexpr int NS_THREADS = 256;
constexpr int NS_WAVES = NS_THREADS / 64;
constexpr int NS_CBA = 4;       // spectrum columns per K22-A item (x 4 fields = 16 complex LDS columns)
constexpr int NS_CBC = 8;       // spectrum columns per K22-C item
constexpr int NS_RB = 8;        // rows per K22-B item (x 4 fields = 32 MFMA rows)
constexpr float NS_4PI2 = 39.47841760435743f, NS_2PI = 6.283185307179586f;

// row stride (in complex) of an LDS tile of Lp complex columns: the four rows one MFMA step reads land on disjoint banks
__host__ __device__ constexpr int ns_row_stride(int Lp) { return Lp == 8 ? 8 : Lp + 8; }
// the real-stage tiles: N + 4 floats per row (>= 2 h = N + 2 rounded up to a multiple of 4; 16 rows x 4 consecutive floats on 64 banks)
__host__ __device__ __forceinline__ int ns_real_stride(int N) { return N + 4; }

__device__ __forceinline__ int ns_wave_number(int idx, int N) { return idx < (N >> 1) ? idx : idx - N; }       // [0 ... N/2-1, -N/2 ... -1]
__device__ __forceinline__ int ns_half_wave_number(int col, int N) { return col < (N >> 1) ? col : -(N >> 1); } // columns 0 ... N/2: Nyquist = -N/2
__device__ __forceinline__ float ns_lap(int kx, int ky, bool dc) { return dc ? 1.0f : NS_4PI2 * (float)(kx * kx + ky * ky); }

// out[a][c] = sum_b in[b][c] e^{-+ 2 pi i a b / N} (INV: +), a, b < N; in: LDS, CT tiles of 8 complex columns, row stride LS.  A wave owns
// 16 output rows x (up to 2 tiles of) 16 real columns; lane (i, k) = (lane & 15, lane >> 4) supplies the twiddle of (row i, term k) and real
// column i of term k, and ends with rows 4 k ... 4 k + 3 of real column i: store(row, real column, value).
template <bool INV, int CT, class Store>
__device__ __forceinline__ void ns_axis0_stage(const float2* in, int N, const float2* tw, Store store) {
    constexpr int NT = CT >= 2 ? 2 : 1, CG = CT / NT, LS = ns_row_stride(CT * 8);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, k = lane >> 4;
    const int row_tiles = N >> 4, ksteps = N >> 2, mask = N - 1;
    const bool odd = i & 1;
    for (int item = wave; item < row_tiles * CG; item += NS_WAVES) {
        const int rt = item / CG, cg = item - rt * CG;
        const int a = rt * 16 + i;
        f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        int idx = (a * k) & mask;
        const int step = (4 * a) & mask;
        const float2* col = in + cg * (NT * 8) + (i >> 1) + (size_t)k * LS;
        for (int ks = 0; ks < ksteps; ++ks) {
            float2 t = tw[idx];
            if (!INV) t.y = -t.y;
            idx = (idx + step) & mask;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float2 v = col[(size_t)(4 * ks) * LS + nt * 8];
                acc[nt] = mfma16(t.x, odd ? v.y : v.x, acc[nt]);
                acc[nt] = mfma16(t.y, odd ? v.x : -v.y, acc[nt]);
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) store(rt * 16 + 4 * k + r, (cg * NT + nt) * 16 + i, acc[nt][r]);
        }
    }
}

// x[m][t] = sum_l c_l Re(U[m][l] e^{+2 pi i l t / N}), t < N: half spectrum -> real, as a real GEMM over kk = (l, re | im) < KP.  U: LDS, MR
// rows of US floats, interleaved, columns kk >= 2 h zero.  c = 1, 2, ..., 2, 1 and the imaginary parts of l = 0 and l = N/2 do not enter
// (irfft).  A wave owns 16 output columns t and all row tiles (they share the twiddle operand); lane (i, k) ends with rows 16 rt + 4 k + r
// of column t = 16 ct + i: emit(ct, acc).
template <int MR, class Emit>
__device__ __forceinline__ void ns_c2r_stage(const float* U, int N, const float2* tw, Emit emit) {
    constexpr int RT = (MR + 15) / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, k = lane >> 4;
    const int US = ns_real_stride(N), ksteps = US >> 2, mask = N - 1, half = N >> 1;
    for (int ct = wave; ct < (N >> 4); ct += NS_WAVES) {
        const int t = 16 * ct + i;
        f32x4 acc[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        int idx = ((k >> 1) * t) & mask;
        const int step = (2 * t) & mask;
        const float* row = U + k;
        for (int ks = 0; ks < ksteps; ++ks) {
            const int l = 2 * ks + (k >> 1);
            const float2 w = tw[idx];
            idx = (idx + step) & mask;
            const bool edge = l == 0 || l >= half;          // (l > N/2: the zero pad columns of U)
            const float bv = (k & 1) ? (edge ? 0.0f : -2.0f * w.y) : (edge ? w.x : 2.0f * w.x);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const float a = row[(size_t)min(16 * rt + i, MR - 1) * US + 4 * ks];
                acc[rt] = mfma16(a, bv, acc[rt]);
            }
        }
        emit(ct, acc);
    }
}

// F[m][c] = sum_t P[m][t] e^{-2 pi i (c >> 1) t / N} (re | im by c & 1), real columns c < 2 h: real -> half spectrum.  P: LDS, NS_RB rows of PS
// floats.  Lane (i, k) ends with rows 4 k + r of real column 16 ct + i: store(row, real column, value) for rows < NS_RB, columns < 2 h.
template <class Store>
__device__ __forceinline__ void ns_r2c_stage(const float* P, int N, const float2* tw, Store store) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, k = lane >> 4;
    const int PS = ns_real_stride(N), ksteps = N >> 2, mask = N - 1, cols = N + 2;
    const float* row = P + (size_t)min(i, NS_RB - 1) * PS + k;
    for (int ct = wave; ct < (cols + 15) >> 4; ct += NS_WAVES) {
        const int c = 16 * ct + i, l = c >> 1;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        int idx = (l * k) & mask;
        const int step = (4 * l) & mask;
        for (int ks = 0; ks < ksteps; ++ks) {
            const float2 w = tw[idx];
            idx = (idx + step) & mask;
            const float a = i < NS_RB ? row[4 * ks] : 0.0f;
            acc = mfma16(a, (c & 1) ? -w.y : w.x, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * k + r < NS_RB && c < cols) store(4 * k + r, c, acc[r]);
    }
}

// K22-A.  NF = 4: the four multiplied spectra of a step; NF = 1: w_h alone (inverse end piece).  LDS: in [N][LS] c64 | tw [N]
template <int NF>
__host__ __device__ __forceinline__ size_t ns_axis0_inv_lds(int N) { return (size_t)N * ns_row_stride(NF * NS_CBA >= 8 ? NF * NS_CBA : 8) * 8 + (size_t)N * 8; }

template <int NF>
__global__ __launch_bounds__(NS_THREADS) void ns2d_axis0_inv_kernel(Ns2dParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int Lp = NF * NS_CBA >= 8 ? NF * NS_CBA : 8, LS = ns_row_stride(Lp), CT = Lp / 8;
    const int N = p.N, h = (N >> 1) + 1;
    float2* sIn = reinterpret_cast<float2*>(smem);
    float2* tw = sIn + (size_t)N * LS;
    for (int n = threadIdx.x; n < N; n += NS_THREADS) tw[n] = p.tw[n];
    if (NF == 1)        // w_h alone fills 4 of the tile's 8 columns: the others are read (never stored from)
        for (int i = threadIdx.x; i < N * LS; i += NS_THREADS) sIn[i] = make_float2(0.f, 0.f);
    const int nblk = (h + NS_CBA - 1) / NS_CBA;
    const long long n_items = (long long)p.B * nblk;
    const size_t plane = (size_t)p.B * N * h;
    for (long long it = blockIdx.x; it < n_items; it += gridDim.x) {
        const long long s = it / nblk;
        const int c0 = (int)(it - s * nblk) * NS_CBA;
        __syncthreads();        // tables ready / the previous item's stage has read sIn
        const float2* src = p.w_h + (size_t)s * N * h;
        for (int e = threadIdx.x; e < N * NS_CBA; e += NS_THREADS) {
            const int b = e / NS_CBA, c = e - b * NS_CBA, col = c0 + c;
            const float2 w = col < h ? src[(size_t)b * h + col] : make_float2(0.f, 0.f);
            float2* dst = sIn + (size_t)b * LS + c;
            if (NF == 4) {
                const int kx = ns_wave_number(b, N), ky = ns_half_wave_number(min(col, h - 1), N);
                const float lap = ns_lap(kx, ky, b == 0 && col == 0), fkx = (float)kx;
                const float2 psi = make_float2(w.x / lap, w.y / lap);
                dst[0] = psi;
                dst[NS_CBA] = make_float2(fkx * psi.x, fkx * psi.y);
                dst[2 * NS_CBA] = w;
                dst[3 * NS_CBA] = make_float2(fkx * w.x, fkx * w.y);
            } else {
                dst[0] = w;
            }
        }
        __syncthreads();
        float* out = reinterpret_cast<float*>(p.ws) + ((size_t)s * N * h + c0) * 2;
        const int valid = 2 * min(NS_CBA, h - c0);
        ns_axis0_stage<true, CT>(sIn, N, tw, [&](int a, int rc, float v) {
            const int f = rc / (2 * NS_CBA), cc = rc - f * (2 * NS_CBA);
            if (f < NF && cc < valid) out[(size_t)f * plane * 2 + (size_t)a * h * 2 + cc] = v;
        });
    }
}

// K22-B.  MODE 0: a step (planes 0 ... 3 -> plane 4); 1: forward end piece (real rows of w_in -> plane 4); 2: inverse end piece (plane 0 ->
// real rows of w_out).  LDS: U [MR][N + 4] f32 | P [NS_RB][N + 4] f32 | tw [N]
__host__ __device__ __forceinline__ size_t ns_axis1_lds(int N, int mode) {
    const int MR = mode == 0 ? 4 * NS_RB : (mode == 2 ? NS_RB : 0), PR = mode == 2 ? 0 : NS_RB;
    return (size_t)(MR + PR) * ns_real_stride(N) * 4 + (size_t)N * 8;
}

template <int MODE>
__global__ __launch_bounds__(NS_THREADS) void ns2d_axis1_kernel(Ns2dParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int MR = MODE == 0 ? 4 * NS_RB : (MODE == 2 ? NS_RB : 0), PR = MODE == 2 ? 0 : NS_RB;
    const int N = p.N, h = (N >> 1) + 1, RS = ns_real_stride(N);
    float* sU = reinterpret_cast<float*>(smem);
    float* sP = sU + (size_t)MR * RS;
    float2* tw = reinterpret_cast<float2*>(sP + (size_t)PR * RS);
    for (int n = threadIdx.x; n < N; n += NS_THREADS) tw[n] = p.tw[n];
    for (int i = threadIdx.x; i < MR * RS; i += NS_THREADS) sU[i] = 0.0f;       // columns >= 2 h: read, never written again
    const int nblk = N / NS_RB;
    const long long n_items = (long long)p.B * nblk;
    const size_t plane = (size_t)p.B * N * h;
    const float inv = 1.0f / ((float)N * (float)N);
    const int lane_k = (threadIdx.x & 63) >> 4, lane_i = threadIdx.x & 15;
    for (long long it = blockIdx.x; it < n_items; it += gridDim.x) {
        const long long s = it / nblk;
        const int row0 = (int)(it - s * nblk) * NS_RB;
        const size_t base = ((size_t)s * N + row0) * h;         // first spectrum entry of the item's rows in a plane
        __syncthreads();        // tables ready / the previous item's stages have read sU and sP
        if constexpr (MODE == 0) {
            for (int e = threadIdx.x; e < NS_RB * h; e += NS_THREADS) {
                const int rl = e / h, l = e - rl * h;
                const float g1 = NS_2PI * inv, g = g1 * (float)ns_half_wave_number(l, N);
                const float2 z0 = p.ws[base + e], z1 = p.ws[plane + base + e], z2 = p.ws[2 * plane + base + e], z3 = p.ws[3 * plane + base + e];
                float* u = sU + (size_t)(4 * rl) * RS + 2 * l;
                *reinterpret_cast<float2*>(u) = make_float2(-g * z0.y, g * z0.x);               // q_h   =  2 pi i ky psi
                *reinterpret_cast<float2*>(u + RS) = make_float2(g1 * z1.y, -g1 * z1.x);        // v_h   = -2 pi i kx psi
                *reinterpret_cast<float2*>(u + 2 * RS) = make_float2(-g * z2.y, g * z2.x);      // w_y_h =  2 pi i ky w_h
                *reinterpret_cast<float2*>(u + 3 * RS) = make_float2(-g1 * z3.y, g1 * z3.x);    // w_x_h =  2 pi i kx w_h
            }
        } else if constexpr (MODE == 2) {
            for (int e = threadIdx.x; e < NS_RB * h; e += NS_THREADS) {
                const int rl = e / h, l = e - rl * h;
                const float2 z = p.ws[base + e];
                *reinterpret_cast<float2*>(sU + (size_t)rl * RS + 2 * l) = make_float2(inv * z.x, inv * z.y);
            }
        } else {
            const float* src = p.w_in + ((size_t)s * N + row0) * N;
            for (int e = threadIdx.x; e < NS_RB * N; e += NS_THREADS) {
                const int rl = e / N, t = e - rl * N;
                sP[(size_t)rl * RS + t] = src[e];
            }
        }
        __syncthreads();
        if constexpr (MODE == 0) {
            // MFMA row m = 4 rl + field: a lane's four results are q, v, w_y, w_x of row rl = 4 rt + k at column t
            ns_c2r_stage<MR>(sU, N, tw, [&](int ct, const f32x4* acc) {
#pragma unroll
                for (int rt = 0; rt < MR / 16; ++rt)
                    sP[(size_t)(4 * rt + lane_k) * RS + 16 * ct + lane_i] = acc[rt][0] * acc[rt][3] + acc[rt][1] * acc[rt][2];
            });
            __syncthreads();
        } else if constexpr (MODE == 2) {
            float* dst = p.w_out + ((size_t)s * N + row0) * N;
            ns_c2r_stage<MR>(sU, N, tw, [&](int ct, const f32x4* acc) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * lane_k + r < NS_RB) dst[(size_t)(4 * lane_k + r) * N + 16 * ct + lane_i] = acc[0][r];
            });
        }
        if constexpr (MODE != 2) {
            float* out = reinterpret_cast<float*>(p.ws + 4 * plane + base);
            ns_r2c_stage(sP, N, tw, [&](int rl, int c, float v) { out[(size_t)rl * h * 2 + c] = v; });
        }
    }
}

// K22-C.  MODE 0: dealias + Crank-Nicolson update of w_h in place; 1: plain store into w_h (forward end piece).  LDS: in [N][8] c64 | tw [N]
__host__ __device__ __forceinline__ size_t ns_axis0_fwd_lds(int N) { return (size_t)N * ns_row_stride(NS_CBC) * 8 + (size_t)N * 8; }

template <int MODE>
__global__ __launch_bounds__(NS_THREADS) void ns2d_axis0_fwd_kernel(Ns2dParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int LS = ns_row_stride(NS_CBC);
    const int N = p.N, h = (N >> 1) + 1;
    float2* sIn = reinterpret_cast<float2*>(smem);
    float2* tw = sIn + (size_t)N * LS;
    for (int n = threadIdx.x; n < N; n += NS_THREADS) tw[n] = p.tw[n];
    const int nblk = (h + NS_CBC - 1) / NS_CBC;
    const long long n_items = (long long)p.B * nblk;
    const size_t plane = (size_t)p.B * N * h;
    for (long long it = blockIdx.x; it < n_items; it += gridDim.x) {
        const long long s = it / nblk;
        const int c0 = (int)(it - s * nblk) * NS_CBC;
        __syncthreads();        // tables ready / the previous item's stage has read sIn
        const float2* src = p.ws + 4 * plane + (size_t)s * N * h;
        for (int e = threadIdx.x; e < N * NS_CBC; e += NS_THREADS) {
            const int b = e / NS_CBC, c = e - b * NS_CBC;
            sIn[(size_t)b * LS + c] = c0 + c < h ? src[(size_t)b * h + c0 + c] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        float* wf = reinterpret_cast<float*>(p.w_h);
        const float* ff = reinterpret_cast<const float*>(p.f_h);
        ns_axis0_stage<false, 1>(sIn, N, tw, [&](int a, int rc, float v) {
            const int col = c0 + (rc >> 1);
            if (col >= h) return;
            const size_t in_sample = ((size_t)a * h + col) * 2 + (rc & 1), o = (size_t)s * N * h * 2 + in_sample;
            if (MODE == 1) {
                wf[o] = v;
            } else {
                const int kx = ns_wave_number(a, N), ky = ns_half_wave_number(col, N);
                const bool keep = 3 * abs(kx) <= N && 3 * abs(ky) <= N;          // |k| <= (2/3) (N/2)
                const float cn = p.half_dt_visc * ns_lap(kx, ky, a == 0 && col == 0);
                const float F = keep ? v : 0.0f, f = ff[p.f_batched ? o : in_sample];
                wf[o] = (-p.dt * F + p.dt * f + (1.0f - cn) * wf[o]) / (1.0f + cn);
            }
        });
    }
}

long long ns2d_ws_bytes(int B, int N) { return 5LL * 8 * B * N * (N / 2 + 1); }

static bool ns2d_prepare(Ns2dParams& p, int B, int N, void* ws) {
    p.B = B; p.N = N; p.ws = static_cast<float2*>(ws);
    p.w_h = nullptr; p.f_h = nullptr; p.w_in = nullptr; p.w_out = nullptr; p.f_batched = 0; p.dt = 0.f; p.half_dt_visc = 0.f;
    p.tw = twiddle_table(N);
    return p.tw != nullptr;     // (every kernel's LDS stays below the 64 KB a launch may ask for without opting in: 51 KB in K22-A at N = 256)
}

static dim3 ns_grid_cols(int B, int N, int cb, size_t lds) { return dim3(ra_grid((long long)B * ((N / 2 + 1 + cb - 1) / cb), lds)); }
static dim3 ns_grid_rows(int B, int N, size_t lds) { return dim3(ra_grid((long long)B * (N / NS_RB), lds)); }

// ns_datagen.py:35-42 (w_h = rfft of the initial vorticity), on the half spectrum
int launch_ns2d_forward(const float* w, float* w_h, void* ws, int B, int N, hipStream_t s) {
    Ns2dParams p;
    if (!ns2d_prepare(p, B, N, ws)) return -6;
    p.w_in = w; p.w_h = reinterpret_cast<float2*>(w_h);
    const double half = 8.0 * B * (double)N * (N / 2 + 1);
    {
        ProfScope prof("uno::ns2d_axis1_kernel<fwd>", 4.0 * B * (double)N * N + half, s);
        hipLaunchKernelGGL(ns2d_axis1_kernel<1>, ns_grid_rows(B, N, ns_axis1_lds(N, 1)), dim3(NS_THREADS), ns_axis1_lds(N, 1), s, p);
    }
    if (int rc = ra_check("ns2d_axis1<fwd>")) return rc;
    {
        ProfScope prof("uno::ns2d_axis0_fwd_kernel<store>", 2.0 * half, s);
        hipLaunchKernelGGL(ns2d_axis0_fwd_kernel<1>, ns_grid_cols(B, N, NS_CBC, ns_axis0_fwd_lds(N)), dim3(NS_THREADS), ns_axis0_fwd_lds(N), s, p);
    }
    return ra_check("ns2d_axis0_fwd<store>");
}

// ns_datagen.py:121-122 (w = irfft(w_h) of a recorded snapshot)
int launch_ns2d_inverse(const float* w_h, float* w, void* ws, int B, int N, hipStream_t s) {
    Ns2dParams p;
    if (!ns2d_prepare(p, B, N, ws)) return -6;
    p.w_h = reinterpret_cast<float2*>(const_cast<float*>(w_h)); p.w_out = w;         // (K22-A only reads w_h)
    const double half = 8.0 * B * (double)N * (N / 2 + 1);
    {
        ProfScope prof("uno::ns2d_axis0_inv_kernel<1>", 2.0 * half, s);
        hipLaunchKernelGGL(ns2d_axis0_inv_kernel<1>, ns_grid_cols(B, N, NS_CBA, ns_axis0_inv_lds<1>(N)), dim3(NS_THREADS), ns_axis0_inv_lds<1>(N), s, p);
    }
    if (int rc = ra_check("ns2d_axis0_inv<1>")) return rc;
    {
        ProfScope prof("uno::ns2d_axis1_kernel<inv>", 4.0 * B * (double)N * N + half, s);
        hipLaunchKernelGGL(ns2d_axis1_kernel<2>, ns_grid_rows(B, N, ns_axis1_lds(N, 2)), dim3(NS_THREADS), ns_axis1_lds(N, 2), s, p);
    }
    return ra_check("ns2d_axis1<inv>");
}

// ns_datagen.py:70-119: n_steps Crank-Nicolson steps, three launches each, one loop
int launch_ns2d_steps(float* w_h, const float* f_h, int f_batched, void* ws, int B, int N, long long n_steps, double visc, double delta_t,
                      hipStream_t s) {
    Ns2dParams p;
    if (!ns2d_prepare(p, B, N, ws)) return -6;
    p.w_h = reinterpret_cast<float2*>(w_h); p.f_h = reinterpret_cast<const float2*>(f_h); p.f_batched = f_batched ? 1 : 0;
    p.dt = (float)delta_t; p.half_dt_visc = (float)(0.5 * delta_t * visc);
    const size_t lds_a = ns_axis0_inv_lds<4>(N), lds_b = ns_axis1_lds(N, 0), lds_c = ns_axis0_fwd_lds(N);
    const dim3 grid_a = ns_grid_cols(B, N, NS_CBA, lds_a), grid_b = ns_grid_rows(B, N, lds_b), grid_c = ns_grid_cols(B, N, NS_CBC, lds_c);
    const double half = 8.0 * B * (double)N * (N / 2 + 1);
    for (long long step = 0; step < n_steps; ++step) {
        {
            ProfScope prof("uno::ns2d_axis0_inv_kernel<4>", 5.0 * half, s);
            hipLaunchKernelGGL(ns2d_axis0_inv_kernel<4>, grid_a, dim3(NS_THREADS), lds_a, s, p);
        }
        {
            ProfScope prof("uno::ns2d_axis1_kernel<step>", 5.0 * half, s);
            hipLaunchKernelGGL(ns2d_axis1_kernel<0>, grid_b, dim3(NS_THREADS), lds_b, s, p);
        }
        {
            ProfScope prof("uno::ns2d_axis0_fwd_kernel<update>", (f_batched ? 4.0 : 3.0) * half, s);
            hipLaunchKernelGGL(ns2d_axis0_fwd_kernel<0>, grid_c, dim3(NS_THREADS), lds_c, s, p);
        }
        if (int rc = ra_check("ns2d step")) return rc;
    }
    return 0;
}

}  // namespace uno
