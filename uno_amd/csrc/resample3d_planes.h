// The three plane-at-a-time kernels of pointwise_op_3D's FFT crop / resample, written once for the two families that run them:
//   resample3d_any.hip   K1a / K5a / K3a  every sum on plain FMA, axes of 2 ... 128
//   resample3d_wide.hip  K1w / K5w / K3w  the long-axis sums on v_mfma_f32_16x16x4_f32, leading axes of 2 ... 256
// Three launches through a workspace of (n_vol, D1 + M1, J2, modes3) c64:
//   K1  one (volume, d1) plane per workgroup pass: real -> modes3 bins along T, then the J2 table rows along W
//   K5  both leading-axis transforms (D1 -> J1 rows -> M1) on 32-column tiles; the J1 spectrum rows exist in LDS only
//   K3  one (volume, h1) plane per pass: J2 rows -> M2 along W, Hermitian weights, half-spectrum -> real along T
// Workgroups are persistent and load their tables once; every plane and volume offset is a 64-bit product; fixed summation order: two
// runs are bit-identical.  The real stages (K1 stage 1, K3 stage 2) give a thread four rows a quarter plane apart (odd row pitch:
// consecutive lanes hit consecutive banks) and are the same code in both families.
//
// A family is a struct F with
//   F::name                                      "any" / "wide": the event-record names are uno::resample3d_<name>_<kernel>
//   F::up(m3)                                    the LDS row length, in complex, of a plane with m3 kept bins
//   F::complex_stage<INV>(in, Lp, n_out, n_sum, freq, tw, N, sink)
//       out[a][l] = sum_b in[b][l] e^{-+ 2 pi i F / N}; forward (INV = false): F = freq[a] b, inverse: F = freq[b] a.  in: LDS, rows of Lp
//       complex, Lp a multiple of F::up(1).  The stage hands its results to `sink`, one of the three types below, through the call
//       operator of its own granularity: (row, first column l0, four complex columns) or (row, REAL column c, value); only the one
//       a family calls is instantiated.  Columns at or beyond a row's length hold garbage, and the sinks drop them where it matters.
// The kernels are templates on F, so their device symbols carry the family as a template argument
// (uno::resample3d_fwd_plane_kernel<uno::ResampleWide>).
#pragma once
#include "resample3d_common.h"
#include <string>

namespace uno {

struct Resample3dParams {
    const float* x;             // (n_vol, D1, D2, D3) f32
    float* y;                   // (n_vol, M1, M2, M3) f32
    float* y_act;               // accumulate form only: (n_vol, M1, M2, M3) f32 = gelu(y) after the accumulation, or nullptr
    float2* Z1;                 // (n_vol, D1, J2, m3) c64
    float2* Z2;                 // (n_vol, M1, J2, m3) c64
    const float2 *tw1i, *tw2i, *tw3i, *tw1o, *tw2o, *tw3o;     // (cos, sin)(2 pi n / N) of D1, D2, D3, M1, M2, M3
    const int *f1_in, *f1_out, *f2_in, *f2_out;
    int n_vol, D1, D2, D3, M1, M2, M3, J1, J2, m3;
    float scale;
    int herm_in, herm_out;
};

constexpr int RA_TILE = 32;     // complex columns per K5 tile

// ---- what a complex stage writes to.  The sinks refer to the kernel's locals and to its parameter block, as the [&] lambdas they
// replace did: with members held by value the compiler schedules the kernels differently (profiles/resample3d_shared_isa.txt).
// rows of `pitch` complex in global memory, of which the first `cols` columns exist (K1 stage 2 -> Z1, K5 -> Z2)
struct GlobalRowSink {
    float2* const& dst;
    const int& pitch;
    const int& cols;
    __device__ __forceinline__ void operator()(int row, int l0, const float2* acc) const {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (l0 + r < cols) dst[(size_t)row * pitch + l0 + r] = acc[r];
    }
    __device__ __forceinline__ void operator()(int row, int c, float v) const {
        if (c < 2 * cols) reinterpret_cast<float*>(dst)[(size_t)row * 2 * pitch + c] = v;
    }
};

// the J1 spectrum rows of a K5 tile, in LDS
struct TileSink {
    float2* const& S;
    __device__ __forceinline__ void operator()(int row, int l0, const float2* acc) const {
        float4* q = reinterpret_cast<float4*>(S + (size_t)row * RA_TILE + l0);
        q[0] = make_float4(acc[0].x, acc[0].y, acc[1].x, acc[1].y);
        q[1] = make_float4(acc[2].x, acc[2].y, acc[3].x, acc[3].y);
    }
    __device__ __forceinline__ void operator()(int row, int c, float v) const { reinterpret_cast<float*>(S)[row * (2 * RA_TILE) + c] = v; }
};

// K3 stage 1 -> U in LDS, times scale and the Hermitian weight of the column's bin
struct WeightedSink {
    float2* const& U;
    const int& Lp;
    const int& M3;
    const Resample3dParams& p;
    __device__ __forceinline__ float weight(int l) const { return p.scale * (p.herm_out ? herm_weight(l, M3) : 1.0f); }
    __device__ __forceinline__ void operator()(int row, int l0, const float2* acc) const {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float f = weight(l0 + r);
            U[(size_t)row * Lp + l0 + r] = make_float2(acc[r].x * f, acc[r].y * f);
        }
    }
    __device__ __forceinline__ void operator()(int row, int c, float v) const {
        reinterpret_cast<float*>(U)[(size_t)row * 2 * Lp + c] = v * weight(c >> 1);
    }
};

// ---- K1.  LDS: A [D2][Lp] c64 | tw2 [D2] | tw3 [D3] | plane [D2][D3 | 1] f32 | f2 [J2]
template <class F>
__global__ __launch_bounds__(RA_THREADS) void resample3d_fwd_plane_kernel(Resample3dParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D2 = p.D2, D3 = p.D3, J2 = p.J2, m3 = p.m3, Lp = F::up(m3), D3p = D3 | 1;
    float2* sA = reinterpret_cast<float2*>(smem);
    float2* tw2 = sA + (size_t)D2 * Lp;
    float2* tw3 = tw2 + D2;
    float* sx = reinterpret_cast<float*>(tw3 + D3);
    int* sf = reinterpret_cast<int*>(sx + (size_t)D2 * D3p);
    for (int n = threadIdx.x; n < D2; n += RA_THREADS) tw2[n] = p.tw2i[n];
    for (int n = threadIdx.x; n < D3; n += RA_THREADS) tw3[n] = p.tw3i[n];
    for (int j = threadIdx.x; j < J2; j += RA_THREADS) sf[j] = ra_mod(p.f2_in[j], D2);
    for (int i = threadIdx.x; i < D2 * Lp; i += RA_THREADS) sA[i] = make_float2(0.f, 0.f);     // the pad columns are read (never stored from)
    const long long n_planes = (long long)p.n_vol * p.D1;
    const int plane_elems = D2 * D3, WQ = (D2 + 3) >> 2;
    for (long long plane = blockIdx.x; plane < n_planes; plane += gridDim.x) {
        __syncthreads();        // tables ready / the previous plane's stage 2 has read sA
        const float* src = p.x + (size_t)plane * plane_elems;
        for (int i = threadIdx.x; i < plane_elems; i += RA_THREADS) {
            const int w = i / D3;
            sx[w * D3p + (i - w * D3)] = src[i];
        }
        __syncthreads();
        // stage 1: A[w][l] = c_l sum_t x[w][t] e^{-2 pi i l t / D3}; rows w = wq + r WQ
        for (int item = threadIdx.x; item < m3 * WQ; item += RA_THREADS) {
            const int l = item / WQ, wq = item - l * WQ;
            int row[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) row[r] = min(wq + r * WQ, D2 - 1) * D3p;
            float ar[4] = {0.f, 0.f, 0.f, 0.f}, ai[4] = {0.f, 0.f, 0.f, 0.f};
            int idx = 0;
            for (int t = 0; t < D3; ++t) {
                const float2 tw = tw3[idx];
                idx += l; if (idx >= D3) idx -= D3;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = sx[row[r] + t];
                    ar[r] = fmaf(v, tw.x, ar[r]);
                    ai[r] = fmaf(-v, tw.y, ai[r]);
                }
            }
            const float hw = p.herm_in ? herm_weight(l, D3) : 1.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int w = wq + r * WQ;
                if (w < D2) sA[(size_t)w * Lp + l] = make_float2(ar[r] * hw, ai[r] * hw);
            }
        }
        __syncthreads();
        // stage 2: Z1[plane][j][l] = sum_w A[w][l] e^{-2 pi i f_j w / D2}
        float2* dst = p.Z1 + (size_t)plane * J2 * m3;
        F::template complex_stage<false>(sA, Lp, J2, D2, sf, tw2, D2, GlobalRowSink{dst, m3, m3});
    }
}

// ---- K5.  LDS: in [D1][32] c64 | S [J1][32] c64 | tw1i [D1] | tw1o [M1] | f_in [J1] | f_out [J1]
template <class F>
__global__ __launch_bounds__(RA_THREADS) void resample3d_axis_kernel(Resample3dParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D1 = p.D1, M1 = p.M1, J1 = p.J1, C = p.J2 * p.m3;
    float2* sIn = reinterpret_cast<float2*>(smem);
    float2* sS = sIn + (size_t)D1 * RA_TILE;
    float2* twi = sS + (size_t)J1 * RA_TILE;
    float2* two = twi + D1;
    int* fi = reinterpret_cast<int*>(two + M1);
    int* fo = fi + J1;
    for (int n = threadIdx.x; n < D1; n += RA_THREADS) twi[n] = p.tw1i[n];
    for (int n = threadIdx.x; n < M1; n += RA_THREADS) two[n] = p.tw1o[n];
    for (int j = threadIdx.x; j < J1; j += RA_THREADS) { fi[j] = ra_mod(p.f1_in[j], D1); fo[j] = ra_mod(p.f1_out[j], M1); }
    const int tiles = (C + RA_TILE - 1) / RA_TILE;
    const long long n_items = (long long)p.n_vol * tiles;
    for (long long it = blockIdx.x; it < n_items; it += gridDim.x) {
        const long long vol = it / tiles;
        const int c0 = (int)(it - vol * tiles) * RA_TILE;
        __syncthreads();        // tables ready / the previous tile's stages have read sIn and sS
        const float2* src = p.Z1 + (size_t)vol * D1 * C + c0;
        for (int i = threadIdx.x; i < D1 * RA_TILE; i += RA_THREADS) {
            const int d = i / RA_TILE, c = i - d * RA_TILE;
            sIn[i] = c0 + c < C ? src[(size_t)d * C + c] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        // S[j][c] = sum_d Z1[d][c] e^{-2 pi i f_in[j] d / D1}
        F::template complex_stage<false>(sIn, RA_TILE, J1, D1, fi, twi, D1, TileSink{sS});
        __syncthreads();
        // Z2[h][c] = sum_j S[j][c] e^{+2 pi i f_out[j] h / M1}
        float2* dst = p.Z2 + (size_t)vol * M1 * C + c0;
        const int cols = min(RA_TILE, C - c0);
        F::template complex_stage<true>(sS, RA_TILE, M1, J1, fo, two, M1, GlobalRowSink{dst, C, cols});
    }
}

// ---- K3.  LDS: Zs [J2][Lp] c64 | U [M2][Lp] c64 | tw2 [M2] | tw3 [M3] | f2 [J2]
// EPI 0: y = result; 1: y += result; 2: y += result and y_act = gelu(y) - the point-wise branch of a one-buffer OperatorBlock_3D
// (reference integral_operators.py:506-512).  Separate instantiations: the plain form pays nothing for the other two.
template <class F, int EPI>
__global__ __launch_bounds__(RA_THREADS) void resample3d_inv_plane_kernel(Resample3dParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M2 = p.M2, M3 = p.M3, J2 = p.J2, m3 = p.m3, Lp = F::up(m3);
    float2* sZ = reinterpret_cast<float2*>(smem);
    float2* sU = sZ + (size_t)J2 * Lp;
    float2* tw2 = sU + (size_t)M2 * Lp;
    float2* tw3 = tw2 + M2;
    int* sf = reinterpret_cast<int*>(tw3 + M3);
    for (int n = threadIdx.x; n < M2; n += RA_THREADS) tw2[n] = p.tw2o[n];
    for (int n = threadIdx.x; n < M3; n += RA_THREADS) tw3[n] = p.tw3o[n];
    for (int j = threadIdx.x; j < J2; j += RA_THREADS) sf[j] = ra_mod(p.f2_out[j], M2);
    for (int i = threadIdx.x; i < J2 * Lp; i += RA_THREADS) sZ[i] = make_float2(0.f, 0.f);     // pad columns: read, never stored from
    const long long n_planes = (long long)p.n_vol * p.M1;
    const int WQ = (M2 + 3) >> 2;
    for (long long plane = blockIdx.x; plane < n_planes; plane += gridDim.x) {
        __syncthreads();        // tables ready / the previous plane's stages have read sZ and sU
        const float2* src = p.Z2 + (size_t)plane * J2 * m3;
        for (int i = threadIdx.x; i < J2 * m3; i += RA_THREADS) {
            const int j = i / m3;
            sZ[(size_t)j * Lp + (i - j * m3)] = src[i];
        }
        __syncthreads();
        // stage 1: U[w][l] = scale c_l sum_j Z2[j][l] e^{+2 pi i f_j w / M2}
        F::template complex_stage<true>(sZ, Lp, M2, J2, sf, tw2, M2, WeightedSink{sU, Lp, M3, p});
        __syncthreads();
        // stage 2: y[w][t] = Re sum_l U[w][l] e^{+2 pi i l t / M3}; rows w = wq + r WQ
        const size_t base = (size_t)plane * M2 * M3;
        float* dst = p.y + base;
        for (int item = threadIdx.x; item < WQ * M3; item += RA_THREADS) {
            const int wq = item / M3, t = item - wq * M3;
            const float2* row[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) row[r] = sU + (size_t)min(wq + r * WQ, M2 - 1) * Lp;
            float old[4] = {0.f, 0.f, 0.f, 0.f};
            if (EPI) {          // the old values are asked for here and first used after the FMA loop, which hides their latency
#pragma unroll
                for (int r = 0; r < 4; ++r) old[r] = dst[(size_t)min(wq + r * WQ, M2 - 1) * M3 + t];
            }
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            int idx = 0;
            for (int l = 0; l < m3; ++l) {
                const float2 tw = tw3[idx];
                idx += t; if (idx >= M3) idx -= M3;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float2 u = row[r][l];
                    acc[r] = fmaf(u.x, tw.x, fmaf(-u.y, tw.y, acc[r]));
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int w = wq + r * WQ;
                if (w >= M2) continue;
                if (EPI == 0) {
                    dst[(size_t)w * M3 + t] = acc[r];
                } else {
                    const float v = old[r] + acc[r];
                    dst[(size_t)w * M3 + t] = v;
                    if (EPI == 2) p.y_act[base + (size_t)w * M3 + t] = uno_gelu(v);
                }
            }
        }
    }
}

// ---- host side
// dynamic LDS of K1 / K5 / K3 (the layouts above); what the entry points refuse beyond 160 KB and what the launcher asks for
template <class F>
void resample3d_lds_bytes(int D1, int D2, int D3, int M1, int M2, int M3, int J1, int J2, int m3, size_t out[3]) {
    out[0] = (size_t)D2 * F::up(m3) * 8 + (size_t)(D2 + D3) * 8 + (size_t)D2 * (D3 | 1) * 4 + (size_t)J2 * 4;
    out[1] = (size_t)(D1 + J1) * RA_TILE * 8 + (size_t)(D1 + M1) * 8 + (size_t)J1 * 8;
    out[2] = (size_t)(J2 + M2) * F::up(m3) * 8 + (size_t)(M2 + M3) * 8 + (size_t)J2 * 4;
}

// arguments validated by the caller (capi_spectral.hip: resample3d_planes_impl); accumulate != 0: y += result and, with
// y_act != nullptr, y_act = gelu(y)
template <class F>
int launch_resample3d_planes(const float* x, float* y, float* y_act, int accumulate, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2,
                             int M3, int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3, float scale,
                             int herm_in, int herm_out, hipStream_t s) {
    Resample3dParams p;
    p.x = x; p.y = y; p.y_act = accumulate ? y_act : nullptr;
    p.Z1 = static_cast<float2*>(ws);
    p.Z2 = p.Z1 + (size_t)n_vol * D1 * J2 * m3;
    p.f1_in = f1_in; p.f1_out = f1_out; p.f2_in = f2_in; p.f2_out = f2_out;
    p.n_vol = n_vol; p.D1 = D1; p.D2 = D2; p.D3 = D3; p.M1 = M1; p.M2 = M2; p.M3 = M3; p.J1 = J1; p.J2 = J2; p.m3 = m3;
    p.scale = scale; p.herm_in = herm_in ? 1 : 0; p.herm_out = herm_out ? 1 : 0;
    p.tw1i = twiddle_table(D1); p.tw2i = twiddle_table(D2); p.tw3i = twiddle_table(D3);
    p.tw1o = twiddle_table(M1); p.tw2o = twiddle_table(M2); p.tw3o = twiddle_table(M3);
    if (!p.tw1i || !p.tw2i || !p.tw3i || !p.tw1o || !p.tw2o || !p.tw3o) return -6;
    size_t lds[3];
    resample3d_lds_bytes<F>(D1, D2, D3, M1, M2, M3, J1, J2, m3, lds);
    const size_t lds_f = lds[0], lds_a = lds[1], lds_i = lds[2];
    static int slot_f[64], slot_a[64], slot_i[3][64];
    // the launches' names: `who` in a launch error, uno::<who>_kernel as an event record (uno::resample3d_any_fwd_plane_kernel, ...)
    static const std::string stem = std::string("resample3d_") + F::name;
    static const std::string who[4] = {stem + "_fwd_plane", stem + "_axis", stem + "_inv_plane", stem + "_inv_plane_acc"};
    static const std::string rec[4] = {"uno::" + who[0] + "_kernel", "uno::" + who[1] + "_kernel", "uno::" + who[2] + "_kernel", "uno::" + who[3] + "_kernel"};
    const int epi = !accumulate ? 0 : (p.y_act ? 2 : 1);
    void (*const inv_kernel)(Resample3dParams) = epi == 0   ? resample3d_inv_plane_kernel<F, 0>
                                                 : epi == 1 ? resample3d_inv_plane_kernel<F, 1>
                                                            : resample3d_inv_plane_kernel<F, 2>;
    if (!ensure_dynamic_lds(reinterpret_cast<const void*>(resample3d_fwd_plane_kernel<F>), lds_f, slot_f) ||
        !ensure_dynamic_lds(reinterpret_cast<const void*>(resample3d_axis_kernel<F>), lds_a, slot_a) ||
        !ensure_dynamic_lds(reinterpret_cast<const void*>(inv_kernel), lds_i, slot_i[epi])) {
        set_error("uno_fft_resample3d_%s: cannot raise the dynamic LDS limit (%zu / %zu / %zu bytes)", F::name, lds_f, lds_a, lds_i);
        return -3;
    }
    const double spec = 8.0 * n_vol * (double)J2 * m3;
    {
        ProfScope prof(rec[0].c_str(), 4.0 * n_vol * (double)D1 * D2 * D3 + spec * D1, s);
        hipLaunchKernelGGL(resample3d_fwd_plane_kernel<F>, dim3(ra_grid((long long)n_vol * D1, lds_f)), dim3(RA_THREADS), lds_f, s, p);
    }
    if (int rc = ra_check(who[0].c_str())) return rc;
    {
        ProfScope prof(rec[1].c_str(), spec * (D1 + M1), s);
        const long long tiles = ((long long)J2 * m3 + RA_TILE - 1) / RA_TILE;
        hipLaunchKernelGGL(resample3d_axis_kernel<F>, dim3(ra_grid(n_vol * tiles, lds_a)), dim3(RA_THREADS), lds_a, s, p);
    }
    if (int rc = ra_check(who[1].c_str())) return rc;
    const double out_bytes = 4.0 * n_vol * (double)M1 * M2 * M3;
    {       // the accumulate forms also read the old y and, with the activation, store twice
        ProfScope prof(rec[epi ? 3 : 2].c_str(), out_bytes * (epi + 1) + spec * M1, s);
        hipLaunchKernelGGL(inv_kernel, dim3(ra_grid((long long)n_vol * M1, lds_i)), dim3(RA_THREADS), lds_i, s, p);
    }
    return ra_check(who[epi ? 3 : 2].c_str());
}

}  // namespace uno
