// Any-grid form of pointwise_op_3D's FFT crop / resample (K1a / K5a / K3a; C ABI: uno_fft_resample3d_any, uno_fft_resample3d_any_acc).
//
// uno_fft_resample3d runs on the MFMA plane-batched kernels (dft2d_plane.hip) and the tiled leading-axis kernels (cdft_axis.hip): even
// kept-row counts (<= 80 / 48), modes3 <= 16, (W, T) planes of <= 1792 elements, T <= 64.  The reference's first 3-D model
// (Uno3D_T40, navier_stokes_uno3d.py:22-237) leaves that range in its last two layers ((32,32,31) -> (48,48,41) -> (64,64,52) at
// S = 64, pad 3), and any grid with an odd kept-row count does.  These kernels compute the same operator - same frequency tables,
// same Hermitian-weight contract, bug-compatible with the reference (include/uno_spectral.h) - for ANY row counts, any
// 1 <= modes3 <= D3/2 + 1 and every axis length in 2 ... 128.  What bounds them is the LDS: a workgroup keeps one real (D2, D3) plane
// plus its (D2, modes3) half-spectrum (K1a), or one (J2, modes3) spectrum plane plus its (M2, modes3) half-inverse (K3a) - at most
// 142 KB of the CU's 160 KB at 128 x 128.
//
// Plain f32 FMA with f32 accumulation; twiddles from LDS tables indexed (k n) mod N.  Three launches through a workspace of
// (n_vol, D1 + M1, J2, modes3) c64:
//   K1a  one (volume, d1) plane per workgroup pass: real -> modes3 bins along T, then the J2 table rows along W
//   K5a  both leading-axis transforms (D1 -> J1 rows -> M1) on 32-column tiles; the J1 spectrum rows exist in LDS only
//   K3a  one (volume, h1) plane per pass: J2 rows -> M2 along W, Hermitian weights, half-spectrum -> real along T
// Workgroups are persistent (the CU count x what the LDS admits) and load their tables once.  The complex stages give every thread
// four neighbouring columns (two ds_read_b128 + one twiddle per 16 FMA); the real stages give it four rows a quarter plane apart
// (odd row pitch: consecutive lanes hit consecutive banks).  Fixed summation order: two runs are bit-identical.
// K3a also has an accumulate form (y += result) and an accumulate + activation form (y_act = gelu(y) in the same pass): the point-wise
// branch of a one-buffer OperatorBlock_3D (reference integral_operators.py:506-512) on these grids.  Separate instantiations: the plain
// form's code is what it was.
#include "resample3d_common.h"

namespace uno {

struct Resample3dAnyParams {
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
    int accumulate;             // K3a: y += result instead of y = result
};

constexpr int RA_TILE = 32;     // columns per K5a tile

__host__ __device__ __forceinline__ int ra_up4(int n) { return (n + 3) & ~3; }

// out[a][l] = sum_b in[b][l] e^{-+ 2 pi i F / N}; forward (INV = false): F = freq[a] b, inverse: F = freq[b] a.  in: LDS, rows of Lp = 4 k
// complex; a thread owns columns l0 ... l0 + 3 of one output row and hands them to `store` (columns >= the row's length hold garbage)
template <bool INV, class Store>
__device__ __forceinline__ void ra_complex_stage(const float2* in, int Lp, int n_out, int n_sum, const int* freq, const float2* tw, int N,
                                                 Store store) {
    const int LG = Lp >> 2;
    const unsigned magic = ra_magic(N);
    for (int item = threadIdx.x; item < n_out * LG; item += RA_THREADS) {
        const int a = item / LG, l0 = (item - a * LG) << 2;
        float2 acc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = make_float2(0.f, 0.f);
        const int fa = INV ? a : freq[a];
        int idx = 0;
        const float2* col = in + l0;
        for (int b = 0; b < n_sum; ++b) {
            float2 t;
            if (INV) {
                const unsigned p = (unsigned)(freq[b] * a);
                t = tw[p - __umulhi(p, magic) * (unsigned)N];
            } else {
                t = tw[idx];
                t.y = -t.y;
                idx += fa; if (idx >= N) idx -= N;
            }
            const float4 v01 = *reinterpret_cast<const float4*>(col + (size_t)b * Lp);
            const float4 v23 = *reinterpret_cast<const float4*>(col + (size_t)b * Lp + 2);
            acc[0].x = fmaf(v01.x, t.x, fmaf(-v01.y, t.y, acc[0].x)); acc[0].y = fmaf(v01.y, t.x, fmaf(v01.x, t.y, acc[0].y));
            acc[1].x = fmaf(v01.z, t.x, fmaf(-v01.w, t.y, acc[1].x)); acc[1].y = fmaf(v01.w, t.x, fmaf(v01.z, t.y, acc[1].y));
            acc[2].x = fmaf(v23.x, t.x, fmaf(-v23.y, t.y, acc[2].x)); acc[2].y = fmaf(v23.y, t.x, fmaf(v23.x, t.y, acc[2].y));
            acc[3].x = fmaf(v23.z, t.x, fmaf(-v23.w, t.y, acc[3].x)); acc[3].y = fmaf(v23.w, t.x, fmaf(v23.z, t.y, acc[3].y));
        }
        store(a, l0, acc);
    }
}

// K1a.  LDS: A [D2][Lp] c64 | tw2 [D2] | tw3 [D3] | plane [D2][D3 | 1] f32 | f2 [J2]
__host__ __device__ __forceinline__ size_t ra_fwd_lds(int D2, int D3, int J2, int m3) {
    return (size_t)D2 * ra_up4(m3) * 8 + (size_t)(D2 + D3) * 8 + (size_t)D2 * (D3 | 1) * 4 + (size_t)J2 * 4;
}

__global__ __launch_bounds__(RA_THREADS) void resample3d_any_fwd_plane_kernel(Resample3dAnyParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D2 = p.D2, D3 = p.D3, J2 = p.J2, m3 = p.m3, Lp = ra_up4(m3), D3p = D3 | 1;
    float2* sA = reinterpret_cast<float2*>(smem);
    float2* tw2 = sA + (size_t)D2 * Lp;
    float2* tw3 = tw2 + D2;
    float* sx = reinterpret_cast<float*>(tw3 + D3);
    int* sf = reinterpret_cast<int*>(sx + (size_t)D2 * D3p);
    for (int n = threadIdx.x; n < D2; n += RA_THREADS) tw2[n] = p.tw2i[n];
    for (int n = threadIdx.x; n < D3; n += RA_THREADS) tw3[n] = p.tw3i[n];
    for (int j = threadIdx.x; j < J2; j += RA_THREADS) sf[j] = ra_mod(p.f2_in[j], D2);
    for (int i = threadIdx.x; i < D2 * Lp; i += RA_THREADS) sA[i] = make_float2(0.f, 0.f);     // the pad columns are read (never stored from)
    const int n_planes = p.n_vol * p.D1, plane_elems = D2 * D3, WQ = (D2 + 3) >> 2;
    for (int plane = blockIdx.x; plane < n_planes; plane += gridDim.x) {
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
        ra_complex_stage<false>(sA, Lp, J2, D2, sf, tw2, D2, [&](int j, int l0, const float2* acc) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (l0 + r < m3) dst[(size_t)j * m3 + l0 + r] = acc[r];
        });
    }
}

// K5a.  LDS: in [D1][32] c64 | S [J1][32] c64 | tw1i [D1] | tw1o [M1] | f_in [J1] | f_out [J1]
__host__ __device__ __forceinline__ size_t ra_axis_lds(int D1, int M1, int J1) {
    return (size_t)(D1 + J1) * RA_TILE * 8 + (size_t)(D1 + M1) * 8 + (size_t)J1 * 8;
}

__global__ __launch_bounds__(RA_THREADS) void resample3d_any_axis_kernel(Resample3dAnyParams p) {
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
        const int vol = (int)(it / tiles), c0 = (int)(it - (long long)vol * tiles) * RA_TILE;
        __syncthreads();        // tables ready / the previous tile's stages have read sIn and sS
        const float2* src = p.Z1 + (size_t)vol * D1 * C + c0;
        for (int i = threadIdx.x; i < D1 * RA_TILE; i += RA_THREADS) {
            const int d = i / RA_TILE, c = i - d * RA_TILE;
            sIn[i] = c0 + c < C ? src[(size_t)d * C + c] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        // S[j][c] = sum_d Z1[d][c] e^{-2 pi i f_in[j] d / D1}
        ra_complex_stage<false>(sIn, RA_TILE, J1, D1, fi, twi, D1, [&](int j, int l0, const float2* acc) {
            float4* q = reinterpret_cast<float4*>(sS + (size_t)j * RA_TILE + l0);
            q[0] = make_float4(acc[0].x, acc[0].y, acc[1].x, acc[1].y);
            q[1] = make_float4(acc[2].x, acc[2].y, acc[3].x, acc[3].y);
        });
        __syncthreads();
        // Z2[h][c] = sum_j S[j][c] e^{+2 pi i f_out[j] h / M1}
        float2* dst = p.Z2 + (size_t)vol * M1 * C + c0;
        ra_complex_stage<true>(sS, RA_TILE, M1, J1, fo, two, M1, [&](int h, int l0, const float2* acc) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (c0 + l0 + r < C) dst[(size_t)h * C + l0 + r] = acc[r];
        });
    }
}

// K3a.  LDS: Zs [J2][Lp] c64 | U [M2][Lp] c64 | tw2 [M2] | tw3 [M3] | f2 [J2]
__host__ __device__ __forceinline__ size_t ra_inv_lds(int M2, int M3, int J2, int m3) {
    return (size_t)(J2 + M2) * ra_up4(m3) * 8 + (size_t)(M2 + M3) * 8 + (size_t)J2 * 4;
}

// EPI 0: y = result; 1: y += result; 2: y += result and y_act = gelu(y)
template <int EPI>
__global__ __launch_bounds__(RA_THREADS) void resample3d_any_inv_plane_kernel(Resample3dAnyParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M2 = p.M2, M3 = p.M3, J2 = p.J2, m3 = p.m3, Lp = ra_up4(m3);
    float2* sZ = reinterpret_cast<float2*>(smem);
    float2* sU = sZ + (size_t)J2 * Lp;
    float2* tw2 = sU + (size_t)M2 * Lp;
    float2* tw3 = tw2 + M2;
    int* sf = reinterpret_cast<int*>(tw3 + M3);
    for (int n = threadIdx.x; n < M2; n += RA_THREADS) tw2[n] = p.tw2o[n];
    for (int n = threadIdx.x; n < M3; n += RA_THREADS) tw3[n] = p.tw3o[n];
    for (int j = threadIdx.x; j < J2; j += RA_THREADS) sf[j] = ra_mod(p.f2_out[j], M2);
    for (int i = threadIdx.x; i < J2 * Lp; i += RA_THREADS) sZ[i] = make_float2(0.f, 0.f);     // pad columns: read, never stored from
    const int n_planes = p.n_vol * p.M1, WQ = (M2 + 3) >> 2;
    for (int plane = blockIdx.x; plane < n_planes; plane += gridDim.x) {
        __syncthreads();        // tables ready / the previous plane's stages have read sZ and sU
        const float2* src = p.Z2 + (size_t)plane * J2 * m3;
        for (int i = threadIdx.x; i < J2 * m3; i += RA_THREADS) {
            const int j = i / m3;
            sZ[(size_t)j * Lp + (i - j * m3)] = src[i];
        }
        __syncthreads();
        // stage 1: U[w][l] = scale c_l sum_j Z2[j][l] e^{+2 pi i f_j w / M2}
        ra_complex_stage<true>(sZ, Lp, M2, J2, sf, tw2, M2, [&](int w, int l0, const float2* acc) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float f = p.scale * (p.herm_out ? herm_weight(l0 + r, M3) : 1.0f);
                sU[(size_t)w * Lp + l0 + r] = make_float2(acc[r].x * f, acc[r].y * f);
            }
        });
        __syncthreads();
        // stage 2: y[w][t] = Re sum_l U[w][l] e^{+2 pi i l t / M3}; rows w = wq + r WQ
        float* dst = p.y + (size_t)plane * M2 * M3;
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
                    if (EPI == 2) p.y_act[(size_t)plane * M2 * M3 + (size_t)w * M3 + t] = uno_gelu(v);
                }
            }
        }
    }
}

int launch_resample3d_any(const float* x, float* y, float* y_act, int accumulate, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3, int J1,
                          const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3, float scale,
                          int herm_in, int herm_out, hipStream_t s) {
    Resample3dAnyParams p;
    p.x = x; p.y = y; p.y_act = accumulate ? y_act : nullptr; p.accumulate = accumulate ? 1 : 0;
    p.Z1 = static_cast<float2*>(ws);
    p.Z2 = p.Z1 + (size_t)n_vol * D1 * J2 * m3;
    p.f1_in = f1_in; p.f1_out = f1_out; p.f2_in = f2_in; p.f2_out = f2_out;
    p.n_vol = n_vol; p.D1 = D1; p.D2 = D2; p.D3 = D3; p.M1 = M1; p.M2 = M2; p.M3 = M3; p.J1 = J1; p.J2 = J2; p.m3 = m3;
    p.scale = scale; p.herm_in = herm_in ? 1 : 0; p.herm_out = herm_out ? 1 : 0;
    p.tw1i = twiddle_table(D1); p.tw2i = twiddle_table(D2); p.tw3i = twiddle_table(D3);
    p.tw1o = twiddle_table(M1); p.tw2o = twiddle_table(M2); p.tw3o = twiddle_table(M3);
    if (!p.tw1i || !p.tw2i || !p.tw3i || !p.tw1o || !p.tw2o || !p.tw3o) return -6;
    const size_t lds_f = ra_fwd_lds(D2, D3, J2, m3), lds_a = ra_axis_lds(D1, M1, J1), lds_i = ra_inv_lds(M2, M3, J2, m3);
    static int slot_f[64], slot_a[64], slot_i[3][64];
    const int epi = !p.accumulate ? 0 : (p.y_act ? 2 : 1);
    const void* inv_kernel = epi == 0   ? reinterpret_cast<const void*>(resample3d_any_inv_plane_kernel<0>)
                             : epi == 1 ? reinterpret_cast<const void*>(resample3d_any_inv_plane_kernel<1>)
                                        : reinterpret_cast<const void*>(resample3d_any_inv_plane_kernel<2>);
    if (!ensure_dynamic_lds(reinterpret_cast<const void*>(resample3d_any_fwd_plane_kernel), lds_f, slot_f) ||
        !ensure_dynamic_lds(reinterpret_cast<const void*>(resample3d_any_axis_kernel), lds_a, slot_a) ||
        !ensure_dynamic_lds(inv_kernel, lds_i, slot_i[epi])) {
        set_error("uno_fft_resample3d_any: cannot raise the dynamic LDS limit (%zu / %zu / %zu bytes)", lds_f, lds_a, lds_i);
        return -3;
    }
    const double spec = 8.0 * n_vol * (double)J2 * m3;
    {
        ProfScope prof("uno::resample3d_any_fwd_plane_kernel", 4.0 * n_vol * (double)D1 * D2 * D3 + spec * D1, s);
        hipLaunchKernelGGL(resample3d_any_fwd_plane_kernel, dim3(ra_grid((long long)n_vol * D1, lds_f)), dim3(RA_THREADS), lds_f, s, p);
    }
    if (int rc = ra_check("resample3d_any_fwd_plane")) return rc;
    {
        ProfScope prof("uno::resample3d_any_axis_kernel", spec * (D1 + M1), s);
        const long long tiles = ((long long)J2 * m3 + RA_TILE - 1) / RA_TILE;
        hipLaunchKernelGGL(resample3d_any_axis_kernel, dim3(ra_grid(n_vol * tiles, lds_a)), dim3(RA_THREADS), lds_a, s, p);
    }
    if (int rc = ra_check("resample3d_any_axis")) return rc;
    const double out_bytes = 4.0 * n_vol * (double)M1 * M2 * M3;
    const dim3 grid_i(ra_grid((long long)n_vol * M1, lds_i));
    if (epi == 0) {
        ProfScope prof("uno::resample3d_any_inv_plane_kernel", out_bytes + spec * M1, s);
        hipLaunchKernelGGL(resample3d_any_inv_plane_kernel<0>, grid_i, dim3(RA_THREADS), lds_i, s, p);
    } else {        // + the read of the old y and, with the activation, the second store
        ProfScope prof("uno::resample3d_any_inv_plane_acc_kernel", out_bytes * (epi == 2 ? 3.0 : 2.0) + spec * M1, s);
        if (epi == 1) hipLaunchKernelGGL(resample3d_any_inv_plane_kernel<1>, grid_i, dim3(RA_THREADS), lds_i, s, p);
        else hipLaunchKernelGGL(resample3d_any_inv_plane_kernel<2>, grid_i, dim3(RA_THREADS), lds_i, s, p);
    }
    return ra_check(epi ? "resample3d_any_inv_plane_acc" : "resample3d_any_inv_plane");
}

}  // namespace uno
