// Wide-axis form of pointwise_op_3D's FFT crop / resample (K1w / K5w / K3w; C ABI: uno_fft_resample3d_wide, uno_fft_resample3d_wide_acc).
//
// The any-grid kernels (resample3d_any.hip) stop at axes of 128 and run every sum on plain FMA.  The reference's 256 x 256 NS-3D models
// (Uno3D_T20_256 / Uno3D_T10_256, navier_stokes_uno3d.py:993-1372) resample (256,256,T) -> (64,64,T) in their first layer and
// (64,64,T) -> (256,256,T) in their last: sums of up to 256 terms along the two complex axes, several times over the machine's
// flop / byte balance on the vector pipe.  These kernels compute the same operator - same frequency tables, same Hermitian-weight
// contract, bug-compatible with the reference (include/uno_spectral.h) - for complex axes of 2 ... 256 and a real axis of 2 ... 64, with
// the long-axis stages on v_mfma_f32_16x16x4_f32 (exact f32, k-ordered).
//
// A complex stage out[a][l] = sum_b E[a][b] in[b][l] is a real GEMM on the interleaved (re, im) columns of `in`:
//   out = Er . in + Ei . in',   in'[b][2l] = -Im in[b][l],  in'[b][2l + 1] = Re in[b][l]
// so a 16-row x 16-real-column tile (8 complex columns) takes two MFMAs per four terms into ONE accumulator, and a layer with 5 ... 12
// kept bins fills 10 ... 24 of 16 / 32 columns.  The A operand is the twiddle itself, looked up in an LDS table at (f b) mod N.
// Three launches through a workspace of (n_vol, D1 + M1, J2, modes3) c64, as in the any-grid family:
//   K1w  one (volume, d1) plane per workgroup pass: real -> modes3 bins along T (FMA, <= 64 terms), then the J2 rows along W (MFMA)
//   K5w  both leading-axis transforms (D1 -> J1 rows -> M1) on 32-column tiles (MFMA); the J1 spectrum rows exist in LDS only
//   K3w  one (volume, h1) plane per pass: J2 rows -> M2 along W (MFMA), Hermitian weights, half-spectrum -> real along T (FMA)
// Workgroups are persistent and load their tables once.  Every plane and volume offset is a 64-bit product; fixed summation order: two
// runs are bit-identical.  K3w has the accumulate (y += result) and accumulate + activation (y_act = gelu(y)) forms of K3a.
// What bounds the family is the LDS: K3w keeps (J2 + M2) rows of up8(modes3) complex - beyond 160 KB (modes3 = 33 with J2 + M2 > 500)
// the call is refused before any launch.
#include "resample3d_common.h"

namespace uno {

struct Resample3dWideParams {
    const float* x;             // (n_vol, D1, D2, D3) f32
    float* y;                   // (n_vol, M1, M2, M3) f32
    float* y_act;               // accumulate form only: gelu(y) after the accumulation, or nullptr
    float2* Z1;                 // (n_vol, D1, J2, m3) c64
    float2* Z2;                 // (n_vol, M1, J2, m3) c64
    const float2 *tw1i, *tw2i, *tw3i, *tw1o, *tw2o, *tw3o;     // (cos, sin)(2 pi n / N) of D1, D2, D3, M1, M2, M3
    const int *f1_in, *f1_out, *f2_in, *f2_out;
    int n_vol, D1, D2, D3, M1, M2, M3, J1, J2, m3;
    float scale;
    int herm_in, herm_out;
};

constexpr int RW_THREADS = RA_THREADS;
constexpr int RW_WAVES = RW_THREADS / 64;
constexpr int RW_TILE = 32;     // complex columns per K5w tile
constexpr int RW_NT = 2;        // 16-column MFMA tiles a wave keeps beside each other (they share the twiddle operand)

__host__ __device__ __forceinline__ int rw_up8(int n) { return (n + 7) & ~7; }

// out[a][l] = sum_b in[b][l] e^{-+ 2 pi i F / N}; forward (INV = false): F = freq[a] b, inverse: F = freq[b] a.  in: LDS, rows of Lp = 8 k
// complex.  A wave owns 16 output rows x RW_NT tiles of 16 real columns; lane (i, k) = (lane & 15, lane >> 4) supplies the twiddle of
// (row i, term k) and real column i of term k, and ends with rows 4 k ... 4 k + 3 of real column i, which it hands to
// store(row, real column, value) (rows >= n_out are not handed over; columns >= the row's length hold garbage).
template <bool INV, class Store>
__device__ __forceinline__ void rw_complex_stage(const float2* in, int Lp, int n_out, int n_sum, const int* freq, const float2* tw, int N,
                                                 Store store) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, k = lane >> 4;
    const int col_tiles = Lp >> 3, col_groups = (col_tiles + RW_NT - 1) / RW_NT, row_tiles = (n_out + 15) >> 4;
    const int ksteps = (n_sum + 3) >> 2;
    const unsigned magic = ra_magic(N);
    const bool odd = i & 1;
    for (int item = wave; item < row_tiles * col_groups; item += RW_WAVES) {
        const int rt = item / col_groups, cg = item - rt * col_groups;
        const int a = min(rt * 16 + i, n_out - 1);
        f32x4 acc[RW_NT];
#pragma unroll
        for (int nt = 0; nt < RW_NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int fa = INV ? a : freq[a];
        int idx = INV ? 0 : (fa * k) % N;
        const int step = INV ? 0 : (4 * fa) % N;
        const float2* col = in + cg * (RW_NT * 8) + (i >> 1);
        for (int ks = 0; ks < ksteps; ++ks) {
            const int b = 4 * ks + k, bc = min(b, n_sum - 1);
            float2 t;
            if (INV) {
                const unsigned p = (unsigned)(freq[bc] * a);
                t = tw[p - __umulhi(p, magic) * (unsigned)N];
            } else {
                t = tw[idx];
                t.y = -t.y;
                idx += step; if (idx >= N) idx -= N;
            }
            if (b >= n_sum) t = make_float2(0.f, 0.f);      // the last step's missing terms (their column operand is row n_sum - 1 again)
#pragma unroll
            for (int nt = 0; nt < RW_NT; ++nt) {
                if (cg * RW_NT + nt >= col_tiles) continue;
                const float2 v = col[(size_t)bc * Lp + nt * 8];
                acc[nt] = mfma16(t.x, odd ? v.y : v.x, acc[nt]);
                acc[nt] = mfma16(t.y, odd ? v.x : -v.y, acc[nt]);
            }
        }
#pragma unroll
        for (int nt = 0; nt < RW_NT; ++nt) {
            if (cg * RW_NT + nt >= col_tiles) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rt * 16 + 4 * k + r;
                if (row < n_out) store(row, (cg * RW_NT + nt) * 16 + i, acc[nt][r]);
            }
        }
    }
}

// K1w.  LDS: A [D2][Lp] c64 | tw2 [D2] | tw3 [D3] | plane [D2][D3 | 1] f32 | f2 [J2]
__host__ __device__ __forceinline__ size_t rw_fwd_lds(int D2, int D3, int J2, int m3) {
    return (size_t)D2 * rw_up8(m3) * 8 + (size_t)(D2 + D3) * 8 + (size_t)D2 * (D3 | 1) * 4 + (size_t)J2 * 4;
}

__global__ __launch_bounds__(RW_THREADS) void resample3d_wide_fwd_plane_kernel(Resample3dWideParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D2 = p.D2, D3 = p.D3, J2 = p.J2, m3 = p.m3, Lp = rw_up8(m3), D3p = D3 | 1;
    float2* sA = reinterpret_cast<float2*>(smem);
    float2* tw2 = sA + (size_t)D2 * Lp;
    float2* tw3 = tw2 + D2;
    float* sx = reinterpret_cast<float*>(tw3 + D3);
    int* sf = reinterpret_cast<int*>(sx + (size_t)D2 * D3p);
    for (int n = threadIdx.x; n < D2; n += RW_THREADS) tw2[n] = p.tw2i[n];
    for (int n = threadIdx.x; n < D3; n += RW_THREADS) tw3[n] = p.tw3i[n];
    for (int j = threadIdx.x; j < J2; j += RW_THREADS) sf[j] = ra_mod(p.f2_in[j], D2);
    for (int i = threadIdx.x; i < D2 * Lp; i += RW_THREADS) sA[i] = make_float2(0.f, 0.f);     // the pad columns are read (never stored from)
    const long long n_planes = (long long)p.n_vol * p.D1;
    const int plane_elems = D2 * D3, WQ = (D2 + 3) >> 2;
    for (long long plane = blockIdx.x; plane < n_planes; plane += gridDim.x) {
        __syncthreads();        // tables ready / the previous plane's stage 2 has read sA
        const float* src = p.x + (size_t)plane * plane_elems;
        for (int i = threadIdx.x; i < plane_elems; i += RW_THREADS) {
            const int w = i / D3;
            sx[w * D3p + (i - w * D3)] = src[i];
        }
        __syncthreads();
        // stage 1: A[w][l] = c_l sum_t x[w][t] e^{-2 pi i l t / D3}; rows w = wq + r WQ
        for (int item = threadIdx.x; item < m3 * WQ; item += RW_THREADS) {
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
        float* dst = reinterpret_cast<float*>(p.Z1 + (size_t)plane * J2 * m3);
        rw_complex_stage<false>(sA, Lp, J2, D2, sf, tw2, D2, [&](int j, int c, float v) {
            if (c < 2 * m3) dst[(size_t)j * 2 * m3 + c] = v;
        });
    }
}

// K5w.  LDS: in [D1][32] c64 | S [J1][32] c64 | tw1i [D1] | tw1o [M1] | f_in [J1] | f_out [J1]
__host__ __device__ __forceinline__ size_t rw_axis_lds(int D1, int M1, int J1) {
    return (size_t)(D1 + J1) * RW_TILE * 8 + (size_t)(D1 + M1) * 8 + (size_t)J1 * 8;
}

__global__ __launch_bounds__(RW_THREADS) void resample3d_wide_axis_kernel(Resample3dWideParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D1 = p.D1, M1 = p.M1, J1 = p.J1, C = p.J2 * p.m3;
    float2* sIn = reinterpret_cast<float2*>(smem);
    float2* sS = sIn + (size_t)D1 * RW_TILE;
    float2* twi = sS + (size_t)J1 * RW_TILE;
    float2* two = twi + D1;
    int* fi = reinterpret_cast<int*>(two + M1);
    int* fo = fi + J1;
    for (int n = threadIdx.x; n < D1; n += RW_THREADS) twi[n] = p.tw1i[n];
    for (int n = threadIdx.x; n < M1; n += RW_THREADS) two[n] = p.tw1o[n];
    for (int j = threadIdx.x; j < J1; j += RW_THREADS) { fi[j] = ra_mod(p.f1_in[j], D1); fo[j] = ra_mod(p.f1_out[j], M1); }
    const int tiles = (C + RW_TILE - 1) / RW_TILE;
    const long long n_items = (long long)p.n_vol * tiles;
    for (long long it = blockIdx.x; it < n_items; it += gridDim.x) {
        const long long vol = it / tiles;
        const int c0 = (int)(it - vol * tiles) * RW_TILE;
        __syncthreads();        // tables ready / the previous tile's stages have read sIn and sS
        const float2* src = p.Z1 + (size_t)vol * D1 * C + c0;
        for (int i = threadIdx.x; i < D1 * RW_TILE; i += RW_THREADS) {
            const int d = i / RW_TILE, c = i - d * RW_TILE;
            sIn[i] = c0 + c < C ? src[(size_t)d * C + c] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        // S[j][c] = sum_d Z1[d][c] e^{-2 pi i f_in[j] d / D1}
        float* sSf = reinterpret_cast<float*>(sS);
        rw_complex_stage<false>(sIn, RW_TILE, J1, D1, fi, twi, D1, [&](int j, int c, float v) { sSf[j * (2 * RW_TILE) + c] = v; });
        __syncthreads();
        // Z2[h][c] = sum_j S[j][c] e^{+2 pi i f_out[j] h / M1}
        float* dst = reinterpret_cast<float*>(p.Z2 + (size_t)vol * M1 * C + c0);
        const int valid = 2 * min(RW_TILE, C - c0);
        rw_complex_stage<true>(sS, RW_TILE, M1, J1, fo, two, M1, [&](int h, int c, float v) {
            if (c < valid) dst[(size_t)h * 2 * C + c] = v;
        });
    }
}

// K3w.  LDS: Zs [J2][Lp] c64 | U [M2][Lp] c64 | tw2 [M2] | tw3 [M3] | f2 [J2]
__host__ __device__ __forceinline__ size_t rw_inv_lds(int M2, int M3, int J2, int m3) {
    return (size_t)(J2 + M2) * rw_up8(m3) * 8 + (size_t)(M2 + M3) * 8 + (size_t)J2 * 4;
}

// EPI 0: y = result; 1: y += result; 2: y += result and y_act = gelu(y)
template <int EPI>
__global__ __launch_bounds__(RW_THREADS) void resample3d_wide_inv_plane_kernel(Resample3dWideParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M2 = p.M2, M3 = p.M3, J2 = p.J2, m3 = p.m3, Lp = rw_up8(m3);
    float2* sZ = reinterpret_cast<float2*>(smem);
    float2* sU = sZ + (size_t)J2 * Lp;
    float2* tw2 = sU + (size_t)M2 * Lp;
    float2* tw3 = tw2 + M2;
    int* sf = reinterpret_cast<int*>(tw3 + M3);
    for (int n = threadIdx.x; n < M2; n += RW_THREADS) tw2[n] = p.tw2o[n];
    for (int n = threadIdx.x; n < M3; n += RW_THREADS) tw3[n] = p.tw3o[n];
    for (int j = threadIdx.x; j < J2; j += RW_THREADS) sf[j] = ra_mod(p.f2_out[j], M2);
    for (int i = threadIdx.x; i < J2 * Lp; i += RW_THREADS) sZ[i] = make_float2(0.f, 0.f);     // pad columns: read, never stored from
    const long long n_planes = (long long)p.n_vol * p.M1;
    const int WQ = (M2 + 3) >> 2;
    for (long long plane = blockIdx.x; plane < n_planes; plane += gridDim.x) {
        __syncthreads();        // tables ready / the previous plane's stages have read sZ and sU
        const float2* src = p.Z2 + (size_t)plane * J2 * m3;
        for (int i = threadIdx.x; i < J2 * m3; i += RW_THREADS) {
            const int j = i / m3;
            sZ[(size_t)j * Lp + (i - j * m3)] = src[i];
        }
        __syncthreads();
        // stage 1: U[w][l] = scale c_l sum_j Z2[j][l] e^{+2 pi i f_j w / M2}
        float* sUf = reinterpret_cast<float*>(sU);
        rw_complex_stage<true>(sZ, Lp, M2, J2, sf, tw2, M2, [&](int w, int c, float v) {
            sUf[(size_t)w * 2 * Lp + c] = v * (p.scale * (p.herm_out ? herm_weight(c >> 1, M3) : 1.0f));
        });
        __syncthreads();
        // stage 2: y[w][t] = Re sum_l U[w][l] e^{+2 pi i l t / M3}; rows w = wq + r WQ
        const size_t base = (size_t)plane * M2 * M3;
        float* dst = p.y + base;
        for (int item = threadIdx.x; item < WQ * M3; item += RW_THREADS) {
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

void resample3d_wide_lds_bytes(int D1, int D2, int D3, int M1, int M2, int M3, int J1, int J2, int m3, size_t out[3]) {
    out[0] = rw_fwd_lds(D2, D3, J2, m3);
    out[1] = rw_axis_lds(D1, M1, J1);
    out[2] = rw_inv_lds(M2, M3, J2, m3);
}

int launch_resample3d_wide(const float* x, float* y, float* y_act, int accumulate, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                           int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3, float scale,
                           int herm_in, int herm_out, hipStream_t s) {
    size_t lds[3];
    resample3d_wide_lds_bytes(D1, D2, D3, M1, M2, M3, J1, J2, m3, lds);
    const size_t lds_f = lds[0], lds_a = lds[1], lds_i = lds[2];        // (within 160 KB: the entry point has refused anything else)
    Resample3dWideParams p;
    p.x = x; p.y = y; p.y_act = accumulate ? y_act : nullptr;
    p.Z1 = static_cast<float2*>(ws);
    p.Z2 = p.Z1 + (size_t)n_vol * D1 * J2 * m3;
    p.f1_in = f1_in; p.f1_out = f1_out; p.f2_in = f2_in; p.f2_out = f2_out;
    p.n_vol = n_vol; p.D1 = D1; p.D2 = D2; p.D3 = D3; p.M1 = M1; p.M2 = M2; p.M3 = M3; p.J1 = J1; p.J2 = J2; p.m3 = m3;
    p.scale = scale; p.herm_in = herm_in ? 1 : 0; p.herm_out = herm_out ? 1 : 0;
    p.tw1i = twiddle_table(D1); p.tw2i = twiddle_table(D2); p.tw3i = twiddle_table(D3);
    p.tw1o = twiddle_table(M1); p.tw2o = twiddle_table(M2); p.tw3o = twiddle_table(M3);
    if (!p.tw1i || !p.tw2i || !p.tw3i || !p.tw1o || !p.tw2o || !p.tw3o) return -6;
    static int slot_f[64], slot_a[64], slot_i[3][64];
    const int epi = !accumulate ? 0 : (p.y_act ? 2 : 1);
    const void* inv_kernel = epi == 0   ? reinterpret_cast<const void*>(resample3d_wide_inv_plane_kernel<0>)
                             : epi == 1 ? reinterpret_cast<const void*>(resample3d_wide_inv_plane_kernel<1>)
                                        : reinterpret_cast<const void*>(resample3d_wide_inv_plane_kernel<2>);
    if (!ensure_dynamic_lds(reinterpret_cast<const void*>(resample3d_wide_fwd_plane_kernel), lds_f, slot_f) ||
        !ensure_dynamic_lds(reinterpret_cast<const void*>(resample3d_wide_axis_kernel), lds_a, slot_a) ||
        !ensure_dynamic_lds(inv_kernel, lds_i, slot_i[epi])) {
        set_error("uno_fft_resample3d_wide: cannot raise the dynamic LDS limit (%zu / %zu / %zu bytes)", lds_f, lds_a, lds_i);
        return -3;
    }
    const double spec = 8.0 * n_vol * (double)J2 * m3;
    {
        ProfScope prof("uno::resample3d_wide_fwd_plane_kernel", 4.0 * n_vol * (double)D1 * D2 * D3 + spec * D1, s);
        hipLaunchKernelGGL(resample3d_wide_fwd_plane_kernel, dim3(ra_grid((long long)n_vol * D1, lds_f)), dim3(RW_THREADS), lds_f, s, p);
    }
    if (int rc = ra_check("resample3d_wide_fwd_plane")) return rc;
    {
        ProfScope prof("uno::resample3d_wide_axis_kernel", spec * (D1 + M1), s);
        const long long tiles = ((long long)J2 * m3 + RW_TILE - 1) / RW_TILE;
        hipLaunchKernelGGL(resample3d_wide_axis_kernel, dim3(ra_grid(n_vol * tiles, lds_a)), dim3(RW_THREADS), lds_a, s, p);
    }
    if (int rc = ra_check("resample3d_wide_axis")) return rc;
    const double out_bytes = 4.0 * n_vol * (double)M1 * M2 * M3;
    const dim3 grid_i(ra_grid((long long)n_vol * M1, lds_i));
    if (epi == 0) {
        ProfScope prof("uno::resample3d_wide_inv_plane_kernel", out_bytes + spec * M1, s);
        hipLaunchKernelGGL(resample3d_wide_inv_plane_kernel<0>, grid_i, dim3(RW_THREADS), lds_i, s, p);
    } else {        // + the read of the old y and, with the activation, the second store
        ProfScope prof("uno::resample3d_wide_inv_plane_acc_kernel", out_bytes * (epi == 2 ? 3.0 : 2.0) + spec * M1, s);
        if (epi == 1) hipLaunchKernelGGL(resample3d_wide_inv_plane_kernel<1>, grid_i, dim3(RW_THREADS), lds_i, s, p);
        else hipLaunchKernelGGL(resample3d_wide_inv_plane_kernel<2>, grid_i, dim3(RW_THREADS), lds_i, s, p);
    }
    return ra_check(epi ? "resample3d_wide_inv_plane_acc" : "resample3d_wide_inv_plane");
}

}  // namespace uno
