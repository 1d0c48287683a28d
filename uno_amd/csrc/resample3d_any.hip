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
// The kernels are those of resample3d_planes.h with the complex stages below: plain f32 FMA with f32 accumulation, twiddles from LDS
// tables indexed (k n) mod N, every thread on four neighbouring columns (two ds_read_b128 + one twiddle per 16 FMA).
#include "resample3d_planes.h"

namespace uno {

struct ResampleAny {
    static constexpr const char* name = "any";
    __host__ __device__ static __forceinline__ int up(int n) { return (n + 3) & ~3; }

    // a thread owns columns l0 ... l0 + 3 of one output row and hands them to `sink`
    template <bool INV, class Sink>
    __device__ static __forceinline__ void complex_stage(const float2* in, int Lp, int n_out, int n_sum, const int* freq, const float2* tw, int N,
                                                         Sink sink) {
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
            sink(a, l0, acc);
        }
    }
};

void resample3d_any_lds_bytes(int D1, int D2, int D3, int M1, int M2, int M3, int J1, int J2, int m3, size_t out[3]) {
    resample3d_lds_bytes<ResampleAny>(D1, D2, D3, M1, M2, M3, J1, J2, m3, out);
}

int launch_resample3d_any(const float* x, float* y, float* y_act, int accumulate, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3, int J1,
                          const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3, float scale,
                          int herm_in, int herm_out, hipStream_t s) {
    return launch_resample3d_planes<ResampleAny>(x, y, y_act, accumulate, ws, n_vol, D1, D2, D3, M1, M2, M3, J1, f1_in, f1_out, J2, f2_in, f2_out, m3,
                                                 scale, herm_in, herm_out, s);
}

}  // namespace uno
