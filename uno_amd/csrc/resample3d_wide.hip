// Wide-axis form of pointwise_op_3D's FFT crop / resample (K1w / K5w / K3w; C ABI: uno_fft_resample3d_wide, uno_fft_resample3d_wide_acc).
//
// The any-grid kernels (resample3d_any.hip) stop at axes of 128 and run every sum on plain FMA.  The reference's 256 x 256 NS-3D models
// (Uno3D_T20_256 / Uno3D_T10_256, navier_stokes_uno3d.py:993-1372) resample (256,256,T) -> (64,64,T) in their first layer and
// (64,64,T) -> (256,256,T) in their last: sums of up to 256 terms along the two complex axes, several times over the machine's
// flop / byte balance on the vector pipe.  These kernels compute the same operator - same frequency tables, same Hermitian-weight
// contract, bug-compatible with the reference (include/uno_spectral.h) - for complex axes of 2 ... 256 and a real axis of 2 ... 64, with
// the long-axis stages on v_mfma_f32_16x16x4_f32 (exact f32, k-ordered).
//
// The kernels are those of resample3d_planes.h with the complex stage below.  A complex stage out[a][l] = sum_b E[a][b] in[b][l] is a
// real GEMM on the interleaved (re, im) columns of `in`:
//   out = Er . in + Ei . in',   in'[b][2l] = -Im in[b][l],  in'[b][2l + 1] = Re in[b][l]
// so a 16-row x 16-real-column tile (8 complex columns) takes two MFMAs per four terms into ONE accumulator, and a layer with 5 ... 12
// kept bins fills 10 ... 24 of 16 / 32 columns.  The A operand is the twiddle itself, looked up in an LDS table at (f b) mod N.  The
// real-axis stages (<= 64 terms) stay on FMA.
// What bounds the family is the LDS: K3w keeps (J2 + M2) rows of up(modes3) complex - beyond 160 KB (modes3 = 33 with J2 + M2 > 500)
// the call is refused before any launch.
#include "resample3d_planes.h"

namespace uno {

constexpr int RW_WAVES = RA_THREADS / 64;
constexpr int RW_NT = 2;        // 16-column MFMA tiles a wave keeps beside each other (they share the twiddle operand)

struct ResampleWide {
    static constexpr const char* name = "wide";
    __host__ __device__ static __forceinline__ int up(int n) { return (n + 7) & ~7; }

    // A wave owns 16 output rows x RW_NT tiles of 16 real columns; lane (i, k) = (lane & 15, lane >> 4) supplies the twiddle of
    // (row i, term k) and real column i of term k, and ends with rows 4 k ... 4 k + 3 of real column i, which it hands to
    // sink(row, real column, value) (rows >= n_out are not handed over).
    template <bool INV, class Sink>
    __device__ static __forceinline__ void complex_stage(const float2* in, int Lp, int n_out, int n_sum, const int* freq, const float2* tw, int N,
                                                         Sink sink) {
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
                    if (row < n_out) sink(row, (cg * RW_NT + nt) * 16 + i, acc[nt][r]);
                }
            }
        }
    }
};

void resample3d_wide_lds_bytes(int D1, int D2, int D3, int M1, int M2, int M3, int J1, int J2, int m3, size_t out[3]) {
    resample3d_lds_bytes<ResampleWide>(D1, D2, D3, M1, M2, M3, J1, J2, m3, out);
}

int launch_resample3d_wide(const float* x, float* y, float* y_act, int accumulate, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                           int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3, float scale,
                           int herm_in, int herm_out, hipStream_t s) {
    return launch_resample3d_planes<ResampleWide>(x, y, y_act, accumulate, ws, n_vol, D1, D2, D3, M1, M2, M3, J1, f1_in, f1_out, J2, f2_in, f2_out, m3,
                                                  scale, herm_in, herm_out, s);
}

}  // namespace uno
