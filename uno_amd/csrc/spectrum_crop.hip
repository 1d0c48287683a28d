// Corner crop of truncated spectra: the (2 m1, m2) corner blocks of a (2 M1, M2) truncated spectrum, m1 <= M1, m2 <= M2.
//
// A truncated spectrum holds the first M1 rows of the full one (frequencies 0 .. M1 - 1) followed by its last M1 rows (frequencies
// -M1 .. -1) and the first M2 columns.  The truncation to fewer modes is a subset of it: lo rows 0 .. m1 - 1, the LAST m1 rows of the
// hi corner, columns 0 .. m2 - 1.  A tensor that two spectral layers transform on the same grid (a skip connection) is therefore
// transformed once, at the larger mode counts, and the layer with fewer modes copies its part (block2d.py, SpectrumShare): a few
// megabytes moved instead of a second pass over the images.  One thread per complex element of the destination.
#include "uno_common.h"

namespace uno {

struct SpectrumCropParams {
    const float2* src; float2* dst;
    long long total;                    // n_img * 2 m1 * m2
    int M1, M2, m1, m2;
    int s_group, s_stride, s_offset;    // spectrum of image i lives at index (i / group) * stride + offset + i % group (Dft2dParams)
    int d_group, d_stride, d_offset;
};

__global__ __launch_bounds__(256) void spectrum_crop_kernel(SpectrumCropParams p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.total) return;
    const int per = 2 * p.m1 * p.m2;
    const int img = (int)(idx / per);
    const int e = (int)(idx - (long long)img * per);
    const int r = e / p.m2, c = e - r * p.m2;
    const int sr = r < p.m1 ? r : r + 2 * (p.M1 - p.m1);         // hi corner: its last m1 rows
    const size_t si = (size_t)(img / p.s_group) * p.s_stride + p.s_offset + img % p.s_group;
    const size_t di = (size_t)(img / p.d_group) * p.d_stride + p.d_offset + img % p.d_group;
    p.dst[di * per + e] = p.src[(si * (2 * p.M1) + sr) * p.M2 + c];
}

int launch_spectrum_crop(const float* src, float* dst, int n_img, int M1, int M2, int m1, int m2, int s_group, int s_stride, int s_offset,
                         int d_group, int d_stride, int d_offset, hipStream_t s) {
    SpectrumCropParams p;
    p.src = reinterpret_cast<const float2*>(src); p.dst = reinterpret_cast<float2*>(dst);
    p.total = (long long)n_img * 2 * m1 * m2;
    p.M1 = M1; p.M2 = M2; p.m1 = m1; p.m2 = m2;
    p.s_group = s_group; p.s_stride = s_stride; p.s_offset = s_offset;
    p.d_group = d_group; p.d_stride = d_stride; p.d_offset = d_offset;
    const long long blocks = (p.total + 255) / 256;
    if (blocks > 0x7fffffffLL) { set_error("spectrum_crop: %lld elements are more than one launch takes", p.total); return -1; }
    {
        ProfScope prof("uno::spectrum_crop_kernel", 2.0 * (double)p.total * 8.0, s);
        hipLaunchKernelGGL(spectrum_crop_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("spectrum_crop launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

}  // namespace uno
