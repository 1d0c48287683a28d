// K25 - the relative Sobolev (H^s) loss of real H x W frames x against targets y, forward and backward.  With X = fft2(x) / (HW), integer
// wavenumbers in fftfreq order and a caller-supplied weight table w2 (H / 2 + 1, W / 2 + 1) read at (|ky|, |kx|):
//
//   sums[b][t] = [ num, den ] = [ sum_k w2(k) |X - Y|^2(k),  sum_k w2(k) |Y|^2(k) ]          over both Hermitian halves
//   ratio      = sqrt(num) / sqrt(den) per frame (per_frame) or of the sums over a sample's frames;  total = sum of ratio
//   gx[b][t]   = g * scale * f / (HW sqrt(num den)),  f = sum_k Z(k) e^{+2 pi i (ky h / H + kx w / W)},  Z = w2 (X - Y);  0 where num == 0
//
// Stock ops make the forward rfft2 -> weight -> abs^2 -> sums and leave autograd an irfft2 chain: about a dozen launches, the complex
// spectrum to memory and back twice.
//
// Forward: K24's band kernel (shell_spectrum.hip) with a weighted sum where that one bins.  One workgroup (4 waves) per (frame, band
// of SB_BW = 16 half-spectrum columns); the frame pair is addressed by four element strides each (batch, frame, row, element).
//   stage A  C1[h][l] = sum_w x[h][w] cos(2 pi l w / W), S1 likewise with sin, on the f32 MFMA (M = 16 frame rows, N = the band's columns,
//            K = w), x and y straight from global memory, the result in LDS as [h / 4][32][h % 4].
//   stage B  Re X = sum_h (cos . C1 - sin . S1), -Im X = sum_h (cos . S1 + sin . C1) on the MFMA (M = 16 rows ky, K = h) for both frames on one
//            twiddle operand; X - Y in registers.  Each lane adds herm(kx) w2 |.|^2 of its modes in tile order, the lanes of a wave are
//            added by xor shuffles, the waves in ascending order: ws[frame][band] = (num, den).  With a spectrum buffer the same pass
//            stores Z per frame as a dense half spectrum (H, W / 2 + 1) complex; without one (no gradient wanted) nothing but the two
//            partial sums leaves the compute unit.
//   finish   one workgroup: the bands of a frame added in ascending order in double and rounded once -> sums; ratio and total for
//            the chosen grouping (a sample's frames in ascending order, in double).
// Backward: one launch, the same two stages with space and spectrum exchanged.  One workgroup per (frame, band of 16 output columns).
//   stage 1  G[ky][w] = sum_kx herm(kx) Z[ky][kx] e^{+2 pi i kx w / W} on the MFMA (M = 16 rows ky, N = the band's columns, K = kx over the
//            whole half spectrum), Z from global memory, G to LDS in stage A's layout.
//   stage 2  f[h][w] = sum_ky (Re G cos(2 pi ky h / H) - Im G sin(...)) on the MFMA (M = 16 rows h, K = ky), times the coefficient - computed
//            from sums and the device-resident g, which holds one value or one per row of the grouping - and written through gx's four
//            element strides: a (B, S, S, T) gradient is written where it lies.
//
// Contract (K24's): float32 only; strides >= 0, nothing copied; 8 <= H, W <= 512, odd sizes included (the inverse kernel holds 512 points a
// side in 72 KB of LDS, the forward one in 136 KB: the range is not narrowed); T >= 1, B >= 0; 64-bit offsets; no atomics; the decomposition
// is a function of (H, W) only (never of B, the CU count or uno_reserve_cus); every sum has a fixed order and a frame's arithmetic does not
// depend on its batch: two calls, a call with CUs reserved and a graph replay give the same bits.  No synchronisation, allocation or
// read-back; the twiddle tables go through upload_table (a first call inside a graph capture works); w2 is the caller's device table.
// No clamping: a zero target gives +inf (NaN for 0 / 0) as the stock form does.
#include "uno_common.h"

namespace uno {

enum { SB_THREADS = 256, SB_WAVES = 4, SB_BW = 16, SB_MAX_TILES = 8 };      // 8 tiles x 4 waves x 16 rows = 512 rows

int sobolev_bands(int W) { return (W / 2 + 1 + SB_BW - 1) / SB_BW; }         // forward: bands of half-spectrum columns
static int sobolev_out_bands(int W) { return (W + SB_BW - 1) / SB_BW; }       // backward: bands of output columns
long long sobolev_ws_floats(int B, int T, int W) { return 2LL * B * T * sobolev_bands(W); }

struct SbView { const float* p; long long sb, sf, sr, se; };
struct SbFwdParams {
    SbView x, y;
    const float* w2;        // (H / 2 + 1, W / 2 + 1)
    float2* ws;             // [B * T][NB] (num, den)
    float2* z;              // [B * T][H][W / 2 + 1] or nullptr
    const float2* twH; const float2* twW;
    int T, H, W, Hp, NB;
    float inv;              // 1 / (H W)
};

// four elements w ... w + 3 of a frame row (zero beyond the row's end)
__device__ __forceinline__ float4 sb_load4(const float* row, bool row_ok, int w, int W, long long se) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!row_ok) return v;
    if (se == 1 && w + 3 < W) return io_ld4(row + w);
    if (w < W) v.x = row[(long long)w * se];
    if (w + 1 < W) v.y = row[(long long)(w + 1) * se];
    if (w + 2 < W) v.z = row[(long long)(w + 2) * se];
    if (w + 3 < W) v.w = row[(long long)(w + 3) * se];
    return v;
}
__device__ __forceinline__ float sb_pick(const float4& v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }

__device__ __forceinline__ float sb_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);      // a + b = b + a: every lane ends with the same bits
    return v;
}
__device__ __forceinline__ double sb_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// grid: B * T * NB workgroups, workgroup g = (b * T + t) * NB + band
__global__ __launch_bounds__(SB_THREADS) void sobolev_band_kernel(SbFwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = p.H, W = p.W, Hp = p.Hp, L = W / 2 + 1;
    float2* stwH = reinterpret_cast<float2*>(smem);                                   // [H]
    float2* stwW = stwH + H;                                                            // [W]
    float* TA = reinterpret_cast<float*>(stwH + ((H + W + 1) & ~1));                    // [2][Hp / 4][32][4]
    float* s_part = TA + (size_t)2 * Hp * 32;                                           // [SB_WAVES][2] (no static LDS: the dynamic limit is the hardware's)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g4 = lane >> 4;
    const int band = (int)(blockIdx.x % (unsigned)p.NB);
    const long long ft = blockIdx.x / (unsigned)p.NB;
    const long long b = ft / p.T, t = ft % p.T;
    for (int n = tid; n < H; n += SB_THREADS) stwH[n] = p.twH[n];
    for (int n = tid; n < W; n += SB_THREADS) stwW[n] = p.twW[n];
    __syncthreads();

    const float* fr[2];
    long long sr[2], se[2];
    fr[0] = p.x.p + b * p.x.sb + t * p.x.sf; sr[0] = p.x.sr; se[0] = p.x.se;
    fr[1] = p.y.p + b * p.y.sb + t * p.y.sf; sr[1] = p.y.sr; se[1] = p.y.se;

    // ---- stage A: 16-row tiles dealt round-robin to the waves
    {
        const int l = (band * SB_BW + j) % W;                      // the B operand's column (columns past W / 2 are computed and never used)
        const unsigned limW = (unsigned)W * 8u, inc = (unsigned)((16 * l) % W) * 8u;
        for (int ht = wave; ht < Hp / 16; ht += SB_WAVES) {
            const int h = ht * 16 + j;                             // the A operand's row; its columns: wc + 4 g4 + s
            const bool ok = h < H;
            const float* row[2];
#pragma unroll
            for (int n = 0; n < 2; ++n) row[n] = fr[n] + (long long)(ok ? h : 0) * sr[n];
            unsigned idx[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) idx[s] = (unsigned)(((4 * g4 + s) * l) % W) * 8u;
            f32x4 accC[2], accS[2];
            float4 nxt[2];
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                accC[n] = f32x4{0.f, 0.f, 0.f, 0.f}; accS[n] = f32x4{0.f, 0.f, 0.f, 0.f};
                nxt[n] = sb_load4(row[n], ok, 4 * g4, W, se[n]);
            }
            for (int wc = 0; wc < W; wc += 16) {
                float4 cur[2];
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    cur[n] = nxt[n];
                    nxt[n] = sb_load4(row[n], ok && wc + 16 < W, wc + 16 + 4 * g4, W, se[n]);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float2 tw = lds_tw(stwW, idx[s]);
                    idx[s] = wrap_add(idx[s], inc, limW);
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const float a = sb_pick(cur[n], s);
                        accC[n] = mfma16(a, tw.x, accC[n]);
                        accS[n] = mfma16(a, tw.y, accS[n]);
                    }
                }
            }
            // lane holds rows 16 ht + 4 g4 + r (r = 0 ... 3) of column j: [ht * 4 + g4][part * 16 + j][r]
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                float* dst = TA + (((size_t)n * (Hp / 4) + ht * 4 + g4) * 32 + j) * 4;
                *reinterpret_cast<f32x4*>(dst) = accC[n];
                *reinterpret_cast<f32x4*>(dst + 64) = accS[n];
            }
        }
    }
    __syncthreads();

    // ---- stage B: 16-row tiles of the output rows ky; each lane adds its weighted modes in tile order
    float num = 0.f, den = 0.f;
    {
        const int l = band * SB_BW + j;
        const bool col_ok = l < L;
        const float herm = (l == 0 || 2 * l == W) ? 1.f : 2.f;
        const unsigned limH = (unsigned)H * 8u;
        float2* zf = p.z ? p.z + (size_t)ft * H * L : nullptr;
#pragma unroll 1
        for (int kt = wave; kt < Hp / 16; kt += SB_WAVES) {
            const int r = (kt * 16 + j) % H;                       // the A operand's output row; its h: 4 hb + g4
            unsigned idx = (unsigned)((r * g4) % H) * 8u;
            const unsigned inc = (unsigned)((4 * r) % H) * 8u;
            f32x4 re[2], im[2];
#pragma unroll
            for (int n = 0; n < 2; ++n) { re[n] = f32x4{0.f, 0.f, 0.f, 0.f}; im[n] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            const float* src = TA + j * 4 + g4;
            for (int hb = 0; hb < Hp / 4; ++hb) {
                const float2 tw = lds_tw(stwH, idx);
                idx = wrap_add(idx, inc, limH);
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const float c1 = src[((size_t)n * (Hp / 4) + hb) * 128], s1 = src[((size_t)n * (Hp / 4) + hb) * 128 + 64];
                    re[n] = mfma16(tw.x, c1, re[n]);
                    re[n] = mfma16(-tw.y, s1, re[n]);
                    im[n] = mfma16(tw.x, s1, im[n]);
                    im[n] = mfma16(tw.y, c1, im[n]);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ky = kt * 16 + 4 * g4 + q;               // the lane's own output row
                if (col_ok && ky < H) {
                    const float w = p.w2[(size_t)(ky < H - ky ? ky : H - ky) * L + l];
                    const float yr = re[1][q] * p.inv, yi = im[1][q] * p.inv;
                    const float dr = re[0][q] * p.inv - yr, di = im[0][q] * p.inv - yi;
                    num += herm * w * (dr * dr + di * di);
                    den += herm * w * (yr * yr + yi * yi);
                    if (zf) zf[(size_t)ky * L + l] = make_float2(w * dr, -(w * di));       // im holds -Im
                }
            }
        }
    }
    num = sb_wave_sum(num);
    den = sb_wave_sum(den);
    if (lane == 0) { s_part[2 * wave] = num; s_part[2 * wave + 1] = den; }
    __syncthreads();
    if (tid == 0) {
        float a = 0.f, d = 0.f;
#pragma unroll
        for (int w = 0; w < SB_WAVES; ++w) { a += s_part[2 * w]; d += s_part[2 * w + 1]; }
        p.ws[blockIdx.x] = make_float2(a, d);
    }
}

// one workgroup.  A thread per row of the grouping (a frame, or a sample): the bands of each of its frames in ascending order in double,
// rounded once -> sums; the row's frames in ascending order in double, rounded once -> ratio; total = sum of ratio in double (rows in
// ascending order per thread, xor-shuffle wave sums, waves in ascending order), rounded once
__global__ __launch_bounds__(SB_THREADS) void sobolev_finish_kernel(const float2* __restrict__ ws, float* __restrict__ sums,
                                                                    float* __restrict__ ratio, float* __restrict__ total, long long rows,
                                                                    int frames_per_row, int NB) {
    __shared__ double s_tot[SB_THREADS / 64];
    const int tid = threadIdx.x;
    double tot = 0.0;
    for (long long row = tid; row < rows; row += SB_THREADS) {
        double gn = 0.0, gd = 0.0;
        for (int t = 0; t < frames_per_row; ++t) {
            const long long ft = row * frames_per_row + t;
            const float2* p = ws + (size_t)ft * NB;
            double dn = 0.0, dd = 0.0;
            for (int c = 0; c < NB; ++c) { dn += (double)p[c].x; dd += (double)p[c].y; }
            const float fn = (float)dn, fd = (float)dd;
            sums[2 * ft] = fn;
            sums[2 * ft + 1] = fd;
            gn += (double)fn; gd += (double)fd;
        }
        const float r = sqrtf((float)gn) / sqrtf((float)gd);
        ratio[row] = r;
        tot += (double)r;
    }
    tot = sb_wave_sum(tot);
    if ((tid & 63) == 0) s_tot[tid >> 6] = tot;
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < SB_THREADS / 64; ++w) a += s_tot[w];
        total[0] = (float)a;
    }
}

struct SbBwdParams {
    const float2* z;        // [B * T][H][W / 2 + 1]
    const float* sums;      // (B, T, 2)
    const float* g;
    float* gx; long long sb, sf, sr, se;
    const float2* twH; const float2* twW;
    int T, H, W, Hp, NB, per_frame, g_per_row;
    float scale;            // the caller's scale / (H W)
};

// grid: B * T * NB workgroups, workgroup g = (b * T + t) * NB + band of 16 output columns
__global__ __launch_bounds__(SB_THREADS) void sobolev_backward_kernel(SbBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = p.H, W = p.W, Hp = p.Hp, L = W / 2 + 1;
    float2* stwH = reinterpret_cast<float2*>(smem);                                   // [H]
    float2* stwW = stwH + H;                                                            // [W]
    float* TG = reinterpret_cast<float*>(stwH + ((H + W + 1) & ~1));                    // [Hp / 4][32][4]: Re G | Im G
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g4 = lane >> 4;
    const int band = (int)(blockIdx.x % (unsigned)p.NB);
    const long long ft = blockIdx.x / (unsigned)p.NB;
    const long long b = ft / p.T, t = ft % p.T;
    for (int n = tid; n < H; n += SB_THREADS) stwH[n] = p.twH[n];
    for (int n = tid; n < W; n += SB_THREADS) stwW[n] = p.twW[n];
    __syncthreads();

    // the coefficient: the frame's own sums, or those of the sample's frames added as the finish kernel adds them
    float coef;
    {
        float num, den;
        if (p.per_frame) { num = p.sums[2 * ft]; den = p.sums[2 * ft + 1]; }
        else {
            double gn = 0.0, gd = 0.0;
            for (int u = 0; u < p.T; ++u) { gn += (double)p.sums[2 * (b * p.T + u)]; gd += (double)p.sums[2 * (b * p.T + u) + 1]; }
            num = (float)gn; den = (float)gd;
        }
        const float gv = p.g[p.g_per_row ? (p.per_frame ? ft : b) : 0];
        coef = num == 0.f ? 0.f : gv * p.scale / (sqrtf(num) * sqrtf(den));
    }

    const int wcol = band * SB_BW + j;                             // the lane's output column
    const float2* zf = p.z + (size_t)ft * H * L;
    // ---- stage 1: 16-row tiles of the spectrum rows ky dealt round-robin to the waves; K = kx in groups of 16, padded with zeros
    {
        const int l = wcol % W;
        const unsigned limW = (unsigned)W * 8u, inc = (unsigned)((16 * l) % W) * 8u;
        for (int kt = wave; kt < Hp / 16; kt += SB_WAVES) {
            const int ky = kt * 16 + j;                            // the A operand's row; its columns kx: kc + 4 g4 + s
            const bool ok = ky < H;
            const float2* row = zf + (size_t)(ok ? ky : 0) * L;
            unsigned idx[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) idx[s] = (unsigned)(((4 * g4 + s) * l) % W) * 8u;
            f32x4 gr = f32x4{0.f, 0.f, 0.f, 0.f}, gi = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int kc = 0; kc < L; kc += 16) {
                float2 zv[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int kx = kc + 4 * g4 + s;
                    zv[s] = make_float2(0.f, 0.f);
                    if (ok && kx < L) {
                        const float2 v = row[kx];
                        const float hw = (kx == 0 || 2 * kx == W) ? 1.f : 2.f;
                        zv[s] = make_float2(hw * v.x, hw * v.y);
                    }
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float2 tw = lds_tw(stwW, idx[s]);
                    idx[s] = wrap_add(idx[s], inc, limW);
                    gr = mfma16(zv[s].x, tw.x, gr);
                    gr = mfma16(-zv[s].y, tw.y, gr);
                    gi = mfma16(zv[s].x, tw.y, gi);
                    gi = mfma16(zv[s].y, tw.x, gi);
                }
            }
            float* dst = TG + ((size_t)(kt * 4 + g4) * 32 + j) * 4;
            *reinterpret_cast<f32x4*>(dst) = gr;
            *reinterpret_cast<f32x4*>(dst + 64) = gi;
        }
    }
    __syncthreads();

    // ---- stage 2: 16-row tiles of the output rows h
    {
        const unsigned limH = (unsigned)H * 8u;
        float* out = p.gx + b * p.sb + t * p.sf + (long long)wcol * p.se;
        for (int ht = wave; ht < Hp / 16; ht += SB_WAVES) {
            const int r = (ht * 16 + j) % H;                       // the A operand's output row; its ky: 4 kb + g4
            unsigned idx = (unsigned)((r * g4) % H) * 8u;
            const unsigned inc = (unsigned)((4 * r) % H) * 8u;
            f32x4 f = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* src = TG + j * 4 + g4;
            for (int kb = 0; kb < Hp / 4; ++kb) {
                const float2 tw = lds_tw(stwH, idx);
                idx = wrap_add(idx, inc, limH);
                const float cr = src[(size_t)kb * 128], ci = src[(size_t)kb * 128 + 64];
                f = mfma16(tw.x, cr, f);
                f = mfma16(-tw.y, ci, f);
            }
            if (wcol < W) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int h = ht * 16 + 4 * g4 + q;
                    if (h < H) out[(long long)h * p.sr] = coef * f[q];
                }
            }
        }
    }
}

static size_t sb_lds(int H, int W, int planes) { return (size_t)((H + W + 1) & ~1) * 8 + (size_t)planes * ((H + 15) / 16 * 16) * 32 * 4; }

int launch_sobolev_forward(const float* x, const long long xs[4], const float* y, const long long ys[4], const float* w2, float* sums, float* ratio,
                           float* total, float* z, float* ws, int B, int T, int H, int W, int per_frame, hipStream_t s) {
    SbFwdParams p;
    p.T = T; p.H = H; p.W = W; p.Hp = (H + 15) / 16 * 16; p.NB = sobolev_bands(W);
    const long long groups = (long long)B * T * p.NB;
    if (groups > 0x7fffffffLL) { set_error("sobolev_forward: %d x %d frames of %d x %d exceed the grid limit", B, T, H, W); return -2; }
    p.twH = twiddle_table(H); p.twW = twiddle_table(W);
    if (!p.twH || !p.twW) return -4;
    p.x = SbView{x, xs[0], xs[1], xs[2], xs[3]};
    p.y = SbView{y, ys[0], ys[1], ys[2], ys[3]};
    p.w2 = w2; p.ws = reinterpret_cast<float2*>(ws); p.z = reinterpret_cast<float2*>(z);
    p.inv = (float)(1.0 / ((double)H * W));
    const size_t lds = sb_lds(H, W, 2) + 2 * SB_WAVES * sizeof(float);
    static int slot[64] = {0};
    if (!ensure_dynamic_lds((const void*)sobolev_band_kernel, lds, slot)) { set_error("sobolev_forward: cannot raise the LDS limit to %zu bytes", lds); return -3; }
    {
        ProfScope prof("uno::sobolev_band_kernel", 8.0 * B * T * (double)H * W + (z ? 8.0 * B * T * (double)H * (W / 2 + 1) : 0.0), s);
        hipLaunchKernelGGL(sobolev_band_kernel, dim3((unsigned)groups), dim3(SB_THREADS), lds, s, p);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("sobolev_forward band launch: %s", hipGetErrorString(e)); return -5; }
    {
        ProfScope prof("uno::sobolev_finish_kernel", 8.0 * groups, s);
        hipLaunchKernelGGL(sobolev_finish_kernel, dim3(1), dim3(SB_THREADS), 0, s, (const float2*)ws, sums, ratio, total,
                           per_frame ? (long long)B * T : (long long)B, per_frame ? 1 : T, p.NB);
    }
    e = hipGetLastError();
    if (e != hipSuccess) { set_error("sobolev_forward finish launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

int launch_sobolev_backward(const float* z, const float* sums, const float* g, int g_per_row, float scale, int per_frame, float* gx,
                            const long long gs[4], int B, int T, int H, int W, hipStream_t s) {
    SbBwdParams p;
    p.T = T; p.H = H; p.W = W; p.Hp = (H + 15) / 16 * 16; p.NB = sobolev_out_bands(W);
    const long long groups = (long long)B * T * p.NB;
    if (groups > 0x7fffffffLL) { set_error("sobolev_backward: %d x %d frames of %d x %d exceed the grid limit", B, T, H, W); return -2; }
    p.twH = twiddle_table(H); p.twW = twiddle_table(W);
    if (!p.twH || !p.twW) return -4;
    p.z = reinterpret_cast<const float2*>(z); p.sums = sums; p.g = g;
    p.gx = gx; p.sb = gs[0]; p.sf = gs[1]; p.sr = gs[2]; p.se = gs[3];
    p.per_frame = per_frame; p.g_per_row = g_per_row;
    p.scale = (float)((double)scale / ((double)H * W));
    const size_t lds = sb_lds(H, W, 1);
    static int slot[64] = {0};
    if (!ensure_dynamic_lds((const void*)sobolev_backward_kernel, lds, slot)) { set_error("sobolev_backward: cannot raise the LDS limit to %zu bytes", lds); return -3; }
    {
        ProfScope prof("uno::sobolev_backward_kernel", 4.0 * B * T * (double)H * W + 8.0 * B * T * (double)H * (W / 2 + 1), s);
        hipLaunchKernelGGL(sobolev_backward_kernel, dim3((unsigned)groups), dim3(SB_THREADS), lds, s, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("sobolev_backward launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

}  // namespace uno
