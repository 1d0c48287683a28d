// K24 - the shell-binned energy spectrum of real H x W frames (and, with a target, of the target and of the difference) in one pass:
//
//   X[ky][kx] = (1 / HW) sum_{h, w} x[h][w] exp(-2 pi i (ky h / H + kx w / W)),   E(k) = sum_{round(hypot(ky, kx)) = k} |X[ky][kx]|^2
//
// over both Hermitian halves: the kernel forms the half spectrum kx = 0 ... W / 2 and weights column kx by 2, columns 0 and (even W)
// W / 2 by 1.  Stock ops make this rfft2 -> abs^2 -> weight -> index_add_: the complex spectrum goes to memory and comes back once per
// frame.  Here it never leaves the compute unit.
//
// One workgroup (4 waves) per (frame, band of SS_BW = 16 half-spectrum columns); the frame is addressed by four element strides
// (batch, frame, row, element), so (B, S, S, T), (B, T, S, S) and sub-sampled views are read where they lie.
//   stage A  C1[h][l] = sum_w x[h][w] cos(2 pi l w / W), S1[h][l] = sum_w x[h][w] sin(...) on the f32 MFMA: M = 16 rows of the frame,
//            N = the band's 16 columns, K = w; x straight from global memory (one guarded 16-byte or four 4-byte loads per lane and
//            16 columns, the next group in flight under the MFMAs), twiddles looked up in an LDS copy of the length-W table by a
//            wrapped running index.  The result goes to LDS as [h / 4][32][h % 4]: a lane's four accumulator rows are one 16-byte
//            store, and stage B's operand reads are 64 consecutive floats per wave.
//   stage B  Re X = sum_h (cos . C1 - sin . S1), -Im X = sum_h (cos . S1 + sin . C1) on the MFMA: M = 16 output rows ky, N = the band's
//            columns, K = h; with a target both transforms run on the same twiddle operand and X - Y is formed in registers (two
//            transforms per frame pair, never three).  |.|^2 times the Hermitian weight and 1 / (HW)^2 is parked in registers until
//            every wave is through stage B, then written OVER the stage-A buffer.
//   binning  thread k owns shell k: it adds that shell's modes of the band in the order of a host-built list (modes sorted by shell,
//            then row, then column; the shell decided in integers: (2k - 1)^2 <= 4 (ky^2 + kx^2) < (2k + 1)^2) and writes the band
//            partial to ws.  A second, small launch adds the bands in ascending order.
//
// No atomics; the decomposition is a function of (H, W) and of whether there is a target (never of B, the CU count or
// uno_reserve_cus), every sum has a fixed order and a frame's arithmetic does not depend on its batch: two calls, a call with CUs
// reserved and a graph replay give the same bits.  A frame is read ceil((W / 2 + 1) / 16) times, once per band; the workgroups of one
// frame have consecutive indices, so all reads after the first are served by L2 / the Infinity Cache (for a time-innermost tensor so
// are the other frames' reads of the cache lines a frame shares with them).
#include "uno_common.h"

#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

namespace uno {

enum { SS_THREADS = 256, SS_WAVES = 4, SS_BW = 16, SS_MAX_TILES = 8 };      // 8 tiles x 4 waves x 16 rows = 512 output rows

static int ss_shell(long long ky, long long kx) {        // round(hypot(ky, kx)) in integers: k = ceil(floor(sqrt(4 (ky^2 + kx^2))) / 2)
    const long long n = 4 * (ky * ky + kx * kx);
    long long m = (long long)std::sqrt((double)n);
    while (m * m > n) --m;
    while ((m + 1) * (m + 1) <= n) ++m;
    return (int)((m + 1) / 2);
}
int shell_spectrum_shells(int H, int W) { return ss_shell(H / 2, W / 2) + 1; }
int shell_spectrum_bands(int W) { return (W / 2 + 1 + SS_BW - 1) / SS_BW; }

struct SsTables { const unsigned short* perm; const int* off; };

// per (device, H, W): perm - for each band the entries (row * 16 + column in band) of its H x min(16, L - band0) modes sorted by shell,
// then row, then column; off [band][K + 1] - where each shell's run starts in perm
static bool ss_tables(int H, int W, SsTables* out) {
    static std::mutex mu;
    static std::map<std::tuple<int, int, int>, SsTables> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { set_error("hipGetDevice failed"); return false; }
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(std::make_tuple(dev, H, W));
    if (it != cache.end()) { *out = it->second; return true; }
    const int L = W / 2 + 1, K = shell_spectrum_shells(H, W), NB = shell_spectrum_bands(W);
    std::vector<unsigned short> perm((size_t)H * L);
    std::vector<int> off((size_t)NB * (K + 1));
    size_t at = 0;
    for (int band = 0; band < NB; ++band) {
        const int l0 = band * SS_BW, nl = L - l0 < SS_BW ? L - l0 : SS_BW;
        std::vector<int> count(K + 1, 0);
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < nl; ++c) ++count[ss_shell(r <= (H - 1) / 2 ? r : r - H, l0 + c) + 1];
        for (int k = 0; k < K; ++k) count[k + 1] += count[k];
        for (int k = 0; k <= K; ++k) off[(size_t)band * (K + 1) + k] = (int)at + count[k];
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < nl; ++c) perm[at + count[ss_shell(r <= (H - 1) / 2 ? r : r - H, l0 + c)]++] = (unsigned short)(r * SS_BW + c);
        at += (size_t)H * nl;
    }
    SsTables t;
    t.perm = static_cast<const unsigned short*>(upload_table(perm.data(), perm.size() * sizeof(unsigned short)));
    t.off = static_cast<const int*>(upload_table(off.data(), off.size() * sizeof(int)));
    if (!t.perm || !t.off) { set_error("shell_spectrum: table upload for %d x %d failed: %s", H, W, hipGetErrorString(hipGetLastError())); return false; }
    cache[std::make_tuple(dev, H, W)] = t;
    *out = t;
    return true;
}

struct SsView { const float* p; long long sb, sf, sr, se; };
struct SsParams {
    SsView x, y;
    float* ws;
    const float2* twH; const float2* twW;
    const unsigned short* perm; const int* off;
    int T, H, W, Hp, K, NB;
    float scale2;           // 1 / (H W)^2
};

// four elements w ... w + 3 of a frame row (zero beyond the row's end)
__device__ __forceinline__ float4 ss_load4(const float* row, bool row_ok, int w, int W, long long se) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!row_ok) return v;
    if (se == 1 && w + 3 < W) return io_ld4(row + w);
    if (w < W) v.x = row[(long long)w * se];
    if (w + 1 < W) v.y = row[(long long)(w + 1) * se];
    if (w + 2 < W) v.z = row[(long long)(w + 2) * se];
    if (w + 3 < W) v.w = row[(long long)(w + 3) * se];
    return v;
}
__device__ __forceinline__ float ss_pick(const float4& v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }

// grid: B * T * NB workgroups, workgroup g = (b * T + t) * NB + band; ws [B * T][NB][NSPEC][K]
template <int NSRC>
__global__ __launch_bounds__(SS_THREADS) void shell_spectrum_band_kernel(SsParams p) {
    constexpr int NSPEC = NSRC == 2 ? 3 : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = p.H, W = p.W, Hp = p.Hp, K = p.K;
    float2* stwH = reinterpret_cast<float2*>(smem);                                   // [H]
    float2* stwW = stwH + H;                                                            // [W]
    float* TA = reinterpret_cast<float*>(stwH + ((H + W + 1) & ~1));                    // [NSRC][Hp / 4][32][4]; later P [NSPEC][Hp][16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g4 = lane >> 4;
    const int band = (int)(blockIdx.x % (unsigned)p.NB);
    const long long ft = blockIdx.x / (unsigned)p.NB;
    const long long b = ft / p.T, t = ft % p.T;
    for (int n = tid; n < H; n += SS_THREADS) stwH[n] = p.twH[n];
    for (int n = tid; n < W; n += SS_THREADS) stwW[n] = p.twW[n];
    __syncthreads();

    const float* fr[NSRC];
    long long sr[NSRC], se[NSRC];
    fr[0] = p.x.p + b * p.x.sb + t * p.x.sf; sr[0] = p.x.sr; se[0] = p.x.se;
    if constexpr (NSRC == 2) { fr[1] = p.y.p + b * p.y.sb + t * p.y.sf; sr[1] = p.y.sr; se[1] = p.y.se; }

    // ---- stage A: 16-row tiles dealt round-robin to the waves
    {
        const int l = (band * SS_BW + j) % W;                      // the B operand's column (columns past W / 2 are computed and never read)
        const unsigned limW = (unsigned)W * 8u, inc = (unsigned)((16 * l) % W) * 8u;
        for (int ht = wave; ht < Hp / 16; ht += SS_WAVES) {
            const int h = ht * 16 + j;                             // the A operand's row; its columns: wc + 4 g4 + s
            const bool ok = h < H;
            const float* row[NSRC];
#pragma unroll
            for (int n = 0; n < NSRC; ++n) row[n] = fr[n] + (long long)(ok ? h : 0) * sr[n];
            unsigned idx[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) idx[s] = (unsigned)(((4 * g4 + s) * l) % W) * 8u;
            f32x4 accC[NSRC], accS[NSRC];
            float4 nxt[NSRC];
#pragma unroll
            for (int n = 0; n < NSRC; ++n) {
                accC[n] = f32x4{0.f, 0.f, 0.f, 0.f}; accS[n] = f32x4{0.f, 0.f, 0.f, 0.f};
                nxt[n] = ss_load4(row[n], ok, 4 * g4, W, se[n]);
            }
            for (int wc = 0; wc < W; wc += 16) {
                float4 cur[NSRC];
#pragma unroll
                for (int n = 0; n < NSRC; ++n) {
                    cur[n] = nxt[n];
                    nxt[n] = ss_load4(row[n], ok && wc + 16 < W, wc + 16 + 4 * g4, W, se[n]);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float2 tw = lds_tw(stwW, idx[s]);
                    idx[s] = wrap_add(idx[s], inc, limW);
#pragma unroll
                    for (int n = 0; n < NSRC; ++n) {
                        const float a = ss_pick(cur[n], s);
                        accC[n] = mfma16(a, tw.x, accC[n]);
                        accS[n] = mfma16(a, tw.y, accS[n]);
                    }
                }
            }
            // lane holds rows 16 ht + 4 g4 + r (r = 0 ... 3) of column j: [ht * 4 + g4][part * 16 + j][r]
#pragma unroll
            for (int n = 0; n < NSRC; ++n) {
                float* dst = TA + (((size_t)n * (Hp / 4) + ht * 4 + g4) * 32 + j) * 4;
                *reinterpret_cast<f32x4*>(dst) = accC[n];
                *reinterpret_cast<f32x4*>(dst + 64) = accS[n];
            }
        }
    }
    __syncthreads();

    // ---- stage B: 16-row tiles of the output rows ky, the results parked in registers
    float hold[SS_MAX_TILES][NSPEC * 4];
    {
        const int l = band * SS_BW + j;
        const float wt = p.scale2 * ((l == 0 || 2 * l == W) ? 1.f : 2.f);
        const unsigned limH = (unsigned)H * 8u;
#pragma unroll
        for (int i = 0; i < SS_MAX_TILES; ++i) {
            const int kt = wave + SS_WAVES * i;
            if (kt < Hp / 16) {
                const int r = (kt * 16 + j) % H;                   // the A operand's output row; its h: 4 hb + g4
                unsigned idx = (unsigned)((r * g4) % H) * 8u;
                const unsigned inc = (unsigned)((4 * r) % H) * 8u;
                f32x4 re[NSRC], im[NSRC];
#pragma unroll
                for (int n = 0; n < NSRC; ++n) { re[n] = f32x4{0.f, 0.f, 0.f, 0.f}; im[n] = f32x4{0.f, 0.f, 0.f, 0.f}; }
                const float* src = TA + j * 4 + g4;
                for (int hb = 0; hb < Hp / 4; ++hb) {
                    const float2 tw = lds_tw(stwH, idx);
                    idx = wrap_add(idx, inc, limH);
#pragma unroll
                    for (int n = 0; n < NSRC; ++n) {
                        const float c1 = src[((size_t)n * (Hp / 4) + hb) * 128], s1 = src[((size_t)n * (Hp / 4) + hb) * 128 + 64];
                        re[n] = mfma16(tw.x, c1, re[n]);
                        re[n] = mfma16(-tw.y, s1, re[n]);
                        im[n] = mfma16(tw.x, s1, im[n]);
                        im[n] = mfma16(tw.y, c1, im[n]);
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    hold[i][q] = (re[0][q] * re[0][q] + im[0][q] * im[0][q]) * wt;
                    if constexpr (NSRC == 2) {
                        const float yr = re[1][q], yi = im[1][q];
                        const float dr = re[0][q] - yr, di = im[0][q] - yi;
                        hold[i][4 + q] = (yr * yr + yi * yi) * wt;
                        hold[i][8 + q] = (dr * dr + di * di) * wt;
                    }
                }
            }
        }
    }
    __syncthreads();                                               // every wave is through with the stage-A buffer
    float* P = TA;                                                 // [NSPEC][Hp * 16]: row ky, column in band
#pragma unroll
    for (int i = 0; i < SS_MAX_TILES; ++i) {
        const int kt = wave + SS_WAVES * i;
        if (kt < Hp / 16) {
#pragma unroll
            for (int sp = 0; sp < NSPEC; ++sp)
#pragma unroll
                for (int q = 0; q < 4; ++q) P[(size_t)sp * Hp * 16 + (kt * 16 + 4 * g4 + q) * 16 + j] = hold[i][sp * 4 + q];
        }
    }
    __syncthreads();

    // ---- binning: thread k adds shell k's modes of this band in list order
    float* out = p.ws + ((size_t)blockIdx.x * NSPEC) * K;
    const int* off = p.off + (size_t)band * (K + 1);
    for (int k = tid; k < K; k += SS_THREADS) {
        const int i1 = off[k + 1];
        float e[NSPEC];
#pragma unroll
        for (int sp = 0; sp < NSPEC; ++sp) e[sp] = 0.f;
        for (int i = off[k]; i < i1; ++i) {
            const int m = p.perm[i];
#pragma unroll
            for (int sp = 0; sp < NSPEC; ++sp) e[sp] += P[(size_t)sp * Hp * 16 + m];
        }
#pragma unroll
        for (int sp = 0; sp < NSPEC; ++sp) out[(size_t)sp * K + k] = e[sp];
    }
}

// spec [n][k] = sum over the bands, ascending, of ws [n / NSPEC][band][n % NSPEC][k]
__global__ __launch_bounds__(SS_THREADS) void shell_spectrum_finish_kernel(const float* __restrict__ ws, float* __restrict__ spec, long long total,
                                                                           int K, int NB, int NSPEC) {
    const long long e = (long long)blockIdx.x * SS_THREADS + threadIdx.x;
    if (e >= total) return;
    const long long n = e / K;
    const int k = (int)(e % K);
    const float* src = ws + ((size_t)(n / NSPEC) * NB * NSPEC + (size_t)(n % NSPEC)) * K + k;
    float a = 0.f;
    for (int band = 0; band < NB; ++band) a += src[(size_t)band * NSPEC * K];
    spec[e] = a;
}

long long shell_spectrum_ws_floats(int B, int T, int H, int W, int with_target) {
    return (long long)B * T * shell_spectrum_bands(W) * (with_target ? 3 : 1) * shell_spectrum_shells(H, W);
}

int launch_shell_spectrum(const float* x, const long long xs[4], const float* y, const long long ys[4], float* spec, float* ws, int B, int T,
                          int H, int W, hipStream_t s) {
    SsParams p;
    p.T = T; p.H = H; p.W = W; p.Hp = (H + 15) / 16 * 16;
    p.K = shell_spectrum_shells(H, W); p.NB = shell_spectrum_bands(W);
    const long long groups = (long long)B * T * p.NB;
    const int nspec = y ? 3 : 1;
    const long long total = (long long)B * T * nspec * p.K;
    if (groups > 0x7fffffffLL || (total + SS_THREADS - 1) / SS_THREADS > 0x7fffffffLL) {
        set_error("shell_spectrum: %d x %d frames of %d x %d exceed the grid limit", B, T, H, W);
        return -2;
    }
    SsTables tab;
    if (!ss_tables(H, W, &tab)) return -4;
    p.perm = tab.perm; p.off = tab.off;
    p.twH = twiddle_table(H); p.twW = twiddle_table(W);
    if (!p.twH || !p.twW) return -4;
    p.x = SsView{x, xs[0], xs[1], xs[2], xs[3]};
    p.y = y ? SsView{y, ys[0], ys[1], ys[2], ys[3]} : SsView{nullptr, 0, 0, 0, 0};
    p.ws = ws;
    p.scale2 = (float)(1.0 / ((double)H * W * (double)H * W));
    const size_t lds = (size_t)((H + W + 1) & ~1) * 8 + (size_t)(y ? 2 : 1) * p.Hp * 32 * 4;
    static int slot1[64] = {0}, slot2[64] = {0};
    const void* kern = y ? (const void*)shell_spectrum_band_kernel<2> : (const void*)shell_spectrum_band_kernel<1>;
    if (!ensure_dynamic_lds(kern, lds, y ? slot2 : slot1)) { set_error("shell_spectrum: cannot raise the LDS limit to %zu bytes", lds); return -3; }
    {
        ProfScope prof("uno::shell_spectrum_band_kernel", 4.0 * B * T * (double)H * W * (y ? 2 : 1), s);
        if (y) hipLaunchKernelGGL(shell_spectrum_band_kernel<2>, dim3((unsigned)groups), dim3(SS_THREADS), lds, s, p);
        else hipLaunchKernelGGL(shell_spectrum_band_kernel<1>, dim3((unsigned)groups), dim3(SS_THREADS), lds, s, p);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("shell_spectrum band launch: %s", hipGetErrorString(e)); return -5; }
    {
        ProfScope prof("uno::shell_spectrum_finish_kernel", 4.0 * total * (p.NB + 1), s);
        hipLaunchKernelGGL(shell_spectrum_finish_kernel, dim3((unsigned)((total + SS_THREADS - 1) / SS_THREADS)), dim3(SS_THREADS), 0, s,
                           (const float*)ws, spec, total, p.K, p.NB, nspec);
    }
    e = hipGetLastError();
    if (e != hipSuccess) { set_error("shell_spectrum finish launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

}  // namespace uno
