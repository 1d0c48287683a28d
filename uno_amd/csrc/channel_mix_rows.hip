// K21: channel-mix layers on SHORT-ROW windows - the two ends of the NS-3D models (fc1 on the un-built skip concatenation with the
// time-axis crop, the lift's second layer with its activation and time-axis padding), forward and backward, and their C entry points.
//
// A short-row window is rows x cols logical pixels; logical pixel (r, c) lives at element r * pitch + col0 + c of its channel plane,
// planes are `plane` elements apart.  For a (B, C, H, W, Tp) tensor rows = H * W and pitch = Tp: the window is along the LAST axis,
// 9 .. 40 kept time steps of 10 .. 52, of any parity and starting at any column - outside what the pixel windows of uno_common.h take
// (image rows: cols % 4 == 0, cols >= 260, window in the corner).  Limits: col0 + cols <= pitch <= 256, rows * pitch < 2^24: a lane
// finds its row with one multiply (q / d = (q * ceil(2^40 / d)) >> 40 exactly while q * d < 2^40).
//
// Lanes map to CONSECUTIVE elements: of the dense side where a kernel reads a window (a wave's 64 reads of a windowed plane are then
// 64 consecutive kept elements, i.e. runs of `cols` contiguous floats with pitch - cols skipped between runs), of the PHYSICAL plane
// where a kernel writes one (whole rows are stored, the border columns as +0.0f from the same store: no clearing launch).  The weights
// are wave-uniform and come through the scalar cache; a wave owns a tile of RM_TO output channels for RM_PX x 64 elements and the waves
// of a workgroup share the element tile (its re-reads for the other output tiles hit the CU's L1).  Products are k-ordered fmaf chains
// in float32.  Launch geometry: a function of the shape alone.
#include "../../include/uno_spectral.h"
#include "uno_common.h"

namespace uno {
namespace {

constexpr int RM_TO = 16;        // output channels per wave tile
constexpr int RM_PX = 4;         // elements per lane (64 apart)

struct RowsGeom {
    int rows, cols, pitch, col0;
    long long plane;
    int P, E;                            // rows * cols logical pixels, rows * pitch physical elements
    unsigned long long mcols, mpitch;    // ceil(2^40 / cols), ceil(2^40 / pitch)
};
__device__ __forceinline__ int rows_div(int n, unsigned long long magic) { return (int)(((unsigned long long)(unsigned)n * magic) >> 40); }

enum { RM_FWD = 0, RM_GRAD = 1, RM_ACTPAD = 2 };
// out[n] = sum_k W(n, k) in[k] (+ bias[n]) for reduction channels [0, K1) of in1, [K1, K) of in2 and output channels [0, N1) -> out1,
// [N1, N) -> out2.
// RM_FWD:    lanes over logical pixels; in on the window, out1 dense; W(n, k) = w[n * Ci + k]
// RM_GRAD:   lanes over physical elements; in dense, out1 / out2 whole rows of planes (border +0); W(n, k) = w[k * Ci + n];
//            dgelu_of (on out1's window) multiplies out1 by gelu'
// RM_ACTPAD: lanes over physical elements; in dense, out1 dense (may be null), out_act = gelu(out) on dense planes of E elements
struct RowsMixParams {
    const float* in1; const float* in2; const float* w; const float* bias;
    float* out1; float* out2; float* out_act; const float* dgelu_of;
    int K1, K, N1, N, Ci, act_in, ntiles, wp, wc;
    RowsGeom g;
};

template <int MODE, bool FULL>
__device__ __forceinline__ void rows_mix_tile(const RowsMixParams& p, const float* in1b, const float* in2b, long long in_plane, int n0,
                                              const int (&ioff)[RM_PX], const bool (&live)[RM_PX], float (&acc)[RM_PX][RM_TO]) {
    const int nmax = p.N - 1;
#pragma unroll
    for (int o = 0; o < RM_TO; ++o) {
        const int n = FULL ? n0 + o : min(n0 + o, nmax);
        const float bv = (MODE != RM_GRAD && p.bias) ? p.bias[n] : 0.f;
#pragma unroll
        for (int j = 0; j < RM_PX; ++j) acc[j][o] = bv;
    }
    for (int k = 0; k < p.K; ++k) {
        const float* src = k < p.K1 ? in1b + (long long)k * in_plane : in2b + (long long)(k - p.K1) * in_plane;
        float x[RM_PX];
#pragma unroll
        for (int j = 0; j < RM_PX; ++j) x[j] = live[j] ? src[ioff[j]] : 0.f;
        if (MODE != RM_GRAD && p.act_in && k < p.K1) {
#pragma unroll
            for (int j = 0; j < RM_PX; ++j) x[j] = uno_gelu(x[j]);
        }
#pragma unroll
        for (int o = 0; o < RM_TO; ++o) {
            const int n = FULL ? n0 + o : min(n0 + o, nmax);
            const float wv = MODE == RM_GRAD ? p.w[(long long)k * p.Ci + n] : p.w[(long long)n * p.Ci + k];
#pragma unroll
            for (int j = 0; j < RM_PX; ++j) acc[j][o] = fmaf(wv, x[j], acc[j][o]);
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void rows_mix_kernel(const RowsMixParams p) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int pw = wave % p.wp, cw = wave / p.wp;
    const long long b = blockIdx.x / (unsigned)p.ntiles;
    const int t = blockIdx.x % (unsigned)p.ntiles;
    const RowsGeom& g = p.g;
    const int L = MODE == RM_FWD ? g.P : g.E;
    int item[RM_PX], ioff[RM_PX], pix[RM_PX];
    bool live[RM_PX], inrange[RM_PX];
#pragma unroll
    for (int j = 0; j < RM_PX; ++j) {
        item[j] = ((t * p.wp + pw) * RM_PX + j) * 64 + lane;
        inrange[j] = item[j] < L;
        const int it = inrange[j] ? item[j] : 0;
        if (MODE == RM_FWD) {
            const int r = rows_div(it, g.mcols), c = it - r * g.cols;
            ioff[j] = r * g.pitch + g.col0 + c;
            pix[j] = it;
            live[j] = inrange[j];
        } else {
            const int r = rows_div(it, g.mpitch), c = it - r * g.pitch - g.col0;
            live[j] = inrange[j] && c >= 0 && c < g.cols;
            pix[j] = live[j] ? r * g.cols + c : 0;
            ioff[j] = pix[j];
        }
    }
    const long long in_plane = MODE == RM_FWD ? g.plane : (long long)g.P;
    const float* in1b = p.in1 + b * p.K1 * in_plane;
    const float* in2b = p.in2 ? p.in2 + b * (p.K - p.K1) * in_plane : p.in1;
    const int nt = (p.N + RM_TO - 1) / RM_TO;
    for (int ot = cw; ot < nt; ot += p.wc) {
        const int n0 = ot * RM_TO;
        float acc[RM_PX][RM_TO];
        if (n0 + RM_TO <= p.N) rows_mix_tile<MODE, true>(p, in1b, in2b, in_plane, n0, ioff, live, acc);
        else rows_mix_tile<MODE, false>(p, in1b, in2b, in_plane, n0, ioff, live, acc);
#pragma unroll
        for (int o = 0; o < RM_TO; ++o) {
            const int n = n0 + o;
            if (n >= p.N) break;
            if (MODE == RM_FWD) {
                float* dst = p.out1 + (b * p.N + n) * (long long)g.P;
#pragma unroll
                for (int j = 0; j < RM_PX; ++j)
                    if (live[j]) dst[pix[j]] = acc[j][o];
            } else if (MODE == RM_GRAD) {
                const bool first = n < p.N1;
                const long long off = first ? (b * p.N1 + n) * g.plane : (b * (p.N - p.N1) + (n - p.N1)) * g.plane;
                float* dst = (first ? p.out1 : p.out2) + off;
                const float* dg = (first && p.dgelu_of) ? p.dgelu_of + off : nullptr;
#pragma unroll
                for (int j = 0; j < RM_PX; ++j) {
                    if (!inrange[j]) continue;
                    float v = 0.f;
                    if (live[j]) v = dg ? acc[j][o] * uno_dgelu(dg[item[j]]) : acc[j][o];
                    dst[item[j]] = v;
                }
            } else {
                float* dst = p.out1 ? p.out1 + (b * p.N + n) * (long long)g.P : nullptr;
                float* dact = p.out_act + (b * p.N + n) * (long long)g.E;
#pragma unroll
                for (int j = 0; j < RM_PX; ++j) {
                    if (!inrange[j]) continue;
                    if (live[j] && dst) dst[pix[j]] = acc[j][o];
                    dact[item[j]] = live[j] ? uno_gelu(acc[j][o]) : 0.f;
                }
            }
        }
    }
}

// gz[n][q] = gelu'(pre[n][q]) * g[n][window(q)] for n_planes planes; one workgroup per 1024 logical pixels of a plane
__global__ __launch_bounds__(256) void rows_dgelu_kernel(const float* pre, const float* gp, float* gz, int ntiles, RowsGeom g) {
    const long long n = blockIdx.x / (unsigned)ntiles;
    const int t = blockIdx.x % (unsigned)ntiles;
    const float* pn = pre + n * g.P;
    const float* gn = gp + n * g.plane;
    float* zn = gz + n * g.P;
    int q[4]; float a[4], d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q[j] = (t * 4 + j) * 256 + threadIdx.x;
        a[j] = d[j] = 0.f;
        if (q[j] < g.P) {
            const int r = rows_div(q[j], g.mcols);
            a[j] = pn[q[j]];
            d[j] = gn[r * g.pitch + g.col0 + (q[j] - r * g.cols)];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (q[j] < g.P) zn[q[j]] = uno_dgelu(a[j]) * d[j];
}

// weight gradient, first stage: workgroup (split, tile) sums gy[o] x[i] over its run of 64-pixel chunks (whole chunks of one batch
// entry, in order) for a 64 x 64 tile of (o, i) and leaves the (Co, Ci + 1) block of its split (column Ci: the bias sums) in `part`;
// the fixed-order second stage is channel_wgrad_reduce_kernel (launch_channel_wgrad_finish).  Thread (to, ti) owns o = to + 16 a,
// i = ti + 16 c: its LDS reads of a pixel column hit 16 + 2 distinct banks.
struct RowsWgradParams {
    const float* gy; const float* x1; const float* x2; float* part;
    int C1, Ci, Co, npc; long long nchunks, cps;
    RowsGeom g;
};
template <bool ACT>
__global__ __launch_bounds__(256) void rows_wgrad_kernel(const RowsWgradParams p) {
    __shared__ float sg[64][65];
    __shared__ float sx[64][65];
    const RowsGeom& g = p.g;
    const int split = blockIdx.x;
    const int otiles = (p.Co + 63) / 64;
    const int o0 = ((int)blockIdx.y % otiles) * 64, i0 = ((int)blockIdx.y / otiles) * 64;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, to = tid >> 4, ti = tid & 15;
    float acc[4][4], bsum[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        bsum[a] = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
    }
    const long long c_begin = split * p.cps;
    const long long c_end = c_begin + p.cps < p.nchunks ? c_begin + p.cps : p.nchunks;
    const int C2 = p.Ci - p.C1;
    for (long long chunk = c_begin; chunk < c_end; ++chunk) {
        const long long b = chunk / p.npc;
        const int q = (int)(chunk - b * p.npc) * 64 + lane;
        const bool valid = q < g.P;
        const int qq = valid ? q : 0;
        const int r = rows_div(qq, g.mcols);
        const int phys = r * g.pitch + g.col0 + (qq - r * g.cols);
        float gv[16], xv[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const int row = wave + 4 * kk, o = o0 + row, i = i0 + row;
            gv[kk] = (valid && o < p.Co) ? p.gy[(b * p.Co + o) * (long long)g.P + qq] : 0.f;
            float v = 0.f;
            if (valid && i < p.Ci) {
                if (i < p.C1) { v = p.x1[(b * p.C1 + i) * g.plane + phys]; if (ACT) v = uno_gelu(v); }
                else v = p.x2[(b * C2 + (i - p.C1)) * g.plane + phys];
            }
            xv[kk] = v;
        }
        __syncthreads();            // the previous chunk's reads are done
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) { sg[wave + 4 * kk][lane] = gv[kk]; sx[wave + 4 * kk][lane] = xv[kk]; }
        __syncthreads();
#pragma unroll 8
        for (int pp = 0; pp < 64; ++pp) {
            float ga[4], xa[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { ga[a] = sg[to + 16 * a][pp]; xa[a] = sx[ti + 16 * a][pp]; }
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                bsum[a] += ga[a];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] = fmaf(ga[a], xa[c], acc[a][c]);
            }
        }
    }
    float* blk = p.part + (size_t)split * p.Co * (p.Ci + 1);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int o = o0 + to + 16 * a;
        if (o >= p.Co) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ti + 16 * c;
            if (i < p.Ci) blk[(size_t)o * (p.Ci + 1) + i] = acc[a][c];
        }
        if (i0 == 0 && ti == 0) blk[(size_t)o * (p.Ci + 1) + p.Ci] = bsum[a];
    }
}

const char* const kRowsLimits = "a short-row window needs 1 <= cols, 0 <= col0, col0 + cols <= pitch <= 256, rows * pitch < 2^24, plane >= rows * pitch, "
                                "1 <= C1, Ci <= 1024, 1 <= Co";

// 0: geometry accepted (*g filled), < 0: refused with the message set
int rows_geom(const char* who, int B, int rows, int cols, int pitch, int col0, long long plane, RowsGeom* g) {
    if (B < 0 || rows < 0) { set_error("%s: bad sizes B=%d rows=%d", who, B, rows); return -1; }
    if (cols < 1 || col0 < 0 || (long long)col0 + cols > pitch || pitch > 256 || (long long)rows * pitch >= (1LL << 24) || plane < (long long)rows * pitch) {
        set_error("%s: %s (got rows=%d cols=%d pitch=%d col0=%d plane=%lld)", who, kRowsLimits, rows, cols, pitch, col0, plane);
        return -2;
    }
    g->rows = rows; g->cols = cols; g->pitch = pitch; g->col0 = col0; g->plane = plane;
    g->P = rows * cols; g->E = rows * pitch;
    g->mcols = ((1ULL << 40) + cols - 1) / (unsigned long long)cols;
    g->mpitch = ((1ULL << 40) + pitch - 1) / (unsigned long long)pitch;
    return 0;
}

int rows_channels(const char* who, int C1, int Ci, int Co) {
    if (C1 < 1 || C1 > Ci || Ci > 1024 || Co < 1) { set_error("%s: %s (got C1=%d Ci=%d Co=%d)", who, kRowsLimits, C1, Ci, Co); return -2; }
    return 0;
}

int launch_rows_mix(const char* who, const char* kname, int mode, RowsMixParams& p, int B, double bytes, hipStream_t s) {
    // waves of a workgroup: over element sub-tiles first, over output tiles when there are several
    const int nt = (p.N + RM_TO - 1) / RM_TO;
    p.wc = nt >= 4 ? 4 : nt >= 2 ? 2 : 1;
    p.wp = 4 / p.wc;
    const int L = mode == RM_FWD ? p.g.P : p.g.E, tile = p.wp * RM_PX * 64;
    p.ntiles = (L + tile - 1) / tile;
    const long long blocks = (long long)B * p.ntiles;
    if (blocks > 0x7fffffffLL) { set_error("%s: too many workgroups (B * tiles = %lld)", who, blocks); return -2; }
    {
        ProfScope prof(kname, bytes, s);
        if (mode == RM_FWD) hipLaunchKernelGGL(rows_mix_kernel<RM_FWD>, dim3((unsigned)blocks), dim3(256), 0, s, p);
        else if (mode == RM_GRAD) hipLaunchKernelGGL(rows_mix_kernel<RM_GRAD>, dim3((unsigned)blocks), dim3(256), 0, s, p);
        else hipLaunchKernelGGL(rows_mix_kernel<RM_ACTPAD>, dim3((unsigned)blocks), dim3(256), 0, s, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s launch: %s", who, hipGetErrorString(e)); return -5; }
    return 0;
}

}  // namespace
}  // namespace uno

using namespace uno;

extern "C" {

int uno_channel_mix2_rows(const float* x1, const float* x2, int C1, const float* w, const float* bias, float* y, int B, int Ci, int Co, int rows,
                          int cols, int pitch, int col0, long long plane, int act_in, void* stream) {
    const char* who = "uno_channel_mix2_rows";
    RowsGeom g;
    if (int rc = rows_geom(who, B, rows, cols, pitch, col0, plane, &g)) return rc;
    if (!x2) C1 = Ci;
    if (int rc = rows_channels(who, C1, Ci, Co)) return rc;
    if (B == 0 || rows == 0) return 0;
    if (!x1 || !w || !y) { set_error("%s: null pointer", who); return -1; }
    RowsMixParams p{};
    p.in1 = x1; p.in2 = x2; p.w = w; p.bias = bias; p.out1 = y;
    p.K1 = C1; p.K = Ci; p.N1 = Co; p.N = Co; p.Ci = Ci; p.act_in = act_in ? 1 : 0; p.g = g;
    return launch_rows_mix(who, "uno::rows_mix_kernel", RM_FWD, p, B, 4.0 * B * (double)g.P * (Ci + Co), (hipStream_t)stream);
}

int uno_channel_mix2_rows_grad(const float* gy, const float* w, int C1, const float* dgelu_of, float* g1, float* g2, int B, int Ci, int Co,
                               int rows, int cols, int pitch, int col0, long long plane, void* stream) {
    const char* who = "uno_channel_mix2_rows_grad";
    RowsGeom g;
    if (int rc = rows_geom(who, B, rows, cols, pitch, col0, plane, &g)) return rc;
    if (int rc = rows_channels(who, C1, Ci, Co)) return rc;
    if (B == 0 || rows == 0) return 0;
    if (!gy || !w || !g1) { set_error("%s: null pointer", who); return -1; }
    RowsMixParams p{};
    p.in1 = gy; p.w = w; p.out1 = g1; p.out2 = g2; p.dgelu_of = dgelu_of;
    p.K1 = Co; p.K = Co; p.N1 = C1; p.N = g2 ? Ci : C1; p.Ci = Ci; p.g = g;           // (g2 == NULL: the first source's gradient alone)
    return launch_rows_mix(who, "uno::rows_grad_kernel", RM_GRAD, p, B, 4.0 * B * ((double)g.P * Co + (double)g.E * p.N), (hipStream_t)stream);
}

int uno_channel_mix_act_padded_rows(const float* x, const float* w, const float* bias, float* y, float* y_act, int B, int Ci, int Co, int rows,
                                    int cols, int pitch, int col0, int act_in, void* stream) {
    const char* who = "uno_channel_mix_act_padded_rows";
    RowsGeom g;
    if (int rc = rows_geom(who, B, rows, cols, pitch, col0, (long long)(rows > 0 ? rows : 0) * (pitch > 0 ? pitch : 0), &g)) return rc;
    if (int rc = rows_channels(who, Ci, Ci, Co)) return rc;
    if (B == 0 || rows == 0) return 0;
    if (!x || !w || !y_act) { set_error("%s: null pointer", who); return -1; }
    RowsMixParams p{};
    p.in1 = x; p.w = w; p.bias = bias; p.out1 = y; p.out_act = y_act;
    p.K1 = Ci; p.K = Ci; p.N1 = Co; p.N = Co; p.Ci = Ci; p.act_in = act_in ? 1 : 0; p.g = g;
    return launch_rows_mix(who, "uno::rows_act_padded_kernel", RM_ACTPAD, p, B,
                           4.0 * B * ((double)g.P * (Ci + (y ? Co : 0)) + (double)g.E * Co), (hipStream_t)stream);
}

int uno_dgelu_rows(const float* pre, const float* g_padded, float* gz, long long n_planes, int rows, int cols, int pitch, int col0,
                   long long plane, void* stream) {
    const char* who = "uno_dgelu_rows";
    RowsGeom g;
    if (n_planes < 0) { set_error("%s: bad sizes planes=%lld", who, n_planes); return -1; }
    if (int rc = rows_geom(who, 1, rows, cols, pitch, col0, plane, &g)) return rc;
    if (n_planes == 0 || rows == 0) return 0;
    if (!pre || !g_padded || !gz) { set_error("%s: null pointer", who); return -1; }
    const int ntiles = (g.P + 1023) / 1024;
    const long long blocks = n_planes * ntiles;
    if (blocks > 0x7fffffffLL) { set_error("%s: too many workgroups (planes * tiles = %lld)", who, blocks); return -2; }
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope prof("uno::rows_dgelu_kernel", 12.0 * (double)n_planes * g.P, s);
        hipLaunchKernelGGL(rows_dgelu_kernel, dim3((unsigned)blocks), dim3(256), 0, s, pre, g_padded, gz, ntiles, g);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s launch: %s", who, hipGetErrorString(e)); return -5; }
    return 0;
}

int uno_channel_wgrad2_rows(const float* gy, const float* x1, const float* x2, int C1, float* gw, float* gb, void* ws, int B, int Ci, int Co,
                            int rows, int cols, int pitch, int col0, long long plane, int act_x, int accumulate, void* stream) {
    const char* who = "uno_channel_wgrad2_rows";
    RowsGeom g;
    if (int rc = rows_geom(who, B, rows, cols, pitch, col0, plane, &g)) return rc;
    if (!x2) C1 = Ci;
    if (int rc = rows_channels(who, C1, Ci, Co)) return rc;
    if (accumulate != 0 && accumulate != 1) { set_error("%s: accumulate is 0 or 1", who); return -1; }
    if (B == 0 || rows == 0) return 0;          // (nothing is summed: gw / gb are left as they are)
    if (!gy || !x1 || !gw || !ws) { set_error("%s: null pointer", who); return -1; }
    hipStream_t s = (hipStream_t)stream;
    RowsWgradParams p{};
    p.gy = gy; p.x1 = x1; p.x2 = x2; p.part = (float*)ws; p.C1 = C1; p.Ci = Ci; p.Co = Co; p.g = g;
    int nsplit = 1;
    channel_wgrad_ws_floats(B, Ci, Co, g.P, &nsplit);         // the scratch holds nsplit (Co, Ci + 1) blocks: a function of the shape alone
    p.npc = (g.P + 63) / 64;
    p.nchunks = (long long)B * p.npc;
    p.cps = (p.nchunks + nsplit - 1) / nsplit;
    const int tiles = ((Co + 63) / 64) * ((Ci + 63) / 64);
    if (tiles > 65535) { set_error("%s: too many weight tiles (%d)", who, tiles); return -2; }
    {
        ProfScope prof("uno::rows_wgrad_kernel", 4.0 * B * (double)g.P * (Ci + Co), s);
        if (act_x) hipLaunchKernelGGL(rows_wgrad_kernel<true>, dim3(nsplit, tiles), dim3(256), 0, s, p);
        else hipLaunchKernelGGL(rows_wgrad_kernel<false>, dim3(nsplit, tiles), dim3(256), 0, s, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s launch: %s", who, hipGetErrorString(e)); return -5; }
    return launch_channel_wgrad_finish((const float*)ws, gw, gb, Ci, Co, nsplit, accumulate, s);
}

}  // extern "C"
