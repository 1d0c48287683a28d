// K23: the Darcy-flow data generator (the reference's MATLAB files Data Generation/darcy Flow/GRF.m, demo.m, solve_gwf.m): dense two-sided
// plane transforms and a float64 conjugate-gradient solve of the 5-point system, preconditioned by the constant-coefficient Laplacian.
// C ABI: uno_darcy_transform, uno_darcy_apply, uno_darcy_solve (capi_darcy.hip).
//
// Grid: K x K nodes i / (K - 1), K in 8 ... 512; unknowns: the n x n interior nodes, n = K - 2, zero Dirichlet values on the border.
//   K23-T  Y[b] = post o (M X[b] M^T) for a batch of N x N planes as TWO launches of one kernel, out = (M in)^T: the second launch
//          transposes back.  M: host-built, (Np, Np) row-major with Np = N rounded up to the 64-wide tile, zero beyond N - the kernel reads
//          it without bounds; the planes are staged through LDS with zero fill.  float64 on vector FMAs (one k-ascending fma chain per
//          entry), float32 on v_mfma_f32_16x16x4_f32 (k-ordered).  Uses: the centres -> nodes and nodes -> centres splines, the GRF's
//          idct2 (float64), the DST-I pair of the preconditioner (float32, post = 1 / (lambda_i + lambda_j) on the first pair).
//   K23-A  Ap = A p, matrix-free: (K - 1)^2 sum over the four faces of (c + c_nbr) / 2 (p - p_nbr), faces formed from the nodal
//          coefficient plane, which may be negative (nothing is assumed about its sign); in the solver p = z + beta p_old is formed on
//          the fly (at the centre and, redundantly but with the same fma, at the four neighbours) and written to the other p buffer.
//          Per-workgroup partial sums of p^T A p.
//   K23-U  x += alpha p, r -= alpha Ap, d = r_new - r_old (over Ap), the float32 copy of r, partial sums of r^T r.
//   K23-P  partial sums of z^T r and z^T d (flexible / Polak-Ribiere beta: the preconditioner runs in float32).
//   K23-S  one workgroup per sample between them: the second stage of every sum, alpha, beta, rho, the residual test and the freeze.
// Sums: thread-serial over the thread's 4 entries, a fixed LDS tree per workgroup, the same tree over the <= 256 partials of the sample -
// no atomics, bit-reproducible, and a sample's partials are its own: its bits do not depend on B.  status[b] != 0 freezes sample b: every
// plane kernel returns at once for it (a workgroup-uniform test on a word only the K23-S launches write), so neither further iterations
// nor the host's look at the status words changes it.  No kernel waits for another workgroup.  Offsets are 64-bit.
#include "resample3d_common.h"

#include <cmath>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace uno {

constexpr int DC_THREADS = 256;
constexpr int DC_PER_WG = 4 * DC_THREADS;       // nodal entries per workgroup of the plane kernels
constexpr int DT_TILE = 64, DT_KC = 16;

template <typename T>
struct DarcyTParams {
    const T* M;             // (Np, Np), zero beyond N
    const T* X;             // (B, N, N)
    T* Y;                   // (B, N, N): Y[b][j][i] = post[j][i] sum_k M[i][k] X[b][k][j]
    const T* post;          // (N, N) or null
    const int* skip;        // (B) or null: sample b is left alone where skip[b] != 0
    int B, N, Np;
};

__device__ __forceinline__ double dt_fma(double a, double b, double c) { return fma(a, b, c); }

template <typename T>
__global__ __launch_bounds__(DC_THREADS) void darcy_transform_kernel(DarcyTParams<T> p) {
    __shared__ T sM[DT_TILE][DT_KC + 1];         // [i][k]
    __shared__ T sX[DT_KC][DT_TILE + 16];        // [k][j]
    const int tiles = p.Np / DT_TILE;
    const int b = blockIdx.x / (tiles * tiles), rem = blockIdx.x - b * tiles * tiles;
    const int i0 = (rem / tiles) * DT_TILE, j0 = (rem % tiles) * DT_TILE;
    if (i0 >= p.N || j0 >= p.N) return;         // (cannot happen: Np - N < 64)
    if (p.skip && p.skip[b] != 0) return;
    const int N = p.N, t = threadIdx.x;
    const T* X = p.X + (size_t)b * N * N;
    T* Y = p.Y + (size_t)b * N * N;
    const int kend = (N + DT_KC - 1) / DT_KC * DT_KC;
    constexpr bool MFMA = sizeof(T) == 4;
    const int lane = t & 63, wave = t >> 6, li = lane & 15, lk = lane >> 4;
    const int tx = t & 15, ty = t >> 4;
    f32x4 acc32[4];
    double acc64[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        acc32[a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) acc64[a][c] = 0.0;
    }
    for (int k0 = 0; k0 < kend; k0 += DT_KC) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = (t >> 4) + 16 * q, c = t & 15;
            sM[r][c] = p.M[(size_t)(i0 + r) * p.Np + k0 + c];
            const int kr = (t >> 6) + 4 * q, jc = t & 63;
            sX[kr][jc] = (k0 + kr < N && j0 + jc < N) ? X[(size_t)(k0 + kr) * N + j0 + jc] : T(0);
        }
        __syncthreads();
        if constexpr (MFMA) {
#pragma unroll
            for (int ks = 0; ks < DT_KC / 4; ++ks) {
                const float a = sM[16 * wave + li][4 * ks + lk];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) acc32[ct] = mfma16(a, sX[4 * ks + lk][16 * ct + li], acc32[ct]);
            }
        } else {
#pragma unroll 4
            for (int k = 0; k < DT_KC; ++k) {
                double av[4], bv[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) { av[a] = sM[4 * tx + a][k]; bv[a] = sX[k][4 * ty + a]; }
#pragma unroll
                for (int a = 0; a < 4; ++a) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc64[a][c] = dt_fma(av[a], bv[c], acc64[a][c]);
                }
            }
        }
    }
    if constexpr (MFMA) {
        // lane (li, lk), register r of tile ct: entry (i = 16 wave + 4 lk + r, j = 16 ct + li)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const int j = j0 + 16 * ct + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + 16 * wave + 4 * lk + r;
                if (i < N && j < N) {
                    const size_t o = (size_t)j * N + i;
                    Y[o] = p.post ? acc32[ct][r] * p.post[o] : acc32[ct][r];
                }
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + 4 * ty + c;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int i = i0 + 4 * tx + a;
                if (i < N && j < N) {
                    const size_t o = (size_t)j * N + i;
                    Y[o] = p.post ? (T)(acc64[a][c] * (double)p.post[o]) : (T)acc64[a][c];
                }
            }
        }
    }
}

template <typename T>
static int darcy_transform_pass(const T* M, const T* X, T* Y, const T* post, const int* skip, int B, int N, hipStream_t s) {
    DarcyTParams<T> p;
    p.M = M; p.X = X; p.Y = Y; p.post = post; p.skip = skip; p.B = B; p.N = N; p.Np = darcy_table_pitch(N);
    const int tiles = p.Np / DT_TILE;
    {
        ProfScope prof(sizeof(T) == 4 ? "uno::darcy_transform_kernel<float>" : "uno::darcy_transform_kernel<double>",
                       (double)sizeof(T) * (2.0 * B * N * N + (double)N * N), s);
        hipLaunchKernelGGL(darcy_transform_kernel<T>, dim3((unsigned)(B * tiles * tiles)), dim3(DC_THREADS), 0, s, p);
    }
    return ra_check("darcy_transform");
}

int darcy_table_pitch(int N) { return (N + DT_TILE - 1) / DT_TILE * DT_TILE; }

// Y = post o (M X M^T): tmp = (M X)^T = X^T M^T, Y = (M tmp)^T = M X M^T
int launch_darcy_transform(const void* M, const void* X, void* Y, void* tmp, const void* post, const int* skip, int B, int N, int f32,
                           hipStream_t s) {
    if (f32) {
        if (int rc = darcy_transform_pass<float>((const float*)M, (const float*)X, (float*)tmp, nullptr, skip, B, N, s)) return rc;
        return darcy_transform_pass<float>((const float*)M, (const float*)tmp, (float*)Y, (const float*)post, skip, B, N, s);
    }
    if (int rc = darcy_transform_pass<double>((const double*)M, (const double*)X, (double*)tmp, nullptr, skip, B, N, s)) return rc;
    return darcy_transform_pass<double>((const double*)M, (const double*)tmp, (double*)Y, (const double*)post, skip, B, N, s);
}

// ---------------------------------------------------------------------------------------------------------------- the solve
struct DarcyParams {
    const double* coef;     // (B, K, K) nodal coefficient
    const double* F;        // (B, K, K) nodal right-hand side (the interior is used)
    double* xout;           // (B, K, K) nodal solution, zero border
    const double* pin;      // apply only: (B, n, n)
    double* r; double* pold; double* pnew; double* ap;      // (B, n, n)
    float* r32; float* z32;                                 // (B, n, n)
    double* part;           // [4][B][W]: p^T A p | r^T r | z^T r | z^T d
    double* scal;           // [B][4]: b^T b, rho, alpha, beta
    int* status; int* iters; double* relres;                // (B) outputs; status != 0 freezes the sample
    int B, K, n, W, first;
    double rtol, s2;        // s2 = (K - 1)^2
};
enum { DC_PAP = 0, DC_RR = 1, DC_ZR = 2, DC_ZD = 3, DC_BB = 0, DC_RHO = 1, DC_ALPHA = 2, DC_BETA = 3 };

__device__ __forceinline__ double darcy_block_sum(double v, double* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
#pragma unroll
    for (int o = DC_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) s[t] += s[t + o];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// nodal entry q of this thread -> (interior?, nodal offset, interior offset, interior row, interior column)
struct DarcyAt { bool in; int nodal, o, i, j; };
__device__ __forceinline__ DarcyAt darcy_at(int q, int K, int n) {
    const int idx = blockIdx.x * DC_PER_WG + q * DC_THREADS + threadIdx.x;
    const int I = idx / K, J = idx - I * K;
    DarcyAt a;
    a.in = idx < K * K && I >= 1 && I <= n && J >= 1 && J <= n;
    a.nodal = idx; a.i = I - 1; a.j = J - 1; a.o = a.i * n + a.j;
    return a;
}

// x = 0 on the whole nodal plane, r = b = the interior of F, its float32 copy, partial sums of b^T b
__global__ __launch_bounds__(DC_THREADS) void darcy_init_kernel(DarcyParams p) {
    __shared__ double red[DC_THREADS];
    const int b = blockIdx.y, K = p.K, n = p.n;
    const size_t nodal = (size_t)b * K * K, inner = (size_t)b * n * n;
    double local = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const DarcyAt a = darcy_at(q, K, n);
        if (a.nodal < K * K) p.xout[nodal + a.nodal] = 0.0;
        if (a.in) {
            const double v = p.F[nodal + a.nodal];
            p.r[inner + a.o] = v;
            p.r32[inner + a.o] = (float)v;
            local = fma(v, v, local);
        }
    }
    const double sum = darcy_block_sum(local, red);
    if (threadIdx.x == 0) p.part[((size_t)DC_RR * p.B + b) * p.W + blockIdx.x] = sum;
}

// SOLVE: the p update fused in; !SOLVE: Ap of a given p (uno_darcy_apply)
template <bool SOLVE>
__global__ __launch_bounds__(DC_THREADS) void darcy_stencil_kernel(DarcyParams p) {
    __shared__ double red[DC_THREADS];
    const int b = blockIdx.y, K = p.K, n = p.n;
    if (SOLVE && p.status[b] != 0) return;
    const size_t inner = (size_t)b * n * n;
    const double* c = p.coef + (size_t)b * K * K;
    const double* pold = (SOLVE ? p.pold : p.pin) + inner;
    const float* z = p.z32 + inner;
    const double beta = SOLVE && !p.first ? p.scal[4 * b + DC_BETA] : 0.0;
    const bool first = p.first != 0;
    auto P = [&](int o) -> double {
        if (!SOLVE) return pold[o];
        return first ? (double)z[o] : fma(beta, pold[o], (double)z[o]);
    };
    double local = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const DarcyAt a = darcy_at(q, K, n);
        if (!a.in) continue;
        const int g = a.nodal;
        const double c0 = c[g], cN = c[g - K], cS = c[g + K], cW = c[g - 1], cE = c[g + 1];
        const double pc = P(a.o);
        const double pN = a.i > 0 ? P(a.o - n) : 0.0, pS = a.i < n - 1 ? P(a.o + n) : 0.0;
        const double pW = a.j > 0 ? P(a.o - 1) : 0.0, pE = a.j < n - 1 ? P(a.o + 1) : 0.0;
        double acc = (0.5 * (c0 + cN)) * (pc - pN);
        acc = fma(0.5 * (c0 + cS), pc - pS, acc);
        acc = fma(0.5 * (c0 + cW), pc - pW, acc);
        acc = fma(0.5 * (c0 + cE), pc - pE, acc);
        const double ap = p.s2 * acc;
        p.ap[inner + a.o] = ap;
        if (SOLVE) {
            p.pnew[inner + a.o] = pc;
            local = fma(pc, ap, local);
        }
    }
    if (SOLVE) {
        const double sum = darcy_block_sum(local, red);
        if (threadIdx.x == 0) p.part[((size_t)DC_PAP * p.B + b) * p.W + blockIdx.x] = sum;
    }
}

__global__ __launch_bounds__(DC_THREADS) void darcy_update_kernel(DarcyParams p) {
    __shared__ double red[DC_THREADS];
    const int b = blockIdx.y, K = p.K, n = p.n;
    if (p.status[b] != 0) return;
    const size_t nodal = (size_t)b * K * K, inner = (size_t)b * n * n;
    const double alpha = p.scal[4 * b + DC_ALPHA];
    double local = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const DarcyAt a = darcy_at(q, K, n);
        if (!a.in) continue;
        const size_t o = inner + a.o;
        p.xout[nodal + a.nodal] = fma(alpha, p.pnew[o], p.xout[nodal + a.nodal]);
        const double r0 = p.r[o], r1 = fma(-alpha, p.ap[o], r0);
        p.r[o] = r1;
        p.ap[o] = r1 - r0;
        p.r32[o] = (float)r1;
        local = fma(r1, r1, local);
    }
    const double sum = darcy_block_sum(local, red);
    if (threadIdx.x == 0) p.part[((size_t)DC_RR * p.B + b) * p.W + blockIdx.x] = sum;
}

__global__ __launch_bounds__(DC_THREADS) void darcy_dot_kernel(DarcyParams p) {
    __shared__ double red[DC_THREADS];
    const int b = blockIdx.y, K = p.K, n = p.n;
    if (p.status[b] != 0) return;
    const size_t inner = (size_t)b * n * n;
    double zr = 0.0, zd = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const DarcyAt a = darcy_at(q, K, n);
        if (!a.in) continue;
        const size_t o = inner + a.o;
        const double z = (double)p.z32[o];
        zr = fma(z, p.r[o], zr);
        if (!p.first) zd = fma(z, p.ap[o], zd);
    }
    const double s_zr = darcy_block_sum(zr, red), s_zd = darcy_block_sum(zd, red);
    if (threadIdx.x == 0) {
        p.part[((size_t)DC_ZR * p.B + b) * p.W + blockIdx.x] = s_zr;
        p.part[((size_t)DC_ZD * p.B + b) * p.W + blockIdx.x] = s_zd;
    }
}

// K23-S, one workgroup per sample.  STAGE 0: after init (b^T b, the outputs' first values: runs for every sample); 1: after K23-A (alpha);
// 2: after K23-P (iteration count, residual test, beta, rho)
template <int STAGE>
__global__ __launch_bounds__(DC_THREADS) void darcy_scalar_kernel(DarcyParams p) {
    __shared__ double red[DC_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    if (STAGE != 0 && p.status[b] != 0) return;
    auto total = [&](int which) { return darcy_block_sum(t < p.W ? p.part[((size_t)which * p.B + b) * p.W + t] : 0.0, red); };
    double* sc = p.scal + 4 * b;
    if (STAGE == 0) {
        const double bb = total(DC_RR);
        if (t == 0) {
            sc[DC_BB] = bb; sc[DC_RHO] = 0.0; sc[DC_ALPHA] = 0.0; sc[DC_BETA] = 0.0;
            p.iters[b] = 0;
            p.relres[b] = bb == 0.0 ? 0.0 : (isfinite(bb) ? 1.0 : bb);
            p.status[b] = bb == 0.0 ? 1 : (isfinite(bb) ? 0 : 2);
        }
    } else if (STAGE == 1) {
        const double pap = total(DC_PAP);
        if (t == 0) {
            if (pap == 0.0 || !isfinite(pap)) p.status[b] = 2;
            else sc[DC_ALPHA] = sc[DC_RHO] / pap;
        }
    } else {
        const double rr = total(DC_RR), zr = total(DC_ZR), zd = total(DC_ZD);
        if (t == 0) {
            const double bb = sc[DC_BB];
            if (!p.first) p.iters[b] += 1;
            p.relres[b] = sqrt(rr / bb);
            const double beta = p.first ? 0.0 : zd / sc[DC_RHO];
            if (!isfinite(rr)) p.status[b] = 2;
            else if (sqrt(rr) <= p.rtol * sqrt(bb)) p.status[b] = 1;
            else if (zr == 0.0 || !isfinite(zr) || !isfinite(beta)) p.status[b] = 2;
            else { sc[DC_RHO] = zr; sc[DC_BETA] = beta; }
        }
    }
}

// the preconditioner's tables per (device, n): the DST-I matrix sqrt(2 / (n + 1)) sin(pi (i + 1) (k + 1) / (n + 1)), its own inverse, padded
// to the tile, and 1 / (lambda_i + lambda_j), lambda_i = (K - 1)^2 4 sin^2(pi (i + 1) / (2 (n + 1))): the 5-point Laplacian's eigenvalues
struct DarcyTables { const float* dst; const float* inv_eig; };
static bool darcy_tables(int n, DarcyTables& out) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, DarcyTables> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { set_error("hipGetDevice failed"); return false; }
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({dev, n});
    if (it != cache.end()) { out = it->second; return true; }
    const double pi = 3.141592653589793238462643383279;
    const int Np = darcy_table_pitch(n);
    std::vector<float> dst((size_t)Np * Np, 0.0f), inv((size_t)n * n);
    std::vector<double> lam(n);
    const double scale = std::sqrt(2.0 / (n + 1));
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < n; ++k) dst[(size_t)i * Np + k] = (float)(scale * std::sin(pi * (double)(((long long)(i + 1) * (k + 1)) % (2 * (n + 1))) / (n + 1)));
        const double sh = std::sin(pi * (i + 1) / (2.0 * (n + 1)));
        lam[i] = (double)(n + 1) * (n + 1) * 4.0 * sh * sh;
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) inv[(size_t)i * n + j] = (float)(1.0 / (lam[i] + lam[j]));
    DarcyTables t;
    t.dst = static_cast<const float*>(upload_table(dst.data(), dst.size() * sizeof(float)));
    t.inv_eig = t.dst ? static_cast<const float*>(upload_table(inv.data(), inv.size() * sizeof(float))) : nullptr;
    if (!t.dst || !t.inv_eig) { set_error("darcy table allocation for n=%d failed: %s", n, hipGetErrorString(hipGetLastError())); return false; }
    cache[{dev, n}] = t;
    out = t;
    return true;
}

static int darcy_wgs(int K) { return (K * K + DC_PER_WG - 1) / DC_PER_WG; }        // <= 256 at K <= 512: one K23-S thread per partial

// planes: 4 float64 + 4 float32 of (B, n, n); partials 4 B W, scalars 4 B float64
long long darcy_ws_bytes(int B, int K) {
    const long long n = K - 2, plane = (long long)B * n * n;
    return 8 * (4 * plane + 4LL * B * darcy_wgs(K) + 4LL * B) + 4 * 4 * plane;
}

int launch_darcy_apply(const double* coef, const double* pin, double* ap, int B, int K, hipStream_t s) {
    DarcyParams p = {};
    p.coef = coef; p.pin = pin; p.ap = ap; p.B = B; p.K = K; p.n = K - 2; p.W = darcy_wgs(K); p.s2 = (double)(K - 1) * (K - 1);
    {
        ProfScope prof("uno::darcy_stencil_kernel<apply>", 8.0 * B * (3.0 * K * K), s);
        hipLaunchKernelGGL(darcy_stencil_kernel<false>, dim3(p.W, B), dim3(DC_THREADS), 0, s, p);
    }
    return ra_check("darcy_stencil<apply>");
}

int launch_darcy_solve(const double* coef, const double* F, double* P, int* iters, double* relres, int* status, void* ws, int B, int K,
                       double rtol, int max_iter, int check_every, hipStream_t s) {
    const int n = K - 2;
    DarcyTables tab;
    if (!darcy_tables(n, tab)) return -6;
    const size_t plane = (size_t)B * n * n;
    DarcyParams p = {};
    p.coef = coef; p.F = F; p.xout = P; p.iters = iters; p.relres = relres; p.status = status;
    p.B = B; p.K = K; p.n = n; p.W = darcy_wgs(K); p.rtol = rtol; p.s2 = (double)(K - 1) * (K - 1);
    double* d = static_cast<double*>(ws);
    p.r = d; double* pbuf[2] = {d + plane, d + 2 * plane}; p.ap = d + 3 * plane;
    p.part = d + 4 * plane; p.scal = p.part + (size_t)4 * B * p.W;
    float* f = reinterpret_cast<float*>(p.scal + (size_t)4 * B);
    p.r32 = f; float* ta = f + plane; float* tb = f + 2 * plane; p.z32 = f + 3 * plane;
    const dim3 grid(p.W, B), block(DC_THREADS);
    const double pb = 8.0 * (double)plane;

    // z = S ((S r S) / (lambda_i + lambda_j)) S in float32: the fast Poisson solve, two K23-T pairs
    auto precondition = [&]() -> int {
        if (int rc = launch_darcy_transform(tab.dst, p.r32, tb, ta, tab.inv_eig, status, B, n, 1, s)) return rc;
        return launch_darcy_transform(tab.dst, tb, p.z32, ta, nullptr, status, B, n, 1, s);
    };
    auto dots = [&]() -> int {
        {
            ProfScope prof("uno::darcy_dot_kernel", 2.5 * pb, s);
            hipLaunchKernelGGL(darcy_dot_kernel, grid, block, 0, s, p);
        }
        {
            ProfScope prof("uno::darcy_scalar_kernel<2>", 24.0 * B * p.W, s);
            hipLaunchKernelGGL(darcy_scalar_kernel<2>, dim3(B), block, 0, s, p);
        }
        return ra_check("darcy_dot");
    };

    p.first = 1;
    {
        ProfScope prof("uno::darcy_init_kernel", 3.5 * pb, s);
        hipLaunchKernelGGL(darcy_init_kernel, grid, block, 0, s, p);
    }
    {
        ProfScope prof("uno::darcy_scalar_kernel<0>", 8.0 * B * p.W, s);
        hipLaunchKernelGGL(darcy_scalar_kernel<0>, dim3(B), block, 0, s, p);
    }
    if (int rc = ra_check("darcy_init")) return rc;
    if (int rc = precondition()) return rc;
    if (int rc = dots()) return rc;

    std::vector<int> host(B);
    for (int k = 0; k < max_iter; ++k) {
        p.first = k == 0;
        p.pold = pbuf[k & 1]; p.pnew = pbuf[(k + 1) & 1];
        {
            ProfScope prof("uno::darcy_stencil_kernel<solve>", 4.5 * pb, s);
            hipLaunchKernelGGL(darcy_stencil_kernel<true>, grid, block, 0, s, p);
        }
        {
            ProfScope prof("uno::darcy_scalar_kernel<1>", 8.0 * B * p.W, s);
            hipLaunchKernelGGL(darcy_scalar_kernel<1>, dim3(B), block, 0, s, p);
        }
        {
            ProfScope prof("uno::darcy_update_kernel", 6.5 * pb, s);
            hipLaunchKernelGGL(darcy_update_kernel, grid, block, 0, s, p);
        }
        if (int rc = ra_check("darcy iteration")) return rc;
        if (int rc = precondition()) return rc;
        p.first = 0;
        if (int rc = dots()) return rc;
        if ((k + 1) % check_every == 0 && k + 1 < max_iter) {       // the host's only look: B status words
            if (hipMemcpyAsync(host.data(), status, sizeof(int) * B, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess) {
                set_error("uno_darcy_solve: reading the status words failed: %s", hipGetErrorString(hipGetLastError()));
                return -5;
            }
            bool all = true;
            for (int b = 0; b < B; ++b) all = all && host[b] != 0;
            if (all) break;
        }
    }
    return 0;
}

}  // namespace uno
