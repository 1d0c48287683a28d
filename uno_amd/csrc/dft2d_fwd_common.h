// K1 - what the three forms of the pruned forward 2-D DFT share (dft2d_fwd_kernel.h: register path, dft2d_fwd_ft_kernel.h: full tile,
// dft2d_fwd_ht_kernel.h: half tile).  The forms differ in how the row stage (stage A) gets its image operand and its twiddles; the
// column bookkeeping, the table builders, the column stage (stage B), the cross-wave reduction, the epilogue store and the launcher
// side of the two tile forms live here, once.  Included by those three headers only.
//
// The device steps are UNO_FWD_* macros, as the kernels' own stage-A steps are (UNO_*_MFMA), not functions: a function, even a
// forced-inline one, is optimised on its own before it is inlined, and that moved the schedule and the register allocation of these
// kernels (per-kernel instruction counts, a wave of occupancy or a few bytes of scratch in the largest ones;
// profiles/k1_shared_stages_isa.txt).  Expanded in place they compile to the code the three copies compiled to.  Each macro names
// the kernel locals it reads; what the helpers below can do as functions without that effect, they do.
#pragma once
#include "uno_common.h"
#include <algorithm>
#include <cstdio>

namespace uno {

constexpr int FWD_TAILMAX = 5;          // tail <= 15 pairs + w = 0 + Nyquist column = 17 elements = 5 k-steps

typedef __attribute__((address_space(3))) void* lds_ptr_t;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    // v_mfma_f32_4x4x1_16b_f32: 16 independent 4x4 outer products, block = lane / 4 (probed on gfx950:
    // tools/probes/mfma4x4_probe.hip): A[i] = lane 4*block + i, B[j] = lane 4*block + j, D[i][j] = lane 4*block + j, reg i
    return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0);
}

// Column-pair bookkeeping of the row stage: pairs (w, W-w), w = 1..P; singles w = 0 and (W even) w = W/2.  Declares P, nfull, prem,
// ntail, tailsteps.  The kernels expand it in place; the launchers read the same numbers through fwd_columns().
#define UNO_FWD_COLUMN_PAIRS(W_)                                                                                                    \
    const int P = ((W_) - 1) >> 1;                                                                                                  \
    const int nfull = P >> 4;                   /* chunks of 16 pairs = 4 k-steps */                                                \
    const int prem = P - (nfull << 4);          /* pairs beyond the last full chunk */                                              \
    const int ntail = prem + 1 + (((W_) & 1) ? 0 : 1);      /* those pairs, then w = 0, then the Nyquist column */                  \
    const int tailsteps = (ntail + 3) >> 2      /* k-steps of the tail */
struct FwdColumns { int nfull, prem, tailsteps; };
__host__ __device__ inline FwdColumns fwd_columns(int W) {
    UNO_FWD_COLUMN_PAIRS(W);
    return FwdColumns{nfull, prem, tailsteps};
}
// The operand-layout twiddle tables (UNO_FWD_BUILD_OPERAND_TABLES) hold 4 nfull + tailsteps k-steps; allocated are these (prefetches
// run to the fifth tail step), in [steps][NTF][64] + [steps][R4][16] float2
#define UNO_FWD_TABLE_STEPS(nfull_) (4 * (nfull_) + FWD_TAILMAX)
inline size_t fwd_table_bytes(int W, int NTF, int R4) { return (size_t)UNO_FWD_TABLE_STEPS(fwd_columns(W).nfull) * ((size_t)NTF * 512 + (size_t)R4 * 128); }

// Entry e_ of the tail-column table sTailW [FWD_TAILMAX][2][64]: left / right column (-1 = none) of the tail element of k-step sq, k-slot
// (ln >> 4): pairs beyond the last full chunk, then w = 0, then the Nyquist column.  Reads W, nfull, prem; leaves ln, sq and the
// element's left column w in scope.
#define UNO_FWD_PUT_TAIL_COLUMNS(e_)                                                                                                \
    const int ln = (e_) & 63, sq = (e_) >> 6;                                                                                       \
    const int q = 4 * sq + (ln >> 4);                                                                                               \
    const bool pair = q < prem;                                                                                                     \
    const bool nyq = (q == prem + 1) && !(W & 1);                                                                                   \
    const int w = pair ? 1 + 16 * nfull + q : (nyq ? (W >> 1) : 0);                                                                 \
    sTailW[(sq * 2 + 0) * 64 + ln] = (pair || q == prem || nyq) ? w : -1;                                                           \
    sTailW[(sq * 2 + 1) * 64 + ln] = pair ? W - w : -1;

// cos / sin(2 pi l w / W) in MFMA operand layout: sTabF [k-step][16-mode stream][lane], sTab4 [k-step][4-mode group][16].
// Reads p.twW, W, m2, nfull, prem, nk, tid, nthreads and the kernel's NTF, R4.
#define UNO_FWD_BUILD_OPERAND_TABLES()                                                                                              \
    for (int e = tid; e < nk * 64; e += nthreads) {                                                                                 \
        const int ln = e & 63, q = e >> 6, ks = ln >> 4;                                                                            \
        unsigned w;                                                                                                                 \
        if (q < 4 * nfull) {                                                                                                        \
            w = 1u + 16u * (q >> 2) + 4u * ks + (q & 3);                                                                            \
        } else {                                                                                                                    \
            const int qt = 4 * (q - 4 * nfull) + ks;                                                                                \
            w = qt < prem ? 1u + 16u * nfull + qt : ((qt == prem + 1 && !(W & 1)) ? (unsigned)(W >> 1) : 0u);                       \
        }                                                                                                                           \
_Pragma("unroll")                                                                                                                   \
        for (int t = 0; t < NTF; ++t) {                                                                                             \
            const unsigned l = (unsigned)min(16 * t + (ln & 15), m2 - 1);                                                           \
            sTabF[((size_t)q * NTF + t) * 64 + ln] = p.twW[(w * l) % (unsigned)W];                                                  \
        }                                                                                                                           \
        if ((ln & 12) == 0) {                                                                                                       \
_Pragma("unroll")                                                                                                                   \
            for (int g = 0; g < R4; ++g) {                                                                                          \
                const unsigned l = (unsigned)min(16 * NTF + 4 * g + (ln & 3), m2 - 1);                                              \
                sTab4[((size_t)q * R4 + g) * 16 + 4 * ks + (ln & 3)] = p.twW[(w * l) % (unsigned)W];                                \
            }                                                                                                                       \
        }                                                                                                                           \
    }

// buffer resource of the direct-to-LDS loads = [128-byte aligned start of the image, end of the tensor): offsets are non-negative,
// anything past the tensor reads as zero.  *a0 = the image's first float, counted from the aligned start.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t image_rsrc(const float* in, int n_img, int H, int W, int image, int* a0) {
    const float* timg = in + (size_t)image * H * W;
    const uintptr_t ibase = reinterpret_cast<uintptr_t>(timg) & ~uintptr_t(127);
    *a0 = (int)((reinterpret_cast<uintptr_t>(timg) - ibase) >> 2);
    const unsigned long long span = reinterpret_cast<uintptr_t>(in + (size_t)n_img * H * W) - ibase;
    return __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void*>(ibase), 0, (int)(unsigned)std::min<unsigned long long>(span, 0xffffffffull), 0x00020000);
}

// One wave's partial spectrum and the stage-B A operand rows this lane owns (Kj: their frequency, jvalid).
// !PAIR_: Xr / Xi = Re / Im of the spectrum rows (MP_ = MT tiles of 16 corner rows), Yr / Yi unused.  PAIR_ (the +-k paired column
// stage of dft2d_fwd_ht_kernel.h): Xr = Re C, Xi = Re S, Yr = -Im C, Yi = -Im S over MP_ tiles of k = 0 .. m1 (the row stage hands
// over Tn = -Im T).  Reads r16, m1, H and the kernel's NT.
#define UNO_FWD_ACCUMULATORS(PAIR_, MP_)                                                                                            \
    int Kj[MP_];                                                                                                                    \
    bool jvalid[MP_];                                                                                                               \
_Pragma("unroll")                                                                                                                   \
    for (int mt = 0; mt < (MP_); ++mt) {                                                                                            \
        const int j = 16 * mt + r16;                                                                                                \
        if constexpr (PAIR_) {                                                                                                      \
            jvalid[mt] = j <= m1;                       /* k = j: 0 .. m1 */                                                        \
            Kj[mt] = jvalid[mt] ? j : 0;                                                                                            \
        } else {                                                                                                                    \
            jvalid[mt] = j < 2 * m1;                                                                                                \
            Kj[mt] = jvalid[mt] ? corner_freq(j, m1, H) : 0;                                                                        \
        }                                                                                                                           \
    }                                                                                                                               \
    f32x4 Xr[MP_][NT], Xi[MP_][NT], Yr[(PAIR_) ? (MP_) : 1][NT], Yi[(PAIR_) ? (MP_) : 1][NT];                                       \
_Pragma("unroll")                                                                                                                   \
    for (int mt = 0; mt < (MP_); ++mt)                                                                                              \
_Pragma("unroll")                                                                                                                   \
        for (int t = 0; t < NT; ++t) {                                                                                              \
            Xr[mt][t] = f32x4{0, 0, 0, 0}; Xi[mt][t] = f32x4{0, 0, 0, 0};                                                           \
            if ((PAIR_) || mt == 0) { Yr[(PAIR_) ? mt : 0][t] = f32x4{0, 0, 0, 0}; Yi[(PAIR_) ? mt : 0][t] = f32x4{0, 0, 0, 0}; }   \
        }

// R4 > 0, after the row stage: the last mode tile's 4x4x1 result is  lane 16 ws + 4 rg + j, reg i = partial
// T[row 4 rg + i][mode 16 NTF + 4 g + j] of k-slot ws.  Sum over the four k-slots, then move to the 16x16x4 accumulator layout
// stage B consumes (lane (kk, n), reg s = T[row 4 kk + s][mode n]); columns n >= 4 R4 of the last tile are zero.
// Reads Qr, Qn, kk, r16 and the kernel's NT, R4; writes Tr[NT - 1], Tn[NT - 1].
#define UNO_FWD_REGROUP_4X4()                                                                                                       \
    if constexpr (R4 > 0) {                                                                                                         \
        f32x4 lastR = f32x4{0, 0, 0, 0}, lastN = f32x4{0, 0, 0, 0};                                                                 \
        const int src = 20 * kk + (r16 & 3);                                                                                        \
_Pragma("unroll")                                                                                                                   \
        for (int g = 0; g < R4; ++g)                                                                                                \
_Pragma("unroll")                                                                                                                   \
            for (int i = 0; i < 4; ++i) {                                                                                           \
                float vr = Qr[g][i], vn = Qn[g][i];                                                                                 \
                vr += __shfl_xor(vr, 16); vn += __shfl_xor(vn, 16);                                                                 \
                vr += __shfl_xor(vr, 32); vn += __shfl_xor(vn, 32);                                                                 \
                const float gr = __shfl(vr, src), gn = __shfl(vn, src);                                                             \
                if ((r16 >> 2) == g) { lastR[i] = gr; lastN[i] = gn; }                                                              \
            }                                                                                                                       \
        Tr[NT - 1] = lastR;                                                                                                         \
        Tn[NT - 1] = lastN;                                                                                                         \
    }

// stage B of row tile rt: X[j][l] += exp(-i theta(j,h)) * T[h][l], h = 16 rt + 4 kk + s.  The stage-A accumulators Tr / Tn (= -Im T)
// ARE the B operand (register r of lane-group g is row 4g+r).  PAIR_: real twiddles, C_k += cos T, S_k += sin T.
// Reads Tr, Tn, sTwH, rt, kk, H, H8 (= 8 H) and the accumulators.
#define UNO_FWD_STAGE_B(PAIR_, MP_)                                                                                                 \
    {                                                                                                                               \
        unsigned idxB[MP_];                                                                                                         \
        float2 twB[MP_];                                                                                                            \
_Pragma("unroll")                                                                                                                   \
        for (int mt = 0; mt < (MP_); ++mt) {                                                                                        \
            const unsigned i0 = 8u * (((unsigned)Kj[mt] * (unsigned)(16 * rt + 4 * kk)) % (unsigned)H);                             \
            twB[mt] = lds_tw(sTwH, i0);                                                                                             \
            idxB[mt] = wrap_add(i0, 8u * (unsigned)Kj[mt], H8);                                                                     \
        }                                                                                                                           \
_Pragma("unroll")                                                                                                                   \
        for (int s = 0; s < 4; ++s) {                                                                                               \
            const bool hvalid = (16 * rt + 4 * kk + s) < H;                                                                         \
            float2 twBn[MP_];                                                                                                       \
_Pragma("unroll")                                                                                                                   \
            for (int mt = 0; mt < (MP_); ++mt) {                                                                                    \
                twBn[mt] = lds_tw(sTwH, idxB[mt]);                                                                                  \
                idxB[mt] = wrap_add(idxB[mt], 8u * (unsigned)Kj[mt], H8);                                                           \
            }                                                                                                                       \
_Pragma("unroll")                                                                                                                   \
            for (int mt = 0; mt < (MP_); ++mt) {                                                                                    \
                const bool v = hvalid && jvalid[mt];                                                                                \
                const float ac = v ? twB[mt].x : 0.f;                                                                               \
                if constexpr (PAIR_) {                                                                                              \
                    const float as = v ? twB[mt].y : 0.f;                                                                           \
_Pragma("unroll")                                                                                                                   \
                    for (int t = 0; t < NT; ++t) {                                                                                  \
                        Xr[mt][t] = mfma16(ac, Tr[t][s], Xr[mt][t]);         /* Re C */                                             \
                        Yr[mt][t] = mfma16(ac, Tn[t][s], Yr[mt][t]);         /* -Im C */                                            \
                        Xi[mt][t] = mfma16(as, Tr[t][s], Xi[mt][t]);         /* Re S */                                             \
                        Yi[mt][t] = mfma16(as, Tn[t][s], Yi[mt][t]);         /* -Im S */                                            \
                    }                                                                                                               \
                } else {                                                                                                            \
                    const float ans = v ? -twB[mt].y : 0.f;                                                                         \
                    const float anc = -ac;                                                                                          \
_Pragma("unroll")                                                                                                                   \
                    for (int t = 0; t < NT; ++t) {                                                                                  \
                        Xr[mt][t] = mfma16(ac, Tr[t][s], Xr[mt][t]);                                                                \
                        Xi[mt][t] = mfma16(anc, Tn[t][s], Xi[mt][t]);                                                               \
                        Xr[mt][t] = mfma16(ans, Tn[t][s], Xr[mt][t]);                                                               \
                        Xi[mt][t] = mfma16(ans, Tr[t][s], Xi[mt][t]);                                                               \
                    }                                                                                                               \
                }                                                                                                                   \
            }                                                                                                                       \
_Pragma("unroll")                                                                                                                   \
            for (int mt = 0; mt < (MP_); ++mt) twB[mt] = twBn[mt];                                                                  \
        }                                                                                                                           \
    }

// One step of the deterministic tree reduction of the per-wave partial spectra through LDS (fixed order): sub-wave wsub_ of an image's
// NW waves hands the accumulator pair (A_, B_) to sub-wave wsub_ - stride_ through that wave's buffer partner_ (evaluated by the
// sending waves only); mine_ is the wave's own buffer.  MP_ * NT * 8 * 64 floats fit a buffer.  Reads NW, lane, NT.
#define UNO_FWD_REDUCE_STEP(A_, B_, MP_, mine_, partner_, wsub_, stride_)                                                           \
    {                                                                                                                               \
        if ((wsub_) >= (stride_) && (wsub_) < 2 * (stride_)) {                                                                      \
            float* dst = (partner_);                                                                                                \
_Pragma("unroll")                                                                                                                   \
            for (int mt = 0; mt < (MP_); ++mt)                                                                                      \
_Pragma("unroll")                                                                                                                   \
                for (int t = 0; t < NT; ++t)                                                                                        \
_Pragma("unroll")                                                                                                                   \
                    for (int r = 0; r < 4; ++r) {                                                                                   \
                        dst[((mt * NT + t) * 8 + r) * 64 + lane] = A_[mt][t][r];                                                    \
                        dst[((mt * NT + t) * 8 + 4 + r) * 64 + lane] = B_[mt][t][r];                                                \
                    }                                                                                                               \
        }                                                                                                                           \
        __syncthreads();                                                                                                            \
        if ((wsub_) < (stride_) && (wsub_) + (stride_) < NW) {                                                                      \
            const float* src = (mine_);                                                                                             \
_Pragma("unroll")                                                                                                                   \
            for (int mt = 0; mt < (MP_); ++mt)                                                                                      \
_Pragma("unroll")                                                                                                                   \
                for (int t = 0; t < NT; ++t)                                                                                        \
_Pragma("unroll")                                                                                                                   \
                    for (int r = 0; r < 4; ++r) {                                                                                   \
                        A_[mt][t][r] += src[((mt * NT + t) * 8 + r) * 64 + lane];                                                   \
                        B_[mt][t][r] += src[((mt * NT + t) * 8 + 4 + r) * 64 + lane];                                               \
                    }                                                                                                               \
        }                                                                                                                           \
        __syncthreads();                                                                                                            \
    }

// epilogue of the wave that holds the sum: scale, Hermitian weight and later-wins row mask, then the 2 m1 x m2 complex results of image
// image_.  Reads p, H, W, m1, m2, r16, kk and the accumulators.
#define UNO_FWD_STORE_SPECTRUM(PAIR_, MP_, image_)                                                                                  \
    {                                                                                                                               \
        float2* out = reinterpret_cast<float2*>(p.out) + spectrum_index(p, (image_)) * 2 * m1 * m2;                                 \
_Pragma("unroll")                                                                                                                   \
        for (int t = 0; t < NT; ++t) {                                                                                              \
            const int l = 16 * t + r16;                                                                                             \
            if (l >= m2) continue;                                                                                                  \
            const float cs_ = p.scale * (p.herm ? herm_weight(l, W) : 1.0f);                                                        \
_Pragma("unroll")                                                                                                                   \
            for (int mt = 0; mt < (MP_); ++mt)                                                                                      \
_Pragma("unroll")                                                                                                                   \
                for (int r = 0; r < 4; ++r) {                                                                                       \
                    const int j = 16 * mt + 4 * kk + r;                                                                             \
                    if constexpr (PAIR_) {                                                                                          \
                        /* k = j:  X[+k] = C - i S; with Yr = -Im C, Yi = -Im S:  Re = Xr - Yi, Im = -Yr - Xi;  X[-k]: S -> -S */   \
                        const float cr = Xr[mt][t][r], sr = Xi[mt][t][r], cn = Yr[(PAIR_) ? mt : 0][t][r], sn = Yi[(PAIR_) ? mt : 0][t][r];\
                        if (j < m1) {                                                                                               \
                            const float f = (p.mask && !row_survives(j, m1, H)) ? 0.f : cs_;                                        \
                            out[(size_t)j * m2 + l] = make_float2((cr - sn) * f, (-cn - sr) * f);                                   \
                        }                                                                                                           \
                        if (j >= 1 && j <= m1) {                                                                                    \
                            const int jm = 2 * m1 - j;                                                                              \
                            const float f = (p.mask && !row_survives(jm, m1, H)) ? 0.f : cs_;                                       \
                            out[(size_t)jm * m2 + l] = make_float2((cr + sn) * f, (-cn + sr) * f);                                  \
                        }                                                                                                           \
                    } else {                                                                                                        \
                        if (j < 2 * m1) {                                                                                           \
                            const float f = (p.mask && !row_survives(j, m1, H)) ? 0.f : cs_;                                        \
                            out[(size_t)j * m2 + l] = make_float2(Xr[mt][t][r] * f, Xi[mt][t][r] * f);                              \
                        }                                                                                                           \
                    }                                                                                                               \
                }                                                                                                                   \
        }                                                                                                                           \
    }

// ---- launcher side of the two tile forms
struct FwdFtGeometry { int nw, g; size_t lds; };

static int ft_device_cu_count() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
        if (cus <= 0) cus = 256;
    }
    return usable_cus(cus);
}

struct FwdTileForm {
    int waves;              // waves per workgroup
    size_t lds_limit;
    int min_cu_waves;       // a CU should hold at least this many waves: (nearly) one / two per SIMD
    size_t (*lds_bytes)(const Dft2dParams& p, int NTF, int R4, int waves);
};

// NW in {1, 2, 4} waves per image, G = waves / NW images per workgroup (fewer when the images do not fill the CUs)
static bool fwd_tile_geometry(const Dft2dParams& p, int NTF, int R4, const FwdTileForm& f, FwdFtGeometry* out) {
    const int nrt = (p.H + 15) / 16, cus = ft_device_cu_count();
    long long best_cost = -1;
    for (int nw = 1; nw <= 4 && nw <= nrt; nw *= 2) {
        int g = f.waves / nw;
        while (g > 1 && (long long)(p.n_img + g - 1) / g < cus) --g;
        while (g > 1 && f.lds_bytes(p, NTF, R4, nw * g) > f.lds_limit) --g;
        const size_t lds = f.lds_bytes(p, NTF, R4, nw * g);
        if (lds > f.lds_limit) continue;
        const long long per_cu = std::max<long long>(1, std::min<long long>((long long)(f.lds_limit / lds), 16 / (nw * g)));
        if (per_cu * nw * g < f.min_cu_waves && (long long)p.n_img * nw >= (long long)f.waves * cus) continue;
        const long long groups = (p.n_img + g - 1) / g;
        const long long rounds = (groups + cus * per_cu - 1) / (cus * per_cu);
        const long long cost = rounds * ((nrt + nw - 1) / nw);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; *out = FwdFtGeometry{nw, g, lds}; }
    }
    return best_cost >= 0;
}

// `name` is the kernel's profile name, `rev` the sweep direction of this launch (next_sweep_reversed(SWEEP_K1), taken by the caller)
template <void (*K)(Dft2dParams)>
static int launch_fwd_tile(const char* name, Dft2dParams p, const FwdFtGeometry& g, int rev, hipStream_t s) {
    static int lds_slot[64];
    if (!ensure_dynamic_lds(reinterpret_cast<const void*>(K), g.lds, lds_slot)) { set_error("dft2d_fwd: cannot raise dynamic LDS to %zu", g.lds); return -4; }
    p.nw = g.nw;
    p.rev = rev;
    {
        ProfScope prof(name, (double)p.n_img * ((double)p.H * p.W * 4.0 + 2.0 * p.m1 * p.m2 * 8.0), s);
        hipLaunchKernelGGL(K, dim3((p.n_img + g.g - 1) / g.g), dim3(64 * g.nw * g.g), g.lds, s, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("dft2d_fwd launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

}  // namespace uno
