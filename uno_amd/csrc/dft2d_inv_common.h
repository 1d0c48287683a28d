// K3 - what the three forms of the pruned inverse 2-D DFT share (dft2d_inv_kernel.h: chunked and full tile, dft2d_inv_add_kernel.h:
// K3-A, full tile + up-sampled addend).  The forms differ in how a row tile leaves the wave (and K3-A in the addend's two MFMA stages);
// the LDS prologue, the wave <-> image assignment, the +-k operand and the MFMA chain of the column stage (stage B'), the row-stage
// chain of one column tile, the row-tile layout of the two full-tile forms with its staging and its whole-line store phase, and the
// launcher live here, once.  Included by those two headers only.
//
// The device steps are UNO_INV_* macros, as on the forward side (dft2d_fwd_common.h) and for the same reason: expanded in place, and
// in the order the kernels had them, they compile to the code the copies compiled to; only the three small index helpers are functions
// (profiles/k3_shared_stages_isa.txt says which pieces were tried as functions or in another order and what that gave).  Each macro
// names the kernel locals it reads.
#pragma once
#include "uno_common.h"
#include <algorithm>
#include <cstdio>

namespace uno {

constexpr size_t INV_LDS_BUDGET = 160 * 1024 - 2048;

// 16-column tiles that cover the computed columns 0 .. W/2 (columns W/2 + 1 .. W - 1 are their mirror images)
__host__ __device__ constexpr int inv_col_tiles(int W) { return ((W >> 1) + 16) >> 4; }
// floats of one wave's row tile in LDS (full-tile forms): 16 rows + alignment phase (< 32) + one dump slot per lane, 16-byte multiple
__host__ __device__ constexpr int inv_ft_tile_stride(int W) { return (16 * W + 32 + 64 + 3) & ~3; }

// ---- what every form names the same way: the grid and the workgroup's waves, then this lane's place in the MFMA operands
#define UNO_INV_GRID_LOCALS()                                                                                                       \
    const int H = p.H, W = p.W, m1 = p.m1, m2 = p.m2;                                                                               \
    const int tid = threadIdx.x;                                                                                                    \
    const int nthreads = blockDim.x;                                                                                                \
    const int NWT = nthreads >> 6;              /* waves in the workgroup */                                                        \
    const int NW = p.nw;                        /* waves per image */                                                               \
    const int Wh = W >> 1                       /* columns 0..Wh are computed, Wh+1..W-1 are their mirror images */
#define UNO_INV_LANE_LOCALS()                                                                                                       \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                                                      \
    const int lane = tid & 63;                                                                                                      \
    const int r16 = lane & 15;                                                                                                      \
    const int kk = lane >> 4

// ---- LDS prologue.  Reads p, H, tid, nthreads / W, m2, nwt and the kernel's KS; the caller ends it with __syncthreads().
#define UNO_INV_FILL_ROW_TWIDDLES()                                                                                                 \
    for (int n = tid; n < H; n += nthreads) sTwH[n] = p.twH[n]
// cos / sin(2 pi l w / W) in MFMA operand layout sTabA [column tile][k-step][lane]: entry (wt, sp, lane = (i, kq)) is column
// w = 16 wt + i, mode l = 4 sp + kq (modes >= m2 face zero operands).  The same for every row tile of every image.
#define UNO_INV_BUILD_OPERAND_TABLE()                                                                                               \
    for (int e = tid; e < nwt * KS * 64; e += nthreads) {                                                                           \
        const int ln = e & 63, q = e >> 6;                                                                                          \
        const int sp = q % KS, wt = q / KS;                                                                                         \
        const unsigned l = (unsigned)min(4 * sp + (ln >> 4), m2 - 1);                                                               \
        const unsigned w = (unsigned)(16 * wt + (ln & 15));                                                                         \
        sTabA[e] = p.twW[(l * w) % (unsigned)W];                                                                                    \
    }

// ---- wave -> (image, wsub): NW waves per image, NWT / NW images per workgroup; waves without an image leave (no barrier may follow).
// Declares slot, wsub, image.  Reads wave, NW, NWT, p.
#define UNO_INV_WAVE_IMAGE()                                                                                                        \
    const int slot = wave / NW, wsub = wave - slot * NW;                                                                            \
    const int image = sweep_x(p.rev) * (NWT / NW) + slot;                                                                           \
    if (image >= p.n_img) return
// the image's 2 m1 x m2 spectrum.  Reads p, m1, m2.
#define UNO_INV_SPECTRUM(image_) (reinterpret_cast<const float2*>(p.in) + spectrum_index(p, (image_)) * 2 * m1 * m2)

// ---- stage-B' A operand, once per image.  The corner rows come in +-k pairs (lo corner row k <-> frequency +k, hi corner row
// 2 m1 - k <-> frequency -k), so with P_k = O[+k] + O[-k], M_k = O[+k] - O[-k]:
//     U[h] = sum_{k=0}^{m1} cos(theta_k h) P_k + i sin(theta_k h) M_k          (theta_k = 2 pi k / H)
// i.e. m1 + 1 real twiddle pairs instead of 2 m1 complex ones - 40 % fewer MFMAs in this stage.
// Operand lane (rho = r16 -> mode 16 t + 4 (rho & 3) + (rho >> 2), k-slot kk -> k = 4 ks + kk); scale, Hermitian weight and the
// later-wins row mask go in here.  LOAD_: false reads nothing (K3-A's knock-out).  Declares Pr, Pi, Mr, Mi [NT][KSK]; reads O (the
// image's spectrum), p, H, W, m1, m2, r16, kk.
#define UNO_INV_COLUMN_OPERAND(LOAD_)                                                                                               \
    float Pr[NT][KSK], Pi[NT][KSK], Mr[NT][KSK], Mi[NT][KSK];                                                                       \
_Pragma("unroll")                                                                                                                   \
    for (int t = 0; t < NT; ++t) {                                                                                                  \
        const int l = 16 * t + 4 * (r16 & 3) + (r16 >> 2);                                                                          \
        const float cs = p.scale * ((p.herm && l < m2) ? herm_weight(l, W) : 1.0f);                                                 \
_Pragma("unroll")                                                                                                                   \
        for (int ks = 0; ks < KSK; ++ks) {                                                                                          \
            const int k = 4 * ks + kk;                                                                                              \
            float2 vp = make_float2(0.f, 0.f), vm = make_float2(0.f, 0.f);                                                          \
            if ((LOAD_) && l < m2 && k < m1 && !(p.mask && !row_survives(k, m1, H))) vp = O[(size_t)k * m2 + l];   /* +k: lo corner row k */       \
            if ((LOAD_) && l < m2 && k >= 1 && k <= m1) vm = O[(size_t)(2 * m1 - k) * m2 + l];                     /* -k: hi corner row 2 m1 - k */ \
            Pr[t][ks] = (vp.x + vm.x) * cs; Pi[t][ks] = (vp.y + vm.y) * cs;                                                         \
            Mr[t][ks] = (vp.x - vm.x) * cs; Mi[t][ks] = (vp.y - vm.y) * cs;                                                         \
        }                                                                                                                           \
    }

// ---- stage B' of row tile rt_ -> Ur, Ui [NT]:  U^T[l][h] = sum_k P_k cos + i M_k sin.  B operand = (cos, sin)(2 pi k h / H) from sTwH,
// lane: k-slot kk (k = 4 ks + kk), column = row h of the tile; the next k-step's twiddle is read one step ahead (LDS latency hides
// behind the MFMAs).  BETWEEN_ runs after the MFMAs of k-step ks (the full-tile form threads its store batches through here).
// Reads Pr .. Mi, sTwH, r16, kk, H, H8 (= 8 H), ksk (k-steps actually needed) and the kernel's NT, KSK.
#define UNO_INV_STAGE_B(rt_, BETWEEN_)                                                                                              \
    {                                                                                                                               \
        const unsigned hB = (unsigned)min(16 * (rt_) + r16, H - 1);                                                                 \
        const unsigned a4 = 8u * ((4u * hB) % (unsigned)H);               /* advance of (k h mod H) per k-step */                   \
        unsigned aj = 8u * (((unsigned)kk * hB) % (unsigned)H);          /* (k h) mod H, k = kk */                                  \
_Pragma("unroll")                                                                                                                   \
        for (int t = 0; t < NT; ++t) { Ur[t] = f32x4{0, 0, 0, 0}; Ui[t] = f32x4{0, 0, 0, 0}; }                                      \
        float2 twb = lds_tw(sTwH, aj);                                                                                              \
_Pragma("unroll")                                                                                                                   \
        for (int ks = 0; ks < KSK; ++ks) {                                                                                          \
            aj = wrap_add(aj, a4, H8);                                                                                              \
            const float2 twn = lds_tw(sTwH, aj);                                                                                    \
            if (ks < ksk) {                                                                                                         \
                const float ns = -twb.y;                                                                                            \
_Pragma("unroll")                                                                                                                   \
                for (int t = 0; t < NT; ++t) {                                                                                      \
                    Ur[t] = mfma16(Pr[t][ks], twb.x, Ur[t]);                                                                        \
                    Ui[t] = mfma16(Pi[t][ks], twb.x, Ui[t]);                                                                        \
                    Ur[t] = mfma16(Mi[t][ks], ns, Ur[t]);                                                                           \
                    Ui[t] = mfma16(Mr[t][ks], twb.y, Ui[t]);                                                                        \
                }                                                                                                                   \
            }                                                                                                                       \
            twb = twn;                                                                                                              \
            BETWEEN_;                                                                                                               \
        }                                                                                                                           \
    }

// ---- row stage (A') of one column tile out of the operand table:  D[w][h] = sum_modes tw[w][mode] U[mode][h], symmetric form
// E_ = sum Ur cos, D_ = sum Ui sin (then y[w] = E - D, y[W - w] = E + D).  The twiddles of column tile next_ are requested into NXT_
// first (sched_barrier keeps the reads in front of the MFMAs), then the chain runs out of CUR_.  STEPS_ >= KS steps, EXTRA_ runs in
// every step sp (K3-A: the addend's stage 2' in the same chain).  Reads tabLane, Ur, Ui and the kernel's KS.
#define UNO_INV_ROW_CHAIN(next_, CUR_, NXT_, E_, D_, STEPS_, EXTRA_)                                                                \
    {                                                                                                                               \
        const float2* nxt = tabLane + (size_t)(next_) * (KS * 64);                                                                  \
_Pragma("unroll")                                                                                                                   \
        for (int sp = 0; sp < KS; ++sp) NXT_[sp] = nxt[sp * 64];                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                                          \
        E_ = f32x4{0, 0, 0, 0}; D_ = f32x4{0, 0, 0, 0};                                                                             \
_Pragma("unroll")                                                                                                                   \
        for (int sp = 0; sp < (STEPS_); ++sp) {                                                                                     \
            if (sp < KS) {                                                                                                          \
                E_ = mfma16(CUR_[sp].x, Ur[sp >> 2][sp & 3], E_);                                                                   \
                D_ = mfma16(CUR_[sp].y, Ui[sp >> 2][sp & 3], D_);                                                                   \
            }                                                                                                                       \
            EXTRA_;                                                                                                                 \
        }                                                                                                                           \
    }

// ---- the row tile of the two full-tile forms.  A wave builds its complete 16 x W tile (one contiguous run of 16 W floats of the
// image) in LDS at the SAME OFFSET MODULO 128 BYTES as in memory - LDS index i <-> memory (tile - phase)[i] - and writes it out as
// whole 128-byte lines, 1 KB per instruction.  Guarded-out elements go to one dump slot per lane behind the tile.  With one wave per
// image (chain) the partial line at the end of a tile is carried to the head of the same buffer, where the next tile's phase puts it.
// LDS: sTabA [nwt][KS][64] float2 | sTwH [H, even] float2 | sTile [NWT][inv_ft_tile_stride(W)] float (inv_ft_lds_bytes()).
// UNO_INV_FT_LDS declares the carve-up; UNO_INV_FT_WAVE_TILE this wave's buf, dump, tabLane, wfast_hi, chain.  They read smem, H, W,
// Wh, nwt, NW, wave, lane and the kernel's KS.
#define UNO_INV_FT_LDS()                                                                                                            \
    float2* sTabA = reinterpret_cast<float2*>(smem);                                                                                \
    float2* sTwH = sTabA + nwt * KS * 64;                                                                                           \
    float* sTile = reinterpret_cast<float*>(sTwH + ((H + 1) & ~1));                                                                 \
    const int tile_stride = inv_ft_tile_stride(W)
#define UNO_INV_FT_WAVE_TILE()                                                                                                      \
    float* buf = sTile + (size_t)wave * tile_stride;                                                                                \
    const int dump = 16 * W + 32 + lane;                    /* where guarded-out elements go */                                     \
    const float2* tabLane = sTabA + lane;                                                                                           \
    const int wfast_hi = W - Wh - 1;                        /* largest w whose mirror column W - w lies in the right half */        \
    const bool chain = NW == 1                              /* consecutive tiles by one wave: carry the partial line */
// Row tile rt_ of image img: declares tile, rows, phase, rowbase (this lane's row) and row_ok.
#define UNO_INV_FT_TILE(rt_)                                                                                                        \
    float* tile = img + (size_t)(rt_) * 16 * W;                                                                                     \
    const int rows = min(16, H - 16 * (rt_));                                                                                       \
    const int phase = (int)((reinterpret_cast<uintptr_t>(tile) >> 2) & 31);       /* LDS index == memory offset (mod 128 B) */      \
    const int rowbase = phase + r16 * W;                                                                                            \
    const bool row_ok = r16 < rows
// column tiles [1, nfast) need no guards when all 16 rows exist
__device__ __forceinline__ int inv_ft_fast_tiles(int rows, int nwt, int wfast_hi) { return rows == 16 ? max(1, min(nwt, (wfast_hi + 1) >> 4)) : 1; }
// Staging column tile wt_: lane (h = r16, g = kk) owns columns 16 wt + 4 g + e (YL_) and their mirrors W - (...) (YR_).  fast_
// (uniform): an interior tile of a full row tile, no guards.
#define UNO_INV_FT_STAGE(wt_, fast_, YL_, YR_)                                                                                      \
    {                                                                                                                               \
        const int w0 = 16 * (wt_) + 4 * kk;                                                                                         \
        const f32x4 yl = (YL_);                                                                                                     \
        const f32x4 yr = (YR_);                                                                                                     \
        if (fast_) {                                                                                                                \
            float* pl = buf + rowbase + w0;                                                                                         \
            float* pr = buf + rowbase + W - w0 - 3;                                                                                 \
            pl[0] = yl[0]; pl[1] = yl[1]; pl[2] = yl[2]; pl[3] = yl[3];                                                             \
            pr[3] = yr[0]; pr[2] = yr[1]; pr[1] = yr[2]; pr[0] = yr[3];                                                             \
        } else {                                                                                                                    \
_Pragma("unroll")                                                                                                                   \
            for (int e = 0; e < 4; ++e) {                                                                                           \
                const int w = w0 + e;                                                                                               \
                buf[(row_ok && w <= Wh) ? rowbase + w : dump] = yl[e];                                                              \
                buf[(row_ok && w >= 1 && w <= wfast_hi) ? rowbase + W - w : dump] = yr[e];                                          \
            }                                                                                                                       \
        }                                                                                                                           \
    }
// four whole 1 KB runs from instruction `it` on: reads first, then the stores
#define UNO_INV_FT_STORE_BATCH()                                                                                                    \
    {                                                                                                                               \
        const float* src = buf + 256 * it + 4 * lane;                                                                               \
        float* dst = gbase + 256 * it + 4 * lane;                                                                                   \
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(src);                                                                      \
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(src + 256);                                                                \
        const f32x4 v2 = *reinterpret_cast<const f32x4*>(src + 512);                                                                \
        const f32x4 v3 = *reinterpret_cast<const f32x4*>(src + 768);                                                                \
        *reinterpret_cast<f32x4*>(dst) = v0;                                                                                        \
        *reinterpret_cast<f32x4*>(dst + 256) = v1;                                                                                  \
        *reinterpret_cast<f32x4*>(dst + 512) = v2;                                                                                  \
        *reinterpret_cast<f32x4*>(dst + 768) = v3;                                                                                  \
        it += 4;                                                                                                                    \
    }
// The tile goes out as whole 128-byte lines.  more_: this wave has another tile after this one.  STORE_: false issues no stores
// (K3-A's knock-out).  INTERLEAVE_ runs behind the head of the tile and may call store_batch() (one batch, if one is left) any number
// of times; what it leaves is stored after it (the batch expanded in the loop: drained through store_batch() K3-A's 14-tile kernels
// came out with another register allocation).  Plain stores: the non-temporal form measured 161 -> 157.5 us (noise) and would keep the
// block's output out of the Infinity Cache for its consumer.  Reads tile, phase, rows, buf, chain, rt, lane, W.
#define UNO_INV_FT_STORE_TILE(more_, STORE_, INTERLEAVE_)                                                                           \
    {                                                                                                                               \
        float* gbase = tile - phase;                                                                                                \
        const int total = phase + rows * W;                                                                                         \
        const bool first = !chain || rt == 0, last = !chain || !(more_);                                                            \
        const int lo = first ? phase : 0;                   /* chained tiles start with the carried head of the line */             \
        const int hi = last ? total : (total & ~31);                                                                                \
        auto store_guarded = [&](int i) {                                                                                           \
            if (i >= hi) return;                                                                                                    \
            if (i >= lo && i + 3 < hi) {                                                                                            \
                *reinterpret_cast<f32x4*>(gbase + i) = *reinterpret_cast<const f32x4*>(buf + i);                                    \
            } else {                                                                                                                \
_Pragma("unroll")                                                                                                                   \
                for (int e = 0; e < 4; ++e)                                                                                         \
                    if (i + e >= lo && i + e < hi) gbase[i + e] = buf[i + e];                                                       \
            }                                                                                                                       \
        };                                                                                                                          \
        const int nfull = (STORE_) ? (hi >> 8) : 0;         /* instructions [1, nfull) cover whole 1 KB runs inside [lo, hi) */     \
        if (STORE_) store_guarded(4 * lane);                                                                                        \
        int it = 1;                                                                                                                 \
        auto store_batch = [&]() { if (it + 4 <= nfull) UNO_INV_FT_STORE_BATCH() };                                                 \
        INTERLEAVE_;                                                                                                                \
        while (it + 4 <= nfull) UNO_INV_FT_STORE_BATCH()                                                                            \
        for (; it < nfull; ++it)                                                                                                    \
            *reinterpret_cast<f32x4*>(gbase + 256 * it + 4 * lane) = *reinterpret_cast<const f32x4*>(buf + 256 * it + 4 * lane);    \
        if (nfull >= 1) store_guarded(256 * nfull + 4 * lane);                                                                      \
        if (!last) {                                                                                                                \
            /* carry the partial last line to the head of the next tile's image (same buffer, next phase = total & 31) */           \
            const int rem = total & 31;                                                                                             \
            float v = 0.f;                                                                                                          \
            if (lane < rem) v = buf[(total & ~31) + lane];                                                                          \
            if (lane < rem) buf[lane] = v;                                                                                          \
        }                                                                                                                           \
    }

// ---- launcher side
struct InvGeometry { int nw, g; size_t lds; bool tab; };        // NW waves per image, G images per workgroup

// K: the kernel; `name`: its profile name; `bytes`: what the launch moves; `who`: the entry point, for error messages; `rev`: the sweep
// direction of this launch (next_sweep_reversed(SWEEP_K3), taken by the caller)
template <void (*K)(Dft2dParams)>
static int launch_inv(const char* name, double bytes, const char* who, Dft2dParams p, const InvGeometry& g, int rev, hipStream_t s) {
    static int lds_slot[64];
    if (!ensure_dynamic_lds(reinterpret_cast<const void*>(K), g.lds, lds_slot)) { set_error("%s: cannot raise dynamic LDS to %zu", who, g.lds); return -4; }
    p.nw = g.nw;
    p.rev = rev;
    {
        ProfScope prof(name, bytes, s);
        hipLaunchKernelGGL(K, dim3((p.n_img + g.g - 1) / g.g), dim3(64 * g.nw * g.g), g.lds, s, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s launch: %s", who, hipGetErrorString(e)); return -5; }
    return 0;
}
// bytes of a plain K3 launch: the images (2 or 4 bytes per element) and the spectra
static double inv_bytes(const Dft2dParams& p, double elem) { return (double)p.n_img * ((double)p.H * p.W * elem + 2.0 * p.m1 * p.m2 * 8.0); }

}  // namespace uno
