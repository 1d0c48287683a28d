// K1, full-tile form that ALSO writes the down-sampled image (K1-FD):  spec = pruned DFT(x)  and  out = A . x . B^T  from ONE read of x.
//
// In a down-sampling operator block K7 (resample2d.hip) and K1 each streamed the same full-resolution tensor from HBM, one after the
// other; the input gradient of an up-sampling block has the same shape.  Here the wave that holds a 16 x W
// tile of the image in LDS for the row stage of the transform (dft2d_fwd_ft_kernel.h: stage A is that kernel's, expanded in place)
// applies the separable banded operator of K7 to it before the tile buffer is handed to the next tile's loads:
//   * column operator, VALU, from the tile in LDS: lane -> output columns 64 e + lane (e < CE, the instantiation's FD_CE or FD_CE2), Y[r][e] = sum_t wtW[j][t] x[r][start_j + t]
//     for the 16 tile rows (taps in ascending order, as K7's column sweep).  The upper half wave reads one column EARLIER, with its taps
//     moved up by one register: at 2:1 the start columns of neighbouring outputs are two floats apart, so the two half waves would hit
//     the same 32 LDS banks - shifted, they take the even and the odd banks.
//   * the next tile is requested (its transfer runs under everything below),
//   * row operator, VALU, registers only: ONE wave walks the tiles of an image top to bottom (NW == 1), so the output rows a tile
//     contributes to are carried in registers across tiles: C[c] = output row ibase(tile) + c, c < FD_NC.  The weights are
//     wave-uniform: a host-built dense [tile][FD_NC][16] table (uno_amd/resample.py fused_resample_tables) handed out lane by lane (v_readlane);
//     4-row pieces of it that are all zero - about half of them at 2:1 - are skipped on a per-tile bit mask (uniform branches).
//   * the rows the tile completed leave as unit-stride stores of Wo floats at the start of the next tile, and the carried rows move down
//     by that count.
// The banded operators add to a kernel whose lone wave per SIMD already runs its phases back to back; what that costs against the
// 815 MB that are no longer read twice is measured in DESIGN.md section 4.
#pragma once
#include "dft2d_fwd_common.h"
#include "dft2d_fwd_ft_kernel.h"

namespace uno {

constexpr int FD_NC = 13;               // carried output rows (12 are open at once at 446 -> 223 and its adjoint twin)
constexpr int FD_KT = 10;               // compiled taps of the column operator, one of them the half-wave shift: KW <= 9
constexpr int FD_CE = 4;                // output columns per lane at the 446^2 level: Wo <= 256
constexpr int FD_CE2 = 2;               // ... and at the 223^2 level: Wo <= 128, the carried rows, the column sums and the taps take half the registers
constexpr int FD_WR = (FD_NC * 16 + 63) / 64;   // registers per lane that hold a tile's [FD_NC][16] piece of the row operator
// development builds (tools/dev/mkvariant.py ... -DUNO_FD_KO=mask): knock-outs for timing - 1: no column operator, 2: no row operator,
// 4: no stores of the resampled rows; 0 in production
#ifndef UNO_FD_KO
#define UNO_FD_KO 0
#endif
constexpr int FD_MINW = 416, FD_MAXW = 447;     // admitted row lengths (the 446^2 level; four 16 x W tiles + the tables fill the LDS)
// ... and the second window, the 223^2 level (CE = FD_CE2): a workgroup's four 16 x W tiles (14.4 KB each at W = 223) and its table set
// (18.6 KB for <2, 3, 1>) take 80.5 KB at 223 x 223, so TWO workgroups share a CU's 160 KB - two waves per SIMD, which is what lets one
// wave's column operator run under the other's MFMA stages.  The upper end is where that stops: at 225 the twiddle tables grow by a
// seventh 16-pair chunk (21.1 KB) and two workgroups of four no longer fit (224 itself puts the 16 rows of an operand read on four LDS
// banks).  The lower end is the one of K3-A's window at this level (dft2d_inv_add_kernel.h); the tail tables (FWD_TAILMAX k-steps: at most
// 15 pairs + w = 0 + the Nyquist column) hold for every row length.
constexpr int FD_MINW2 = 192, FD_MAXW2 = 223;
constexpr size_t FD_LDS_HALF = (160 * 1024) / 2 - 1024;     // per workgroup where two share a CU

// CE: output columns per lane (FD_CE | FD_CE2); the FD_CE2 instantiations are compiled for two waves per SIMD (<= 256 registers)
template <int NT, int MT, int R4, int CE = FD_CE>
__global__ __launch_bounds__(256, CE == FD_CE2 ? 2 : 1) void dft2d_fwd_fd_kernel(Dft2dParams p) {
    constexpr int NTF = R4 > 0 ? NT - 1 : NT;       // full 16-mode streams
    constexpr int NQ = R4 > 0 ? R4 : 1;
    constexpr int NTFA = NTF > 0 ? NTF : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = p.H, W = p.W, m1 = p.m1, m2 = p.m2;
    const int Ho = p.fd_Ho, Wo = p.fd_Wo;
    const int tid = threadIdx.x;
    const int nthreads = blockDim.x;
    const int NWT = nthreads >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int r16 = lane & 15;
    const int kk = lane >> 4;
    const unsigned H8 = 8u * H;
    UNO_FWD_COLUMN_PAIRS(W);
    const int nk = 4 * nfull + tailsteps;

    const int tile_stride = (16 * W + 32 + 3) & ~3;                            // tile + alignment phase
    float* sTile = reinterpret_cast<float*>(smem);                             // [NWT][tile_stride]
    float2* sTabF = reinterpret_cast<float2*>(sTile + (size_t)NWT * tile_stride);   // [nk][NTF][64]
    const int nka = UNO_FWD_TABLE_STEPS(nfull);                                    // allocated k-steps
    float2* sTab4 = sTabF + (size_t)nka * NTF * 64;                            // [nk][R4][16]
    float2* sTwH = sTab4 + (size_t)nka * R4 * 16;
    int* sTailW = reinterpret_cast<int*>(sTwH + H);                            // [FWD_TAILMAX][2][64]: left / right column of a tail element (-1 = none)

    // one wave per image, tiles in order (the carried rows need no cross-wave hand-over)
    const int image = sweep_x(p.rev) * NWT + wave;
    const bool active = image < p.n_img;
    const int nrt = (H + 15) >> 4;
    float* buf = sTile + (size_t)wave * tile_stride;

    // ---- direct-to-LDS tile loads
    int a0;
    const __amdgpu_buffer_rsrc_t rsrc = image_rsrc(p.in, p.n_img, H, W, active ? image : 0, &a0);
    auto request_tile = [&](int rt) {
        // tile rt occupies floats [toff, toff + rows W) from the aligned base; LDS index i <-> float (toff & ~31) + i
        const int toff = a0 + rt * 16 * W;
        const int rows = min(16, H - 16 * rt);
        const int total = (toff & 31) + rows * W;
        const int npiece = (total + 255) >> 8;
        const unsigned v0 = (unsigned)(((toff & ~31) + 4 * lane) * 4);
        for (int i = 0; i < npiece; ++i)
            if (256 * i + 4 * lane < total)         // the last piece stops at the end of the tile (lanes beyond it are masked off)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)(buf + 256 * i), 16, v0 + 1024u * (unsigned)i, 0, 0, FT_AUX);
    };
    if (active) request_tile(0);

    // ---- tables (built while the first tile is on its way)
    for (int n = tid; n < H; n += nthreads) sTwH[n] = p.twH[n];
    for (int e = tid; e < FWD_TAILMAX * 64; e += nthreads) { UNO_FWD_PUT_TAIL_COLUMNS(e); }
    UNO_FWD_BUILD_OPERAND_TABLES();

    // ---- column operator of this lane's CE output columns: first source column sc (moved so that all FD_KT reads stay inside the
    // row, and one to the left in the upper half wave) and the taps, moved up by as much; everything outside the band is an exact zero
    int sc[CE];
    float wc[CE][FD_KT];
    {
        const int KW = p.fd_KW;
#pragma unroll
        for (int e = 0; e < CE; ++e) {
            const int j = min(64 * e + lane, Wo - 1);
            const int s = p.fd_startW[j];
            sc[e] = max(min(s - (lane >> 5), W - FD_KT), 0);
            const int d = s - sc[e];
#pragma unroll
            for (int t = 0; t < FD_KT; ++t) {
                const int u = t - d;                // tap of the band table that meets source column sc + t
                const bool in = u >= 0 && u < KW && s + u < W;
                const float wv = p.fd_wtW[(size_t)j * KW + min(max(u, 0), KW - 1)];
                wc[e][t] = in ? wv : 0.f;
            }
        }
    }
    __syncthreads();

    UNO_FWD_ACCUMULATORS(false, MT);            // Xr, Xi: this wave's spectrum; Kj, jvalid: the corner rows this lane owns

    const float2* tabF = sTabF + lane;
    const float2* tab4 = sTab4 + 4 * kk + (lane & 3);

    float C[FD_NC][CE];                      // carried output rows ibase(tile) + c, columns 64 e + lane
#pragma unroll
    for (int c = 0; c < FD_NC; ++c)
#pragma unroll
        for (int e = 0; e < CE; ++e) C[c][e] = 0.f;

    if (active) {
        float* const oimg = p.fd_out + (size_t)image * Ho * Wo;
        // ---- the rows a tile completed: unit-stride stores, then the carried rows move down by their number.  Issued at the START of the
        // next tile (and after the last): the s_waitcnt vmcnt(0) that meets a tile also waits for every store before it, and right behind
        // the row operator that was 28 exposed store round trips per image (50 us of 410 at 1024 x 446^2, knock-out 4)
        int pend_ibase = 0, pend_ncomp = 0;
        auto flush_rows = [&]() {
#pragma unroll
            for (int c = 0; c < FD_NC; ++c) {
                if (c < pend_ncomp && (unsigned)(pend_ibase + c) < (unsigned)Ho && !(UNO_FD_KO & 4)) {
                    float* orow = oimg + (size_t)(pend_ibase + c) * Wo;
#pragma unroll
                    for (int e = 0; e < CE; ++e)
                        if (64 * e + lane < Wo) orow[64 * e + lane] = C[c][e];
                }
            }
#pragma unroll
            for (int n = 1; n < 16; n *= 2) {
                if (pend_ncomp & n) {
#pragma unroll
                    for (int c = 0; c < FD_NC; ++c)
#pragma unroll
                        for (int e = 0; e < CE; ++e) C[c][e] = (c + n < FD_NC) ? C[(c + n < FD_NC) ? c + n : 0][e] : 0.f;
                }
            }
        };
        for (int rt = 0; rt < nrt; ++rt) {
            const int toff = a0 + rt * 16 * W;
            const int phase = toff & 31;
            const int rows = min(16, H - 16 * rt);
            const float* row = buf + phase + r16 * W;           // this lane's image row inside the LDS tile
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the tile has landed
            flush_rows();
            if (rows < 16) {
                // rows past the image: zero them (their products are masked in stage B, but 0 * garbage could be NaN; the column
                // operator below turns them into exact zeros that meet zero row weights)
                for (int i = phase + rows * W + lane; i < phase + 16 * W; i += 64) buf[i] = 0.f;
            }
            // this tile's piece of the row operator, one entry per lane and register (handed out by v_readlane below: the stores of the
            // output rows keep the compiler from reading it through scalar loads), and its four descriptor words; they arrive under stage A
            const float* wd = p.fd_rowop + (size_t)rt * (FD_NC * 16);
            float wv[FD_WR];
#pragma unroll
            for (int k = 0; k < FD_WR; ++k) wv[k] = wd[min(64 * k + lane, FD_NC * 16 - 1)];
            int tinfo = p.fd_tiles[4 * rt + (lane & 3)];

            f32x4 Tr[NT], Tn[NT];           // Tn = -Im T
            f32x4 Qr[NQ], Qn[NQ];           // 4x4x1 accumulators of the 4-mode groups (R4 > 0)
#pragma unroll
            for (int t = 0; t < NT; ++t) { Tr[t] = f32x4{0, 0, 0, 0}; Tn[t] = f32x4{0, 0, 0, 0}; }
#pragma unroll
            for (int g = 0; g < NQ; ++g) { Qr[g] = f32x4{0, 0, 0, 0}; Qn[g] = f32x4{0, 0, 0, 0}; }
#define UNO_FD_MFMA(E_, D_, TWF_, TW4_)                                                   \
    do {                                                                                  \
        _Pragma("unroll") for (int t = 0; t < NTF; ++t) {                                 \
            Tr[t] = mfma16((E_), (TWF_)[t].x, Tr[t]);                                     \
            Tn[t] = mfma16((D_), (TWF_)[t].y, Tn[t]);                                     \
        }                                                                                 \
        _Pragma("unroll") for (int g = 0; g < R4; ++g) {                                  \
            Qr[g] = mfma4((E_), (TW4_)[g].x, Qr[g]);                                   \
            Qn[g] = mfma4((D_), (TW4_)[g].y, Qn[g]);                                   \
        }                                                                                 \
    } while (0)

            // ---- stage A (the full-tile form's), full chunks: lane (row r16, k-slot kk) owns column pairs w = 1 + 16 c + 4 kk + s, s = 0..3;
            // image operands AND twiddles of chunk c + 1 are requested before the MFMAs of chunk c are issued
            struct RowOps { float xl[4], xr[4]; float2 twF[4][NTFA], tw4[4][NQ]; };
            RowOps opA, opB;
            const float* pl = row + 1 + 4 * kk;                 // left columns of chunk 0
            const float* pr = row + W - 4 - 4 * kk;             // mirrored columns of chunk 0 (ascending address)
            auto load_ops = [&](RowOps& o, int c) {
                // k-steps 4 c .. 4 c + 3: chunk c, or (c = nfull) the first tail k-steps' twiddles with the last chunk's (unused) image values
                const int cn = min(c, max(nfull - 1, 0));
                const float2* tf = tabF + (size_t)(4 * c) * (NTF * 64);
                const float2* t4 = tab4 + (size_t)(4 * c) * (R4 * 16);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    o.xl[s] = pl[16 * cn + s]; o.xr[s] = pr[-16 * cn + s];
#pragma unroll
                    for (int t = 0; t < NTF; ++t) o.twF[s][t] = tf[(s * NTF + t) * 64];
#pragma unroll
                    for (int g = 0; g < R4; ++g) o.tw4[s][g] = t4[(s * R4 + g) * 16];
                }
            };
            auto chunk = [&](RowOps& cur, RowOps& nxt, int c) {
                load_ops(nxt, c + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float E = cur.xl[s] + cur.xr[3 - s];
                    const float D = cur.xl[s] - cur.xr[3 - s];
                    UNO_FD_MFMA(E, D, cur.twF[s], cur.tw4[s]);
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            load_ops(opA, 0);
            {
                int c = 0;
                for (; c + 2 <= nfull; c += 2) { chunk(opA, opB, c); chunk(opB, opA, c + 1); }
                if (c < nfull) { chunk(opA, opB, c); opA = opB; }               // (odd chunk count: one copy per tile)
            }
            float2 (&twF)[4][NTFA] = opA.twF;
            float2 (&tw4)[4][NQ] = opA.tw4;
            // ---- tail k-steps: pairs beyond the last full chunk, then w = 0, then the Nyquist column; the twiddles of the first
            // four are already in twF / tw4
            {
                const float2* tf = tabF + (size_t)(4 * nfull) * (NTF * 64);
                const float2* t4 = tab4 + (size_t)(4 * nfull) * (R4 * 16);
                float TL[FWD_TAILMAX], TR[FWD_TAILMAX];
#pragma unroll
                for (int s = 0; s < FWD_TAILMAX; ++s) {
                    const int wl = sTailW[(s * 2 + 0) * 64 + lane], wr = sTailW[(s * 2 + 1) * 64 + lane];
                    const float vl = row[max(wl, 0)], vr = row[max(wr, 0)];
                    TL[s] = wl >= 0 ? vl : 0.f; TR[s] = wr >= 0 ? vr : 0.f;
                }
                float2 twF5[NTFA], tw45[NQ];
#pragma unroll
                for (int t = 0; t < NTF; ++t) twF5[t] = tf[(4 * NTF + t) * 64];
#pragma unroll
                for (int g = 0; g < R4; ++g) tw45[g] = t4[(4 * R4 + g) * 16];
#pragma unroll
                for (int s = 0; s < FWD_TAILMAX; ++s) {
                    if (s < tailsteps) {
                        const float E = TL[s] + TR[s];
                        const float D = TL[s] - TR[s];
                        if (s < 4) UNO_FD_MFMA(E, D, twF[s], tw4[s]);
                        else UNO_FD_MFMA(E, D, twF5, tw45);
                    }
                }
            }
#undef UNO_FD_MFMA

            // ---- column operator on the 16 tile rows, from LDS (rows past the image are zero)
            float Y[16][CE];
            {
                // the reads of row r + 1 are issued before the products of row r (two operand sets in ping-pong; sched_barrier keeps the
                // compiler from hoisting all 640 reads of the tile to the front, which spilled)
                const float* trow = buf + phase;
                float xv[2][CE][FD_KT];
                auto read_row = [&](float (&x)[CE][FD_KT], int r) {
#pragma unroll
                    for (int e = 0; e < CE; ++e) {
                        const float* q = trow + r * W + sc[e];
#pragma unroll
                        for (int t = 0; t < FD_KT; ++t) x[e][t] = q[t];
                    }
                };
                if (!(UNO_FD_KO & 1)) read_row(xv[0], 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (UNO_FD_KO & 1) { for (int e = 0; e < CE; ++e) Y[r][e] = 0.f; continue; }
                    if (r + 1 < 16) read_row(xv[(r + 1) & 1], r + 1);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int e = 0; e < CE; ++e) {
                        float acc = 0.f;
#pragma unroll
                        for (int t = 0; t < FD_KT; ++t) acc = fmaf(wc[e][t], xv[r & 1][e][t], acc);
                        asm volatile("" : "+v"(acc));           // (keeps the sum here: its only readers sit under the uniform branches of the row operator)
                        Y[r][e] = acc;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // the row stage and the column operator have read the tile: request the next one, it lands during what follows
            // (the operator piece is taken through an empty asm first: the compiler waits for it HERE, not after the tile loads, whose
            // number it cannot count - that wait would be for the whole next tile)
#pragma unroll
            for (int k = 0; k < FD_WR; ++k) asm volatile("" : "+v"(wv[k]));
            asm volatile("" : "+v"(tinfo));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (rt + 1 < nrt) request_tile(rt + 1);

            // ---- row operator into the carried rows (wave-uniform weights; all-zero 4-row pieces skipped)
            const int ibase = __builtin_amdgcn_readlane(tinfo, 0);
            const int ncomp = __builtin_amdgcn_readlane(tinfo, 1);
            const unsigned mlo = (unsigned)__builtin_amdgcn_readlane(tinfo, 2);
            const unsigned mhi = (unsigned)__builtin_amdgcn_readlane(tinfo, 3);
#pragma unroll
            for (int c = 0; c < FD_NC; ++c) {
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const int b = 4 * c + q4;
                    const unsigned bit = b < 32 ? (mlo >> (b & 31)) & 1u : (mhi >> ((b - 32) & 31)) & 1u;
                    if (bit && !(UNO_FD_KO & 2)) {
#pragma unroll
                        for (int r = 4 * q4; r < 4 * q4 + 4; ++r) {
                            const float w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wv[(c * 16 + r) >> 6]), (c * 16 + r) & 63));
#pragma unroll
                            for (int e = 0; e < CE; ++e) C[c][e] = fmaf(w, Y[r][e], C[c][e]);
                        }
                    }
                }
            }
            // (the rows this tile completed leave at the start of the next tile, see flush_rows)
            pend_ibase = ibase;
            pend_ncomp = ncomp;

            UNO_FWD_REGROUP_4X4();              // the 4-mode groups join Tr / Tn
            UNO_FWD_STAGE_B(false, MT);         // columns: X += F T
        }
        flush_rows();
    }

    if (active) UNO_FWD_STORE_SPECTRUM(false, MT, image);
}

// ---- launcher side
// one wave per image whatever the image count (fwd_tile_geometry would give a lone image several waves): up to four images per workgroup
// output columns per lane of the window W belongs to; 0: outside both
static int fwd_fd_columns_per_lane(int W) {
    return (W >= FD_MINW && W <= FD_MAXW) ? FD_CE : ((W >= FD_MINW2 && W <= FD_MAXW2) ? FD_CE2 : 0);
}

static bool fwd_fd_geometry(const Dft2dParams& p, int NT, int MT, int R4, FwdFtGeometry* out) {
    (void)MT;
    const int NTF = R4 > 0 ? NT - 1 : NT;
    const int ce = fwd_fd_columns_per_lane(p.W);
    if (p.bf16 || p.rowfreq || ce == 0) return false;
    if (p.fd_Ho < 1 || p.fd_Wo < 1 || p.fd_Wo > 64 * ce || p.fd_KW < 1 || p.fd_KW > FD_KT - 1) return false;
    if ((long long)p.fd_Ho * p.fd_Wo > 0x7fffffffLL / 4) return false;
    const int cus = ft_device_cu_count();
    // 223^2 level: up to four images per workgroup and two workgroups per CU (the LDS of each within half a CU's); where four tiles and
    // the tables do not fit that, fewer images per workgroup
    const size_t budget = ce == FD_CE2 ? FD_LDS_HALF : FT_LDS_BUDGET;
    int g = 4;
    while (g > 1 && (long long)(p.n_img + g - 1) / g < cus) --g;
    while (g > 1 && fwd_ft_lds_bytes(p, NTF, R4, g) > budget) --g;
    const size_t lds = fwd_ft_lds_bytes(p, NTF, R4, g);
    if (lds > budget) return false;
    *out = FwdFtGeometry{1, g, lds};
    return true;
}

template <int NT, int MT, int R4, int CE = FD_CE>
static int launch_fwd_fd(Dft2dParams p, const FwdFtGeometry& g, hipStream_t s) {
    auto K = dft2d_fwd_fd_kernel<NT, MT, R4, CE>;
    static int lds_slot[64];
    if (!ensure_dynamic_lds(reinterpret_cast<const void*>(K), g.lds, lds_slot)) { set_error("dft2d_fwd_fd: cannot raise dynamic LDS to %zu", g.lds); return -4; }
    char name[64];
    if constexpr (CE == FD_CE) snprintf(name, sizeof(name), "uno::dft2d_fwd_fd_kernel<%d, %d, %d>", NT, MT, R4);
    else snprintf(name, sizeof(name), "uno::dft2d_fwd_fd_kernel<%d, %d, %d, %d>", NT, MT, R4, CE);
    p.nw = 1;
    p.rev = fwd_ft_sweep();             // once per launch, the K1 family's counter
    {
        ProfScope prof(name, (double)p.n_img * ((double)p.H * p.W * 4.0 + (double)p.fd_Ho * p.fd_Wo * 4.0 + 2.0 * p.m1 * p.m2 * 8.0), s);
        hipLaunchKernelGGL(K, dim3((p.n_img + g.g - 1) / g.g), dim3(64 * g.g), g.lds, s, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("dft2d_fwd_fd launch: %s", hipGetErrorString(e)); return -5; }
    return 0;
}

}  // namespace uno
