// K1, full-tile form - pruned forward 2-D DFT with the image tile staged in LDS.
//
// Same mathematics and the same MFMA structure as dft2d_fwd_kernel (dft2d_fwd_kernel.h: symmetric row stage on
// v_mfma_f32_16x16x4_f32 / 4x4x1_16b, stage-A accumulators consumed as the stage-B operand in place), but the two things that
// bound that kernel are gone (measured):
//   * its A operand came straight from global memory as 16 rows x 64-byte pieces at 4-byte alignment, two pieces per
//     instruction, three chunks (6 KB) in flight per wave: latency-bound at 3.4 TB/s.  Here a wave's 16 x W tile - ONE
//     contiguous run of the image - is copied into LDS by direct-to-LDS loads (buffer_load_dwordx4 ... lds: 1 KB of whole
//     128-byte lines per instruction, no VGPRs, the entire 27 KB tile in flight at once), placed at its memory offset modulo
//     128 bytes; the next tile is requested as soon as the row stage has read the current one, so the transfer runs under
//     the column stage.
//   * its B operand (twiddles) was gathered from a W-entry table by an integer-walked index (3 VALU + a conflict-prone
//     gather per operand).  Here the workgroup tabulates cos / sin(2 pi l w / W) once in MFMA operand layout
//     [k-step][stream][lane]; the inner loop reads it at immediate offsets.
// 27 KB of tile per wave + 36 KB of table let four waves share a CU (one per SIMD) - enough for the MFMA pipe because nothing
// in a wave's instruction stream waits on HBM any more except the one s_waitcnt per tile.
#pragma once
#include "dft2d_fwd_common.h"

namespace uno {

constexpr size_t FT_LDS_BUDGET = 160 * 1024 - 2048;
constexpr int FT_AUX = 2;               // cache policy of the tile loads: 2 = non-temporal (each line is read once)
constexpr int FT_MAXW = 160;            // widest image the full-tile form takes (see fwd_ft_geometry)

template <int NT, int MT, int R4>
__global__ __launch_bounds__(256) void dft2d_fwd_ft_kernel(Dft2dParams p) {
    constexpr int NTF = R4 > 0 ? NT - 1 : NT;       // full 16-mode streams
    constexpr int NQ = R4 > 0 ? R4 : 1;
    constexpr int NTFA = NTF > 0 ? NTF : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = p.H, W = p.W, m1 = p.m1, m2 = p.m2;
    const int tid = threadIdx.x;
    const int nthreads = blockDim.x;
    const int NWT = nthreads >> 6;
    const int NW = p.nw;
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

    const int slot = wave / NW, wsub = wave - slot * NW;
    const int image = sweep_x(p.rev) * (NWT / NW) + slot;
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
    if (active && wsub < nrt) request_tile(wsub);

    // ---- tables (built while the first tile is on its way)
    for (int n = tid; n < H; n += nthreads) sTwH[n] = p.twH[n];
    for (int e = tid; e < FWD_TAILMAX * 64; e += nthreads) { UNO_FWD_PUT_TAIL_COLUMNS(e); }
    UNO_FWD_BUILD_OPERAND_TABLES();
    __syncthreads();

    UNO_FWD_ACCUMULATORS(false, MT);            // Xr, Xi: this wave's partial spectrum; Kj, jvalid: the corner rows this lane owns

    const float2* tabF = sTabF + lane;
    const float2* tab4 = sTab4 + 4 * kk + (lane & 3);

    if (active) {
        for (int rt = wsub; rt < nrt; rt += NW) {
            const int toff = a0 + rt * 16 * W;
            const int phase = toff & 31;
            const int rows = min(16, H - 16 * rt);
            const float* row = buf + phase + r16 * W;           // this lane's image row inside the LDS tile
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the tile has landed
            if (rows < 16) {
                // rows past the image: zero them (their products are masked in stage B, but 0 * garbage could be NaN)
                for (int i = phase + rows * W + lane; i < phase + 16 * W; i += 64) buf[i] = 0.f;
            }

            f32x4 Tr[NT], Tn[NT];           // Tn = -Im T
            f32x4 Qr[NQ], Qn[NQ];           // 4x4x1 accumulators of the 4-mode groups (R4 > 0)
#pragma unroll
            for (int t = 0; t < NT; ++t) { Tr[t] = f32x4{0, 0, 0, 0}; Tn[t] = f32x4{0, 0, 0, 0}; }
#pragma unroll
            for (int g = 0; g < NQ; ++g) { Qr[g] = f32x4{0, 0, 0, 0}; Qn[g] = f32x4{0, 0, 0, 0}; }
#define UNO_FT_MFMA(E_, D_, TWF_, TW4_)                                                   \
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

            // ---- stage A, full chunks: lane (row r16, k-slot kk) owns column pairs w = 1 + 16 c + 4 kk + s, s = 0..3.
            // One wave per SIMD: image operands AND twiddles of chunk c + 1 are requested before the MFMAs of chunk c are issued
            // (sched_barrier keeps the requests there), so no LDS latency sits in front of an MFMA.
            // (two operand sets in ping-pong, as in the half-tile form: no copies of the next chunk's operands after every MFMA block)
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
                    UNO_FT_MFMA(E, D, cur.twF[s], cur.tw4[s]);
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
                        if (s < 4) UNO_FT_MFMA(E, D, twF[s], tw4[s]);
                        else UNO_FT_MFMA(E, D, twF5, tw45);
                    }
                }
            }
#undef UNO_FT_MFMA
            // the row stage has read the tile: request the next one, it lands during stage B
            if (rt + NW < nrt) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                request_tile(rt + NW);
            }

            UNO_FWD_REGROUP_4X4();              // the 4-mode groups join Tr / Tn
            UNO_FWD_STAGE_B(false, MT);         // columns: X += F T
        }
    }

    // ---- several waves per image: the partial spectra are combined through the (now free) tile buffers
    if (NW > 1) __syncthreads();            // every wave of the workgroup is done with its tile buffer
    for (int stride = 2; stride >= 1; stride >>= 1) {
        if (stride >= NW) continue;
        UNO_FWD_REDUCE_STEP(Xr, Xi, MT, buf, sTile + (size_t)(wave - stride) * tile_stride, wsub, stride);
    }
    if (active && wsub == 0) UNO_FWD_STORE_SPECTRUM(false, MT, image);
}

// ---- launcher side
static size_t fwd_ft_lds_bytes(const Dft2dParams& p, int NTF, int R4, int waves) {
    const size_t tile_stride = (size_t)((16 * p.W + 32 + 3) & ~3);
    // (the reduction reuses the tile buffers)
    return (size_t)waves * tile_stride * 4 + fwd_table_bytes(p.W, NTF, R4) + (size_t)p.H * 8 + FWD_TAILMAX * 2 * 64 * 4;
}

// four waves per workgroup; a CU should hold (nearly) one wave per SIMD
static bool fwd_ft_geometry(const Dft2dParams& p, int NT, int MT, int R4, FwdFtGeometry* out) {
    const int NTF = R4 > 0 ? NT - 1 : NT;
    // the tile's rows sit W floats apart: W % 8 == 0 puts the 16 rows of an operand read on 4 or fewer LDS banks
    if (p.bf16 || p.rowfreq || p.W % 8 == 0 || ((p.W - 1) >> 1) < 16) return false;
    // Measured (tools/kbench.py, 1024 images x 64 ch): 111^2 18.5 us against 21.5 for the register-path kernel, 223^2 47.9 / 47.3,
    // 421^2 243 / 212: with one wave per SIMD the row stage's LDS / VALU work and its MFMAs run back to back instead of
    // overlapping (ablations: 64 us of operand traffic + 83 us of row-stage MFMAs + 40 us of column stage + 60 us of exposed
    // tile loads), which the three waves per SIMD of the register path hide.  Large tiles therefore stay on that kernel.
    if (p.W > FT_MAXW) return false;
    if ((size_t)MT * NT * 8 * 64 > (size_t)16 * p.W) return false;             // reduction slots must fit a tile buffer
    return fwd_tile_geometry(p, NTF, R4, FwdTileForm{4, FT_LDS_BUDGET, 3, fwd_ft_lds_bytes}, out);
}

// the sweep direction of one launch of a full-tile form (this kernel and dft2d_fwd_fd_kernel.h, which shares its stage A and its counter)
static int fwd_ft_sweep() { return next_sweep_reversed(SWEEP_K1); }

template <int NT, int MT, int R4>
static int launch_fwd_ft(const Dft2dParams& p, const FwdFtGeometry& g, hipStream_t s) {
    char name[64];
    snprintf(name, sizeof(name), "uno::dft2d_fwd_ft_kernel<%d, %d, %d>", NT, MT, R4);
    return launch_fwd_tile<dft2d_fwd_ft_kernel<NT, MT, R4>>(name, p, g, fwd_ft_sweep(), s);
}

}  // namespace uno
