// K3-A - K3 (full-tile form) with the UP-SAMPLED point-wise branch added in registers before the tile is staged:
//
//   y[h][w] = Re iDFT_trunc(O)[h][w]  +  sum_{u,v} Rh[h][u] Rw[w][v] t[u][v]
//
// i.e. `x1_out + x2_out` of an up-sampling operator block (reference integral_operators.py:272-273, with x2_out =
// F.interpolate(conv(x), bicubic, align_corners, antialias), :240-242, evaluated from the LOW-resolution 1x1-convolution result t)
// and, transposed, the input gradient of a down-sampling block.  Rounds 1-5 ran this as K3 (writes y) followed by the accumulating
// form of K7 (reads t, reads y, writes y): 1.83 GB for an ideal 1.02 GB at the 223^2 -> 446^2 level of the Darcy model, the largest
// family of the step.  Here y is written once and t is read (twice, from L2) by the kernel that produces y.
//
// Why this form and not the one costed in round 2 (~1 700 VALU / LDS instructions per tile, LDS full at 446 columns): the kernel is
// bound by its stores with the MFMA pipe ~40 % busy, LDS is full (4 x 28.9 KB of tiles + 35.8 KB twiddle operands of 160 KB), one wave
// per SIMD leaves nothing to hide VALU work behind - but MFMA slots are free.  Both 1-D operators are banded: a 16-row output tile
// reads <= 12 rows of t, 16 output columns read <= 12 columns (up-sampling by two or more).  So per (column tile, side):
//   stage 1'  C^T[u][w] = sum_v t[u][v] Rw[w][v]      A operand = t straight from global: lane (row u, k-slot kk) loads the 12-byte piece
//                                                     t[u][v0 + 3 kk .. + 2] - ONE load per lane, k-step ks <-> column v0 + 3 kk + ks;
//                                                     B operand = the column operator in operand layout, loop-invariant: registers
//   stage 2'  D[w][h]  += sum_u C^T[u][w] Rh[h][u]    the stage-1' accumulators ARE the A operand (register e of lane (kk, n) = row
//                                                     u = 3 kk + e of C^T, column n: the trick K3's own two stages use);
//                                                     B operand = the row operator of the tile: three registers per tile
// D[w][h] comes out in the layout of the transform's own result (lane (h, g): columns 4 g .. 4 g + 3 of the column tile and, for the
// mirrored side, W - (4 g ..)), so the addend meets the transform in registers: 6 + 6 MFMAs per column tile next to the transform's
// 2 KS, no LDS, ~4 VALU.
// Memory ordering: loads and stores share the vmcnt counter, and this kernel lives on stores that drain asynchronously over a whole
// tile time - waiting for a load means waiting for every store issued before it (knock-outs, tools/dev/k3a_time.py: with the loads
// requested AFTER the column loop the kernel took 397 us, 267 without the loads, 187 without loads and addend MFMAs = K3 alone).  So the
// loads of tile rt + 1 (28 pieces of t + 3 operator registers) are issued at the TOP of tile rt, straight behind the stores of tile
// rt - 1, and consumed after tile rt's column loop (stage 1' of every column tile, results parked in registers) but before tile rt's
// stores are issued: what they wait for has had a whole column loop to drain.  The column loop is fully unrolled (NWTM column tiles) so
// that the parked operands are registers.
#pragma once
#include "dft2d_inv_kernel.h"
#include <type_traits>

namespace uno {

constexpr int ADD_KE = 3;           // k-steps of both banded operators: bands of <= 12 source rows / columns per 16 outputs

__device__ __forceinline__ f32x4 f4(float a, float b, float c, float d) { return f32x4{a, b, c, d}; }
typedef float f32x3 __attribute__((ext_vector_type(3)));

template <int KS, int KSK, int NWTM>
__global__ __launch_bounds__(256, ((NWTM <= 7 && KS <= 4) ? 2 : 1)) void dft2d_inv_ft_add_kernel(Dft2dParams p) {
    constexpr int NT = (KS + 3) / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    UNO_INV_GRID_LOCALS();
    constexpr int nwt = NWTM;                                              // == inv_col_tiles(W) (launcher): the column loop is straight-line code
    UNO_INV_FT_LDS();
    UNO_INV_LANE_LOCALS();
    const unsigned H8 = 8u * H;

    UNO_INV_FILL_ROW_TWIDDLES();
    UNO_INV_BUILD_OPERAND_TABLE()
    __syncthreads();

    UNO_INV_WAVE_IMAGE();
    const int ko = p.exp & 0xff;                 // development knock-outs: 1 no addend loads, 2 no spectrum reload, 4 no stores, 8 no stage 1', 16 no stage 2'
    // KSK == (m1 + 4) >> 2 k-steps of the column stage exactly (K3 compiles 2 JT + 1 >= that and skips the rest at run time: here every
    // register counts)
    constexpr int ksk = KSK;
    constexpr bool EARLY = !(NWTM <= 7 && KS <= 4);      // one wave per SIMD: operands requested DURING the tile's column loop; two waves per SIMD: after it
    const float2* O = UNO_INV_SPECTRUM(image);

    // ---- the addend's loop-invariant operands: column operator, B operand of stage 1' (lane (k-slot kk, column n = r16))
    const int Hs = p.add_Hs, Ws = p.add_Ws;
    float colB[NWTM][2][ADD_KE];
#pragma unroll
    for (int wt = 0; wt < NWTM; ++wt)
#pragma unroll
        for (int sd = 0; sd < 2; ++sd)
#pragma unroll
            for (int ks = 0; ks < ADD_KE; ++ks)
                colB[wt][sd][ks] = p.add_colop[((size_t)(wt * 2 + sd) * ADD_KE + ks) * 64 + lane];
    // t of this image through a buffer resource: reads past the image return zero (they only ever meet zero weights)
    const float* timg = p.add_src + (size_t)image * Hs * Ws;
    const __amdgpu_buffer_rsrc_t trsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(timg), 0, Hs * Ws * 4, 0x00020000);
    // A-operand row of this lane: MFMA row m = r16 = 4 a + e <-> source row p0 + 3 a + e (e < 3; e = 3: unused, any valid row)
    const int urel = ADD_KE * (r16 >> 2) + min(r16 & 3, ADD_KE - 1);

    float* img = p.out + (size_t)image * H * W;
    const int nrt = (H + 15) >> 4;
    UNO_INV_FT_WAVE_TILE();

    // column stage's A operand, once per image
    UNO_INV_COLUMN_OPERAND(!(ko & 2))
    f32x4 Ur[NT], Ui[NT];
    auto stage_b = [&](int rt) { UNO_INV_STAGE_B(rt, (void)0) };
    // the addend of row tile rt, first half: operands requested (request), stage 1' of every column tile (reduce) -> Ct
    float rowB[ADD_KE], rowN[ADD_KE];           // row operator of the tile (B operand of stage 2') and of the next one
    f32x3 piece[NWTM][2];
    f32x4 Ct[NWTM][2];                          // C^T of (column tile, side): A operand of stage 2'
    // first source column of every (column tile, side), byte offset, once (scalar registers): a load of the table inside the tile loop
    // is no longer provably unclobbered and becomes a vector load + readfirstlane loop in the middle of the MFMA stream
    int v0s[NWTM][2];
#pragma unroll
    for (int wt = 0; wt < NWTM; ++wt)
#pragma unroll
        for (int sd = 0; sd < 2; ++sd) v0s[wt][sd] = __builtin_amdgcn_readfirstlane(p.add_v0[wt * 2 + sd] * 4);
    int voff_next = 0;
    auto request_rows = [&](int rt) {            // row operator of tile rt + this lane's byte offset into t for its pieces
        if (ko & 1) {
#pragma unroll
            for (int e = 0; e < ADD_KE; ++e) rowN[e] = 0.f;
            return;
        }
#pragma unroll
        for (int e = 0; e < ADD_KE; ++e) rowN[e] = p.add_rowop[((size_t)rt * ADD_KE + e) * 64 + lane];
        const int p0 = __builtin_amdgcn_readfirstlane(p.add_p0[rt]);
        voff_next = (min(p0 + urel, Hs - 1) * Ws + ADD_KE * kk) * 4;
    };
    auto request_piece = [&](int wt) {           // the two 12-byte pieces of column tile wt (compile-time wt)
        if (ko & 1) { piece[wt][0] = f32x3{0, 0, 0}; piece[wt][1] = f32x3{0, 0, 0}; return; }
#pragma unroll
        for (int sd = 0; sd < 2; ++sd) {
            piece[wt][sd] = __builtin_bit_cast(f32x3, __builtin_amdgcn_raw_buffer_load_b96(trsrc, voff_next, v0s[wt][sd], 0));
        }
    };
    auto request = [&](int rt) {
        request_rows(rt);
#pragma unroll
        for (int wt = 0; wt < NWTM; ++wt) request_piece(wt);
    };
    auto reduce = [&]() {
#pragma unroll
        for (int e = 0; e < ADD_KE; ++e) rowB[e] = rowN[e];
        if (ko & 8) {
#pragma unroll
            for (int wt = 0; wt < NWTM; ++wt) { Ct[wt][0] = f32x4{0, 0, 0, 0}; Ct[wt][1] = f32x4{0, 0, 0, 0}; }
            return;
        }
#pragma unroll
        for (int wt = 0; wt < NWTM; ++wt) {
            f32x4 c0 = f32x4{0, 0, 0, 0}, c1 = f32x4{0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < ADD_KE; ++ks) {
                c0 = mfma16(piece[wt][0][ks], colB[wt][0][ks], c0);
                c1 = mfma16(piece[wt][1][ks], colB[wt][1][ks], c1);
            }
            Ct[wt][0] = c0; Ct[wt][1] = c1;
        }
    };

    // de-phase the waves (development knob p.exp: units of 512 cycles per wave index / workgroup parity)
    if ((p.exp >> 8) > 0) {
        const int nsl = ((wave & 3) + 4 * (int)(blockIdx.x & 1)) * (p.exp >> 8);
        for (int i = 0; i < nsl; ++i) __builtin_amdgcn_s_sleep(8);
    }
    if (wsub < nrt) { request(wsub); stage_b(wsub); reduce(); }

    for (int rt = wsub; rt < nrt; rt += NW) {
        UNO_INV_FT_TILE(rt);
        const int nfast = inv_ft_fast_tiles(rows, nwt, wfast_hi);
        const bool more = rt + NW < nrt;
        // the NEXT tile's addend operands are requested now, straight behind the previous tile's stores: they land while this tile's
        // column loop runs (that is also the time those stores have to drain - loads and stores share one in-order counter)
        if (EARLY) request_rows(more ? rt + NW : rt);        // (last tile: valid addresses, results unused - no control flow around the loads)

        // ---- stage A' + stage 2' of the addend, column tile by column tile; tile wt - 1 is staged under tile wt's MFMAs.
        // FULL: all 16 rows exist - column tiles 1 .. NWTM - 2 need no guards, the last one by a uniform test
        asm volatile("" ::: "memory");          // the (tile-invariant) twiddle reads of the unrolled column loop stay inside the tile loop: registers
        auto columns = [&](auto full_t) {
            constexpr bool FULL = decltype(full_t)::value;
            f32x4 Ey[2], Dy[2], aL[2], aR[2];
            float2 tw[2][KS];
#pragma unroll
            for (int sp = 0; sp < KS; ++sp) tw[0][sp] = tabLane[sp * 64];
            auto stage = [&](int wt, bool fast, const f32x4& E, const f32x4& D, const f32x4& al, const f32x4& ar) {
                UNO_INV_FT_STAGE(wt, fast, E - D + al, E + D + ar)
            };
            auto is_fast = [&](int wt) { return FULL && wt >= 1 && (wt < NWTM - 1 || wt < nfast); };
#pragma unroll
            for (int wt = 0; wt < NWTM; ++wt) {
                const int cur = wt & 1, nx = cur ^ 1;
                f32x4 E, D, al = f32x4{0, 0, 0, 0}, ar = f32x4{0, 0, 0, 0};
                UNO_INV_ROW_CHAIN(wt + 1 < NWTM ? wt + 1 : wt, tw[cur], tw[nx], E, D, KS > ADD_KE ? KS : ADD_KE,
                                  if (sp < ADD_KE && !(ko & 16)) { al = mfma16(Ct[wt][0][sp], rowB[sp], al); ar = mfma16(Ct[wt][1][sp], rowB[sp], ar); })
                Ey[cur] = E; Dy[cur] = D; aL[cur] = al; aR[cur] = ar;
                // the NEXT row tile's pieces of this column tile, spread over the column loop: the previous tile's stores are still
                // draining through the same path, two loads at a time slip in between them (all 28 at the top of the tile: 343 us)
                if (EARLY) request_piece(wt);
                if (wt >= 1) stage(wt - 1, is_fast(wt - 1), Ey[nx], Dy[nx], aL[nx], aR[nx]);
            }
            stage(NWTM - 1, is_fast(NWTM - 1), Ey[(NWTM - 1) & 1], Dy[(NWTM - 1) & 1], aL[(NWTM - 1) & 1], aR[(NWTM - 1) & 1]);
        };
        if (rows == 16) columns(std::true_type{}); else columns(std::false_type{});

        // ---- next tile: operands requested, column stage and stage 1' done BEFORE this tile's stores are issued (header)
        if (more) {
            if (!EARLY) request(rt + NW);
            stage_b(rt + NW);
            reduce();
        }

        UNO_INV_FT_STORE_TILE(more, !(ko & 4), (void)0)
    }
}

// ---- launcher side: the form applies where K3-FT does (same LDS geometry), the column tiles fit the unrolled loop and the operand
// tables are given
static bool inv_add_shape_ok(const Dft2dParams& p) {
    const int nwt = inv_col_tiles(p.W);
    const int KS = (p.m2 + 3) / 4, KSK = (p.m1 + 4) >> 2;
    // (the unrolled column loop is compiled for 7 and 14 column tiles: rows of 192 .. 223 and 416 .. 447 elements)
    return (nwt == 7 || nwt == 14) && KS <= 6 && KSK >= 1 && KSK <= 7 && !p.bf16 && p.add_Ws >= 4 * ADD_KE && p.add_Hs >= 1;
}

template <int KS, int KSK, int NWTM>
static int launch_inv_add(const Dft2dParams& p, const InvGeometry& g, hipStream_t s) {
    char name[64];
    snprintf(name, sizeof(name), "uno::dft2d_inv_ft_add_kernel<%d, %d, %d>", KS, KSK, NWTM);
    const double bytes = (double)p.n_img * ((double)p.H * p.W * 4.0 + (double)p.add_Hs * p.add_Ws * 4.0 + 2.0 * p.m1 * p.m2 * 8.0);
    return launch_inv<dft2d_inv_ft_add_kernel<KS, KSK, NWTM>>(name, bytes, "dft2d_inv_add", p, g, next_sweep_reversed(SWEEP_K3), s);
}

template <int KS, int KSK>
static int launch_inv_add_t(const Dft2dParams& p, hipStream_t s) {
    InvGeometry ft;
    if (!inv_ft_geometry(p, KS, &ft)) { set_error("dft2d_inv_add: the full-tile form does not apply to %dx%d", p.H, p.W); return -3; }
    if (inv_col_tiles(p.W) == 7) return launch_inv_add<KS, KSK, 7>(p, ft, s);
    return launch_inv_add<KS, KSK, 14>(p, ft, s);
}

}  // namespace uno
