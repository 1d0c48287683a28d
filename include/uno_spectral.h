/* uno_spectral.h - C ABI of the MI355X-native U-NO spectral-convolution hot path.
 *
 * Drop-in boundary for the path BASELINE.json's north_star names: the reference
 * (ashiq24/UNO) has no FFI - the path is Python calling torch ops - so each entry point
 * below replaces one span of reference Python; the binding a maintainer adds is the
 * ctypes stub shown in INTEGRATION.md (uno_amd/_native.py is that stub, in-tree).
 *
 * Conventions
 *  - every pointer is DEVICE memory of the current HIP device, borrowed for the call;
 *  - float tensors are contiguous float32; complex tensors are interleaved (re, im)
 *    float32 pairs (torch.complex64 / view_as_real layout), passed as float*;
 *  - `stream` is a hipStream_t (NULL = default stream); calls only enqueue work;
 *  - return 0 on success, <0 on error (uno_last_error() gives the message; nothing was
 *    enqueued for argument errors).  Error classes mirror what the reference surfaces as
 *    torch RuntimeError: shape/mode incompatibilities.
 *  - truncated-spectrum layout: (batch, channels, corner-rows = 2*modes1, modes2) for 2-D
 *    with the "lo" corner rows first (rows [:modes1] of rfft2) then the "hi" corner rows
 *    (rows [-modes1:]).
 *  - no state is retained between calls except immutable per-(device, N) twiddle tables.
 */
#ifndef UNO_SPECTRAL_H
#define UNO_SPECTRAL_H

#ifdef __cplusplus
extern "C" {
#endif

#define UNO_SPECTRAL_ABI_VERSION 14

/* ABI version of the loaded library (== UNO_SPECTRAL_ABI_VERSION it was built with). */
int uno_abi_version(void);
/* ABI 12 (no reference counterpart).  `bytes` bytes of host data in a fresh device allocation of the current device that is never
 * freed (an operand table a binding caches per shape), complete on return; NULL on failure.  Unlike a plain hipMalloc + hipMemcpy it
 * may be called while a stream is being captured into a hipGraph - the library's own tables are built this way, so a shape that
 * first appears inside a capture does not end the capture. */
void* uno_upload_table(const void* host, long long bytes);

/* Message of the last failing call on this thread ("" if none). */
const char* uno_last_error(void);

/* Bytes of scratch `ws` the 2-D forward / backward entry points need. */
long long uno_spectral_conv2d_fwd_ws_bytes(int B, int Ci, int Co, int m1, int m2);
long long uno_spectral_conv2d_bwd_ws_bytes(int B, int Ci, int Co, int m1, int m2);

/* SpectralConv2d_Uno.forward - reference integral_operators.py:181-207
 *   x  (B, Ci, H, W) f32;  w1, w2 (Ci, Co, m1, m2) c64;  y (B, Co, Ho, Wo) f32 [out]
 *   xtrunc (B, Ci, 2*m1, m2) c64 [out] - the truncated rfft2(x, norm="forward"), the only
 *   tensor backward needs besides the weights.  ws: scratch of ..._fwd_ws_bytes. */
int uno_spectral_conv2d_forward(const float* x, const float* w1, const float* w2, float* y,
                                float* xtrunc, void* ws, int B, int Ci, int Co, int H, int W,
                                int Ho, int Wo, int m1, int m2, void* stream);

/* Autograd adjoint of the above (PyTorch's FftC2R/Bmm/CopySlices/FftR2C backward chain,
 * SURVEY.md section 3.3 / Appendix A.2).  Complex gradients follow PyTorch's convention
 * dL/dRe + i dL/dIm.  gx / (gw1, gw2) may be NULL to skip that gradient.
 *   gy (B, Co, Ho, Wo) f32;  xtrunc as saved by forward;  gx (B, Ci, H, W) f32 [out]
 *   gw1, gw2 (Ci, Co, m1, m2) c64 [out] */
int uno_spectral_conv2d_backward(const float* gy, const float* xtrunc, const float* w1,
                                 const float* w2, float* gx, float* gw1, float* gw2, void* ws,
                                 int B, int Ci, int Co, int H, int W, int Ho, int Wo, int m1,
                                 int m2, void* stream);

/* Mixed-precision form of the two entry points above (BASELINE.json config 5: bf16 activations, f32 accumulation; the
 * reference itself raises on bf16 input, so this is an opt-in extension of integral_operators.py:181-207, not a replacement):
 * x / y and gy / gx are bfloat16 (same shapes, contiguous), read and written as such by the pruned DFT kernels (8-byte
 * loads / stores of four values, << 16 on load, round-to-nearest-even on store); weights, the truncated spectrum, every
 * accumulation and the weight gradients stay f32 / c64.  Half-precision weight STORAGE is the caller's cast. */
int uno_spectral_conv2d_forward_bf16(const void* x, const float* w1, const float* w2, void* y,
                                     float* xtrunc, void* ws, int B, int Ci, int Co, int H, int W,
                                     int Ho, int Wo, int m1, int m2, void* stream);
int uno_spectral_conv2d_backward_bf16(const void* gy, const float* xtrunc, const float* w1,
                                      const float* w2, void* gx, float* gw1, float* gw2, void* ws,
                                      int B, int Ci, int Co, int H, int W, int Ho, int Wo, int m1,
                                      int m2, void* stream);

/* The FFT crop / resample of pointwise_op_3D (reference integral_operators.py:448-463: unnormalised rfftn, four corners of
 * half the OUTPUT size copied into an INPUT-sized zero spectrum, irfftn(s = output size)) as a pruned DFT - pruned inverse DFT
 * pair with explicit frequency tables: along a complex axis the reference keeps spectrum indices r_j and reads index r_j as
 * frequency r_j of the output-length transform (irfftn trims / zero-pads at the END of the axis - bug-compatible, including
 * the misplaced negative frequencies when sizes differ).
 *   x (n_vol, D1, D2, D3) f32 -> y (n_vol, M1, M2, M3) f32;  f1_in / f1_out (J1 ints, device), f2_in / f2_out (J2 ints, device):
 *   forward / inverse frequency of kept row j along axes 1 / 2 (J1, J2 even; J1 <= 80, J2 <= 48); m3 kept half-spectrum bins;
 *   herm_in / herm_out: Hermitian column weights on the forward / inverse side (0 / 1 for the operator, 1 / 0 for its adjoint,
 *   which is the same call with sizes and tables swapped).  Planes of 16 ... 1792 (in) / 2048 (out) elements, D3, M3 <= 64. */
long long uno_fft_resample3d_ws_bytes(int n_vol, int D1, int M1, int J1, int J2, int m3);
int uno_fft_resample3d(const float* x, float* y, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                       int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3,
                       float scale, int herm_in, int herm_out, void* stream);

/* The same, ACCUMULATING into y (y += resampled x) and, with y_act != NULL, writing y_act = gelu(y) in the same pass (ABI 7): the
 * point-wise branch of OperatorBlock_3D (reference integral_operators.py:506-512: x1_out + x2_out, then F.gelu) lands in the buffer
 * the spectral branch wrote - neither the sum nor the activation is a separate pass. */
int uno_fft_resample3d_acc(const float* x, float* y, float* y_act, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                           int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3,
                           float scale, int herm_in, int herm_out, void* stream);

/* ABI 13.  The same operator as uno_fft_resample3d (same tables, same Hermitian-weight contract, the adjoint again the same call with
 * sizes and tables swapped) on kernels without its shape limits: any J1, J2 in 1 ... 128 (odd counts included), any
 * 1 <= m3 <= D3/2 + 1 (and <= M3/2 + 1), every axis length of x and y in 2 ... 128 - planes of up to 128 x 128 elements.  Outside that
 * range the call returns an error that names the limits; table entries are reduced modulo the axis length.  This is what the last two
 * layers of the reference's Uno3D_T40 need (navier_stokes_uno3d.py:145-159: (32,32,31) -> (48,48,41) -> (64,64,52) at S = 64, pad 3).
 * Plain f32 FMA kernels, f32 accumulation, results independent of the launch geometry.
 *   ws: uno_fft_resample3d_any_ws_bytes = 8 n_vol (D1 + M1) J2 m3 bytes. */
long long uno_fft_resample3d_any_ws_bytes(int n_vol, int D1, int M1, int J1, int J2, int m3);
int uno_fft_resample3d_any(const float* x, float* y, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                           int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3,
                           float scale, int herm_in, int herm_out, void* stream);

/* ABI 14.  uno_fft_resample3d_any ACCUMULATING into y (y += resampled x) and, with y_act != NULL, writing y_act = gelu(y) in the same
 * pass: what uno_fft_resample3d_acc is to uno_fft_resample3d, for the point-wise branch of an OperatorBlock_3D (reference
 * integral_operators.py:506-512: x1_out + x2_out, then F.gelu) on a grid outside the pruned-DFT range.  Same validation, limits and
 * workspace (uno_fft_resample3d_any_ws_bytes) as uno_fft_resample3d_any; the transform's summation order is that of the plain call, so
 * y holds exactly (old y) + (the plain call's result) in one float32 addition.  y_act == NULL: accumulate only.  y_act == y, x == y and
 * x == y_act are refused (negative code, the message names the argument). */
int uno_fft_resample3d_any_acc(const float* x, float* y, float* y_act, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                               int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3,
                               float scale, int herm_in, int herm_out, void* stream);

/* The same operator once more (no ABI change: new entry points only), for the grids of the reference's 256 x 256 NS-3D models
 * (Uno3D_T20_256 / Uno3D_T10_256, navier_stokes_uno3d.py:993-1181 / :1184-1372: conv0 resamples (256,256,T) -> (64,64,T), conv8
 * (64,64,T) -> (256,256,T); the operator itself is integral_operators.py:448-463, quirks kept).  The two leading (complex) axes of x and y
 * in 2 ... 256, the last (real) axis in 2 ... 64, any J1, J2 in 1 ... 256, any 1 <= m3 <= D3/2 + 1 (and <= M3/2 + 1).  Tables, Hermitian
 * weights, adjoint convention, workspace size and the _acc form (y += result; y_act = gelu(y) when y_act != NULL; y_act == y, x == y and
 * x == y_act refused) are those of uno_fft_resample3d_any / _any_acc.  The sums along the two complex axes run on v_mfma_f32_16x16x4_f32
 * (exact f32, fixed order: two runs are bit-identical); plane and volume offsets are 64-bit.  Outside the range the call returns an error
 * that names the limits; a combination inside it whose kernels would need more than 160 KB of LDS (modes3 = 33 with J2 + M2 > 500) is
 * refused with -2 before any launch. */
long long uno_fft_resample3d_wide_ws_bytes(int n_vol, int D1, int M1, int J1, int J2, int m3);
int uno_fft_resample3d_wide(const float* x, float* y, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                            int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3,
                            float scale, int herm_in, int herm_out, void* stream);
int uno_fft_resample3d_wide_acc(const float* x, float* y, float* y_act, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                                int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3,
                                float scale, int herm_in, int herm_out, void* stream);

/* SpectralConv3d_Uno.forward - reference integral_operators.py:385-427
 *   x (B, Ci, H, W, T) f32;  w[0..3] = weights1..4 (Ci, Co, m1, m2, m3) c64 in the reference's corner
 *   order (lo,lo), (hi,lo), (lo,hi), (hi,hi);  y (B, Co, Ho, Wo, To) f32 [out]
 *   xtrunc (B, Ci, 4, m1, m2, m3) c64 [out]: truncated rfftn(x, norm="forward"), corner-major. */
long long uno_spectral_conv3d_fwd_ws_bytes(int B, int Ci, int Co, int H, int Ho, int m1, int m2, int m3);
long long uno_spectral_conv3d_bwd_ws_bytes(int B, int Ci, int Co, int H, int Ho, int m1, int m2, int m3);
int uno_spectral_conv3d_forward(const float* x, const float* const* w, float* y, float* xtrunc, void* ws,
                                int B, int Ci, int Co, int H, int W, int T, int Ho, int Wo, int To,
                                int m1, int m2, int m3, void* stream);
/* Adjoint; gx or gw (array of 4 output pointers) may be NULL to skip that gradient. */
int uno_spectral_conv3d_backward(const float* gy, const float* xtrunc, const float* const* w, float* gx,
                                 float* const* gw, void* ws, int B, int Ci, int Co, int H, int W, int T,
                                 int Ho, int Wo, int To, int m1, int m2, int m3, void* stream);

/* The two 3-D transforms of the calls above as stages of their own (no ABI change: new entry points only).
 *   forward: volumes x (n_vol, D1, D2, D3) f32 -> corner-major truncated spectra (.., 4, m1, m2, m3) c64, times `scale`;
 *            adjoint = 1: the Hermitian-weighted, masked form the backward pass applies to the output gradient.
 *   inverse: spectra -> volumes y (n_vol, D1, D2, D3) f32, times `scale`; weighted = 1: Hermitian weights and later-wins masks
 *            (the forward pass's irfftn).
 * Placement on the SPECTRUM side, the convention of uno_dft2d_forward_grouped: volume i of a (B, group) batch <-> spectrum volume
 * (i / group) * stride + offset + i % group of a (B, stride, 4, m1, m2, m3) tensor - each source of a channel concatenation is
 * transformed into (read from) its channel range of one spectrum tensor.  group = stride = offset = 0: plain (spectrum volume i).
 * Grouped calls need group >= 1, offset >= 0, offset + group <= stride and n_vol % group == 0.  The volume side is always dense.
 * Per call the library takes the one-workgroup-per-volume kernels or the plane-by-plane path, as inside the layer; the latter uses
 * ws, uno_dft3d_ws_bytes(n_vol, D1, m2, m3) = 8 * n_vol * D1 * 2 m2 * m3 bytes (always required).  Arguments are checked on the
 * host before any launch (negative return, uno_last_error names the argument); n_vol == 0 succeeds without touching the device. */
long long uno_dft3d_ws_bytes(int n_vol, int D1, int m2, int m3);
int uno_dft3d_forward_grouped(const float* x, float* spec, void* ws, int n_vol, int D1, int D2, int D3, int m1, int m2, int m3,
                              float scale, int adjoint, int group, int stride, int offset, void* stream);
int uno_dft3d_inverse_grouped(const float* spec, float* y, void* ws, int n_vol, int D1, int D2, int D3, int m1, int m2, int m3,
                              float scale, int weighted, int group, int stride, int offset, void* stream);

/* uno_spectral_conv3d_forward / _backward on the channel concatenation of two tensors, which is never built (a skip connection):
 *   x1 (B, C1, H, W, T), x2 (B, Ci - C1, H, W, T), 0 < C1 < Ci;  gx1 / gx2 [out] of the same shapes, distinct buffers.
 * w, y, xtrunc (B, Ci, 4, m1, m2, m3), gw and both workspace sizes are those of the one-source calls; each source is transformed
 * into (its gradient out of) its channel range of the one spectrum tensor, everything else is unchanged.  The choice between the
 * transform kernel families is made for the concatenation's volume count, so each source runs the kernels the one-source call on
 * the concatenation runs and the results are those of that call, bit for bit.  x2 == NULL / gx2 == NULL:
 * the one-source call on x1 / gx1 (C1 ignored).  With gx2 given gx1 is required.  All launches go on `stream`. */
int uno_spectral_conv3d_forward2(const float* x1, const float* x2, int C1, const float* const* w, float* y, float* xtrunc, void* ws,
                                 int B, int Ci, int Co, int H, int W, int T, int Ho, int Wo, int To, int m1, int m2, int m3,
                                 void* stream);
int uno_spectral_conv3d_backward2(const float* gy, const float* xtrunc, const float* const* w, float* gx1, float* gx2, int C1,
                                  float* const* gw, void* ws, int B, int Ci, int Co, int H, int W, int T, int Ho, int Wo, int To,
                                  int m1, int m2, int m3, void* stream);

/* Pruned complex DFT along the leading axis of a 3-D transform:
 *   inverse = 0: planes (n_img, H, 2*m2*m3) c64 -> corner-major spectrum (n_img, 4, m1, m2, m3) c64
 *   inverse = 1: the reverse direction (e^{+i...}); mask_overlap applies on the spectrum side. */
int uno_cdft_axis(const float* in, float* out, int inverse, int n_img, int H, int m1, int m2, int m3,
                  float scale, int mask_overlap, void* stream);

/* Stage-level entry points (the three kernels the two calls above are built from). */

/* Pruned forward DFT: spec[img][j][l] = scale * c_l * keep_j * sum x e^{-2 pi i (K_j h/H + l w/W)}
 *   images (n_img, H, W) f32 -> spec (n_img, 2*m1, m2) c64.
 *   hermitian_cols: multiply column l by 1 (l = 0, Nyquist) or 2 - used for gO in backward.
 *   mask_overlap:   zero lo-corner rows j >= H - m1 (later slice-assignment wins). */
int uno_dft2d_forward(const float* images, float* spec, int n_img, int H, int W, int m1, int m2,
                      float scale, int hermitian_cols, int mask_overlap, void* stream);

/* Pruned inverse DFT: images[h][w] = Re sum_{j,l} scale * c_l * keep_j * spec[j][l] e^{+2 pi i (...)}. */
int uno_dft2d_inverse(const float* spec, float* images, int n_img, int H, int W, int m1, int m2,
                      float scale, int hermitian_cols, int mask_overlap, void* stream);

/* ABI 11.  Data parallelism (reference train loops are single-process; BASELINE.json north_star: RCCL all-reduce beside the backward
 * pass): set aside `n` compute units for concurrently running communication kernels.  Launch geometries that size themselves to the
 * device ("one workgroup per CU", persistent grids) then count on the remaining CUs.  Returns the previous value; 0 = none (default). */
int uno_reserve_cus(int n);

/* ABI 11.  (no reference counterpart) Alternating sweep direction: consecutive launches of the streaming kernels walk their work items
 * (images, batch entries, pixel tiles) in opposite directions, so that a kernel starts with the part of a > 256 MB tensor its predecessor
 * touched last - the part the Infinity Cache still holds.  Results do not depend on it.  enable = 0 turns it off (every launch front to
 * back); returns the previous setting (default 255 = every family; 1 is stored as 255).  Other values 0 .. 255 are a mask of kernel families
 * (development).  A value with bit 8 set (256 | mask) PINS the direction: every launch of a masked family runs reversed and the per-thread
 * launch counter is neither read nor advanced (the masked-off families run front to back); for tests, which can then run one launch both
 * ways - backward launches included, whose counter belongs to another thread.  The value returned then is that 256 | mask.  A negative
 * value never pins: its low eight bits are the mask, as before. */
int uno_sweep_alternation(int enable);

/* ABI 11.  Pruned inverse DFT PLUS the up-sampled point-wise branch in one pass over the output:
 *   images[h][w] = (uno_dft2d_inverse's result) + sum_{u,v} Rh[h][u] Rw[w][v] addend[u][v]
 * = `x1_out + x2_out` of an up-sampling operator block, reference integral_operators.py:272-273, with x2_out the bicubic /
 * align_corners / antialias interpolation (:240-242) of the LOW-resolution 1x1-convolution result `addend` (n_img, Hs, Ws) - the
 * convolution and the interpolation commute - and, with the transposed operators, the input gradient of a down-sampling block.
 * Rh (H x Hs) and Rw (W x Ws) are banded (<= 12 source rows per 16 output rows, <= 12 source columns per 16 output columns:
 * up-sampling by two or more) and given as operand tables the caller builds once per size pair (uno_amd/resample.py
 * upsample_add_tables):
 *   tile_p0 [ceil(H/16)]           first source row of each 16-row output tile
 *   row_op  [ceil(H/16)][3][64]    entry (tile, e, lane) = Rh[16 tile + lane % 16][tile_p0 + 3 (lane / 16) + e]
 *   col_v0  [nwt][2]               first source column of (column tile, side), nwt = ((W/2) + 16) / 16; <= Ws - 12
 *   col_op  [nwt][2][3][64]        entry (wt, side, ks, lane) = Rw[w][col_v0 + 3 (lane / 16) + ks], w = 16 wt + lane % 16 (side 0)
 *                                  or W - 16 wt - lane % 16 (side 1); zero for w outside [0, W)
 * uno_dft2d_inverse_add_applies: 1 where the fused kernel exists (float32, rows of 192..223 or 416..447 elements whose 16-row
 * tiles fit the LDS, modes1 <= 27, modes2 <= 24), else 0 - the caller then runs uno_dft2d_inverse followed by uno_resample2d. */
int uno_dft2d_inverse_add_applies(int n_img, int H, int W, int m1, int m2, int Hs, int Ws);
int uno_dft2d_inverse_add(const float* spec, float* images, int n_img, int H, int W, int m1, int m2, float scale, int hermitian_cols,
                          int mask_overlap, const float* addend, int Hs, int Ws, const int* tile_p0, const float* row_op,
                          const int* col_v0, const float* col_op, void* stream);

/* (added under ABI 14: new entry points only, nothing existing changes)  Pruned forward DFT PLUS the down-sampled image from one read of the images:
 *   spec as uno_dft2d_forward_grouped writes it (group <= 0: the plain layout), and
 *   resampled[i][j] = sum_{h,w} A[i][h] B[j][w] images[h][w]      (n_img, Ho, Wo) f32
 * = the truncated input spectrum and the bicubic / align_corners / antialias interpolation (reference integral_operators.py:240-242) of
 * a down-sampling operator block's input, which uno_resample2d followed by uno_dft2d_forward read twice - and, with the transposed
 * operators, the gradient spectrum and the point-wise gradient of an up-sampling block.  B (Wo x W) is uno_resample2d's band table of
 * the columns: col_start [Wo] first source column, col_wt [Wo][KW] taps (zero past the row's end).  A (Ho x H) is given per 16-row
 * tile of the IMAGE (the kernel carries the output rows a tile contributes to in registers, 13 at most; uno_amd/resample.py
 * fused_resample_tables builds the tables once per size pair):
 *   row_tiles [ceil(H/16)][4]       first carried output row i0, output rows complete after this tile (stored, then dropped from the
 *                                   carried set), bits 0..31 and 32..51 of the mask whose bit 4 c + q is set where
 *                                   row_op[tile][c][4 q .. 4 q + 3] holds a non-zero weight
 *   row_op    [ceil(H/16)][13][16]  entry (tile, c, r) = A[i0 + c][16 tile + r], zero outside the matrix
 * uno_dft2d_forward_resample_applies: 1 where the fused kernel exists (float32; rows of 416..447 elements with Wo <= 256, or rows of
 * 192..223 elements with Wo <= 128; KW <= 9, (modes1, modes2) in 17..24 x 17..20 or 1..8 x 1..8, the tiles fit the LDS), else 0 - the
 * caller then runs the two calls. */
int uno_dft2d_forward_resample_applies(int n_img, int H, int W, int m1, int m2, int Ho, int Wo, int KW);
int uno_dft2d_forward_resample(const float* images, float* spec, int n_img, int H, int W, int m1, int m2, float scale, int hermitian_cols,
                               int mask_overlap, int group, int stride, int offset, float* resampled, int Ho, int Wo, const int* col_start,
                               const float* col_wt, int KW, const int* row_tiles, const float* row_op, void* stream);

/* (added under ABI 14: a new entry point only)  The truncation to (m1, m2) modes of spectra truncated to (M1, M2) modes, m1 <= M1 and
 * m2 <= M2: dst rows 0 .. m1 - 1 = src rows 0 .. m1 - 1 (lo corner), dst rows m1 .. 2 m1 - 1 = the LAST m1 rows of src (hi corner),
 * columns 0 .. m2 - 1.  A tensor that two spectral layers transform on one grid with the same scale and flags (reference
 * darcy_flow_uno2d.py:110 and :121 both take x_c0) is transformed once at the larger mode counts; the other layer's spectrum is this
 * copy.  src (.., 2 M1, M2) and dst (.., 2 m1, m2) c64 in uno_dft2d_forward_grouped's layout each (group <= 0: plain); dst != src. */
int uno_spectrum_crop(const float* src, float* dst, int n_img, int M1, int M2, int m1, int m2, int src_group, int src_stride, int src_offset,
                      int dst_group, int dst_stride, int dst_offset, void* stream);

/* The two transforms with bfloat16 images (the stages of uno_spectral_conv2d_*_bf16); spectra are c64 as above. */
int uno_dft2d_forward_bf16(const void* images, float* spec, int n_img, int H, int W, int m1, int m2,
                           float scale, int hermitian_cols, int mask_overlap, void* stream);
int uno_dft2d_inverse_bf16(const float* spec, void* images, int n_img, int H, int W, int m1, int m2,
                           float scale, int hermitian_cols, int mask_overlap, void* stream);

/* The same transforms with the spectra of a (B, group) batch of images placed at channels [offset, offset + group) of a
 * (B, stride, 2*m1, m2) spectrum tensor (image i <-> spectrum (i / group) * stride + offset + i % group): lets an
 * operator block consume torch.cat([x1, x2], dim=1) (reference darcy_flow_uno2d.py:117-125) from its two sources. */
int uno_dft2d_forward_grouped(const float* images, float* spec, int n_img, int H, int W, int m1, int m2, float scale,
                              int hermitian_cols, int mask_overlap, int group, int stride, int offset, void* stream);
int uno_dft2d_inverse_grouped(const float* spec, float* images, int n_img, int H, int W, int m1, int m2, float scale,
                              int hermitian_cols, int mask_overlap, int group, int stride, int offset, void* stream);

/* Per-mode channel mixing on the truncated spectrum, `ncorner` weight tensors of
 * `modes_per_corner` modes each (2-D: ncorner = 2, modes_per_corner = m1*m2).
 *   op 0: out[b,o] = sum_i in[b,i] * w[i,o]        (einsum "bixy,ioxy->boxy", :178-179)
 *   op 1: out[b,i] = sum_o in[b,o] * conj(w[i,o])  (grad wrt the input spectrum)
 *   in (B, Cin, ncorner*modes) c64, w[c] (Ci, Co, modes) c64, out (B, Cout, ncorner*modes) c64 */
int uno_mode_mix(const float* in, const float* const* w, float* out, int op, int B, int Ci, int Co,
                 int ncorner, int modes_per_corner, void* stream);

/* gw[c][i,o] = sum_b conj(xtrunc[b,i]) * go[b,o] per mode. */
int uno_mode_wgrad(const float* xtrunc, const float* go, float* const* gw, int B, int Ci, int Co,
                   int ncorner, int modes_per_corner, void* stream);
/* ABI 11.  Both per-mode GEMMs of a backward pass - the autograd adjoints of the einsum at reference integral_operators.py:178-179 /
 * :382-383 - from one launch where the kernels allow (else two): gx_spec[b,i] = sum_o go[b,o] conj(w[i,o]) and
 * gw[i,o] (+)= sum_b conj(xtrunc[b,i]) go[b,o]; `accumulate` adds into gw. */
int uno_mode_backward(const float* xtrunc, const float* go, const float* const* w, float* gx_spec, float* const* gw, int B, int Ci,
                      int Co, int ncorner, int modes_per_corner, int accumulate, void* stream);
/* uno_mode_wgrad with accumulate != 0: gw[c] += (in-place accumulation into a parameter's gradient buffer). */
int uno_mode_wgrad_acc(const float* xtrunc, const float* go, float* const* gw, int B, int Ci, int Co, int ncorner,
                       int modes_per_corner, int accumulate, void* stream);
/* Launch-plan queries (additive: added WITHOUT an ABI bump, UNO_SPECTRAL_ABI_VERSION stays 14).  Host only: no device call, no
 * buffers.  They run the size checks and the launch decision of the calls above - the library has ONE decision function, which the
 * launchers use too - and write it to `plan`; a call with these sizes launches exactly that.  Errors: the real call's codes and
 * uno_last_error text (bad sizes: -1; an operand spanning 2 GiB or more per corner: -2, "... spans ..."), and -1 for a null `plan`
 * or an op outside 0 ... 2.
 *   uno_mode_gemm_plan: the GEMM of uno_mode_mix (op 0 / 1; w_half != 0: uno_mode_mix_f16w) or of uno_mode_wgrad(_acc) (op 2; `accumulate`
 *   is ignored for op 0 / 1, `w_half` for op 2).  plan: UNO_MODE_GEMM_PLAN_INTS ints
 *     [0]  family: 0 nothing to launch (B = 0), 1 LDS-staged uno::mode_gemm_kernel<qc, pipe, half, acc>,
 *                  2 4x4x1 uno::mode_gemm_blocks_kernel<variant, half, acc>
 *     [1..3]  the GEMM's M, N, K (op 0: B, Co, Ci; op 1: B, Ci, Co; op 2: Ci, Co, B)
 *     [4]  qc: modes per workgroup, 16 or 8 (family 1, else 0)        [5]  pipe: pipelined K loop (family 1, else 0)
 *     [6]  variant: 0 <4, 4, 2>, 1 <4, 2, 4>, 2 <2, 4, 4> (family 2, else -1)
 *     [7]  KS: waves that share a K range, 1 / 2 / 4 (family 2, else 0)  [8]  adjacent: the kernel's adjacent_modes (family 2, else 0)
 *     [9]  why the 4x4x1 form was not taken: bit 0 padded (more than 20 % idle mode blocks), bit 1 huge_out (K <= 32 and an output
 *          above 200 MB); 0 in family 2
 *     [10] half, [11] acc: the kernel's last two template flags (acc is 0 with half-precision weights)
 *     [12..14] grid x, y, z       [15] dynamic LDS bytes
 *   uno_mode_backward_plan: uno_mode_backward.  plan: UNO_MODE_BACKWARD_PLAN_INTS ints
 *     [0]  paired: 1 = one launch of uno::mode_gemm_blocks_pair_kernel<variant of role a, acc of role b>, 0 = role b's launch, then role a's
 *     [1]  Ga: workgroups [0, Ga) of the pair launch run role a        [2] the pair launch's grid      [3] its dynamic LDS bytes
 *     [4..19]  role a, the input gradient (op 1), [20..35] role b, the weight gradient (op 2): each as uno_mode_gemm_plan reports it */
#define UNO_MODE_GEMM_PLAN_INTS 16
#define UNO_MODE_BACKWARD_PLAN_INTS 36
int uno_mode_gemm_plan(int op, int B, int Ci, int Co, int ncorner, int modes_per_corner, int w_half, int accumulate, int* plan);
int uno_mode_backward_plan(int B, int Ci, int Co, int ncorner, int modes_per_corner, int accumulate, int* plan);
/* uno_spectral_conv2d_backward in all three storage formats (io_format 0: f32 images; 1: bf16 images; 2: bf16 images + fp16 (re, im)
 * weights) with accumulate_gw != 0: gw1 / gw2 += instead of =. */
int uno_spectral_conv2d_backward_acc(const void* gy, const float* xtrunc, const void* w1, const void* w2, void* gx,
                                     float* gw1, float* gw2, void* ws, int B, int Ci, int Co, int H, int W, int Ho, int Wo,
                                     int m1, int m2, int io_format, int accumulate_gw, void* stream);

/* Separable banded resampling out = A . in . B^T of n_img images (H, W) -> (Ho, Wo): the resampling half of
 * pointwise_op_2D (reference integral_operators.py:240-242, bicubic / align_corners / antialias) and, with the
 * transposed band tables, its adjoint.  Row i of A has its first nonzero at column startH[i] and KH weights
 * wtH[i*KH .. i*KH+KH-1] (zero padded); likewise B.  tmp: scratch of 4*n_img*min(Ho*W, H*Wo) bytes.
 * Optional dense row-tile form of A for the fused single-pass kernel (NULL / 0 to use the two-pass kernels):
 * tile k covers output rows 16k..16k+15, reads input rows tile_p0[k] .. tile_p0[k]+NP-1 and has weights
 * tile_w[(k*NP + u)*16 + r] = A[16k + r][tile_p0[k] + u].
 * accumulate != 0: out += A . in . B^T (the spectral and the point-wise branch of an operator block write one
 * buffer: reference integral_operators.py:273 `x1_out + x2_out`, and the sum of their input gradients). */
int uno_resample2d(const float* in, float* out, float* tmp, int n_img, int H, int W, int Ho, int Wo,
                   const int* startH, const float* wtH, int KH, const int* startW, const float* wtW, int KW,
                   const int* tile_p0, const float* tile_w, int NP, int accumulate, void* stream);

/* Channel mixing of a channels-first tensor, y[b][o][p] = sum_i Wm(o,i) x[b][i][p] (+ bias[o]): the 1x1
 * convolution of pointwise_op_2D / pointwise_op_3D (reference integral_operators.py:219, 439: nn.Conv2d/3d(in,
 * out, 1)) and the lift / projection nn.Linear layers of the U-NO models (navier_stokes_uno2d.py fc0/fc1/fc2)
 * applied without the channels-last permute.  x (B, Ci, P), y (B, Co, P), P = pixels per sample (contiguous).
 * transpose_w = 0: w is (Co, Ci) row-major; transpose_w = 1: w is (Ci, Co) row-major and Wm = w^T (this is
 * the input-gradient call: x := grad_y, Ci := forward Co).  bias may be NULL.  accumulate != 0: y += (as in
 * uno_resample2d).
 * Fused activation forms for a layer whose input tensor is kept PRE-activation (the model's `fc(F.gelu(t))` patterns,
 * reference darcy_flow_uno2d.py:98-101, 128-131): act_in != 0 applies the exact-erf GELU to x as it is read (y = Wm gelu(x)
 * + bias); dgelu_of != NULL (B, Co, P) multiplies the product by gelu'(dgelu_of) - the input-gradient call then returns the
 * gradient of the pre-activation tensor.  The two are mutually exclusive.  accumulate = 2 (with dgelu_of): y = (y + product) *
 * gelu'(dgelu_of) - the call that adds the LAST contribution to the gradient of a block's activation also applies the block's
 * GELU derivative to the completed sum (reference integral_operators.py:282-283 backward), no separate pass. */
int uno_channel_mix(const float* x, const float* w, const float* bias, float* y, int B, int Ci, int Co,
                    long long P, int transpose_w, int accumulate, int act_in, const float* dgelu_of, void* stream);

/* Weight / bias gradient of uno_channel_mix: gw[o][i] = sum_{b,p} gy[b][o][p] x[b][i][p], gb[o] = sum gy[b][o][p]
 * (gb may be NULL).  ws: scratch of uno_channel_wgrad_ws_bytes() bytes; partial sums are combined in a fixed
 * order (bit-reproducible run to run).  act_x != 0: x := gelu(x) as it is read (see uno_channel_mix). */
long long uno_channel_wgrad_ws_bytes(int B, int Ci, int Co, long long P);
int uno_channel_wgrad(const float* gy, const float* x, float* gw, float* gb, void* ws, int B, int Ci, int Co,
                      long long P, int act_x, void* stream);

/* uno_channel_mix / uno_channel_wgrad for a layer whose input is the channel concatenation of TWO tensors (the skip
 * connections of the U-NO models: reference darcy_flow_uno2d.py:117-127 `torch.cat([x_c4, x_c0], dim=1)` -> conv5,
 * `torch.cat([x_c5, x_fc0], dim=1)` -> fc1) without building the concatenation, one pass over every operand:
 *   x1 (B, C1, P) holds input channels [0, C1), x2 (B, Ci - C1, P) the rest (x2 = NULL: one source, C1 ignored);
 *   y1 (B, Co1, P) receives output channels [0, Co1), y2 (B, Co - Co1, P) the rest (y2 = NULL: one destination) - the
 *   transposed call on grad_y then yields the two input gradients of the layer from ONE read of grad_y;
 *   w is the layer's full (Co, Ci) weight (transpose_w = 1: (Ci, Co)), bias (Co) or NULL;
 *   act_in applies to x1 only, dgelu_of (B, Co1, P) to y1 only (the pre-activation source of the pair);
 *   y_act (B, Co, P) or NULL: additionally receives gelu(y) - the activation of a block without normalisation written by the
 *   kernel that completes the pre-activation sum (reference integral_operators.py:282-283), single destination only;
 *   proj_w (Co), proj_b (1) or NULL, proj_out (B, P): the call also writes proj_out[b][p] = proj_b + sum_o proj_w[o] gelu(y[b][o][p]),
 *   the one-channel projection `fc2(F.gelu(fc1(x)))` that ends the models (darcy_flow_uno2d.py:128-131) in the pass that produces
 *   y (which is still written: the backward of uno_gelu_project_forward needs it); Co <= 64, single destination.
 * Splits must be multiples of 16 (C1) / 64 (Co1; 128 when Co is a multiple of 128) channels; uno_channel_wgrad2 needs
 * C1 % 64 == 0 and P >= 64 (x2 = NULL: any shape).  gw is the full (Co, Ci) gradient; accumulate != 0: gw / gb += (the kernels
 * write a parameter's gradient buffer in place: the unrolled roll-out of ns_train_2d.py:46-68 sums 40 contributions per weight).
 * uno_channel_wgrad2 with accumulate = 3 runs the first stage only: the split-K partial sums stay in ws
 * (uno_channel_wgrad_ws_bytes() bytes = nparts blocks of (Co, Ci + 1) floats, bias sums in column Ci), gw / gb are not touched
 * (may be NULL); uno_channel_wgrad_finish() then sums `nparts` CONSECUTIVE blocks - the ws of one call, or of the T calls of a
 * roll-out laid out one after the other - into gw / gb (gb may be NULL) in the fixed order of the blocks: one second stage per
 * layer and training step instead of one per use. */
int uno_channel_mix2(const float* x1, const float* x2, int C1, const float* w, const float* bias, float* y1, float* y2, int Co1,
                     float* y_act, int B, int Ci, int Co, long long P, int transpose_w, int accumulate, int act_in,
                     const float* dgelu_of, const float* proj_w, const float* proj_b, float* proj_out, void* stream);
int uno_channel_wgrad2(const float* gy, const float* x1, const float* x2, int C1, float* gw, float* gb, void* ws, int B, int Ci,
                       int Co, long long P, int act_x, int accumulate, void* stream);
int uno_channel_wgrad_finish(const void* parts, float* gw, float* gb, int Ci, int Co, long long nparts, int accumulate, void* stream);

/* Final projection of the U-NO models fused with the GELU in front of it (reference darcy_flow_uno2d.py:128-131:
 * `x_fc1 = F.gelu(self.fc1(x)); x_out = self.fc2(x_fc1)` with fc2 = Linear(C, 1)), channels-first:
 *   out[b][p] = bias[0] + sum_c w[c] * gelu(pre[b][c][p])          pre (B, C, P), out (B, P), exact-erf GELU, bias may be NULL
 * backward: gpre = gelu'(pre) * w[c] * gout,  gw[c] = sum gout * gelu(pre),  gb[0] = sum gout  (gb may be NULL);
 * ws: scratch of uno_gelu_project_bwd_ws_bytes() bytes (fixed-order partial sums). */
int uno_gelu_project_forward(const float* pre, const float* w, const float* bias, float* out, int B, int C, long long P,
                             void* stream);
long long uno_gelu_project_bwd_ws_bytes(int B, int C, long long P);
int uno_gelu_project_backward(const float* pre, const float* w, const float* gout, float* gpre, float* gw, float* gb,
                              void* ws, int B, int C, long long P, void* stream);

/* The projection over TWO sources (additive: the ABI version stays 14, no existing entry point changes).  The reference's UNO_P and
 * UNO_S256 end in `x_fc1 = F.gelu(self.fc1(x_c6)); x_fc1 = torch.cat([x_fc1, x_fc], dim=3); x_out = self.fc2(x_fc1)`
 * (navier_stokes_uno2d.py:121-125, 320-324) with x_fc = gelu(fc(x)), the first lift activation, and fc2 = Linear(C1 + C2, 1):
 *   out[b][p] = bias[0] + sum_{c<C1} w[c] * gelu(pre[b][c][p]) + sum_{d<C2} w[C1+d] * f(s[b][d][p])
 * pre (B, C1, P), s (B, C2, P), w (C1 + C2), out (B, P); f = gelu when act2 = 1 (s is kept pre-activation), the identity when
 * act2 = 0; C1, C2 >= 1 and C1 + C2 <= 1024.  The concatenation is never built: each source is read once.
 * backward: gpre = gelu'(pre) * w[c] * gout,  gs = f'(s) * w[C1+d] * gout (gs may be NULL: not written),
 *   gw[e] = sum gout * (gelu(pre) | f(s)) for all C1 + C2 entries,  gb[0] = sum gout (gb may be NULL);
 * ws: scratch of uno_gelu_project2_bwd_ws_bytes() bytes (fixed-order partial sums: two calls give the same bits).  Float32, dense. */
int uno_gelu_project2_forward(const float* pre, const float* s, const float* w, const float* bias, float* out, int B, int C1, int C2,
                              long long P, int act2, void* stream);
long long uno_gelu_project2_bwd_ws_bytes(int B, int C1, int C2, long long P);
int uno_gelu_project2_backward(const float* pre, const float* s, const float* w, const float* gout, float* gpre, float* gs, float* gw,
                               float* gb, void* ws, int B, int C1, int C2, long long P, int act2, void* stream);

/* Per-time-step relative L2 error in one pass (additive: the ABI version stays 14).  The reference's NS-3D loop computes, for every
 * batch and under no_grad, `sum_t LpLoss(size_average=False)(out[..., t], y[..., t])` (ns_train_3d.py:55-62, 84-98) - the number it
 * prints and selects checkpoints by; its 2-D test loop (ns_train_2d.py:133-150) needs the same per step and for the whole trajectory.
 * pred, target: dense float32 (B, P, T), T innermost (the model's (B, S, S, T_f) output, P = S * S).  Written by the call:
 *   sums   (B, T, 2)   [b][t][0] = sum_p (pred - target)^2,  [b][t][1] = sum_p target^2
 *   rel    (B, T + 1)  [b][t] = sqrt(num) / sqrt(den) for t < T;  [b][T] = sqrt(sum_t num) / sqrt(sum_t den), the whole trajectory
 *   totals (2)         [0] = sum_b sum_{t<T} rel[b][t] (the reference's temp_step_loss);  [1] = sum_b rel[b][T]
 * 1 <= T <= 256, P >= 1, any B * P * T (64-bit offsets); B == 0 returns 0 without touching the device.  No clamping: a zero target
 * slice gives +inf (NaN for 0 / 0) as torch.norm(.) / torch.norm(.) does.  Two launches, no atomics; the chunk decomposition is a
 * function of (P, T) alone (not of the CU count or uno_reserve_cus), so two calls give the same bits.
 * ws: scratch of uno_rel_l2_steps_ws_bytes() bytes (never shrinks as P grows).  Forward only: the training loss is not this call. */
long long uno_rel_l2_steps_ws_bytes(int B, long long P, int T);
int uno_rel_l2_steps(const float* pred, const float* target, float* sums, float* rel, float* totals, void* ws, int B, long long P, int T,
                     void* stream);

/* The gradient of the two totals of uno_rel_l2_steps at pred, one launch (additive: the ABI version stays 14) - the NS-3D training
 * step takes its loss (totals[1]) and its per-step metric (totals[0]) from ONE forward pass over (out, y) with it.
 * pred, target: the forward call's inputs; sums (B, T, 2): as the forward call wrote it; g_full, g_step: the upstream gradients of
 * totals[1] and totals[0], one float32 each ON THE DEVICE (never read by the host), either may be NULL (= 0); gx (B, P, T): written,
 *   gx[b][p][t] = (pred - target)[b][p][t] * (cf[b] + cs[b][t])
 *   cf[b]       = g_full / (sqrt(sum_t num) * sqrt(sum_t den)),   cs[b][t] = g_step / (sqrt(num[b][t]) * sqrt(den[b][t]))
 * with (num, den) = sums[b][t] and the whole-trajectory sums formed as the forward call's finish launch forms them.  A coefficient
 * whose num is 0 is 0 (the backward of torch.linalg.vector_norm, uno_rel_l2_backward's rule); den is not clamped.  No gradient for target.
 * Limits as the forward call: 1 <= T <= 256, P >= 1, 64-bit offsets, B == 0 returns 0 without touching the device.  No atomics; the
 * launch is sized by the device's compute units less uno_reserve_cus, and every element is one product, so the result does not depend
 * on that size.  16-byte loads and stores where T % 4 == 0 and pred, target and gx are 16-byte aligned, 4-byte ones otherwise. */
int uno_rel_l2_steps_backward(const float* pred, const float* target, const float* sums, const float* g_full, const float* g_step, float* gx,
                              int B, long long P, int T, void* stream);

/* The relative L2 TRAINING loss and its gradient (additive: the ABI version stays 14).  The reference's three training loops call
 * `LpLoss(size_average=False)(x.view(B, -1), y.view(B, -1))` (utilities3.py:86-100; train_darcy.py:53, ns_train_2d.py:55,
 * ns_train_3d.py:58-64) - about six small launches forward and eight backward as stock ops, 40 times per NS-2D roll-out.
 * x, y: float32 seen as (B, N); element [b][e] of x lies x_row * b + x_elem * e ELEMENTS from x (likewise y): a time slice
 * `out[..., t].view(B, -1)` is x_elem = T_f.  Strides are >= 0 (0: a broadcast operand).
 * uno_rel_l2_forward - two launches (partial sums over (chunk, row), then one workgroup), written by the call:
 *   sums  (B, 2)  [b][0] = sum_e (x - y)^2,  [b][1] = sum_e y^2
 *   ratio (B)     sqrt(sums[b][0]) / sqrt(sums[b][1])
 *   total (1)     sum_b ratio[b]
 * uno_rel_l2_backward - one launch: gx (B, N) dense, gx[b][e] = g[b] * scale * (x - y)[b][e] / (sqrt(num_b) * sqrt(den_b)) with
 *   (num_b, den_b) = sums[b] of the forward call; g lives on the device - B values (g_per_row = 1) or one (g_per_row = 0) - and is never
 *   read by the host.  Where num_b == 0 the row's gradient is 0 (the backward of torch.linalg.vector_norm).  No gradient for y.
 * No clamping: a zero target row gives ratio = +inf (NaN for 0 / 0) as torch.norm(.) / torch.norm(.) does.
 * B >= 0, N >= 1, any B * N (64-bit offsets); B == 0 returns 0 without touching the device.  No atomics; the chunk decomposition is a
 * function of N alone (4096 elements per chunk, at most 64 chunks; not of the CU count or uno_reserve_cus) and chunk partials are
 * summed in double in ascending order and rounded once: two calls, a call under uno_reserve_cus and a graph replay give the same bits.
 * 16-byte loads where both element strides are 1 and every row of x and y starts 16-byte aligned, 4-byte loads otherwise.
 * ws: scratch of uno_rel_l2_ws_bytes() = 8 * B * chunks(N) bytes (0 for bad sizes; never shrinks as N grows). */
long long uno_rel_l2_ws_bytes(int B, long long N);
int uno_rel_l2_forward(const float* x, long long x_row, long long x_elem, const float* y, long long y_row, long long y_elem, float* sums,
                       float* ratio, float* total, void* ws, int B, long long N, void* stream);
int uno_rel_l2_backward(const float* x, long long x_row, long long x_elem, const float* y, long long y_row, long long y_elem,
                        const float* sums, const float* g, int g_per_row, float scale, float* gx, int B, long long N, void* stream);

/* K24 (additive: the ABI version stays 14; no reference counterpart): the shell-binned energy spectrum of real frames, the figure a
 * turbulence surrogate is judged by next to its relative L2 error.  For a frame u of H x W samples: U = fft2(u) / (H W) with integer
 * wavenumbers in fftfreq order, shell s(ky, kx) = round(hypot(ky, kx)) decided in integers ((2k - 1)^2 <= 4 (ky^2 + kx^2) < (2k + 1)^2),
 * K = round(hypot(H / 2, W / 2)) + 1 shells (integer halves), E(k) = sum over BOTH Hermitian halves of |U|^2 on shell k: sum_k E(k) = mean(u^2).
 * x: float32, B * T frames; sample b, frame t, row h, column w lies x_batch * b + x_frame * t + x_row * h + x_elem * w ELEMENTS from x:
 *   (B, S, S, T) time-innermost is (S S T, 1, S T, T), (B, T, S, S) is (T S S, S S, S, 1), a [::r, ::r] view multiplies row and element
 *   strides by r.  Strides are >= 0; nothing is copied.  y: an optional target (NULL: none) with strides of its own.
 * spec, written dense: (B, T, 1, K) without y; (B, T, 3, K) = [E_x, E_y, E_{x - y}] with y - two transforms per frame pair, the third
 *   spectrum from the difference of the two in registers, so sum_k E_{x-y} / sum_k E_y = (relative L2 error)^2.
 * Two launches: one workgroup per (frame, band of 16 half-spectrum columns) - both DFT axes as dense sums on the f32 MFMA, |.|^2 with the
 * Hermitian weight (2 for 0 < kx < W / 2, else 1), each shell's modes of the band added by one thread in a fixed order - then the bands
 * added in ascending order.  The complex spectrum is never written to memory.  No atomics; the decomposition is a function of (H, W)
 * and of whether y is given, not of B, the CU count or uno_reserve_cus: two calls, a call under uno_reserve_cus and a graph replay give
 * the same bits, and a sample's spectrum does not depend on its batch.  No synchronisation, allocation or read-back; twiddle tables
 * and the sorted shell lists are built on the host (float64 / integers) once per (device, H, W) and uploaded as uno_upload_table does
 * (safe under graph capture).  8 <= H, W <= 512 (odd sizes included), T >= 1, B >= 0, B * T * ceil((W / 2 + 1) / 16) < 2^31; 64-bit
 * offsets; B == 0 returns 0 without touching the device.  ws: scratch of uno_shell_spectrum_ws_bytes() bytes (0 for bad sizes), need
 * not be initialised.  Errors (-1, before any launch): null x / spec / ws, sizes out of range, a negative stride. */
long long uno_shell_spectrum_ws_bytes(int B, int T, int H, int W, int with_target);
int uno_shell_spectrum(const float* x, long long x_batch, long long x_frame, long long x_row, long long x_elem, const float* y,
                       long long y_batch, long long y_frame, long long y_row, long long y_elem, float* spec, void* ws, int B, int T, int H,
                       int W, void* stream);

/* The relative Sobolev (H^s) loss of real frames and its gradient (K25, sobolev_loss.hip; additive: the ABI version stays 14).  With
 * X = fft2(x) / (H W), integer wavenumbers in fftfreq order and a weight table w2 (H / 2 + 1, W / 2 + 1), float32 on the device, read at
 * (|ky|, |kx|):
 *   sums (B, T, 2) = [ sum_k w2 |X - Y|^2, sum_k w2 |Y|^2 ] over both Hermitian halves, per frame;
 *   per_frame = 1: ratio (B, T) = sqrt(num) / sqrt(den);  per_frame = 0: ratio (B) from the sums over a sample's frames;
 *   total (1) = sum of ratio.
 * x, y: float32 frames addressed as uno_shell_spectrum's, four element strides >= 0 each; nothing is copied.  z: NULL, or a buffer of
 * B * T * H * (W / 2 + 1) complex64 that receives Z = w2 (X - Y) per frame for the backward call; with NULL no spectrum leaves the
 * compute unit.  Two launches: one workgroup per (frame, band of 16 half-spectrum columns), both DFT axes dense sums on the f32 MFMA,
 * herm(kx) w2 |.|^2 reduced per band in a fixed order, then one workgroup adds the bands in ascending order and forms ratio and total.
 * uno_sobolev_backward: gx[b][t] = g * scale * f / (H W sqrt(num den)), f = the unnormalised inverse real 2-D DFT of Z (one launch: one
 * workgroup per (frame, band of 16 output columns), Z from memory, the half-transformed band in LDS), 0 where num == 0; num, den: the
 * frame's sums (per_frame = 1) or the sample's; g: float32 on the device, never read by the host - one value (g_per_row = 0) or one per
 * row of the grouping; gx is written through its own four element strides >= 0 (a (B, S, S, T) gradient where it lies).  No gradient
 * for y.  No clamping: a zero target gives inf / NaN as the stock form does.
 * No atomics; the decomposition is a function of (H, W) only, every sum has a fixed order and a frame's arithmetic does not depend on its
 * batch: two calls, a call under uno_reserve_cus and a graph replay give the same bits.  No synchronisation, allocation or read-back;
 * twiddle tables are uploaded as uno_upload_table does (safe under graph capture).  float32 only; 8 <= H, W <= 512 (odd sizes included,
 * both kernels hold 512 points a side in LDS), T >= 1, B >= 0, 64-bit offsets; B == 0 returns 0 without touching the device.  ws:
 * scratch of uno_sobolev_ws_bytes() bytes (0 for bad sizes), 8-byte aligned, need not be initialised.  Errors (-1, before any launch):
 * a null pointer (z excepted), sizes out of range, a negative stride, per_frame / g_per_row not 0 or 1. */
long long uno_sobolev_ws_bytes(int B, int T, int H, int W);
int uno_sobolev_forward(const float* x, long long x_batch, long long x_frame, long long x_row, long long x_elem, const float* y,
                        long long y_batch, long long y_frame, long long y_row, long long y_elem, const float* w2, float* sums, float* ratio,
                        float* total, void* z, void* ws, int B, int T, int H, int W, int per_frame, void* stream);
int uno_sobolev_backward(const void* z, const float* sums, const float* g, int g_per_row, float scale, int per_frame, float* gx,
                         long long gx_batch, long long gx_frame, long long gx_row, long long gx_elem, int B, int T, int H, int W,
                         void* stream);

/* One step of the NS-2D evaluation roll-out in one launch (additive: the ABI version stays 14).  The reference's validation and test
 * loops (ns_train_2d.py:94-107, 141-157) run the model T_f times under no_grad, feed each prediction back into the input window and
 * report the sum of the per-step relative L2 errors and the error of the whole trajectory; between two forward passes they spend a
 * `cat` for the window, a strided slice of the target, six launches of LpLoss and a `cat` that rebuilds the prediction.  Dense float32:
 *   window (B, C, P)  channels-first; channels [0, T_in) are the frames, [T_in, C) the model's positional features (never touched)
 *   frame  (B, P)     the model's new prediction
 *   target (B, T, P)  the ground truth, TIME-MAJOR (one transposing copy per batch: every step reads a dense slice)
 *   pred   (B, T, P)  or NULL
 * uno_rollout_advance, step t:  ws[b][chunk][t] = (sum (frame - target[:, t])^2, sum target[:, t]^2) over the chunk's pixels;
 *   pred[b][t][:] = frame[b][:] if pred is given;  if shift != 0 the window moves IN PLACE: window[b][k][:] = window[b][k + 1][:] for
 *   k < T_in - 1, then window[b][T_in - 1][:] = frame[b][:] (one thread moves a pixel's whole column in ascending k: no second buffer).
 *   frame, target, pred and ws must not overlap the window or each other.
 *   Without ground truth (a free-running roll-out): target == NULL together with ws == NULL makes the same pass with no sums - only
 *   pred[b][t][:] = frame[b][:] and the shift, of which at least one must be asked for.  T is then pred's time length and nothing else:
 *   any T >= 1 (the cap of 256 belongs to the finish kernel's workspace).  One of target / ws without the other is refused.
 * uno_rollout_finish, after the last step (every t of 0 ... T - 1 written): the finish launch of uno_rel_l2_steps on ws -
 *   sums (B, T, 2), rel (B, T + 1), totals (2) with the meaning they have there; rel[b][T] = sqrt(sum_t num) / sqrt(sum_t den) is the
 *   whole-trajectory error, so the prediction never has to be assembled for it.
 * 1 <= T_in <= C, 1 <= T <= 256, 0 <= t < T, P >= 1 (64-bit offsets); B == 0 returns 0 without touching the device.  No atomics; the
 * chunk decomposition is a function of P alone (about 1024 pixels per chunk, at most 64 chunks; not of the CU count or
 * uno_reserve_cus), so two calls give the same bits.  No clamping: a zero target slice gives +inf (NaN for 0 / 0).  16-byte accesses
 * where P % 4 == 0.  ws: uno_rollout_ws_bytes() = 8 * B * chunks(P) * T bytes (0 for bad sizes; never shrinks as P grows). */
long long uno_rollout_ws_bytes(int B, long long P, int T);
int uno_rollout_advance(float* window, const float* frame, const float* target, float* pred, void* ws, int B, int C, int T_in, long long P,
                        int T, int t, int shift, void* stream);
int uno_rollout_finish(const void* ws, float* sums, float* rel, float* totals, int B, long long P, int T, void* stream);

/* The NS-2D TRAINING roll-out without a window tensor (additive: the ABI version stays 14).  The reference's training loop
 * (ns_train_2d.py:46-68) runs the model T_f times, concatenates each prediction into the input window (`xx = torch.cat((xx[..., step:],
 * im), dim=-1)`), sums `myloss(im, y)` over the steps and runs ONE backward through the unrolled chain: per step a `cat`, six launches
 * of LpLoss, and in the backward pass a zero-fill and a copy per slice of every `cat` plus the additions that merge a window's
 * gradients.  The window of step t is T_in consecutive frames of the sequence "the T_in given frames, then the predictions", and the
 * only layer that reads it is the first lift `fc`, a point-wise map of C = T_in + F channels to Cm.  Dense float32:
 *   given  (B, T_in, P)    the input frames, channels-first
 *   pred, target, gpred (B, T, P)   time-major, as uno_rollout_advance writes pred (shift = 0) and reads target
 *   feat   (F, P)          the model's positional features: ONE table for all batch entries (may be NULL when F = 0)
 *   w (Cm, C), bias (Cm) or NULL   columns in the order [frames, features]
 *   frame j of the sequence = given[:, j] for j < T_in, otherwise pred[:, j - T_in]
 * uno_rollout_lift, window t:  h[b][m][p] = bias[m] + sum_{k<T_in} w[m][k] frame_{t+k}[b][p] + sum_{f<F} w[m][T_in+f] feat[f][p],
 *   summed in ascending column order; reads pred[:, 0 ... t - 1] (pred may be NULL for t = 0).
 * uno_rollout_lift_backward, window t, given gh (B, Cm, P) - ONE launch:
 *   parts: the workgroup of (b, chunk) writes block [t][b][chunk] of (Cm, C + 1) floats, gw[m][c] = sum gh x over its pixels with the
 *     bias sums in column C - the layout uno_channel_wgrad_finish sums.  parts holds uno_rollout_lift_bwd_ws_bytes() bytes = the blocks
 *     of all T windows back to back: after the T calls ONE uno_channel_wgrad_finish(parts, gw, gb, C, Cm, bytes / (4 Cm (C + 1)), ...)
 *     gives the layer's weight and bias gradient of the whole roll-out;
 *   gpred[b][q][p] += sum_m w[m][k] gh[b][m][p] for every predicted frame q = t + k - T_in >= 0 of the window but the newest (the caller
 *     clears gpred before the first call of a backward pass; a thread owns its pixel: no atomics);
 *   for t >= 1, gframe (B, P) = the COMPLETE gradient of the newest frame q = t - 1, the model's output of step t - 1:
 *     gpred[b][q][p] + sum_m w[m][T_in-1] gh[b][m][p] + gL[0] (pred - target)[b][q][p] / (sqrt(num[b][q]) sqrt(den[b][q]))
 *     - complete when the windows are walked in DESCENDING t, as a backward pass walks them: every later window has added its share.
 *     num / den are the `sums` (B, T, 2) of uno_rollout_finish, gL (1 float on the device) the gradient at the loss: no host
 *     synchronisation.  Where num == 0 the loss term is 0 (the backward of torch.linalg.vector_norm); a zero den gives inf / NaN.
 *     For t = 0 nothing but parts is written (target, sums, gL, gpred, gframe and pred may be NULL).
 * uno_rollout_loss_seed: gframe[b][p] = gL[0] (pred - target)[b][T-1][p] / (sqrt(num[b][T-1]) sqrt(den[b][T-1])), the gradient of the
 *   last frame (no lift follows it).
 * 1 <= T_in, 0 <= F, T_in + F <= 32, 1 <= Cm <= 64, 1 <= T <= 256, 0 <= t < T, P >= 1; B == 0 returns 0 without touching the device.
 * The chunk decomposition is uno_rollout_advance's (a function of P alone) and every sum runs in a fixed order: two calls, a call under
 * uno_reserve_cus and a graph replay give the same bits.  The training loss itself is totals[0] of uno_rollout_finish. */
int uno_rollout_lift(const float* given, const float* pred, const float* feat, const float* w, const float* bias, float* h, int B, int T_in,
                     int F, int Cm, long long P, int T, int t, void* stream);
long long uno_rollout_lift_bwd_ws_bytes(int B, int T_in, int F, int Cm, long long P, int T);
int uno_rollout_lift_backward(const float* gh, const float* given, const float* pred, const float* target, const float* feat, const float* w,
                              const float* sums, const float* gL, float* gpred, float* gframe, void* parts, int B, int T_in, int F, int Cm,
                              long long P, int T, int t, void* stream);
int uno_rollout_loss_seed(const float* pred, const float* target, const float* sums, const float* gL, float* gframe, int B, long long P, int T,
                          void* stream);

/* The same three calls on a WINDOW of a wider plane (ABI 10).  The reference crops the domain padding before its last two layers
 * (darcy_flow_uno2d.py:125-131: `x_c5[..., :-padding, :-padding]`, then fc1 - GELU - fc2 on S x S points); here those layers read
 * the padded (S + pad)^2 tensors in place and touch the domain only: the pixel axis of the call is rows x cols logical pixels,
 * row r starting r * pitch elements into a channel plane, channel planes `plane` elements apart (plane >= rows * pitch) - for
 * EVERY operand of the call (x1, x2, y1, y2, y_act, dgelu_of; gy; pre, gpre; proj_out and gout with one plane per batch entry).
 * cols is a multiple of 4 with 260 <= cols <= pitch and rows * cols < 2^24: pass the domain width rounded UP to a multiple of 4 -
 * the extra columns are ordinary points of the padded grid (their output gradient is zero).  Elements outside the window are
 * neither read nor written: a gradient tensor produced by a windowed call must have its border cleared by the caller.
 * Float32 only; uno_channel_mix2_win runs the tiled and split kernels (not the wide / few-input forms), uno_channel_wgrad2_win needs
 * more than 4 input channels; scratch sizes as for the dense calls with P = rows * cols. */
int uno_channel_mix2_win(const float* x1, const float* x2, int C1, const float* w, const float* bias, float* y1, float* y2, int Co1,
                         float* y_act, int B, int Ci, int Co, int rows, int cols, int pitch, long long plane, int transpose_w,
                         int accumulate, int act_in, const float* dgelu_of, const float* proj_w, const float* proj_b, float* proj_out,
                         void* stream);
int uno_channel_wgrad2_win(const float* gy, const float* x1, const float* x2, int C1, float* gw, float* gb, void* ws, int B, int Ci,
                           int Co, int rows, int cols, int pitch, long long plane, int act_x, int accumulate, void* stream);
int uno_gelu_project_backward_win(const float* pre, const float* w, const float* gout, float* gpre, float* gw, float* gb, void* ws,
                                  int B, int C, int rows, int cols, int pitch, long long plane, void* stream);
/* ABI 12.  The backward pass of the models' last two layers in two launches, the gradient at fc1's output never in memory
 * (reference darcy_flow_uno2d.py:125-131, `x = self.fc1(x); x = F.gelu(x); x = self.fc2(x)` on `torch.cat([x_c5, x_fc0], dim=1)`;
 * uno_gelu_project_backward wrote that gradient - 726 MB at 421^2, batch 16 - and the input-gradient and weight-gradient calls each
 * read it back).  With pre = fc1's output kept by the forward call, w2 = fc2's weights (Co) and gout (B, plane) the gradient at the
 * model output, gy[b][o][q] = w2[o] gelu'(pre[b][o][q]) gout[b][q] is formed where the two kernels stage their operand:
 *   g1 (B, C1, plane), g2 (B, Ci - C1, plane) = w^T gy, split at the sources (g1 multiplied by gelu'(x1) when act_in: x1 was read through
 *     the GELU); gw (Co, Ci) [+]= gy [gelu](x1) | x2 ^T, gb (Co) [+]= sum gy (accumulate_w = 1 adds; gb may be NULL);
 *     gw2 (Co) = sum gelu(pre) gout, gb2 (1) = sum gout (overwritten; gb2 may be NULL).
 * Geometry as the *_win calls (rows x cols window of planes `plane` elements apart, row r at r * pitch; elements outside the window are
 * neither read nor written), or rows = cols = pitch = 0: dense planes of `plane` pixels.  x2 = NULL: one source (C1 is ignored).
 * uno_project_backward_applies: 1 where both kernels take the shape (float32; Ci a multiple of 128, Co a multiple of 16 below 128, sources
 * split at a multiple of 64, >= 100 000 pixels in all, a multiple of 4 per plane) - elsewhere use the three separate calls.
 * ws: uno_project_backward_ws_bytes(B, Ci, Co, pixels per plane = rows * cols) bytes. */
int uno_project_backward_applies(int B, int C1, int Ci, int Co, int rows, int cols, int pitch, long long plane);
long long uno_project_backward_ws_bytes(int B, int Ci, int Co, long long P);
int uno_project_backward(const float* x1, const float* x2, int C1, const float* w, const float* pre, const float* w2, const float* gout,
                         float* g1, float* g2, float* gw, float* gb, float* gw2, float* gb2, void* ws, int B, int Ci, int Co, int rows,
                         int cols, int pitch, long long plane, int act_in, int accumulate_w, void* stream);
/* Everything outside the top-left rows x cols corner of n_planes contiguous (Hp, Wp) float32 planes := 0 (the border a windowed
 * call leaves untouched in a fresh gradient tensor). */
int uno_clear_border(float* t, long long n_planes, int Hp, int Wp, int rows, int cols, void* stream);
/* The end of the lift with the domain padding (reference darcy_flow_uno2d.py:100-107: `x_fc0 = self.fc0(x_fc); x_fc0 = F.gelu(x_fc0)`,
 * permute, `F.pad(x_fc0, [0, padding, 0, padding])`) in one pass: y_act (B, Co, Hp, Wp) = zero-pad(gelu(Wm [gelu](x (B, Ci, H, W)) + bias))
 * at the end of both axes, written by the layer's own store epilogue; y (B, Co, H, W) or NULL: the pre-activation result, kept only
 * if the caller wants it.  Backward without it: uno_channel_mix_dgelu_padded RECOMPUTES the layer (Ci << Co: reading x again is
 * half of what storing and re-reading y costs) and returns gz (B, Co, H, W) = gelu'(Wm [gelu](x) + bias) * g_padded[..., :H, :W] -
 * the gradient at the layer's output, ready for uno_channel_mix (transposed) / uno_channel_wgrad.
 * 260 <= W <= Wp, H * W < 2^24, float32. */
int uno_channel_mix_act_padded(const float* x, const float* w, const float* bias, float* y, float* y_act, int B, int Ci, int Co, int H,
                               int W, int Hp, int Wp, int act_in, void* stream);
int uno_channel_mix_dgelu_padded(const float* x, const float* w, const float* bias, const float* g_padded, float* gz, int B, int Ci,
                                 int Co, int H, int W, int Hp, int Wp, int act_in, void* stream);
/* The whole lift of the 2-D models (reference darcy_flow_uno2d.py:98-107): x (B, Cin <= 3, H, W) = [a(x, y), x, y] channels-first,
 *   h = fc_n1(x) (Cm = 16 or 32 channels; w1 (Cm, Cin), b1 (Cm) or NULL),  z = fc0(gelu(h)) (w0 (Co, Cm), b0 or NULL),
 *   act (B, Co, Hp, Wp) = zero-pad(gelu(z))
 * with NEITHER h nor z stored: h is 12 bytes per pixel of input against 128 of output, so every kernel that needs it evaluates it
 * from x.  With Cm = 32, Co = 64 the forward pass is one dedicated kernel that writes whole padded rows, and the backward pass is
 * one kernel per pixel tile (recomputed a = gelu(h) and z; gz = gelu'(z) g and gh = gelu'(h) w0^T gz stay on the chip, both layers'
 * weight-gradient sums are accumulated there) plus two small reductions; other widths run the generic kernels with gz and gh in
 * scratch.
 * uno_lift_backward: g_act (B, Co, Hp, Wp) -> gw1 (Cm, Cin), gb1 (Cm) or NULL, gw0 (Co, Cm), gb0 (Co) or NULL (written, not
 * accumulated; no gradient for x - it is data); ws: uno_lift_bwd_ws_bytes() bytes.  260 <= W <= Wp, H * W < 2^24, float32. */
int uno_lift_forward(const float* x, const float* w1, const float* b1, const float* w0, const float* b0, float* act, int B, int Cin,
                     int Cm, int Co, int H, int W, int Hp, int Wp, void* stream);
long long uno_lift_bwd_ws_bytes(int B, int Cin, int Cm, int Co, int H, int W);
int uno_lift_backward(const float* x, const float* w1, const float* b1, const float* w0, const float* b0, const float* g_act, float* gw1,
                      float* gb1, float* gw0, float* gb0, void* ws, int B, int Cin, int Cm, int Co, int H, int W, int Hp, int Wp,
                      void* stream);
/* ABI 11.  The same with a SECOND gradient of the padded activation, valid on the H x W domain of the same (Hp, Wp) planes: the lift's
 * output feeds two layers (conv0 and, through the skip connection, fc1: reference darcy_flow_uno2d.py:108-127), and the kernel that
 * streams the gradient adds the two as it reads them - no accumulation pass over the 64-channel tensor.  g_act2 may be NULL.
 * uno_lift_backward_takes_second: 1 where the one-kernel form runs (only it takes the second tensor). */
int uno_lift_backward_takes_second(int B, int Cin, int Cm, int Co, int H, int W, int Hp, int Wp);
int uno_lift_backward2(const float* x, const float* w1, const float* b1, const float* w0, const float* b0, const float* g_act,
                       const float* g_act2, float* gw1, float* gb1, float* gw0, float* gb0, void* ws, int B, int Cin, int Cm, int Co,
                       int H, int W, int Hp, int Wp, void* stream);

/* GELU followed by zero padding at the end of both axes (the lift's last activation + domain padding, reference
 * darcy_flow_uno2d.py:103-107): backward = 0: out (n_img, Hp, Wp) = pad(gelu(s (n_img, H, W))), gy ignored;
 * backward = 1: out (n_img, H, W) = gelu'(s) * gy[:, :H, :W] with gy (n_img, Hp, Wp). */
int uno_gelu_pad(const float* s, const float* gy, float* out, int n_img, int H, int W, int Hp, int Wp, int backward,
                 void* stream);

/* InstanceNorm (affine, biased variance, eps, no running statistics) optionally fused with the exact-erf GELU that follows
 * it in an operator block (reference integral_operators.py:269-270, 277-283; 3-D :497-498, 506-512).  x, y: (rows, N) with
 * rows = batch * C (channel of row r = r % C) and N = grid points; gamma, beta: (C) or NULL; mean, rstd: (rows) outputs kept
 * for the backward.  Backward: gx, and the per-row sums s1 = sum g_z, s2 = sum g_z * xhat (g_z = gradient at the affine
 * output) whose sums over the batch are the gradients of beta and gamma. */
int uno_instnorm_forward(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long long rows,
                         int C, long long N, float eps, int gelu, void* stream);
int uno_instnorm_backward(const float* x, const float* gy, const float* gamma, const float* beta, const float* mean,
                          const float* rstd, float* gx, float* s1, float* s2, long long rows, int C, long long N, int gelu,
                          void* stream);

/* One Adam update of one parameter tensor with the reference optimiser's semantics (Adam.py:27-52): coupled L2
 * weight decay (g += wd p) and, for complex tensors, the second moment from g conj(g) (one real entry per complex
 * entry).  p, g, m: float views (interleaved re/im when is_complex), v: n floats; n = entries (complex entries when
 * is_complex); step = 1-based step count for the bias corrections.  Updates p, m, v in place. */
int uno_adam_step(float* p, const float* g, float* m, float* v, long long n, int is_complex, double lr, double beta1,
                  double beta2, double eps, double weight_decay, int step, void* stream);

/* The same update for a list of parameter tensors (host arrays of device pointers / sizes / flags): one call per
 * optimiser step instead of one per tensor. */
int uno_adam_step_multi(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                        const long long* n, const int* is_complex, double lr, double beta1, double beta2, double eps,
                        double weight_decay, int step, void* stream);

/* The same with the step count kept ON THE DEVICE (ABI 7), so that the update can be captured in a HIP graph and replayed:
 * `step_counter` (one int32, the number of steps taken so far: zero before the first step, the loaded count after a resume) is
 * advanced by one and the bias corrections lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t) are evaluated in double by a one-thread kernel
 * into `scalars` (FOUR floats of device scratch owned by the caller: the two corrections, eps, weight_decay), which the update
 * kernel reads instead of kernel arguments.  Same arithmetic as uno_adam_step_multi with step = t.
 * ABI 9: `hyper` (NULL, or three doubles on the device: lr, eps, weight_decay) - when given, the three are read from the device at
 * execution time instead of from the arguments, so a learning-rate schedule (reference ns_train_2d.py:37,113) takes effect on
 * the next replay of a captured step: the caller rewrites the doubles between replays. */
int uno_adam_step_multi_dev(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                            const long long* n, const int* is_complex, double lr, double beta1, double beta2, double eps,
                            double weight_decay, int* step_counter, float* scalars, const double* hyper, void* stream);

/* K26 (additive: these entry points were added WITHOUT an ABI bump, UNO_SPECTRAL_ABI_VERSION stays 14): the global L2 norm of a list of gradient tensors, the clip coefficient and the skip flag - all ON THE DEVICE, so that
 * "clip the gradient norm, skip a non-finite step" needs no host read and can be captured with the update.  g, n, is_complex: the
 * tables of uno_adam_step_multi (complex gradients count as their 2n floats).  Stage 1 writes one double partial sum of squares per
 * 1024 floats of every tensor into `ws` (uno_grad_norm_ws_bytes(...) bytes, caller-owned, need not be initialised: every partial
 * stage 2 reads was written by stage 1 of the same call); stage 2, one workgroup, adds them in a fixed order.  No atomics: the result
 * is bit-reproducible.  `max_norm`: ONE double on the device, read at execution time (+inf: never clip).  `state`: the record of
 * UNO_GRAD_NORM_RECORD doubles on the device, zeroed once by the caller:
 *   [UNO_GRAD_NORM_NORM]      the norm of this call (sqrt of a double sum: finite whenever it is representable)
 *   [UNO_GRAD_NORM_COEF]      min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_), evaluated in double, rounded to float
 *                             once; 1 when the norm is not finite
 *   [UNO_GRAD_NORM_FINITE]    1 / 0
 *   [.._STEPS, .._CLIPPED, .._SKIPPED, .._NONFINITE, .._SUM, .._MAX]   running figures since the caller last zeroed them: calls, calls
 *                             with coef < 1, calls with a non-finite norm under skip_nonfinite, calls with a non-finite norm, the sum
 *                             and the maximum of the finite norms. */
#define UNO_GRAD_NORM_NORM 0
#define UNO_GRAD_NORM_COEF 1
#define UNO_GRAD_NORM_FINITE 2
#define UNO_GRAD_NORM_STEPS 3
#define UNO_GRAD_NORM_CLIPPED 4
#define UNO_GRAD_NORM_SKIPPED 5
#define UNO_GRAD_NORM_NONFINITE 6
#define UNO_GRAD_NORM_SUM 7
#define UNO_GRAD_NORM_MAX 8
#define UNO_GRAD_NORM_RECORD 9
long long uno_grad_norm_ws_bytes(int n_tensors, const long long* n, const int* is_complex);
int uno_grad_norm(int n_tensors, const float* const* g, const long long* n, const int* is_complex, const double* max_norm,
                  int skip_nonfinite, double* ws, long long ws_bytes, double* state, void* stream);

/* uno_adam_step_multi_dev guarded by the record uno_grad_norm wrote earlier on the same stream: every gradient value is multiplied by
 * the clip coefficient BEFORE the coupled weight decay (g = coef g; g += wd p: "clip, then step()"), and - skip_nonfinite - a step
 * whose norm is not finite writes nothing: parameters, both moments and the step counter stay as they are, bit for bit. */
int uno_adam_step_multi_guarded(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                                const long long* n, const int* is_complex, double lr, double beta1, double beta2, double eps,
                                double weight_decay, int* step_counter, float* scalars, const double* hyper, const double* clip_state,
                                int skip_nonfinite, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Mixed precision (BASELINE.json configs[4]: bf16 activations, half-precision weight storage, f32 accumulation).
 * The reference has no behaviour here (integral_operators.py:187 raises on bfloat16 input); the contract is "the float32
 * operator applied to the values the kernels read (inputs rounded once to bf16 / fp16), output rounded once to bf16".
 * `_bf16` entry points are their float32 namesakes with ACTIVATION tensors (x, y, grad tensors, `dgelu_of`) stored as
 * bfloat16 (void*); weights, biases, statistics, weight gradients, spectra and every accumulation stay float32 / complex64.
 * `_f16w` / `_mixed`: the complex weights are read as (re, im) float16 pairs; weight gradients come back complex64 (they
 * belong to the float32 master copy an optimiser keeps).
 */
int uno_spectral_conv2d_forward_mixed(const void* x_bf16, const void* w1_f16, const void* w2_f16, void* y_bf16,
                                      float* xtrunc, void* ws, int B, int Ci, int Co, int H, int W, int Ho, int Wo,
                                      int modes1, int modes2, void* stream);
int uno_spectral_conv2d_backward_mixed(const void* gy_bf16, const float* xtrunc, const void* w1_f16, const void* w2_f16,
                                       void* gx_bf16, float* gw1, float* gw2, void* ws, int B, int Ci, int Co, int H, int W,
                                       int Ho, int Wo, int modes1, int modes2, void* stream);
int uno_mode_mix_f16w(const float* in, const void* const* w_f16, float* out, int op, int B, int Ci, int Co, int ncorner,
                      int modes_per_corner, void* stream);
int uno_dft2d_forward_grouped_bf16(const void* images, float* spec, int n_img, int H, int W, int m1, int m2, float scale,
                                   int hermitian_cols, int mask_overlap, int group, int stride, int offset, void* stream);
int uno_dft2d_inverse_grouped_bf16(const float* spec, void* images, int n_img, int H, int W, int m1, int m2, float scale,
                                   int hermitian_cols, int mask_overlap, int group, int stride, int offset, void* stream);
int uno_resample2d_bf16(const void* in, void* out, float* tmp, int n_img, int H, int W, int Ho, int Wo, const int* startH,
                        const float* wtH, int KH, const int* startW, const float* wtW, int KW, const int* tile_p0,
                        const float* tile_w, int NP, int accumulate, void* stream);
int uno_channel_mix_bf16(const void* x, const float* w, const float* bias, void* y, int B, int Ci, int Co, long long P,
                         int transpose_w, int accumulate, int act_in, const void* dgelu_of, void* stream);
int uno_channel_wgrad_bf16(const void* gy, const void* x, float* gw, float* gb, void* ws, int B, int Ci, int Co, long long P,
                           int act_x, void* stream);
int uno_channel_mix2_bf16(const void* x1, const void* x2, int C1, const float* w, const float* bias, void* y1, void* y2, int Co1,
                          void* y_act, int B, int Ci, int Co, long long P, int transpose_w, int accumulate, int act_in,
                          const void* dgelu_of, const float* proj_w, const float* proj_b, void* proj_out, void* stream);
int uno_channel_wgrad2_bf16(const void* gy, const void* x1, const void* x2, int C1, float* gw, float* gb, void* ws, int B, int Ci,
                            int Co, long long P, int act_x, int accumulate, void* stream);
int uno_gelu_project_forward_bf16(const void* pre, const float* w, const float* bias, void* out, int B, int C, long long P,
                                  void* stream);
int uno_gelu_project_backward_bf16(const void* pre, const float* w, const void* gout, void* gpre, float* gw, float* gb,
                                   void* ws, int B, int C, long long P, void* stream);
int uno_gelu_pad_bf16(const void* s, const void* gy, void* out, int n_img, int H, int W, int Hp, int Wp, int backward,
                      void* stream);
int uno_instnorm_forward_bf16(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                              long long rows, int C, long long N, float eps, int gelu, void* stream);
int uno_instnorm_backward_bf16(const void* x, const void* gy, const float* gamma, const float* beta, const float* mean,
                               const float* rstd, void* gx, float* s1, float* s2, long long rows, int C, long long N,
                               int gelu, void* stream);

/* Scratch for the any-mode transforms (ABI 7).  Mode counts beyond the MFMA kernels' compiled range (modes1 > 40 or modes2 > 48 - the
 * reference's DEFAULT modes dim1//2 - 1, dim2//2, integral_operators.py:153-158) run two-pass plain-FMA transforms that need
 *   uno_dft2d_any_ws_bytes(n_img, H, W, m1, m2) = 8 n_img H m2 bytes of device scratch (0 inside the MFMA range)
 * per transform.  The library allocates nothing itself: the caller registers a device buffer for the calling THREAD with
 * uno_scratch_provide(ptr, bytes) before a call that may take that form (every uno_dft2d_* / uno_spectral_conv2d_* entry point; the
 * composite ones run their two transforms one after the other on the caller's stream, so max over the two sizes is enough), and clears it
 * with uno_scratch_provide(NULL, 0) afterwards.  The buffer must stay valid until the enqueued work has run (stream-ordered allocators:
 * free it on the same stream).  A call that needs more than was provided fails with -6 and a message naming the size. */
long long uno_dft2d_any_ws_bytes(int n_img, int H, int W, int m1, int m2);
int uno_scratch_provide(void* ptr, long long bytes);
/* ABI 10: the channel-mix entry points (uno_channel_mix*, uno_channel_mix2*) also look at the registered scratch.  Their wide layers
 * (>= 128 input channels; 32 on bfloat16 activations) run on three-piece bf16 operands; with uno_channel_mix_ws_bytes(Ci, Co, P, bf16)
 * = 6 Ci Co bytes of 16-byte aligned scratch (0: the shape never takes that form) the weights are split ONCE per call by a small
 * launch instead of by every workgroup.  Optional: without (enough) scratch the call runs as before, with identical results. */
long long uno_channel_mix_ws_bytes(int Ci, int Co, long long P, int bf16);

/* Batched transposing copy between the channels-last and the channels-first layout of an activation (ABI 8):
 *   out[b][c][r] = in[b][r][c],   b < B, r < R, c < C
 * in: R rows of C contiguous floats at pitch ld_in >= C, batch stride sb_in; out: C rows of R contiguous floats at pitch
 * ld_out >= R, batch stride sb_out (pitches and strides in floats).  The reference's blocks accept any strides because they go
 * through torch.fft / F.conv (integral_operators.py:187, 233); its model files hand the first block a channels-last tensor
 * (darcy_flow_uno2d.py:104-107: `permute` of the nn.Linear lift + F.pad; navier_stokes_uno3d.py:316-318) and their autograd
 * graph hands channels-last gradients back.  The kernels of this library read channels-first images, so the host side converts
 * with this entry point (R = pixels, C = channels: NHWC -> NCHW; R = channels, C = pixels: NCHW -> NHWC) instead of a generic
 * strided copy. */
int uno_transpose_batched(const float* in, float* out, int B, long long R, int C, long long ld_in, long long sb_in,
                          long long ld_out, long long sb_out, void* stream);

/* Short-row windows (additive, ABI 14): the two ends of the NS-3D models on (B, C, H, W, Tp) tensors without the concatenation, the
 * time-axis crop, the separate GELU and the time-axis padding.  A window is rows x cols logical pixels; logical pixel (r, c) lives at
 * element r * pitch + col0 + c of its channel plane and planes are `plane` >= rows * pitch elements apart (rows = H * W, pitch = Tp).
 * Accepted: 1 <= cols, 0 <= col0, col0 + cols <= pitch <= 256 (any parity), rows * pitch < 2^24, 1 <= C1 <= Ci <= 1024, 1 <= Co;
 * anything else returns a negative code with a message naming these limits before any launch.  B == 0 or rows == 0: a successful
 * no-op (nothing is written).  float32; no allocation, no synchronisation, no table: capturable on the first call; the launch geometry
 * is a function of the shape alone (not of uno_reserve_cus or the sweep direction) and no result depends on what the outputs held. */
/* y (B, Co, rows * cols) dense = w (Co, Ci) . cat([gelu](x1), x2) + bias with x1 (B, C1, plane), x2 (B, Ci - C1, plane) read through
 * the window and nothing outside it (x2 == NULL: one source of Ci channels).  Replaces `torch.cat([x_c8, x_fc0], dim=1)`, the crop
 * `x_c8[..., :-self.padding]` and `self.fc1` of the reference (navier_stokes_uno3d.py:358-382; the `[padding:-padding]` form of :566-570). */
int uno_channel_mix2_rows(const float* x1, const float* x2, int C1, const float* w, const float* bias, float* y, int B, int Ci, int Co,
                          int rows, int cols, int pitch, int col0, long long plane, int act_in, void* stream);
/* Backward of the above for the sources (what autograd does for navier_stokes_uno3d.py:358-382: zero-fill, slice copy, two narrowing
 * copies): gy (B, Co, rows * cols) dense -> g1 (B, C1, plane) and g2 (B, Ci - C1, plane; NULL: not wanted) = w^T gy inside the window
 * and +0.0f in the border columns, the first rows * pitch elements of every plane from ONE pass (elements beyond are not touched by
 * this call; the Python binding, which allocates g1 / g2 itself, zero-fills such a tail).
 * dgelu_of (B, C1, plane; NULL: none): g1 is multiplied by gelu'(dgelu_of) on the window (the act_in form). */
int uno_channel_mix2_rows_grad(const float* gy, const float* w, int C1, const float* dgelu_of, float* g1, float* g2, int B, int Ci,
                               int Co, int rows, int cols, int pitch, int col0, long long plane, void* stream);
/* Weight / bias gradient of the same layer (fc1 of navier_stokes_uno3d.py:380): gw (Co, Ci), gb (Co) or NULL from gy dense and the
 * windowed sources; the contract of uno_channel_wgrad2 (two stages, fixed summation order, no atomics; accumulate = 1 adds to gw / gb);
 * ws: uno_channel_wgrad_ws_bytes(B, Ci, Co, rows * cols) bytes. */
int uno_channel_wgrad2_rows(const float* gy, const float* x1, const float* x2, int C1, float* gw, float* gb, void* ws, int B, int Ci,
                            int Co, int rows, int cols, int pitch, int col0, long long plane, int act_x, int accumulate, void* stream);
/* The time-axis form of uno_channel_mix_act_padded - `x_fc0 = self.fc0(x_fc)`, `F.gelu(x_fc0)` and `F.pad(x_fc0, [0, self.padding, ...])`
 * of the reference (navier_stokes_uno3d.py:304-318) from the layer's own store: x (B, Ci, rows * cols) dense -> y (B, Co, rows * cols)
 * = w . [gelu](x) + bias (NULL: not kept) and y_act (B, Co, rows * pitch) = gelu(y) at columns [col0, col0 + cols) of every row,
 * +0.0f left and right of them. */
int uno_channel_mix_act_padded_rows(const float* x, const float* w, const float* bias, float* y, float* y_act, int B, int Ci, int Co,
                                    int rows, int cols, int pitch, int col0, int act_in, void* stream);
/* gz (n_planes, rows * cols) dense = gelu'(pre) * g_padded[window], pre dense, g_padded (n_planes, plane): the backward of the padding
 * and the GELU of navier_stokes_uno3d.py:306-318; the layer's own gradients follow from uno_channel_mix / uno_channel_wgrad on gz. */
int uno_dgelu_rows(const float* pre, const float* g_padded, float* gz, long long n_planes, int rows, int cols, int pitch, int col0,
                   long long plane, void* stream);

/* K22 (additive, ABI 14): the 2-D Navier-Stokes pseudo-spectral solver of the reference's data generator (Data Generation/Navier Stocks/
 * ns_datagen.py:15-140, vorticity form, Crank-Nicolson in time), whose torch.rfft / torch.irfft calls no current PyTorch has.
 * State: the half spectrum w_h (B, N, N/2 + 1) c64, interleaved, un-normalised like fft2 - the reference's irfft(onesided=False) reads
 * columns 0 ... N/2 of its full spectrum only, so nothing else ever influences an output.  f32; N a power of two in 32 ... 256; B >= 0,
 * B * N below 2^31.  ws: uno_ns2d_ws_bytes(B, N) = 5 * 8 * B * N * (N/2 + 1) bytes of scratch, which a call need not find initialised
 * (0 for sizes outside the range).  Every sum is a dense length-N sum on v_mfma_f32_16x16x4_f32 in a fixed order, and a sample's
 * arithmetic does not depend on B: two runs, a run split into two calls and a sample inside any batch give the same bits.  No entry
 * point synchronises, allocates or reads back (the (cos, sin) table of N is uploaded once per device as every transform here does, safe
 * under graph capture).  Offsets are 64-bit.  B == 0 or n_steps == 0: success, no launch.
 *   uno_ns2d_forward: w (B, N, N) f32 -> w_h = rfft2(w) (ns_datagen.py:26, 29: the initial vorticity and the forcing).  2 launches.
 *   uno_ns2d_inverse: w_h -> w (B, N, N) f32 = irfft2(w_h, s = (N, N)) (ns_datagen.py:125-127: a recorded snapshot): complex inverse along
 *     axis 0, then half spectrum -> real along axis 1 with the imaginary parts of columns 0 and N/2 ignored, 1 / N^2.  w_h is only read.
 *     2 launches.
 *   uno_ns2d_steps: n_steps time steps of ns_datagen.py:67-118 on w_h in place, 3 launches each from one loop: wave numbers
 *     [0 ... N/2-1, -N/2 ... -1] on both axes, the Nyquist row and column carrying k = -N/2 in the derivative multipliers and in
 *     lap = 4 pi^2 (kx^2 + ky^2) (not zeroed), lap[0,0] = 1, the dealias mask |k| <= (2/3)(N/2) on both axes on the non-linear term only,
 *     w_h <- (-dt F_h + dt f_h + (1 - dt visc lap / 2) w_h) / (1 + dt visc lap / 2).  f_h: the forcing's half spectrum (uno_ns2d_forward of
 *     f), (N, N/2 + 1) c64 shared by the batch (f_batched = 0) or (B, N, N/2 + 1) (f_batched != 0); must not alias w_h.
 * Errors (-1, before any launch): null pointers, N not a power of two or outside 32 ... 256, B < 0 or too large, n_steps < 0, delta_t not
 * finite or not positive, visc negative or not finite. */
long long uno_ns2d_ws_bytes(int B, int N);
int uno_ns2d_forward(const float* w, float* w_h, void* ws, int B, int N, void* stream);
int uno_ns2d_inverse(const float* w_h, float* w, void* ws, int B, int N, void* stream);
int uno_ns2d_steps(float* w_h, const float* f_h, int f_batched, void* ws, int B, int N, long long n_steps, double visc, double delta_t,
                   void* stream);

/* K23 (additive: these entry points were added WITHOUT an ABI bump, UNO_SPECTRAL_ABI_VERSION stays 14): the Darcy-flow data generator of
 * the reference's MATLAB files (Data Generation/darcy Flow/GRF.m, demo.m, solve_gwf.m).  Grid: K x K nodes i / (K - 1), K in 8 ... 512;
 * unknowns: the n x n interior nodes, n = K - 2, zero Dirichlet values on the border; 0 <= B <= 65535.  Planes are dense row-major.
 * Every sum has a fixed order (no atomics) and a sample's arithmetic does not depend on B, on its batch partners or on check_every: two
 * runs and a sample inside any batch give the same bits.  B == 0: success, no launch.
 *   uno_darcy_table_pitch(N): rows = columns of the zero-padded operand table of an N x N transform (N rounded up to the 64-wide tile; 0
 *     for N outside 1 ... 512).
 *   uno_darcy_transform: Y[b] = post o (M X[b] M^T), b < B, N x N planes, N in 1 ... 512, float32 (f32 != 0: v_mfma_f32_16x16x4_f32) or
 *     float64 (vector FMAs; one k-ascending chain per entry and pass).  M: (pitch, pitch) row-major, zero beyond N x N; post: (N, N) or
 *     NULL; tmp: B N N elements of scratch; X, Y, tmp distinct.  2 launches.  Replaces idct2 (GRF.m:21: M = the orthonormal inverse
 *     DCT-II matrix) and interp2(..., 'spline') between the uniform cell-centre and node grids (solve_gwf.m:11-12 and 35: M = the
 *     not-a-knot spline matrix), and is the DST-I pair of the solver's fast Poisson preconditioner.
 *   uno_darcy_apply: Ap (B, n, n) = A p, A the matrix of solve_gwf.m:16-32 applied and never formed: (K - 1)^2 times the sum over the
 *     four faces of (c + c_neighbour) / 2 (p - p_neighbour), p = 0 outside the interior; coef (B, K, K): the NODAL coefficient, any
 *     sign (the spline of a thresholded field overshoots below zero).  1 launch.
 *   uno_darcy_solve: P (B, K, K) = the nodal solution of A P = F on the interior with a zero border (solve_gwf.m:14-33, A \ F(:) replaced by
 *     conjugate gradients in float64, preconditioned by the constant-coefficient 5-point Laplacian applied as a float32 fast Poisson
 *     solve; flexible beta).  coef, F (B, K, K) float64 nodal planes.  Sample b stops (is frozen) once |r|_2 <= rtol |b|_2 - status 1 -
 *     or when p^T A p, rho or a norm is zero or not finite - status 2; status 0: max_iter reached.  iters (B) int32, relres (B)
 *     float64 = |r|_2 / |b|_2 of the recursive residual, status (B) int32.  F = 0: P = 0, 0 iterations, status 1.  The loop runs in the
 *     entry point, 9 launches per iteration; alpha and beta are formed on the device; the host reads the B status words once per
 *     check_every iterations (a stream synchronisation: not capturable) and stops when all are set.  ws: uno_darcy_ws_bytes(B, K)
 *     bytes, 8-byte aligned, need not be initialised (0 for sizes outside the range).
 * Errors (-1, before any launch): null pointers, K outside 8 ... 512, B outside 0 ... 65535, rtol not positive and finite,
 * max_iter < 1, check_every < 1, aliased buffers. */
long long uno_darcy_ws_bytes(int B, int K);
int uno_darcy_table_pitch(int N);
int uno_darcy_transform(const void* M, const void* X, void* Y, void* tmp, const void* post, int B, int N, int f32, void* stream);
int uno_darcy_apply(const double* coef, const double* p, double* Ap, int B, int K, void* stream);
int uno_darcy_solve(const double* coef, const double* F, double* P, int* iters, double* relres, int* status, void* ws, int B, int K,
                    double rtol, int max_iter, int check_every, void* stream);

/* Optional in-library kernel timing (HIP events recorded on the launch stream around every kernel
 * this library enqueues), used by bench.py for the live roofline figure.
 *   uno_profile_begin(max_records): start recording (drops records beyond max_records).
 *   uno_profile_end():   stop, wait for the recorded events, return the number of records.
 *   uno_profile_get(i, name, name_len, &ms, &bytes): record i - kernel name as rocprofv3 prints it
 *     (e.g. "uno::dft2d_fwd_kernel<2, 3>"), its duration in ms and its ALGORITHMIC bytes
 *     (each operand counted once, DESIGN.md section "Roofline accounting"). */
int uno_profile_begin(int max_records);
int uno_profile_end(void);
int uno_profile_get(int index, char* name, int name_len, double* ms, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* UNO_SPECTRAL_H */
