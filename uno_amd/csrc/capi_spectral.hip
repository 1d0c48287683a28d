// C ABI of libuno_spectral.so, the spectral entry points: pruned 2-D transforms, per-mode GEMMs, the leading-axis transform, the 2-D and
// 3-D spectral convolutions, 3-D FFT resampling and their *_ws_bytes (core: capi.hip).
#include "../../include/uno_spectral.h"
#include "uno_common.h"

#include <cstdlib>
#include <map>
#include <mutex>

namespace uno {

static int check_modes2d(const char* who, int H, int W, int Ho, int Wo, int m1, int m2) {
    if (H < 1 || W < 1 || Ho < 1 || Wo < 1) { set_error("%s: empty grid %dx%d -> %dx%d", who, H, W, Ho, Wo); return -1; }
    if (m1 < 1 || m1 > H || m1 > Ho) {
        set_error("%s: modes1=%d incompatible with grid rows %d -> %d (need 1 <= modes1 <= min rows)", who, m1, H, Ho);
        return -1;
    }
    if (m2 < 1 || m2 > W / 2 + 1 || m2 > Wo / 2 + 1) {
        set_error("%s: modes2=%d incompatible with grid cols %d -> %d (need modes2 <= cols/2+1)", who, m2, W, Wo);
        return -1;
    }
    return 0;
}

static int dft2d(bool inverse, const float* in, float* out, int n_img, int H, int W, int m1, int m2, float scale,
                 int herm, int mask, hipStream_t s, int sp_group = 0, int sp_stride = 0, int sp_offset = 0, int bf16 = 0, int n_decide = 0) {
    const char* who = inverse ? "uno_dft2d_inverse" : "uno_dft2d_forward";
    if (n_img < 0) { set_error("%s: negative image count", who); return -1; }
    if (n_img > 0 && (!in || !out)) { set_error("%s: null pointer", who); return -1; }
    if (int rc = check_modes2d(who, H, W, H, W, m1, m2)) return rc;
    if (n_img == 0) return 0;
    Dft2dParams p;
    p.in = in; p.out = out; p.n_img = n_img; p.H = H; p.W = W; p.m1 = m1; p.m2 = m2;
    p.scale = scale; p.herm = herm ? 1 : 0; p.mask = mask ? 1 : 0; p.bf16 = bf16 ? 1 : 0;
    if (sp_group <= 0) { sp_group = n_img; sp_stride = 0; sp_offset = 0; }          // plain layout: spectrum i of image i
    if (sp_offset < 0 || sp_stride < sp_offset + sp_group || n_img % sp_group) {
        if (!(sp_stride == 0 && sp_offset == 0 && sp_group == n_img)) {
            set_error("%s: bad spectrum grouping (group %d, stride %d, offset %d, images %d)", who, sp_group, sp_stride, sp_offset, n_img);
            return -1;
        }
    }
    p.sp_group = sp_group; p.sp_stride = sp_stride; p.sp_offset = sp_offset;
    p.twH = twiddle_table(H);
    p.twW = twiddle_table(W);
    if (!p.twH || !p.twW) return -6;
    // mode counts beyond the compiled MFMA range (the reference's default modes, integral_operators.py:153-158): any-mode form
    if (m1 > 40 || m2 > 48) return launch_dft2d_generic(p, inverse, thread_scratch().ptr, thread_scratch().bytes, s);
    // many small images (3-D planes, coarse 2-D levels): plane-batched kernels (dft2d_plane.hip).  n_decide > 0: the image count the choice
    // is made for (one source of a two-source layer call takes the kernels its concatenation would take)
    Dft2dParams q = p;
    if (n_decide > 0) q.n_img = n_decide;
    if (inverse ? dft2d_inv_plane_applies(q) : dft2d_fwd_plane_applies(q))
        return inverse ? launch_dft2d_inv_plane(p, s) : launch_dft2d_fwd_plane(p, s);
    // bfloat16 images: row stage on the bf16 MFMA (dft2d_b16.hip)
    if (dft2d_b16_applies(p)) {
        const int rc = inverse ? launch_dft2d_inv_b16(p, s) : launch_dft2d_fwd_b16(p, s);
        if (rc != -3) return rc;        // -3: the shape's LDS need exceeds a CU (tall images with many row modes): the f32-MFMA forms take it
    }
    return inverse ? launch_dft2d_inv(p, s) : launch_dft2d_fwd(p, s);
}

// op 0: forward mix, op 1: grad wrt input spectrum, op 2: weight grad
// rc: 0 = launch p; 1 = nothing to launch (done); negative = error
static int mode_gemm_params(ModeGemmParams& p, int op, const float2* act, const float2* const* w, const float2* go, float2* out_act,
                            float2* const* out_w, int B, int Ci, int Co, int nc, int Mc, hipStream_t s, int w_half, int accumulate,
                            bool plan_only = false) {
    if (B < 0 || Ci < 1 || Co < 1 || nc < 1 || nc > 4 || Mc < 1) {
        set_error("mode gemm: bad sizes B=%d Ci=%d Co=%d corners=%d modes=%d", B, Ci, Co, nc, Mc);
        return -1;
    }
    if (B == 0 && op != 2) return 1;
    const long long P = (long long)nc * Mc;
    p.ncorner = nc; p.Mc = Mc; p.accumulate = (op == 2 && accumulate) ? 1 : 0;
    p.A.half = 0; p.B.half = (op != 2 && w_half) ? 1 : 0;
    for (int c = 0; c < 4; ++c) { p.A.base[c] = nullptr; p.B.base[c] = nullptr; p.out[c] = nullptr; }
    if (op == 0) {              // O[b,o] = sum_i X[b,i] W[i,o]
        p.M = B; p.N = Co; p.K = Ci;
        p.A.s0 = (long long)Ci * P; p.A.s1 = P; p.A.conj = 0;
        p.B.s0 = (long long)Co * Mc; p.B.s1 = Mc; p.B.conj = 0;
        p.o_sm = (long long)Co * P; p.o_sn = P;
        for (int c = 0; c < nc; ++c) { p.A.base[c] = act + (long long)c * Mc; p.B.base[c] = w[c]; p.out[c] = out_act + (long long)c * Mc; }
    } else if (op == 1) {       // gX[b,i] = sum_o gO[b,o] conj(W[i,o])
        p.M = B; p.N = Ci; p.K = Co;
        p.A.s0 = (long long)Co * P; p.A.s1 = P; p.A.conj = 0;
        p.B.s0 = Mc; p.B.s1 = (long long)Co * Mc; p.B.conj = 1;
        p.o_sm = (long long)Ci * P; p.o_sn = P;
        for (int c = 0; c < nc; ++c) { p.A.base[c] = act + (long long)c * Mc; p.B.base[c] = w[c]; p.out[c] = out_act + (long long)c * Mc; }
    } else {                    // gW[i,o] = sum_b conj(X[b,i]) gO[b,o]
        p.M = Ci; p.N = Co; p.K = B;
        p.A.s0 = P; p.A.s1 = (long long)Ci * P; p.A.conj = 1;
        p.B.s0 = (long long)Co * P; p.B.s1 = P; p.B.conj = 0;
        p.o_sm = (long long)Co * Mc; p.o_sn = Mc;
        for (int c = 0; c < nc; ++c) { p.A.base[c] = act + (long long)c * Mc; p.B.base[c] = go + (long long)c * Mc; p.out[c] = out_w[c]; }
        if (B == 0) {
            if (accumulate || plan_only) return 1;
            for (int c = 0; c < nc; ++c)
                if (hipMemsetAsync(out_w[c], 0, sizeof(float2) * (size_t)Ci * Co * Mc, s) != hipSuccess) { set_error("memset failed"); return -5; }
            return 1;
        }
    }
    return 0;
}

static int mode_gemm(int op, const float2* act, const float2* const* w, const float2* go, float2* out_act,
                     float2* const* out_w, int B, int Ci, int Co, int nc, int Mc, hipStream_t s, int w_half = 0, int accumulate = 0) {
    ModeGemmParams p;
    const int rc = mode_gemm_params(p, op, act, w, go, out_act, out_w, B, Ci, Co, nc, Mc, s, w_half, accumulate);
    if (rc != 0) return rc < 0 ? rc : 0;
    return launch_mode_gemm(p, s);
}

// both GEMMs of a backward pass: gX = gO conj(W) (op 1) and gW (+)= conj(X) gO (op 2), one launch where the kernels allow
static int mode_backward(const float2* xtrunc, const float2* go, const float2* const* w, float2* gx_spec, float2* const* gw, int B, int Ci,
                         int Co, int nc, int Mc, hipStream_t s, int accumulate) {
    ModeGemmParams pa, pb;
    const int ra = mode_gemm_params(pa, 1, go, w, nullptr, gx_spec, nullptr, B, Ci, Co, nc, Mc, s, 0, 0);
    if (ra < 0) return ra;
    const int rb = mode_gemm_params(pb, 2, xtrunc, nullptr, go, nullptr, gw, B, Ci, Co, nc, Mc, s, 0, accumulate);
    if (rb < 0) return rb;
    if (ra == 0 && rb == 0) return launch_mode_gemm_pair(pa, pb, s);
    if (rb == 0) if (int rc = launch_mode_gemm(pb, s)) return rc;
    if (ra == 0) return launch_mode_gemm(pa, s);
    return 0;
}

}  // namespace uno

using namespace uno;


// A side stream per device for work that is independent of the caller's critical path (the weight-gradient GEMM of a
// backward call next to input-gradient GEMM + inverse DFT).  fork(): side waits for everything enqueued on `s` so far;
// join(): `s` waits for the side stream.  The mutex is held from fork to join, so concurrent callers on one device take
// turns (enqueueing is short).  Works under stream capture (event fork / join is the capture-safe pattern).
namespace {
struct SideStream {
    hipStream_t s = nullptr;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    std::mutex mu;
    bool ok = false;
};
SideStream* side_stream_of_current_device() {
    static std::mutex mu;
    static std::map<int, SideStream*> table;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> g(mu);
    auto it = table.find(dev);
    if (it != table.end()) return it->second->ok ? it->second : nullptr;
    SideStream* ss = new SideStream();
    ss->ok = hipStreamCreateWithFlags(&ss->s, hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&ss->fork_ev, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&ss->join_ev, hipEventDisableTiming) == hipSuccess;
    table[dev] = ss;
    return ss->ok ? ss : nullptr;
}
}  // namespace

extern "C" {

long long uno_dft2d_any_ws_bytes(int n_img, int H, int W, int m1, int m2) {
    (void)W;
    if (n_img <= 0 || H <= 0 || m2 <= 0) return 0;
    return (m1 > 40 || m2 > 48) ? 8LL * n_img * H * m2 : 0;
}

long long uno_spectral_conv2d_fwd_ws_bytes(int B, int Ci, int Co, int m1, int m2) {
    (void)Ci;
    return 8LL * B * Co * 2 * m1 * m2;
}

long long uno_spectral_conv2d_bwd_ws_bytes(int B, int Ci, int Co, int m1, int m2) {
    return 8LL * B * (Ci + Co) * 2 * m1 * m2;
}

int uno_dft2d_forward(const float* images, float* spec, int n_img, int H, int W, int m1, int m2, float scale,
                      int hermitian_cols, int mask_overlap, void* stream) {
    return dft2d(false, images, spec, n_img, H, W, m1, m2, scale, hermitian_cols, mask_overlap, (hipStream_t)stream);
}

int uno_dft2d_inverse(const float* spec, float* images, int n_img, int H, int W, int m1, int m2, float scale,
                      int hermitian_cols, int mask_overlap, void* stream) {
    return dft2d(true, spec, images, n_img, H, W, m1, m2, scale, hermitian_cols, mask_overlap, (hipStream_t)stream);
}

// K3 + up-sampled addend (dft2d_inv_add_kernel.h): where the form applies
int uno_dft2d_inverse_add_applies(int n_img, int H, int W, int m1, int m2, int Hs, int Ws) {
    if (n_img < 1 || H < 1 || W < 1 || m1 < 1 || m2 < 1 || Hs < 1 || Ws < 1 || m1 > H || m2 > W / 2 + 1 || m1 > 40 || m2 > 48) return 0;
    Dft2dParams p;
    p.n_img = n_img; p.H = H; p.W = W; p.m1 = m1; p.m2 = m2; p.herm = 1; p.mask = 1;
    p.sp_group = n_img; p.sp_stride = 0;
    p.add_Hs = Hs; p.add_Ws = Ws;
    if (dft2d_inv_plane_applies(p)) return 0;           // (many small images take the plane-batched kernels)
    return dft2d_inv_add_applies(p) ? 1 : 0;
}

int uno_dft2d_inverse_add(const float* spec, float* images, int n_img, int H, int W, int m1, int m2, float scale, int hermitian_cols,
                          int mask_overlap, const float* addend, int Hs, int Ws, const int* tile_p0, const float* row_op,
                          const int* col_v0, const float* col_op, void* stream) {
    const char* who = "uno_dft2d_inverse_add";
    if (n_img < 0) { set_error("%s: negative image count", who); return -1; }
    if (n_img > 0 && (!spec || !images || !addend || !tile_p0 || !row_op || !col_v0 || !col_op)) { set_error("%s: null pointer", who); return -1; }
    if (int rc = check_modes2d(who, H, W, H, W, m1, m2)) return rc;
    if (Hs < 1 || Ws < 12 || (long long)Hs * Ws * 4 > 0x7fffffffLL) { set_error("%s: bad addend grid %dx%d", who, Hs, Ws); return -1; }
    if (n_img == 0) return 0;
    if (!uno_dft2d_inverse_add_applies(n_img, H, W, m1, m2, Hs, Ws)) {
        set_error("%s: the fused form does not apply to %d images of %dx%d, modes (%d, %d) (query uno_dft2d_inverse_add_applies)", who, n_img, H, W, m1, m2);
        return -3;
    }
    Dft2dParams p;
    p.in = spec; p.out = images; p.n_img = n_img; p.H = H; p.W = W; p.m1 = m1; p.m2 = m2;
    p.scale = scale; p.herm = hermitian_cols ? 1 : 0; p.mask = mask_overlap ? 1 : 0;
    p.sp_group = n_img; p.sp_stride = 0;
    p.twH = twiddle_table(H);
    p.twW = twiddle_table(W);
    if (!p.twH || !p.twW) return -6;
    p.add_src = addend; p.add_Hs = Hs; p.add_Ws = Ws; p.add_p0 = tile_p0; p.add_rowop = row_op; p.add_v0 = col_v0; p.add_colop = col_op;
#ifdef UNO_K3A_DEV       // development builds: knock-out switches of the kernel (tools/dev/k3a_time.py), see dft2d_inv_add_kernel.h
    { static const int dev_exp = getenv("UNO_K3A_STAGGER") ? atoi(getenv("UNO_K3A_STAGGER")) : 0; p.exp = dev_exp; }
#endif
    return launch_dft2d_inv_add(p, (hipStream_t)stream);
}

// K1 + down-sampled image (dft2d_fwd_fd_kernel.h): where the form applies
static void fwd_resample_shape(Dft2dParams& p, int n_img, int H, int W, int m1, int m2, int Ho, int Wo, int KW) {
    p.n_img = n_img; p.H = H; p.W = W; p.m1 = m1; p.m2 = m2;
    p.fd_Ho = Ho; p.fd_Wo = Wo; p.fd_KW = KW;
}

int uno_dft2d_forward_resample_applies(int n_img, int H, int W, int m1, int m2, int Ho, int Wo, int KW) {
    if (n_img < 1 || H < 1 || W < 1 || m1 < 1 || m2 < 1 || Ho < 1 || Wo < 1 || KW < 1 || m1 > H || m2 > W / 2 + 1 || m1 > 40 || m2 > 48) return 0;
    Dft2dParams p;
    fwd_resample_shape(p, n_img, H, W, m1, m2, Ho, Wo, KW);
    return dft2d_fwd_fd_applies(p) ? 1 : 0;
}

int uno_dft2d_forward_resample(const float* images, float* spec, int n_img, int H, int W, int m1, int m2, float scale, int hermitian_cols,
                               int mask_overlap, int group, int stride, int offset, float* resampled, int Ho, int Wo, const int* col_start,
                               const float* col_wt, int KW, const int* row_tiles, const float* row_op, void* stream) {
    const char* who = "uno_dft2d_forward_resample";
    if (n_img < 0) { set_error("%s: negative image count", who); return -1; }
    if (n_img > 0 && (!images || !spec || !resampled || !col_start || !col_wt || !row_tiles || !row_op)) { set_error("%s: null pointer", who); return -1; }
    if (int rc = check_modes2d(who, H, W, H, W, m1, m2)) return rc;
    if (Ho < 1 || Wo < 1 || KW < 1) { set_error("%s: bad output grid %dx%d or band (%d taps)", who, Ho, Wo, KW); return -1; }
    if (n_img == 0) return 0;
    if (group <= 0) { group = n_img; stride = 0; offset = 0; }          // plain layout: spectrum i of image i
    else if (offset < 0 || stride < offset + group || n_img % group) {
        set_error("%s: bad spectrum grouping (group %d, stride %d, offset %d, images %d)", who, group, stride, offset, n_img);
        return -1;
    }
    if (!uno_dft2d_forward_resample_applies(n_img, H, W, m1, m2, Ho, Wo, KW)) {
        set_error("%s: the fused form does not apply to %d images of %dx%d -> %dx%d, modes (%d, %d), %d taps (query uno_dft2d_forward_resample_applies)",
                  who, n_img, H, W, Ho, Wo, m1, m2, KW);
        return -3;
    }
    Dft2dParams p;
    fwd_resample_shape(p, n_img, H, W, m1, m2, Ho, Wo, KW);
    p.in = images; p.out = spec; p.scale = scale; p.herm = hermitian_cols ? 1 : 0; p.mask = mask_overlap ? 1 : 0;
    p.sp_group = group; p.sp_stride = stride; p.sp_offset = offset;
    p.twH = twiddle_table(H);
    p.twW = twiddle_table(W);
    if (!p.twH || !p.twW) return -6;
    p.fd_out = resampled; p.fd_startW = col_start; p.fd_wtW = col_wt; p.fd_tiles = row_tiles; p.fd_rowop = row_op;
    return launch_dft2d_fwd_fd(p, (hipStream_t)stream);
}

// the truncation to (m1, m2) modes of spectra truncated to (M1, M2): a copy of the corner blocks (spectrum_crop.hip)
int uno_spectrum_crop(const float* src, float* dst, int n_img, int M1, int M2, int m1, int m2, int src_group, int src_stride, int src_offset,
                      int dst_group, int dst_stride, int dst_offset, void* stream) {
    const char* who = "uno_spectrum_crop";
    if (n_img < 0) { set_error("%s: negative image count", who); return -1; }
    if (m1 < 1 || m2 < 1 || m1 > M1 || m2 > M2 || (long long)M1 * M2 > 0x7fffffffLL / 4) {
        set_error("%s: bad mode counts (%d, %d) -> (%d, %d) (need 1 <= m1 <= M1, 1 <= m2 <= M2)", who, M1, M2, m1, m2);
        return -1;
    }
    if (n_img == 0) return 0;
    if (!src || !dst) { set_error("%s: null pointer", who); return -1; }
    if (src == dst) { set_error("%s: dst must not alias src", who); return -1; }
    if (src_group <= 0) { src_group = n_img; src_stride = 0; src_offset = 0; }          // plain layout: spectrum i of image i
    else if (src_offset < 0 || src_stride < src_offset + src_group || n_img % src_group) {
        set_error("%s: bad source grouping (group %d, stride %d, offset %d, images %d)", who, src_group, src_stride, src_offset, n_img);
        return -1;
    }
    if (dst_group <= 0) { dst_group = n_img; dst_stride = 0; dst_offset = 0; }
    else if (dst_offset < 0 || dst_stride < dst_offset + dst_group || n_img % dst_group) {
        set_error("%s: bad destination grouping (group %d, stride %d, offset %d, images %d)", who, dst_group, dst_stride, dst_offset, n_img);
        return -1;
    }
    return launch_spectrum_crop(src, dst, n_img, M1, M2, m1, m2, src_group, src_stride, src_offset, dst_group, dst_stride, dst_offset,
                                (hipStream_t)stream);
}

int uno_dft2d_forward_bf16(const void* images, float* spec, int n_img, int H, int W, int m1, int m2, float scale,
                           int hermitian_cols, int mask_overlap, void* stream) {
    return dft2d(false, static_cast<const float*>(images), spec, n_img, H, W, m1, m2, scale, hermitian_cols, mask_overlap,
                 (hipStream_t)stream, 0, 0, 0, 1);
}

int uno_dft2d_inverse_bf16(const float* spec, void* images, int n_img, int H, int W, int m1, int m2, float scale,
                           int hermitian_cols, int mask_overlap, void* stream) {
    return dft2d(true, spec, static_cast<float*>(images), n_img, H, W, m1, m2, scale, hermitian_cols, mask_overlap,
                 (hipStream_t)stream, 0, 0, 0, 1);
}

int uno_dft2d_forward_grouped(const float* images, float* spec, int n_img, int H, int W, int m1, int m2, float scale,
                              int hermitian_cols, int mask_overlap, int group, int stride, int offset, void* stream) {
    if (group < 1) { set_error("uno_dft2d_forward_grouped: group must be positive"); return -1; }
    return dft2d(false, images, spec, n_img, H, W, m1, m2, scale, hermitian_cols, mask_overlap, (hipStream_t)stream, group, stride, offset);
}

int uno_dft2d_forward_grouped_bf16(const void* images, float* spec, int n_img, int H, int W, int m1, int m2, float scale,
                                   int hermitian_cols, int mask_overlap, int group, int stride, int offset, void* stream) {
    if (group < 1) { set_error("uno_dft2d_forward_grouped_bf16: group must be positive"); return -1; }
    return dft2d(false, static_cast<const float*>(images), spec, n_img, H, W, m1, m2, scale, hermitian_cols, mask_overlap,
                 (hipStream_t)stream, group, stride, offset, 1);
}

int uno_dft2d_inverse_grouped_bf16(const float* spec, void* images, int n_img, int H, int W, int m1, int m2, float scale,
                                   int hermitian_cols, int mask_overlap, int group, int stride, int offset, void* stream) {
    if (group < 1) { set_error("uno_dft2d_inverse_grouped_bf16: group must be positive"); return -1; }
    return dft2d(true, spec, static_cast<float*>(images), n_img, H, W, m1, m2, scale, hermitian_cols, mask_overlap,
                 (hipStream_t)stream, group, stride, offset, 1);
}

int uno_dft2d_inverse_grouped(const float* spec, float* images, int n_img, int H, int W, int m1, int m2, float scale,
                              int hermitian_cols, int mask_overlap, int group, int stride, int offset, void* stream) {
    if (group < 1) { set_error("uno_dft2d_inverse_grouped: group must be positive"); return -1; }
    return dft2d(true, spec, images, n_img, H, W, m1, m2, scale, hermitian_cols, mask_overlap, (hipStream_t)stream, group, stride, offset);
}

static int mode_mix_impl(const float* in, const float* const* w, float* out, int op, int B, int Ci, int Co, int ncorner,
                         int modes_per_corner, void* stream, int w_half) {
    if (!w || (B > 0 && (!in || !out))) { set_error("uno_mode_mix: null pointer"); return -1; }
    if (op != 0 && op != 1) { set_error("uno_mode_mix: op must be 0 or 1"); return -1; }
    if (ncorner < 1 || ncorner > 4) { set_error("uno_mode_mix: ncorner=%d out of range", ncorner); return -1; }
    for (int c = 0; c < ncorner; ++c)
        if (!w[c]) { set_error("uno_mode_mix: null weight pointer %d", c); return -1; }
    return mode_gemm(op, reinterpret_cast<const float2*>(in), reinterpret_cast<const float2* const*>(w), nullptr,
                     reinterpret_cast<float2*>(out), nullptr, B, Ci, Co, ncorner, modes_per_corner, (hipStream_t)stream, w_half);
}

int uno_mode_mix(const float* in, const float* const* w, float* out, int op, int B, int Ci, int Co, int ncorner,
                 int modes_per_corner, void* stream) {
    return mode_mix_impl(in, w, out, op, B, Ci, Co, ncorner, modes_per_corner, stream, 0);
}

int uno_mode_mix_f16w(const float* in, const void* const* w, float* out, int op, int B, int Ci, int Co, int ncorner,
                      int modes_per_corner, void* stream) {
    return mode_mix_impl(in, reinterpret_cast<const float* const*>(w), out, op, B, Ci, Co, ncorner, modes_per_corner, stream, 1);
}

static int mode_wgrad_impl(const float* xtrunc, const float* go, float* const* gw, int B, int Ci, int Co, int ncorner,
                           int modes_per_corner, int accumulate, void* stream) {
    if (!gw || (B > 0 && (!xtrunc || !go))) { set_error("uno_mode_wgrad: null pointer"); return -1; }
    if (ncorner < 1 || ncorner > 4) { set_error("uno_mode_wgrad: ncorner=%d out of range", ncorner); return -1; }
    for (int c = 0; c < ncorner; ++c)
        if (!gw[c]) { set_error("uno_mode_wgrad: null output pointer %d", c); return -1; }
    return mode_gemm(2, reinterpret_cast<const float2*>(xtrunc), nullptr, reinterpret_cast<const float2*>(go), nullptr,
                     reinterpret_cast<float2* const*>(gw), B, Ci, Co, ncorner, modes_per_corner, (hipStream_t)stream, 0, accumulate);
}

int uno_mode_wgrad(const float* xtrunc, const float* go, float* const* gw, int B, int Ci, int Co, int ncorner,
                   int modes_per_corner, void* stream) {
    return mode_wgrad_impl(xtrunc, go, gw, B, Ci, Co, ncorner, modes_per_corner, 0, stream);
}

int uno_mode_backward(const float* xtrunc, const float* go, const float* const* w, float* gx_spec, float* const* gw, int B, int Ci, int Co,
                      int ncorner, int modes_per_corner, int accumulate, void* stream) {
    if (!w || !gw || (B > 0 && (!xtrunc || !go || !gx_spec))) { set_error("uno_mode_backward: null pointer"); return -1; }
    if (ncorner < 1 || ncorner > 4) { set_error("uno_mode_backward: ncorner=%d out of range", ncorner); return -1; }
    for (int c = 0; c < ncorner; ++c)
        if (!w[c] || !gw[c]) { set_error("uno_mode_backward: null weight / gradient pointer %d", c); return -1; }
    return mode_backward(reinterpret_cast<const float2*>(xtrunc), reinterpret_cast<const float2*>(go), reinterpret_cast<const float2* const*>(w),
                         reinterpret_cast<float2*>(gx_spec), reinterpret_cast<float2* const*>(gw), B, Ci, Co, ncorner, modes_per_corner,
                         (hipStream_t)stream, accumulate);
}

int uno_mode_wgrad_acc(const float* xtrunc, const float* go, float* const* gw, int B, int Ci, int Co, int ncorner,
                       int modes_per_corner, int accumulate, void* stream) {
    return mode_wgrad_impl(xtrunc, go, gw, B, Ci, Co, ncorner, modes_per_corner, accumulate, stream);
}

// The operand descriptions of a call without its buffers: mode_gemm_params on placeholder addresses (the plan depends on sizes and strides
// only; nothing is read through them), with the real call's size checks and error text.  rc as mode_gemm_params.
static int mode_plan_params(ModeGemmParams& p, int op, int B, int Ci, int Co, int ncorner, int modes_per_corner, int w_half, int accumulate) {
    static float2 placeholder[1];
    const float2* const w[4] = {placeholder, placeholder, placeholder, placeholder};
    float2* const ow[4] = {placeholder, placeholder, placeholder, placeholder};
    if (ncorner < 1 || ncorner > 4) { set_error("%s: ncorner=%d out of range", op == 2 ? "uno_mode_wgrad" : "uno_mode_mix", ncorner); return -1; }
    return mode_gemm_params(p, op, placeholder, w, placeholder, placeholder, ow, B, Ci, Co, ncorner, modes_per_corner, nullptr, w_half, accumulate, true);
}

static void mode_plan_ints(const ModeGemmParams& p, const ModeGemmPlan& pl, int* out) {
    const bool lds = pl.family == 1, blocks = pl.family == 2;
    const int v[UNO_MODE_GEMM_PLAN_INTS] = {pl.family, p.M, p.N, p.K, lds ? pl.qc : 0, lds ? pl.pipe : 0, blocks ? pl.variant : -1, blocks ? pl.KS : 0,
                                            blocks ? pl.adjacent : 0, pl.refused, pl.half, pl.acc, pl.grid[0], pl.grid[1], pl.grid[2], pl.lds};
    for (int i = 0; i < UNO_MODE_GEMM_PLAN_INTS; ++i) out[i] = v[i];
}

int uno_mode_gemm_plan(int op, int B, int Ci, int Co, int ncorner, int modes_per_corner, int w_half, int accumulate, int* plan) {
    if (!plan) { set_error("uno_mode_gemm_plan: null pointer"); return -1; }
    if (op < 0 || op > 2) { set_error("uno_mode_gemm_plan: op must be 0, 1 or 2"); return -1; }
    for (int i = 0; i < UNO_MODE_GEMM_PLAN_INTS; ++i) plan[i] = 0;
    ModeGemmParams p;
    const int rc = mode_plan_params(p, op, B, Ci, Co, ncorner, modes_per_corner, w_half, accumulate);
    if (rc != 0) return rc < 0 ? rc : 0;           // 1: nothing to launch (family 0)
    ModeGemmPlan pl;
    if (int e = mode_gemm_plan(p, pl)) return e;
    mode_plan_ints(p, pl, plan);
    return 0;
}

int uno_mode_backward_plan(int B, int Ci, int Co, int ncorner, int modes_per_corner, int accumulate, int* plan) {
    if (!plan) { set_error("uno_mode_backward_plan: null pointer"); return -1; }
    for (int i = 0; i < UNO_MODE_BACKWARD_PLAN_INTS; ++i) plan[i] = 0;
    // the steps of mode_backward, planned instead of launched
    ModeGemmParams pa, pb;
    const int ra = mode_plan_params(pa, 1, B, Ci, Co, ncorner, modes_per_corner, 0, 0);
    if (ra < 0) return ra;
    const int rb = mode_plan_params(pb, 2, B, Ci, Co, ncorner, modes_per_corner, 0, accumulate);
    if (rb < 0) return rb;
    ModeGemmPairPlan pp = {};
    if (ra == 0 && rb == 0) {
        if (int e = mode_gemm_pair_plan(pa, pb, pp)) return e;
    } else {
        if (rb == 0) if (int e = mode_gemm_plan(pb, pp.b)) return e;
        if (ra == 0) if (int e = mode_gemm_plan(pa, pp.a)) return e;
    }
    plan[0] = pp.paired; plan[1] = pp.Ga; plan[2] = pp.grid; plan[3] = pp.lds;
    if (ra == 0) mode_plan_ints(pa, pp.a, plan + 4);
    if (rb == 0) mode_plan_ints(pb, pp.b, plan + 4 + UNO_MODE_GEMM_PLAN_INTS);
    return 0;
}

// `group` > 0: grouped placement of the corner-major side (CdftParams::sp_group); the callers have validated it
static int cdft_axis(const float* in, float* out, int inverse, int n_img, int H, int m1, int m2, int m3, float scale, int mask_overlap,
                     int group, int stride, int offset, void* stream) {
    if (n_img < 0 || H < 1 || m1 < 1 || m1 > H || m2 < 1 || m3 < 1) {
        set_error("uno_cdft_axis: bad sizes n_img=%d H=%d modes=(%d,%d,%d)", n_img, H, m1, m2, m3);
        return -1;
    }
    if (n_img == 0) return 0;
    if (!in || !out) { set_error("uno_cdft_axis: null pointer"); return -1; }
    CdftParams p;
    p.in = in; p.out = out; p.n_img = n_img; p.H = H; p.C = 2 * m2 * m3; p.m1 = m1; p.m2 = m2; p.m3 = m3;
    p.scale = scale; p.mask = mask_overlap ? 1 : 0;
    if (group > 0) { p.sp_group = group; p.sp_stride = stride; p.sp_offset = offset; }
    p.tw = twiddle_table(H);
    if (!p.tw) return -6;
    if (m1 > 40) return launch_cdft_generic(p, inverse != 0, (hipStream_t)stream);
    return launch_cdft(p, inverse != 0, (hipStream_t)stream);
}

int uno_cdft_axis(const float* in, float* out, int inverse, int n_img, int H, int m1, int m2, int m3, float scale,
                  int mask_overlap, void* stream) {
    return cdft_axis(in, out, inverse, n_img, H, m1, m2, m3, scale, mask_overlap, 0, 0, 0, stream);
}

// ---- FFT crop / resample of pointwise_op_3D (reference integral_operators.py:448-463) as pruned transforms with explicit
// frequency tables.  Along a complex axis of length N resampled to M the reference keeps the spectrum INDICES
// r in ([0, M/2) u [N - M/2, N)) n [0, min(N, M)) and irfftn reads index r as frequency r of a length-M transform (its trimming /
// zero-padding happens at the end of the axis): forward frequency f_in[j] = r_j on N points, inverse frequency f_out[j] = r_j on
// M points - the binding builds the tables, so this entry point is the general "pruned DFT - pruned inverse DFT" pair.
long long uno_fft_resample3d_ws_bytes(int n_vol, int D1, int M1, int J1, int J2, int m3) {
    const long long C = (long long)J2 * m3;
    return 8LL * n_vol * ((long long)D1 * C + (long long)M1 * C + (long long)J1 * C);
}

static int fft_resample3d_impl(const float* x, float* y, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                               int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3,
                               float scale, int herm_in, int herm_out, int accumulate, float* act_out, void* stream) {
    const char* who = "uno_fft_resample3d";
    if (n_vol < 0 || D1 < 1 || D2 < 1 || D3 < 1 || M1 < 1 || M2 < 1 || M3 < 1) { set_error("%s: bad sizes", who); return -1; }
    if (J1 < 2 || (J1 & 1) || J2 < 2 || (J2 & 1) || J1 > 80 || J2 > 48 || m3 < 1 || m3 > D3 / 2 + 1 || m3 > M3 / 2 + 1) {
        set_error("%s: row counts must be even (J1=%d <= 80, J2=%d <= 48) and 1 <= modes3=%d <= n/2+1", who, J1, J2, m3);
        return -1;
    }
    if (n_vol == 0) return 0;
    if (!x || !y || !ws || !f1_in || !f1_out || !f2_in || !f2_out) { set_error("%s: null pointer", who); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const long long C = (long long)J2 * m3;
    float* Z1 = static_cast<float*>(ws);                          // (n_vol * D1, J2, m3) c64
    float* Z2 = Z1 + 2LL * n_vol * D1 * C;                        // (n_vol * M1, J2, m3) c64
    float* S = Z2 + 2LL * n_vol * M1 * C;                         // (n_vol, 4, J1/2, J2/2, m3) c64
    Dft2dParams p;
    p.n_img = n_vol * D1; p.H = D2; p.W = D3; p.m1 = J2 / 2; p.m2 = m3; p.herm = herm_in ? 1 : 0;
    p.sp_group = p.n_img; p.sp_stride = 0;
    p.in = x; p.out = Z1; p.rowfreq = f2_in;
    p.twH = twiddle_table(D2); p.twW = twiddle_table(D3);
    if (!p.twH || !p.twW) return -6;
    if (!dft2d_fwd_plane_applies(p)) { set_error("%s: input planes %d x %d (%d of them) are outside the plane-batched kernels' range", who, D2, D3, p.n_img); return -2; }
    if (int rc = launch_dft2d_fwd_plane(p, s)) return rc;
    CdftParams c;
    c.n_img = n_vol; c.C = (int)C; c.m1 = J1 / 2; c.m2 = J2 / 2; c.m3 = m3;
    c.in = Z1; c.out = S; c.H = D1; c.rowfreq = f1_in; c.tw = twiddle_table(D1);
    if (!c.tw) return -6;
    if (int rc = launch_cdft(c, false, s)) return rc;
    c.in = S; c.out = Z2; c.H = M1; c.rowfreq = f1_out; c.tw = twiddle_table(M1);
    if (!c.tw) return -6;
    if (int rc = launch_cdft(c, true, s)) return rc;
    p.n_img = n_vol * M1; p.H = M2; p.W = M3; p.scale = scale; p.herm = herm_out ? 1 : 0;
    p.sp_group = p.n_img;
    p.in = Z2; p.out = y; p.rowfreq = f2_out;
    p.twH = twiddle_table(M2); p.twW = twiddle_table(M3);
    if (!p.twH || !p.twW) return -6;
    if (!dft2d_inv_plane_applies(p)) { set_error("%s: output planes %d x %d (%d of them) are outside the plane-batched kernels' range", who, M2, M3, p.n_img); return -2; }
    p.accumulate = accumulate ? 1 : 0; p.act_out = act_out;
    return launch_dft2d_inv_plane(p, s);
}

int uno_fft_resample3d(const float* x, float* y, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                       int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3,
                       float scale, int herm_in, int herm_out, void* stream) {
    return fft_resample3d_impl(x, y, ws, n_vol, D1, D2, D3, M1, M2, M3, J1, f1_in, f1_out, J2, f2_in, f2_out, m3, scale, herm_in, herm_out,
                               0, nullptr, stream);
}

int uno_fft_resample3d_acc(const float* x, float* y, float* y_act, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                           int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3,
                           float scale, int herm_in, int herm_out, void* stream) {
    return fft_resample3d_impl(x, y, ws, n_vol, D1, D2, D3, M1, M2, M3, J1, f1_in, f1_out, J2, f2_in, f2_out, m3, scale, herm_in, herm_out,
                               1, y_act, stream);
}

// ---- the same operator on the two plane-at-a-time kernel families (resample3d_planes.h): any row counts, 1 <= modes3 <= n/2 + 1
struct Resample3dFamily {
    int max_lead, max_last, max_rows;       // largest length of the two leading axes, of the last axis, largest kept-row count (from 2, 2, 1)
    int vol_bits;                           // n_vol < 2^vol_bits: n_vol x max_lead fits an int
    decltype(&resample3d_any_lds_bytes) lds_bytes;
    decltype(&launch_resample3d_any) launch;
};
// resample3d_any.hip: every sum on plain FMA; resample3d_wide.hip: the long-axis stages on the MFMA
static const Resample3dFamily RESAMPLE3D_ANY = {128, 128, 128, 24, resample3d_any_lds_bytes, launch_resample3d_any};
static const Resample3dFamily RESAMPLE3D_WIDE = {256, 64, 256, 23, resample3d_wide_lds_bytes, launch_resample3d_wide};

static long long resample3d_planes_ws_bytes(int n_vol, int D1, int M1, int J2, int m3) {       // the J1 spectrum rows live in LDS only
    return 8LL * n_vol * ((long long)D1 + M1) * J2 * m3;
}
long long uno_fft_resample3d_any_ws_bytes(int n_vol, int D1, int M1, int J1, int J2, int m3) { (void)J1; return resample3d_planes_ws_bytes(n_vol, D1, M1, J2, m3); }
long long uno_fft_resample3d_wide_ws_bytes(int n_vol, int D1, int M1, int J1, int J2, int m3) { (void)J1; return resample3d_planes_ws_bytes(n_vol, D1, M1, J2, m3); }

static int resample3d_planes_impl(const Resample3dFamily& fam, const char* who, const float* x, float* y, float* y_act, int accumulate, void* ws,
                                  int n_vol, int D1, int D2, int D3, int M1, int M2, int M3, int J1, const int* f1_in, const int* f1_out, int J2,
                                  const int* f2_in, const int* f2_out, int m3, float scale, int herm_in, int herm_out, void* stream) {
    const int lead[4] = {D1, D2, M1, M2}, last[2] = {D3, M3};
    bool ok = true;
    for (int d : lead) ok = ok && d >= 2 && d <= fam.max_lead;
    for (int d : last) ok = ok && d >= 2 && d <= fam.max_last;
    if (!ok) {
        if (fam.max_lead == fam.max_last)
            set_error("%s: grid (%d,%d,%d) -> (%d,%d,%d): every axis length must be in 2 ... %d", who, D1, D2, D3, M1, M2, M3, fam.max_lead);
        else
            set_error("%s: grid (%d,%d,%d) -> (%d,%d,%d): the two leading axis lengths must be in 2 ... %d and the last in 2 ... %d", who, D1, D2, D3,
                      M1, M2, M3, fam.max_lead, fam.max_last);
        return -1;
    }
    if (J1 < 1 || J1 > fam.max_rows || J2 < 1 || J2 > fam.max_rows) {
        set_error("%s: kept-row counts J1=%d, J2=%d must be in 1 ... %d", who, J1, J2, fam.max_rows);
        return -1;
    }
    if (m3 < 1 || m3 > D3 / 2 + 1 || m3 > M3 / 2 + 1) {
        set_error("%s: need 1 <= modes3=%d <= n/2+1 on the last axis %d -> %d", who, m3, D3, M3);
        return -1;
    }
    if (n_vol < 0 || (n_vol >> fam.vol_bits)) { set_error("%s: bad volume count %d (0 ... 2^%d - 1)", who, n_vol, fam.vol_bits); return -1; }
    size_t lds[3];
    fam.lds_bytes(D1, D2, D3, M1, M2, M3, J1, J2, m3, lds);       // (never beyond the limit on the any-grid family's axes: 142 KB at most)
    if (lds[0] > 160 * 1024 || lds[1] > 160 * 1024 || lds[2] > 160 * 1024) {
        set_error("%s: grid (%d,%d,%d) -> (%d,%d,%d) with J1=%d, J2=%d, modes3=%d needs %zu / %zu / %zu bytes of LDS (forward plane / leading "
                  "axis / inverse plane kernel): the limit is 163840 per workgroup", who, D1, D2, D3, M1, M2, M3, J1, J2, m3, lds[0], lds[1], lds[2]);
        return -2;
    }
    if (accumulate) {       // the kernels read x while they write y, and read y back before they write y_act
        if (y_act && y_act == y) { set_error("%s: y_act must not alias y", who); return -1; }
        if (x && x == y) { set_error("%s: x must not alias y", who); return -1; }
        if (x && x == y_act) { set_error("%s: x must not alias y_act", who); return -1; }
    }
    if (n_vol == 0) return 0;
    if (!x || !y || !ws || !f1_in || !f1_out || !f2_in || !f2_out) { set_error("%s: null pointer", who); return -1; }
    return fam.launch(x, y, y_act, accumulate, ws, n_vol, D1, D2, D3, M1, M2, M3, J1, f1_in, f1_out, J2, f2_in, f2_out, m3, scale, herm_in, herm_out,
                      (hipStream_t)stream);
}

int uno_fft_resample3d_any(const float* x, float* y, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                           int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3,
                           float scale, int herm_in, int herm_out, void* stream) {
    return resample3d_planes_impl(RESAMPLE3D_ANY, "uno_fft_resample3d_any", x, y, nullptr, 0, ws, n_vol, D1, D2, D3, M1, M2, M3, J1, f1_in, f1_out, J2,
                                  f2_in, f2_out, m3, scale, herm_in, herm_out, stream);
}

int uno_fft_resample3d_any_acc(const float* x, float* y, float* y_act, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                               int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3,
                               float scale, int herm_in, int herm_out, void* stream) {
    return resample3d_planes_impl(RESAMPLE3D_ANY, "uno_fft_resample3d_any_acc", x, y, y_act, 1, ws, n_vol, D1, D2, D3, M1, M2, M3, J1, f1_in, f1_out,
                                  J2, f2_in, f2_out, m3, scale, herm_in, herm_out, stream);
}

int uno_fft_resample3d_wide(const float* x, float* y, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                            int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3,
                            float scale, int herm_in, int herm_out, void* stream) {
    return resample3d_planes_impl(RESAMPLE3D_WIDE, "uno_fft_resample3d_wide", x, y, nullptr, 0, ws, n_vol, D1, D2, D3, M1, M2, M3, J1, f1_in, f1_out,
                                  J2, f2_in, f2_out, m3, scale, herm_in, herm_out, stream);
}

int uno_fft_resample3d_wide_acc(const float* x, float* y, float* y_act, void* ws, int n_vol, int D1, int D2, int D3, int M1, int M2, int M3,
                                int J1, const int* f1_in, const int* f1_out, int J2, const int* f2_in, const int* f2_out, int m3,
                                float scale, int herm_in, int herm_out, void* stream) {
    return resample3d_planes_impl(RESAMPLE3D_WIDE, "uno_fft_resample3d_wide_acc", x, y, y_act, 1, ws, n_vol, D1, D2, D3, M1, M2, M3, J1, f1_in, f1_out,
                                  J2, f2_in, f2_out, m3, scale, herm_in, herm_out, stream);
}

static int check_modes3d(const char* who, int H, int W, int T, int Ho, int Wo, int To, int m1, int m2, int m3) {
    if (H < 1 || W < 1 || T < 1 || Ho < 1 || Wo < 1 || To < 1) { set_error("%s: empty grid", who); return -1; }
    if (m1 < 1 || m1 > H || m1 > Ho) { set_error("%s: modes1=%d incompatible with axis %d -> %d", who, m1, H, Ho); return -1; }
    if (m2 < 1 || m2 > W || m2 > Wo) { set_error("%s: modes2=%d incompatible with axis %d -> %d", who, m2, W, Wo); return -1; }
    if (m3 < 1 || m3 > T / 2 + 1 || m3 > To / 2 + 1) {
        set_error("%s: modes3=%d incompatible with axis %d -> %d (need modes3 <= n/2+1)", who, m3, T, To);
        return -1;
    }
    return 0;
}

// volumes (n_vol, D1, D2, D3) -> corner-major truncated spectra (n_vol, 4, m1, m2, m3); `adjoint` = the Hermitian-weighted, masked form
// the backward pass applies to the output gradient.  One workgroup per volume where that fits (K1v), else plane by plane (K1p) into
// the workspace Z (n_vol * D1, 2 m2, m3) c64 and the leading axis from there (K5).  `group` > 0 places spectrum i at volume
// (i / group) * stride + offset + i % group of `spec` (validated by the callers); the volume side and Z keep their addressing.
// n_decide > 0: the volume count the choice between the kernel families is made for (the two-source layer calls pass the
// concatenation's, so that each source runs the kernels the one-source call on the concatenation runs: the same bits per volume).
static int fwd_transform3d(const float* x, float* spec, float* Z, int n_vol, int D1, int D2, int D3, int m1, int m2, int m3, float scale,
                           int adjoint, hipStream_t s, int group = 0, int stride = 0, int offset = 0, int n_decide = 0) {
    if (vol3d_fwd_applies(n_decide > 0 ? n_decide : n_vol, D1, D2, D3, m1, m2, m3)) {
        Vol3dParams v;
        v.in = x; v.out = spec; v.n_vol = n_vol; v.D1 = D1; v.D2 = D2; v.D3 = D3; v.m1 = m1; v.m2 = m2; v.m3 = m3;
        v.scale = scale; v.herm = adjoint;
        if (group > 0) { v.sp_group = group; v.sp_stride = stride; v.sp_offset = offset; }
        v.tw1 = twiddle_table(2 * D1); v.tw2 = twiddle_table(2 * D2); v.tw3 = twiddle_table(D3);
        if (!v.tw1 || !v.tw2 || !v.tw3) return -6;
        return launch_dft3d_fwd_volume(v, s);
    }
    if (int rc = dft2d(false, x, Z, n_vol * D1, D2, D3, m2, m3, scale, adjoint, adjoint, s, 0, 0, 0, 0, n_decide * D1)) return rc;
    return cdft_axis(Z, spec, 0, n_vol, D1, m1, m2, m3, 1.0f, adjoint, group, stride, offset, (void*)s);
}

// the inverse: corner-major spectra -> volumes; `weighted` = Hermitian weights + later-wins masks (the forward pass's irfftn)
static int inv_transform3d(const float* spec, float* y, float* Z, int n_vol, int D1, int D2, int D3, int m1, int m2, int m3, float scale,
                           int weighted, hipStream_t s, int group = 0, int stride = 0, int offset = 0, int n_decide = 0) {
    if (vol3d_inv_applies(n_decide > 0 ? n_decide : n_vol, D1, D2, D3, m1, m2, m3)) {
        Vol3dParams v;
        v.in = spec; v.out = y; v.n_vol = n_vol; v.D1 = D1; v.D2 = D2; v.D3 = D3; v.m1 = m1; v.m2 = m2; v.m3 = m3;
        v.scale = scale; v.herm = weighted;
        if (group > 0) { v.sp_group = group; v.sp_stride = stride; v.sp_offset = offset; }
        v.tw1 = twiddle_table(2 * D1); v.tw2 = twiddle_table(2 * D2); v.tw3 = twiddle_table(D3);
        if (!v.tw1 || !v.tw2 || !v.tw3) return -6;
        return launch_dft3d_inv_volume(v, s);
    }
    if (int rc = cdft_axis(spec, Z, 1, n_vol, D1, m1, m2, m3, 1.0f, weighted, group, stride, offset, (void*)s)) return rc;
    return dft2d(true, Z, y, n_vol * D1, D2, D3, m2, m3, scale, weighted, weighted, s, 0, 0, 0, 0, n_decide * D1);
}

long long uno_spectral_conv3d_fwd_ws_bytes(int B, int Ci, int Co, int H, int Ho, int m1, int m2, int m3) {
    const long long C = 2LL * m2 * m3;
    return 8LL * B * ((long long)Ci * H * C + (long long)Co * Ho * C + 4LL * Co * m1 * m2 * m3);
}

long long uno_spectral_conv3d_bwd_ws_bytes(int B, int Ci, int Co, int H, int Ho, int m1, int m2, int m3) {
    const long long C = 2LL * m2 * m3;
    return 8LL * B * ((long long)Ci * H * C + (long long)Co * Ho * C + 4LL * (Ci + Co) * m1 * m2 * m3);
}

int uno_spectral_conv3d_forward(const float* x, const float* const* w, float* y, float* xtrunc, void* ws, int B, int Ci,
                                int Co, int H, int W, int T, int Ho, int Wo, int To, int m1, int m2, int m3, void* stream) {
    const char* who = "uno_spectral_conv3d_forward";
    if (B < 0 || Ci < 1 || Co < 1) { set_error("%s: bad sizes B=%d Ci=%d Co=%d", who, B, Ci, Co); return -1; }
    if (int rc = check_modes3d(who, H, W, T, Ho, Wo, To, m1, m2, m3)) return rc;
    if (B == 0) return 0;
    if (!x || !w || !y || !xtrunc || !ws) { set_error("%s: null pointer", who); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const long long C = 2LL * m2 * m3, Mc = (long long)m1 * m2 * m3;
    float* Z1 = static_cast<float*>(ws);                         // (B*Ci*H, 2 m2, m3) c64
    float* Z2 = Z1 + 2LL * B * Ci * H * C;                        // (B*Co*Ho, 2 m2, m3) c64
    float* O5 = Z2 + 2LL * B * Co * Ho * C;                       // (B, Co, 4, m1, m2, m3) c64
    const float inv_n = 1.0f / ((float)H * (float)W * (float)T);
    // rfftn over (W, T) plane by plane, then the H axis                       (reference :398)
    if (int rc = fwd_transform3d(x, xtrunc, Z1, B * Ci, H, W, T, m1, m2, m3, inv_n, 0, s)) return rc;
    // four corner einsums "bixyz,ioxyz->boxyz"                                  (reference :410-421)
    if (int rc = uno_mode_mix(xtrunc, w, O5, 0, B, Ci, Co, 4, (int)Mc, stream)) return rc;
    // irfftn(out_ft, s=(Ho, Wo, To), norm="forward"); later-wins masks are separable per axis (reference :400-426)
    return inv_transform3d(O5, y, Z2, B * Co, Ho, Wo, To, m1, m2, m3, 1.0f, 1, s);
}

int uno_spectral_conv3d_backward(const float* gy, const float* xtrunc, const float* const* w, float* gx, float* const* gw,
                                 void* ws, int B, int Ci, int Co, int H, int W, int T, int Ho, int Wo, int To, int m1,
                                 int m2, int m3, void* stream) {
    const char* who = "uno_spectral_conv3d_backward";
    if (B < 0 || Ci < 1 || Co < 1) { set_error("%s: bad sizes B=%d Ci=%d Co=%d", who, B, Ci, Co); return -1; }
    if (int rc = check_modes3d(who, H, W, T, Ho, Wo, To, m1, m2, m3)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long C = 2LL * m2 * m3, Mc = (long long)m1 * m2 * m3;
    if (B == 0) {
        if (gw)
            for (int c = 0; c < 4; ++c)
                if (hipMemsetAsync(gw[c], 0, 8ULL * Ci * Co * Mc, s) != hipSuccess) { set_error("memset failed"); return -5; }
        return 0;
    }
    if (!gy || !xtrunc || !w || !ws) { set_error("%s: null pointer", who); return -1; }
    float* Z1 = static_cast<float*>(ws);
    float* Z2 = Z1 + 2LL * B * Ci * H * C;
    float* gO = Z2 + 2LL * B * Co * Ho * C;
    float* gX = gO + 2LL * B * Co * 4 * Mc;
    if (int rc = fwd_transform3d(gy, gO, Z2, B * Co, Ho, Wo, To, m1, m2, m3, 1.0f, 1, s)) return rc;
    // The weight gradient stays on the caller's stream (measured round 3, one box, A/B: on the side stream next to the
    // input-gradient GEMM and the inverse transform - the 2-D arrangement - the C4 block backward took 127 us against 119.5 us
    // in sequence: at 4 corners of weights the two per-mode GEMMs are each bound by the same weight / spectrum streams)
    // (round 6, measured and not adopted here: both GEMMs in one launch - uno_mode_backward, what the 2-D layers use - took 48.0 us at the
    // C4 block against 24.5 + 21.0 in sequence: with four corners of weights each role fills the chip on its own)
    if (gw)
        if (int rc = uno_mode_wgrad(xtrunc, gO, gw, B, Ci, Co, 4, (int)Mc, stream)) return rc;
    if (gx) {
        if (int rc = uno_mode_mix(gO, w, gX, 1, B, Ci, Co, 4, (int)Mc, stream)) return rc;
        const float inv_n = 1.0f / ((float)H * (float)W * (float)T);
        if (int rc = inv_transform3d(gX, gx, Z1, B * Ci, H, W, T, m1, m2, m3, inv_n, 0, s)) return rc;
    }
    return 0;
}

// ---- the 3-D transforms as stages of their own, with a grouped placement on the spectrum side (uno_dft2d_forward_grouped's convention)
long long uno_dft3d_ws_bytes(int n_vol, int D1, int m2, int m3) {
    if (n_vol <= 0 || D1 <= 0 || m2 <= 0 || m3 <= 0) return 0;
    return 8LL * n_vol * D1 * 2 * m2 * m3;
}

// group <= 0 with stride == offset == 0: plain; else the grouped placement's conditions.  0, or -1 with the offending argument named.
static int check_grouping3d(const char* who, int n_vol, int group, int stride, int offset) {
    if (group <= 0) {
        if (stride != 0 || offset != 0) { set_error("%s: group=%d must be >= 1 when stride=%d / offset=%d are given (plain: all three 0)", who, group, stride, offset); return -1; }
        return 0;
    }
    if (offset < 0) { set_error("%s: offset=%d must be >= 0", who, offset); return -1; }
    if ((long long)offset + group > stride) { set_error("%s: stride=%d must be >= offset + group = %d + %d", who, stride, offset, group); return -1; }
    if (n_vol % group) { set_error("%s: n_vol=%d must be a multiple of group=%d", who, n_vol, group); return -1; }
    return 0;
}

static int dft3d_stage(const char* who, bool inverse, const float* in, float* out, void* ws, int n_vol, int D1, int D2, int D3, int m1, int m2,
                       int m3, float scale, int flag, int group, int stride, int offset, void* stream) {
    if (n_vol < 0) { set_error("%s: n_vol=%d must be >= 0", who, n_vol); return -1; }
    if (int rc = check_modes3d(who, D1, D2, D3, D1, D2, D3, m1, m2, m3)) return rc;
    if (int rc = check_grouping3d(who, n_vol, group, stride, offset)) return rc;
    if (n_vol == 0) return 0;
    const char* in_name = inverse ? "spec" : "x";
    const char* out_name = inverse ? "y" : "spec";
    if (!in) { set_error("%s: null pointer %s", who, in_name); return -1; }
    if (!out) { set_error("%s: null pointer %s", who, out_name); return -1; }
    if (!ws) { set_error("%s: null pointer ws (uno_dft3d_ws_bytes)", who); return -1; }
    float* Z = static_cast<float*>(ws);
    if (inverse) return inv_transform3d(in, out, Z, n_vol, D1, D2, D3, m1, m2, m3, scale, flag ? 1 : 0, (hipStream_t)stream, group, stride, offset);
    return fwd_transform3d(in, out, Z, n_vol, D1, D2, D3, m1, m2, m3, scale, flag ? 1 : 0, (hipStream_t)stream, group, stride, offset);
}

int uno_dft3d_forward_grouped(const float* x, float* spec, void* ws, int n_vol, int D1, int D2, int D3, int m1, int m2, int m3, float scale,
                              int adjoint, int group, int stride, int offset, void* stream) {
    return dft3d_stage("uno_dft3d_forward_grouped", false, x, spec, ws, n_vol, D1, D2, D3, m1, m2, m3, scale, adjoint, group, stride, offset, stream);
}

int uno_dft3d_inverse_grouped(const float* spec, float* y, void* ws, int n_vol, int D1, int D2, int D3, int m1, int m2, int m3, float scale,
                              int weighted, int group, int stride, int offset, void* stream) {
    return dft3d_stage("uno_dft3d_inverse_grouped", true, spec, y, ws, n_vol, D1, D2, D3, m1, m2, m3, scale, weighted, group, stride, offset, stream);
}

// ---- the 3-D layer on the channel concatenation of two tensors, never built: each source is transformed into (out of) its channel
// range of the one spectrum tensor by the kernels the concatenation would run (n_decide = B * Ci: results bit-equal to the one-source
// call on the concatenation); the per-mode GEMMs and the other transform are the one-source calls'
static int check_two_sources(const char* who, int C1, int Ci) {
    if (C1 < 1 || C1 >= Ci) { set_error("%s: C1=%d must satisfy 0 < C1 < Ci=%d", who, C1, Ci); return -1; }
    return 0;
}

int uno_spectral_conv3d_forward2(const float* x1, const float* x2, int C1, const float* const* w, float* y, float* xtrunc, void* ws, int B,
                                 int Ci, int Co, int H, int W, int T, int Ho, int Wo, int To, int m1, int m2, int m3, void* stream) {
    const char* who = "uno_spectral_conv3d_forward2";
    if (!x2) return uno_spectral_conv3d_forward(x1, w, y, xtrunc, ws, B, Ci, Co, H, W, T, Ho, Wo, To, m1, m2, m3, stream);
    if (B < 0 || Ci < 1 || Co < 1) { set_error("%s: bad sizes B=%d Ci=%d Co=%d", who, B, Ci, Co); return -1; }
    if (int rc = check_two_sources(who, C1, Ci)) return rc;
    if (int rc = check_modes3d(who, H, W, T, Ho, Wo, To, m1, m2, m3)) return rc;
    if (B == 0) return 0;
    if (!x1 || !w || !y || !xtrunc || !ws) { set_error("%s: null pointer", who); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const long long C = 2LL * m2 * m3, Mc = (long long)m1 * m2 * m3;
    const int C2 = Ci - C1;
    float* Z1 = static_cast<float*>(ws);                         // (B*C1*H | B*C2*H, 2 m2, m3) c64: one part per source
    float* Z1b = Z1 + 2LL * B * C1 * H * C;
    float* Z2 = Z1 + 2LL * B * Ci * H * C;                        // (B*Co*Ho, 2 m2, m3) c64
    float* O5 = Z2 + 2LL * B * Co * Ho * C;                       // (B, Co, 4, m1, m2, m3) c64
    const float inv_n = 1.0f / ((float)H * (float)W * (float)T);
    if (int rc = fwd_transform3d(x1, xtrunc, Z1, B * C1, H, W, T, m1, m2, m3, inv_n, 0, s, C1, Ci, 0, B * Ci)) return rc;
    if (int rc = fwd_transform3d(x2, xtrunc, Z1b, B * C2, H, W, T, m1, m2, m3, inv_n, 0, s, C2, Ci, C1, B * Ci)) return rc;
    if (int rc = uno_mode_mix(xtrunc, w, O5, 0, B, Ci, Co, 4, (int)Mc, stream)) return rc;
    return inv_transform3d(O5, y, Z2, B * Co, Ho, Wo, To, m1, m2, m3, 1.0f, 1, s);
}

int uno_spectral_conv3d_backward2(const float* gy, const float* xtrunc, const float* const* w, float* gx1, float* gx2, int C1,
                                  float* const* gw, void* ws, int B, int Ci, int Co, int H, int W, int T, int Ho, int Wo, int To, int m1,
                                  int m2, int m3, void* stream) {
    const char* who = "uno_spectral_conv3d_backward2";
    if (!gx2) return uno_spectral_conv3d_backward(gy, xtrunc, w, gx1, gw, ws, B, Ci, Co, H, W, T, Ho, Wo, To, m1, m2, m3, stream);
    if (B < 0 || Ci < 1 || Co < 1) { set_error("%s: bad sizes B=%d Ci=%d Co=%d", who, B, Ci, Co); return -1; }
    if (int rc = check_two_sources(who, C1, Ci)) return rc;
    if (int rc = check_modes3d(who, H, W, T, Ho, Wo, To, m1, m2, m3)) return rc;
    if (!gx1) { set_error("%s: null pointer gx1 (gx2 is given)", who); return -1; }
    if (gx1 == gx2) { set_error("%s: gx1 must not alias gx2", who); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const long long C = 2LL * m2 * m3, Mc = (long long)m1 * m2 * m3;
    if (B == 0) {
        if (gw)
            for (int c = 0; c < 4; ++c)
                if (hipMemsetAsync(gw[c], 0, 8ULL * Ci * Co * Mc, s) != hipSuccess) { set_error("memset failed"); return -5; }
        return 0;
    }
    if (!gy || !xtrunc || !w || !ws) { set_error("%s: null pointer", who); return -1; }
    const int C2 = Ci - C1;
    float* Z1 = static_cast<float*>(ws);
    float* Z1b = Z1 + 2LL * B * C1 * H * C;
    float* Z2 = Z1 + 2LL * B * Ci * H * C;
    float* gO = Z2 + 2LL * B * Co * Ho * C;
    float* gX = gO + 2LL * B * Co * 4 * Mc;
    if (int rc = fwd_transform3d(gy, gO, Z2, B * Co, Ho, Wo, To, m1, m2, m3, 1.0f, 1, s)) return rc;
    if (gw)
        if (int rc = uno_mode_wgrad(xtrunc, gO, gw, B, Ci, Co, 4, (int)Mc, stream)) return rc;
    if (int rc = uno_mode_mix(gO, w, gX, 1, B, Ci, Co, 4, (int)Mc, stream)) return rc;
    const float inv_n = 1.0f / ((float)H * (float)W * (float)T);
    if (int rc = inv_transform3d(gX, gx1, Z1, B * C1, H, W, T, m1, m2, m3, inv_n, 0, s, C1, Ci, 0, B * Ci)) return rc;
    return inv_transform3d(gX, gx2, Z1b, B * C2, H, W, T, m1, m2, m3, inv_n, 0, s, C2, Ci, C1, B * Ci);
}

static int spectral_conv2d_forward(const float* x, const float* w1, const float* w2, float* y, float* xtrunc, void* ws,
                                   int B, int Ci, int Co, int H, int W, int Ho, int Wo, int m1, int m2, void* stream, int bf16, int w_half = 0) {
    if (B < 0 || Ci < 1 || Co < 1) { set_error("uno_spectral_conv2d_forward: bad sizes B=%d Ci=%d Co=%d", B, Ci, Co); return -1; }
    if (int rc = check_modes2d("uno_spectral_conv2d_forward", H, W, Ho, Wo, m1, m2)) return rc;
    if (B == 0) return 0;           // empty batch: nothing to do (empty tensors carry null pointers)
    if (!x || !w1 || !w2 || !y || !xtrunc || !ws) { set_error("uno_spectral_conv2d_forward: null pointer"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    float* O = static_cast<float*>(ws);
    // rfft2(x, norm="forward") restricted to the two corners            (reference :187)
    if (int rc = dft2d(false, x, xtrunc, B * Ci, H, W, m1, m2, 1.0f / ((float)H * (float)W), 0, 0, s, 0, 0, 0, bf16)) return rc;
    // einsum("bixy,ioxy->boxy") with weights1 / weights2                  (reference :198-203)
    const float* wv[2] = {w1, w2};
    if (int rc = mode_mix_impl(xtrunc, wv, O, 0, B, Ci, Co, 2, m1 * m2, stream, w_half)) return rc;
    // irfft2(out_ft, s=(Ho, Wo), norm="forward"), later-wins on overlapping rows (reference :190-206)
    return dft2d(true, O, y, B * Co, Ho, Wo, m1, m2, 1.0f, 1, 1, s, 0, 0, 0, bf16);
}

int uno_spectral_conv2d_forward(const float* x, const float* w1, const float* w2, float* y, float* xtrunc, void* ws,
                                int B, int Ci, int Co, int H, int W, int Ho, int Wo, int m1, int m2, void* stream) {
    return spectral_conv2d_forward(x, w1, w2, y, xtrunc, ws, B, Ci, Co, H, W, Ho, Wo, m1, m2, stream, 0);
}

int uno_spectral_conv2d_forward_bf16(const void* x, const float* w1, const float* w2, void* y, float* xtrunc, void* ws,
                                     int B, int Ci, int Co, int H, int W, int Ho, int Wo, int m1, int m2, void* stream) {
    return spectral_conv2d_forward(static_cast<const float*>(x), w1, w2, static_cast<float*>(y), xtrunc, ws, B, Ci, Co, H, W, Ho, Wo,
                                   m1, m2, stream, 1);
}

static int spectral_conv2d_backward(const float* gy, const float* xtrunc, const float* w1, const float* w2, float* gx,
                                    float* gw1, float* gw2, void* ws, int B, int Ci, int Co, int H, int W, int Ho, int Wo,
                                    int m1, int m2, void* stream, int bf16, int w_half = 0, int accumulate_gw = 0) {
    if (B > 0 && (!gy || !xtrunc || !w1 || !w2 || !ws)) { set_error("uno_spectral_conv2d_backward: null pointer"); return -1; }
    if ((gw1 == nullptr) != (gw2 == nullptr)) { set_error("uno_spectral_conv2d_backward: gw1/gw2 must both be given or both be NULL"); return -1; }
    if (B < 0 || Ci < 1 || Co < 1) { set_error("uno_spectral_conv2d_backward: bad sizes B=%d Ci=%d Co=%d", B, Ci, Co); return -1; }
    if (int rc = check_modes2d("uno_spectral_conv2d_backward", H, W, Ho, Wo, m1, m2)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long P = 2LL * m1 * m2;
    float* gO = static_cast<float*>(ws);
    float* gX = gO + 2LL * B * Co * P;
    if (B == 0) {
        if (gw1 && !accumulate_gw) {
            if (hipMemsetAsync(gw1, 0, 8ULL * Ci * Co * m1 * m2, s) != hipSuccess || hipMemsetAsync(gw2, 0, 8ULL * Ci * Co * m1 * m2, s) != hipSuccess) {
                set_error("memset failed"); return -5;
            }
        }
        return 0;
    }
    // gO = c (.) keep (.) DFT_trunc(gy)                                   (adjoint of irfft2 + CopySlices)
    if (int rc = dft2d(false, gy, gO, B * Co, Ho, Wo, m1, m2, 1.0f, 1, 1, s, 0, 0, 0, bf16)) return rc;
    // The weight gradient only shares gO with the input-gradient chain: it runs on the side stream next to the
    // (under-filled) input-gradient GEMM and the store-bound inverse DFT.
    // (round 6, measured and not adopted HERE: both per-mode GEMMs in one launch - uno_mode_backward, what the stage-by-stage callers use -
    // took the C2 block backward from 352-355 to 361 us: this composite already hides the weight gradient behind the inverse transform)
    SideStream* side = (gw1 && gx) ? side_stream_of_current_device() : nullptr;
    int rc_w = 0;
    if (gw1) {
        float* gwv[2] = {gw1, gw2};
        if (side) {
            side->mu.lock();
            if (hipEventRecord(side->fork_ev, s) != hipSuccess || hipStreamWaitEvent(side->s, side->fork_ev, 0) != hipSuccess) {
                side->mu.unlock();
                side = nullptr;
            }
        }
        rc_w = mode_wgrad_impl(xtrunc, gO, gwv, B, Ci, Co, 2, m1 * m2, accumulate_gw, side ? (void*)side->s : stream);
    }
    int rc_x = 0;
    if (gx && rc_w == 0) {
        const float* wv[2] = {w1, w2};
        rc_x = mode_mix_impl(gO, wv, gX, 1, B, Ci, Co, 2, m1 * m2, stream, w_half);
        // gx = 1/(H W) Re iDFT_trunc(gX)                                   (adjoint of rfft2(norm="forward"))
        if (rc_x == 0) rc_x = dft2d(true, gX, gx, B * Ci, H, W, m1, m2, 1.0f / ((float)H * (float)W), 0, 0, s, 0, 0, 0, bf16);
    }
    if (side) {
        const bool joined = hipEventRecord(side->join_ev, side->s) == hipSuccess && hipStreamWaitEvent(s, side->join_ev, 0) == hipSuccess;
        side->mu.unlock();
        if (!joined) { set_error("uno_spectral_conv2d_backward: side-stream join failed"); return -5; }
    }
    return rc_w ? rc_w : rc_x;
}

int uno_spectral_conv2d_backward(const float* gy, const float* xtrunc, const float* w1, const float* w2, float* gx,
                                 float* gw1, float* gw2, void* ws, int B, int Ci, int Co, int H, int W, int Ho, int Wo,
                                 int m1, int m2, void* stream) {
    return spectral_conv2d_backward(gy, xtrunc, w1, w2, gx, gw1, gw2, ws, B, Ci, Co, H, W, Ho, Wo, m1, m2, stream, 0);
}

int uno_spectral_conv2d_backward_bf16(const void* gy, const float* xtrunc, const float* w1, const float* w2, void* gx,
                                      float* gw1, float* gw2, void* ws, int B, int Ci, int Co, int H, int W, int Ho, int Wo,
                                      int m1, int m2, void* stream) {
    return spectral_conv2d_backward(static_cast<const float*>(gy), xtrunc, w1, w2, static_cast<float*>(gx), gw1, gw2, ws, B, Ci, Co,
                                    H, W, Ho, Wo, m1, m2, stream, 1);
}

int uno_spectral_conv2d_backward_acc(const void* gy, const float* xtrunc, const void* w1, const void* w2, void* gx,
                                     float* gw1, float* gw2, void* ws, int B, int Ci, int Co, int H, int W, int Ho, int Wo,
                                     int m1, int m2, int io_format, int accumulate_gw, void* stream) {
    if (io_format < 0 || io_format > 2) { set_error("uno_spectral_conv2d_backward_acc: io_format %d (0 f32, 1 bf16, 2 bf16 + fp16 weights)", io_format); return -1; }
    return spectral_conv2d_backward(static_cast<const float*>(gy), xtrunc, static_cast<const float*>(w1), static_cast<const float*>(w2),
                                    static_cast<float*>(gx), gw1, gw2, ws, B, Ci, Co, H, W, Ho, Wo, m1, m2, stream, io_format >= 1,
                                    io_format == 2, accumulate_gw ? 1 : 0);
}

int uno_spectral_conv2d_forward_mixed(const void* x, const void* w1, const void* w2, void* y, float* xtrunc, void* ws,
                                      int B, int Ci, int Co, int H, int W, int Ho, int Wo, int m1, int m2, void* stream) {
    return spectral_conv2d_forward(static_cast<const float*>(x), static_cast<const float*>(w1), static_cast<const float*>(w2),
                                   static_cast<float*>(y), xtrunc, ws, B, Ci, Co, H, W, Ho, Wo, m1, m2, stream, 1, 1);
}

int uno_spectral_conv2d_backward_mixed(const void* gy, const float* xtrunc, const void* w1, const void* w2, void* gx,
                                       float* gw1, float* gw2, void* ws, int B, int Ci, int Co, int H, int W, int Ho, int Wo,
                                       int m1, int m2, void* stream) {
    return spectral_conv2d_backward(static_cast<const float*>(gy), xtrunc, static_cast<const float*>(w1), static_cast<const float*>(w2),
                                    static_cast<float*>(gx), gw1, gw2, ws, B, Ci, Co, H, W, Ho, Wo, m1, m2, stream, 1, 1);
}

}  // extern "C"
