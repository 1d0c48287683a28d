// C ABI of libuno_spectral.so, the point-wise entry points: banded resampling, channel mix / weight gradient (K8 / K9), border clearing,
// the lift, the projected-back backward pass, the GELU forms, the batched transpose, InstanceNorm and Adam (core: capi.hip).
#include "../../include/uno_spectral.h"
#include "uno_common.h"

using namespace uno;

extern "C" {

static int resample2d_impl(const void* in, void* out, float* tmp, int n_img, int H, int W, int Ho, int Wo, const int* startH,
                           const float* wtH, int KH, const int* startW, const float* wtW, int KW, const int* tile_p0,
                           const float* tile_w, int NP, int accumulate, int bf16, void* stream) {
    if (n_img < 0 || H < 1 || W < 1 || Ho < 1 || Wo < 1) { set_error("uno_resample2d: bad sizes"); return -1; }
    if (n_img == 0) return 0;
    if (!in || !out || !tmp || !startH || !wtH || !startW || !wtW) { set_error("uno_resample2d: null pointer"); return -1; }
    return launch_resample2d(in, out, tmp, n_img, H, W, Ho, Wo, startH, wtH, KH, startW, wtW, KW, tile_p0, tile_w, NP, accumulate, bf16, (hipStream_t)stream);
}

int uno_resample2d(const float* in, float* out, float* tmp, int n_img, int H, int W, int Ho, int Wo, const int* startH,
                   const float* wtH, int KH, const int* startW, const float* wtW, int KW, const int* tile_p0,
                   const float* tile_w, int NP, int accumulate, void* stream) {
    return resample2d_impl(in, out, tmp, n_img, H, W, Ho, Wo, startH, wtH, KH, startW, wtW, KW, tile_p0, tile_w, NP, accumulate, 0, stream);
}

int uno_resample2d_bf16(const void* in, void* out, float* tmp, int n_img, int H, int W, int Ho, int Wo, const int* startH,
                        const float* wtH, int KH, const int* startW, const float* wtW, int KW, const int* tile_p0,
                        const float* tile_w, int NP, int accumulate, void* stream) {
    return resample2d_impl(in, out, tmp, n_img, H, W, Ho, Wo, startH, wtH, KH, startW, wtW, KW, tile_p0, tile_w, NP, accumulate, 1, stream);
}

static int channel_mix_impl(const void* x, const float* w, const float* bias, void* y, int B, int Ci, int Co, long long P,
                            int transpose_w, int accumulate, int act_in, const void* dgelu_of, int bf16, void* stream) {
    if (B < 0 || Ci < 1 || Co < 1 || P < 0) { set_error("uno_channel_mix: bad sizes B=%d Ci=%d Co=%d P=%lld", B, Ci, Co, P); return -1; }
    if (B == 0 || P == 0) return 0;
    if (!x || !w || !y) { set_error("uno_channel_mix: null pointer"); return -1; }
    return launch_channel_mix(x, w, bias, y, B, Ci, Co, P, transpose_w, accumulate, act_in, dgelu_of, bf16, (hipStream_t)stream,
                              thread_scratch().ptr, thread_scratch().bytes);
}

long long uno_channel_mix_ws_bytes(int Ci, int Co, long long P, int bf16) {
    if (Ci < 1 || Co < 1 || P < 1) return 0;
    return channel_mix_ws_bytes(Ci, Co, P, bf16);
}

int uno_channel_mix(const float* x, const float* w, const float* bias, float* y, int B, int Ci, int Co, long long P,
                    int transpose_w, int accumulate, int act_in, const float* dgelu_of, void* stream) {
    return channel_mix_impl(x, w, bias, y, B, Ci, Co, P, transpose_w, accumulate, act_in, dgelu_of, 0, stream);
}

int uno_channel_mix_bf16(const void* x, const float* w, const float* bias, void* y, int B, int Ci, int Co, long long P,
                         int transpose_w, int accumulate, int act_in, const void* dgelu_of, void* stream) {
    return channel_mix_impl(x, w, bias, y, B, Ci, Co, P, transpose_w, accumulate, act_in, dgelu_of, 1, stream);
}

static int channel_mix2_impl(const void* x1, const void* x2, int C1, const float* w, const float* bias, void* y1, void* y2, int Co1,
                             void* y_act, int B, int Ci, int Co, long long P, int transpose_w, int accumulate, int act_in,
                             const void* dgelu_of, const float* proj_w, const float* proj_b, void* proj_out, int bf16, void* stream,
                             const PixelWindow& win = PixelWindow()) {
    if (B < 0 || Ci < 1 || Co < 1 || P < 0) { set_error("uno_channel_mix2: bad sizes B=%d Ci=%d Co=%d P=%lld", B, Ci, Co, P); return -1; }
    if (B == 0 || P == 0) return 0;
    if (!x1 || !w || !y1) { set_error("uno_channel_mix2: null pointer"); return -1; }
    ChannelMixArgs a{};
    a.x = x1; a.x2 = x2; a.w = w; a.bias = bias; a.y = y1; a.y2 = y2; a.y_act = y_act; a.dgelu_of = dgelu_of;
    a.B = B; a.Ci = Ci; a.Co = Co; a.C1 = x2 ? C1 : Ci; a.Co1 = y2 ? Co1 : Co; a.P = P;
    a.transpose_w = transpose_w; a.accumulate = accumulate; a.act_in = act_in; a.bf16 = bf16;
    a.proj_w = proj_w; a.proj_b = proj_b; a.proj_out = proj_out;
    a.win = win;
    a.ws = thread_scratch().ptr; a.ws_bytes = thread_scratch().bytes;
    return launch_channel_mix2(a, (hipStream_t)stream);
}

int uno_channel_mix2(const float* x1, const float* x2, int C1, const float* w, const float* bias, float* y1, float* y2, int Co1,
                     float* y_act, int B, int Ci, int Co, long long P, int transpose_w, int accumulate, int act_in,
                     const float* dgelu_of, const float* proj_w, const float* proj_b, float* proj_out, void* stream) {
    return channel_mix2_impl(x1, x2, C1, w, bias, y1, y2, Co1, y_act, B, Ci, Co, P, transpose_w, accumulate, act_in, dgelu_of,
                             proj_w, proj_b, proj_out, 0, stream);
}

int uno_channel_mix2_bf16(const void* x1, const void* x2, int C1, const float* w, const float* bias, void* y1, void* y2, int Co1,
                          void* y_act, int B, int Ci, int Co, long long P, int transpose_w, int accumulate, int act_in,
                          const void* dgelu_of, const float* proj_w, const float* proj_b, void* proj_out, void* stream) {
    return channel_mix2_impl(x1, x2, C1, w, bias, y1, y2, Co1, y_act, B, Ci, Co, P, transpose_w, accumulate, act_in, dgelu_of,
                             proj_w, proj_b, proj_out, 1, stream);
}

// the pixel axis of a *_win call: rows x cols logical pixels, row r at r * pitch of a channel plane, planes `plane` elements apart
// (who == nullptr: a query - no error text is left)
static bool make_window(const char* who, int rows, int cols, int pitch, long long plane, PixelWindow* win, long long* P) {
    if (rows < 1 || cols < 1 || pitch < cols || plane < 1) { if (who) set_error("%s: bad window rows=%d cols=%d pitch=%d plane=%lld", who, rows, cols, pitch, plane); return false; }
    win->plane = plane; win->cols = cols; win->pitch = pitch;
    *P = (long long)rows * cols;
    return true;
}

int uno_channel_mix2_win(const float* x1, const float* x2, int C1, const float* w, const float* bias, float* y1, float* y2, int Co1,
                         float* y_act, int B, int Ci, int Co, int rows, int cols, int pitch, long long plane, int transpose_w,
                         int accumulate, int act_in, const float* dgelu_of, const float* proj_w, const float* proj_b, float* proj_out,
                         void* stream) {
    PixelWindow win; long long P;
    if (!make_window("uno_channel_mix2_win", rows, cols, pitch, plane, &win, &P)) return -1;
    return channel_mix2_impl(x1, x2, C1, w, bias, y1, y2, Co1, y_act, B, Ci, Co, P, transpose_w, accumulate, act_in, dgelu_of,
                             proj_w, proj_b, proj_out, 0, stream, win);
}

// ---- the backward pass of `fc2(F.gelu(fc1(cat)))` without the gradient at fc1's output in memory (ABI 12)
static bool project_backward_geometry(const char* who, int rows, int cols, int pitch, long long plane, PixelWindow* win, long long* P) {
    if (rows == 0 && cols == 0 && pitch == 0) {          // dense planes
        if (plane < 1) { if (who) set_error("%s: bad plane size %lld", who, plane); return false; }
        *win = PixelWindow(); *P = plane;
        return true;
    }
    if (!make_window(who, rows, cols, pitch, plane, win, P)) return false;
    if (const char* why = pix_window_error(*win, *P)) { if (who) set_error("%s: %s", who, why); return false; }
    return true;
}

int uno_project_backward_applies(int B, int C1, int Ci, int Co, int rows, int cols, int pitch, long long plane) {
    PixelWindow win; long long P;
    if (B < 1 || B > 65535 || Ci < 1 || Co < 1 || C1 < 1 || C1 > Ci || !project_backward_geometry(nullptr, rows, cols, pitch, plane, &win, &P)) return 0;
    // the input gradients: the wide kernel's general form on fc1's Co channels -> Ci gradient channels, destinations split at C1
    if (Ci % 128 || Co % 16 || Co >= 128 || P < 128 || P % 4 || (C1 < Ci && C1 % 64)) return 0;
    if ((long long)Ci * plane >= (1LL << 29) || (long long)Ci * Co >= (1LL << 30)) return 0;
    return channel_wgrad_pb_applies(B, Ci, Co, C1, P) ? 1 : 0;
}

long long uno_project_backward_ws_bytes(int B, int Ci, int Co, long long P) {
    if (B < 1 || Ci < 1 || Co < 1 || P < 1) return 0;
    return 4LL * channel_wgrad_pb_ws_floats(B, Ci, Co, P);
}

int uno_project_backward(const float* x1, const float* x2, int C1, const float* w, const float* pre, const float* w2, const float* gout,
                         float* g1, float* g2, float* gw, float* gb, float* gw2, float* gb2, void* ws, int B, int Ci, int Co, int rows,
                         int cols, int pitch, long long plane, int act_in, int accumulate_w, void* stream) {
    PixelWindow win; long long P;
    if (B < 0 || Ci < 1 || Co < 1) { set_error("uno_project_backward: bad sizes B=%d Ci=%d Co=%d", B, Ci, Co); return -1; }
    if (!project_backward_geometry("uno_project_backward", rows, cols, pitch, plane, &win, &P)) return -1;
    if (accumulate_w != 0 && accumulate_w != 1) { set_error("uno_project_backward: accumulate_w is 0 or 1"); return -1; }
    if (!gw || !gw2) { set_error("uno_project_backward: null pointer"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        if ((!accumulate_w && (hipMemsetAsync(gw, 0, sizeof(float) * Co * Ci, s) != hipSuccess || (gb && hipMemsetAsync(gb, 0, sizeof(float) * Co, s) != hipSuccess))) ||
            hipMemsetAsync(gw2, 0, sizeof(float) * Co, s) != hipSuccess || (gb2 && hipMemsetAsync(gb2, 0, sizeof(float), s) != hipSuccess)) {
            set_error("uno_project_backward: memset failed");
            return -5;
        }
        return 0;
    }
    if (!x2) C1 = Ci;
    if (!uno_project_backward_applies(B, C1, Ci, Co, rows, cols, pitch, plane)) {
        set_error("uno_project_backward: shape outside the fused kernels' range (query uno_project_backward_applies)");
        return -3;
    }
    if (!x1 || !w || !pre || !w2 || !gout || !g1 || (x2 && !g2) || !ws) { set_error("uno_project_backward: null pointer"); return -1; }
    {   // both input gradients from one pass over the pre-activation
        ChannelMixArgs a{};
        a.x = pre; a.w = w; a.y = g1; a.y2 = x2 ? g2 : nullptr; a.dgelu_of = act_in ? x1 : nullptr;
        a.B = B; a.Ci = Co; a.Co = Ci; a.C1 = Co; a.Co1 = x2 ? C1 : Ci; a.P = P; a.transpose_w = 1;
        a.win = win; a.pb_w2 = w2; a.pb_g = gout;
        if (int rc = launch_channel_mix2(a, s)) return rc;
    }
    WgradProjectedBack pb;
    pb.w2 = w2; pb.g = gout; pb.gw2 = gw2; pb.gb2 = gb2;
    return launch_channel_wgrad2(pre, x1, x2, C1, gw, gb, (float*)ws, B, Ci, Co, P, act_in, accumulate_w, 0, s, win, pb);
}

int uno_clear_border(float* t, long long n_planes, int Hp, int Wp, int rows, int cols, void* stream) {
    if (n_planes < 0 || Hp < 1 || Wp < 1 || rows < 0 || rows > Hp || cols < 0 || cols > Wp) {
        set_error("uno_clear_border: bad sizes planes=%lld (%d, %d) keep (%d, %d)", n_planes, Hp, Wp, rows, cols);
        return -1;
    }
    if (n_planes == 0) return 0;
    if (!t) { set_error("uno_clear_border: null pointer"); return -1; }
    return launch_clear_border(t, n_planes, Hp, Wp, rows, cols, (hipStream_t)stream);
}

static int lift_padded(const char* who, const float* x, const float* w, const float* bias, float* y, float* y_act, const float* gmul, int B,
                       int Ci, int Co, int H, int W, int Hp, int Wp, int act_in, void* stream) {
    if (B < 0 || Ci < 1 || Co < 1 || H < 1 || W < 1 || Hp < H || Wp < W) {
        set_error("%s: bad sizes B=%d Ci=%d Co=%d (%d, %d) -> (%d, %d)", who, B, Ci, Co, H, W, Hp, Wp);
        return -1;
    }
    if (B == 0) return 0;
    if (!x || !w || (!y && !y_act) || (gmul && !y)) { set_error("%s: null pointer", who); return -1; }
    ChannelMixArgs a{};
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.y_act = y_act; a.gmul = gmul;
    a.B = B; a.Ci = Ci; a.Co = Co; a.C1 = Ci; a.Co1 = Co; a.P = (long long)H * W; a.act_in = act_in;
    a.act_cols = W; a.act_pitch = Wp; a.act_plane = (long long)Hp * Wp;
    if (int rc = launch_channel_mix2(a, (hipStream_t)stream)) return rc;
    return y_act ? launch_clear_border(y_act, (long long)B * Co, Hp, Wp, H, W, (hipStream_t)stream) : 0;
}

int uno_channel_mix_act_padded(const float* x, const float* w, const float* bias, float* y, float* y_act, int B, int Ci, int Co, int H, int W,
                               int Hp, int Wp, int act_in, void* stream) {
    if (!y_act) { set_error("uno_channel_mix_act_padded: null pointer"); return -1; }
    return lift_padded("uno_channel_mix_act_padded", x, w, bias, y, y_act, nullptr, B, Ci, Co, H, W, Hp, Wp, act_in, stream);
}

int uno_channel_mix_dgelu_padded(const float* x, const float* w, const float* bias, const float* g_padded, float* gz, int B, int Ci, int Co,
                                 int H, int W, int Hp, int Wp, int act_in, void* stream) {
    if (!g_padded || !gz) { set_error("uno_channel_mix_dgelu_padded: null pointer"); return -1; }
    return lift_padded("uno_channel_mix_dgelu_padded", x, w, bias, gz, nullptr, g_padded, B, Ci, Co, H, W, Hp, Wp, act_in, stream);
}

// ---- the whole lift (reference darcy_flow_uno2d.py:98-107) with its first layer's output never stored
static int lift_check(const char* who, int B, int Cin, int Cm, int Co, int H, int W, int Hp, int Wp) {
    if (B < 0 || Cin < 1 || Cin > 3 || Cm < 5 || Cm > 32 || Cm % 16 || Co < 1 || H < 1 || W < 260 || Hp < H || Wp < W || (long long)H * W >= (1LL << 24)) {
        set_error("%s: needs 1 .. 3 input channels, 16 or 32 middle channels, 260 <= W <= Wp, H <= Hp, H * W < 2^24 (got B=%d %d -> %d -> %d, (%d, %d) -> (%d, %d))",
                  who, B, Cin, Cm, Co, H, W, Hp, Wp);
        return -1;
    }
    return 0;
}

// size limits of the fused lift kernels (lift_bwd.hip: 32-bit element offsets into the padded planes, 24-bit pixel slots over H x Wp):
// grids beyond them take the layer-by-layer forms below instead of failing (advisor finding, round 5)
static bool lift_fused_fits(int B, int H, int Hp, int Wp, int Co) {
    return (long long)Hp * Wp * Co < (1LL << 31) && B <= 65535 && (long long)H * Wp < (1LL << 24);
}

int uno_lift_forward(const float* x, const float* w1, const float* b1, const float* w0, const float* b0, float* act, int B, int Cin, int Cm,
                     int Co, int H, int W, int Hp, int Wp, void* stream) {
    if (int rc = lift_check("uno_lift_forward", B, Cin, Cm, Co, H, W, Hp, Wp)) return rc;
    if (B == 0) return 0;
    if (!x || !w1 || !w0 || !act) { set_error("uno_lift_forward: null pointer"); return -1; }
    if (lift_bwd_fused_applies(Cin, Cm, Co, W, (long long)H * W) && lift_fused_fits(B, H, Hp, Wp, Co) && (Wp & ~3) >= 260 && (Wp & ~3) >= W) {      // K16 (lift_bwd.hip): the dedicated kernel at the Darcy widths
        if (int rc = launch_lift_forward_fused(x, w1, b1, w0, b0, act, B, Cin, H, W, Hp, Wp, (hipStream_t)stream)) return rc;
        return launch_clear_border(act, (long long)B * Co, Hp, Wp, H, Wp, (hipStream_t)stream);         // the rows below the domain
    }
    ChannelMixArgs a{};
    a.x = x; a.w = w0; a.bias = b0; a.y = nullptr; a.y_act = act;
    a.B = B; a.Ci = Cm; a.Co = Co; a.C1 = Cm; a.Co1 = Co; a.P = (long long)H * W; a.act_in = 1;
    a.act_cols = W; a.act_pitch = Wp; a.act_plane = (long long)Hp * Wp;
    a.vh_x = x; a.vh_w = w1; a.vh_b = b1; a.vh_ci = Cin; a.vh_mode = 1;
    if (int rc = launch_channel_mix2(a, (hipStream_t)stream)) return rc;
    return launch_clear_border(act, (long long)B * Co, Hp, Wp, H, W, (hipStream_t)stream);
}

// scratch of uno_lift_backward: gz (B, Co, H, W), g_h (B, Cm, H, W), then the larger of the two weight-gradient scratches
static long long lift_wgrad_ws(int B, int Cin, int Cm, int Co, long long P) {
    const long long a = 4LL * channel_wgrad_ws_floats(B, Cm, Co, P, nullptr), b = 4LL * channel_wgrad_ws_floats(B, Cin, Cm, P, nullptr);
    return a > b ? a : b;
}
long long uno_lift_bwd_ws_bytes(int B, int Cin, int Cm, int Co, int H, int W) {
    if (B < 1 || Cin < 1 || Cm < 1 || Co < 1 || H < 1 || W < 1) return 0;
    const long long P = (long long)H * W;
    return 4LL * B * P * (Co + Cm) + lift_wgrad_ws(B, Cin, Cm, Co, P);
}

int uno_lift_backward_takes_second(int B, int Cin, int Cm, int Co, int H, int W, int Hp, int Wp) {
    if (B < 1 || Cin < 1 || Cin > 3 || Cm < 5 || Cm > 32 || Cm % 16 || Co < 1 || H < 1 || W < 260 || Hp < H || Wp < W) return 0;
    return (lift_bwd_fused_applies(Cin, Cm, Co, W, (long long)H * W) && lift_fused_fits(B, H, Hp, Wp, Co)) ? 1 : 0;
}

int uno_lift_backward2(const float* x, const float* w1, const float* b1, const float* w0, const float* b0_, const float* g_act, const float* g_act2,
                       float* gw1, float* gb1, float* gw0, float* gb0, void* ws, int B, int Cin, int Cm, int Co, int H, int W, int Hp, int Wp,
                       void* stream);

int uno_lift_backward(const float* x, const float* w1, const float* b1, const float* w0, const float* b0_, const float* g_act, float* gw1,
                      float* gb1, float* gw0, float* gb0, void* ws, int B, int Cin, int Cm, int Co, int H, int W, int Hp, int Wp, void* stream) {
    return uno_lift_backward2(x, w1, b1, w0, b0_, g_act, nullptr, gw1, gb1, gw0, gb0, ws, B, Cin, Cm, Co, H, W, Hp, Wp, stream);
}

int uno_lift_backward2(const float* x, const float* w1, const float* b1, const float* w0, const float* b0_, const float* g_act, const float* g_act2,
                       float* gw1, float* gb1, float* gw0, float* gb0, void* ws, int B, int Cin, int Cm, int Co, int H, int W, int Hp, int Wp,
                       void* stream) {
    if (int rc = lift_check("uno_lift_backward", B, Cin, Cm, Co, H, W, Hp, Wp)) return rc;
    if (g_act2 && !uno_lift_backward_takes_second(B, Cin, Cm, Co, H, W, Hp, Wp) && B > 0) {
        set_error("uno_lift_backward2: a second gradient tensor goes with the fused kernel only (query uno_lift_backward_takes_second)");
        return -3;
    }
    if (!gw1 || !gw0) { set_error("uno_lift_backward: null pointer"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        if (hipMemsetAsync(gw1, 0, sizeof(float) * Cm * Cin, s) != hipSuccess || hipMemsetAsync(gw0, 0, sizeof(float) * Co * Cm, s) != hipSuccess ||
            (gb1 && hipMemsetAsync(gb1, 0, sizeof(float) * Cm, s) != hipSuccess) || (gb0 && hipMemsetAsync(gb0, 0, sizeof(float) * Co, s) != hipSuccess)) {
            set_error("uno_lift_backward: memset failed");
            return -5;
        }
        return 0;
    }
    if (!x || !w1 || !w0 || !g_act || !ws) { set_error("uno_lift_backward: null pointer"); return -1; }
    const long long P = (long long)H * W;
    if (lift_bwd_fused_applies(Cin, Cm, Co, W, P) && lift_fused_fits(B, H, Hp, Wp, Co)) {
        // one kernel per pixel tile: neither gz nor gh leaves the chip (lift_bwd.hip); ws = the two arrays of partial-sum blocks
        float* part = static_cast<float*>(ws);
        const long long nparts = lift_bwd_fused_parts(B, H, W);
        float* part1 = part + (size_t)nparts * Co * (Cm + 1);
        if (int rc = launch_lift_backward_fused(x, w1, b1, w0, b0_, g_act, part, part1, B, Cin, H, W, Hp, Wp, s, g_act2)) return rc;
        if (int rc = launch_channel_wgrad_finish(part, gw0, gb0, Cm, Co, nparts, 0, s)) return rc;
        return launch_channel_wgrad_finish(part1, gw1, gb1, Cin, Cm, nparts, 0, s);
    }
    // (measured and dropped, round 5: batch entries in groups whose gz stays in the 256 MB Infinity Cache between the kernel that writes
    // it and the two that read it - groups of 2 / 4 / 8 of 16 ran the step at 13.1-13.3 / 12.8 / 12.65 ms against 12.37-12.40 whole: the
    // shorter launches lose more to ramp and tail than the cache gives)
    float* gz = static_cast<float*>(ws);
    float* gh = gz + (size_t)B * Co * P;
    float* wws = gh + (size_t)B * Cm * P;
    // 1. gz = gelu'(fc0(gelu(h))) * g_act[..., :H, :W], the layer recomputed from the virtual h = fc_n1(x)
    {
        ChannelMixArgs a{};
        a.x = x; a.w = w0; a.bias = b0_; a.y = gz; a.gmul = g_act;
        a.B = B; a.Ci = Cm; a.Co = Co; a.C1 = Cm; a.Co1 = Co; a.P = P; a.act_in = 1;
        a.act_cols = W; a.act_pitch = Wp; a.act_plane = (long long)Hp * Wp;
        a.vh_x = x; a.vh_w = w1; a.vh_b = b1; a.vh_ci = Cin; a.vh_mode = 1;
        if (int rc = launch_channel_mix2(a, s)) return rc;
    }
    // 2. g_h = (w0^T gz) * gelu'(h)
    {
        ChannelMixArgs a{};
        a.x = gz; a.w = w0; a.y = gh; a.B = B; a.Ci = Co; a.Co = Cm; a.C1 = Co; a.Co1 = Cm; a.P = P; a.transpose_w = 1;
        a.vh_x = x; a.vh_w = w1; a.vh_b = b1; a.vh_ci = Cin; a.vh_mode = 2;
        if (int rc = launch_channel_mix2(a, s)) return rc;
    }
    // 3. fc0's weight / bias gradient: gz x gelu(h)^T;  4. fc_n1's: g_h x x^T
    if (int rc = launch_channel_wgrad_vh(gz, x, w1, b1, Cin, gw0, gb0, wws, B, Cm, Co, P, 1, s, 0)) return rc;
    return launch_channel_wgrad2(gh, x, nullptr, Cin, gw1, gb1, wws, B, Cin, Cm, P, 0, 0, 0, s);
}

long long uno_channel_wgrad_ws_bytes(int B, int Ci, int Co, long long P) {
    if (B < 1 || Ci < 1 || Co < 1 || P < 1) return 0;
    return 4LL * channel_wgrad_ws_floats(B, Ci, Co, P, nullptr);
}

static int channel_wgrad_impl(const void* gy, const void* x, float* gw, float* gb, void* ws, int B, int Ci, int Co, long long P,
                              int act_x, int bf16, void* stream) {
    if (B < 0 || Ci < 1 || Co < 1 || P < 0) { set_error("uno_channel_wgrad: bad sizes B=%d Ci=%d Co=%d P=%lld", B, Ci, Co, P); return -1; }
    if (!gw) { set_error("uno_channel_wgrad: null pointer"); return -1; }
    if (B == 0 || P == 0) {
        if (hipMemsetAsync(gw, 0, sizeof(float) * Co * Ci, (hipStream_t)stream) != hipSuccess ||
            (gb && hipMemsetAsync(gb, 0, sizeof(float) * Co, (hipStream_t)stream) != hipSuccess)) { set_error("uno_channel_wgrad: memset failed"); return -5; }
        return 0;
    }
    if (!gy || !x || !ws) { set_error("uno_channel_wgrad: null pointer"); return -1; }
    return launch_channel_wgrad(gy, x, gw, gb, (float*)ws, B, Ci, Co, P, act_x, bf16, (hipStream_t)stream);
}

int uno_channel_wgrad(const float* gy, const float* x, float* gw, float* gb, void* ws, int B, int Ci, int Co, long long P,
                      int act_x, void* stream) {
    return channel_wgrad_impl(gy, x, gw, gb, ws, B, Ci, Co, P, act_x, 0, stream);
}

int uno_channel_wgrad_bf16(const void* gy, const void* x, float* gw, float* gb, void* ws, int B, int Ci, int Co, long long P,
                           int act_x, void* stream) {
    return channel_wgrad_impl(gy, x, gw, gb, ws, B, Ci, Co, P, act_x, 1, stream);
}

static int channel_wgrad2_impl(const void* gy, const void* x1, const void* x2, int C1, float* gw, float* gb, void* ws, int B, int Ci,
                               int Co, long long P, int act_x, int accumulate, int bf16, void* stream, const PixelWindow& win = PixelWindow()) {
    if (B < 0 || Ci < 1 || Co < 1 || P < 0) { set_error("uno_channel_wgrad2: bad sizes B=%d Ci=%d Co=%d P=%lld", B, Ci, Co, P); return -1; }
    if (accumulate < 0 || accumulate > 3 || accumulate == 2) { set_error("uno_channel_wgrad2: accumulate is 0, 1 or 3 (got %d)", accumulate); return -1; }
    if (!gw && accumulate != 3) { set_error("uno_channel_wgrad2: null pointer"); return -1; }
    if (B == 0 || P == 0) {
        if (accumulate == 3) {      // an empty call's partial sums are zeros
            if (!ws) { set_error("uno_channel_wgrad2: null pointer"); return -1; }
            if (hipMemsetAsync(ws, 0, uno_channel_wgrad_ws_bytes(B, Ci, Co, P), (hipStream_t)stream) != hipSuccess) { set_error("uno_channel_wgrad2: memset failed"); return -5; }
            return 0;
        }
        if (accumulate) return 0;
        if (hipMemsetAsync(gw, 0, sizeof(float) * Co * Ci, (hipStream_t)stream) != hipSuccess ||
            (gb && hipMemsetAsync(gb, 0, sizeof(float) * Co, (hipStream_t)stream) != hipSuccess)) { set_error("uno_channel_wgrad2: memset failed"); return -5; }
        return 0;
    }
    if (!gy || !x1 || !ws) { set_error("uno_channel_wgrad2: null pointer"); return -1; }
    return launch_channel_wgrad2(gy, x1, x2, x2 ? C1 : Ci, gw, gb, (float*)ws, B, Ci, Co, P, act_x, accumulate, bf16, (hipStream_t)stream, win);
}

int uno_channel_wgrad2_win(const float* gy, const float* x1, const float* x2, int C1, float* gw, float* gb, void* ws, int B, int Ci, int Co,
                           int rows, int cols, int pitch, long long plane, int act_x, int accumulate, void* stream) {
    PixelWindow win; long long P;
    if (!make_window("uno_channel_wgrad2_win", rows, cols, pitch, plane, &win, &P)) return -1;
    return channel_wgrad2_impl(gy, x1, x2, C1, gw, gb, ws, B, Ci, Co, P, act_x, accumulate, 0, stream, win);
}

int uno_channel_wgrad2(const float* gy, const float* x1, const float* x2, int C1, float* gw, float* gb, void* ws, int B, int Ci, int Co,
                       long long P, int act_x, int accumulate, void* stream) {
    return channel_wgrad2_impl(gy, x1, x2, C1, gw, gb, ws, B, Ci, Co, P, act_x, accumulate, 0, stream);
}

int uno_channel_wgrad2_bf16(const void* gy, const void* x1, const void* x2, int C1, float* gw, float* gb, void* ws, int B, int Ci, int Co,
                            long long P, int act_x, int accumulate, void* stream) {
    return channel_wgrad2_impl(gy, x1, x2, C1, gw, gb, ws, B, Ci, Co, P, act_x, accumulate, 1, stream);
}

int uno_channel_wgrad_finish(const void* parts, float* gw, float* gb, int Ci, int Co, long long nparts, int accumulate, void* stream) {
    if (Ci < 1 || Co < 1 || nparts < 1) { set_error("uno_channel_wgrad_finish: bad sizes Ci=%d Co=%d blocks=%lld", Ci, Co, nparts); return -1; }
    if (!parts || !gw) { set_error("uno_channel_wgrad_finish: null pointer"); return -1; }
    return launch_channel_wgrad_finish((const float*)parts, gw, gb, Ci, Co, nparts, accumulate, (hipStream_t)stream);
}

int uno_adam_step(float* p, const float* g, float* m, float* v, long long n, int is_complex, double lr, double beta1, double beta2,
                  double eps, double weight_decay, int step, void* stream) {
    if (n < 0 || step < 1 || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) {
        set_error("uno_adam_step: bad arguments n=%lld step=%d betas=(%g, %g)", n, step, beta1, beta2);
        return -1;
    }
    if (n == 0) return 0;
    if (!p || !g || !m || !v) { set_error("uno_adam_step: null pointer"); return -1; }
    return launch_adam(p, g, m, v, n, is_complex, lr, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
}

int uno_adam_step_multi(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                        const long long* n, const int* is_complex, double lr, double beta1, double beta2, double eps,
                        double weight_decay, int step, void* stream) {
    if (n_tensors < 0 || (n_tensors > 0 && (!p || !g || !m || !v || !n || !is_complex))) {
        set_error("uno_adam_step_multi: bad arguments");
        return -1;
    }
    if (step < 1 || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) {
        set_error("uno_adam_step_multi: bad arguments step=%d betas=(%g, %g)", step, beta1, beta2);
        return -1;
    }
    for (int t = 0; t < n_tensors; ++t) {
        if (n[t] < 0) { set_error("uno_adam_step_multi: tensor %d has n=%lld", t, n[t]); return -1; }
        if (n[t] > 0 && (!p[t] || !g[t] || !m[t] || !v[t])) { set_error("uno_adam_step_multi: null pointer (tensor %d)", t); return -1; }
    }
    // one launch per 24 tensors (csrc/adam.hip): the tensors' descriptors travel in the kernel arguments
    return launch_adam_multi(n_tensors, p, g, m, v, n, is_complex, lr, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
}

int uno_adam_step_multi_dev(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                            const long long* n, const int* is_complex, double lr, double beta1, double beta2, double eps,
                            double weight_decay, int* step_counter, float* scalars, const double* hyper, void* stream) {
    if (n_tensors < 0 || (n_tensors > 0 && (!p || !g || !m || !v || !n || !is_complex)) || !step_counter || !scalars) {
        set_error("uno_adam_step_multi_dev: bad arguments");
        return -1;
    }
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) { set_error("uno_adam_step_multi_dev: bad betas (%g, %g)", beta1, beta2); return -1; }
    for (int t = 0; t < n_tensors; ++t) {
        if (n[t] < 0) { set_error("uno_adam_step_multi_dev: tensor %d has n=%lld", t, n[t]); return -1; }
        if (n[t] > 0 && (!p[t] || !g[t] || !m[t] || !v[t])) { set_error("uno_adam_step_multi_dev: null pointer (tensor %d)", t); return -1; }
    }
    if (int rc = launch_adam_advance(step_counter, scalars, hyper, lr, eps, weight_decay, beta1, beta2, (hipStream_t)stream)) return rc;
    return launch_adam_multi(n_tensors, p, g, m, v, n, is_complex, lr, beta1, beta2, eps, weight_decay, 1, (hipStream_t)stream, scalars);
}

static int grad_norm_tables_ok(const char* who, int n_tensors, const long long* n, const int* is_complex) {
    if (n_tensors < 0 || (n_tensors > 0 && (!n || !is_complex))) { set_error("%s: bad arguments", who); return 0; }
    for (int t = 0; t < n_tensors; ++t)
        if (n[t] < 0 || n[t] > (1LL << 60)) { set_error("%s: tensor %d has n=%lld", who, t, n[t]); return 0; }
    return 1;
}

long long uno_grad_norm_ws_bytes(int n_tensors, const long long* n, const int* is_complex) {
    if (!grad_norm_tables_ok("uno_grad_norm_ws_bytes", n_tensors, n, is_complex)) return -1;
    return 8 * grad_norm_partials(n_tensors, n, is_complex);
}

int uno_grad_norm(int n_tensors, const float* const* g, const long long* n, const int* is_complex, const double* max_norm,
                  int skip_nonfinite, double* ws, long long ws_bytes, double* state, void* stream) {
    if (!grad_norm_tables_ok("uno_grad_norm", n_tensors, n, is_complex)) return -1;
    if ((n_tensors > 0 && !g) || !max_norm || !state) { set_error("uno_grad_norm: null pointer"); return -1; }
    for (int t = 0; t < n_tensors; ++t)
        if (n[t] > 0 && !g[t]) { set_error("uno_grad_norm: null pointer (tensor %d)", t); return -1; }
    const long long need = 8 * grad_norm_partials(n_tensors, n, is_complex);
    if (ws_bytes < need || (need > 0 && !ws)) { set_error("uno_grad_norm: workspace of %lld bytes, %lld needed", ws_bytes, need); return -1; }
    return launch_grad_norm(n_tensors, g, n, is_complex, max_norm, skip_nonfinite, ws, state, (hipStream_t)stream);
}

int uno_adam_step_multi_guarded(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                                const long long* n, const int* is_complex, double lr, double beta1, double beta2, double eps,
                                double weight_decay, int* step_counter, float* scalars, const double* hyper, const double* clip_state,
                                int skip_nonfinite, void* stream) {
    if (n_tensors < 0 || (n_tensors > 0 && (!p || !g || !m || !v || !n || !is_complex)) || !step_counter || !scalars || !clip_state) {
        set_error("uno_adam_step_multi_guarded: bad arguments");
        return -1;
    }
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) { set_error("uno_adam_step_multi_guarded: bad betas (%g, %g)", beta1, beta2); return -1; }
    for (int t = 0; t < n_tensors; ++t) {
        if (n[t] < 0) { set_error("uno_adam_step_multi_guarded: tensor %d has n=%lld", t, n[t]); return -1; }
        if (n[t] > 0 && (!p[t] || !g[t] || !m[t] || !v[t])) { set_error("uno_adam_step_multi_guarded: null pointer (tensor %d)", t); return -1; }
    }
    const int skip = skip_nonfinite ? 1 : 0;
    if (int rc = launch_adam_advance(step_counter, scalars, hyper, lr, eps, weight_decay, beta1, beta2, (hipStream_t)stream, clip_state, skip)) return rc;
    return launch_adam_multi(n_tensors, p, g, m, v, n, is_complex, lr, beta1, beta2, eps, weight_decay, 1, (hipStream_t)stream, scalars, clip_state, skip);
}

static int gelu_project_forward_impl(const void* pre, const float* w, const float* bias, void* out, int B, int C, long long P, int bf16, void* stream) {
    if (B < 0 || C < 1 || P < 0) { set_error("uno_gelu_project_forward: bad sizes B=%d C=%d P=%lld", B, C, P); return -1; }
    if (B == 0 || P == 0) return 0;
    if (!pre || !w || !out) { set_error("uno_gelu_project_forward: null pointer"); return -1; }
    return launch_gelu_project_fwd(pre, w, bias, out, B, C, P, bf16, (hipStream_t)stream);
}

int uno_gelu_project_forward(const float* pre, const float* w, const float* bias, float* out, int B, int C, long long P, void* stream) {
    return gelu_project_forward_impl(pre, w, bias, out, B, C, P, 0, stream);
}

int uno_gelu_project_forward_bf16(const void* pre, const float* w, const float* bias, void* out, int B, int C, long long P, void* stream) {
    return gelu_project_forward_impl(pre, w, bias, out, B, C, P, 1, stream);
}

long long uno_gelu_project_bwd_ws_bytes(int B, int C, long long P) {
    if (B < 1 || C < 1 || P < 1) return 0;
    return 4LL * gelu_project_ws_floats(B, C, P);
}

static int gelu_project_backward_impl(const void* pre, const float* w, const void* gout, void* gpre, float* gw, float* gb, void* ws, int B,
                                      int C, long long P, int bf16, void* stream, const PixelWindow& win = PixelWindow()) {
    if (B < 0 || C < 1 || P < 0) { set_error("uno_gelu_project_backward: bad sizes B=%d C=%d P=%lld", B, C, P); return -1; }
    if (!gw) { set_error("uno_gelu_project_backward: null pointer"); return -1; }
    if (B == 0 || P == 0) {
        if (hipMemsetAsync(gw, 0, sizeof(float) * C, (hipStream_t)stream) != hipSuccess ||
            (gb && hipMemsetAsync(gb, 0, sizeof(float), (hipStream_t)stream) != hipSuccess)) { set_error("uno_gelu_project_backward: memset failed"); return -5; }
        return 0;
    }
    if (!pre || !w || !gout || !gpre || !ws) { set_error("uno_gelu_project_backward: null pointer"); return -1; }
    return launch_gelu_project_bwd(pre, w, gout, gpre, gw, gb, (float*)ws, B, C, P, bf16, (hipStream_t)stream, win);
}

int uno_gelu_project_backward_win(const float* pre, const float* w, const float* gout, float* gpre, float* gw, float* gb, void* ws, int B,
                                  int C, int rows, int cols, int pitch, long long plane, void* stream) {
    PixelWindow win; long long P;
    if (!make_window("uno_gelu_project_backward_win", rows, cols, pitch, plane, &win, &P)) return -1;
    return gelu_project_backward_impl(pre, w, gout, gpre, gw, gb, ws, B, C, P, 0, stream, win);
}

int uno_gelu_project_backward(const float* pre, const float* w, const float* gout, float* gpre, float* gw, float* gb, void* ws, int B,
                              int C, long long P, void* stream) {
    return gelu_project_backward_impl(pre, w, gout, gpre, gw, gb, ws, B, C, P, 0, stream);
}

int uno_gelu_project_backward_bf16(const void* pre, const float* w, const void* gout, void* gpre, float* gw, float* gb, void* ws, int B,
                                   int C, long long P, void* stream) {
    return gelu_project_backward_impl(pre, w, gout, gpre, gw, gb, ws, B, C, P, 1, stream);
}

// two-source form of K11 (float32, dense): entries [0, C1) of w go with gelu(pre), entries [C1, C1 + C2) with s (gelu(s) when act2)
static bool gelu_project2_sizes(const char* who, int B, int C1, int C2, long long P, int act2) {
    if (B < 0 || C1 < 1 || C2 < 1 || P < 0) { set_error("%s: bad sizes B=%d C1=%d C2=%d P=%lld", who, B, C1, C2, P); return false; }
    if ((long long)C1 + C2 > 1024) { set_error("%s: C1 + C2 = %lld channels, at most 1024", who, (long long)C1 + C2); return false; }
    if (act2 != 0 && act2 != 1) { set_error("%s: act2 is 0 or 1 (got %d)", who, act2); return false; }
    return true;
}

int uno_gelu_project2_forward(const float* pre, const float* s, const float* w, const float* bias, float* out, int B, int C1, int C2,
                              long long P, int act2, void* stream) {
    if (!gelu_project2_sizes("uno_gelu_project2_forward", B, C1, C2, P, act2)) return -1;
    if (B == 0 || P == 0) return 0;
    if (!pre || !s || !w || !out) { set_error("uno_gelu_project2_forward: null pointer"); return -1; }
    GeluProjectSecond two;
    two.s = s; two.C1 = C1; two.act = act2;
    return launch_gelu_project_fwd(pre, w, bias, out, B, C1 + C2, P, 0, (hipStream_t)stream, &two);
}

long long uno_gelu_project2_bwd_ws_bytes(int B, int C1, int C2, long long P) {
    if (B < 1 || C1 < 1 || C2 < 1 || P < 1 || (long long)C1 + C2 > 1024) return 0;
    return 4LL * gelu_project_ws_floats(B, C1 + C2, P);
}

int uno_gelu_project2_backward(const float* pre, const float* s, const float* w, const float* gout, float* gpre, float* gs, float* gw,
                               float* gb, void* ws, int B, int C1, int C2, long long P, int act2, void* stream) {
    if (!gelu_project2_sizes("uno_gelu_project2_backward", B, C1, C2, P, act2)) return -1;
    if (!gw) { set_error("uno_gelu_project2_backward: null pointer"); return -1; }
    if (B == 0 || P == 0) {
        if (hipMemsetAsync(gw, 0, sizeof(float) * (C1 + C2), (hipStream_t)stream) != hipSuccess ||
            (gb && hipMemsetAsync(gb, 0, sizeof(float), (hipStream_t)stream) != hipSuccess)) { set_error("uno_gelu_project2_backward: memset failed"); return -5; }
        return 0;
    }
    if (!pre || !s || !w || !gout || !gpre || !ws) { set_error("uno_gelu_project2_backward: null pointer"); return -1; }
    GeluProjectSecond two;
    two.s = s; two.gs = gs; two.C1 = C1; two.act = act2;
    return launch_gelu_project_bwd(pre, w, gout, gpre, gw, gb, (float*)ws, B, C1 + C2, P, 0, (hipStream_t)stream, PixelWindow(), &two);
}

// K17: per-time-step relative L2 error (forward only), dense float32 (B, P, T)
static bool rel_l2_steps_sizes(const char* who, int B, long long P, int T) {
    if (B < 0 || P < 1 || T < 1) { set_error("%s: bad sizes B=%d P=%lld T=%d", who, B, P, T); return false; }
    if (T > 256) { set_error("%s: T = %d time steps, at most 256", who, T); return false; }
    return true;
}

long long uno_rel_l2_steps_ws_bytes(int B, long long P, int T) {
    if (B < 1 || P < 1 || T < 1 || T > 256) return 0;
    return 4LL * rel_l2_steps_ws_floats(B, P, T);
}

int uno_rel_l2_steps(const float* pred, const float* target, float* sums, float* rel, float* totals, void* ws, int B, long long P, int T,
                     void* stream) {
    if (!rel_l2_steps_sizes("uno_rel_l2_steps", B, P, T)) return -1;
    if (B == 0) return 0;
    if (!pred || !target || !sums || !rel || !totals || !ws) { set_error("uno_rel_l2_steps: null pointer"); return -1; }
    return launch_rel_l2_steps(pred, target, sums, rel, totals, (float*)ws, B, P, T, (hipStream_t)stream);
}

int uno_rel_l2_steps_backward(const float* pred, const float* target, const float* sums, const float* g_full, const float* g_step, float* gx,
                              int B, long long P, int T, void* stream) {
    if (!rel_l2_steps_sizes("uno_rel_l2_steps_backward", B, P, T)) return -1;
    if (B == 0) return 0;
    if (!pred || !target || !sums || !gx) { set_error("uno_rel_l2_steps_backward: null pointer"); return -1; }
    return launch_rel_l2_steps_backward(pred, target, sums, g_full, g_step, gx, B, P, T, (hipStream_t)stream);
}

// K20: the relative L2 training loss and its gradient, float32 (B, N) views with a row stride and an element stride each
static bool rel_l2_sizes(const char* who, int B, long long N, long long xrs, long long xes, long long yrs, long long yes) {
    if (B < 0 || N < 1) { set_error("%s: bad sizes B=%d N=%lld", who, B, N); return false; }
    if (xrs < 0 || xes < 0 || yrs < 0 || yes < 0) {
        set_error("%s: bad strides x (%lld, %lld) y (%lld, %lld): none may be negative", who, xrs, xes, yrs, yes);
        return false;
    }
    return true;
}

long long uno_rel_l2_ws_bytes(int B, long long N) {
    if (B < 1 || N < 1) return 0;
    return 4LL * rel_l2_ws_floats(B, N);
}

int uno_rel_l2_forward(const float* x, long long x_row, long long x_elem, const float* y, long long y_row, long long y_elem, float* sums,
                       float* ratio, float* total, void* ws, int B, long long N, void* stream) {
    if (!rel_l2_sizes("uno_rel_l2_forward", B, N, x_row, x_elem, y_row, y_elem)) return -1;
    if (B == 0) return 0;
    if (!x || !y || !sums || !ratio || !total || !ws) { set_error("uno_rel_l2_forward: null pointer"); return -1; }
    return launch_rel_l2_forward(x, x_row, x_elem, y, y_row, y_elem, sums, ratio, total, (float*)ws, B, N, (hipStream_t)stream);
}

int uno_rel_l2_backward(const float* x, long long x_row, long long x_elem, const float* y, long long y_row, long long y_elem, const float* sums,
                        const float* g, int g_per_row, float scale, float* gx, int B, long long N, void* stream) {
    if (!rel_l2_sizes("uno_rel_l2_backward", B, N, x_row, x_elem, y_row, y_elem)) return -1;
    if (g_per_row != 0 && g_per_row != 1) { set_error("uno_rel_l2_backward: g_per_row = %d, 0 (one scalar) or 1 (one per row)", g_per_row); return -1; }
    if (B == 0) return 0;
    if (!x || !y || !sums || !g || !gx) { set_error("uno_rel_l2_backward: null pointer"); return -1; }
    return launch_rel_l2_backward(x, x_row, x_elem, y, y_row, y_elem, sums, g, g_per_row, scale, gx, B, N, (hipStream_t)stream);
}

// K24: shell-binned energy spectra of strided float32 frames (forward only)
static bool shell_spectrum_sizes(int B, int T, int H, int W) { return B >= 0 && T >= 1 && H >= 8 && H <= 512 && W >= 8 && W <= 512; }

long long uno_shell_spectrum_ws_bytes(int B, int T, int H, int W, int with_target) {
    if (!shell_spectrum_sizes(B, T, H, W) || B < 1) return 0;
    return 4LL * shell_spectrum_ws_floats(B, T, H, W, with_target);
}

int uno_shell_spectrum(const float* x, long long x_batch, long long x_frame, long long x_row, long long x_elem, const float* y, long long y_batch,
                       long long y_frame, long long y_row, long long y_elem, float* spec, void* ws, int B, int T, int H, int W, void* stream) {
    if (!shell_spectrum_sizes(B, T, H, W)) {
        set_error("uno_shell_spectrum: bad sizes B=%d T=%d H=%d W=%d (B >= 0, T >= 1, 8 <= H, W <= 512)", B, T, H, W);
        return -1;
    }
    const long long xs[4] = {x_batch, x_frame, x_row, x_elem}, ys[4] = {y_batch, y_frame, y_row, y_elem};
    for (int i = 0; i < 4; ++i)
        if (xs[i] < 0 || (y && ys[i] < 0)) {
            set_error("uno_shell_spectrum: bad strides x (%lld, %lld, %lld, %lld) y (%lld, %lld, %lld, %lld): none may be negative", xs[0], xs[1],
                      xs[2], xs[3], ys[0], ys[1], ys[2], ys[3]);
            return -1;
        }
    if (B == 0) return 0;
    if (!x || !spec || !ws) { set_error("uno_shell_spectrum: null pointer"); return -1; }
    return launch_shell_spectrum(x, xs, y, ys, spec, (float*)ws, B, T, H, W, (hipStream_t)stream);
}

// K25: the relative Sobolev loss of strided float32 frames and its gradient
static bool sobolev_sizes(const char* who, int B, int T, int H, int W) {
    if (B >= 0 && T >= 1 && H >= 8 && H <= 512 && W >= 8 && W <= 512) return true;
    set_error("%s: bad sizes B=%d T=%d H=%d W=%d (B >= 0, T >= 1, 8 <= H, W <= 512)", who, B, T, H, W);
    return false;
}

long long uno_sobolev_ws_bytes(int B, int T, int H, int W) {
    if (B < 1 || T < 1 || H < 8 || H > 512 || W < 8 || W > 512) return 0;
    return 4LL * sobolev_ws_floats(B, T, W);
}

int uno_sobolev_forward(const float* x, long long x_batch, long long x_frame, long long x_row, long long x_elem, const float* y, long long y_batch,
                        long long y_frame, long long y_row, long long y_elem, const float* w2, float* sums, float* ratio, float* total, void* z,
                        void* ws, int B, int T, int H, int W, int per_frame, void* stream) {
    if (!sobolev_sizes("uno_sobolev_forward", B, T, H, W)) return -1;
    if (per_frame != 0 && per_frame != 1) { set_error("uno_sobolev_forward: per_frame = %d, 0 (one ratio per sample) or 1 (one per frame)", per_frame); return -1; }
    const long long xs[4] = {x_batch, x_frame, x_row, x_elem}, ys[4] = {y_batch, y_frame, y_row, y_elem};
    for (int i = 0; i < 4; ++i)
        if (xs[i] < 0 || ys[i] < 0) {
            set_error("uno_sobolev_forward: bad strides x (%lld, %lld, %lld, %lld) y (%lld, %lld, %lld, %lld): none may be negative", xs[0], xs[1],
                      xs[2], xs[3], ys[0], ys[1], ys[2], ys[3]);
            return -1;
        }
    if (B == 0) return 0;
    if (!x || !y || !w2 || !sums || !ratio || !total || !ws) { set_error("uno_sobolev_forward: null pointer"); return -1; }
    return launch_sobolev_forward(x, xs, y, ys, w2, sums, ratio, total, (float*)z, (float*)ws, B, T, H, W, per_frame, (hipStream_t)stream);
}

int uno_sobolev_backward(const void* z, const float* sums, const float* g, int g_per_row, float scale, int per_frame, float* gx, long long gx_batch,
                         long long gx_frame, long long gx_row, long long gx_elem, int B, int T, int H, int W, void* stream) {
    if (!sobolev_sizes("uno_sobolev_backward", B, T, H, W)) return -1;
    if (g_per_row != 0 && g_per_row != 1) { set_error("uno_sobolev_backward: g_per_row = %d, 0 (one scalar) or 1 (one per row)", g_per_row); return -1; }
    if (per_frame != 0 && per_frame != 1) { set_error("uno_sobolev_backward: per_frame = %d, 0 (one ratio per sample) or 1 (one per frame)", per_frame); return -1; }
    const long long gs[4] = {gx_batch, gx_frame, gx_row, gx_elem};
    for (int i = 0; i < 4; ++i)
        if (gs[i] < 0) {
            set_error("uno_sobolev_backward: bad strides gx (%lld, %lld, %lld, %lld): none may be negative", gs[0], gs[1], gs[2], gs[3]);
            return -1;
        }
    if (B == 0) return 0;
    if (!z || !sums || !g || !gx) { set_error("uno_sobolev_backward: null pointer"); return -1; }
    return launch_sobolev_backward((const float*)z, sums, g, g_per_row, scale, per_frame, gx, gs, B, T, H, W, (hipStream_t)stream);
}

// K18: one step of the NS-2D evaluation roll-out (forward only), dense float32; the finish launch is K17's
static bool rollout_sizes(const char* who, int B, long long P, int T) {
    if (B < 0 || P < 1 || T < 1) { set_error("%s: bad sizes B=%d P=%lld T=%d", who, B, P, T); return false; }
    if (T > 256) { set_error("%s: T = %d time steps, at most 256", who, T); return false; }
    return true;
}

long long uno_rollout_ws_bytes(int B, long long P, int T) {
    if (B < 1 || P < 1 || T < 1 || T > 256) return 0;
    return 4LL * rollout_ws_floats(B, P, T);
}

int uno_rollout_advance(float* window, const float* frame, const float* target, float* pred, void* ws, int B, int C, int T_in, long long P,
                        int T, int t, int shift, void* stream) {
    // target == NULL together with ws == NULL: the pass without sums (a free-running roll-out); T is then pred's time length only and
    // the finish kernel's cap of 256 steps does not apply to it
    if (!target != !ws) {
        set_error("uno_rollout_advance: null %s beside %s (target and ws go together: both, or neither for the pass without sums)",
                  target ? "ws" : "target", target ? "a target" : "a workspace");
        return -1;
    }
    if (target) { if (!rollout_sizes("uno_rollout_advance", B, P, T)) return -1; }
    else if (B < 0 || P < 1 || T < 1) { set_error("uno_rollout_advance: bad sizes B=%d P=%lld T=%d", B, P, T); return -1; }
    if (C < 1 || T_in < 1 || T_in > C || t < 0 || t >= T) {
        set_error("uno_rollout_advance: bad sizes C=%d T_in=%d (1 ... C) t=%d (0 ... T - 1 = %d)", C, T_in, t, T - 1);
        return -1;
    }
    if (!target && !pred && !shift) { set_error("uno_rollout_advance: without a target, pred or shift must ask for something"); return -1; }
    if (B == 0) return 0;
    if (!window || !frame) { set_error("uno_rollout_advance: null pointer"); return -1; }
    return launch_rollout_advance(window, frame, target, pred, (float*)ws, B, C, T_in, P, T, t, shift, (hipStream_t)stream);
}

int uno_rollout_finish(const void* ws, float* sums, float* rel, float* totals, int B, long long P, int T, void* stream) {
    if (!rollout_sizes("uno_rollout_finish", B, P, T)) return -1;
    if (B == 0) return 0;
    if (!ws || !sums || !rel || !totals) { set_error("uno_rollout_finish: null pointer"); return -1; }
    return launch_rel_l2_steps_finish((const float*)ws, sums, rel, totals, B, T, rollout_chunks(P, nullptr), (hipStream_t)stream);
}

// K19 / K19-B: the first lift of the NS-2D training roll-out and its backward (rollout_train.hip), dense float32
static bool rollout_lift_sizes(const char* who, int B, int T_in, int F, int Cm, long long P, int T) {
    if (!rollout_sizes(who, B, P, T)) return false;
    if (T_in < 1 || F < 0 || Cm < 1) { set_error("%s: bad sizes T_in=%d F=%d Cm=%d", who, T_in, F, Cm); return false; }
    if (T_in > 32 || F > 32 || T_in + F > 32 || Cm > 64) {
        set_error("%s: C = T_in + F = %d + %d input channels (at most 32), Cm = %d lifted channels (at most 64)", who, T_in, F, Cm);
        return false;
    }
    return true;
}

int uno_rollout_lift(const float* given, const float* pred, const float* feat, const float* w, const float* bias, float* h, int B, int T_in,
                     int F, int Cm, long long P, int T, int t, void* stream) {
    if (!rollout_lift_sizes("uno_rollout_lift", B, T_in, F, Cm, P, T)) return -1;
    if (t < 0 || t >= T) { set_error("uno_rollout_lift: bad sizes t=%d (0 ... T - 1 = %d)", t, T - 1); return -1; }
    if (B == 0) return 0;
    if (!given || (t > 0 && !pred) || (F > 0 && !feat) || !w || !h) { set_error("uno_rollout_lift: null pointer"); return -1; }
    return launch_rollout_lift(given, pred, feat, w, bias, h, B, T_in, F, Cm, P, T, t, (hipStream_t)stream);
}

long long uno_rollout_lift_bwd_ws_bytes(int B, int T_in, int F, int Cm, long long P, int T) {
    if (B < 1 || P < 1 || T < 1 || T > 256 || T_in < 1 || F < 0 || T_in > 32 || F > 32 || T_in + F > 32 || Cm < 1 || Cm > 64) return 0;
    return 4LL * rollout_lift_bwd_ws_floats(B, T_in + F, Cm, P, T);
}

int uno_rollout_lift_backward(const float* gh, const float* given, const float* pred, const float* target, const float* feat, const float* w,
                              const float* sums, const float* gL, float* gpred, float* gframe, void* parts, int B, int T_in, int F, int Cm,
                              long long P, int T, int t, void* stream) {
    if (!rollout_lift_sizes("uno_rollout_lift_backward", B, T_in, F, Cm, P, T)) return -1;
    if (t < 0 || t >= T) { set_error("uno_rollout_lift_backward: bad sizes t=%d (0 ... T - 1 = %d)", t, T - 1); return -1; }
    if (B == 0) return 0;
    if (!gh || !given || (F > 0 && !feat) || !w || !parts || (t > 0 && (!pred || !target || !sums || !gL || !gpred || !gframe))) {
        set_error("uno_rollout_lift_backward: null pointer");
        return -1;
    }
    return launch_rollout_lift_backward(gh, given, pred, target, feat, w, sums, gL, gpred, gframe, (float*)parts, B, T_in, F, Cm, P, T, t,
                                        (hipStream_t)stream);
}

int uno_rollout_loss_seed(const float* pred, const float* target, const float* sums, const float* gL, float* gframe, int B, long long P, int T,
                          void* stream) {
    if (!rollout_sizes("uno_rollout_loss_seed", B, P, T)) return -1;
    if (B == 0) return 0;
    if (!pred || !target || !sums || !gL || !gframe) { set_error("uno_rollout_loss_seed: null pointer"); return -1; }
    return launch_rollout_loss_seed(pred, target, sums, gL, gframe, B, P, T, (hipStream_t)stream);
}

static int gelu_pad_impl(const void* s, const void* gy, void* out, int n_img, int H, int W, int Hp, int Wp, int backward, int bf16, void* stream) {
    if (n_img < 0 || H < 1 || W < 1 || Hp < H || Wp < W) { set_error("uno_gelu_pad: bad sizes (%d, %d) -> (%d, %d)", H, W, Hp, Wp); return -1; }
    if (n_img == 0) return 0;
    if (!s || !out || (backward && !gy)) { set_error("uno_gelu_pad: null pointer"); return -1; }
    return launch_gelu_pad(s, gy, out, n_img, H, W, Hp, Wp, backward, bf16, (hipStream_t)stream);
}

int uno_gelu_pad(const float* s, const float* gy, float* out, int n_img, int H, int W, int Hp, int Wp, int backward, void* stream) {
    return gelu_pad_impl(s, gy, out, n_img, H, W, Hp, Wp, backward, 0, stream);
}

int uno_gelu_pad_bf16(const void* s, const void* gy, void* out, int n_img, int H, int W, int Hp, int Wp, int backward, void* stream) {
    return gelu_pad_impl(s, gy, out, n_img, H, W, Hp, Wp, backward, 1, stream);
}

int uno_transpose_batched(const float* in, float* out, int B, long long R, int C, long long ld_in, long long sb_in, long long ld_out,
                          long long sb_out, void* stream) {
    if (B < 0 || R < 0 || C < 0 || ld_in < C || ld_out < R || sb_in < 0 || sb_out < 0) {
        set_error("uno_transpose_batched: bad sizes (B %d, R %lld, C %d, pitches %lld / %lld)", B, R, C, ld_in, ld_out);
        return -1;
    }
    if (B == 0 || R == 0 || C == 0) return 0;
    if (!in || !out) { set_error("uno_transpose_batched: null pointer"); return -1; }
    return launch_transpose_batched(in, out, B, R, C, ld_in, sb_in, ld_out, sb_out, (hipStream_t)stream);
}

static int instnorm_forward_impl(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, long long rows, int C,
                                 long long N, float eps, int gelu, int bf16, void* stream) {
    if (rows < 0 || C < 1 || N < 1 || (rows % C) != 0) { set_error("uno_instnorm_forward: bad sizes rows=%lld C=%d N=%lld", rows, C, N); return -1; }
    if (rows == 0) return 0;
    if (!x || !y || !mean || !rstd) { set_error("uno_instnorm_forward: null pointer"); return -1; }
    return launch_instnorm_fwd(x, gamma, beta, y, mean, rstd, rows, C, N, eps, gelu, bf16, (hipStream_t)stream);
}

int uno_instnorm_forward(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long long rows, int C,
                         long long N, float eps, int gelu, void* stream) {
    return instnorm_forward_impl(x, gamma, beta, y, mean, rstd, rows, C, N, eps, gelu, 0, stream);
}

int uno_instnorm_forward_bf16(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, long long rows, int C,
                              long long N, float eps, int gelu, void* stream) {
    return instnorm_forward_impl(x, gamma, beta, y, mean, rstd, rows, C, N, eps, gelu, 1, stream);
}

static int instnorm_backward_impl(const void* x, const void* gy, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                  void* gx, float* s1, float* s2, long long rows, int C, long long N, int gelu, int bf16, void* stream) {
    if (rows < 0 || C < 1 || N < 1 || (rows % C) != 0) { set_error("uno_instnorm_backward: bad sizes rows=%lld C=%d N=%lld", rows, C, N); return -1; }
    if (rows == 0) return 0;
    if (!x || !gy || !mean || !rstd || !gx || !s1 || !s2) { set_error("uno_instnorm_backward: null pointer"); return -1; }
    return launch_instnorm_bwd(x, gy, gamma, beta, mean, rstd, gx, s1, s2, rows, C, N, gelu, bf16, (hipStream_t)stream);
}

int uno_instnorm_backward(const float* x, const float* gy, const float* gamma, const float* beta, const float* mean, const float* rstd,
                          float* gx, float* s1, float* s2, long long rows, int C, long long N, int gelu, void* stream) {
    return instnorm_backward_impl(x, gy, gamma, beta, mean, rstd, gx, s1, s2, rows, C, N, gelu, 0, stream);
}

int uno_instnorm_backward_bf16(const void* x, const void* gy, const float* gamma, const float* beta, const float* mean, const float* rstd,
                               void* gx, float* s1, float* s2, long long rows, int C, long long N, int gelu, void* stream) {
    return instnorm_backward_impl(x, gy, gamma, beta, mean, rstd, gx, s1, s2, rows, C, N, gelu, 1, stream);
}

}  // extern "C"
