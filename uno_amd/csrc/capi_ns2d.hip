// C ABI of libuno_spectral.so, the data generator's entry points: the 2-D Navier-Stokes solver (K22, ns2d_solver.hip) and its workspace size.
#include "../../include/uno_spectral.h"
#include "uno_common.h"

#include <cmath>

namespace uno {

static bool ns2d_size_ok(int N) { return N >= 32 && N <= 256 && (N & (N - 1)) == 0; }

// sizes shared by the three entry points; 0: fine
static int ns2d_check(const char* who, int B, int N) {
    if (!ns2d_size_ok(N)) { set_error("%s: N=%d must be a power of two in 32 ... 256", who, N); return -1; }
    if (B < 0 || (long long)B * N > 0x7fffffffLL) { set_error("%s: bad batch size %d (0 ... 2^31 / N - 1)", who, B); return -1; }
    return 0;
}

}  // namespace uno

using namespace uno;

extern "C" {

long long uno_ns2d_ws_bytes(int B, int N) { return (B < 0 || !ns2d_size_ok(N)) ? 0 : ns2d_ws_bytes(B, N); }

// ns_datagen.py:26, 29
int uno_ns2d_forward(const float* w, float* w_h, void* ws, int B, int N, void* stream) {
    if (int rc = ns2d_check("uno_ns2d_forward", B, N)) return rc;
    if (B == 0) return 0;
    if (!w || !w_h || !ws) { set_error("uno_ns2d_forward: null pointer"); return -1; }
    return launch_ns2d_forward(w, w_h, ws, B, N, (hipStream_t)stream);
}

// ns_datagen.py:125-127
int uno_ns2d_inverse(const float* w_h, float* w, void* ws, int B, int N, void* stream) {
    if (int rc = ns2d_check("uno_ns2d_inverse", B, N)) return rc;
    if (B == 0) return 0;
    if (!w_h || !w || !ws) { set_error("uno_ns2d_inverse: null pointer"); return -1; }
    return launch_ns2d_inverse(w_h, w, ws, B, N, (hipStream_t)stream);
}

// ns_datagen.py:67-118
int uno_ns2d_steps(float* w_h, const float* f_h, int f_batched, void* ws, int B, int N, long long n_steps, double visc, double delta_t,
                   void* stream) {
    const char* who = "uno_ns2d_steps";
    if (int rc = ns2d_check(who, B, N)) return rc;
    if (n_steps < 0) { set_error("%s: negative step count %lld", who, n_steps); return -1; }
    if (!std::isfinite(delta_t) || delta_t <= 0.0) { set_error("%s: delta_t=%g must be finite and positive", who, delta_t); return -1; }
    if (!std::isfinite(visc) || visc < 0.0) { set_error("%s: visc=%g must be finite and not negative", who, visc); return -1; }
    if (B == 0 || n_steps == 0) return 0;
    if (!w_h || !f_h || !ws) { set_error("%s: null pointer", who); return -1; }
    if (f_h == w_h) { set_error("%s: f_h must not alias w_h", who); return -1; }
    return launch_ns2d_steps(w_h, f_h, f_batched, ws, B, N, n_steps, visc, delta_t, (hipStream_t)stream);
}

}  // extern "C"
