// C ABI of libuno_spectral.so, the Darcy-flow data generator's entry points (K23, darcy_solver.hip): the two-sided plane transform, the
// 5-point operator alone and the preconditioned conjugate-gradient solve, with the workspace size.
#include "../../include/uno_spectral.h"
#include "uno_common.h"

#include <cmath>

namespace uno {

static bool darcy_size_ok(int K) { return K >= 8 && K <= 512; }

// sizes shared by the grid entry points; 0: fine
static int darcy_check(const char* who, int B, int K) {
    if (!darcy_size_ok(K)) { set_error("%s: K=%d must lie in 8 ... 512", who, K); return -1; }
    if (B < 0 || B > 65535) { set_error("%s: bad batch size %d (0 ... 65535)", who, B); return -1; }
    return 0;
}

}  // namespace uno

using namespace uno;

extern "C" {

long long uno_darcy_ws_bytes(int B, int K) { return (B < 0 || B > 65535 || !darcy_size_ok(K)) ? 0 : darcy_ws_bytes(B, K); }

int uno_darcy_table_pitch(int N) { return N < 1 || N > 512 ? 0 : darcy_table_pitch(N); }

// GRF.m:21 (idct2), solve_gwf.m:11-12, 35 (interp2 'spline' on uniform grids), and the solver's DST-I pair
int uno_darcy_transform(const void* M, const void* X, void* Y, void* tmp, const void* post, int B, int N, int f32, void* stream) {
    const char* who = "uno_darcy_transform";
    if (N < 1 || N > 512) { set_error("%s: N=%d must lie in 1 ... 512", who, N); return -1; }
    if (B < 0 || B > 65535) { set_error("%s: bad batch size %d (0 ... 65535)", who, B); return -1; }
    if (B == 0) return 0;
    if (!M || !X || !Y || !tmp) { set_error("%s: null pointer", who); return -1; }
    if (tmp == X || tmp == Y || X == Y) { set_error("%s: X, Y and tmp must be three different buffers", who); return -1; }
    return launch_darcy_transform(M, X, Y, tmp, post, nullptr, B, N, f32 ? 1 : 0, (hipStream_t)stream);
}

// solve_gwf.m:16-32 (the matrix A, applied and never formed)
int uno_darcy_apply(const double* coef, const double* p, double* Ap, int B, int K, void* stream) {
    if (int rc = darcy_check("uno_darcy_apply", B, K)) return rc;
    if (B == 0) return 0;
    if (!coef || !p || !Ap) { set_error("uno_darcy_apply: null pointer"); return -1; }
    if (p == Ap) { set_error("uno_darcy_apply: Ap must not alias p"); return -1; }
    return launch_darcy_apply(coef, p, Ap, B, K, (hipStream_t)stream);
}

// solve_gwf.m:14-33 (F(2:K-1,2:K-1), A, A\F(:) and the zero border)
int uno_darcy_solve(const double* coef, const double* F, double* P, int* iters, double* relres, int* status, void* ws, int B, int K,
                    double rtol, int max_iter, int check_every, void* stream) {
    const char* who = "uno_darcy_solve";
    if (int rc = darcy_check(who, B, K)) return rc;
    if (!(rtol > 0.0) || !std::isfinite(rtol)) { set_error("%s: rtol=%g must be finite and positive", who, rtol); return -1; }
    if (max_iter < 1) { set_error("%s: max_iter=%d must be at least 1", who, max_iter); return -1; }
    if (check_every < 1) { set_error("%s: check_every=%d must be at least 1", who, check_every); return -1; }
    if (B == 0) return 0;
    if (!coef || !F || !P || !iters || !relres || !status || !ws) { set_error("%s: null pointer", who); return -1; }
    if (reinterpret_cast<uintptr_t>(ws) % 8) { set_error("%s: the workspace must be 8-byte aligned", who); return -1; }
    if (P == coef || P == F) { set_error("%s: P must not alias an input", who); return -1; }
    return launch_darcy_solve(coef, F, P, iters, relres, status, ws, B, K, rtol, max_iter, check_every, (hipStream_t)stream);
}

}  // extern "C"
