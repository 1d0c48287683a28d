// Twiddle-index arithmetic, the persistent launch geometry and the launch check of the plane-at-a-time kernels of pointwise_op_3D's FFT
// crop / resample (resample3d_planes.h: K1a / K5a / K3a and K1w / K5w / K3w), which ns2d_solver.hip uses too.
#pragma once
#include "uno_common.h"
#include <algorithm>

namespace uno {

constexpr int RA_THREADS = 256;

// ceil(2^32 / N): p / N == umulhi(p, magic) whenever p (magic N - 2^32) < 2^32.  magic N - 2^32 < N, so for every p < 2^32 / N: p < 2^25
// at N <= 128 and p < 2^24 at N <= 256.  The products taken here are (frequency < N) x (position < N): below 2^14 at N <= 128 (K3a /
// K5a), below 2^16 at N <= 256 (K3w / K5w).
__host__ __device__ __forceinline__ unsigned ra_magic(int N) { return 0xFFFFFFFFu / (unsigned)N + 1u; }
__device__ __forceinline__ int ra_mod(int f, int N) { f %= N; return f < 0 ? f + N : f; }       // table entries are the caller's: keep every twiddle index inside the table

// persistent grid: the usable CUs x the workgroups of RA_THREADS threads a CU holds beside each other at this LDS size (at most 8)
static int ra_grid(long long n_items, size_t lds) {
    const long long per_cu = std::max<long long>(1, std::min<long long>(8, (160 * 1024) / (long long)std::max<size_t>(lds, 1)));
    return (int)std::max<long long>(1, std::min<long long>(n_items, (long long)current_usable_cus() * per_cu));
}

static int ra_check(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s launch: %s", who, hipGetErrorString(e)); return -5; }
    return 0;
}

}  // namespace uno
