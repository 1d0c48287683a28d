// K1-FD: the instantiations of the forward transform that also writes the down-sampled image (dft2d_fwd_fd_kernel.h), one per mode-count
// class - the tap counts of the banded operators are run-time values, so the forward 2:1 operator and the adjoint of the 1:2
// up-sampling run the same code
#include "dft2d_fwd_fd_kernel.h"

namespace uno {

// (NT, MT, R4) of launch_dft2d_fwd's rule; the compiled classes: modes2 17..20 with modes1 17..24 (the 446^2 level of the Darcy model, and
// c0's shared transform on the 223^2 level), modes2 1..8 with modes1 <= 8; each with four output columns per lane (rows of 416..447
// floats) and with two (rows of 192..223 floats)
static bool fd_class(const Dft2dParams& p, int* NT, int* MT, int* R4) {
    if (p.m1 < 1 || p.m2 < 1 || p.m1 > 40 || p.m2 > 48) return false;
    *NT = (p.m2 + 15) / 16; *MT = (2 * p.m1 + 15) / 16;
    const int rem = p.m2 - 16 * (*NT - 1);
    if (rem > 8) return false;
    *R4 = (rem + 3) / 4;
    return (*NT == 2 && *MT == 3 && *R4 == 1) || (*NT == 1 && *MT == 1 && (*R4 == 1 || *R4 == 2));
}

bool dft2d_fwd_fd_applies(const Dft2dParams& p) {
    int NT, MT, R4;
    FwdFtGeometry g;
    return fd_class(p, &NT, &MT, &R4) && fwd_fd_geometry(p, NT, MT, R4, &g);
}

int launch_dft2d_fwd_fd(const Dft2dParams& p, hipStream_t s) {
    int NT, MT, R4;
    FwdFtGeometry g;
    if (!fd_class(p, &NT, &MT, &R4) || !fwd_fd_geometry(p, NT, MT, R4, &g)) { set_error("dft2d_fwd_fd: the form does not apply"); return -3; }
    if (fwd_fd_columns_per_lane(p.W) == FD_CE2) {       // the 223^2 level: two output columns per lane
        if (NT == 2) return launch_fwd_fd<2, 3, 1, FD_CE2>(p, g, s);
        return R4 == 1 ? launch_fwd_fd<1, 1, 1, FD_CE2>(p, g, s) : launch_fwd_fd<1, 1, 2, FD_CE2>(p, g, s);
    }
    if (NT == 2) return launch_fwd_fd<2, 3, 1>(p, g, s);
    return R4 == 1 ? launch_fwd_fd<1, 1, 1>(p, g, s) : launch_fwd_fd<1, 1, 2>(p, g, s);
}

}  // namespace uno
