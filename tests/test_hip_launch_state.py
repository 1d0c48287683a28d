"""The two process-wide launch switches - the sweep direction (uno_sweep_alternation, csrc/uno_common.h: "only the ORDER changes") and the
compute units set aside for communication kernels (uno_reserve_cus, which feeds every device-sized launch geometry) - on the kernels that
read them.  pytest -m gpu

Direction: every family that takes a direction from next_sweep_reversed runs pinned forward and pinned reversed (bit 8 of the setting: the
tests cannot see or set the launch counter of autograd's thread).  Each result meets the float64 reference of its operation at the bound
that operation's own test file uses (named beside every case), and the two results are bit-equal - partial-sum outputs and weight / bias
gradients included.  Reserved CUs: 0, 16 (what DarcyTrainer sets under data parallelism) and 248 (usable_cus' floor of 8, which reaches
the several-images-per-workgroup forms with a partial last group at a few dozen images); reference parity only - the waves per image
change the cross-wave reduction order.

DIRECTION_CASES is also the table the CPU-side census (tests/test_launch_state_cpu.py) holds against the launchers in csrc."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import spectral_oracle as so
from test_hip_redzone import redzone  # noqa: F401  (fixture: guarded device allocations)

pytestmark = pytest.mark.gpu

K1, K3, K7, K8, K9, NORM, PROJ, LIFT = 1, 2, 4, 8, 16, 32, 64, 128          # SWEEP_* of csrc/uno_common.h


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def state():
    """set(direction, mask, reserve) -> None; whatever the first calls of the two setters returned is put back afterwards"""
    from uno_amd import _native
    L = _native.lib()
    first = {}

    def set_(direction="alternate", mask=255, reserve=0):
        d = _native.sweep_direction(direction, mask)
        r = _native.reserve_cus(reserve)
        first.setdefault("dir", d)
        first.setdefault("res", r)
    try:
        yield set_
    finally:
        torch.cuda.synchronize()
        if "dir" in first:
            L.uno_sweep_alternation(first["dir"])
            L.uno_reserve_cus(first["res"])


def rel(a, b):
    """l2-relative distance of a device result from a float64 reference (tests/test_hip_channel_mix.py: rel)"""
    b = torch.as_tensor(b).to(a.device) if not torch.is_tensor(b) else b.to(a.device)
    d = (a.double() - b.double()).norm().item()
    n = b.double().norm().item()
    return d / n if n > 0 else d


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=g)).to(dev())


# ---------------------------------------------------------------------------------------------------------------- the cases
# A case is a function -> list of (name, result tensor, float64 reference or None, bound).  None: a partial-sum output whose reference is
# checked through the sum that follows it; it still takes part in the bit-equality of the two directions.

def _fwd_ref(x, m1, m2, scale):
    """tests/test_hip_spectral2d.py: test_dft2d_forward_stage with (hermitian_cols, mask_overlap) = (True, True)"""
    n, _, H, W = x.shape
    ref = so.truncated_rfft2_dense(x.double().cpu().numpy(), m1, m2) * (H * W) * scale
    return ref * so.hermitian_weights(W, m2)[None, None, None, :] * so.later_wins_mask(H, m1)[None, None, :, None]


def _inv_ref(O, H, W, m1, m2, scale):
    """tests/test_hip_spectral2d.py: test_dft2d_inverse_stage with (True, True)"""
    O = O.cpu().numpy().astype(np.complex128)
    Gh = so._dft(so.corner_rows(H, m1), H, +1.0)
    Gw = so._dft(np.arange(m2), W, +1.0)
    U = np.einsum("bojl,jh->bohl", O * so.later_wins_mask(H, m1)[None, None, :, None], Gh)
    return scale * np.einsum("bohl,lw->bohw", U * so.hermitian_weights(W, m2), Gw).real


TOL_DFT = 2e-5          # tests/test_hip_spectral2d.py: TOL


def _dft_fwd(n, H, W, m1, m2, dtype=torch.float32):
    from uno_amd import _native
    x = _rn(_g(1000 + H * 7 + W + n), n, 1, H, W).to(dtype)
    got = _native.dft2d_forward(x, m1, m2, scale=0.5, hermitian_cols=True, mask_overlap=True)
    return [("spectrum", got, _fwd_ref(x, m1, m2, 0.5), TOL_DFT)]


def _dft_inv(n, H, W, m1, m2, dtype=torch.float32):
    from uno_amd import _native
    O = torch.randn(n, 1, 2 * m1, m2, dtype=torch.cfloat, generator=_g(2000 + H * 7 + W + n)).to(dev())
    got = _native.dft2d_inverse(O, H, W, scale=0.25, hermitian_cols=True, mask_overlap=True, dtype=dtype)
    # bf16 images: tests/test_hip_b16_transforms.py: TOL_BF16
    return [("images", got, _inv_ref(O, H, W, m1, m2, 0.25), 3e-3 if dtype == torch.bfloat16 else TOL_DFT)]


def _dft_inv_add(n=5, Hs=100, Ws=105, H=200, W=210, m1=6, m2=5):
    """tests/test_hip_fused_upsample.py: test_fused_inverse_add_matches_two_kernels_and_float64 (1e-6 against float64 of the plain
    inverse + the dense operators)"""
    from uno_amd import _native
    from uno_amd import resample as rs
    assert _native.dft2d_inverse_add_applies(n, H, W, m1, m2, Hs, Ws)
    tabs = rs.upsample_add_tables(Hs, Ws, H, W, str(dev()), False)
    g = _g(7)
    spec = torch.randn(n, 2 * m1, m2, dtype=torch.complex64, generator=g).to(dev())
    t = _rn(g, n, Hs, Ws)
    fused = _native.dft2d_inverse(spec, H, W, 1.0, True, True, addend=(t, tabs))
    plain = _native.dft2d_inverse(spec, H, W, 1.0, True, True)
    Rh, Rw = rs._matrix(Hs, H), rs._matrix(Ws, W)
    ref = plain.double() + torch.einsum("hu,nuv,wv->nhw", Rh.double().to(dev()), t.double(), Rw.double().to(dev()))
    return [("images", fused, ref, 1e-6)]


TOL_BF = 4e-3           # tests/test_hip_bf16_block.py: TOL_BF (bf16 results against the reference rounded to bf16: _cmp_bf)


def _bf_ref(ref):
    """tests/test_hip_bf16_block.py: _cmp_bf compares with the reference rounded to bfloat16"""
    return ref.float().to(torch.bfloat16).double()


def _k7(H, W, Ho, Wo, accumulate=False, bf16=False):
    """tests/test_hip_resample.py: test_resample_forward_backward_vs_torch_cpu (2e-6 against torch's CPU op, here in float64);
    bf16: tests/test_hip_bf16_block.py: test_resample_bf16 (TOL_BF, here against float64 of the same bf16 values)"""
    from uno_amd.resample import resample_adjoint, resample_forward
    g = _g(H * 31 + Wo)
    x, gy = torch.randn(3, 3, H, W, generator=g), torch.randn(3, 3, Ho, Wo, generator=g)
    if bf16:
        xb, gb = x.bfloat16(), gy.bfloat16()
        xc = xb.double().requires_grad_(True)
        yc = F.interpolate(xc, size=(Ho, Wo), mode="bicubic", align_corners=True, antialias=True)
        yc.backward(gb.double())
        if accumulate:
            b0 = torch.randn(3, 3, Ho, Wo, generator=g).bfloat16()
            y = resample_forward(xb.to(dev()), Ho, Wo, out=b0.to(dev()))
            return [("y", y, _bf_ref(yc.detach() + b0.double()), TOL_BF)]
        return [("y", resample_forward(xb.to(dev()), Ho, Wo), _bf_ref(yc.detach()), TOL_BF),
                ("gx", resample_adjoint(gb.to(dev()), H, W), _bf_ref(xc.grad), TOL_BF)]
    xc = x.double().requires_grad_(True)
    yc = F.interpolate(xc, size=(Ho, Wo), mode="bicubic", align_corners=True, antialias=True)
    yc.backward(gy.double())
    if accumulate:
        b0, b1 = torch.randn(3, 3, Ho, Wo, generator=g), torch.randn(3, 3, H, W, generator=g)
        y = resample_forward(x.to(dev()), Ho, Wo, out=b0.to(dev()))
        gx = resample_adjoint(gy.to(dev()), H, W, out=b1.to(dev()))
        return [("y", y, yc.detach() + b0.double(), 2e-6), ("gx", gx, xc.grad + b1.double(), 2e-6)]
    return [("y", resample_forward(x.to(dev()), Ho, Wo), yc.detach(), 2e-6), ("gx", resample_adjoint(gy.to(dev()), H, W), xc.grad, 2e-6)]


def _mix_ref(x, w, b):
    """tests/test_hip_channel_mix.py: _ref"""
    y = torch.matmul(w.double(), x.double())
    return y if b is None else y + b.double().view(1, -1, 1)


def _gelu64(t):
    return F.gelu(t.double())


def _dgelu64(t):
    p = t.double().requires_grad_(True)
    F.gelu(p).sum().backward()
    return p.grad


def _k8(B, Ci, Co, P, tol, dtype=torch.float32, act_in=False):
    """K8 on one source: forward with bias and the transposed (input-gradient) call.  tests/test_hip_channel_mix.py: 2e-6 for the f32-MFMA
    forms (test_forward / test_transposed), 1e-6 for K8-S (test_split_bf16_wide_layers), 3e-3 on bf16 activations
    (test_split_bf16_64_channel_tiles)"""
    from uno_amd import _native
    g = _g(B * 1000 + Ci * 10 + Co)
    x, w, b = _rn(g, B, Ci, P).to(dtype), _rn(g, Co, Ci, scale=Ci ** -0.5), _rn(g, Co)
    gy = _rn(g, B, Co, P).to(dtype)
    y = _native.channel_mix2(x, None, w, b, act_in=True) if act_in else _native.channel_mix(x, w, b)
    gx = _native.channel_mix(gy, w, None, transpose_w=True)
    xin = _gelu64(x.float()) if act_in else x
    return [("y", y, _mix_ref(xin, w, b), tol), ("gx", gx, torch.matmul(w.double().t(), gy.double()), tol)]


def _k8_two(B=3, C1=16, C2=48, Co=40, P=515):
    """two sources with the activated copy, two destinations with gelu' (tests/test_hip_channel_mix.py: test_two_source_forward,
    test_two_destination_input_gradients: 2e-6)"""
    from uno_amd import _native
    g = _g(C1 + 3 * C2 + Co + P)
    x1, x2, w, b = _rn(g, B, C1, P), _rn(g, B, C2, P), _rn(g, Co, C1 + C2), _rn(g, Co)
    y, act = _native.channel_mix2(x1, x2, w, b, y_act=True)
    ref = _mix_ref(torch.cat([x1, x2], 1), w, b)
    D1, D2 = 64, 64
    gy, wt, pre = _rn(g, B, 64, P), _rn(g, 64, D1 + D2), _rn(g, B, D1, P)
    g1, g2 = _native.channel_mix2(gy, None, wt, None, transpose_w=True, split_out=D1, dgelu_of=pre)
    full = torch.matmul(wt.double().t(), gy.double())
    return [("y", y, ref, 2e-6), ("act", act, _gelu64(ref), 2e-6), ("g1", g1, full[:, :D1] * _dgelu64(pre), 2e-6), ("g2", g2, full[:, D1:], 2e-6)]


def _crop(t, rows, cols, pitch):
    """tests/test_hip_window.py: _crop"""
    B, C = t.shape[:2]
    return t.view(B, C, -1, pitch)[:, :, :rows, :cols].reshape(B, C, rows * cols).contiguous()


WIN = (7, 260, 301, 11)         # rows, cols, pitch (odd: cols != pitch, rows start 4-byte aligned only), plane rows (tests/test_hip_window.py)


def _k8_window(C1=64, C2=64, Co=64):
    """tests/test_hip_window.py: test_forward_window_equals_dense_on_the_crop / test_input_gradient_window; held here to float64 at the
    dense calls' own bound (tests/test_hip_channel_mix.py: 2e-6); everything outside the window stays as it was"""
    from uno_amd import _native
    rows, cols, pitch, H = WIN
    g = _g(rows + cols + C1 + Co)
    x1, x2 = _rn(g, 3, C1, H * pitch), _rn(g, 3, C2, H * pitch)
    w, b = _rn(g, Co, C1 + C2, scale=(C1 + C2) ** -0.5), _rn(g, Co)
    out = torch.empty((3, Co, H * pitch), dtype=torch.float32, device=dev()).fill_(7.25)      # (torch.empty: guarded under the redzone fixture)
    _native.channel_mix2(x1, x2, w, b, act_in=True, out=out, window=(rows, cols, pitch))
    ref = _mix_ref(torch.cat([_gelu64(_crop(x1, rows, cols, pitch)), _crop(x2, rows, cols, pitch).double()], 1), w, b)
    v = out.view(3, Co, H, pitch)
    assert bool((v[:, :, rows:] == 7.25).all()) and bool((v[:, :, :rows, cols:] == 7.25).all()), "the windowed call wrote outside its window"
    gy, wt, pre = _rn(g, 3, 64, H * pitch), _rn(g, 64, 64, scale=0.125), _rn(g, 3, 64, H * pitch)
    gx = torch.empty((3, 64, H * pitch), dtype=torch.float32, device=dev()).fill_(7.25)
    _native.channel_mix2(gy, None, wt, None, transpose_w=True, out=gx, dgelu_of=pre, window=(rows, cols, pitch))
    gref = torch.matmul(wt.double().t(), _crop(gy, rows, cols, pitch).double()) * _dgelu64(_crop(pre, rows, cols, pitch))
    v = gx.view(3, 64, H, pitch)
    assert bool((v[:, :, rows:] == 7.25).all()) and bool((v[:, :, :rows, cols:] == 7.25).all()), "the windowed call wrote outside its window"
    return [("y", _crop(out, rows, cols, pitch), ref, 2e-6), ("gx", _crop(gx, rows, cols, pitch), gref, 2e-6), ("y plane", out, None, 0), ("gx plane", gx, None, 0)]


def _k8_padded(B=3, Ci=16, Co=40, H=9, W=300, ph=2, pw=5):
    """tests/test_hip_window.py: test_lift_with_padded_activation (2e-6; 3e-6 for the recomputing backward kernel)"""
    from uno_amd import _native
    g = _g(H + W + Co)
    x, w, b = _rn(g, B, Ci, H, W), _rn(g, Co, Ci, scale=Ci ** -0.5), _rn(g, Co)
    y, act = _native.channel_mix_act_padded(x, w, b, H + ph, W + pw, act_in=True)
    yr = torch.matmul(w.double(), _gelu64(x).view(B, Ci, -1)).view(B, Co, H, W) + b.double().view(1, -1, 1, 1)
    gp = _rn(g, B, Co, H + ph, W + pw)
    gz = _native.channel_mix_dgelu_padded(x, w, b, gp, act_in=True)
    return [("y", y, yr, 2e-6), ("act", act, F.pad(F.gelu(yr), [0, pw, 0, ph]), 2e-6), ("gz", gz, _dgelu64(yr) * gp[:, :, :H, :W].double(), 3e-6)]


def _k9(B, C1, C2, Co, P, tol, act_x=False, dtype=torch.float32):
    """tests/test_hip_channel_mix.py: test_wgrad / test_two_source_wgrad (2e-5), test_wide_wgrad_split_bf16 (2e-6)"""
    from uno_amd import _native
    g = _g(C1 + C2 + Co + P)
    gy, x1 = _rn(g, B, Co, P).to(dtype), _rn(g, B, C1, P).to(dtype)
    x2 = _rn(g, B, C2, P).to(dtype) if C2 else None
    gw, gb = _native.channel_wgrad2(gy, x1, x2, act_x=act_x) if C1 > 4 else _native.channel_wgrad(gy, x1)
    xs = [_gelu64(x1.float()) if act_x else x1.double()] + ([x2.double()] if C2 else [])
    return [("gw", gw, torch.einsum("bop,bip->oi", gy.double(), torch.cat(xs, 1)), tol), ("gb", gb, gy.double().sum(dim=(0, 2)), tol)]


def _k9_window(C1=64, C2=64, Co=32):
    """tests/test_hip_window.py: test_weight_gradient_window (2e-5 against float64 on the crop)"""
    from uno_amd import _native
    rows, cols, pitch, H = WIN
    win = (rows, cols, pitch)
    g = _g(rows + C1 + Co)
    gy, x1, x2 = _rn(g, 3, Co, H * pitch), _rn(g, 3, C1, H * pitch), _rn(g, 3, C2, H * pitch)
    gw, gb = _native.channel_wgrad2(gy, x1, x2, need_bias=True, act_x=True, window=win)
    xc = torch.cat([_gelu64(_crop(x1, *win)), _crop(x2, *win).double()], 1)
    gyc = _crop(gy, *win).double()
    return [("gw", gw, torch.einsum("bop,bip->oi", gyc, xc), 2e-5), ("gb", gb, gyc.sum((0, 2)), 2e-5)]


def _norm(shape, gelu, dtype=torch.float32):
    """tests/test_hip_instnorm.py: test_instance_norm_gelu (3e-6 forward, 2e-5 input / weight / bias gradients, against float64); the
    per-row statistics and partial sums (mean, rstd, s1, s2: one slot per row) take part in the bit-equality"""
    from uno_amd import _native
    B, C = shape[:2]
    g = _g(sum(shape))
    x, gy = (3.0 * torch.randn(*shape, generator=g) + 1.5).to(dev()).to(dtype), _rn(g, *shape).to(dtype)
    gamma, beta = _rn(g, C), _rn(g, C)
    y, mean, rstd = _native.instnorm_forward(x, gamma, beta, 1e-5, gelu)
    gx, s1, s2 = _native.instnorm_backward(x, gy, gamma, beta, mean, rstd, gelu)
    x2, g2, b2 = (t.double().detach().requires_grad_(True) for t in (x, gamma, beta))
    y2 = F.instance_norm(x2, weight=g2, bias=b2, eps=1e-5)
    y2 = F.gelu(y2) if gelu else y2
    rgx, rgg, rgb = torch.autograd.grad(y2, (x2, g2, b2), gy.double())
    if dtype == torch.bfloat16:
        # tests/test_hip_bf16_block.py: test_instnorm_bf16 (TOL_BF for y and gx against the bf16-rounded reference, 1e-4 for the partial sums;
        # here against float64 on the same bf16 inputs)
        return [("y", y, _bf_ref(y2.detach()), TOL_BF), ("gx", gx, _bf_ref(rgx), TOL_BF), ("gamma grad", s2.sum(0), rgg, 1e-4),
                ("beta grad", s1.sum(0), rgb, 1e-4), ("mean", mean, None, 0), ("rstd", rstd, None, 0), ("s1", s1, None, 0), ("s2", s2, None, 0)]
    return [("y", y, y2.detach(), 3e-6), ("gx", gx, rgx, 2e-5), ("gamma grad", s2.sum(0), rgg, 2e-5), ("beta grad", s1.sum(0), rgb, 2e-5),
            ("mean", mean, None, 0), ("rstd", rstd, None, 0), ("s1", s1, None, 0), ("s2", s2, None, 0)]


def _proj_bwd(window):
    """tests/test_hip_pointwise_fused.py: test_gelu_project (2e-6 input gradient, 2e-5 weight / bias gradients, float64);
    tests/test_hip_window.py: test_gelu_project_backward_window for the windowed form"""
    from uno_amd import _native
    B, Cc = 3, 64
    g = _g(17)
    if window:
        rows, cols, pitch, H = WIN
        win, P = (rows, cols, pitch), H * pitch
    else:
        win, P = None, 1037
    pre, gout, w = _rn(g, B, Cc, P), _rn(g, B, P), _rn(g, Cc)
    gpre, gw, gb = _native.gelu_project_backward(pre, w, gout, need_bias=True, window=win)
    pc = _crop(pre, *win) if window else pre
    gc = _crop(gout.view(B, 1, -1), *win).view(B, -1) if window else gout
    p2, w2 = pc.double().requires_grad_(True), w.double().requires_grad_(True)
    out = torch.einsum("c,bcp->bp", w2, F.gelu(p2))
    rp, rw = torch.autograd.grad(out, (p2, w2), gc.double())
    return [("gpre", _crop(gpre, *win) if window else gpre, rp, 2e-6), ("gw", gw, rw, 2e-5), ("gb", gb, gc.double().sum().view(1), 2e-5)]


def _lift(B, Cin, Cm, Co, H, W, ph, pw, second):
    """tests/test_hip_window.py: test_whole_lift_without_stored_intermediates (3e-6 forward, 3e-5 parameter gradients, float64);
    second: uno_lift_backward2's two-gradient form (test_lift_backward_adds_a_second_gradient_as_it_reads), held to float64 of the sum"""
    from uno_amd import _native
    gen = _g(B + Cin + Cm + Co + H + W)
    x, w1, w0 = _rn(gen, B, Cin, H, W), _rn(gen, Cm, Cin), _rn(gen, Co, Cm, scale=Cm ** -0.5)
    b1, b0 = _rn(gen, Cm), _rn(gen, Co)
    act = _native.lift_forward(x, w1, b1, w0, b0, H + ph, W + pw)
    d = [t.double().requires_grad_(True) for t in (w1, b1, w0, b0)]
    h = torch.einsum("mk,bkhw->bmhw", d[0], x.double()) + d[1].view(1, -1, 1, 1)
    z = torch.einsum("om,bmhw->bohw", d[2], F.gelu(h)) + d[3].view(1, -1, 1, 1)
    ref = F.pad(F.gelu(z), [0, pw, 0, ph])
    gact = _rn(gen, *act.shape)
    total = gact.double()
    g2 = None
    if second:
        assert _native.lift_backward_takes_second(x, w1, w0, H + ph, W + pw)
        g2 = torch.full(act.shape, float("nan"), device=dev())
        g2[:, :, :H, :W] = _rn(gen, B, Co, H, W)
        total = total.clone()
        total[:, :, :H, :W] += g2[:, :, :H, :W].double()
    ref.backward(total)
    got = _native.lift_backward(x, w1, b1, w0, b0, gact, g2)
    return [("act", act, ref.detach(), 3e-6)] + [(n, a, r.grad, 3e-5) for n, a, r in zip(("gw1", "gb1", "gw0", "gb0"), got, d)]


# name: (family bit, case).  Shapes: B = 3 (sweep_y), odd tile counts with a ragged last pixel tile (P not a multiple of 128), more than
# one output-channel tile (ncot > 1: Co = 70 on 64-channel tiles, 256 on 128-channel tiles), rows = B * C odd, lift widths whose
# tile groups do not divide by 8, windows with cols != pitch
DIRECTION_CASES = {
    # K1 / K3: W % 8 != 0 and 33 <= W <= 160 full-tile forms; W >= 200 the half-tile form; W % 8 == 0 K3's staged form; H not a multiple of 16
    "k1_ft": (K1, lambda: _dft_fwd(35, 40, 44, 4, 5)),
    "k1_ht": (K1, lambda: _dft_fwd(3, 40, 223, 8, 8)),
    "k3": (K3, lambda: _dft_inv(35, 40, 48, 4, 5)),
    "k3_bf16": (K3, lambda: _dft_inv(5, 12, 48, 4, 5, torch.bfloat16)),
    "k3_ft": (K3, lambda: _dft_inv(35, 40, 44, 4, 5)),
    "k3a_inverse_add": (K3, _dft_inv_add),
    "k7_down": (K7, lambda: _k7(37, 50, 29, 31)),
    "k7_up": (K7, lambda: _k7(22, 37, 45, 50)),
    "k7_accumulate": (K7, lambda: _k7(40, 36, 20, 18, accumulate=True)),
    "k7_down_bf16": (K7, lambda: _k7(37, 50, 29, 31, bf16=True)),
    "k7_up_bf16": (K7, lambda: _k7(22, 37, 45, 50, bf16=True)),
    "k7_accumulate_bf16": (K7, lambda: _k7(40, 36, 20, 18, accumulate=True, bf16=True)),
    "k8_generic": (K8, lambda: _k8(3, 20, 70, 1037, 2e-6)),
    "k8_generic_act_in": (K8, lambda: _k8(3, 32, 70, 1037, 2e-6, act_in=True)),
    "k8_wide128": (K8, lambda: _k8(3, 64, 256, 128 * 5 + 37, 2e-6)),
    "k8_split": (K8, lambda: _k8(3, 128, 256, 1111, 1e-6)),
    "k8_split_bf16": (K8, lambda: _k8(3, 256, 64, 1111, 3e-3, torch.bfloat16)),
    "k8_two_sources_two_destinations": (K8, _k8_two),
    "k8_window": (K8, _k8_window),
    "k8_act_padded_dgelu_padded": (K8, _k8_padded),
    # vec_kernel<false, false> (more than 32 input channels, no GELU on read), its narrow form (<= 32 input channels), and the streaming
    # few-input kernel (Ci <= 4), which takes the launcher's direction argument but maps its work items without it
    "k9_vector": (K9, lambda: _k9(3, 64, 0, 40, 1037, 2e-5)),
    "k9_narrow": (K9, lambda: _k9(3, 24, 0, 40, 1037, 2e-5)),
    "k9_few_in": (K9, lambda: _k9(3, 3, 0, 17, 1025, 2e-5)),
    "k9_split": (K9, lambda: _k9(3, 192, 0, 48, 33400 + 29, 2e-6)),
    "k9_wgrad2": (K9, lambda: _k9(3, 64, 64, 64, 446 * 9 + 3, 2e-5, act_x=True)),
    "k9_window": (K9, _k9_window),
    "norm_reg_gelu": (NORM, lambda: _norm((3, 5, 9, 13), True)),
    "norm_reg_plain": (NORM, lambda: _norm((3, 5, 111, 111), False)),
    "norm_sweep_gelu": (NORM, lambda: _norm((1, 3, 300, 300), True)),
    "norm_sweep_plain": (NORM, lambda: _norm((1, 3, 300, 300), False)),
    "norm_reg_gelu_bf16": (NORM, lambda: _norm((3, 5, 37, 41), True, torch.bfloat16)),
    "norm_reg_plain_bf16": (NORM, lambda: _norm((3, 5, 111, 111), False, torch.bfloat16)),
    "norm_sweep_gelu_bf16": (NORM, lambda: _norm((1, 3, 300, 300), True, torch.bfloat16)),
    "norm_sweep_plain_bf16": (NORM, lambda: _norm((1, 3, 300, 300), False, torch.bfloat16)),
    "proj_backward": (PROJ, lambda: _proj_bwd(False)),
    "proj_backward_win": (PROJ, lambda: _proj_bwd(True)),
    # lift, 32 -> 64 channels: the fused forward and backward kernels of csrc/lift_bwd.hip (one and two gradients); 7 x 261 and 9 x 283
    # leave ragged tile groups.  16 -> 24 channels: the unfused path - K8 with the virtual input (forward and the recomputing gelu' kernel)
    # and K9's virtual-input launcher (launch_channel_wgrad_vh)
    "lift_forward_backward": (LIFT, lambda: _lift(3, 3, 32, 64, 7, 261, 0, 3, False)),
    "lift_backward2": (LIFT, lambda: _lift(3, 2, 32, 64, 9, 283, 2, 2, True)),
    "lift_unfused_virtual_input": (K8 | K9, lambda: _lift(3, 1, 16, 24, 9, 300, 0, 5, False)),
}


def _check(results, what):
    for name, got, ref, tol in results:
        assert bool(torch.isfinite(got.float()).all()), f"{what}: {name} is not finite"
        if ref is not None:
            e = rel(got, ref)
            print(f"[{what}] {name}: {e:.2e} (bound {tol:.0e})")
            assert e < tol, (what, name, e)


@pytest.mark.parametrize("direction", ["forward", "reversed"])
@pytest.mark.parametrize("name", list(DIRECTION_CASES))
def test_each_direction_meets_the_float64_reference(state, name, direction):
    state(direction)
    _check(DIRECTION_CASES[name][1](), f"{name} {direction}")


@pytest.mark.parametrize("name", list(DIRECTION_CASES))
def test_the_two_directions_are_bit_equal(state, name):
    state("forward")
    fwd = DIRECTION_CASES[name][1]()
    state("reversed")
    rev = DIRECTION_CASES[name][1]()
    for (n, a, _, _), (_, b, _, _) in zip(fwd, rev):
        assert torch.equal(a, b), f"{name}: {n} depends on the sweep direction"


def test_alternating_launches_are_bit_equal(state):
    """the default setting: six back-to-back calls of a single-launch operation (three forward, three reversed) agree bit for bit"""
    from uno_amd import _native
    state("alternate")
    g = _g(3)
    x, gamma, beta = _rn(g, 3, 5, 37, 41), _rn(g, 5), _rn(g, 5)
    outs = [_native.instnorm_forward(x, gamma, beta, 1e-5, True) for _ in range(6)]
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)


def test_a_masked_off_family_ignores_the_pin(state):
    """reversed pinned for K8 only: the setting reads back as set, InstanceNorm results equal the all-forward run and K8 still meets its
    reference.  By the contract under test the results are bit-equal in EITHER direction, so this cannot show which direction the
    masked-off family took, nor that the counter stood still: it shows that a mask with one family pinned disturbs no result.  The
    mask arithmetic itself is held by tests/test_launch_state_cpu.py."""
    from uno_amd import _native
    state("forward")
    base = DIRECTION_CASES["norm_reg_gelu"][1]()
    state("reversed", mask=K8)
    assert _native.lib().uno_sweep_alternation(256 | K8) == (256 | K8)
    pinned = DIRECTION_CASES["norm_reg_gelu"][1]()
    for (n, a, _, _), (_, b, _, _) in zip(base, pinned):
        assert torch.equal(a, b), n
    _check(pinned, "norm with K8 pinned")
    _check(DIRECTION_CASES["k8_generic"][1](), "k8 pinned alone")


# ---------------------------------------------------------------------------------------------------------------- reserved CUs
# usable_cus (csrc/uno_common.h) = device CUs - reserved, at least 8: 256 / 240 / 8 on the 256-CU device.  The geometry loops
# (fwd_ft_geometry, inv_geometry, inv_ft_geometry) start from g = 4 / nw (12 / nw in inv_geometry) images per workgroup and lower g while
# ceil(n_img / g) < usable CUs.
#   H = 12: one row tile (nrt = 1), so only nw = 1 is tried.  At 8 CUs: n_img = 17 -> g = 2 (ceil(17 / 3) = 6 < 8 <= ceil(17 / 2) = 9, last
#   group holds 1 image), 26 -> g = 3 (ceil(26 / 4) = 7 < 8 <= ceil(26 / 3) = 9, last group 2), 35 -> g = 4 (ceil(35 / 4) = 9, last group 3;
#   inv_geometry: g = 5 gives 7 < 8, so 4 there as well).
#   H = 40: nrt = 3, nw in {1, 2} (full-tile forms) or {1, 2, 3} (inv_geometry).  At 8 CUs and n_img = 17 all groups fit one round, so the cost
#   is ceil(nrt / nw): full-tile forms take (nw, g) = (2, 2) (cost 2 against 3; 17 = 8 x 2 + 1), inv_geometry (3, 2) (g = 4 -> ceil(17 / 4) = 5,
#   3 -> 6, 2 -> 9; cost 64 against 128 / 192).
#   From 128 images on, f32 images of up to 2048 points and W <= 64 go to the plane-batched kernels before any of these loops is asked
#   (capi_spectral.hip, dft2d_plane.hip: plane_shape_ok), so the many-image cases use W = 68 (W % 8 != 0, <= FT_MAXW = 160, 16 W >= 512
#   reduction slots: K1-FT / K3-FT, g from 4) and W = 72 (W % 8 == 0: K3 through inv_geometry, g from 12; the forward transform takes the
#   register form, one image per workgroup).  H = 12, nw = 1:
#   n_img = 1000: ceil(1000 / 4) = 250 >= 240 but < 256 - reserve 16 keeps g = 4 (250 full groups), reserve 0 lowers it to g = 3
#   (ceil(1000 / 3) = 334, last group 1) in all three loops (inv_geometry: ceil(1000 / 5) = 200 < 240); reserve 248: g = 4, and g = 12 in
#   inv_geometry (ceil(1000 / 12) = 84 >= 8, last group 4).
#   n_img = 1027, reserve 0: ceil(1027 / 4) = 257 >= 256 (ceil(1027 / 5) = 206 < 256) - the real-device g = 4 with a last group of 3.
RESERVES = [0, 16, 248]
TRANSFORM_SHAPES = [  # n_img, H, W, m1, m2
    (17, 12, 44, 4, 5), (26, 12, 44, 4, 5), (35, 12, 44, 4, 5), (17, 12, 48, 4, 5), (26, 12, 48, 4, 5), (35, 12, 48, 4, 5),
    (17, 40, 44, 4, 5), (17, 40, 48, 4, 5), (1000, 12, 68, 4, 5), (1000, 12, 72, 4, 5), (1027, 12, 68, 4, 5), (1027, 12, 72, 4, 5),
    # plane-batched K1p / K3p (n_img >= 128, small planes): a persistent grid of resident workgroups x usable CUs - at 8 CUs every
    # workgroup loops over many images (tests/test_hip_spectral2d.py: DFT_SHAPES)
    (1100, 10, 14, 5, 5), (131, 23, 23, 11, 12),
]


@pytest.mark.parametrize("direction", ["forward", "reversed"])
@pytest.mark.parametrize("reserve", RESERVES)
@pytest.mark.parametrize("shape", TRANSFORM_SHAPES)
def test_transforms_under_reserved_cus(state, redzone, shape, reserve, direction):  # noqa: F811
    """forward and inverse transform (and, off the plane-batched shapes, the inverse to bf16 images on the f32-MFMA kernel: W < 64) at
    every reserve setting, pinned both ways, with every output between guard bands (tests/test_hip_redzone.py)"""
    state(direction, reserve=reserve)
    _check(_dft_fwd(*shape), f"forward {shape} reserve {reserve} {direction}")
    _check(_dft_inv(*shape), f"inverse {shape} reserve {reserve} {direction}")
    if shape[2] >= 44:
        _check(_dft_inv(*shape, dtype=torch.bfloat16), f"bf16 inverse {shape} reserve {reserve} {direction}")
    assert redzone.check(f"transforms {shape} reserve {reserve}") >= 2


@pytest.mark.parametrize("reserve", RESERVES)
@pytest.mark.parametrize("shape", [(17, 16, 67, 6, 6), (26, 24, 72, 5, 9), (35, 17, 65, 3, 3), (1027, 16, 67, 6, 6)])
def test_bf16_transforms_under_reserved_cus(state, redzone, shape, reserve):  # noqa: F811
    """the bf16-MFMA transforms (csrc/dft2d_b16.hip; W >= 64, H >= 16): tests/test_hip_b16_transforms.py's references and bounds (2e-5 for
    the f32 spectrum of bf16 images, 3e-3 for bf16 images)"""
    state("alternate", reserve=reserve)
    n, H, W, m1, m2 = shape
    _check(_dft_fwd(n, H, W, m1, m2, torch.bfloat16), f"bf16 forward {shape} reserve {reserve}")
    _check(_dft_inv(n, H, W, m1, m2, torch.bfloat16), f"bf16 inverse {shape} reserve {reserve}")
    assert redzone.check(f"bf16 transforms {shape} reserve {reserve}") >= 2


@pytest.mark.parametrize("reserve", RESERVES)
def test_inverse_add_under_reserved_cus(state, redzone, reserve):  # noqa: F811
    state("reversed", reserve=reserve)
    _check(_dft_inv_add(n=17), f"inverse_add reserve {reserve}")
    assert redzone.check(f"inverse_add reserve {reserve}") >= 2


@pytest.mark.parametrize("direction", ["forward", "reversed"])
@pytest.mark.parametrize("reserve", RESERVES)
@pytest.mark.parametrize("cfg", [(2, 4, 3, (16, 16, 10), (16, 16, 10), (6, 6, 4)), (1, 8, 8, (32, 32, 13), (24, 24, 15), (11, 11, 5)),
                                 (2, 3, 5, (9, 20, 7), (11, 14, 12), (4, 7, 4))])
def test_spectral_conv3d_planes_under_reserved_cus(state, redzone, cfg, reserve, direction):  # noqa: F811
    """SpectralConv3d with few volumes (below the 48 the per-volume kernels need): the (W, T) planes go through the plane-batched K1p /
    K3p by their row-frequency entry, 128 ... 256 planes per transform on a persistent grid that shrinks with the usable CUs, so that at
    8 CUs every workgroup loops.  Reference and bound: tests/test_hip_spectral3d.py: test_seeded_3d_vs_dense_oracle (SEEDED3, TOL)"""
    from test_hip_spectral3d import TOL
    from uno_amd.spectral3d import spectral_conv3d
    B, Ci, Co, din, dout, modes = cfg
    rng = np.random.default_rng(B + Ci * 7 + sum(din) + sum(modes))
    x = rng.standard_normal((B, Ci, *din)).astype(np.float32)
    sc = (1 / (2 * Ci)) ** 0.5
    ws = [(sc * (rng.standard_normal((Ci, Co, *modes)) + 1j * rng.standard_normal((Ci, Co, *modes)))).astype(np.complex64) for _ in range(4)]
    gy = rng.standard_normal((B, Co, *dout)).astype(np.float32)
    y_ref, X = so.spectral_conv3d_dense(x, ws, *dout)
    gx_ref, gws_ref, _, _ = so.spectral_conv3d_dense_bwd(gy, X, ws, *din)
    state(direction, reserve=reserve)
    xd = torch.from_numpy(x).to(dev()).requires_grad_(True)
    wd = [torch.from_numpy(w).to(dev()).requires_grad_(True) for w in ws]
    y = spectral_conv3d(xd, wd, *dout)
    y.backward(torch.from_numpy(gy).to(dev()))
    assert rel_err(y.detach().cpu().numpy(), y_ref) < TOL
    assert rel_err(xd.grad.cpu().numpy(), gx_ref) < TOL
    for k in range(4):
        assert rel_err(wd[k].grad.cpu().numpy(), gws_ref[k]) < TOL, k
    assert redzone.check(f"spectral_conv3d {cfg} reserve {reserve}") >= 4


@pytest.mark.parametrize("reserve", RESERVES)
def test_any_grid_resample_under_reserved_cus(state, redzone, reserve):  # noqa: F811
    """uno_fft_resample3d_any and its accumulating forms on a persistent grid of usable CUs x at most 8 workgroups: 20 volumes x 15 planes =
    300 forward items and 20 x 7 = 140 inverse items against 64 workgroups at 8 CUs, so every workgroup loops.  Reference and bound:
    tests/test_hip_resample3d_any.py (_reference_sequence, TOL of tests/test_hip_spectral3d.py)"""
    from test_hip_resample3d_any import _reference_sequence, _run_any
    from test_hip_spectral3d import TOL
    from uno_amd import _native
    from uno_amd.spectral3d import _resample3d_plan_any
    state("alternate", reserve=reserve)
    din, dout = (15, 15, 9), (7, 7, 6)
    g = _g(5)
    x, gy = torch.randn(4, 5, *din, generator=g), torch.randn(4, 5, *dout, generator=g)
    yr, gxr = _reference_sequence(x, gy, dout)
    y, gx = _run_any(x, gy, dout)
    assert rel(y, yr) < TOL and rel(gx, gxr) < TOL
    t1, t2, m3 = _resample3d_plan_any(din, dout, dev())
    scale = 1.0 / (dout[0] * dout[1] * dout[2])
    base = _rn(g, 4, 5, *dout)
    out, act = _native.fft_resample3d_any(x.to(dev()), dout, (t1, t1), (t2, t2), m3, scale, adjoint=False, out=base.clone(), act=True)
    assert rel(out, yr + base.double().cpu()) < TOL and rel(act, F.gelu(yr + base.double().cpu())) < TOL
    out2 = _native.fft_resample3d_any(x.to(dev()), dout, (t1, t1), (t2, t2), m3, scale, adjoint=False, out=base.clone())
    assert torch.equal(out2, out)
    assert redzone.check(f"any-grid resample reserve {reserve}") >= 4


def test_windowed_calls_reversed_between_guard_bands(state, redzone):  # noqa: F811
    state("reversed")
    _check(_k8_window(), "k8 window reversed")
    _check(_k9_window(), "k9 window reversed")
    _check(_proj_bwd(True), "projection backward window reversed")
    assert redzone.check("reversed windowed calls") >= 3


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_small_darcy_step_reversed_with_reserved_cus(state):
    """One training step of the Darcy model at a small ragged grid with {reversed pinned, 16 CUs reserved}, against the float64 oracle
    model of tests/test_hip_headline_parity.py at that file's bounds (1e-4 output, loss and every parameter gradient)"""
    from test_hip_headline_parity import _assert_grads
    from uno_amd.harness import DarcyTrainer, UNO_9, lp_loss_rel_sum, synthetic_darcy_batch
    B, S, width = 2, 75, 16          # (S = 75: padded 80, levels 40 / 20 - the ragged small form of tests/test_hip_redzone.py)
    torch.manual_seed(0)
    ref = UNO_9(3, width, pad=5, block_cls=so.OracleOperatorBlock2d)
    prod = UNO_9(3, width, pad=5)
    prod.load_state_dict(ref.state_dict(), strict=True)
    prod = prod.to(dev())
    a, u = synthetic_darcy_batch(B, S, 1234, "cpu")
    out_ref = ref(a)
    loss_ref = lp_loss_rel_sum(out_ref.reshape(B, -1), u.reshape(B, -1))
    loss_ref.backward()
    state("reversed", reserve=16)
    out = prod(a.to(dev()))
    assert rel_err(out.detach().cpu().numpy(), out_ref.detach().numpy()) < 1e-4
    tr = DarcyTrainer(prod, lr=1e-3, weight_decay=1e-3)
    loss = tr.step(a.to(dev()), u.to(dev()))
    assert abs(float(loss) - float(loss_ref)) < 1e-4 * abs(float(loss_ref))
    print("worst parameter gradient:", _assert_grads(prod, ref, 1e-4, skip=("conv1.w.conv.bias", "conv4.w.conv.bias")))


def test_small_ns3d_step_reversed_with_reserved_cus(state, monkeypatch):
    """One training step of the NS-3D model at a small size (Uno3D_T20 of width 4 on 32 x 32 x 10, batch 2) with {reversed pinned, 16 CUs
    reserved}, held to the float64 oracle by tests/test_hip_workload_parity.py's own machinery - host_reference (R64 and the
    float32-oracle floors), compare_to_reference and its bound MODEL_TOL - with only the model size and the batch replaced"""
    import test_hip_workload_parity as wp
    from uno_amd.harness import ComplexAdam, Uno3D_T20

    def build(wl, block_cls=None):
        torch.manual_seed(0)
        return Uno3D_T20(6, 4, pad=3, **({} if block_cls is None else {"block_cls": block_cls}))

    def inputs(wl):
        g = _g(1234)
        return torch.randn(2, 32, 32, 10, 1, generator=g), torch.randn(2, 32, 32, 20, generator=g)
    monkeypatch.setattr(wp, "build_model", build)
    monkeypatch.setattr(wp, "make_inputs", inputs)
    wl = "c4_w8"
    ref = wp.host_reference(wl)
    prod = build(wl)
    prod.load_state_dict(ref["state"], strict=True)
    prod = prod.to(dev())
    inp = tuple(t.to(dev()) for t in ref["inputs"])
    state("reversed", reserve=16)
    opt = ComplexAdam(prod.parameters(), lr=1e-3, weight_decay=1e-4)
    opt.zero_grad(set_to_none=True)
    pred, loss = wp.forward_backward(wl, prod, inp)
    grads = {k: p.grad.clone() for k, p in prod.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    bad = wp.compare_to_reference("small NS-3D step, reversed, reserve 16", ref, pred, loss, grads, tol=wp.MODEL_TOL)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- graph capture
def test_a_captured_step_keeps_its_capture_time_state(state):
    """The direction and the geometry are baked into the captured kernel arguments: a GraphedStep captured under {reversed, reserve 248}
    and replayed under {forward, reserve 0} gives the eager step of the capture-time state bit for bit.  (Results do not depend on the
    direction, so it is the reserve-248 geometry - waves per image, hence the cross-wave reduction order - that would make a replay
    differ if it re-read the state.)"""
    from uno_amd.harness import ComplexAdam, GraphedStep, UNO, ns2d_rollout_loss

    def make():
        torch.manual_seed(5)
        m = UNO(14, 4).to(dev())
        return m, ComplexAdam(m.parameters(), lr=1e-3, weight_decay=1e-4)
    g = _g(9)
    xx, yy = _rn(g, 2, 64, 64, 10), _rn(g, 2, 64, 64, 3)
    state("reversed", reserve=248)
    me, oe = make()
    mg, og = make()
    gs = GraphedStep(mg, og, lambda a, b: ns2d_rollout_loss(mg, a, b, T_f=3, step=1), (xx, yy))
    ns2d_rollout_loss(me, xx, yy, T_f=3, step=1).backward()         # (as tests/test_harness_ns.py: the first backward pass runs use by use)
    oe.zero_grad(set_to_none=True)
    le = ns2d_rollout_loss(me, xx, yy, T_f=3, step=1)
    le.backward()
    torch.cuda.synchronize()
    state("forward", reserve=0)
    lg = gs.step(xx, yy)
    assert float(lg) == float(le)
    for (k, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(pe.grad, pg.grad), k


# ---------------------------------------------------------------------------------------------------------------- last
def test_zz_the_process_is_back_at_its_defaults():
    from uno_amd import _native
    L = _native.lib()
    a = L.uno_sweep_alternation(255)
    r = L.uno_reserve_cus(0)
    assert (a, r) == (255, 0)
