"""K1-FD (uno_dft2d_forward_resample) against K7 + K1 at the Darcy 446^2 and 223^2 levels, Infinity Cache flushed before every timed launch:
median / min us.  python tools/dev/fdtime.py [lib.so|-] [446|223]   (a -DUNO_FD_KO=mask variant of tools/dev/mkvariant.py times the knock-outs)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from uno_amd import _native
if len(sys.argv) > 1 and sys.argv[1] != "-":
    _native.LIB_PATH = os.path.abspath(sys.argv[1])
from uno_amd.resample import fused_resample_tables, resample_adjoint, resample_forward
dev = torch.device("cuda:0")
torch.manual_seed(0)
level = int(sys.argv[2]) if len(sys.argv) > 2 else 446
junk = torch.empty(80 * 1024 * 1024, device=dev)      # 320 MB: flushes the Infinity Cache between timed launches
def timed(fn, n=12):
    ts = []
    for _ in range(n):
        junk.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]
# (channels, grid, modes, adjoint): the step's sites - 446: conv0 forward; 223: conv1 forward with c0's shared transform (modes 18), with its
# own modes (8), and conv4 backward (the adjoint of 111 -> 223, Hermitian weights and mask)
sites = [(64, 446, 18, False)] if level == 446 else [(128, 223, 18, False), (128, 223, 8, False), (128, 223, 8, True)]
who = os.path.basename(sys.argv[1]) if len(sys.argv) > 1 else "product"
for C, S, m, adj in sites:
    x = torch.randn(16, C, S, S, device=dev)
    tabs = fused_resample_tables(S, S, S // 2, S // 2, str(dev), adj)
    fused = lambda: _native.dft2d_forward_resample(x, m, m, S // 2, S // 2, tabs, 1.0, adj, adj)
    pair = lambda: ((resample_adjoint if adj else resample_forward)(x, S // 2, S // 2), _native.dft2d_forward(x, m, m, 1.0, adj, adj))
    for _ in range(3): fused(); pair()
    print(who, f"{16 * C} x {S}^2 modes {m}{' adjoint' if adj else ''}: fused median/min us %.1f %.1f" % timed(fused), "| K7 + K1 pair %.1f %.1f" % timed(pair), flush=True)
