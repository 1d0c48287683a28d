"""K1-FD (uno_dft2d_forward_resample) against K7 + K1 at the Darcy 446^2 level, Infinity Cache flushed before every timed launch: median / min us.
python tools/dev/fdtime.py [lib.so|-]   (a -DUNO_FD_KO=mask variant of tools/dev/mkvariant.py times the knock-outs)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from uno_amd import _native
if len(sys.argv) > 1 and sys.argv[1] != "-":
    _native.LIB_PATH = os.path.abspath(sys.argv[1])
from uno_amd.resample import fused_resample_tables, resample_forward
dev = torch.device("cuda:0")
torch.manual_seed(0)
x = torch.randn(16, 64, 446, 446, device=dev)
junk = torch.empty(80 * 1024 * 1024, device=dev)      # 320 MB: flushes the Infinity Cache between timed launches
tabs = fused_resample_tables(446, 446, 223, 223, str(dev), False)
def timed(fn, n=12):
    ts = []
    for _ in range(n):
        junk.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]
fused = lambda: _native.dft2d_forward_resample(x, 18, 18, 223, 223, tabs, 1.0)
pair = lambda: (resample_forward(x, 223, 223), _native.dft2d_forward(x, 18, 18, 1.0))
for _ in range(3): fused(); pair()
print(os.path.basename(sys.argv[1]) if len(sys.argv) > 1 else "product", "fused median/min us %.1f %.1f" % timed(fused), "| K7 + K1 pair %.1f %.1f" % timed(pair), flush=True)
