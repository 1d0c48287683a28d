"""Time of the NS-2D evaluation roll-out (reference ns_train_2d.py:86-117, 133-168) at configuration C3 - UNO(14, 32), 64^2, batch 32 -
for T_f = 40 and T_f = 10, in three forms on the same model and inputs:
  stock    the reference's loop written out: channels-last window, model(xx), `cat` of the prediction, LpLoss per step and for the
           whole trajectory
  native   harness.ns2d_rollout_errors, eager: one uno_rollout_advance (K18) between two forward passes, one finish launch
  graph    harness.GraphedRollout: the native roll-out replayed from one HIP graph
(developer tool; bench.py is the contract).
usage: python tools/rollout_eval_time.py [calls]

One process, the forms alternated call by call; every form warmed up first; median and min .. max of `calls` (at least 30) timed calls,
device events around each call with one synchronisation at its end - the time covers the host's enqueueing where that is the longer of
the two.  The stock form is timed a second time as a fourth column (`stock again`): the distance between the two stock columns is the
run-to-run spread the other differences are read against.  A fifth, `graph in place`, is the replay on a batch that already lies in the
graph's input buffers (GraphedRollout.static_in): the replay without the two input copies.  Needs an MI355X: there is no CPU path."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from uno_amd.harness import UNO, GraphedRollout, ns2d_rollout_errors

if not torch.cuda.is_available():
    sys.exit("rollout_eval_time.py: no HIP device")
calls = max(30, int(sys.argv[1])) if sys.argv[1:] else 30
dev = torch.device("cuda:0")
B, S, T_IN, WIDTH = 32, 64, 10, 32


def lp_loss(x, y):
    """LpLoss(size_average=False).rel written out (utilities3.py:86-100)"""
    n = x.shape[0]
    diff = torch.norm(x.reshape(n, -1) - y.reshape(n, -1), 2, 1)
    return torch.sum(diff / torch.norm(y.reshape(n, -1), 2, 1))


def stock_loop(model, xx, yy, T_f):
    """ns_train_2d.py:141-157 -> (test_l2_step, test_l2) of one batch"""
    with torch.no_grad():
        loss = 0
        for t in range(T_f):
            y = yy[..., t:t + 1]
            im = model(xx)
            loss = loss + lp_loss(im.reshape(B, -1), y.reshape(B, -1))
            pred = im if t == 0 else torch.cat((pred, im), -1)
            xx = torch.cat((xx[..., 1:], im), dim=-1)
        return loss, lp_loss(pred.reshape(B, -1), yy.reshape(B, -1))


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return sorted(v)[len(v) // 2], min(v), max(v)


def ab(forms, n, warm=3):
    """-> {name: (median, min, max)} in ms; the forms alternate call by call"""
    for _ in range(warm):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(n):
        for k, fn in forms.items():
            t[k].append(one(fn))
    return {k: stats(v) for k, v in t.items()}


def fmt(s):
    return f"{s[0]:8.3f} ms ({s[1]:.3f} .. {s[2]:.3f})"


def dist(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


print(f"# NS-2D evaluation roll-out, UNO({T_IN + 4}, {WIDTH}), {S}^2, batch {B}, float32, synthetic data, one MI355X "
      f"({torch.cuda.get_device_name(0)}); {calls} alternated calls each, median (min .. max)")
torch.manual_seed(0)
model = UNO(T_IN + 4, WIDTH).to(dev).eval()
for T_f in (40, 10):
    g = torch.Generator().manual_seed(T_f)
    xx, yy = torch.randn(B, S, S, T_IN, generator=g).to(dev), torch.randn(B, S, S, T_f, generator=g).to(dev)
    graphed = GraphedRollout(model, T_f, (xx, yy))
    s_step, s_full = stock_loop(model, xx, yy, T_f)
    n = ns2d_rollout_errors(model, xx, yy, T_f).errors
    r = graphed.errors(xx, yy).errors
    forms = {"stock": lambda: stock_loop(model, xx, yy, T_f), "native": lambda: ns2d_rollout_errors(model, xx, yy, T_f),
             "graph": lambda: graphed.errors(xx, yy), "stock again": lambda: stock_loop(model, xx, yy, T_f),
             "graph in place": lambda: graphed.errors(*graphed.static_in)}
    res = ab(forms, calls)
    print(f"T_f = {T_f}")
    for k, v in res.items():
        print(f"  {k:12s} {fmt(v)}   {v[0] / res['stock'][0]:.3f} of stock")
    print(f"  spread between the two stock columns {abs(res['stock'][0] - res['stock again'][0]) / res['stock'][0]:.2%} of the median")
    print(f"  value distance: native / stock step_sum {dist(n.step_sum, s_step):.1e} full_sum {dist(n.full_sum, s_full):.1e}   "
          f"graph / native step_sum {dist(r.step_sum, n.step_sum):.1e} full_sum {dist(r.full_sum, n.full_sum):.1e}")
    del graphed
    torch.cuda.empty_cache()
