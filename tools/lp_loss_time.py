"""Time of the training loss `LpLoss(size_average=False)(out.view(B, -1), y.view(B, -1))` forward + backward (reference
utilities3.py:86-100, train_darcy.py:53-54) in its two forms: the native one (harness.LpLoss -> uno_rel_l2_forward / uno_rel_l2_backward,
K20: two launches forward, one backward) and the stock ops of lp_loss_rel_sum (`sub`, two `norm`s, `div`, `sum` and their backward),
at (B, N) = (16, 421^2), the Darcy headline, and (32, 64^2), one step of the NS-2D roll-out; the device launches of one call of each
form, counted with torch.profiler; then the Darcy step at 421^2, batch 16, UNO_9(3, 64, pad=5) written as train_darcy.py:47-59 writes
it - `.item()` and `gc.collect()` included, then without the collection, then without either - on the drop-in classes (dropin/),
beside the same loop with the loss in stock ops and harness.DarcyTrainer.step on the same data; then the NS-2D roll-out step of
ns_train_2d.py:46-68 (UNO(14, 32), 64^2, batch 32, T_f = 10, eager) with LpLoss on K20 and with the loss in stock ops
(developer tool; bench.py is the contract).
usage: python tools/lp_loss_time.py [calls] [all | loss | darcy | ns2d]

One process, the forms alternated call by call; every shape warmed up first; median and min .. max of `calls` (at least 50) timed calls
(20 steps for the Darcy section), device events around each call with one synchronisation at its end - the time covers the host's
enqueueing where that is the longer of the two.  Needs an MI355X: there is no CPU path."""
import gc
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[0:0] = [os.path.join(ROOT, "dropin"), ROOT]
import torch

from uno_amd.harness import DarcyTrainer, LpLoss, lp_loss_rel_sum, synthetic_darcy_batch

if not torch.cuda.is_available():
    sys.exit("lp_loss_time.py: no HIP device")
section = "all"
if sys.argv[1:] and sys.argv[-1] in ("all", "loss", "darcy", "ns2d"):
    section = sys.argv.pop()
calls = max(50, int(sys.argv[1])) if sys.argv[1:] else 60
dev = torch.device("cuda:0")
SHAPES = [(16, 421 * 421), (32, 64 * 64)]


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return sorted(v)[len(v) // 2], min(v), max(v)


def ab(forms, n, warm=5):
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


def launches(fn):
    """device kernels and memory operations one call of fn enqueues, or None where the profiler gives no device events"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA]
    return names or None


def loss_section():
    print(f"# LpLoss(size_average=False) forward + backward on (B, N) float32, one MI355X ({torch.cuda.get_device_name(0)}); "
          f"{calls} alternated calls each, median (min .. max)")
    myloss = LpLoss(size_average=False)
    faster = []
    for B, N in SHAPES:
        g = torch.Generator().manual_seed(1)
        y = torch.randn(B, N, generator=g).to(dev)
        x = (y + 0.1 * torch.randn(B, N, generator=g).to(dev)).requires_grad_(True)

        def native():
            x.grad = None
            loss = myloss(x, y)
            loss.backward()
            return loss

        def stock():
            x.grad = None
            loss = lp_loss_rel_sum(x, y)
            loss.backward()
            return loss
        a, ga = float(native().detach()), x.grad.clone()
        b, gb = float(stock().detach()), x.grad.clone()
        r = ab({"native": native, "stock": stock}, calls)
        moved = 20.0 * B * N / 1e6            # forward reads x and y, backward reads both and writes the gradient
        print(f"({B}, {N})  native {fmt(r['native'])}   stock {fmt(r['stock'])}   ratio {r['native'][0] / r['stock'][0]:.3f}"
              f"   {moved:.1f} MB algorithmic = {moved / r['native'][0] / 1e3:.2f} TB/s   value distance {abs(a - b) / abs(b):.1e}"
              f"   gradient distance {float((ga - gb).norm() / gb.norm()):.1e}")
        faster.append(r["native"][0] < r["stock"][0])
        try:
            ln, ls = launches(native), launches(stock)
        except Exception as e:                  # the profiler is a convenience here: the timings above do not depend on it
            ln = ls = None
            print(f"    launch count unavailable: {type(e).__name__}: {e}")
        if ln and ls:
            print(f"    device launches per forward + backward: native {len(ln)}, stock {len(ls)}")
            print(f"      native: {', '.join(n.split('(')[0][-48:] for n in ln)}")
            print(f"      stock:  {', '.join(n.split('(')[0][-48:] for n in ls)}")
    print("# native is faster at both sizes" if all(faster) else "# native is NOT faster at: "
          + ", ".join(str(s) for s, f in zip(SHAPES, faster) if not f))


def darcy_section():
    import darcy_flow_uno2d
    from Adam import Adam
    import utilities3
    steps = 20
    S, B = 421, 16
    a, u = synthetic_darcy_batch(B, S, 1234, dev)
    torch.manual_seed(0)
    model = darcy_flow_uno2d.UNO_9(3, 64, pad=5).to(dev)
    optimizer = Adam(model.parameters(), lr=1e-3, weight_decay=1e-3, amsgrad=False)
    myloss = utilities3.LpLoss(size_average=False)
    torch.manual_seed(0)
    twin = darcy_flow_uno2d.UNO_9(3, 64, pad=5).to(dev)
    trainer = DarcyTrainer(twin, lr=1e-3, weight_decay=1e-3)
    state = {"train_l2": 0.0}

    def script_step():
        """train_darcy.py:47-59 (the batch is already on the device)"""
        x, y = a.cuda(), u.cuda()
        batch_size = x.shape[0]
        optimizer.zero_grad()
        out = model(x).reshape(batch_size, S, S)
        loss = myloss(out.view(batch_size, -1), y.view(batch_size, -1))
        loss.backward()
        optimizer.step()
        state["train_l2"] += loss.item()
        del x, y, out, loss
        gc.collect()

    def script_step_no_gc(item=True):
        """the same without the script's `gc.collect()`, and without its `.item()` too"""
        optimizer.zero_grad()
        out = model(a).reshape(B, S, S)
        loss = myloss(out.view(B, -1), u.view(B, -1))
        loss.backward()
        optimizer.step()
        if item:
            state["train_l2"] += loss.item()

    def script_step_stock_loss():
        """the loop body without `.item()` and `gc.collect()`, the loss in stock ops"""
        optimizer.zero_grad()
        out = model(a).reshape(B, S, S)
        lp_loss_rel_sum(out.view(B, -1), u.view(B, -1)).backward()
        optimizer.step()

    r = ab({"script": script_step, "script_no_gc": script_step_no_gc, "script_no_sync": lambda: script_step_no_gc(False),
            "stock_loss": script_step_stock_loss, "trainer": lambda: trainer.step(a, u)}, steps, warm=3)
    print(f"# Darcy {S}^2, batch {B}, UNO_9(3, 64, pad=5), float32, synthetic data; {steps} alternated steps each, median (min .. max)")
    for key, what in (("script", "train_darcy.py:47-59 on dropin/ (with .item() and gc.collect())"),
                      ("script_no_gc", "the same loop body without gc.collect()"),
                      ("script_no_sync", "the same loop body without .item() and gc.collect()"),
                      ("stock_loss", "  ... and with the loss in stock ops (lp_loss_rel_sum)"), ("trainer", "harness.DarcyTrainer.step")):
        print(f"{what:66s} {fmt(r[key])} = {B / r[key][0] * 1e3:7.1f} samples/s")


def ns2d_section():
    import navier_stokes_uno2d
    from Adam import Adam
    import utilities3
    steps, S, B, T_in, T_f = 10, 64, 32, 10, 10
    torch.manual_seed(0)
    model = navier_stokes_uno2d.UNO(T_in + 4, 32).to(dev)
    optimizer = Adam(model.parameters(), lr=1e-3, weight_decay=1e-3, amsgrad=False)
    g = torch.Generator().manual_seed(2)
    xx0, yy = torch.randn(B, S, S, T_in, generator=g).to(dev), torch.randn(B, S, S, T_f, generator=g).to(dev)

    def rollout_step(myloss):
        """ns_train_2d.py:46-68 without its `.item()`"""
        loss, xx = 0, xx0
        for t in range(T_f):
            y = yy[..., t:t + 1]
            im = model(xx)
            loss += myloss(im.reshape(B, -1), y.reshape(B, -1))
            xx = torch.cat((xx[..., 1:], im), dim=-1)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()

    native, stock = utilities3.LpLoss(size_average=False), lp_loss_rel_sum
    r = ab({"native": lambda: rollout_step(native), "stock": lambda: rollout_step(stock)}, steps, warm=2)
    print(f"# NS-2D roll-out step as ns_train_2d.py:46-68 writes it, UNO({T_in + 4}, 32), {S}^2, batch {B}, T_f = {T_f}, eager, on dropin/; "
          f"{steps} alternated steps each, median (min .. max)")
    print(f"LpLoss on K20 {fmt(r['native'])}   loss in stock ops {fmt(r['stock'])}   ratio {r['native'][0] / r['stock'][0]:.3f}")


if section in ("all", "loss"):
    loss_section()
if section in ("all", "darcy"):
    darcy_section()
if section in ("all", "ns2d"):
    ns2d_section()
