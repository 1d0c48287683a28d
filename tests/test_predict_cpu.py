"""The predict stage (uno_amd/harness/predict.py) on the host: the checkpoint record's round trip, the Predictor against direct calls of
the model (models on the oracle's blocks through `block_cls`: the product's spectral layers have no CPU path), the resolution check
against the kernel families' own predicates, the command line's argument errors and its .mat file.

Nothing here has a tolerance: batching must give the rows a direct call gives (the oracle blocks treat every sample on its own), so
rows are compared bit for bit where the same ops ran on the same batch and with torch's default allclose where the batch size differs
(the stock GEMMs may block a batch of 2 and of 5 differently)."""
import json

import pytest
import torch

import dropin_loops
from oracle import spectral_oracle as so
from uno_amd.harness import DeviceDataset, MatReader, lp_loss_rel_sum, models
from uno_amd.harness import predict as P
from uno_amd.spectral3d import _resample3d_pruned_applies, resample3d_any_applies, resample3d_wide_applies

B2, B3 = so.OracleOperatorBlock2d, so.OracleOperatorBlock3d


def block_of(cls):
    return B3 if issubclass(cls, models.Uno3D_T20) else B2


# (class name, in_width, width, further constructor arguments): every class of harness.models, at a small width
ALL = [("UNO_9", 3, 4, {"pad": 5}), ("UNO", 7, 4, {}), ("UNO_P", 7, 4, {"pad": 4}), ("UNO_S256", 5, 4, {}),
       ("Uno3D_T20", 6, 2, {"pad": 3}), ("Uno3D_T10", 6, 2, {}), ("Uno3D_T9", 6, 2, {"pad": 3, "pad_both": True}), ("Uno3D_T40", 6, 2, {}),
       ("Uno3D_T20_256", 6, 2, {}), ("Uno3D_T10_256", 6, 2, {"factor": 1})]


def same_parameters(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


# ------------------------------------------------------------------------------------------------------------ record round trip
def test_every_model_class_is_listed():
    import inspect
    classes = sorted(n for n, c in vars(models).items() if inspect.isclass(c) and issubclass(c, torch.nn.Module) and c.__module__ == models.__name__)
    assert classes == sorted(P.MODEL_CLASSES) == sorted(a[0] for a in ALL)


@pytest.mark.parametrize("name,in_width,width,kw", ALL, ids=[a[0] for a in ALL])
def test_record_round_trip_for_every_model_class(name, in_width, width, kw, tmp_path):
    cls = getattr(models, name)
    torch.manual_seed(3)
    model = cls(in_width, width, block_cls=block_of(cls), **kw)
    weights = str(tmp_path / "w.pt")
    torch.save(model.state_dict(), weights)
    record = {"model": name, "ctor": {"in_width": in_width, "width": width, **kw}}
    with open(weights + ".json", "w") as f:
        json.dump(record, f)
    for again in (P.load_model(weights, block_cls=block_of(cls)),                                # the record beside the weights
                  P.load_model(weights, weights + ".json", block_cls=block_of(cls)),
                  P.load_model(model.state_dict(), record, block_cls=block_of(cls)),
                  P.load_model(weights, model=name, in_width=in_width, width=width, block_cls=block_of(cls), **kw)):    # no record
        assert type(again) is cls and not again.training
        same_parameters(model, again)


@pytest.mark.parametrize("loop", dropin_loops.LOOPS)
def test_record_round_trip_for_the_recorded_tiny_configurations(loop, tmp_path):
    cfg = dropin_loops.record()["loops"][loop]
    blk = B3 if loop == "ns3d" else B2
    model = dropin_loops.build_model(cfg, models, blk)
    weights = str(tmp_path / "w.pt")
    torch.save(model.state_dict(), weights)
    record = {"model": cfg["cls"], "ctor": {"in_width": cfg["ctor"][0], "width": cfg["ctor"][1], **cfg["ctor_kw"]}}
    again = P.load_model(weights, record, block_cls=blk)
    assert type(again).__name__ == cfg["cls"]
    same_parameters(model, again)


def test_fit_writes_the_record_load_model_reads(tmp_path):
    """fit's own record, without a training run: checkpoint_record on the parsed arguments' stand-in"""
    from types import SimpleNamespace
    from uno_amd.harness import fit
    model = models.UNO(14, 4, block_cls=B2)
    a = SimpleNamespace(loop="ns2d", in_width=14, width=4, pad=None, factor=None, sub=1, size=64, samples=None, gen_batch=7, t_in=10, t_f=2,
                        ntrain=4, nval=2, ntest=1, seed=21)
    rec = fit.checkpoint_record(a, model, fit.FitRecord(best_epoch=0, best_val=0.5, test=(0.25, 0.125)))
    path = str(tmp_path / "w.pt.json")
    fit.write_record(path, rec)
    back = P.read_record(path)
    assert back == rec and back["model"] == "UNO" and back["ctor"] == {"in_width": 14, "width": 4} and back["test"] == [0.25, 0.125]
    assert {"loop", "t_in", "t_f", "size", "samples", "gen_batch", "ntrain", "nval", "ntest", "seed", "best_epoch", "best_val"} <= set(back)
    torch.save(model.state_dict(), str(tmp_path / "w.pt"))
    same_parameters(model, P.load_model(str(tmp_path / "w.pt"), block_cls=B2))


def test_a_missing_or_contradictory_record_is_named(tmp_path):
    model = models.UNO(14, 4, block_cls=B2)
    sd = model.state_dict()
    with pytest.raises(ValueError, match="no checkpoint record"):
        P.load_model(sd, block_cls=B2)
    with pytest.raises(ValueError, match="cannot be read"):
        P.load_model(sd, str(tmp_path / "absent.json"), block_cls=B2)
    with pytest.raises(ValueError, match='no "ctor" entry'):
        P.load_model(sd, {"model": "UNO"}, block_cls=B2)
    with pytest.raises(ValueError, match='no "width"'):
        P.load_model(sd, {"model": "UNO", "ctor": {"in_width": 14}}, block_cls=B2)
    rec = {"model": "UNO", "ctor": {"in_width": 14, "width": 4}}
    with pytest.raises(ValueError, match="model=UNO_P contradicts the record, which names UNO"):
        P.load_model(sd, rec, model="UNO_P", block_cls=B2)
    with pytest.raises(ValueError, match="width=8 contradicts the record, which holds width=4"):
        P.load_model(sd, rec, width=8, block_cls=B2)
    with pytest.raises(ValueError, match="no such class"):
        P.load_model(sd, model="UNO_10", in_width=14, width=4, block_cls=B2)
    with pytest.raises(ValueError, match="needs width="):
        P.load_model(sd, model="UNO", in_width=14, block_cls=B2)
    with pytest.raises(RuntimeError, match="size mismatch"):          # strict: the wrong width is load_state_dict's own error
        P.load_model(sd, model="UNO", in_width=14, width=8, block_cls=B2)
    same_parameters(model, P.load_model(sd, rec, width=4, pad=0, block_cls=B2))      # agreeing and additional arguments pass


# ------------------------------------------------------------------------------------------------------ Predictor vs direct call
def test_darcy_batches_give_the_rows_of_a_direct_call():
    torch.manual_seed(5)
    model = models.UNO_9(3, 4, pad=5, block_cls=B2)
    g = torch.Generator().manual_seed(1)
    x, y = torch.rand(5, 72, 72, 1, generator=g), torch.rand(5, 72, 72, generator=g)
    model.train()
    r = P.Predictor(model, batch_size=2).darcy(x, y)                    # batches of 2, 2 and 1
    assert model.training                                               # the previous mode is back
    model.eval()
    with torch.no_grad():
        whole = model(x).reshape(5, 72, 72)
        by_batch = torch.cat([model(x[lo:lo + 2]).reshape(-1, 72, 72) for lo in (0, 2, 4)])
    assert r.pred.shape == (5, 72, 72) and torch.equal(r.pred, by_batch)
    assert torch.allclose(r.pred, whole)
    each = torch.stack([lp_loss_rel_sum(by_batch[i:i + 1], y[i:i + 1]) for i in range(5)])
    assert r.err.shape == (5,) and torch.allclose(r.err, each, rtol=1e-6, atol=0)
    assert r.err_step is None and r.err_full is None
    again = P.Predictor(model, batch_size=2).darcy(DeviceDataset(x, y))
    assert torch.equal(again.pred, r.pred) and torch.equal(again.err, r.err)
    assert P.Predictor(model, batch_size=8).darcy(x).err is None


def test_ns2d_stock_path_is_the_reference_loop():
    """T_in 3, horizon 5, S 64 against the loop of ns_train_2d.py written out (the `cat` window); targets for the first 3 steps only"""
    torch.manual_seed(6)
    model = models.UNO(7, 4, block_cls=B2)
    g = torch.Generator().manual_seed(2)
    xx, yy = torch.randn(3, 64, 64, 3, generator=g), torch.randn(3, 64, 64, 3, generator=g)
    r = P.Predictor(model, batch_size=2).ns2d(xx, 5, yy)
    assert r.pred.shape == (3, 64, 64, 5) and r.err_step.shape == (3, 3) and r.err_full.shape == (3,)
    model.eval()
    rows = []
    with torch.no_grad():
        for lo, hi in ((0, 2), (2, 3)):
            w, pred = xx[lo:hi], None
            for t in range(5):
                im = model(w)
                pred = im if t == 0 else torch.cat((pred, im), -1)
                w = torch.cat((w[..., 1:], im), dim=-1)
            rows.append(pred)
    pred = torch.cat(rows)
    assert torch.equal(r.pred, pred)
    for b in range(3):
        for t in range(3):
            assert torch.allclose(r.err_step[b, t], lp_loss_rel_sum(pred[b:b + 1, ..., t], yy[b:b + 1, ..., t]), rtol=1e-6, atol=0)
        assert torch.allclose(r.err_full[b], lp_loss_rel_sum(pred[b:b + 1, ..., :3], yy[b:b + 1]), rtol=1e-6, atol=0)
    free = P.Predictor(model, batch_size=2).ns2d(xx, 5)
    assert torch.equal(free.pred, pred) and free.err_step is None
    assert P.Predictor(model, batch_size=2).ns2d(xx, yy=yy).pred.shape == (3, 64, 64, 3)         # the horizon defaults to yy's length
    with pytest.raises(ValueError, match="horizon"):
        P.Predictor(model).ns2d(xx)
    with pytest.raises(ValueError, match="horizon = 0"):
        P.Predictor(model).ns2d(xx, 0)


def test_ns3d_two_calls_are_two_hand_chained_calls():
    torch.manual_seed(7)
    model = models.Uno3D_T10(6, 2, pad=3, block_cls=B3)
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(3, 32, 32, 10, 1, generator=g), torch.randn(3, 32, 32, 20, generator=g)
    r = P.Predictor(model, batch_size=2).ns3d(x, calls=2, y=y)
    assert r.pred.shape == (3, 32, 32, 20) and r.err_step.shape == (3, 20) and r.err_full.shape == (3,)
    model.eval()
    rows = []
    with torch.no_grad():
        for lo, hi in ((0, 2), (2, 3)):
            first = model(x[lo:hi])
            second = model(first[..., -10:, :])
            rows.append(torch.cat((first, second), dim=-2).reshape(hi - lo, 32, 32, 20))
    pred = torch.cat(rows)
    assert torch.equal(r.pred, pred)
    for b in range(3):
        assert torch.allclose(r.err_step[b, 13], lp_loss_rel_sum(pred[b:b + 1, ..., 13], y[b:b + 1, ..., 13]), rtol=1e-6, atol=0)
        assert torch.allclose(r.err_full[b], lp_loss_rel_sum(pred[b:b + 1], y[b:b + 1]), rtol=1e-6, atol=0)
    one = P.Predictor(model, batch_size=4).ns3d(x[..., 0])               # (n, S, S, T_in) is taken too
    assert one.pred.shape == (3, 32, 32, 10) and torch.allclose(one.pred, pred[..., :10]) and one.err_step is None
    with pytest.raises(ValueError, match="calls = 0"):
        P.Predictor(model).ns3d(x, calls=0)
    with pytest.raises(ValueError, match="30 target frames, 2 call"):
        P.Predictor(model).ns3d(x, calls=2, y=torch.randn(3, 32, 32, 30))


# ------------------------------------------------------------------------------------------------------------- resolution check
def families(cls, S, T_in, **kw):
    model = cls(6, 2, **kw)                     # product blocks: nothing is launched, the check is host arithmetic
    enable_both(model)
    return {lp.name: lp.family for lp in P.check_resolution(model, S, T_in)}, model


def enable_both(model):
    from uno_amd.integral_operators import enable_native_resample3d_any, enable_native_resample3d_wide
    enable_native_resample3d_any(model)
    enable_native_resample3d_wide(model)


def test_resolution_check_holds_the_traced_table_for_uno3d_t20():
    f, _ = families(models.Uno3D_T20, 64, 10, pad=3)
    assert set(f.values()) == {"pruned"} and list(f) == list(models.Uno3D_T20._NAMES)
    f, _ = families(models.Uno3D_T20, 80, 10, pad=3)
    assert {k for k, v in f.items() if v != "pruned"} == {"conv8"} and f["conv8"] == "any"
    f, _ = families(models.Uno3D_T20, 256, 10, pad=3)
    assert {k for k, v in f.items() if v == "wide"} == {"conv0", "conv1", "conv7", "conv8"}


CLASSES_3D = [(models.Uno3D_T20, (64, 80, 96, 128, 256), (10, 20)), (models.Uno3D_T10, (64, 80, 96, 128, 256), (10, 20)),
              (models.Uno3D_T40, (64, 80, 96, 128, 256), (10, 20)), (models.Uno3D_T9, (64, 96, 128), (6,))]


@pytest.mark.parametrize("cls,sizes,t_ins", CLASSES_3D, ids=[c[0].__name__ for c in CLASSES_3D])
def test_every_layer_has_a_native_family_and_it_is_the_predicates_choice(cls, sizes, t_ins):
    """One combination of the table has NO native family, by the predicates themselves: Uno3D_T40 at S = 256 with T_in = 20 stretches
    the padded time axis of 26 to 83 and 104 points at conv7 / conv8, past the wide-axis family's last-axis limit of 64 (and S = 256 is
    past the any-grid family's 128).  It must be refused, naming conv7; every other combination must pass."""
    model = cls(6, 2, pad=3)
    enable_both(model)
    for S in sizes:
        for T_in in t_ins:
            if (cls, S, T_in) == (models.Uno3D_T40, 256, 20):
                with pytest.raises(ValueError, match=r"layer conv7 resamples \(128, 128, 62\) -> \(192, 192, 83\), which no native kernel family"):
                    P.check_resolution(model, S, T_in)
                continue
            plan = P.check_resolution(model, S, T_in)
            assert [lp.name for lp in plan] == list(cls._NAMES)
            padding = int(3 * 0.1 * T_in)
            grids, _ = cls._plan(S, S, T_in + padding, padding)
            din = (S, S, T_in + padding)
            for lp, dout in zip(plan, grids):
                assert (lp.din, lp.dout) == (din, tuple(dout))
                want = "pruned" if _resample3d_pruned_applies(din, dout) else "any" if resample3d_any_applies(din, dout) else \
                    "wide" if resample3d_wide_applies(din, dout) else None
                assert lp.family == want and want is not None, (S, T_in, lp)
                din = tuple(dout)


def test_a_layer_no_family_takes_is_named():
    model = models.Uno3D_T20(6, 2, pad=3)                   # the default model: not opted in
    with pytest.raises(ValueError, match=r"layer conv8 resamples \(60, 60, 26\) -> \(80, 80, 26\), which no native kernel family takes"):
        P.check_resolution(model, 80, 10)
    enable_both(model)
    with pytest.raises(ValueError, match="layer conv0 resamples"):
        P.check_resolution(model, 320, 10)                  # beyond the wide-axis family's 256
    oracle = models.Uno3D_T20(6, 2, pad=3, block_cls=B3)    # oracle blocks run torch.fft: any grid the modes fit
    assert {lp.family for lp in P.check_resolution(oracle, 80, 10)} == {None}


def test_modes_that_do_not_fit_are_refused_naming_the_layer():
    with pytest.raises(ValueError, match=r"Uno3D_T9 at 32 x 32 x 6: layer conv1 keeps 18 modes on axis 1, .* output grid \(16, 16, 7\) has 16"):
        P.check_resolution(models.Uno3D_T9(6, 2, pad=3, block_cls=B3), 32, 6)
    assert len(P.check_resolution(models.Uno3D_T9(6, 2, pad=3, block_cls=B3), 36, 6)) == 7
    with pytest.raises(ValueError, match=r"UNO at 48 x 48: layer L0 keeps 22 modes on axis 2, .* output grid \(36, 36\) has 36"):
        P.check_resolution(models.UNO(14, 4, block_cls=B2), 48)
    assert [lp.dout for lp in P.check_resolution(models.UNO(14, 4, block_cls=B2), 96)] == [(72, 72), (48, 48), (24, 24), (24, 24), (48, 48), (72, 72), (96, 96)]
    with pytest.raises(ValueError, match="UNO_S256 at 128 x 128: layer L0"):
        P.check_resolution(models.UNO_S256(5, 4, block_cls=B2), 128)
    assert len(P.check_resolution(models.UNO_S256(5, 4, block_cls=B2), 256)) == 7
    # (the 3-D 256 models' modes still fit at half their design grid - 32 modes on 128 // 4 points - and no further down)
    assert len(P.check_resolution(models.Uno3D_T20_256(6, 2, block_cls=B3), 128, 10)) == 9
    with pytest.raises(ValueError, match=r"Uno3D_T20_256 at 64 x 64 x 10: layer conv0 keeps 32 modes on axis 1, .* output grid \(16, 16, 12\) has 16"):
        P.check_resolution(models.Uno3D_T20_256(6, 2, block_cls=B3), 64, 10)
    plan = P.check_resolution(models.UNO_9(3, 4, pad=5, block_cls=B2), 86)                       # the padding scale is ceil(86 / 85) = 2
    assert plan[0].din == (96, 96) and plan[-1].dout == (96, 96)
    assert P.check_resolution(models.UNO_9(3, 4, pad=5, block_cls=B2), 85)[0].din == (90, 90)
    with pytest.raises(ValueError, match="UNO_9 at 30 x 30: layer conv0 keeps 18 modes on axis 1"):
        P.check_resolution(models.UNO_9(3, 4, pad=5, block_cls=B2), 30)


def test_the_predictor_refuses_a_grid_before_running_anything():
    model = models.UNO(7, 4, block_cls=B2)
    calls = []
    model.register_forward_pre_hook(lambda *a: calls.append(1))
    with pytest.raises(ValueError, match="layer L0"):
        P.Predictor(model).ns2d(torch.randn(1, 48, 48, 3), 2)
    assert not calls


# --------------------------------------------------------------------------------------------------------------- command line
def run_main(args, capsys):
    with pytest.raises(SystemExit) as e:
        P.main(args)
    return e.value, capsys.readouterr().err


def test_command_line_argument_errors(tmp_path, capsys):
    base = ["--weights", str(tmp_path / "w.pt"), "--data", str(tmp_path / "d.mat")]
    explicit = ["--model", "UNO", "--in-width", "14", "--width", "4"]
    for args, words in ((["ns2d", *base], "no checkpoint record"),
                        (["ns2d", *base, "--model", "UNO"], "--in-width and --width"),
                        (["ns2d", *base, *explicit, "--calls", "2"], "--calls belongs to ns3d"),
                        (["ns3d", *base, *explicit, "--horizon", "5"], "--horizon belongs to ns2d"),
                        (["darcy", *base, *explicit, "--size", "64"], "--sub belongs to darcy"),
                        (["ns2d", *base, *explicit, "--sub", "2"], "--sub belongs to darcy"),
                        (["ns2d", *base, *explicit, "--no-pred"], "--no-pred without --out"),
                        (["ns2d", *base, *explicit], "needs --ntrain, --nval, --ntest and --seed"),
                        (["ns2d", *base, *explicit, "--split", "all"], "--samples"),
                        (["ns2d", *base, "--record", str(tmp_path / "absent.json")], "cannot be read"),
                        (["burgers", *base], "invalid choice")):
        status, err = run_main(args, capsys)
        assert status.code == 2 and words in err, (args, err)
    with open(tmp_path / "w.pt.json", "w") as f:
        json.dump({"loop": "darcy", "model": "UNO_9", "ctor": {"in_width": 3, "width": 4}, "ntrain": 4, "nval": 2, "ntest": 1, "seed": 1}, f)
    status, err = run_main(["ns2d", *base], capsys)
    assert status.code == 2 and "records a darcy run, not ns2d" in err


def test_the_mat_file_is_read_back_by_matreader(tmp_path):
    pytest.importorskip("scipy.io")
    g = torch.Generator().manual_seed(4)
    pred = torch.randn(3, 8, 8, 5, generator=g).permute(0, 2, 3, 1).permute(0, 3, 1, 2)         # a view, as ns2d returns one
    r = P.Prediction(pred, err_step=torch.rand(3, 2, generator=g), err_full=torch.rand(3, generator=g))
    index = torch.tensor([6, 0, 3])
    path = str(tmp_path / "pred.mat")
    P.write_mat(path, r, index)
    reader = MatReader(path)
    assert torch.equal(reader.read_field("pred"), pred)
    assert torch.equal(reader.read_field("err_step"), r.err_step) and torch.equal(reader.read_field("err_full").reshape(-1), r.err_full)
    assert reader.read_field("index").reshape(-1).tolist() == [6.0, 0.0, 3.0]
    P.write_mat(path, P.Prediction(pred[..., 0], err=r.err_full), index, with_pred=False)
    reader = MatReader(path)
    assert "pred" not in reader.data and torch.equal(reader.read_field("err").reshape(-1), r.err_full)


def test_the_split_is_fits_split():
    from uno_amd.harness import fit
    a = torch.arange(9.0).reshape(9, 1)
    parts = fit._split(a, a, 4, 2, 2, 17)
    cuts = fit._split_cuts(9, 4, 2, 2, 17)
    assert [p[0].reshape(-1).tolist() for p in parts] == [c.tolist() for c in cuts]
    assert sorted(torch.cat(cuts).tolist()) == sorted(set(torch.cat(cuts).tolist())) and len(torch.cat(cuts)) == 8
