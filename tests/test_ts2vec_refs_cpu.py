"""CPU side of the TS2Vec encoder: the restatement of tests/ts2vec_refs.py against the reference's recorded outputs
(tests/golden/ts2vec_*.npz, make_golden_ts2vec.py), state-dict and checkpoint interoperability, and every argument
error of encode, the probes and the command-line tool -- none of which needs a device."""
import argparse
import os

import numpy as np
import pytest
import torch

import ts2vec_refs as R
from conftest import GOLDEN, golden

CASES = {"a": dict(input_dims=2, hidden_dims=16, output_dims=32, depth=3),
         "b": dict(input_dims=1, hidden_dims=16, output_dims=16, depth=6),
         "c": dict(input_dims=3, hidden_dims=32, output_dims=48, depth=2)}
SAVED = os.path.join(GOLDEN, "ts2vec_saved.pt")


def _weights(f):
    return {k[2:]: f[k] for k in f.files if k.startswith("w/")}


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", CASES)
def test_f64_restatement_reproduces_the_reference(name):
    """Semantics, not rounding: the reference's fp32 forward is within 1e-6 of the f64 restatement (its own fp32 / fp64
    difference is 1.2e-6 at max |y| = 3.1 on a default-width net) for every mask and both windows."""
    f = golden(f"ts2vec_{name}.npz")
    sd = _weights(f)
    j = 0
    while f"x{j}" in f.files:
        x = f[f"x{j}"]
        for mk in R.MASKS:
            m = R.mask_of(mk, x.shape[0], x.shape[1], f[f"mask{j}"])
            for pooled, key in ((False, f"y{j}/{mk}"), (True, f"pool{j}/{mk}")):
                got = R.encode_ref(sd, x, m, torch.float64, pooled).numpy()
                assert got.shape == f[key].shape
                assert np.isfinite(got).all() and np.abs(got - f[key]).max() <= 1e-6, (name, j, mk, pooled)
                got32 = R.encode_ref(sd, x, m, torch.float32, pooled).numpy()
                assert got32.dtype == np.float32 and np.abs(got32 - f[key]).max() <= 1e-5
        j += 1
    assert j == (2 if name == "c" else 1)


def test_fixture_cases_are_what_they_claim():
    a, b, c = (golden(f"ts2vec_{n}.npz") for n in "abc")
    assert a["x0"].shape == (3, 37, 2) and b["x0"].shape == (2, 20, 1)
    assert c["x0"].shape == (2, 1, 3) and c["x1"].shape == (2, 2, 3)
    nan = np.isnan(a["x0"])
    assert nan[0, 5].all() and nan[1, 10].tolist() == [False, True] and nan.sum() == 3
    assert R.n_blocks(R.plain(_weights(b))) == 7                  # dilations 1..64 against T = 20
    for f in (a, b, c):
        for mk in R.MASKS:
            assert np.array_equal(f[f"pool0/{mk}"], f[f"y0/{mk}"].max(1))
        assert not f["mask0"].all()


def test_missing_steps_in_the_restatement():
    """A step with one NaN channel counts as missing; an all-NaN sequence is the all-masked one."""
    sd = R.seeded_state(2, 16, 16, 2, seed=1)
    x = torch.randn(2, 9, 2, generator=torch.Generator().manual_seed(2))
    y = x.clone()
    y[0, 4, 1] = float("nan")
    keep = torch.ones(2, 9, dtype=torch.bool)
    keep[0, 4] = False
    assert torch.equal(R.encode_ref(sd, y), R.encode_ref(sd, x, keep))
    z = torch.full_like(x, float("nan"))
    assert torch.equal(R.encode_ref(sd, z), R.encode_ref(sd, x, torch.zeros(2, 9, dtype=torch.bool)))
    assert torch.isfinite(R.encode_ref(sd, z)).all()


# ------------------------------------------------------------------------------------------------ state dicts
@pytest.mark.parametrize("name", CASES)
def test_state_dict_keys_match_the_reference_both_ways(name):
    from arcweld.ts2vec import TSEncoder, averaged_state_dict, encoder_from_state_dict, strip_averaged
    ref = {k: torch.as_tensor(v) for k, v in _weights(golden(f"ts2vec_{name}.npz")).items()}
    enc = TSEncoder(CASES[name]["input_dims"], CASES[name]["output_dims"], hidden_dims=CASES[name]["hidden_dims"],
                    depth=CASES[name]["depth"])
    plain, n_avg = strip_averaged(ref)
    assert n_avg == 1
    own = enc.state_dict()
    assert list(own) == list(plain) and all(own[k].shape == plain[k].shape for k in own)
    enc.load_state_dict(plain)                                   # strict: the reference's dict loads as is
    back = averaged_state_dict(enc, n_avg)
    assert list(back) == list(ref)                               # and the AveragedModel's order comes back
    assert all(torch.equal(back[k], ref[k]) for k in ref)
    built = encoder_from_state_dict(ref)
    assert (built.input_dims, built.output_dims, built.hidden_dims, built.depth) == tuple(
        CASES[name][k] for k in ("input_dims", "output_dims", "hidden_dims", "depth"))
    assert not built.training


def test_the_reference_constructor_signature():
    import inspect
    from arcweld.ts2vec import TSEncoder
    from model.ts2vec import TS2Vec
    from model.ts2vec.encoder import TSEncoder as Same
    assert Same is TSEncoder
    assert list(inspect.signature(TSEncoder.__init__).parameters)[1:] == ["input_dims", "output_dims", "hidden_dims",
                                                                          "depth"]
    p = inspect.signature(TS2Vec.__init__).parameters
    assert list(p)[1:] == ["input_dims", "output_dims", "hidden_dims", "depth", "device", "lr", "batch_size",
                           "max_train_length", "temporal_unit", "after_iter_callback", "after_epoch_callback"]
    assert (p["output_dims"].default, p["hidden_dims"].default, p["depth"].default, p["batch_size"].default) == (
        320, 64, 10, 16)
    assert list(inspect.signature(TS2Vec.encode).parameters)[1:] == ["data", "mask", "encoding_window", "causal",
                                                                    "sliding_length", "sliding_padding", "batch_size"]


def test_loader_reads_the_file_ts2vec_save_writes(tmp_path):
    from arcweld.ts2vec import load_checkpoint
    from model.ts2vec import TS2Vec
    raw = torch.load(SAVED, map_location="cpu", weights_only=True)
    assert "n_averaged" in raw and all(k == "n_averaged" or k.startswith("module.") for k in raw)
    enc = load_checkpoint(SAVED)
    assert (enc.input_dims, enc.output_dims, enc.hidden_dims, enc.depth) == (3, 48, 32, 2)
    want = _weights(golden("ts2vec_c.npz"))
    for k, v in enc.state_dict().items():
        assert np.array_equal(v.numpy(), want["module." + k]), k
    m = TS2Vec(3, output_dims=48, hidden_dims=32, depth=2, device="cpu")
    m.load(SAVED)
    out = tmp_path / "again.pt"
    m.save(str(out))
    again = torch.load(str(out), map_location="cpu", weights_only=True)
    assert list(again) == list(raw) and all(torch.equal(again[k], raw[k]) and again[k].dtype == raw[k].dtype
                                            for k in raw)
    with pytest.raises(RuntimeError):                            # another architecture's file is refused (strict load)
        TS2Vec(3, output_dims=48, hidden_dims=32, depth=3, device="cpu").load(SAVED)
    with pytest.raises(ValueError, match="state_dict"):
        from arcweld.ts2vec import encoder_from_state_dict
        encoder_from_state_dict({"n_averaged": torch.tensor(1), "module.something": torch.zeros(1)})


def test_fit_points_at_the_follow_up():
    from model.ts2vec import TS2Vec
    with pytest.raises(NotImplementedError, match="not built"):
        TS2Vec(2, output_dims=16, hidden_dims=16, depth=1, device="cpu").fit(np.zeros((2, 8, 2)))


def test_the_binding_has_the_new_entry_points():
    from arcweld import _native as nat
    assert {"aw_ts_input_fc", "aw_ts_conv", "aw_ts_pool_workspace", "aw_ts_describe"} <= set(nat.SIGNATURES)
    assert nat.AW_TS_MAX_T >= 2000 and nat.AW_TS_MAX_WIDTH == 512 and nat.AW_TS_MAX_CIN == 8
    assert len(nat.SIGNATURES["aw_ts_conv"]) == 15


# ------------------------------------------------------------------------------------------------ encode's arguments
@pytest.mark.parametrize("kw, name", [
    (dict(mask="binomial"), "mask"), (dict(mask="continuous"), "mask"), (dict(mask="sometimes"), "mask"),
    (dict(mask=torch.ones(2, 9)), "mask"), (dict(mask=torch.ones(2, 8, dtype=torch.bool)), "mask"),
    (dict(encoding_window=5), "encoding_window"), (dict(encoding_window="multiscale"), "encoding_window"),
    (dict(encoding_window="full"), "encoding_window"), (dict(sliding_length=4), "sliding_length"),
    (dict(sliding_padding=2), "sliding_length"), (dict(causal=True), "causal"), (dict(batch_size=0), "batch_size"),
    (dict(batch_size=2.5), "batch_size")])
def test_encode_refuses_what_is_not_built(kw, name):
    from arcweld.ts2vec import TSEncoder
    enc = TSEncoder(2, 16, hidden_dims=16, depth=1)
    with pytest.raises(ValueError, match=f"^{name}: ") as e:
        enc.encode(torch.zeros(2, 9, 2), **kw)
    if kw.get("mask") in ("binomial", "continuous") or name in ("sliding_length", "causal") or kw.get(
            "encoding_window") in (5, "multiscale"):
        assert "not built" in str(e.value)


@pytest.mark.parametrize("data, name", [
    (torch.zeros(2, 9), "data"), (torch.zeros(2, 9, 3), "data"), (torch.zeros(2, 9, 2, dtype=torch.int64), "data"),
    ([[1.0]], "data"), (torch.zeros(1, 0, 2), "data"), (torch.zeros(1, 4097, 2), "data")])
def test_encode_refuses_bad_data(data, name):
    from arcweld.ts2vec import TSEncoder
    with pytest.raises(ValueError, match=f"^{name}: "):
        TSEncoder(2, 16, hidden_dims=16, depth=1).encode(data)


def test_encode_has_no_cpu_path():
    from arcweld import _native as nat
    from arcweld.ts2vec import TSEncoder
    with pytest.raises(nat.NativeError, match="no CPU path"):
        TSEncoder(2, 16, hidden_dims=16, depth=1).encode(torch.zeros(2, 9, 2))


# ------------------------------------------------------------------------------------------------ probes and the tool
def _splits():
    return [(torch.zeros(60, 200, 2), torch.arange(60) % 2) for _ in range(3)]


@pytest.mark.parametrize("probe", ["latent_knn_probe", "latent_linear_probe", "latent_svm_probe"])
def test_probes_take_the_ts2vec_dataset(probe):
    import arcweld.retrieve as r
    fn = getattr(r, probe)

    class Called(Exception):
        pass

    class Stub:
        def encode(self, x, encoding_window=None):
            assert encoding_window == "full_series" and tuple(x.shape[1:]) == (200, 2)
            raise Called

    with pytest.raises(ValueError, match="^ts2vec: dataset ts2vec needs"):
        fn(_splits(), 1, dataset="ts2vec")
    with pytest.raises(ValueError, match="^ts2vec: dataset ts2vec needs"):
        fn(_splits(), 1, dataset="ts2vec", ts2vec=object())
    with pytest.raises(ValueError, match="^ts2vec: belongs to dataset 'ts2vec'"):
        fn(_splits(), 1, dataset="asimow", ts2vec=Stub())
    with pytest.raises(ValueError) as e:                          # the existing message, to the letter
        fn(_splits(), 1, dataset="raw")
    assert str(e.value) == "dataset: expected 'asimow' or 'latent_vq_vae', got 'raw'"
    with pytest.raises(ValueError, match="^vqvae: dataset latent_vq_vae needs the frozen VQ-VAE$"):
        fn(_splits(), 1)
    if torch.cuda.is_available():                                 # past the checks the features come from encode
        with pytest.raises(Called):
            fn(_splits(), 1, dataset="ts2vec", ts2vec=Stub())


def test_dtw_keeps_requiring_the_raw_cycles():
    from arcweld.retrieve import latent_knn_probe
    with pytest.raises(ValueError, match="^metric: 'dtw' warps .* needs dataset 'asimow'"):
        latent_knn_probe(_splits(), 1, dataset="ts2vec", ts2vec=object(), metric="dtw")


def _args(*argv):
    import probe_latent_space as cli
    return cli, cli.parser().parse_args(list(argv))


def test_cli_ts2vec_dataset(tmp_path):
    cli, a = _args("--dataset", "ts2vec", "--ts2vec-model", SAVED)
    assert isinstance(a, argparse.Namespace) and a.dataset == "ts2vec" and a.ts2vec_model == SAVED
    enc = cli.load_ts2vec(a, "cpu")                               # widths and depth from the checkpoint's shapes
    assert (enc.input_dims, enc.output_dims, enc.hidden_dims, enc.depth) == (3, 48, 32, 2)
    assert cli.load_ts2vec(_args("--dataset", "asimow")[1], "cpu") is None
    for argv, msg in ((("--dataset", "ts2vec"), "--ts2vec-model"),
                      (("--dataset", "ts2vec", "--ts2vec-model", str(tmp_path / "none.pt")), "--ts2vec-model"),
                      (("--dataset", "asimow", "--ts2vec-model", SAVED), "--ts2vec-model belongs to --dataset ts2vec"),
                      (("--dataset", "ts2vec", "--ts2vec-model", SAVED, "--metric", "dtw"), "--dataset asimow")):
        for protocol in ("knn", "linear", "svm"):
            if "--metric" in argv and protocol != "knn":
                continue
            cli, a = _args(*argv, "--protocol", protocol, "--out", str(tmp_path / "o.json"))
            with pytest.raises(SystemExit) as e:
                cli.main(a)
            assert msg in str(e.value)
    bad = tmp_path / "bad.pt"
    torch.save({"n_averaged": torch.tensor(1), "module.x": torch.zeros(2)}, str(bad))
    with pytest.raises(SystemExit, match="not a TS2Vec checkpoint"):
        cli.load_ts2vec(_args("--dataset", "ts2vec", "--ts2vec-model", str(bad))[1], "cpu")
