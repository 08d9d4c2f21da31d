"""The scoring surface without a GPU: score_welding_cycles.py's flags and its refusal to run without trained models,
and the argument checks of score_ids / score_cycles that come before any device work (CPU tensors throughout: any
launch would raise NativeError instead)."""
import pytest
import torch


def test_scoring_flags_parse_with_their_defaults():
    import score_welding_cycles as swc
    a = swc.parser().parse_args([])
    assert (a.n_cycles, a.n_seqs, a.data_npz, a.seed, a.precision, a.out) == (20, 16, "", 0, "fp32", "cycle_scores.npz")
    assert a.vqvae_model.endswith(".ckpt") and a.transformer_model == ""
    b = swc.parser().parse_args(["--n-cycles", "4", "--n-seqs", "3", "--seed", "9", "--precision", "bf16",
                                 "--vqvae-model", "a.ckpt", "--transformer-model", "b.ckpt", "--out", "o.npz",
                                 "--data-npz", "d.npz"])
    assert (b.n_cycles, b.n_seqs, b.seed, b.precision, b.vqvae_model, b.transformer_model, b.out, b.data_npz) == \
        (4, 3, 9, "bf16", "a.ckpt", "b.ckpt", "o.npz", "d.npz")
    with pytest.raises(SystemExit):
        swc.parser().parse_args(["--prompt-cycles", "1"])        # nothing is generated: no such flag


def test_the_refusal_is_the_generation_scripts_own():
    import generate_welding_cycles as gwc
    import score_welding_cycles as swc
    assert swc.require_checkpoint is gwc.require_checkpoint


@pytest.mark.parametrize("missing", ["--vqvae-model", "--transformer-model"])
def test_a_missing_checkpoint_exits_with_a_clear_message(tmp_path, missing):
    import score_welding_cycles as swc
    present = tmp_path / "present.ckpt"
    present.write_bytes(b"")                     # existence is checked before anything is loaded
    paths = {"--vqvae-model": str(present), "--transformer-model": str(present)}
    paths[missing] = str(tmp_path / "absent.ckpt")
    args = swc.parser().parse_args([v for kv in paths.items() for v in kv] + ["--out", str(tmp_path / "o.npz")])
    with pytest.raises(SystemExit) as e:
        swc.main(args)
    assert missing in str(e.value) and "not found" in str(e.value) and "absent.ckpt" in str(e.value)
    assert "needs both trained models" in str(e.value)
    assert not (tmp_path / "o.npz").exists()


def _decoder(**kw):
    from model.transformer_decoder import MyTransformerDecoder
    args = dict(d_model=16, n_classes=6, seq_len=33, n_blocks=1, n_head=2)
    args.update(kw)
    return MyTransformerDecoder(**args)


def _vqvae(**kw):
    from model.vq_vae_patch_embedd import VQVAEPatch
    return VQVAEPatch(hidden_dim=8, input_dim=2, num_embeddings=4, embedding_dim=4, n_resblocks=1, learning_rate=1e-3,
                      batch_norm=False, **kw)                     # S = 16 ids per window of 200 x 2


def test_score_ids_checks_its_ids_before_touching_the_device():
    d = _decoder()
    for bad in (torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, 8), torch.zeros(8, dtype=torch.int64),
                torch.zeros(2, 3, 4, dtype=torch.int64), [[0, 1, 2]]):
        with pytest.raises(ValueError, match="int64 ids of shape"):
            d.score_ids(bad)
    for n in (0, 1, 34):
        with pytest.raises(ValueError, match="seq_len"):
            d.score_ids(torch.zeros(2, n, dtype=torch.int64))
    for v in (0, 7, -1):
        with pytest.raises(ValueError, match="valid_ids"):
            d.score_ids(torch.zeros(2, 8, dtype=torch.int64), valid_ids=v)
    with pytest.raises(ValueError, match="groups"):
        d.score_groups(torch.zeros(2, 8, dtype=torch.int64), 2, 4)        # 8 targets from 8 ids


def test_score_cycles_checks_the_cycles_and_the_fit_before_touching_the_device():
    from arcweld.generate import score_cycles
    v, d = _vqvae(), _decoder()                                           # two cycles of 16 ids + the start token
    x = torch.zeros(2, 400, 2)
    for bad in (x.double(), x[0], x[:, :399], x[:, :0], torch.zeros(2, 600, 2), torch.zeros(2, 400, 3), None):
        with pytest.raises(ValueError, match="score_cycles: x must be"):
            score_cycles(v, d, bad)
    with pytest.raises(ValueError, match=r"n_classes 7.*= 6"):
        score_cycles(v, _decoder(n_classes=7), x)
    with pytest.raises(ValueError, match=r"seq_len 32.*n_cycles\*S \+ 1"):
        score_cycles(v, _decoder(seq_len=32), x)
    with pytest.raises(ValueError, match="seq_len 1,"):
        score_cycles(v, _decoder(seq_len=1), x)


def test_score_cycles_refuses_the_residual_quantiser():
    from arcweld.generate import score_cycles
    try:
        v = _vqvae(use_improved_vq=True)
    except Exception as e:      # noqa: BLE001
        pytest.skip(f"the residual quantizer cannot be constructed on this host: {e!r}")
    with pytest.raises(ValueError, match="use_improved_vq"):
        score_cycles(v, _decoder(), torch.zeros(2, 400, 2))
