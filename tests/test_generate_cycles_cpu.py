"""The generation surface without a GPU: the entry script's flags and its refusal to run without trained models, and
the argument checks of the ids -> signals path that come before any device work."""
import pytest
import torch


def test_generation_flags_parse_with_their_defaults():
    import generate_welding_cycles as gwc
    a = gwc.parser().parse_args([])
    assert (a.n_cycles, a.prompt_cycles, a.n_seqs, a.data_npz, a.do_sample, a.top_k, a.temperature, a.seed,
            a.precision, a.out) == (20, 10, 16, "", False, None, 1.0, 0, "fp32", "generated_cycles.npz")
    assert a.vqvae_model.endswith(".ckpt") and a.transformer_model == ""
    b = gwc.parser().parse_args(["--do-sample", "--top-k", "5", "--temperature", "0.8", "--n-cycles", "4",
                                 "--prompt-cycles", "1", "--n-seqs", "3", "--seed", "9", "--precision", "bf16",
                                 "--vqvae-model", "a.ckpt", "--transformer-model", "b.ckpt", "--out", "o.npz",
                                 "--data-npz", "d.npz"])
    assert (b.do_sample, b.top_k, b.temperature, b.n_cycles, b.prompt_cycles, b.n_seqs, b.seed, b.precision,
            b.vqvae_model, b.transformer_model, b.out, b.data_npz) == \
        (True, 5, 0.8, 4, 1, 3, 9, "bf16", "a.ckpt", "b.ckpt", "o.npz", "d.npz")


@pytest.mark.parametrize("missing", ["--vqvae-model", "--transformer-model"])
def test_a_missing_checkpoint_exits_with_a_clear_message(tmp_path, missing):
    import generate_welding_cycles as gwc
    present = tmp_path / "present.ckpt"
    present.write_bytes(b"")                     # existence is checked before anything is loaded
    paths = {"--vqvae-model": str(present), "--transformer-model": str(present)}
    paths[missing] = str(tmp_path / "absent.ckpt")
    args = gwc.parser().parse_args([v for kv in paths.items() for v in kv] + ["--out", str(tmp_path / "o.npz")])
    with pytest.raises(SystemExit) as e:
        gwc.main(args)
    assert missing in str(e.value) and "not found" in str(e.value) and "absent.ckpt" in str(e.value)
    assert not (tmp_path / "o.npz").exists()


def _tiny(**kw):
    from model.vq_vae_patch_embedd import VQVAEPatch
    return VQVAEPatch(hidden_dim=8, input_dim=2, num_embeddings=4, embedding_dim=4, n_resblocks=1, learning_rate=1e-3,
                      batch_norm=False, **kw)


def test_tokenize_decode_ids_rejects_a_ragged_length_before_touching_the_device():
    from arcweld import tokenize
    m = _tiny()                                  # S = 16; CPU tensors: any device work would raise NativeError
    for n in (15, 17, 33):
        with pytest.raises(ValueError, match="not a multiple of the 16 ids per window"):
            tokenize.decode_ids(m, torch.zeros(2, n, dtype=torch.int64))
    with pytest.raises(ValueError):
        tokenize.decode_ids(m, torch.zeros(16, dtype=torch.int64))


def test_improved_vq_has_no_way_back_from_ids():
    try:
        m = _tiny(use_improved_vq=True)
    except Exception as e:      # noqa: BLE001
        pytest.skip(f"the residual quantizer cannot be constructed on this host: {e!r}")
    with pytest.raises(NotImplementedError, match="use_improved_vq"):
        m.decode_ids(torch.zeros(1, 16, dtype=torch.int64))
    from arcweld import vqvae as engine
    with pytest.raises(NotImplementedError, match="use_improved_vq"):
        engine.decode(m, torch.zeros(16, dtype=torch.int64))
