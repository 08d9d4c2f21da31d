"""The beam-search surface without a GPU: the entry script's flags, the argument checks of ``beam_search_ids`` and
``continue_cycles`` that come before any device work, and the binding of aw_beam_args."""
import pytest
import torch


def test_the_beam_flags_parse_with_their_defaults():
    import generate_welding_cycles as gwc
    a = gwc.parser().parse_args([])
    assert (a.num_beams, a.num_return) == (None, 1)
    b = gwc.parser().parse_args(["--num-beams", "8", "--num-return", "3"])
    assert (b.num_beams, b.num_return) == (8, 3)


def _decoder(n_classes=6):
    from model.transformer_decoder import MyTransformerDecoder
    return MyTransformerDecoder(d_model=16, n_classes=n_classes, seq_len=33, n_blocks=1, n_head=2)


@pytest.mark.parametrize("kw, match", [
    (dict(num_beams=0), "num_beams"), (dict(num_beams=33), "num_beams"), (dict(num_beams=-1), "num_beams"),
    (dict(num_beams=4, num_return=0), "num_return"), (dict(num_beams=4, num_return=5), "num_return"),
    (dict(num_beams=4, n_new=26), "seq_len"), (dict(num_beams=4, n_new=-1), "seq_len"),
    (dict(num_beams=4, valid_ids=0), "valid_ids"), (dict(num_beams=4, valid_ids=7), "valid_ids"),
])
def test_beam_search_ids_checks_its_arguments_before_touching_the_device(kw, match):
    d = _decoder()
    x = torch.zeros(2, 8, dtype=torch.int64)          # CPU ids: any device work would raise NativeError instead
    kw = dict(kw)
    n_new = kw.pop("n_new", 4)
    with pytest.raises(ValueError, match=match):
        d.beam_search_ids(x, n_new, **kw)


def test_beam_search_ids_refuses_more_candidates_than_a_workgroup_ranks():
    d = _decoder(n_classes=1026)                      # 32 * 1024 > 16384 >= 16 * 1024
    x = torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="16384"):
        d.beam_search_ids(x, 4, 32, valid_ids=1024)
    with pytest.raises(ValueError, match="16384"):
        d.beam_search_ids(x, 4, 17, valid_ids=1024)
    with pytest.raises(ValueError, match="int64"):
        d.beam_search_ids(x.float(), 4, 4)


@pytest.mark.parametrize("kw", [dict(do_sample=True), dict(top_k=3), dict(top_p=0.9), dict(min_p=0.1),
                                dict(temperature=0.8), dict(do_sample=True, top_p=0.9, temperature=2.0)])
def test_continue_cycles_refuses_beam_search_with_the_sampling_arguments(kw):
    from arcweld.generate import continue_cycles
    with pytest.raises(ValueError, match="num_beams"):       # before the models are looked at
        continue_cycles(None, None, torch.zeros(1, 200, 2), 2, num_beams=4, **kw)


def test_the_argument_struct_matches_the_header():
    """aw_beam_args field for field: names and order as the header declares them, pointer / int widths."""
    import ctypes
    import re

    from arcweld import _native
    src = open(_native.HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} aw_beam_args;", src).group(1)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == [f[0] for f in _native.BeamArgs._fields_]
    kinds = dict(_native.BeamArgs._fields_)
    assert kinds["ldl"] is ctypes.c_int64 and kinds["logits"] is ctypes.c_void_p
    assert all(kinds[k] is ctypes.c_int for k in ("B", "W_in", "W_out", "V", "n_valid"))
    assert all(kinds[k] is ctypes.c_void_p for k in ("scores_in", "scores_out", "parent_out", "token_out", "logp_out",
                                                     "bad_count"))
    assert int(re.search(r"#define AW_BEAM_MAX_W (\d+)", src).group(1)) == _native.BEAM_MAX_W
    for name in ("aw_beam_step", "aw_beam_gather", "aw_beam_backtrack"):
        assert name in _native.SIGNATURES
