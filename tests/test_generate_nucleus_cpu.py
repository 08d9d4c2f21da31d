"""The nucleus / min-p / log-probability surface of generation without a GPU: the entry script's new flags, the range
checks of ``generate_ids`` that come before any device work, and the binding of aw_sample_args."""
import pytest
import torch


def test_the_new_generation_flags_parse_with_their_defaults():
    import generate_welding_cycles as gwc
    a = gwc.parser().parse_args([])
    assert (a.top_p, a.min_p, a.logp) == (None, None, False)
    b = gwc.parser().parse_args(["--top-p", "0.9", "--min-p", "0.05", "--logp", "--do-sample"])
    assert (b.top_p, b.min_p, b.logp, b.do_sample) == (0.9, 0.05, True, True)
    assert gwc.parser().parse_args(["--logp", "--no-logp"]).logp is False


def _decoder():
    from model.transformer_decoder import MyTransformerDecoder
    return MyTransformerDecoder(d_model=16, n_classes=6, seq_len=33, n_blocks=1, n_head=2)


@pytest.mark.parametrize("kw", [dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.2), dict(top_p=float("nan")),
                                dict(min_p=1.0), dict(min_p=-0.1), dict(min_p=float("nan")),
                                dict(top_p=0.9, min_p=1.5, return_logp=True)])
def test_generate_ids_checks_top_p_and_min_p_before_touching_the_device(kw):
    d = _decoder()
    x = torch.zeros(2, 8, dtype=torch.int64)          # CPU ids: any device work would raise NativeError instead
    with pytest.raises(ValueError, match="min_p" if "min_p" in kw else "top_p"):
        d.generate_ids(x, 4, do_sample=True, **kw)


def test_the_argument_struct_matches_the_header():
    """aw_sample_args field for field: names and order as the header declares them, pointer / int / float widths."""
    import ctypes
    import re

    from arcweld import _native
    src = open(_native.HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} aw_sample_args;", src).group(1)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == [f[0] for f in _native.SampleArgs._fields_]
    kinds = dict(_native.SampleArgs._fields_)
    assert kinds["top_p"] is ctypes.c_float and kinds["seed"] is ctypes.c_uint64 and kinds["step"] is ctypes.c_int64
    assert kinds["ld_lp"] is ctypes.c_int64 and kinds["n_valid"] is ctypes.c_int
    assert kinds["logp_out"] is ctypes.c_void_p
    assert "aw_sample_next_ex" in _native.SIGNATURES
