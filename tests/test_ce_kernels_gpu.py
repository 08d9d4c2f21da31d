"""aw_ce_fwd / aw_ce_bwd / aw_ce_finalize called directly, against fp64 cross entropy on the same logits.

aw_ce_fwd has five code paths (ce_fwd_rows_kernel<4|8|9|16> for V <= 256, 512, 576, 1024 and ce_fwd_kernel above);
every path runs at its first and last width, with targets on the first and last lane of every 64-column chunk, rows
beyond one pass of the grid (R = 4100 > 4096 waves, so the next-row prefetch runs), and 1e30 in every padding column
and in two rows past R, so that any read outside [R][V] moves the row maximum."""
import math

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

V_PATHS = [(1, 2, 63, 64, 65, 256), (257, 512), (513, 514, 576), (577, 1024), (1025, 1500)]
ALL_V = [v for path in V_PATHS for v in path]
CASES = [(V, R) for V in ALL_V for R in (1, 17, 100)] + [(V, 4100) for V in (70, 514, 1030)]
IGNORES = (-1, -100, 3)
POISON = 1e30
PAD = 6


def _K():
    from arcweld import kernels
    return kernels


def _targets(V, R, ignore, frac, g):
    """First and last lane of every 64-column chunk (clipped to < V) in turn, then random ids; ``frac`` of the rows
    ignored (ignore_index = 3 also ignores the rows whose target happens to be class 3)."""
    edges = sorted({c for k in range(0, V, 64) for c in (k, min(k + 63, V - 1))})
    y = torch.tensor([edges[(r + R) % len(edges)] for r in range(R)], dtype=torch.int64)
    rnd = torch.randint(0, V, (R,), generator=g)
    half = torch.arange(R) >= max(len(edges), R // 2)
    y = torch.where(half, rnd, y)
    if frac >= 1.0:
        y[:] = ignore
    elif frac > 0:
        y[torch.rand(R, generator=g) < frac] = ignore
    elif 0 <= ignore < V:
        y[y == ignore] = (ignore + 1) % V if V > 1 else 0
    return y


def _logits(V, R, y, ignore, hard, g):
    x = 3 * torch.randn(R, V, generator=g)
    if hard:
        x = x + 30 * (torch.randint(0, 2, (R, 1), generator=g) * 2 - 1).float()          # per-row shift of +-30
        low = torch.rand(R, V, generator=g) < 0.1
        x = torch.where(low, x.max(1, keepdim=True).values - 80, x)                        # 80 below the row max
        ninf = torch.rand(R, V, generator=g) < 0.1
        keep_col = torch.where((y != ignore) & (y >= 0), y, torch.zeros_like(y)).clamp(0, V - 1)
        ninf[torch.arange(R), keep_col] = False                                            # never the target / all
        x = torch.where(ninf, torch.full_like(x, float("-inf")), x)
    return x


def _padded(x, ld, fill, dtype=torch.float32):
    """(R + 2, ld) buffer of ``fill`` holding x in [:R, :V]; returns the buffer and its [:R] view."""
    R, V = x.shape
    buf = torch.full((R + 2, ld), fill, device="cuda", dtype=dtype)
    buf[:R, :V] = x.cuda().to(dtype)
    return buf, buf[:R]


def _check(V, R, pad, ignore, frac, hard):
    K = _K()
    g = torch.Generator().manual_seed(V * 7919 + R * 31 + pad + (1 if hard else 0))
    y = _targets(V, R, ignore, frac, g)
    x = _logits(V, R, y, ignore, hard, g)
    assert not torch.isinf(x).all(1).any()
    _, logits = _padded(x, V + pad, POISON)
    yd = y.cuda()
    lse_ref, loss_ref, count_ref, d_ref = kr.ce_ref(x.double().cuda(), yd, ignore)

    loss_sum = torch.zeros(1, device="cuda", dtype=torch.float64)
    count = torch.zeros(1, device="cuda", dtype=torch.float64)
    lse = torch.full((R + 2,), float("nan"), device="cuda")
    K.ce_fwd(logits, V, yd, ignore, loss_sum, count, lse[:R])
    torch.cuda.synchronize()
    assert torch.isnan(lse[R:]).all()
    e_lse = kr.max_err(lse[:R], lse_ref)
    e_loss = abs(loss_sum.item() - loss_ref.item())
    print(f"ce V={V} R={R} pad={pad} hard={hard}: lse err {e_lse:.3e} loss_sum err {e_loss:.3e} of {loss_ref.item():.4g}")
    torch.testing.assert_close(lse[:R].double(), lse_ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(loss_sum[0], loss_ref, rtol=1e-4, atol=1e-4)
    assert count.item() == count_ref.item()

    out = torch.full((1,), 123.0, device="cuda")
    K.ce_finalize(loss_sum, count, out)
    if count_ref.item() > 0:
        torch.testing.assert_close(out[0].double(), loss_ref / count_ref, rtol=1e-4, atol=1e-4)
    else:
        assert math.isnan(out.item())                       # as torch.nn.functional.cross_entropy

    gscale = torch.tensor([0.7], device="cuda")
    for dtype in (torch.float32, torch.bfloat16):
        for dpad in (0, PAD):
            buf, dl = _padded(torch.zeros(R, V), V + dpad, float("nan"), dtype)
            buf[:R] = float("nan")
            K.ce_bwd(logits, V, yd, ignore, lse[:R], count, gscale, dl)
            torch.cuda.synchronize()
            assert torch.isfinite(dl[:, :V]).all()
            assert torch.count_nonzero(dl[:, V:]) == 0 and not torch.isnan(dl[:, V:]).any()
            assert torch.isnan(buf[R:]).all()
            if count_ref.item() == 0:
                assert torch.count_nonzero(dl) == 0
            ref = d_ref * 0.7
            if dtype == torch.float32 and dpad == 0:
                print(f"ce V={V} R={R} pad={pad} hard={hard}: dlogits err {kr.max_err(dl[:, :V], ref):.3e} "
                      f"of {ref.abs().max().item():.3e}")
            kr.close(dl[:, :V], ref, f"dlogits {dtype} ldd=V+{dpad}",
                     extra_rel=kr.BF16_REL if dtype == torch.bfloat16 else 0.0)

    # a second call accumulates into the same loss_sum / count (the groups of one fused step)
    lse2 = torch.empty(R, device="cuda")
    K.ce_fwd(logits, V, yd, ignore, loss_sum, count, lse2)
    torch.cuda.synchronize()
    assert torch.equal(lse2, lse[:R])
    torch.testing.assert_close(loss_sum[0], 2 * loss_ref, rtol=1e-4, atol=1e-4)
    assert count.item() == 2 * count_ref.item()


@pytest.mark.parametrize("hard", [False, True], ids=["randn", "shifted"])
@pytest.mark.parametrize("pad", [0, PAD], ids=["ldl=V", "ldl=V+6"])
@pytest.mark.parametrize("V,R", CASES)
def test_ce_forward_backward(V, R, pad, hard):
    _check(V, R, pad, IGNORES[(V + R) % 3], 0.3, hard)


@pytest.mark.parametrize("V", [64, 514, 1030])
def test_ce_no_row_ignored(V):
    _check(V, 100, PAD, -100, 0.0, False)


@pytest.mark.parametrize("V", [64, 514, 1030])
@pytest.mark.parametrize("ignore", IGNORES)
def test_ce_all_rows_ignored(V, ignore):
    """count == 0: the loss is NaN as in torch, dlogits exactly 0."""
    _check(V, 100, PAD, ignore, 1.0, True)
