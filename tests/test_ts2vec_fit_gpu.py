"""``model.ts2vec.TS2Vec.fit`` on the device: a seeded three-iteration trajectory against a replay on the CPU
restatement (tests/ts2vec_loss_refs.py: the same seeds, the same order of draws), and the bookkeeping of the
reference's training loop.

The tolerance is the rule of tests/test_ts2vec_gpu.py: e_ref = |replay_f32 - replay_f64| is the reference arithmetic's
own rounding over the trajectory; the device run stays within 4 e_ref of the f64 replay (one f32 ulp more for a loss,
which is itself rounded to f32).
"""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import ts2vec_loss_refs as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, ITERS, BATCH, LR = 1234, 3, 4, 1e-3


def _data(n=8, T=24, C=2, seed=81):
    return np.random.RandomState(seed).randn(n, T, C).astype(np.float64)


def _replay(sd0, data, dtype):
    """The reference's loop restated: shuffled batches from torch's generator; per iteration crop_l, crop_left,
    crop_eleft, crop_eright and the row offsets from np.random, then view 1's binomial mask, then view 2's; AdamW;
    the running mean of the weights."""
    p = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in sd0.items()}
    avg = {k: v.detach().clone() for k, v in p.items()}
    opt = torch.optim.AdamW(list(p.values()), lr=LR)
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    loader = DataLoader(TensorDataset(torch.from_numpy(data).to(torch.float)), batch_size=BATCH, shuffle=True,
                        drop_last=True)
    losses, n_avg = [], 1
    while len(losses) < ITERS:
        for (x,) in loader:
            if len(losses) >= ITERS:
                break
            ts_l, B = x.shape[1], x.shape[0]
            crop_l = np.random.randint(low=2, high=ts_l + 1)
            left = np.random.randint(ts_l - crop_l + 1)
            right = left + crop_l
            eleft = np.random.randint(left + 1)
            eright = np.random.randint(low=right, high=ts_l + 1)
            off = np.random.randint(low=-eleft, high=ts_l - eright + 1, size=B)
            views = []
            for start, length in ((off + eleft, right - eleft), (off + left, eright - left)):
                v = torch.stack([x[i, s:s + length] for i, s in enumerate(start)])
                keep = np.random.binomial(1, 0.5, size=(B, length)).astype(bool)
                views.append(L.encoder_forward(p, v, keep))
            loss = L.hierarchical(views[0][:, -crop_l:], views[1][:, :crop_l], 0.5, 0)
            opt.zero_grad()
            loss.backward()
            opt.step()
            with torch.no_grad():
                for k in p:
                    avg[k] += (p[k] - avg[k]) / (n_avg + 1)
            n_avg += 1
            losses.append(float(loss.detach()))
    return losses, {k: v.detach() for k, v in p.items()}, avg


def _model(**kw):
    from model.ts2vec import TS2Vec
    torch.manual_seed(7)
    args = dict(output_dims=16, hidden_dims=16, depth=2, device=DEV, lr=LR, batch_size=BATCH)
    args.update(kw)
    return TS2Vec(2, **args)


def test_three_iterations_follow_the_replay():
    data = _data()
    m = _model()
    m.net.repr_dropout.p = 0.0
    sd0 = {k: v.clone() for k, v in m.net.state_dict().items()}
    seen = []
    m.after_iter_callback = lambda model, loss: seen.append(loss)
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    log = m.fit(data, n_iters=ITERS)
    l64, p64, a64 = _replay(sd0, data, torch.float64)
    l32, p32, a32 = _replay(sd0, data, torch.float32)
    assert len(seen) == ITERS and m.n_iters == ITERS and m.n_averaged == 1 + ITERS and m.n_epochs == 1
    worst = 0.0
    for i in range(ITERS):
        err, e_ref = abs(seen[i] - l64[i]), abs(l32[i] - l64[i])
        ulp = float(np.spacing(np.float32(abs(l64[i]))))
        print(f"iteration {i}: loss {seen[i]:.7f} replay {l64[i]:.7f} err {err:.3e} e_ref {e_ref:.3e}")
        assert err <= 4 * e_ref + ulp, (i, err, e_ref)
    assert len(log) == 1                                                 # 2 iterations per epoch: one epoch completed
    e_log = abs(np.mean(l32[:2]) - np.mean(l64[:2]))
    assert abs(log[0] - np.mean(l64[:2])) <= 4 * e_log + float(np.spacing(np.float32(log[0])))
    for which, net, r64, r32 in (("_net", m._net, p64, p32), ("net", m.net, a64, a32)):
        for name, v in net.state_dict().items():
            err = float((v.cpu().double() - r64[name]).abs().max())
            e_ref = float((r32[name].double() - r64[name]).abs().max())
            worst = max(worst, err / e_ref if e_ref else 0.0)
            print(f"{which}.{name}: err {err:.3e} e_ref {e_ref:.3e} ratio {err / e_ref if e_ref else 0:.2f}")
            assert err <= 4 * e_ref, (which, name, err, e_ref)
    print(f"worst parameter ratio {worst:.2f}")


def test_bookkeeping_with_dropout_on(tmp_path):
    data = _data(n=9)
    epochs = []
    m = _model(after_epoch_callback=lambda model, loss: epochs.append(loss))
    assert m._net is m.net
    torch.manual_seed(1)
    np.random.seed(1)
    log = m.fit(data, n_epochs=2)                                        # 9 series, batch 4, drop_last: 2 per epoch
    assert len(log) == 2 == len(epochs) and m.n_epochs == 2 and m.n_iters == 4 and m.n_averaged == 5
    assert all(np.isfinite(v) and v > 0 for v in log)
    assert m._net is not m.net and m._net.training and not m.net.training
    assert any(not torch.equal(a, b) for a, b in zip(m.net.parameters(), m._net.parameters()))
    log = m.fit(data, n_iters=5)                                         # stops in the middle of the third epoch
    assert log == [] and m.n_iters == 5 and m.n_epochs == 2 and m.n_averaged == 6
    rep = m.encode(data.astype(np.float32), encoding_window="full_series")
    assert rep.shape == (9, 16) and np.isfinite(rep).all()
    path = tmp_path / "model.pt"
    m.save(str(path))
    sd = torch.load(str(path), map_location="cpu")
    assert set(sd) == {"n_averaged"} | {"module." + k for k in m.net.state_dict()} and int(sd["n_averaged"]) == 6
    fresh = _model()
    fresh.load(str(path))
    assert fresh.n_averaged == 6 and fresh._net is fresh.net
    assert np.array_equal(fresh.encode(data.astype(np.float32)), m.encode(data.astype(np.float32)))


def test_defaults_and_a_batch_larger_than_the_data():
    m = _model(batch_size=16)
    torch.manual_seed(2)
    np.random.seed(2)
    log = m.fit(_data(n=3, T=12), n_epochs=1)                            # the batch shrinks to the 3 series
    assert len(log) == 1 and m.n_iters == 1


def test_max_train_length_with_nan_padded_series():
    data = _data(n=3, T=50)
    data[0, 40:] = np.nan                                                # a short series: NaN at the end
    data[1, 25:] = np.nan                                                # its second section is all NaN: dropped
    data[2, 7, 0] = np.nan                                               # a single missing sample
    m = _model(max_train_length=20, temporal_unit=1)
    torch.manual_seed(3)
    np.random.seed(3)
    log = m.fit(data, n_epochs=2)                                        # sections of 25 -> windows of 20
    assert len(log) == 2 and all(np.isfinite(v) for v in log) and m.n_iters == 2
    assert all(torch.isfinite(p).all() for p in m.net.parameters())
