"""bench.py's command line (CPU): a plain run asks for nothing beside the headline figure, --full switches the rest
on, and --dump-outputs writes float32 arrays whose sampled elements are the same in every run."""
import os
import sys

import numpy as np
import torch

import bench


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_not_full(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup, a.only) == (False, None, 7, 2, "all")
    a = _args(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_float32_capped_and_repeatable(tmp_path, monkeypatch):
    torch.manual_seed(0)
    m = torch.nn.Linear(300, 200)
    flat = np.concatenate([m.weight.detach().numpy().reshape(-1), m.bias.detach().numpy()])
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 4 * 100000)     # 2 arrays of at most 100000 elements: all of it
    bench.dump_outputs(str(tmp_path / "whole"), m, torch.tensor(1.5))
    assert sorted(os.listdir(tmp_path / "whole")) == ["loss.npy", "params.npy"]
    assert np.array_equal(np.load(tmp_path / "whole" / "loss.npy"), np.array([1.5], np.float32))
    assert np.array_equal(np.load(tmp_path / "whole" / "params.npy"), flat)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 4 * 1000)       # at most 1000 elements each: a sample
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), m, torch.tensor(1.5))
    total = 0
    for n in ("loss.npy", "params.npy"):
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b)
        total += a.nbytes
    assert total <= bench.DUMP_MAX_BYTES
    p = np.load(tmp_path / "a" / "params.npy")
    assert p.shape == (1000,)
    j = 0                                  # the sample keeps the order of the flat array
    for v in p:
        while flat[j] != v:
            j += 1
        j += 1


def test_reset_training_state_restores_what_setup_left():
    class Set:
        forced = 0

        def refresh(self, force=False):
            self.forced += int(force)

    class Opt:
        pass

    opt, m, st = Opt(), torch.nn.Linear(2, 2), Set()
    p0 = torch.arange(6.0)
    opt._flat = {"p": p0 + 3, "m": torch.ones(6), "v": torch.ones(6), "step": torch.tensor([9])}
    opt._step_count = 9
    m._rng_counter = torch.tensor([9])
    m.__dict__["_operand_sets"] = {"k": st}
    p_buf = opt._flat["p"]
    bench.reset_training_state(m, opt, p0)
    assert opt._flat["p"] is p_buf and torch.equal(p_buf, p0)         # restored in place: captured graphs read it
    assert not opt._flat["m"].any() and not opt._flat["v"].any() and int(opt._flat["step"]) == 0
    assert opt._step_count == 0 and int(m._rng_counter) == 0 and st.forced == 1
