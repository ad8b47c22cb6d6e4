"""Checkpoints of the Adagrad / RMSprop / MagSGD optimizers: the libtorch archives <NAME>_OPTIM.lt (rlgpu_optim_lt
--optimizer), RLGPU_OPTIM.safetensors' <NAME>.optim_type, and a Learner that resumes on the same bytes."""
import json
import os
import warnings

import numpy as np
import pytest

from rlgpu import checkpoint as ckpt
from rlgpu.ppo import make_sequential

ARCH = dict(obs=12, out=5, layers=(8, 6))


def _seq():
    return make_sequential(ARCH["obs"], ARCH["out"], ARCH["layers"], True)


def _tool():
    if not os.path.exists(ckpt.OPTIM_TOOL):
        pytest.skip("rlgpu_optim_lt not built")


@pytest.mark.parametrize("kind", ["adagrad", "rmsprop", "magsgd"])
def test_optimizer_archive_round_trip(tmp_path, kind):
    """write_optim_archive / read_optim_archive with each new type, through the matching libtorch class: Adagrad's sum
    and RMSprop's square_avg (the exp_avg_sq span) and the step come back bit for bit with exp_avg zero; MagSGD's file
    (an SGD without state) is written, loads, and reads as step 0 and zeros."""
    _tool()
    shapes = [tuple(p.shape) for p in _seq().parameters()]
    n = sum(int(np.prod(s)) for s in shapes)
    rng = np.random.default_rng(3)
    m, v = np.zeros(n, np.float32), rng.random(n).astype(np.float32)
    p = str(tmp_path / "POLICY_OPTIM.lt")
    ckpt.write_optim_archive(p, shapes, 17, 3e-4, (0.9, 0.999), 1e-8, 1e-2, m, v, optimizer=kind)
    assert os.path.getsize(p) > 0
    step, m2, v2 = ckpt.read_optim_archive(p, shapes, optimizer=kind)
    assert m2.shape == v2.shape == (n,) and not m2.any()
    if kind == "magsgd":
        assert step == 0 and not v2.any()
    else:
        assert step == 17
        np.testing.assert_array_equal(v2.view(np.uint32), v.view(np.uint32))
    with pytest.raises(ValueError, match="optimizer must be one of"):
        ckpt.write_optim_archive(p, shapes, 1, 3e-4, (0.9, 0.999), 1e-8, 1e-2, m, v, optimizer="sgd")


class _PPO:
    """test_checkpoint.py's stub: one model on the host, with the options dict checkpoint.save reads."""
    models = (0,)

    def __init__(self, seq, optimizer=None):
        import torch
        self.seq = seq
        self.n = sum(p.numel() for p in seq.parameters())
        self.params = torch.cat([p.detach().reshape(-1) for p in seq.parameters()]).clone()
        self.m, self.v, self.step = torch.zeros(self.n), torch.zeros(self.n), 0
        self.optim_options = {"lr": (1e-3,) * 3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 1e-2}
        if optimizer is not None:
            self.optim_options["optimizer"] = (optimizer,) * 3

    def torch_module(self, mi):
        return self.seq

    def model_sizes(self, mi):
        return [p.numel() for p in self.seq.parameters()]

    def model_range(self, mi):
        return 0, self.n

    def refresh_half(self):
        pass

    def optimizer_state(self):
        return self.step, self.m, self.v

    def set_optimizer_step(self, step):
        self.step = step

    def model_optimizer_step(self, mi):
        return self.step

    def set_model_optimizer_step(self, mi, step):
        self.step = step


class _Stat:
    def to_json(self):
        return {"mean": 0.0, "var": 1.0, "count": 0}

    def read_json(self, j):
        pass


class _Learner:
    total_steps, iteration = 100, 1

    def __init__(self, ppo):
        self.ppo = ppo
        self.return_stat = _Stat()


def test_safetensors_records_the_type_and_mismatch_resets(tmp_path):
    """checkpoint.save writes <NAME>.optim_type; a file without the key loads as AdamW with no warning (an old
    checkpoint); a stored type the handle's optimizer cannot use warns by name and zeroes that model's state and step;
    Adam and AdamW read each other's state."""
    _tool()
    import torch
    from safetensors.torch import load_file, save_file
    seq = _seq()
    src = _PPO(seq, "rmsprop")
    src.v.uniform_()
    src.step = 9
    path = ckpt.save(_Learner(src), str(tmp_path / "a"))
    t = load_file(os.path.join(path, ckpt.OPTIM_FILE))
    assert int(t["policy.optim_type"][0]) == ckpt.OPTIMIZERS["rmsprop"] == 3
    step, m2, v2 = ckpt.read_optim_archive(os.path.join(path, "POLICY_OPTIM.lt"), [tuple(p.shape) for p in seq.parameters()],
                                           optimizer="rmsprop")
    assert step == 9 and np.array_equal(v2, src.v.numpy())
    # the same type: loads, silently
    dst = _PPO(seq, "rmsprop")
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)
        ckpt.load(_Learner(dst), str(tmp_path / "a"))
    assert dst.step == 9 and torch.equal(dst.v, src.v)
    # another type: warned by name, reset
    dst = _PPO(seq, "adagrad")
    dst.m.fill_(1.0)
    dst.v.fill_(1.0)
    with pytest.warns(UserWarning, match='model "policy".*rmsprop.*adagrad.*optimizer will be reset'):
        ckpt.load(_Learner(dst), str(tmp_path / "a"))
    assert dst.step == 0 and not dst.m.any() and not dst.v.any()
    # a file without the key (an old checkpoint): AdamW state, for AdamW and Adam alike, with no warning
    old = {k: x for k, x in t.items() if not k.endswith(".optim_type")}
    old["policy.exp_avg"] = torch.full((src.n,), 0.5)
    os.makedirs(tmp_path / "b" / "100")
    save_file(old, str(tmp_path / "b" / "100" / ckpt.OPTIM_FILE))
    for f in ("POLICY.lt", ckpt.STATS_FILE):
        with open(os.path.join(path, f), "rb") as fi, open(tmp_path / "b" / "100" / f, "wb") as fo:
            fo.write(fi.read())
    for kind in (None, "adamw", "adam"):
        dst = _PPO(seq, kind)
        with warnings.catch_warnings():
            warnings.simplefilter("error", UserWarning)
            ckpt.load(_Learner(dst), str(tmp_path / "b"))
        assert dst.step == 9 and torch.equal(dst.v, src.v) and float(dst.m.min()) == 0.5
    dst = _PPO(seq, "magsgd")
    with pytest.warns(UserWarning, match="adamw.*magsgd.*optimizer will be reset"):
        ckpt.load(_Learner(dst), str(tmp_path / "b"))
    assert dst.step == 0 and not dst.m.any() and not dst.v.any()
    assert json.load(open(os.path.join(path, ckpt.STATS_FILE)))["total_timesteps"] == 100


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rmsprop", "magsgd"])
def test_learner_resumes_byte_identical(gpu, tmp_path, kind):
    """A Learner (4 arenas, rollout 8, layers [64]) with the optimizer: one iteration, save, one more iteration gives
    parameters A.  A fresh Learner loads the checkpoint -- parameters, optimizer state and type, counters -- and is
    handed what a checkpoint does not hold and the first Learner had at the save (the arenas, the rollout's row 0 and
    the sampling counter: a fresh Learner would otherwise start at the kickoff); its one iteration gives A', byte for
    byte A.  Everything is finite and moved from the initial values."""
    import torch
    from safetensors.torch import load_file
    from rlgpu.learner import Learner, LearnerConfig
    folder = str(tmp_path / "ck")
    cfg = dict(num_arenas=4, rollout_len=8, mini_batch_size=128, seed=5, policy_layers=(64,), critic_layers=(64,),
               optimizer=kind, checkpoint_folder=folder, ts_per_save=10 ** 12, train_against_old_versions=False)
    L = Learner(LearnerConfig(**cfg), device=gpu)
    assert L.ppo.get_optimizer(0) == L.ppo.get_optimizer(1) == kind
    init = L.ppo.flat().clone()
    L.iterate()
    path = L.save()
    torch.cuda.synchronize()
    t = load_file(os.path.join(path, ckpt.OPTIM_FILE))
    assert [int(t[n + ".optim_type"][0]) for n in ("policy", "critic")] == [ckpt.OPTIMIZERS[kind]] * 2
    assert os.path.getsize(os.path.join(path, "POLICY_OPTIM.lt")) > 0
    saved = [x.clone() for x in (L.ppo.params, *L.ppo.optimizer_state()[1:])]
    saved_step = L.ppo.optimizer_state()[0]
    hidden = (L.env.get_arenas(), L._stats().rng_step, L.obs[0].clone(), L.masks[0].clone())
    L.iterate()
    A = L.ppo.flat().clone()
    L2 = Learner(LearnerConfig(**cfg), device=gpu)
    assert L2.last_checkpoint is not None and L2.iteration == 1
    step2, m2, v2 = L2.ppo.optimizer_state()
    assert step2 == saved_step > 0
    for a, b in zip(saved, (L2.ppo.params, m2, v2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if kind == "rmsprop":
        assert bool(v2.any()) and not bool(m2.any())
    else:
        assert not bool(v2.any()) and not bool(m2.any())
    L2.env.set_arenas(hidden[0])
    L2._set_stat("rng_step", hidden[1])
    L2.obs[0].copy_(hidden[2])
    L2.masks[0].copy_(hidden[3])
    L2.iterate()
    A2 = L2.ppo.flat()
    assert torch.isfinite(A).all() and torch.isfinite(A2).all()
    assert torch.equal(A.view(torch.int32), A2.view(torch.int32)), float((A - A2).abs().max())
    assert float((A != init).float().mean()) > 0.5 and float((saved[0] != L.ppo.params).float().mean()) > 0.5
    L.close()
    L2.close()
