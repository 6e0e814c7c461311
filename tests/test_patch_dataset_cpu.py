"""CPU: the host side of patch supply against the reference's recorded runs (G21, tests/golden/gen_golden_patch_dataset.py):
the samplers' decisions, TensorDataset's sampler loop, the speculation / replay logic of the device loader fed with numpy
criteria, and the pickle contract.  Every comparison is on integers or recorded values: bit for bit."""
import pickle

import numpy as np
import pytest
import torch

from patch_dataset_kit import crop, fixture, numpy_judge, numpy_stat, runs_of, sampler_of, volumes_of

SEED = 2024
WITH_SAMPLER = [n for n, c in fixture()["configs"].items() if c["sampler"] is not None and n != "never"]


class _Coins:
    """np.random.rand that deals the recorded coins, in order"""

    def __init__(self, coins):
        self.coins, self.used = list(coins), 0

    def __call__(self):
        self.used += 1
        return self.coins[self.used - 1]


@pytest.mark.parametrize("name", WITH_SAMPLER)
def test_host_sampler_decisions_equal_the_reference(name, monkeypatch):
    """every recorded attempt but a sample's last is rejected, the last accepted, and exactly the recorded coins are drawn"""
    cfg = fixture()["configs"][name]
    sampler = sampler_of(cfg)
    _, _, _, raw, labels = volumes_of(cfg)
    assert max(len(r[0]) for r in runs_of(name)) <= 501
    for starts, coins, _, _ in runs_of(name):
        deal = _Coins(coins)
        monkeypatch.setattr(np.random, "rand", deal)
        decisions = [bool(sampler(*crop(raw, labels, st, cfg["patch"], cfg.get("with_channels", False)))) for st in starts]
        assert decisions == [False] * (len(starts) - 1) + [True]
        assert deal.used == len(coins)


@pytest.mark.parametrize("name", WITH_SAMPLER)
def test_device_criterion_agrees_with_the_host_sampler(name):
    """the record a sampler hands the device path, judged on numpy statistics, decides every recorded attempt as the sampler
    itself does (criterion only: an attempt that drew a coin had failed it)"""
    cfg = fixture()["configs"][name]
    crit = sampler_of(cfg).device_criterion()
    _, _, _, raw, labels = volumes_of(cfg)
    for starts, coins, _, _ in runs_of(name):
        met = []
        for st in starts:
            r, l = crop(raw, labels, st, cfg["patch"], cfg.get("with_channels", False))
            met.append(crit.met(numpy_stat(crit, r, l), l.size))
        assert met[:-1] == [False] * (len(starts) - 1) and met[-1] == (len(coins) < len(starts))


def test_samplers_the_device_cannot_judge_say_so():
    from torch_em_amd.data import MinIntensitySampler, MinNoToBackgroundBoundarySampler
    from torch_em_amd.data.sampler import device_criterion

    class Trafo:
        bg_label, mask_label = 0, -1

        def __call__(self, y):
            return y.copy()
    for sampler in (MinIntensitySampler(1, "mean"), MinIntensitySampler(1, "std"), MinIntensitySampler(1, lambda x: x.sum()),
                    MinNoToBackgroundBoundarySampler(Trafo()), lambda x, y: True):
        with pytest.raises(NotImplementedError, match="TensorDataset"):
            device_criterion(sampler)
    assert device_criterion(None) is None
    y = np.zeros((4, 4), np.int32)
    y[0, 0] = 3
    assert MinNoToBackgroundBoundarySampler(Trafo(), min_fraction=0.05)(None, y) is True


@pytest.mark.parametrize("name", ["fg_int", "inst", "median", "sem_per_id", "two"])
def test_tensor_dataset_honours_its_sampler(name):
    """volume `a` needs no padding, so TensorDataset's loop under sample s's stream returns the reference's crop; the crop it
    returns is one the criterion accepts or a coin let through, never a rejected one"""
    from torch_em_amd.data import TensorDataset
    cfg = fixture()["configs"][name]
    raw, labels, _, _, _ = volumes_of(cfg)
    seen = []

    class Spy:
        def __init__(self, inner):
            self.inner = inner

        def __call__(self, x, y):
            seen.append(bool(self.inner(x, y)))
            return seen[-1]
    ds = TensorDataset([raw], [labels], patch_shape=tuple(cfg["patch"]), sampler=Spy(sampler_of(cfg)), label_dtype=torch.int64)
    for s, (starts, _, want_raw, want_labels) in enumerate(runs_of(name)):
        del seen[:]
        np.random.set_state(np.random.RandomState([SEED, s]).get_state())
        x, y = ds[0]
        assert seen == [False] * (len(starts) - 1) + [True]
        assert np.array_equal(x[0].numpy(), want_raw.astype(np.float32)) and np.array_equal(y[0].numpy(), want_labels)


def test_tensor_dataset_gives_up_after_500_attempts():
    from torch_em_amd.data import TensorDataset
    cfg = fixture()["configs"]["never"]
    assert int(fixture()["never/raises"]) == 1
    raw, labels, _, _, _ = volumes_of(cfg)
    calls = []
    inner = sampler_of(cfg)

    def sampler(x, y):
        calls.append(1)
        return inner(x, y)
    ds = TensorDataset([raw], [labels], patch_shape=tuple(cfg["patch"]), sampler=sampler)
    np.random.seed(0)
    with pytest.raises(RuntimeError, match="Could not sample a valid batch in 500 attempts"):
        ds[0]
    assert len(calls) == 501   # the first draw and 500 re-draws are judged; the 501st re-draw raises


def test_tensor_dataset_without_sampler_is_unchanged():
    """values and np.random consumption of the sampler-less path equal the run recorded before the sampler loop existed"""
    import importlib.util
    import os

    from conftest import GOLDEN
    from torch_em_amd.data import TensorDataset
    spec = importlib.util.spec_from_file_location("gen_golden_patch_dataset", os.path.join(GOLDEN, "gen_golden_patch_dataset.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    state = np.random.get_state()
    try:
        x, y, nxt = gen.run_tensor_dataset(TensorDataset)
    finally:
        np.random.set_state(state)
    fx = fixture()
    assert x.dtype == fx["tds/raw"].dtype and np.array_equal(x, fx["tds/raw"]) and np.array_equal(y, fx["tds/labels"])
    assert int(nxt) == int(fx["tds/next"])


@pytest.mark.parametrize("per_round", [1, 3, 8])
def test_speculation_reproduces_the_reference_sequences(per_round):
    """the loader's replay logic with criteria computed in numpy: the boxes tried, the coins consumed and the accepted box of
    every stored sample, for every stored configuration, whatever the number of candidates per round"""
    from torch_em_amd.data.device_dataset import Candidate, sample_state, speculate
    for name, cfg in fixture()["configs"].items():
        _, _, _, raw, labels = volumes_of(cfg)
        spans = [sh - p for sh, p in zip(labels.shape, cfg["patch"])]
        sampler = sampler_of(cfg)
        judge = None if sampler is None else numpy_judge(cfg)
        p_reject = None if sampler is None else sampler.p_reject
        if name == "never":
            with pytest.raises(RuntimeError, match="Could not sample a valid batch in 500 attempts"):
                speculate([Candidate(sample_state(SEED, 0), 0, spans)], judge, p_reject, per_round)
            continue
        runs = runs_of(name)
        rounds = []

        def counted(items, judge=judge):
            rounds.append(len(items))
            return judge(items)
        cands = [Candidate(sample_state(SEED, s), 0, spans) for s in range(len(runs))]
        accepted = speculate(cands, counted, p_reject, per_round)
        for c, acc, (starts, coins, _, _) in zip(cands, accepted, runs):
            assert np.array_equal(np.array(c.starts), starts), name
            assert c.coins == coins.tolist() and tuple(acc) == tuple(starts[-1]), name
        if sampler is not None:   # one judge call per round, and only unresolved samples come back
            need = max(len(r[0]) for r in runs)
            assert len(rounds) == -(-need // per_round) and rounds == sorted(rounds, reverse=True), (name, rounds)


def test_speculation_keeps_the_attempt_limit_exact():
    """a sample accepted at its 501st attempt is returned, one that would need a 502nd raises -- for a round size that does not
    divide 501 as well"""
    from torch_em_amd.data.device_dataset import Candidate, sample_state, speculate
    for per_round in (1, 8, 501):
        for first_ok, ok in ((500, True), (501, False)):
            seen = []

            def judge(items):
                out = [len(seen) + k == first_ok for k in range(len(items))]
                seen.extend(items)
                return out
            c = Candidate(sample_state(1, 2), 0, [5, 0, 7])
            if ok:
                speculate([c], judge, 1.0, per_round)
                assert len(c.starts) == 501 and len(c.coins) == 500 and all(st[1] == 0 for st in c.starts)
            else:
                with pytest.raises(RuntimeError, match="in 500 attempts"):
                    speculate([c], judge, 1.0, per_round)
                assert len(seen) == 501


def test_pickle_drops_the_volumes():
    """the trainer pickles train_loader.dataset into every checkpoint: the configuration travels, the volumes do not, and a
    restored dataset refuses to sample with the reference's message"""
    from torch_em_amd.data import DeviceSegmentationDataset, MinInstanceSampler
    ds = object.__new__(DeviceSegmentationDataset)
    unpicklable = lambda: None  # noqa: E731  (stands for device volumes: pickling it would fail)
    ds.__dict__.update(raw=unpicklable, labels=unpicklable, _ids=unpicklable, _sel=unpicklable, patch_shape=(4, 8, 16),
                       sampler=MinInstanceSampler(3), _len=7, _ndim=3)
    back = pickle.loads(pickle.dumps(ds))
    assert back.raw is None and back.labels is None and back._ids is None and back._sel is None
    assert back.patch_shape == (4, 8, 16) and len(back) == 7 and back.sampler.min_num_instances == 3
    assert ds.raw is unpicklable   # the live dataset keeps its volumes
    for use in (lambda: back.judge([]), lambda: back.gather([], [])):
        with pytest.raises(RuntimeError, match="has not been properly deserialized"):
            use()
    assert DeviceSegmentationDataset.compute_len((9, 20, 37), (4, 8, 16)) == 14
