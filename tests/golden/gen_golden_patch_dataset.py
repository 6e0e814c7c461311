"""Golden vectors made by RUNNING THE REFERENCE's SegmentationDataset and samplers (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_patch_dataset.py      (the reference's location: gen_golden_trainer.py)

G21 `torch_em.data.segmentation_dataset.SegmentationDataset._get_sample` (data/segmentation_dataset.py:155-216) with the samplers
    of `torch_em.data.sampler`, imported through `import_reference` of gen_golden_trainer.py.  The dataset reads files through
    `load_data` and applies a region of interest through `elf.wrapper.RoiWrapper`; neither elf nor a file is involved here, so
    two names of the reference's module are bound to stand-ins before the class runs: `load_data` -> the identity (the "path"
    IS the array) and `RoiWrapper` -> a view that slices the array with the roi.  Parity with those two is therefore not
    pinned by this fixture; every other line of `_get_sample`, `_sample_bounding_box`, `ensure_patch_shape` and the samplers is.
    Per configuration <c> and sample number s, `np.random.set_state` puts the global stream into
    `RandomState([SEED, s]).get_state()` -- the stream the device loader gives sample s -- and `_get_sample` runs with the
    bounding boxes and the sampler's coins recorded:
        <c>/starts   int16 [attempts, rank]: the start of every box tried, in order (a sample's last one was accepted)
        <c>/coins    float64: the `np.random.rand()` coins the sampler drew, in order
        <c>/counts   int64 [N_SAMPLES, 2]: attempts and coins of sample s -- starts and coins are the samples' runs, concatenated
        <c>/raw, <c>/labels: [N_SAMPLES, ...] what `_get_sample` returned (padded, squeezed)
    plus the volumes (`vol/<name>/raw`, `vol/<name>/labels`) and `configs`: the JSON of CONFIGS.  A configuration that can
    never accept is stored as "raises": 1 with no samples.
    The generator asserts that no stored run needs more than 500 attempts, that one needs more than 3, that one accepts through
    the coin, and that one configuration raises -- so the limits the tests use hide nothing.
The fixture is data (inputs + what the reference computed); no reference source is copied.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "g21_patch_dataset.npz")
SEED = 2024
N_SAMPLES = 3

# name -> volume, patch_shape, sampler class and arguments, dataset arguments
CONFIGS = {
    "none": dict(vol="a", patch=(4, 8, 16), sampler=None),
    "fg_int": dict(vol="a", patch=(4, 8, 16), sampler="MinForegroundSampler", args=dict(min_fraction=0.3, background_id=0)),
    "fg_list": dict(vol="a", patch=(4, 8, 16), sampler="MinForegroundSampler",
                    args=dict(min_fraction=0.2, background_id=[0, 12], p_reject=0.7)),
    "sem_count": dict(vol="a", patch=(4, 8, 16), sampler="MinSemanticLabelForegroundSampler",
                      args=dict(semantic_ids=[3, 7, 99], min_fraction=150)),
    "sem_per_id": dict(vol="a", patch=(4, 8, 16), sampler="MinSemanticLabelForegroundSampler",
                       args=dict(semantic_ids=[3, 7], min_fraction=0.02, min_fraction_per_id=True)),
    "inst": dict(vol="a", patch=(4, 8, 16), sampler="MinInstanceSampler",
                 args=dict(min_num_instances=3, min_size=5, exclude_ids=[12])),
    "inst_2d": dict(vol="b", patch=(1, 16, 16), ndim=2, sampler="MinInstanceSampler", args=dict(min_num_instances=3, p_reject=0.9)),
    "two": dict(vol="a", patch=(4, 8, 16), sampler="MinTwoInstanceSampler", args=dict(p_reject=0.5)),
    "median": dict(vol="a", patch=(4, 8, 16), sampler="MinIntensitySampler", args=dict(min_intensity=99, function="median")),
    "max_f32": dict(vol="b", patch=(1, 16, 16), sampler="MinIntensitySampler", args=dict(min_intensity=1.5, function="max")),
    "min_chan": dict(vol="d", patch=(4, 8, 16), with_channels=True, sampler="MinIntensitySampler",
                     args=dict(min_intensity=-90, function="min", p_reject=0.8)),
    "median_pad": dict(vol="c", patch=(4, 8, 16), sampler="MinIntensitySampler", args=dict(min_intensity=150.25, function="median")),
    "fg_pad": dict(vol="c", patch=(4, 8, 16), sampler="MinForegroundSampler", args=dict(min_fraction=0.25)),
    "fg_roi": dict(vol="a", patch=(4, 8, 16), roi=[[1, 8], [2, 20], [0, 30]], sampler="MinForegroundSampler",
                   args=dict(min_fraction=0.3)),
    "never": dict(vol="a", patch=(4, 8, 16), sampler="MinInstanceSampler", args=dict(min_num_instances=50)),
}


def make_volumes():
    """a: (9, 20, 37) uint8 raw / int32 labels; b: (1, 33, 35) float32 raw / uint8 labels; c: (3, 20, 37), the z axis shorter than
    the patch, uint16 raw / int64 labels; d: (5, 12, 21), 3-channel int16 raw / uint16 labels.  Blobs are brighter than background."""
    rs = np.random.RandomState(7)
    la = np.zeros((9, 20, 37), np.int32)
    la[2:6, 4:12, 20:30], la[5:9, 12:18, 2:9], la[0:2, 0:3, 30:37], la[7, 3, 15] = 3, 7, 12, 5
    ra = (rs.randint(0, 100, la.shape) + 110 * (la > 0)).astype(np.uint8)
    lb = np.zeros((1, 33, 35), np.uint8)
    lb[0, 3:12, 5:17], lb[0, 10:25, 20:33], lb[0, 26:33, 0:9], lb[0, 20:22, 10:12] = 1, 2, 4, 9
    rb = (rs.rand(*lb.shape) + (lb > 0)).astype(np.float32)
    lc = la[3:6].astype(np.int64) * 1000003
    rc = (rs.randint(0, 200, lc.shape) + 40000 * (lc > 0)).astype(np.uint16)
    ld = la[2:7, 4:16, 16:37].astype(np.uint16)
    rd = (rs.randint(-100, 100, (3,) + ld.shape) + 200 * (ld > 0)[None]).astype(np.int16)
    return {"a": (ra, la), "b": (rb, lb), "c": (rc, lc), "d": (rd, ld)}


class _Roi:
    """the slicing stand-in for elf.wrapper.RoiWrapper"""

    def __init__(self, data, roi):
        self._view = data[roi]
        self.shape = self._view.shape

    def __getitem__(self, bb):
        return self._view[bb]


def dataset_kwargs(cfg):
    kw = dict(with_channels=bool(cfg.get("with_channels", False)))
    if cfg.get("roi") is not None:
        kw["roi"] = tuple(slice(a, b) for a, b in cfg["roi"])
    if cfg.get("ndim") is not None:
        kw["ndim"] = cfg["ndim"]
    return kw


def run_tensor_dataset(TensorDataset):
    """this package's host TensorDataset WITHOUT a sampler, under np.random.seed(5): two images (the second shorter than the
    patch in z: reflect padding), a random image per sample -> the samples and the next draw of the global stream"""
    ra, la = make_volumes()["a"]
    ds = TensorDataset([ra, ra[:3]], [la, la[:3]], patch_shape=(4, 8, 16), n_samples=4)
    np.random.seed(5)
    items = [ds[i] for i in range(len(ds))]
    return (np.stack([x.numpy() for x, _ in items]), np.stack([y.numpy() for _, y in items]), np.int64(np.random.randint(0, 2 ** 31)))


def main():
    sys.path[:0] = [HERE, ROOT]
    from gen_golden_trainer import import_reference
    import_reference()
    import torch_em.data.sampler as ref_sampler
    import torch_em.data.segmentation_dataset as ref
    ref.load_data = lambda path, key: path
    ref.RoiWrapper = _Roi
    vols = make_volumes()
    out = {"configs": np.array(json.dumps(CONFIGS)), "seed": np.int64(SEED)}
    for name, (r, l) in vols.items():
        out[f"vol/{name}/raw"], out[f"vol/{name}/labels"] = r, l
    most, by_coin, raised = 0, 0, 0
    for cname, cfg in CONFIGS.items():
        sampler = None if cfg["sampler"] is None else getattr(ref_sampler, cfg["sampler"])(**cfg["args"])
        raw, labels = vols[cfg["vol"]]
        ds = ref.SegmentationDataset(raw, None, labels, None, patch_shape=tuple(cfg["patch"]), sampler=sampler, **dataset_kwargs(cfg))
        starts, coins = [], []
        sample_bb, rand = ds._sample_bounding_box, np.random.rand

        def rec_bb():
            bb = sample_bb()
            starts.append([s.start for s in bb])
            return bb

        def rec_rand(*a):
            v = rand(*a)
            coins.append(v)
            return v
        ds._sample_bounding_box = rec_bb
        runs = []
        for s in range(N_SAMPLES):
            del starts[:], coins[:]
            np.random.set_state(np.random.RandomState([SEED, s]).get_state())
            np.random.rand = rec_rand
            try:
                x, y = ds._get_sample(0)
            except RuntimeError as e:
                assert "Could not sample a valid batch in 500 attempts" in str(e), e
                assert len(starts) == 502 and len(coins) == 501   # the 502nd box is drawn and never judged
                out[f"{cname}/raises"] = np.int64(1)
                raised += 1
                break
            finally:
                np.random.rand = rand
            assert len(starts) <= 501
            accepted_by_coin = len(coins) == len(starts)   # every attempt failed its criterion, the last coin let it through
            by_coin += accepted_by_coin
            most = max(most, len(starts))
            runs.append((np.array(starts, dtype=np.int16), np.array(coins, dtype=np.float64), x, y))
            print(cname, s, "attempts", len(starts), "coins", len(coins), "by coin" if accepted_by_coin else "", x.shape, x.dtype, y.dtype)
        if runs:
            out[f"{cname}/starts"] = np.concatenate([r[0] for r in runs])
            out[f"{cname}/coins"] = np.concatenate([r[1] for r in runs])
            out[f"{cname}/counts"] = np.array([[len(r[0]), len(r[1])] for r in runs], dtype=np.int64)
            out[f"{cname}/raw"], out[f"{cname}/labels"] = np.stack([r[2] for r in runs]), np.stack([r[3] for r in runs])
    # recorded with the TensorDataset as it was before it learned to call its sampler (`tds/...`): the sampler-less path must
    # keep its values and its consumption of np.random
    from torch_em_amd.data.tensor_dataset import TensorDataset
    out["tds/raw"], out["tds/labels"], out["tds/next"] = run_tensor_dataset(TensorDataset)
    assert most > 3, most
    assert by_coin >= 1 and raised == 1, (by_coin, raised)
    np.savez_compressed(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes; most attempts", most, "accepted by coin", by_coin)


if __name__ == "__main__":
    main()
