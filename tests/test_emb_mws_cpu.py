"""CPU: the host-side argument checks of ops.embedding_edges / ops.merge_background_by_embedding_ (they come before anything
touches a device) and the C-ABI declarations of csrc/embmws.hip."""
import os
import re

import pytest
import torch

from conftest import ROOT

OFFS = [[-1, 0], [0, -1], [-9, 0]]


@pytest.mark.parametrize("kwargs, error, match", [
    ({"offsets": [[-1, 0], [0, -1, 0]]}, ValueError, "one length"),
    ({"emb": torch.zeros(1, 2, 3, 4, 4), "offsets": OFFS}, ValueError, "need D = 1"),
    ({"offsets": [[0, -1]] * 33}, ValueError, "at most 32"),
    ({"distance_type": "cosine"}, NotImplementedError, "cosine"),
    ({"distance_type": "linf"}, ValueError, "distance_type"),
    ({"delta": 0.0}, ValueError, "delta"),
    ({"delta": -1.5}, ValueError, "delta"),
    ({"strides": [2, 2, 2]}, ValueError, "strides"),
    ({"n_attractive": 4}, ValueError, "n_attractive"),
    ({"emb": torch.zeros(1, 65, 1, 4, 4)}, ValueError, "at most 64"),
])
def test_embedding_edges_refusals(kwargs, error, match):
    from torch_em_amd import ops
    args = {"emb": torch.zeros(1, 2, 1, 4, 4), "offsets": OFFS, "delta": 0.5, "n_attractive": 2, "strides": None,
            "distance_type": "l2", **kwargs}
    with pytest.raises(error, match=match):
        ops.embedding_edges(**args)


def test_merge_background_refusals():
    from torch_em_amd import ops
    ids, emb = torch.ones(1, 1, 4, 4, dtype=torch.int32), torch.zeros(1, 2, 1, 4, 4)
    with pytest.raises(ValueError, match="delta"):
        ops.merge_background_by_embedding_(ids, emb, 0)
    with pytest.raises(ValueError, match="int32 ids"):
        ops.merge_background_by_embedding_(ids.long(), emb, 0.5)
    with pytest.raises(ValueError, match="float32 embeddings"):
        ops.merge_background_by_embedding_(ids, emb[:, :, :, :3], 0.5)


def test_header_declares_the_entry_points():
    from torch_em_amd import _lib
    text = open(os.path.join(ROOT, "include", "tem_hip.h")).read()
    for name in ("tem_emb_edges", "tem_emb_bg_ws", "tem_emb_bg_stats"):
        assert re.search(r"^int(64_t)? %s\(" % name, text, flags=re.M) and name in _lib.SIGNATURES, name
    assert "#define TEM_EMB_MAX_DIM 64" in text
