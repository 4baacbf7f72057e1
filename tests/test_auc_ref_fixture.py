"""CPU check of the fixture of tests/test_gpu_auc_split_train.py (tests/_auc_split_fixture.py): in a float64 restatement of the stacked
"sgc" run, "strictly more validation hits" keeps epoch 0 for at least one replica while the validation AUC selects a later epoch - the
property the GPU test asserts of the device's run."""
import numpy as np

import _auc_split_fixture as fx


def test_the_fixture_separates_the_two_rules():
    p = fx.graph200()
    labels, masks = p["labels"], p["masks"]
    assert 0.1 < labels.mean() < 0.2 and masks.shape == (fx.R, 3, fx.N) and len({int(m.sum()) for m in masks[:, 1]}) == fx.R  # unequal splits
    assert not (masks.sum(1) > 1).any()
    for r in range(fx.R):
        assert set(labels[masks[r, 1]]) == {0, 1}  # both classes among every replica's validation rows
    by_hits, by_auc = fx.sgc_host_run(p)
    stuck = by_hits == 0
    assert stuck.any() and (by_auc[stuck] > 0).all(), (by_hits, by_auc)
    codes = fx.split_codes(masks)
    assert codes.shape == (fx.N, fx.R) and codes.dtype == np.uint8 and set(np.unique(codes)) <= {0, 1, 2, 3}
