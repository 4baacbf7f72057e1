"""CPU tests of the grid run's host side (wdg_amd.split_train): select_settings on hand-written [G, S, 3] tables, the chunk cut of
grid_search, and the refusals that come before any device is asked for."""
import numpy as np
import pytest


def _masks(n=40, S=3):
    masks = np.zeros((S, 3, n), bool)
    for s in range(S):
        masks[s, 0, s:20 + s], masks[s, 1, 20 + s:30 + s], masks[s, 2, 30 + s:37 + s] = True, True, True
    return masks


def test_a_tie_goes_to_the_lowest_setting_index():
    from wdg_amd.split_train import select_settings
    best = np.array([[[7, 3, 4], [5, 1, 0]],
                     [[9, 6, 2], [8, 4, 1]],
                     [[9, 2, 7], [8, 9, 3]]])  # settings 1 and 2 tie on both splits: 1 is picked, although 2 tests better on split 1
    out = select_settings(best, n_val=[10, 16], n_test=[12, 10])
    assert out["setting"].tolist() == [1, 1] and out["best_epoch"].tolist() == [2, 1]
    assert out["val_acc"].tolist() == [0.9, 0.5] and out["test_acc"].tolist() == [0.5, 0.4]
    assert out["test_mean"] == pytest.approx(0.45) and out["test_std"] == pytest.approx(np.std([0.5, 0.4], ddof=1))
    # the setting of the best mean validation accuracy: (0.9 + 0.5) / 2 for settings 1 and 2 alike - the lower index again
    assert out["mean_val_acc"].tolist() == pytest.approx([(0.7 + 5 / 16) / 2, 0.7, 0.7]) and out["best_mean_setting"] == 1
    assert out["best_mean_test_mean"] == pytest.approx(0.45)
    # per split, not per grid: each split may pick its own setting
    best = np.array([[[7, 3, 4], [2, 1, 0]], [[6, 6, 2], [8, 4, 1]]])
    out = select_settings(best, [10, 10], [10, 10])
    assert out["setting"].tolist() == [0, 1] and out["test_acc"].tolist() == [0.3, 0.4]
    assert out["best_mean_setting"] == 1 and out["best_mean_test_mean"] == pytest.approx(0.5) and out["best_mean_test_std"] == pytest.approx(np.std([0.6, 0.4], ddof=1))


def test_a_replica_without_a_best_epoch_never_wins():
    from wdg_amd.split_train import select_settings
    best = np.array([[[-1, 0, 0], [-1, 0, 0]],
                     [[0, 5, 3], [-1, 0, 0]]])  # split 0: zero validation hits still beat "none yet"; split 1: nobody has a best epoch
    out = select_settings(best, [10, 10], [10, 10])
    assert out["setting"].tolist() == [1, 0] and out["test_acc"].tolist() == [0.5, 0.0] and out["val_acc"].tolist() == [0.0, -1.0]
    assert out["mean_val_acc"].tolist() == [0.0, 0.0] and out["best_mean_setting"] == 0
    # a -1 row's other words are not read as counts
    best = np.array([[[-1, 99, 99]], [[3, 2, 1]]])
    out = select_settings(best, [10], [10])
    assert out["setting"].tolist() == [1] and out["test_acc"].tolist() == [0.2] and out["best_mean_test_mean"] == pytest.approx(0.2)


def test_a_single_split_has_deviation_zero():
    from wdg_amd.split_train import select_settings
    out = select_settings(np.array([[[4, 3, 0]], [[6, 5, 9]]]), [8], [10])
    assert out["setting"].tolist() == [1] and out["test_mean"] == 0.5 and out["test_std"] == 0.0 and out["best_mean_test_std"] == 0.0
    assert np.isfinite(out["test_std"])


def test_select_settings_refuses_other_tables():
    from wdg_amd.split_train import select_settings
    with pytest.raises(ValueError):
        select_settings(np.zeros((2, 3)), [1, 1, 1], [1, 1, 1])
    with pytest.raises(ValueError):
        select_settings(np.zeros((2, 3, 3)), [1, 1, 1], [1, 1, 1])        # floats: the table holds counts
    with pytest.raises(ValueError):
        select_settings(np.zeros((2, 3, 3), np.int64), [1, 1], [1, 1, 1])  # one count per split
    with pytest.raises(ValueError):
        select_settings(np.zeros((2, 3, 3), np.int64), [1, 0, 1], [1, 1, 1])


def test_the_chunk_cut_keeps_whole_settings_in_order():
    from wdg_amd.split_train import chunk_settings, default_max_replicas
    assert chunk_settings(12, 10, 120) == [(0, 12)]
    assert chunk_settings(12, 10, 64) == [(0, 6), (6, 12)]          # 64 replicas hold six whole settings, not 6.4
    assert chunk_settings(12, 10, 50) == [(0, 5), (5, 10), (10, 12)]
    assert chunk_settings(4, 3, 6) == [(0, 2), (2, 4)] and chunk_settings(4, 3, 3) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert chunk_settings(1, 7, 1000) == [(0, 1)]
    for G, S, cap in ((12, 10, 64), (7, 3, 10), (5, 4, 4)):
        cut = chunk_settings(G, S, cap)
        assert [g for a, b in cut for g in range(a, b)] == list(range(G)) and all(0 < (b - a) * S <= cap for a, b in cut)
    with pytest.raises(ValueError):
        chunk_settings(12, 10, 9)                                    # not even one setting fits
    with pytest.raises(ValueError):
        chunk_settings(0, 10, 100)
    # the default: whole settings within the activation budget - n * R * hidden * 4 bytes, five such buffers for "gcn"
    assert default_max_replicas(2708, 64, "gcn", 10) == ((1 << 30) // (2708 * 64 * 4 * 5)) // 10 * 10 == 300
    assert default_max_replicas(2708, 64, "mlp2", 10) > default_max_replicas(2708, 64, "gcn", 10)
    assert default_max_replicas(10 ** 7, 64, "gcn", 10) == 10       # never less than one setting


def test_grid_search_refuses_before_it_asks_for_a_device():
    from wdg_amd.split_train import grid_search
    masks, x, labels = _masks(), np.zeros((40, 4), np.float32), np.arange(40) % 4
    grid = [dict(lr=0.01, weight_decay=5e-4, dropout=0.0), dict(lr=0.05, weight_decay=0.0, dropout=0.5)]
    with pytest.raises(ValueError, match="max_replicas"):
        grid_search(None, x, labels, masks, grid, kind="mlp2", max_replicas=2)           # fewer than the three splits of one setting
    with pytest.raises(ValueError):
        grid_search(None, x, labels, masks, [], kind="mlp2")                             # no setting
    with pytest.raises(ValueError):
        grid_search(None, x, labels, masks, [dict(lr=0.01, weight_decay=0.0)], kind="mlp2")   # a setting without its dropout
    with pytest.raises(ValueError):
        grid_search(None, x, labels, masks, grid, kind="mlp1")                           # dropout without a hidden layer
    with pytest.raises(ValueError):
        grid_search(None, x, labels, masks, grid, kind="acm_gcn")
    with pytest.raises(ValueError):
        grid_search(None, x, labels, masks.astype(np.int32), grid, kind="mlp2")


def test_sequences_need_the_device_optimizer():
    """a per-replica lr, weight_decay or dropout with the default optimizer is refused, with a message that names the remedy -
    before the masks are looked at and before any device is asked for"""
    from wdg_amd.split_train import SplitTrainBatch
    masks, x, labels = _masks(), np.zeros((40, 4), np.float32), np.arange(40) % 4
    for kw in (dict(lr=[0.01, 0.02, 0.03]), dict(weight_decay=[0.0, 1e-3, 1e-2]), dict(dropout=[0.0, 0.5, 0.5]),
               dict(lr=np.array([0.01, 0.02, 0.03]), optimizer="torch")):
        with pytest.raises(ValueError, match='optimizer="device"'):
            SplitTrainBatch(None, x, labels, masks, kind="mlp2", **kw)
    with pytest.raises(ValueError):
        SplitTrainBatch(None, x, labels, masks, kind="mlp2", optimizer="sgd")
    with pytest.raises(ValueError):
        SplitTrainBatch(None, x, labels, masks, kind="mlp2", optimizer="device", lr=[0.01, 0.02])            # two values, three replicas
    with pytest.raises(ValueError):
        SplitTrainBatch(None, x, labels, masks, kind="mlp1", optimizer="device", dropout=[0.0, 0.0, 0.0])    # no hidden layer
    with pytest.raises(ValueError):
        SplitTrainBatch(None, x, labels, masks, kind="mlp2", optimizer="device", dropout=[0.0, 1.0, 0.5])    # a probability of 1
    with pytest.raises(ValueError):
        SplitTrainBatch(None, x, labels, masks, kind="mlp2", optimizer="device", replica_ids=[0, 1])
    with pytest.raises(ValueError):
        SplitTrainBatch(None, x, labels, masks, kind="mlp2", optimizer="device", replica_ids=[0, -1, 2])
