"""The fixture of tests/test_gpu_auc_split_train.py, host side only: a 200-node random graph with 85/15 binary labels, 16 features - a
large constant one, which decides the prediction of a freshly initialised model for EVERY row, and a weak class signal in the others,
which moves the ranking long before it moves a prediction - and three replicas with unequal splits.  sgc_host_run restates a stacked
"sgc" run on the CPU (torch autograd, float64) closely enough to say which epochs the two selection rules pick."""
import numpy as np
import torch

import _auc_ref as ref

N, F, R, LR, EPOCHS, SEED = 200, 16, 3, 0.05, 6, 2


def graph200():
    rng = np.random.default_rng(5)
    labels = (rng.random(N) < 0.15).astype(np.int64)
    x = (0.6 * rng.standard_normal((N, F)) + 0.5 * labels[:, None] * (np.arange(F) % 2 == 1)).astype(np.float32)
    x[:, 0] = 4.0
    src = np.repeat(np.arange(N), 3)
    dst = rng.integers(0, N, 3 * N)
    keep = src != dst
    src, dst = np.concatenate([src[keep], dst[keep]]), np.concatenate([dst[keep], src[keep]])
    edges = np.unique(np.stack([src, dst]), axis=1)
    masks = np.zeros((R, 3, N), bool)
    for r, (a, b, t) in enumerate(((0.5, 0.25, 0.25), (0.6, 0.2, 0.18), (0.4, 0.3, 0.27))):
        perm = rng.permutation(N)
        i, j, k = int(a * N), int((a + b) * N), int((a + b + t) * N)
        masks[r, 0, perm[:i]], masks[r, 1, perm[i:j]], masks[r, 2, perm[j:k]] = True, True, True
    adj = torch.sparse_coo_tensor(torch.from_numpy(edges), torch.ones(edges.shape[1]), (N, N))
    return dict(n=N, f=F, c=2, labels=labels, x=x, masks=masks, adj=adj, edges=edges)


def split_codes(masks):
    return np.ascontiguousarray((masks[:, 0] * 1 + masks[:, 1] * 2 + masks[:, 2] * 3).astype(np.uint8).T)  # [n, R]


def replay(logits_per_epoch, labels, split, cs, patience=0):
    """the rule of include/wdg.h over the logits of every epoch -> (the state of tests/_auc_ref.py, u2 of every epoch, pairs)"""
    n_rep = split.shape[1]
    st = ref.new_state(n_rep, len(logits_per_epoch))
    pairs = None
    for s, z in enumerate(logits_per_epoch):
        u2, pairs = ref.auc_job(z, labels, split, n_rep, cs)
        ref.step(st, u2, s, 1, patience)
    return st, st["curve"], pairs


def sgc_host_run(p, seed=SEED, lr=LR, epochs=EPOCHS, weight_decay=5e-4):
    """-> (best epoch by strictly more validation hits [R], best epoch by the validation AUC integer [R]) of a float64 restatement of the
    stacked "sgc" run: Y = D^-1 (A + I) X, logits = Y W, Xavier weights from the run's own generators, torch's Adam, an evaluation of the
    stepped weights per epoch"""
    from wdg_amd.split_train import replica_seed, xavier
    n = p["n"]
    a = np.zeros((n, n))
    a[p["edges"][0], p["edges"][1]] = 1.0
    a += np.eye(n)
    y = torch.from_numpy((a / a.sum(1, keepdims=True)) @ p["x"].astype(np.float64))
    labels = torch.from_numpy(p["labels"])
    by_hits, by_auc = [], []
    for r in range(p["masks"].shape[0]):
        w = xavier(p["f"], 2, torch.Generator(device="cpu").manual_seed(replica_seed(seed, r))).double().requires_grad_()
        opt = torch.optim.Adam([w], lr=lr, weight_decay=weight_decay)
        train, val = (torch.from_numpy(p["masks"][r, k]) for k in (0, 1))
        best_hits, best_u2, e_hits, e_auc = -1, -1, 0, 0
        for e in range(epochs):
            opt.zero_grad()
            torch.nn.functional.cross_entropy((y @ w)[train], labels[train]).backward()
            opt.step()
            with torch.no_grad():
                z = (y @ w)[val]
            hits = int((z.argmax(1) == labels[val]).sum())
            u2, _ = ref.u2_pairs((z[:, 1] - z[:, 0]).float().numpy(), p["labels"][p["masks"][r, 1]])
            if hits > best_hits:
                best_hits, e_hits = hits, e
            if u2 > best_u2:
                best_u2, e_auc = u2, e
        by_hits.append(e_hits)
        by_auc.append(e_auc)
    return np.array(by_hits), np.array(by_auc)
