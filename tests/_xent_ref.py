"""numpy restatement of wdg_xent_eval_batched_f32 as include/wdg.h defines it: for stacked logits [n, R cs] (replica r's classes
are columns r cs .. r cs + C - 1) the cross-entropy gradient of every replica's train rows, its validation / test hits and its
model selection - in float64 (the yardstick of the GPU tests) or float32 (the kernel's own order of operations; its distance from
float64 sizes their bound).  tests/test_xent_ref.py pins it against torch.nn.functional.cross_entropy autograd and argmax."""
import numpy as np

TRAIN, VALID, TEST = 1, 2, 3


def xent_grad(logits, labels, split, n_train, C, cs, dtype=np.float64):
    """-> dlogits [n, R cs] of `dtype`: (softmax(z) - onehot(label)) * (1 / n_train_r) on the rows with split code 1, +0 elsewhere and
    in the padding columns.  m = max z; e = exp(z - m); s = e_0 + e_1 + ... in that order; the quotient, the subtraction and the
    product follow, each rounded to `dtype`.  1 / n_train_r is formed in float64 and rounded to `dtype` (the host's (float)(1 / n)).
    A label outside 0 .. C - 1 matches no class; a NaN among the z's makes the C gradients NaN.  Columns beyond R cs are not read."""
    dt = np.dtype(dtype).type
    split = np.asarray(split)
    n, R = split.shape
    labels = np.asarray(labels)
    out = np.zeros((n, R * cs), dtype)
    for r in range(R):
        rows = np.nonzero(split[:, r] == TRAIN)[0]
        if rows.size == 0:
            continue
        z = np.asarray(logits)[rows, r * cs:r * cs + C].astype(dtype)
        with np.errstate(invalid="ignore"):
            m = z.max(1, keepdims=True)  # (numpy's max hands a NaN on)
            e = np.exp(z - m)
            s = e[:, 0].copy()
            for k in range(1, C):
                s = s + e[:, k]
            onehot = (np.arange(C)[None, :] == labels[rows][:, None]).astype(dtype)
            out[rows, r * cs:r * cs + C] = (e / s[:, None] - onehot) * dt(1.0 / float(n_train[r]))
    return out


def predictions(logits, R, C, cs):
    """-> int [n, R]: the first k with z_k == max z, or -2 (matches no label, not even -1) for a row with a NaN among its z's"""
    z = np.asarray(logits)[:, :R * cs].reshape(logits.shape[0], R, cs)[:, :, :C]
    nan = np.isnan(z).any(2)
    pred = np.where(nan[..., None], -np.inf, z).argmax(2)  # (numpy: the first maximum)
    return np.where(nan, -2, pred)


def xent_hits(logits, labels, split, C, cs):
    """-> int [R, 2]: validation hits, test hits of every replica"""
    split = np.asarray(split)
    pred = predictions(np.asarray(logits), split.shape[1], C, cs)
    hit = pred == np.asarray(labels)[:, None]
    return np.stack([(hit & (split == VALID)).sum(0), (hit & (split == TEST)).sum(0)], 1).astype(np.int64)


def select(best, hits, step):
    """the model selection: best [R, 3] (validation hits of the best call, -1 = none yet; test hits at it; its step) after a call that
    counted `hits` [R, 2] with the step word at `step` - replaced where the validation hits are STRICTLY greater"""
    best = np.array(best, np.int64)
    better = hits[:, 0] > best[:, 0]
    best[better] = np.concatenate([hits[better], np.full((int(better.sum()), 1), step, np.int64)], 1)
    return best


def make_case(n, R, C, cs, seed, no_test_replica=None, train_only=False):
    """one job's host side: labels int32 [n] (uniform over the classes, ONE of them -1, in a row every replica uses), split uint8 [n, R]
    with replica r's own cut of a seeded permutation (train 35 % + 7 % per replica, validation 20 % + 3 % per replica, of the rest all
    but every fifth row test: unequal sizes, some rows unused), n_train [R].  no_test_replica: a replica whose test rows are unused
    instead; train_only: every row outside the train sets is unused (code 0)."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, n).astype(np.int32)
    split = np.zeros((n, R), np.uint8)
    for r in range(R):
        perm = rng.permutation(n)
        a = max(1, int(n * min(0.35 + 0.07 * r, 0.7)))
        b = min(n, a + max(1, int(n * min(0.2 + 0.03 * r, 0.25))))
        split[perm[:a], r] = TRAIN
        if not train_only:
            split[perm[a:b], r] = VALID
            rest = perm[b:]
            if r != no_test_replica:
                split[rest[np.arange(rest.size) % 5 != 4], r] = TEST
    labels[int(rng.integers(0, n))] = -1
    return dict(n=n, R=R, C=C, cs=cs, labels=labels, split=split, n_train=(split == TRAIN).sum(0).astype(np.int64))


def normal_logits(case, ld, seed, scale=4.0, fill=0.0):
    """fp32 [n, ld]: standard normal times `scale` in the class columns, `fill` in the padding columns and between R cs and ld"""
    rng = np.random.default_rng(seed)
    n, R, C, cs = case["n"], case["R"], case["C"], case["cs"]
    out = np.full((n, ld), fill, np.float32)
    for r in range(R):
        out[:, r * cs:r * cs + C] = (rng.standard_normal((n, C)) * scale).astype(np.float32)
    return out


def grid_logits(case, ld, seed, lift=0.0, lift_test=None, fill=0.0):
    """fp32 [n, ld] for the exact checks: multiples of 1 / 64 in [-4, 4] (fp32 and fp64 agree on every maximum); on about 5 % of the
    (row, replica) pairs a second class is set equal to the maximum (the first one wins); on a fraction `lift` of the validation
    pairs and `lift_test` (default: lift) of the test pairs the label's class is raised to 5 (so the hit counts can be steered);
    then ONE row gets a NaN in every replica's first class."""
    rng = np.random.default_rng(seed)
    n, R, C, cs = case["n"], case["R"], case["C"], case["cs"]
    labels, split = case["labels"], case["split"]
    lift_test = lift if lift_test is None else lift_test
    out = np.full((n, ld), fill, np.float32)
    for r in range(R):
        z = (rng.integers(-256, 257, (n, C)) / 64.0).astype(np.float32)
        u = rng.random(n)
        want = np.where(split[:, r] == TEST, lift_test, lift)
        rows = np.nonzero((u < want) & (labels >= 0))[0]
        z[rows, labels[rows]] = 5.0
        if C > 1:
            tie = np.nonzero(rng.random(n) < 0.05)[0]
            other = (z[tie].argmax(1) + rng.integers(1, C, tie.size)) % C
            z[tie, other] = z[tie].max(1)
        out[:, r * cs:r * cs + C] = z
    scored = np.nonzero(((split == VALID) | (split == TEST)).any(1))[0]
    nan_row = int(scored[0]) if scored.size else 0
    out[nan_row, np.arange(R) * cs] = np.nan
    return out
