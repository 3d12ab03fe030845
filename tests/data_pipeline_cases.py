"""NumPy restatement of the loader's laws (DESIGN.md §4 "Loader"): the epoch permutation, the weighted draw, the crop offset
and the gather.  Integer arithmetic and single IEEE double operations only, so the device must agree bit for bit.
tests/test_data_pipeline_host.py checks the restatement by itself; tests/test_data_pipeline_gpu.py holds the kernels to it."""
import numpy as np

from oracle.philox import philox4x32_10, make_key

TAG_DATA = 3
_TAGW = TAG_DATA << 24


def _philox(c0, c1, c2, c3, seed):
    c0 = np.asarray(c0, dtype=np.uint64)
    ctr = np.empty(c0.shape + (4,), dtype=np.uint64)
    ctr[..., 0], ctr[..., 1], ctr[..., 2], ctr[..., 3] = c0, c1, c2, c3
    return philox4x32_10(ctr, make_key(int(seed))).astype(np.uint64)


def feistel_half_bits(n):
    """Half of the even width w with 2**w >= max(n, 4)."""
    half = 1
    while (1 << (2 * half)) < n:
        half += 1
    return half


def perm(g, n, seed, epoch):
    """perm_epoch(g) for an array of positions g < n: 4-round balanced Feistel over w bits, cycle-walked into [0, n)."""
    g = np.asarray(g, dtype=np.uint64)
    assert g.size == 0 or int(g.max()) < n
    half = np.uint64(feistel_half_bits(n))
    mask = np.uint64((1 << int(half)) - 1)
    elo = int(epoch) & 0xFFFFFFFF
    x = g.copy()
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        v = x[todo]
        l, r = v >> half, v & mask
        for j in range(4):
            f = _philox(r, j, elo, _TAGW, seed)[..., 0] & mask
            l, r = r, l ^ f
        v = (l << half) | r
        x[todo] = v
        todo[todo] = v >= np.uint64(n)
    return x.astype(np.int64)


def positions(rank, world, k0, count):
    """g = rank + world * k for k = k0 .. k0 + count - 1."""
    return np.uint64(rank) + np.uint64(world) * (np.uint64(k0) + np.arange(count, dtype=np.uint64))


def samples_per_rank(n, world):
    return n // world


def batches_per_epoch(n, world, batch, drop_last):
    m = samples_per_rank(n, world)
    return m // batch if drop_last else -(-m // batch)


def sampler_weights(labels, hard_negative=None, strategy="balanced", hard_negative_weight=1.0):
    """float64 weight per clip: 1 / count[label] (balanced), times hard_negative_weight on the flagged clips (weighted)."""
    labels = np.asarray(labels).astype(np.int64)
    if strategy == "none":
        return np.ones(labels.shape, dtype=np.float64)
    assert strategy in ("balanced", "weighted")
    w = 1.0 / np.bincount(labels)[labels].astype(np.float64)
    if strategy == "weighted" and hard_negative is not None:
        w = w * np.where(np.asarray(hard_negative, dtype=bool), np.float64(hard_negative_weight), np.float64(1.0))
    return w


def cdf_table(weights):
    """The shared table: np.cumsum in float64, cut after the last non-zero weight."""
    w = np.asarray(weights, dtype=np.float64)
    assert w.ndim == 1 and (w >= 0).all() and np.isfinite(w).all() and (w > 0).any()
    n_eff = int(np.flatnonzero(w > 0)[-1]) + 1
    return np.cumsum(w[:n_eff])


def table_draw(g, cdf, seed, epoch):
    """First i with cdf[i] > u53 * 2**-53 * total, clamped to the last entry."""
    g = np.asarray(g, dtype=np.uint64)
    x = _philox(g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), int(epoch) & 0xFFFFFFFF, _TAGW | 1, seed)
    u53 = ((x[..., 0] << np.uint64(32)) | x[..., 1]) >> np.uint64(11)
    target = (u53.astype(np.float64) * np.float64(2.0 ** -53)) * np.float64(cdf[-1])
    return np.minimum(np.searchsorted(cdf, target, side="right"), len(cdf) - 1).astype(np.int64)


def indices(n, strategy, seed, epoch, rank, world, k0, count, cdf=None, shuffle=True):
    g = positions(rank, world, k0, count)
    if strategy != "none":
        return table_draw(g, cdf, seed, epoch)
    if not shuffle:
        assert g.size == 0 or int(g.max()) < n
        return g.astype(np.int64)
    return perm(g, n, seed, epoch)


def crop_offsets(g, lengths, n_out, seed, epoch, training):
    """mulhi32(philox(g, epoch, tag 2)[0], len - n_out + 1) where len > n_out and training, else 0."""
    g = np.asarray(g, dtype=np.uint64)
    lengths = np.asarray(lengths, dtype=np.int64)
    x0 = _philox(g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), int(epoch) & 0xFFFFFFFF, _TAGW | 2, seed)[..., 0]
    span = np.maximum(lengths - n_out + 1, 0).astype(np.uint64)
    off = ((x0 * span) >> np.uint64(32)).astype(np.int64)
    return np.where((lengths > n_out) & bool(training), off, 0)


def batch(bank, lengths, labels, n_out, strategy, seed, epoch, rank, world, k0, count, cdf=None, shuffle=True, training=True):
    """-> (wave int16 (count, n_out), targets int64, clip_index int32, offsets int64) of one loader batch."""
    bank, lengths = np.asarray(bank), np.asarray(lengths, dtype=np.int64)
    idx = indices(bank.shape[0], strategy, seed, epoch, rank, world, k0, count, cdf, shuffle)
    ln = np.clip(lengths[idx], 0, bank.shape[1])
    off = crop_offsets(positions(rank, world, k0, count), ln, n_out, seed, epoch, training)
    out = np.zeros((count, n_out), dtype=np.int16)
    for b in range(count):
        m = int(min(ln[b], n_out))
        out[b, :m] = bank[idx[b], off[b]:off[b] + m]
    return out, np.asarray(labels)[idx].astype(np.int64), idx.astype(np.int32), off


def zero_run_weights(n=64, seed=0):
    """Random weights with zero-weight clips at the start, in the middle and at the end of the table."""
    w = np.random.default_rng(seed).random(n) + 0.05
    w[:3] = 0.0
    w[n // 2:n // 2 + 5] = 0.0
    w[-4:] = 0.0
    return w
