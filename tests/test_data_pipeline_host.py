"""Host: the loader's laws as restated in tests/data_pipeline_cases.py meet their own conditions (bijection, shards, zero
weights, class shares), and the host side of wakeword_trainer_home_amd.data.loader agrees with the restatement."""
import numpy as np
import pytest
import torch

from tests import data_pipeline_cases as C

PERM_SIZES = (1, 2, 3, 5, 16, 17, 1000, 4097, 65537)


@pytest.mark.parametrize("n", PERM_SIZES)
def test_perm_is_a_bijection(n):
    for seed, epoch in ((0, 0), (1, 0), (0, 1), (7, 2 ** 31 + 5)):
        p = C.perm(np.arange(n), n, seed, epoch)
        assert p.min() >= 0 and p.max() < n
        assert np.array_equal(np.sort(p), np.arange(n)), (n, seed, epoch)


def test_feistel_width_is_the_even_width_covering_n():
    for n, half in ((1, 1), (4, 1), (5, 2), (16, 2), (17, 3), (65536, 8), (65537, 9), (2 ** 31 - 1, 16)):
        assert C.feistel_half_bits(n) == half


@pytest.mark.parametrize("n", [k for k in PERM_SIZES if k >= 16])
def test_epoch_and_seed_change_the_order(n):
    base = C.perm(np.arange(n), n, 0, 0)
    assert not np.array_equal(base, C.perm(np.arange(n), n, 0, 1))
    assert not np.array_equal(base, C.perm(np.arange(n), n, 1, 0))
    assert np.array_equal(base, C.perm(np.arange(n), n, 0, 0))
    # only the low word of the epoch enters the counter
    assert np.array_equal(C.perm(np.arange(n), n, 0, 5), C.perm(np.arange(n), n, 0, 2 ** 32 + 5))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [17, 1000, 4097])
def test_shards_are_disjoint_equal_and_cover_the_permutation(n, world):
    m = C.samples_per_rank(n, world)
    shards = [C.indices(n, "none", 3, 1, r, world, 0, m) for r in range(world)]
    assert all(len(s) == m for s in shards)
    union = np.concatenate(shards)
    assert len(np.unique(union)) == m * world
    full = C.perm(np.arange(n), n, 3, 1)
    dropped = np.setdiff1d(full, union)
    assert len(dropped) == n - m * world <= world - 1
    assert np.array_equal(np.sort(dropped), np.sort(full[m * world:]))      # the tail of the epoch order is what is dropped
    # shuffle off: the ranks interleave the clips in order
    assert np.array_equal(C.indices(n, "none", 3, 1, world - 1, world, 0, m, shuffle=False), world - 1 + world * np.arange(m))


def test_len_arithmetic():
    assert C.batches_per_epoch(1000, 1, 64, False) == 16 and C.batches_per_epoch(1000, 1, 64, True) == 15
    assert C.batches_per_epoch(1000, 3, 64, False) == 6 and C.batches_per_epoch(1000, 3, 64, True) == 5      # 333 per rank
    assert C.batches_per_epoch(128, 2, 64, False) == 1 and C.batches_per_epoch(128, 2, 64, True) == 1
    assert C.batches_per_epoch(5, 8, 4, False) == 0
    from wakeword_trainer_home_amd.data import ShardedEpochSampler
    for n, world in ((1000, 1), (1000, 3), (17, 8), (5, 8)):
        assert len(ShardedEpochSampler(n, 0, 0, world)) == C.samples_per_rank(n, world)


def test_zero_weight_clips_are_never_drawn():
    w = C.zero_run_weights()
    cdf = C.cdf_table(w)
    assert len(cdf) == len(w) - 4                      # cut after the last non-zero weight
    for epoch in (0, 1):
        idx = C.table_draw(C.positions(0, 1, 0, 20000), cdf, 0, epoch)
        assert (w[idx] > 0).all()
        assert set(np.unique(idx)) == set(np.flatnonzero(w > 0))       # and every other clip is
    # a target that rounds up to the total lands on the last clip WITH weight
    assert np.minimum(np.searchsorted(cdf, cdf[-1], side="right"), len(cdf) - 1) == len(w) - 5


def test_weighted_draw_of_a_single_clip():
    cdf = C.cdf_table(np.array([0.25]))
    assert (C.table_draw(C.positions(0, 1, 0, 100), cdf, 0, 0) == 0).all()
    assert (C.indices(1, "balanced", 0, 0, 1, 2, 5, 100, cdf=cdf) == 0).all()


def _labels_10pct(n=5000):
    y = np.zeros(n, dtype=np.int64)
    y[::10] = 1
    return y


def test_balanced_draws_half_positives():
    y = _labels_10pct()
    cdf = C.cdf_table(C.sampler_weights(y, None, "balanced"))
    idx = C.table_draw(C.positions(0, 1, 0, 20000), cdf, 0, 0)
    share = y[idx].mean()
    assert abs(share - 0.5) <= 0.02, share


def test_hard_negative_weight_triples_the_share():
    y = _labels_10pct()
    hn = np.zeros(len(y), dtype=bool)
    hn[1::50] = True                                   # 100 of the 4500 negatives
    g = C.positions(0, 1, 0, 20000)
    base = C.table_draw(g, C.cdf_table(C.sampler_weights(y, hn, "balanced")), 0, 0)
    hard = C.table_draw(g, C.cdf_table(C.sampler_weights(y, hn, "weighted", 3.0)), 0, 0)
    assert abs(hn[hard].mean() - 3.0 * hn[base].mean()) <= 0.02, (hn[hard].mean(), hn[base].mean())
    # the shares the weights themselves promise: 1/90 of the mass before, 3/(3 + 44 + 45) after
    for idx, w in ((base, C.sampler_weights(y, hn, "balanced")), (hard, C.sampler_weights(y, hn, "weighted", 3.0))):
        assert abs(hn[idx].mean() - w[hn].sum() / w.sum()) <= 0.02
    assert hn[hard].mean() > 2.0 * hn[base].mean() > 0
    # "balanced" ignores the flags, and a weight of 1 changes nothing
    assert np.array_equal(C.sampler_weights(y, hn, "balanced"), C.sampler_weights(y, None, "balanced"))
    assert np.array_equal(C.sampler_weights(y, hn, "weighted", 1.0), C.sampler_weights(y, None, "balanced"))


def test_crop_offsets_stay_inside_the_clip():
    g = C.positions(1, 3, 0, 4000)
    ln = np.random.default_rng(1).integers(0, 300, 4000)
    off = C.crop_offsets(g, ln, 100, 5, 2, True)
    assert (off >= 0).all() and (off[ln <= 100] == 0).all() and (off + 100 <= np.maximum(ln, 100)).all()
    long = ln > 101
    assert (off[long] % 2 == 0).any() and (off[long] % 2 == 1).any()
    assert (C.crop_offsets(g, ln, 100, 5, 2, False) == 0).all()
    assert (C.crop_offsets(g, np.full(4000, 101), 100, 5, 2, True) <= 1).all()


def test_gather_restatement_pads_and_crops():
    bank = np.arange(1, 3 * 12 + 1, dtype=np.int16).reshape(3, 12)
    out, tg, ci, off = C.batch(bank, [12, 5, 0], [1, 0, 1], 8, "none", 0, 0, 0, 1, 0, 3, shuffle=False, training=False)
    assert np.array_equal(ci, [0, 1, 2]) and np.array_equal(tg, [1, 0, 1]) and (off == 0).all()
    assert np.array_equal(out[0], bank[0, :8]) and np.array_equal(out[1], list(bank[1, :5]) + [0, 0, 0]) and not out[2].any()


# ---------------------------------------------------------------------------------------------- the package's host side
def test_sampler_equals_the_restatement():
    from wakeword_trainer_home_amd.data import ShardedEpochSampler, sampler_weights
    for n in (1, 2, 5, 17, 1000, 65537):
        for world in (1, 2, 3):
            for rank in range(world):
                for epoch in (0, 1, 2 ** 31 + 5):
                    s = ShardedEpochSampler(n, seed=9, rank=rank, world=world)
                    s.set_epoch(epoch)
                    ref = C.indices(n, "none", 9, epoch, rank, world, 0, n // world)
                    assert np.array_equal(s.indices(), ref)
                    assert list(s) == ref.tolist() and len(s) == len(ref)
    s = ShardedEpochSampler(1000, seed=9, rank=1, world=3, shuffle=False)
    assert np.array_equal(s.indices(4), 1 + 3 * np.arange(333))
    w = C.zero_run_weights(1000)
    y = (np.arange(1000) % 10 == 0).astype(np.int64)
    assert np.array_equal(sampler_weights(y, None, "balanced"), C.sampler_weights(y, None, "balanced"))
    hn = np.arange(1000) % 7 == 1
    assert np.array_equal(sampler_weights(y, hn, "weighted", 2.5), C.sampler_weights(y, hn, "weighted", 2.5))
    assert np.array_equal(sampler_weights(torch.from_numpy(y), torch.from_numpy(hn), "weighted", 2.5),
                          C.sampler_weights(y, hn, "weighted", 2.5))
    assert np.array_equal(sampler_weights(y, hn, "none"), np.ones(1000))
    for strategy in ("balanced", "weighted"):
        s = ShardedEpochSampler(1000, seed=2, rank=2, world=3, strategy=strategy, weights=w)
        assert np.array_equal(s.cdf_host, C.cdf_table(w))
        assert np.array_equal(s.indices(7), C.indices(1000, strategy, 2, 7, 2, 3, 0, 333, cdf=C.cdf_table(w)))
        assert np.array_equal(s.indices(7, k0=300, count=20), s.indices(7)[300:320])


def test_sampler_feeds_a_host_dataloader():
    from wakeword_trainer_home_amd.data import ShardedEpochSampler
    data = torch.arange(100)
    s = ShardedEpochSampler(100, seed=1, rank=1, world=2)
    dl = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data), batch_size=16, sampler=s)
    for epoch in (0, 1):
        s.set_epoch(epoch)
        got = torch.cat([b[0] for b in dl]).numpy()
        assert np.array_equal(got, C.indices(100, "none", 1, epoch, 1, 2, 0, 50))


def test_error_messages_and_conventions():
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.data import DeviceClipBank, ShardedEpochSampler, sampler_weights
    from wakeword_trainer_home_amd.data.loader import cumulative_table
    assert nat.ABI_VERSION == 17
    assert "ww_loader_batch" in nat.EXPORTS and "ww_loader_indices" in nat.EXPORTS
    for call in (lambda: sampler_weights([0, 1], None, "uniform"), lambda: ShardedEpochSampler(4, strategy="uniform")):
        with pytest.raises(ValueError) as e:
            call()
        assert all(name in str(e.value) for name in ("weighted", "balanced", "none")) and "uniform" in str(e.value)
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        DeviceClipBank(torch.zeros(2, 8, dtype=torch.int16), [0, 1], device="cpu")
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        DeviceClipBank.synthetic(2, 8, device="cpu")
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        ShardedEpochSampler(4).device_indices("cpu")
    with pytest.raises(ValueError, match="needs per-clip weights"):
        ShardedEpochSampler(4, strategy="balanced")
    with pytest.raises(ValueError, match="positive sum"):
        cumulative_table(np.zeros(4))
    with pytest.raises(ValueError, match="rank"):
        ShardedEpochSampler(4, rank=2, world=2)
    with pytest.raises(ValueError, match="outside an epoch"):
        ShardedEpochSampler(10, rank=0, world=2).indices(0, k0=0, count=6)
