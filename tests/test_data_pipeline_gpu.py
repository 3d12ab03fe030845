"""GPU: ww_loader_indices / ww_loader_batch and the loader built on them, bit for bit against the NumPy restatement of the laws
(tests/data_pipeline_cases.py, itself checked in tests/test_data_pipeline_host.py)."""
import numpy as np
import pytest
import torch

from tests import data_pipeline_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _weights(n):
    """Zero-weight runs at the start, in the middle and at the end wherever the table is long enough to have them."""
    return C.zero_run_weights(n, seed=n) if n >= 16 else np.arange(1, n + 1, dtype=np.float64)


@pytest.mark.parametrize("strategy", ["none", "balanced", "weighted"])
@pytest.mark.parametrize("n", [1, 2, 5, 17, 1000, 65537])
def test_indices_match_the_restatement(n, strategy):
    from wakeword_trainer_home_amd.data import ShardedEpochSampler
    w = None if strategy == "none" else _weights(n)
    cdf = None if w is None else C.cdf_table(w)
    launches = 0
    for world in (1, 2, 3):
        for rank in range(world):
            s = ShardedEpochSampler(n, seed=11, rank=rank, world=world, strategy=strategy, weights=w)
            m = len(s)
            assert m == n // world
            for epoch in (0, 1, 2 ** 31 + 5):
                ref = C.indices(n, strategy, 11, epoch, rank, world, 0, m, cdf=cdf)
                s.set_epoch(epoch)
                assert np.array_equal(s.device_indices(DEV).cpu().numpy(), ref), (world, rank, epoch)
                if w is not None and m:
                    assert (w[ref] > 0).all()
                for B in (1, 7, 64):
                    nb = -(-m // B)
                    for i in sorted({0, nb // 2, nb - 1} & set(range(nb))):      # first, middle and (ragged) last batch
                        k0, cnt = i * B, min(B, m - i * B)
                        got = s.device_indices(DEV, epoch, k0, cnt).cpu().numpy()
                        assert got.dtype == np.int32 and np.array_equal(got, ref[k0:k0 + cnt]), (world, rank, epoch, B, i)
                        launches += 1
    assert launches > 0
    if strategy == "none":
        s = ShardedEpochSampler(n, seed=11, rank=0, world=1, shuffle=False)
        assert np.array_equal(s.device_indices(DEV).cpu().numpy(), np.arange(n))
        with pytest.raises(ValueError, match="position"):
            s.device_indices(DEV, 0, n, 1)                                      # one past the epoch


def _bank_case(n_out, L, n_clips=24, seed=0):
    """Clips of every length the copy treats differently, filled with values that tell every sample apart."""
    rng = np.random.default_rng(seed + n_out + L)
    special = [0, 1, n_out - 1, n_out, n_out + 1, L]
    lengths = np.array([min(max(v, 0), L) for v in special] * (n_clips // len(special)), dtype=np.int64)
    bank = rng.integers(-32768, 32767, (n_clips, L), dtype=np.int16)
    bank[bank == 0] = 7                                  # a copied sample is never mistaken for padding
    labels = (np.arange(n_clips) % 3 == 0).astype(np.uint8)
    return bank, lengths, labels


def _run_batch(bank_dev, strategy, seed, epoch, rank, world, k0, B, n_out, training, shuffle=True, cdf_dev=None):
    """ww_loader_batch into rows 1..B of sentinel-filled buffers -> (wave, targets, clip_index) and the guards."""
    from wakeword_trainer_home_amd import _native as nat
    wave = torch.full((B + 2, n_out), SENTINEL, dtype=torch.int16, device=DEV)
    tg = torch.full((B + 2,), SENTINEL, dtype=torch.int64, device=DEV)
    ci = torch.full((B + 2,), SENTINEL, dtype=torch.int32, device=DEV)
    code = nat.SAMPLER_PERM if strategy == "none" else nat.SAMPLER_TABLE
    nat.loader_batch(bank_dev.wave, bank_dev.lengths, bank_dev.labels, code, shuffle, training, cdf_dev, seed, epoch, rank, world,
                     k0, wave[1:B + 1], tg[1:B + 1], ci[1:B + 1])
    wave, tg, ci = wave.cpu().numpy(), tg.cpu().numpy(), ci.cpu().numpy()
    for guard in (wave[0], wave[-1], tg[[0, -1]], ci[[0, -1]]):
        assert (guard == SENTINEL).all(), "the launch wrote outside its rows"
    return wave[1:-1], tg[1:-1], ci[1:-1]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("rel", ["equal", "below", "above"])
@pytest.mark.parametrize("n_out", [8, 250, 4001, 24000])
def test_gather_matches_the_restatement(n_out, rel, training):
    from wakeword_trainer_home_amd.data import DeviceClipBank
    L = {"equal": n_out, "below": n_out - 3, "above": n_out + 37}[rel]
    bank, lengths, labels = _bank_case(n_out, L)
    dev_bank = DeviceClipBank(torch.from_numpy(bank), torch.from_numpy(labels), torch.from_numpy(lengths), device=DEV)
    n = len(bank)
    w = C.zero_run_weights(n, seed=3)
    cdf = C.cdf_table(w)
    cdf_dev = torch.from_numpy(cdf).to(DEV)
    seen_off = []
    # a whole epoch in one batch (odd row count: every second destination row is 2-byte aligned only when n_out is odd);
    # a rank's ragged second batch; draws with replacement
    for strategy, rank, world, k0, B in (("none", 0, 1, 0, n), ("none", 1, 2, 7, 5), ("weighted", 2, 3, 64, 9)):
        for epoch in (0, 3):
            table = cdf if strategy != "none" else None
            ref_w, ref_t, ref_i, off = C.batch(bank, lengths, labels, n_out, strategy, 5, epoch, rank, world, k0, B, cdf=table,
                                               training=training)
            got_w, got_t, got_i = _run_batch(dev_bank, strategy, 5, epoch, rank, world, k0, B, n_out, training,
                                             cdf_dev=cdf_dev if table is not None else None)
            assert np.array_equal(got_i, ref_i) and np.array_equal(got_t, ref_t)
            bad = np.argwhere(got_w != ref_w)
            assert bad.size == 0, f"first mismatch (row, sample) {bad[0]} of {len(bad)}; clip {ref_i[bad[0][0]]} off {off[bad[0][0]]}"
            seen_off.append(off)
    seen_off = np.concatenate(seen_off)
    if rel == "above" and training:
        assert ((seen_off % 2 == 1)).any() and ((seen_off > 0) & (seen_off % 2 == 0)).any(), "no odd and even crop offset drawn"
    else:
        assert (seen_off == 0).all()


def test_offsets_beyond_2_to_31():
    """54 000 x 40 000 int16 = 4.3 GB: patterns on the first row, the last row and the rows around element 2^31 only."""
    from wakeword_trainer_home_amd.data import DeviceClipBank
    n, L, n_out, B = 54000, 40000, 24000, 64
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < 6 * 2 ** 30:
        pytest.skip("less than 6 GB of device memory free")
    mid = 2 ** 31 // L                                   # the row that holds element 2^31
    assert mid * L < 2 ** 31 < (mid + 1) * L
    rows = [0, mid - 1, mid, mid + 1, n - 1]
    wave = torch.empty((n, L), dtype=torch.int16, device=DEV)
    pattern = np.random.default_rng(31).integers(-32768, 32767, (len(rows), L), dtype=np.int16)
    for r, p in zip(rows, pattern):
        wave[r] = torch.from_numpy(p).to(DEV)
    labels = torch.zeros(n, dtype=torch.uint8)
    labels[rows] = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8)
    bank = DeviceClipBank(wave, labels, device=DEV)
    w = np.zeros(n)
    w[rows] = [1.0, 2.0, 3.0, 2.0, 1.0]
    cdf = C.cdf_table(w)
    got_w, got_t, got_i = _run_batch(bank, "weighted", 1, 0, 0, 1, 0, B, n_out, True, cdf_dev=torch.from_numpy(cdf).to(DEV))
    idx = C.indices(n, "weighted", 1, 0, 0, 1, 0, B, cdf=cdf)
    assert set(idx) == set(rows), "64 draws over five rows miss one: change the seed"
    off = C.crop_offsets(C.positions(0, 1, 0, B), np.full(B, L), n_out, 1, 0, True)
    assert np.array_equal(got_i, idx) and np.array_equal(got_t, labels.numpy()[idx])
    for b in range(B):
        assert np.array_equal(got_w[b], pattern[rows.index(idx[b]), off[b]:off[b] + n_out]), (b, idx[b], off[b])
    del bank, wave
    torch.cuda.empty_cache()


def _small_loader(**kw):
    from wakeword_trainer_home_amd.data import DeviceBatchLoader, DeviceClipBank
    bank, lengths, labels = _bank_case(250, 287, n_clips=48)
    dev_bank = DeviceClipBank(torch.from_numpy(bank), torch.from_numpy(labels), torch.from_numpy(lengths), device=DEV)
    return (bank, lengths, labels), DeviceBatchLoader(dev_bank, n_out=250, **kw)


def test_three_batches_held_at_once_stay_correct():
    (bank, lengths, labels), loader = _small_loader(batch_size=7, seed=4)
    loader.set_epoch(2)
    assert len(loader) == 7
    held = []
    for batch in loader:
        held.append(batch)
        if len(held) < 3:
            continue
        torch.cuda.synchronize()
        first = len(held) - 3
        for j, (wv, tg, meta) in enumerate(held[-3:]):
            k0 = (first + j) * 7
            ref_w, ref_t, ref_i, _ = C.batch(bank, lengths, labels, 250, "none", 4, 2, 0, 1, k0, min(7, 48 - k0))
            assert wv.dtype == torch.int16 and tg.dtype == torch.int64 and meta["clip_index"].dtype == torch.int32
            assert wv.is_cuda and tg.is_cuda and meta["clip_index"].is_cuda
            assert np.array_equal(wv.cpu().numpy(), ref_w) and np.array_equal(tg.cpu().numpy(), ref_t)
            assert np.array_equal(meta["clip_index"].cpu().numpy(), ref_i)
    assert len(held) == 7 and held[-1][0].shape == (6, 250)                 # 48 = 6 * 7 + 6: the ragged last batch
    assert loader.RING >= 4                                                 # the Trainer holds three and one is being written
    (_, _, _), dropping = _small_loader(batch_size=7, seed=4, drop_last=True)
    assert len(dropping) == 6 and sum(1 for _ in dropping) == 6


def test_two_ranks_in_one_process_split_the_permutation():
    _, a = _small_loader(batch_size=5, seed=8, rank=0, world=2)
    _, b = _small_loader(batch_size=5, seed=8, rank=1, world=2)
    for epoch in (0, 1):
        streams = []
        for loader in (a, b):
            loader.set_epoch(epoch)
            streams.append(torch.cat([meta["clip_index"].clone() for _, _, meta in loader]).cpu().numpy())
        assert len(streams[0]) == len(streams[1]) == 24
        assert not set(streams[0]) & set(streams[1])
        assert np.array_equal(np.sort(np.concatenate(streams)), np.arange(48))
        full = C.perm(np.arange(48), 48, 8, epoch)
        assert np.array_equal(streams[0], full[0::2]) and np.array_equal(streams[1], full[1::2])


def test_evaluation_order_is_the_bank_order_with_offset_zero():
    (bank, lengths, labels), loader = _small_loader(batch_size=16, shuffle=False, training=False)
    rows = torch.cat([w.clone() for w, _, _ in loader]).cpu().numpy()
    loader.set_epoch(5)                                                      # no epoch dependence without shuffle
    idx = torch.cat([meta["clip_index"].clone() for _, _, meta in loader]).cpu().numpy()
    assert np.array_equal(idx, np.arange(48))
    for i in range(48):
        m = min(lengths[i], 250)
        assert np.array_equal(rows[i, :m], bank[i, :m]) and not rows[i, m:].any()


def test_loader_from_config_and_float_banks():
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.data import DeviceBatchLoader, DeviceClipBank, make_synthetic_batch
    cfg = get_preset("large_dataset")
    x, y = make_synthetic_batch(6, 400, seed=2)
    bank = DeviceClipBank(x, y, hard_negative=[0, 1, 0, 0, 1, 0], device=DEV)
    assert np.array_equal(bank.wave.cpu().numpy(), make_synthetic_batch(6, 400, seed=2, dtype=torch.int16)[0].numpy())
    loader = DeviceBatchLoader.from_config(bank, cfg, rank=1, world=2)
    assert loader.batch_size == 128 and loader.n_out == 40000 and loader.sampler.strategy == "weighted"
    assert loader.sampler.seed == cfg.augmentation.seed and (loader.sampler.rank, loader.sampler.world) == (1, 2)
    from wakeword_trainer_home_amd.data import sampler_weights
    w = sampler_weights(y.numpy(), np.array([0, 1, 0, 0, 1, 0]), "weighted", cfg.loss.hard_negative_weight)
    assert np.array_equal(loader.sampler.cdf_host, C.cdf_table(w))
    (wv, tg, meta), = list(loader)
    assert wv.shape == (3, 40000) and not wv[:, 400:].any()
    syn = DeviceClipBank.synthetic(5, 300, seed=3, device=DEV)
    assert syn.wave.shape == (5, 300) and syn.wave.dtype == torch.int16 and syn.labels.dtype == torch.uint8


class _Rec:
    def __init__(self, swap=None):
        self.loss, self.swap = [], swap

    def on_epoch_start(self, epoch):
        if self.swap is not None:
            self.swap(epoch)

    def on_batch_end(self, batch_idx, loss, acc):
        self.loss.append(loss)


def test_trainer_runs_epochs_from_the_device_loader(tmp_path):
    """Trainer.train() over a DeviceBatchLoader: set_epoch(0), set_epoch(1), six steps, and the per-step losses of a Trainer
    fed the same six batches as plain Python lists.

    Run-to-run spread of the list-fed Trainer over one list (same code path as before this loader existed), fp32 mode, B=8,
    1.5 s clips, six steps: 0.0 -- two runs are bit-equal, so equality is required here."""
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.data import DeviceBatchLoader, DeviceClipBank
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer

    class Recording(DeviceBatchLoader):
        seen = None

        def set_epoch(self, epoch):
            self.seen = (self.seen or []) + [epoch]
            super().set_epoch(epoch)

    def config():
        cfg = get_preset("cnn_small_logmel40")
        cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = 2, 0, 8
        cfg.optimizer.mixed_precision = False
        return cfg

    bank = DeviceClipBank.synthetic(27, 24000, seed=6, pos_rate=0.4, device=DEV)
    kw = dict(batch_size=8, n_out=24000, seed=13, drop_last=True)
    # the six batches, copied out of a loader of their own
    source, lists = DeviceBatchLoader(bank, **kw), []
    for epoch in (0, 1):
        source.set_epoch(epoch)
        lists.append([(w.clone(), t.clone(), {"clip_index": m["clip_index"].clone()}) for w, t, m in source])
    assert [len(x) for x in lists] == [3, 3]
    assert not torch.equal(lists[0][0][0], lists[1][0][0])                  # the second epoch has its own order
    val = lists[0][:1]

    torch.manual_seed(5)
    init = {k: v.clone() for k, v in create_model("cnn_small", dropout=0.0).state_dict().items()}
    results = []
    for mode in ("loader", "lists"):
        model = create_model("cnn_small", dropout=0.0)
        model.load_state_dict(init)
        loader = Recording(bank, **kw) if mode == "loader" else lists[0]
        t = Trainer(model, loader, val, config(), checkpoint_dir=tmp_path / mode, device=DEV)
        assert t.native and t._native_loss
        rec = _Rec(swap=None if mode == "loader" else lambda epoch, t=t: setattr(t, "train_loader", lists[epoch]))
        t.add_callback(rec)
        t.train()
        assert t.state.global_step == 6 and len(rec.loss) == 6 and np.isfinite(rec.loss).all()
        results.append(rec.loss)
        if mode == "loader":
            assert loader.seen == [0, 1]
    print("per-step losses, loader:", results[0], "lists:", results[1])
    assert results[0] == results[1]
