"""Device-resident clip bank and rank-sharded batch loader (DESIGN.md §4 "Loader").

The reference feeds its trainer from a host ``DataLoader`` over ``WakewordDataset`` (``src/data``, absent from the snapshot).
Here the clips live in HBM as int16 -- the ``large_dataset`` preset's 1 M clips of 2.5 s are 80 GB -- and ONE launch per batch
(``ww_loader_batch``) draws the clip of every sample, copies it with crop or zero-pad and writes targets and clip indices: no
host worker, no H2D copy and no index tensor built in Python stands between two training steps.  The sampling laws are stateless
functions of (seed, epoch, rank, world, position), so every rank computes its own shard without talking to the others, and
``ShardedEpochSampler`` hands the same order to an ordinary host ``DataLoader``.
"""
import numpy as np
import torch
from torch.utils.data import Sampler

from .. import _native as nat

STRATEGIES = ("weighted", "balanced", "none")


def _check_strategy(strategy):
    if strategy not in STRATEGIES:
        raise ValueError(f"Unknown sampler_strategy: {strategy!r}. Valid strategies: {', '.join(STRATEGIES)}")
    return strategy


def _need_cuda(device):
    if torch.device(device).type != "cuda":
        raise nat.NativeError(f"the clip bank and its loader live on an MI355X ('cuda') device, got {device!r}: there is no CPU "
                              "fallback for the HIP hot path")


def sampler_weights(labels, hard_negative=None, strategy="weighted", hard_negative_weight=1.0) -> np.ndarray:
    """float64 weight per clip.  "balanced": 1 / count[label], so every class present gets the same total mass; "weighted": the
    same, times ``hard_negative_weight`` on the clips flagged in ``hard_negative``; "none": ones."""
    _check_strategy(strategy)
    labels = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).astype(np.int64)
    if labels.ndim != 1 or labels.size == 0 or labels.min() < 0:
        raise ValueError("labels must be a non-empty 1-D array of non-negative class ids")
    if strategy == "none":
        return np.ones(labels.shape, dtype=np.float64)
    w = 1.0 / np.bincount(labels)[labels].astype(np.float64)
    if strategy == "weighted" and hard_negative is not None:
        hn = np.asarray(hard_negative.cpu() if isinstance(hard_negative, torch.Tensor) else hard_negative).astype(bool)
        if hn.shape != labels.shape:
            raise ValueError("hard_negative must have one flag per clip")
        w = w * np.where(hn, np.float64(hard_negative_weight), np.float64(1.0))
    return w


def cumulative_table(weights) -> np.ndarray:
    """The table both the device and the restatement search: ``np.cumsum`` in float64, built ONCE on the host and cut after the
    last non-zero weight (the clamp of the draw then never lands on a zero-weight clip)."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.size == 0 or not np.isfinite(w).all() or (w < 0).any() or not (w > 0).any():
        raise ValueError("sampler weights must be a non-empty 1-D array of finite, non-negative numbers with a positive sum")
    return np.cumsum(w[:int(np.flatnonzero(w > 0)[-1]) + 1])


class DeviceClipBank:
    """``n_clips`` clips of up to ``L`` samples as int16 ``(n_clips, L)`` on the device, with per-clip length, label and
    hard-negative flag.  Float waveforms are rounded by the rule of ``make_synthetic_batch`` (``x * 32767``, round half to even)."""

    def __init__(self, wave, labels, lengths=None, hard_negative=None, device="cuda"):
        _need_cuda(device)
        wave = torch.as_tensor(wave)
        if wave.dim() != 2 or wave.shape[0] < 1 or wave.shape[1] < 1:
            raise ValueError(f"wave must be (n_clips, L), got {tuple(wave.shape)}")
        if wave.shape[0] >= 2 ** 31 or wave.shape[1] >= 2 ** 31:
            raise ValueError("the bank holds at most 2^31-1 clips of 2^31-1 samples")
        if wave.dtype != torch.int16:
            if not wave.dtype.is_floating_point:
                raise ValueError(f"wave must be int16 or floating point, got {wave.dtype}")
            wave = (wave.to(device).float() * 32767.0).round().clamp_(-32768.0, 32767.0).to(torch.int16)
        self.wave = wave.to(device).contiguous()
        n, L = self.wave.shape
        labels = torch.as_tensor(labels).reshape(-1)
        if labels.numel() != n or (n and (int(labels.min()) < 0 or int(labels.max()) > 255)):
            raise ValueError("labels must hold one class id in [0, 255] per clip")
        self.labels = labels.to(device=device, dtype=torch.uint8).contiguous()
        if lengths is None:
            self.lengths = torch.full((n,), L, dtype=torch.int32, device=device)
        else:
            lengths = torch.as_tensor(lengths).reshape(-1)
            if lengths.numel() != n or int(lengths.min()) < 0 or int(lengths.max()) > L:
                raise ValueError(f"lengths must hold one value in [0, {L}] per clip")
            self.lengths = lengths.to(device=device, dtype=torch.int32).contiguous()
        if hard_negative is None:
            self.hard_negative = None
        else:
            hn = torch.as_tensor(hard_negative).reshape(-1)
            if hn.numel() != n:
                raise ValueError("hard_negative must hold one flag per clip")
            self.hard_negative = hn.to(device=device, dtype=torch.bool)
        self.device = self.wave.device

    @classmethod
    def synthetic(cls, n_clips, n_samples=24000, seed=1234, pos_rate=0.1, device="cuda"):
        """The clips of ``make_synthetic_batch`` (N(0, 0.1^2) clipped to [-1, 1], Bernoulli(pos_rate) labels), generated on the
        device in slices so that no float copy of the whole bank ever exists."""
        _need_cuda(device)
        g = torch.Generator(device=device).manual_seed(seed)
        wave = torch.empty((n_clips, n_samples), dtype=torch.int16, device=device)
        rows = max(1, (64 << 20) // max(n_samples, 1))
        for i in range(0, n_clips, rows):
            m = min(rows, n_clips - i)
            x = (torch.randn(m, n_samples, generator=g, device=device) * 0.1).clamp_(-1.0, 1.0)
            wave[i:i + m] = (x * 32767.0).round().to(torch.int16)
        labels = (torch.rand(n_clips, generator=g, device=device) < pos_rate).to(torch.uint8)
        return cls(wave, labels, device=device)

    def __len__(self):
        return self.wave.shape[0]

    @property
    def n_samples(self):
        return self.wave.shape[1]

    def weights(self, strategy, hard_negative_weight=1.0) -> np.ndarray:
        return sampler_weights(self.labels, self.hard_negative, strategy, hard_negative_weight)

    def class_stats(self) -> dict:
        """``{"positive": clips labelled 1, "negative": clips labelled 0}``: the ``dataset_stats`` that
        ``calculate_class_weights`` / ``class_weights_from_config`` take (one host read; call it once, not per step)."""
        counts = torch.bincount(self.labels.long(), minlength=2).cpu()
        return {"positive": int(counts[1]), "negative": int(counts[0])}


_TAGW = 3 << 24          # WW_TAG_DATA in the top byte of ctr[3]
_M32 = np.uint64(0xFFFFFFFF)


def _philox(c0, c1, c2, c3, seed):
    """Philox4x32-10 over arrays of counters, key = the 64-bit seed -> the four output words as uint64 arrays."""
    c = [np.broadcast_to(np.asarray(v, dtype=np.uint64), np.shape(c0)).copy() for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & _M32, p1 & _M32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & _M32, p0 & _M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c


def epoch_permutation(g, n_clips, seed, epoch) -> np.ndarray:
    """perm_epoch at positions ``g`` (all < n_clips), on the host: the law ``ww_loader_batch`` applies on the device."""
    half = 1
    while (1 << (2 * half)) < n_clips:
        half += 1
    half, mask, n = np.uint64(half), np.uint64((1 << half) - 1), np.uint64(n_clips)
    x = np.array(g, dtype=np.uint64)
    walking = np.flatnonzero(np.ones(x.shape, dtype=bool))
    while walking.size:                    # cycle-walk: the values that left [0, n) take another turn
        l, r = x[walking] >> half, x[walking] & mask
        for rnd in range(4):
            l, r = r, l ^ (_philox(r, rnd, epoch & 0xFFFFFFFF, _TAGW, seed)[0] & mask)
        x[walking] = (l << half) | r
        walking = walking[x[walking] >= n]
    return x.astype(np.int64)


def table_draws(g, cdf, seed, epoch) -> np.ndarray:
    """The with-replacement draw at positions ``g`` from the cumulative table, on the host."""
    g = np.asarray(g, dtype=np.uint64)
    x = _philox(g & _M32, g >> np.uint64(32), epoch & 0xFFFFFFFF, _TAGW | 1, seed)
    u53 = ((x[0] << np.uint64(32)) | x[1]) >> np.uint64(11)
    target = u53.astype(np.float64) * np.float64(2.0 ** -53) * np.float64(cdf[-1])
    return np.minimum(np.searchsorted(cdf, target, side="right"), len(cdf) - 1).astype(np.int64)


class ShardedEpochSampler(Sampler):
    """This rank's clip indices of an epoch: ``floor(n_clips / world)`` of them, sample ``k`` at epoch position
    ``g = rank + world * k``.  "none": ``perm_epoch(g)`` (or ``g`` with shuffle off), disjoint between ranks; "balanced" /
    "weighted": drawn with replacement from ``weights``.  ``indices`` evaluates the laws on the host, so as a torch ``Sampler``
    it gives a host ``DataLoader`` the order the device loader draws; ``device_indices`` is the kernel (``ww_loader_indices``)."""

    def __init__(self, n_clips, seed=0, rank=0, world=1, strategy="none", weights=None, shuffle=True):
        _check_strategy(strategy)
        if n_clips < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError(f"need n_clips >= 1 and 0 <= rank < world, got n_clips={n_clips} rank={rank} world={world}")
        self.n_clips, self.seed, self.rank, self.world = int(n_clips), int(seed), int(rank), int(world)
        self.strategy, self.shuffle, self.epoch = strategy, bool(shuffle), 0
        self.cdf_host, self._cdf_dev = None, {}
        if strategy != "none":
            if weights is None:
                raise ValueError(f"sampler_strategy {strategy!r} needs per-clip weights (sampler_weights)")
            if len(weights) != n_clips:
                raise ValueError("weights must hold one value per clip")
            self.cdf_host = cumulative_table(weights)
        self.code = nat.SAMPLER_PERM if strategy == "none" else nat.SAMPLER_TABLE

    def table(self, device):
        """The cumulative table on ``device`` (uploaded once), None for "none"."""
        if self.cdf_host is None:
            return None
        key = str(device)
        if key not in self._cdf_dev:
            self._cdf_dev[key] = torch.from_numpy(self.cdf_host).to(device)
        return self._cdf_dev[key]

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.n_clips // self.world

    def _range(self, k0, count):
        count = len(self) - k0 if count is None else count
        if k0 < 0 or count < 0:
            raise ValueError(f"bad sample range k0={k0} count={count}")
        return int(k0), int(count)

    def indices(self, epoch=None, k0=0, count=None) -> np.ndarray:
        """int64 host array: the clips of samples ``k0 .. k0 + count - 1`` (default: the whole epoch)."""
        k0, count = self._range(k0, count)
        epoch = self.epoch if epoch is None else int(epoch)
        g = np.uint64(self.rank) + np.uint64(self.world) * (np.uint64(k0) + np.arange(count, dtype=np.uint64))
        if self.cdf_host is not None:
            return table_draws(g, self.cdf_host, self.seed, epoch)
        if count and int(g[-1]) >= self.n_clips:
            raise ValueError(f"sample {k0 + count - 1} of rank {self.rank}/{self.world} lies outside an epoch of {self.n_clips}")
        return epoch_permutation(g, self.n_clips, self.seed, epoch) if self.shuffle else g.astype(np.int64)

    def device_indices(self, device, epoch=None, k0=0, count=None) -> torch.Tensor:
        """The same as an int32 tensor computed on ``device`` by ``ww_loader_indices``."""
        _need_cuda(device)
        k0, count = self._range(k0, count)
        if count == 0:
            return torch.empty((0,), dtype=torch.int32, device=device)
        return nat.loader_indices(self.n_clips, self.code, self.shuffle, self.table(device), self.seed,
                                  self.epoch if epoch is None else epoch, self.rank, self.world, k0, count, device=device)

    def __iter__(self):
        return iter(self.indices().tolist())


class DeviceBatchLoader:
    """Iterates ``(int16 (B, n_out) cuda, int64 (B,) cuda, {"clip_index": int32 (B,) cuda, "ready": Event})`` over this rank's
    shard of an epoch -- the ``(inputs, targets, metadata)`` contract the Trainer unpacks -- with one kernel launch per batch on
    the current stream.

    The outputs are views of a ring of ``RING`` buffer sets: a batch stays valid until ``RING`` further batches have been
    requested.  The Trainer holds three (running, staged, fetched), so four never hands out a buffer that is still in flight.
    ``metadata["ready"]`` is recorded behind the launch; a consumer that reads the batch on another stream waits for it (the
    Trainer's input stage does)."""

    RING = 4

    def __init__(self, bank, batch_size, n_out, strategy="none", seed=0, rank=0, world=1, hard_negative_weight=1.0, shuffle=True,
                 drop_last=False, training=True):
        if not isinstance(bank, DeviceClipBank):
            raise TypeError("bank must be a DeviceClipBank")
        if batch_size < 1 or n_out < 1:
            raise ValueError(f"batch_size and n_out must be positive, got {batch_size} and {n_out}")
        self.bank, self.batch_size, self.n_out = bank, int(batch_size), int(n_out)
        self.drop_last, self.training = bool(drop_last), bool(training)
        weights = None if strategy == "none" else bank.weights(_check_strategy(strategy), hard_negative_weight)
        self.sampler = ShardedEpochSampler(len(bank), seed, rank, world, strategy, weights, shuffle)
        self._ring = None
        self._slot = 0

    @classmethod
    def from_config(cls, bank, config, rank=0, world=1, **kw):
        """``training.batch_size``, ``data.sample_rate x audio_duration``, ``loss.sampler_strategy``, ``loss.hard_negative_weight``
        and ``augmentation.seed`` of a WakewordConfig."""
        return cls(bank, config.training.batch_size, int(config.data.sample_rate * config.data.audio_duration),
                   strategy=config.loss.sampler_strategy, seed=config.augmentation.seed, rank=rank, world=world,
                   hard_negative_weight=config.loss.hard_negative_weight, **kw)

    def set_epoch(self, epoch):
        self.sampler.set_epoch(epoch)

    @property
    def epoch(self):
        return self.sampler.epoch

    def __len__(self):
        m = len(self.sampler)
        return m // self.batch_size if self.drop_last else -(-m // self.batch_size)

    def _buffers(self):
        if self._ring is None:
            dev, B = self.bank.device, self.batch_size
            self._ring = [(torch.empty((B, self.n_out), dtype=torch.int16, device=dev),
                           torch.empty((B,), dtype=torch.int64, device=dev),
                           torch.empty((B,), dtype=torch.int32, device=dev), torch.cuda.Event()) for _ in range(self.RING)]
        slot = self._ring[self._slot]
        self._slot = (self._slot + 1) % self.RING
        return slot

    def __iter__(self):
        s, epoch, m = self.sampler, self.sampler.epoch, len(self.sampler)
        for i in range(len(self)):
            k0 = i * self.batch_size
            B = min(self.batch_size, m - k0)
            wave, targets, clip_index, ready = self._buffers()
            wave, targets, clip_index = wave[:B], targets[:B], clip_index[:B]
            nat.loader_batch(self.bank.wave, self.bank.lengths, self.bank.labels, s.code, s.shuffle, self.training, s.table(self.bank.device),
                             s.seed, epoch, s.rank, s.world, k0, wave, targets, clip_index)
            ready.record()
            yield wave, targets, {"clip_index": clip_index, "ready": ready}
