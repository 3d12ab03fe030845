from .feature_extraction import FeatureExtractor
from .augmentation import AudioAugmentation, SpecAugment
from .dataset import SyntheticClipDataset, make_synthetic_batch
from .loader import DeviceBatchLoader, DeviceClipBank, ShardedEpochSampler, sampler_weights

__all__ = ["FeatureExtractor", "SpecAugment", "SyntheticClipDataset", "make_synthetic_batch", "DeviceClipBank",
           "DeviceBatchLoader", "ShardedEpochSampler", "sampler_weights"]
